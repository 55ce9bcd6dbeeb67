#!/usr/bin/env python3
"""Golden for pose_resnet_psa (NUM_LAYERS 18, gaussian, 256x192): CPU forward (the module in fp64) + UDP decode of one
synthetic crop, produced by the REFERENCE's own module files (PSA.py, pose_resnet_psa.py) and get_final_preds.  Build
container only (it needs the reference checkout); the fixture holds data only, no weights: they are re-drawn from the
seed (udp_pose_amd.synth_resnet.synth_pose_resnet_psa_state_dict) and the stored calibration statistics.

    python tools/gen_golden_resnet_psa.py   # writes tests/golden/resnet18_psa.npz

Before writing, it checks that the fixture can carry the GPU test: the fp32 and fp64 restatements
(tests/resnet_psa_ref.py) agree with the reference on every joint's arg-max, and more than half the joints have a
DARK Taylor step below 1.5 px (the conditioning filter of the keypoint comparison).  Otherwise pick another seed.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg                                                      # noqa: E402  (reference loader helpers)
from udp_pose_amd import synth                                                # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_psa_state_dict        # noqa: E402

EXTRA = {"FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
         "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 18}
LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
SEED = 7


def load_reference_module():
    """The reference's lib/models/__init__.py imports torchvision: the two module files are loaded one by one."""
    gg.load_reference()
    models = os.path.join(gg.REF, "lib", "models")
    gg._load("refmodels.PSA", os.path.join(models, "PSA.py"), "refmodels")
    return gg._load("refmodels.pose_resnet_psa", os.path.join(models, "pose_resnet_psa.py"), "refmodels")


def reference_net(ref, num_layers):
    return ref.get_pose_net(gg.model_cfg(dict(EXTRA, NUM_LAYERS=num_layers), 17, "gaussian"), is_train=False)


def main():
    torch.manual_seed(0)                                                # (the module's own initialisation; overwritten below)
    ref = load_reference_module()
    inference = sys.modules["ref_inference"]
    nets = {}
    for num_layers in (18, 34):                                         # the weight-file contract of both depths
        nets[num_layers] = reference_net(ref, num_layers)
        want = {k: tuple(v.shape) for k, v in nets[num_layers].state_dict().items()}
        got = {k: tuple(v.shape) for k, v in synth_pose_resnet_psa_state_dict(seed=1, layers=LAYERS[num_layers]).items()}
        assert list(got) == list(want) and got == want, "synth key order / shapes != the reference module's at %d" % num_layers
        print("resnet%d-psa" % num_layers, len(want), "keys,", sum(int(np.prod(s)) for s in want.values()), "elements")
    net = nets[18]
    sd = synth_pose_resnet_psa_state_dict(seed=SEED)
    net.load_state_dict(sd, strict=True)
    # BatchNorm running statistics := those of one calibration batch (momentum None = plain average over one step)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = None
            m.reset_running_stats()
    net.train()
    with torch.no_grad():
        net(torch.from_numpy(synth.synth_crops(8, 256, 192, seed=17)))
    net.eval()
    with torch.no_grad():
        yc = net(torch.from_numpy(synth.synth_crops(8, 256, 192, seed=17)))
    scale = 0.25 / float(yc.std())
    calib = {k: v.numpy().copy() for k, v in net.state_dict().items() if "running_" in k}
    sd = synth_pose_resnet_psa_state_dict(seed=SEED, calib=calib, final_scale=scale)
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    # The fixture is the reference module's fp64 forward (rounded to fp32 for storage): the distance of its fp32 forward
    # from that is printed, tests/test_resnet_psa_cpu.py takes its fp32 bound from it.
    with torch.no_grad():
        hm32 = net(x).numpy()
        hm = net.double()(x.double()).numpy()
    print("reference module: max |fp32 - fp64|", float(np.abs(hm32 - hm).max()))
    hm = hm.astype(np.float32)
    c, s = synth.synth_center_scale(1, seed=3)
    cfgd = gg.AttrDict({"MODEL": {"TARGET_TYPE": "gaussian"}, "TEST": {"POST_PROCESS": True}, "LOSS": {"KPD": 4.0}})
    preds, maxvals, pin = inference.get_final_preds(cfgd, hm.copy(), c, s)
    # can the fixture carry the GPU test?  (tests/test_gpu_resnet_psa.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resnet_psa_ref as R                                        # noqa: E402
    from oracle import decode as odec                                 # noqa: E402
    am = hm.reshape(1, 17, -1).argmax(2)
    for dt in (torch.float32, torch.float64):
        y = R.forward(sd, x, dtype=dt).numpy()
        assert np.array_equal(y.reshape(1, 17, -1).argmax(2), am), "arg-max of the %s restatement differs: pick another seed" % dt
        print("restatement", dt, "max |diff| to the reference", float(np.abs(y - hm).max()))
    coords, _, _ = odec.get_max_preds(hm)
    good = np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2) < 1.5
    assert good.mean() > 0.5, "only %d of %d joints are well conditioned: pick another seed" % (good.sum(), good.size)
    print("well-conditioned joints", int(good.sum()), "of", good.size)
    keys = {k: list(v.shape) for k, v in sd.items()}
    out = os.path.join(gg.OUT, "resnet18_psa.npz")
    np.savez_compressed(out, heatmaps=hm, preds=preds, maxvals=maxvals, pin=pin, center=c, scale=s, final_scale=np.float64(scale),
                        keys=np.array(sorted("%s:%s" % (k, "x".join(map(str, v))) for k, v in keys.items())),
                        **{"calib_" + k: v for k, v in calib.items()})
    print("resnet18-psa", hm.shape, "absmax", float(np.abs(hm).max()), "std", float(hm.std()), preds[0, :2],
          os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
