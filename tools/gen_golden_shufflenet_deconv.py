#!/usr/bin/env python3
"""Goldens for the two deconv-head ShuffleNets, pose_shufflenetv2_10x (1.0x) and pose_shufflenetv2_plus (Small), gaussian,
256x192: CPU forward + UDP decode of one synthetic crop, produced by the REFERENCE's own module files and
get_final_preds.  Build container only (it needs the reference checkout); the fixtures hold data only.

    python tools/gen_golden_shufflenet_deconv.py   # writes tests/golden/shufflenetv2_10x_deconv.npz and
                                                   #        tests/golden/shufflenetv2_plus_small_deconv.npz

Before writing, it checks that each fixture can carry the GPU test: the fp32 and fp64 restatements
(tests/deconv_heads_ref.py) agree with the reference on every joint's arg-max, and more than half the joints have a
DARK Taylor step below 1.5 px (the conditioning filter of the keypoint comparison); and, beyond the siblings' guard,
every joint's two highest pixels are more than 2e-3 apart (twice the heat-map gate: seed 7 of the 1.0x net had a joint
with a gap of 2.2e-5, which the fp32 restatement reproduced and the split-fp16 GPU run, 7e-5 off, did not).
Otherwise pick another seed.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg                                               # noqa: E402  (reference loader helpers)
from udp_pose_amd import synth                                         # noqa: E402
from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict  # noqa: E402
from udp_pose_amd.synth_shufflenet_plus import synth_shufflenet_plus_deconv_state_dict  # noqa: E402

HEAD = {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4],
        "FINAL_CONV_KERNEL": 1}
# name -> (backbone file, pose module file, MODEL_SIZE, state-dict generator, seed, fixture)
NETS = {"pose_shufflenetv2_10x": ("shufflenetv2", "pose_shufflenetv2_10x", "1.0x", synth_shufflenet_deconv_state_dict, 8,
                                  "shufflenetv2_10x_deconv.npz"),
        "pose_shufflenetv2_plus": ("shufflenetv2_plus", "pose_shufflenetv2_plus", "Small", synth_shufflenet_plus_deconv_state_dict, 7,
                                   "shufflenetv2_plus_small_deconv.npz")}


def gen(name, inference, seed=None):
    backbone, module, size, synth_sd, seed0, fixture = NETS[name]
    seed = seed0 if seed is None else seed
    models = os.path.join(gg.REF, "lib", "models")
    gg._load("refmodels.backbones." + backbone, os.path.join(models, "backbones/%s.py" % backbone), "refmodels.backbones")
    ref = gg._load("refmodels." + module, os.path.join(models, module + ".py"), "refmodels")
    cfg = gg.model_cfg(dict(HEAD, MODEL_SIZE=size), 17, "gaussian")
    dict.__getitem__(cfg, "MODEL")["IMAGE_SIZE"] = [192, 256]           # the ShuffleNetV2+ backbone asserts multiples of 32 on it
    net = ref.get_pose_net(cfg, is_train=False)
    sd = synth_sd(seed=seed)
    assert list(sd) == list(net.state_dict()), "%s: synth key order != the reference module's" % name
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in net.state_dict().items())
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
    sd = synth_sd(seed=seed, calib=calib, final_scale=scale)
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    with torch.no_grad():
        hm = net(x).numpy()
    c, s = synth.synth_center_scale(1, seed=3)
    cfgd = gg.AttrDict({"MODEL": {"TARGET_TYPE": "gaussian"}, "TEST": {"POST_PROCESS": True}, "LOSS": {"KPD": 4.0}})
    preds, maxvals, pin = inference.get_final_preds(cfgd, hm.copy(), c, s)
    # can the fixture carry the GPU test?  (tests/test_gpu_deconv_heads.py)
    import deconv_heads_ref as R                                      # noqa: E402
    from oracle import decode as odec                                 # noqa: E402
    am = hm.reshape(1, 17, -1).argmax(2)
    for dt in (torch.float32, torch.float64):
        y = R.FORWARD[name](sd, x, dtype=dt).numpy()
        assert np.array_equal(y.reshape(1, 17, -1).argmax(2), am), "arg-max of the %s restatement differs: pick another seed" % dt
        print(name, "restatement", dt, "max |diff| to the reference", float(np.abs(y - hm).max()))
    # a joint whose two highest pixels lie closer than twice the 1e-3 heat-map gate has no arg-max a conforming output
    # must reproduce (the fp32 restatement can agree by luck): every joint needs that margin
    top2 = np.sort(hm.reshape(17, -1), axis=1)[:, -2:]
    gap = float((top2[:, 1] - top2[:, 0]).min())
    print(name, "smallest gap between a joint's two highest pixels", gap)
    assert gap > 2e-3, "a joint's arg-max is a near tie (gap %.3g): pick another seed" % gap
    coords, _, _ = odec.get_max_preds(hm)
    good = np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2) < 1.5
    assert good.mean() > 0.5, "only %d of %d joints are well conditioned: pick another seed" % (good.sum(), good.size)
    print(name, "well-conditioned joints", int(good.sum()), "of", good.size)
    keys = {k: list(v.shape) for k, v in sd.items()}
    out = os.path.join(gg.OUT, fixture)
    np.savez_compressed(out, heatmaps=hm, preds=preds, maxvals=maxvals, pin=pin, center=c, scale=s, final_scale=np.float64(scale),
                        keys=np.array(["%s:%s" % (k, "x".join(map(str, v))) for k, v in keys.items()]),
                        **{"calib_" + k: v for k, v in calib.items()})
    print(name, hm.shape, "absmax", float(np.abs(hm).max()), "std", float(hm.std()), preds[0, :2], os.path.getsize(out), "bytes")


def main():
    gg.load_reference()
    inference = sys.modules["ref_inference"]
    models = os.path.join(gg.REF, "lib", "models")
    pkg = type(sys)("refmodels.backbones")
    pkg.__path__ = [os.path.join(models, "backbones")]
    sys.modules["refmodels.backbones"] = pkg
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for name in NETS:
        gen(name, inference)


if __name__ == "__main__":
    main()
