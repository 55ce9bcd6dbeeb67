"""pose_resnet_psa (ResNet-18 / 34 with polarized self-attention) on the GPU: the whole network against the reference
module's own heat-maps / get_final_preds output (tests/golden/resnet18_psa.npz) and against the fp64 restatement
(tests/resnet_psa_ref.py), and the bit-equalities of the runtime (replay, eager, mirrored half, sub-batch lanes)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_psa_ref as R                                               # noqa: E402
from oracle import decode as odec                                        # noqa: E402
from udp_pose_amd import _lib, synth                                     # noqa: E402
from udp_pose_amd.inference import decode_device                         # noqa: E402
from udp_pose_amd.model import MODELS                                    # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_psa_state_dict   # noqa: E402

EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
         "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 18}


def _cfg(**extra):
    return {"MODEL": {"NAME": "pose_resnet_psa", "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": dict(EXTRA, **extra)}}


def _dark_shift(hm):
    coords, _, _ = odec.get_max_preds(hm)
    return np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2)


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "resnet18_psa.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    return g, synth_pose_resnet_psa_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))


@pytest.fixture(scope="module")
def res18(golden_dir):
    return _fixture(golden_dir)[1]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_res18_psa_matches_reference_fixture(golden_dir, dtype):
    g, sd = _fixture(golden_dir)
    net = MODELS["pose_resnet_psa"](_cfg(), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19)).cuda()
    hm = net(x).clone()
    got = hm.cpu().numpy()
    assert got.shape == (1, 17, 64, 48)
    print("res18-psa %s heat-map error %.3g" % (dtype, float(np.abs(got - g["heatmaps"]).max())))
    assert float(np.abs(got - g["heatmaps"]).max()) <= 1e-3
    np.testing.assert_array_equal(got.reshape(1, 17, -1).argmax(2), g["heatmaps"].reshape(1, 17, -1).argmax(2))
    c, s = np.asarray(g["center"], np.float64), np.asarray(g["scale"], np.float64)
    preds, maxvals, _, idx = decode_device(hm, torch.from_numpy(c), torch.from_numpy(s), "gaussian", True, 4.0, True)
    torch.cuda.synchronize()
    assert float(np.abs(maxvals.cpu().numpy() - g["maxvals"]).max()) <= 1e-3
    preds = preds.cpu().numpy()
    # decode of the device heat-maps == oracle decode of the same maps (well-conditioned joints)
    hp, _, _, hidx = odec.get_final_preds("gaussian", True, 4.0, got.copy(), c, s)
    np.testing.assert_array_equal(idx.cpu().numpy(), hidx)
    hgood = _dark_shift(got) < 1.5
    assert float(np.abs(preds - hp)[hgood].max()) <= 1e-3
    # keypoints vs the reference's get_final_preds: median 1e-3 px, 2e-2 px on the joints whose Taylor step is a
    # genuine sub-pixel refinement (DARK amplifies 1e-5 heat-map noise where the Hessian is near singular)
    err = np.abs(preds - g["preds"]).max(axis=2)
    good = _dark_shift(g["heatmaps"].astype(np.float32)) < 1.5
    print("res18-psa %s keypoint error px: median %.2g, max(well-conditioned %d/%d) %.2g, max(all) %.2g"
          % (dtype, np.median(err), good.sum(), good.size, err[good].max(), err.max()))
    assert good.mean() > 0.5 and err[good].max() < 2e-2 and np.median(err) < 1e-3
    assert len(net.program(256, 192)._ops) == 65


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_res34_psa_128x96_matches_fp64_restatement(dtype):
    """ResNet-34 at 128x96, two images: layer 4 runs the 512-channel attention on a 4x3 map."""
    sd = synth_pose_resnet_psa_state_dict(seed=11, layers=(3, 4, 6, 3))
    x = torch.from_numpy(synth.synth_crops(2, 128, 96, seed=23))
    R.forward(sd, x, calibrate=True)                                      # BatchNorm statistics of this batch
    ref = R.forward(sd, x, dtype=torch.float64).numpy()
    net = MODELS["pose_resnet_psa"](_cfg(NUM_LAYERS=34), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    got = net(x.cuda()).clone().cpu().numpy()
    assert got.shape == (2, 17, 32, 24)
    scale = max(1.0, float(np.abs(ref).max()))
    print("res34-psa %s heat-map error %.3g (scale %.3g)" % (dtype, float(np.abs(got - ref).max()), scale))
    assert float(np.abs(got - ref).max()) <= 1e-3 * scale
    np.testing.assert_array_equal(got.reshape(2, 17, -1).argmax(2), ref.reshape(2, 17, -1).argmax(2))
    prog = net.program(128, 96)
    assert len(prog._ops) == 121
    assert [(op["cin"], op["hin"], op["win"]) for op in prog._ops if op["kind"] == _lib.UDP_OP_PSA_POOL][-1] == (512, 4, 3)


@pytest.mark.parametrize("dtype", ["f16x2", "f32"])
def test_res18_psa_flip_batch16(res18, dtype):
    """N = 16 with the flip test (32 images per launch sequence, so the sub-batch lanes engage): replay == eager, and
    the mirrored half equals an explicit forward of the W-mirrored batch bit for bit (every reduction of the attention
    kernels has an order fixed per image)."""
    net = MODELS["pose_resnet_psa"](_cfg(), is_train=False, dtype=dtype).load_state_dict(res18).to("cuda")
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=33)).repeat(2, 1, 1, 1)
    x[10:] += 0.01 * torch.randn(6, 3, 256, 192, generator=torch.Generator().manual_seed(1))
    xd = x.cuda()
    raw = net.raw_forward(xd, flip_test=True).clone()
    assert raw.shape == (32, 17, 64, 48) and torch.isfinite(raw).all()
    assert torch.equal(raw, net.raw_forward(xd, flip_test=True))           # graph replay
    net.use_graph = False
    assert torch.equal(raw, net.raw_forward(xd, flip_test=True))           # eager launches
    net.use_graph = True
    mirrored = net.raw_forward(torch.flip(xd, dims=[3]).contiguous()).clone()
    assert torch.equal(mirrored, raw[16:])
    assert torch.equal(raw[0], raw[8]) and not torch.equal(raw[2], raw[10])
    one = net.raw_forward(xd[5:6].contiguous()).clone()                    # batch size changes no number
    assert torch.equal(one[0], raw[5])
    ref = R.forward(res18, torch.cat([x[13:14], torch.flip(x[13:14], dims=[3])])).numpy()
    assert float(np.abs(raw[[13, 29]].cpu().numpy() - ref).max()) <= 1e-3


def test_res18_psa_sub_batch_lanes_change_no_number(res18):
    n = 16
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=71)).cuda().repeat(2, 1, 1, 1).contiguous()
    x += 0.01 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    out = {}
    saved = os.environ.get("UDP_POSE_LANES")
    try:
        for lanes in ("1", "2"):
            os.environ["UDP_POSE_LANES"] = lanes
            net = MODELS["pose_resnet_psa"](_cfg(), is_train=False, dtype="f16x2").load_state_dict(res18).to("cuda")
            a = net.raw_forward(x, flip_test=True).clone()
            assert torch.equal(a, net.raw_forward(x, flip_test=True)) and torch.isfinite(a).all()
            assert _lib.lib().udp_hrnet_lanes(net._compiled[(256, 192)][0], C.c_int(n)) == int(lanes)
            out[lanes] = a
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_LANES", None)
        else:
            os.environ["UDP_POSE_LANES"] = saved
    assert torch.equal(out["1"], out["2"])


def test_res18_psa_flops_and_overflow_flag(res18):
    net = MODELS["pose_resnet_psa"](_cfg(), is_train=False, dtype="f16x2").load_state_dict(res18).to("cuda")
    _lib.f16x2_overflow(reset=True)
    net(torch.from_numpy(synth.synth_crops(2, 256, 192, seed=3)).cuda())
    handle, _, prog = net._compiled[(256, 192)]
    assert abs(_lib.lib().udp_hrnet_flops_per_image(handle) - 2 * prog.macs_per_image()) <= 1e-6 * prog.macs_per_image()
    assert _lib.lib().udp_hrnet_num_launches(handle) == 65
    assert not _lib.f16x2_overflow(reset=True)
