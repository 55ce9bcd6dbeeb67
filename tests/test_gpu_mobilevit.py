"""pose_mobilevit_pixel_shuffle on the GPU: the xxs net against the heat-maps / get_final_preds output of the reference's
own module (tests/golden/mobilevit_xxs_ps.npz), the xxs / xs / s nets at 64x64 against the fp64 restatement
(tests/mobilevit_ref.py), and the executor's invariants (replay == eager, one lane == two, exact-zero pad channels)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mobilevit_ref as R
from oracle import decode as odec
from udp_pose_amd import _lib, synth
from udp_pose_amd.inference import decode_device
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilevit import synth_mobilevit_state_dict

pytestmark = pytest.mark.gpu

NAME = "pose_mobilevit_pixel_shuffle"


def _cfg(size="xxs", target="gaussian", **extra):
    return {"MODEL": {"NAME": NAME, "NUM_JOINTS": 17, "TARGET_TYPE": target,
                      "EXTRA": dict({"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": size, "FINAL_CONV_KERNEL": 1},
                                    **extra)}}


def _net(sd, dtype, size="xxs", target="gaussian"):
    return MODELS[NAME](_cfg(size, target), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()


def _dark_shift(hm):
    coords, _, _ = odec.get_max_preds(hm)
    return np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_xxs_matches_reference_fixture(golden_dir, dtype):
    """Measured max |heat-map - fixture|: see NOTES.md (the contract is 1e-3)."""
    g = np.load(os.path.join(golden_dir, "mobilevit_xxs_ps.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_mobilevit_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    net = _net(sd, dtype)
    hm = net(torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19)).cuda()).clone()
    got = hm.cpu().numpy()
    assert got.shape == (1, 17, 64, 48)
    err = float(np.abs(got - g["heatmaps"]).max())
    print("mobilevit xxs %s: max |heat-map - fixture| %.3g, %d launches" % (dtype, err, len(net.program(256, 192)._ops)))
    assert err <= 1e-3
    np.testing.assert_array_equal(got.reshape(1, 17, -1).argmax(2), g["heatmaps"].reshape(1, 17, -1).argmax(2))
    c, s = np.asarray(g["center"], np.float64), np.asarray(g["scale"], np.float64)
    preds, maxvals, _, _ = decode_device(hm, torch.from_numpy(c), torch.from_numpy(s), "gaussian", True, 4.0, True)
    torch.cuda.synchronize()
    assert float(np.abs(maxvals.cpu().numpy() - g["maxvals"]).max()) <= 1e-3
    # keypoints vs the reference's get_final_preds, at the tolerance tests/test_gpu_mobilevitv2.py uses for the same
    # comparison: median 1e-3 px, 2e-2 px on the joints whose Taylor step is a genuine sub-pixel refinement
    kerr = np.abs(preds.cpu().numpy() - g["preds"]).max(axis=2)
    good = _dark_shift(g["heatmaps"].astype(np.float32)) < 1.5
    print("keypoint error px: median %.2g, max(well-conditioned %d/%d) %.2g, max(all) %.2g"
          % (np.median(kerr), good.sum(), good.size, kerr[good].max(), kerr.max()))
    assert good.mean() > 0.5 and kerr[good].max() < 2e-2 and np.median(kerr) < 1e-3
    handle = net._compiled[(256, 192)][0]
    macs = net.program(256, 192).macs_per_image()
    assert abs(_lib.lib().udp_hrnet_flops_per_image(handle) - 2 * macs) <= 1e-6 * macs


HW = (64, 64)
_cache = {}


def _small(size, target="gaussian"):
    """Seeded weights of a small net with BatchNorm statistics calibrated on 256 crops, the crops of the tests (3 of
    them) and their fp64 heat-maps [normal | mirrored]; computed once per size."""
    key = (size, target)
    if key not in _cache:
        h, w = HW
        sd = synth_mobilevit_state_dict(seed=11 + len(size) + h, model_size=size, target_type=target)
        # 256 calibration crops: at H/32 = 2 x 2 pixels a BatchNorm of layer 5 sees 4 samples per crop
        yc = R.forward(sd, torch.from_numpy(synth.synth_crops(256, h, w, seed=5)), calibrate=True)
        k = 0.25 / float(yc.std())
        sd["final_layer.weight"], sd["final_layer.bias"] = sd["final_layer.weight"] * k, sd["final_layer.bias"] * k
        x = torch.from_numpy(synth.synth_crops(3, h, w, seed=9))
        ref = torch.cat([R.forward(sd, x, dtype=torch.float64), R.forward(sd, torch.flip(x, dims=[3]), dtype=torch.float64)])
        _cache[key] = (sd, x, ref.numpy())
    return _cache[key]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", ["xxs", "xs", "s"])
def test_small_nets_match_fp64_restatement(size, n, flip, dtype):
    """xs and s: 48 / 120 / 144 / 240 channels and head widths 30 / 36 / 60 are no multiples of 32 or 8."""
    sd, x, ref = _small(size)
    h, w = HW
    net = _net(sd, dtype, size)
    xd = x[:n].cuda().contiguous()
    raw = net.raw_forward(xd, flip_test=flip).clone()
    want = np.concatenate([ref[:n], ref[3:3 + n]]) if flip else ref[:n]
    assert raw.shape == want.shape == (n * (2 if flip else 1), 17, h // 4, w // 4)
    err = float(np.abs(raw.cpu().numpy() - want).max())
    scale = max(1.0, float(np.abs(want).max()))
    print("mobilevit %s n=%d flip=%d %s: max err %.3g (scale %.3g)" % (size, n, flip, dtype, err, scale))
    assert err <= 1e-3 * scale
    if flip:                                                     # the mirrored half == the forward of the mirrored input
        assert torch.equal(net.raw_forward(torch.flip(xd, dims=[3]).contiguous()), raw[n:])


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_graph_replay_equals_eager(dtype):
    sd, x, _ = _small("s")
    net = _net(sd, dtype, "s")
    xd = x.cuda()
    a = net.raw_forward(xd, flip_test=True).clone()
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # replay
    net.use_graph = False
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # eager launches
    assert torch.isfinite(a).all()


def test_two_sub_batch_lanes_change_no_number():
    sd, x, _ = _small("xxs")
    xd = torch.from_numpy(synth.synth_crops(17, HW[0], HW[1], seed=9)).cuda()
    out = {}
    saved = os.environ.get("UDP_POSE_LANES")                                 # read by the library at every forward
    try:
        for lanes in ("1", "2"):
            os.environ["UDP_POSE_LANES"] = lanes
            net = _net(sd, "f16x2", "xxs")
            out[lanes] = net.raw_forward(xd, flip_test=True).clone()
            assert _lib.lib().udp_hrnet_lanes(net._compiled[HW][0], C.c_int(17)) == int(lanes)
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_LANES", None)
        else:
            os.environ["UDP_POSE_LANES"] = saved
    assert torch.equal(out["1"], out["2"]) and torch.isfinite(out["1"]).all()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_pad_channels_are_exact_zeros(dtype):
    """One eager forward on a workspace poisoned with NaN: every stored channel that is read was written first, and the
    pad channels were written as zeros (a NaN would survive a zero weight)."""
    sd, x, ref = _small("xs")
    net = _net(sd, dtype, "xs")
    net.use_graph = False
    xd = x.cuda().contiguous()
    net.raw_forward(xd)                                                      # allocates the workspace
    net._ws.fill_(0xFF)                                                      # NaN in fp32 and in both fp16 planes
    got = net.raw_forward(xd).clone()
    assert not torch.isnan(got).any()
    assert float(np.abs(got.cpu().numpy() - ref[:3]).max()) <= 1e-3 * max(1.0, float(np.abs(ref).max()))


def test_offset_target_has_51_channels():
    sd, x, ref = _small("xxs", "offset")
    net = _net(sd, "f16x2", "xxs", "offset")
    got = net(x.cuda().contiguous()).clone().cpu().numpy()
    assert got.shape == (3, 51, 16, 16)
    assert float(np.abs(got - ref[:3]).max()) <= 1e-3 * max(1.0, float(np.abs(ref).max()))
