"""pose_mobilenetv3_small_pixel_shuffle and pose_mobilenetv3_small on the GPU against the fp64 restatement of the block
table (tests/mobilenetv3_ref.py -- torchvision is not installed, so no fixture of the reference's own module exists):
64x64 / 96x64 inputs with and without the flip-test half, one 256x192 crop per net, and the executor's invariants
(replay == eager, one lane == two, flops)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mobilenetv3_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilenetv3 import synth_mobilenetv3_state_dict

pytestmark = pytest.mark.gpu

NETS = {"pixel_shuffle": "pose_mobilenetv3_small_pixel_shuffle", "deconv": "pose_mobilenetv3_small"}
EXTRA = {"pixel_shuffle": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1},
         "deconv": {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
                    "NUM_DECONV_KERNELS": [4, 4, 4], "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1}}
SIZES = {"pixel_shuffle": (64, 64), "deconv": (96, 64)}          # H / 32 = 2 and 3
_cache = {}


def _net(head, sd, dtype):
    cfg = {"MODEL": {"NAME": NETS[head], "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": EXTRA[head]}}
    return MODELS[NETS[head]](cfg, is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()


def _case(head, hw=None):
    """Seeded weights with BatchNorm statistics calibrated on 256 crops (at H / 32 = 2 or 3 a late BatchNorm sees 4 or 6
    samples per crop: tests/test_gpu_shufflenet_plus.py has the numbers), 17 crops (one at 256x192) and their fp64
    heat-maps [normal | mirrored]; computed once per (head, size)."""
    h, w = hw or SIZES[head]
    key = (head, h, w)
    if key not in _cache:
        big = (h, w) == (256, 192)
        sd = synth_mobilenetv3_state_dict(seed=13 + h, head=head)
        yc = R.forward(sd, torch.from_numpy(synth.synth_crops(8 if big else 256, h, w, seed=5)), calibrate=True)
        k = 0.25 / float(yc.std())
        sd["final_layer.weight"], sd["final_layer.bias"] = sd["final_layer.weight"] * k, sd["final_layer.bias"] * k
        x = torch.from_numpy(synth.synth_crops(1 if big else 17, h, w, seed=9))
        ref = torch.cat([R.forward(sd, x, dtype=torch.float64), R.forward(sd, torch.flip(x, dims=[3]), dtype=torch.float64)])
        _cache[key] = (sd, x, ref.numpy())
    return _cache[key]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("n", [3, 17])
@pytest.mark.parametrize("head", ["pixel_shuffle", "deconv"])
def test_small_inputs_match_fp64_restatement(head, n, flip, dtype):
    sd, x, ref = _case(head)
    h, w = SIZES[head]
    net = _net(head, sd, dtype)
    xd = x[:n].cuda().contiguous()
    raw = net.raw_forward(xd, flip_test=flip).clone()
    want = np.concatenate([ref[:n], ref[17:17 + n]]) if flip else ref[:n]
    assert raw.shape == want.shape == (n * (2 if flip else 1), 17, h // 4, w // 4)
    err = float(np.abs(raw.cpu().numpy() - want).max())
    scale = max(1.0, float(np.abs(want).max()))
    print("mobilenetv3 %s n=%d flip=%d %s: max err %.3g (scale %.3g)" % (head, n, flip, dtype, err, scale))
    assert err <= 1e-3 * scale
    if flip:                                                     # the mirrored half == the forward of the mirrored input
        assert torch.equal(net.raw_forward(torch.flip(xd, dims=[3]).contiguous()), raw[n:])


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("head", ["pixel_shuffle", "deconv"])
def test_full_size_crop(head, dtype):
    """One 256x192 crop: the 1e-3 gate, arg-max equality and the flop count (measured errors: NOTES.md)."""
    sd, x, ref = _case(head, (256, 192))
    net = _net(head, sd, dtype)
    got = net(x.cuda()).clone().cpu().numpy()
    assert got.shape == (1, 17, 64, 48)
    err = float(np.abs(got - ref[:1]).max())
    prog = net.program(256, 192)
    print("mobilenetv3 %s 256x192 %s: max |heat-map - fp64| %.3g (max |ref| %.3g), %d launches" % (head, dtype, err, float(np.abs(ref).max()),
                                                                                              len(prog._ops)))
    assert err <= 1e-3 * max(1.0, float(np.abs(ref[:1]).max()))
    np.testing.assert_array_equal(got.reshape(1, 17, -1).argmax(2), ref[:1].reshape(1, 17, -1).argmax(2))
    macs = prog.macs_per_image()
    assert abs(_lib.lib().udp_hrnet_flops_per_image(net._compiled[(256, 192)][0]) - 2 * macs) <= 1e-6 * macs


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("head", ["pixel_shuffle", "deconv"])
def test_graph_replay_equals_eager(head, dtype):
    sd, x, _ = _case(head)
    net = _net(head, sd, dtype)
    xd = x.cuda()
    a = net.raw_forward(xd, flip_test=True).clone()
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # replay
    net.use_graph = False
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # eager launches
    assert torch.isfinite(a).all()


@pytest.mark.parametrize("head", ["pixel_shuffle", "deconv"])
def test_two_sub_batch_lanes_change_no_number(head):
    sd, x, _ = _case(head)
    xd = x.cuda()
    out = {}
    saved = os.environ.get("UDP_POSE_LANES")                                 # read by the library at every forward
    try:
        for lanes in ("1", "2"):
            os.environ["UDP_POSE_LANES"] = lanes
            net = _net(head, sd, "f16x2")
            out[lanes] = net.raw_forward(xd, flip_test=True).clone()
            assert _lib.lib().udp_hrnet_lanes(net._compiled[SIZES[head]][0], C.c_int(17)) == int(lanes)
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_LANES", None)
        else:
            os.environ["UDP_POSE_LANES"] = saved
    assert torch.equal(out["1"], out["2"])
