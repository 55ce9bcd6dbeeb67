"""Sub-batch lanes write their heat-maps in place (csrc/hrnet.hip: udp_hrnet_forward, ConvParams::out_skip).

A batch of 16 crops or more runs as two halves on two streams.  With the flip test each half computes [its images |
their mirrored copies] while the caller's layout is [all images | all mirrored]: the output conv of each lane now puts
its mirrored rows behind ALL the plain images itself, where four device-to-device copies did it before.  Only the
weight-stationary split-fp16 kernels can; a program whose output conv is another kernel keeps the staging copies.

The mini HRNet (width 32) at 64x64, 16 and 17 crops (an even and an uneven split), flip test on and off: one lane
(UDP_POSE_LANES=1) and two lanes give the same heat-maps, bit for bit, on the first call (graph capture) and on a replay;
the output tensor is pre-filled with NaN and followed by guard rows: every row is written, the guards are not.
UDP_POSE_HEAD_WS=0 makes the planner give the output conv plain weights -- the LDS-staged kernel, which has no out_skip:
that program runs its two lanes through the staging copies and still matches one lane."""
import pytest
import torch

from test_gpu_program_ops import _env
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import PoseHighResolutionNetHip

pytestmark = pytest.mark.gpu

GUARD = 1234.5


def _net():
    extra = synth.scaled_extra(32, modules=(1, 1, 1), blocks=1)
    cfg = {"MODEL": {"EXTRA": extra, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian"}}
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=3)
    return PoseHighResolutionNetHip(cfg, dtype="f16x2").load_state_dict(sd).to("cuda:0")


def _forward_twice(x, flip, lanes):
    """Two graph forwards (capture, replay) of a fresh net into a NaN-filled tensor with two guard rows behind it."""
    n, _, h, w = x.shape
    rows = n * (2 if flip else 1)
    with _env(UDP_POSE_LANES=str(lanes)):
        net = _net()
        handle = net._compile(h, w)[0]
        assert _lib.lib().udp_hrnet_lanes(handle, n) == lanes
        xin, _ = net._stage(handle, x, flip)
        full = torch.empty(rows + 2, 17, h // 4, w // 4, device="cuda")
        outs = []
        for _ in range(2):
            full[:rows] = float("nan")
            full[rows:] = GUARD
            _lib.check(_lib.lib().udp_hrnet_forward(handle, _lib.ptr(xin), n, int(flip), _lib.ptr(net._ws), net._ws.numel(),
                                                    _lib.ptr(full), 1, _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert torch.isfinite(full[:rows]).all(), "rows left unwritten"
            assert bool((full[rows:] == GUARD).all()), "wrote behind the output"
            outs.append(full[:rows].clone())
        assert torch.equal(outs[0], outs[1]), "the replay differs from the first call"
        net._release()
    return outs[0]


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("n", [16, 17])
def test_two_lanes_equal_one_lane(n, flip):
    x = torch.from_numpy(synth.synth_crops(n, 64, 64, seed=9)).cuda()
    assert torch.equal(_forward_twice(x, flip, 1), _forward_twice(x, flip, 2))


def test_output_conv_without_out_skip_keeps_the_staging_copies():
    x = torch.from_numpy(synth.synth_crops(17, 64, 64, seed=9)).cuda()
    with _env(UDP_POSE_HEAD_WS="0"):
        assert torch.equal(_forward_twice(x, True, 1), _forward_twice(x, True, 2))
