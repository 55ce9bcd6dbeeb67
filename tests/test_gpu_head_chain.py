"""The chained head (csrc/conv_ws.hip: conv_head_chain_kernel; csrc/hrnet.hip: mark_head_chain): the 1x1 conv
32 -> 128 with three up-sampled addends and ReLU that ends an HRNet-W32 program, and the 1x1 conv 128 -> 17 that writes
the heat-maps, run as ONE launch that never writes the 128-channel map.  UDP_POSE_NO_HEAD_CHAIN=1 keeps the two launches.

  * op level (a hand-made program in the style of tests/microprog.py: stem, the pair, nothing else): the heat-maps
    against the fp64 evaluation with Y quantised as the format stores it, under microprog's rule 3 x CPU-fp32 error + 4
    ulp; bit-equal to the two launches; the UDP_POSE_DEBUG_TILES line only when the pair is taken; the poisoned
    workspace -- the intermediate buffer included -- untouched by the fused run.  Shapes: 8x8 maps x 3 images (192
    pixels: six 32-pixel wave groups of one workgroup, up-maps 4x4, 2x2, 1x1) and 16x24 x 1 (384 pixels: two
    workgroups, the second half empty).  Maps are multiples of 8x8 (shift 3), so every wave group is full: there is no
    ragged group to reach.
  * range guard (the manner of tests/test_gpu_f16x2_range.py): one value of Y just below 65520, at 65520, hugely
    negative before the ReLU, and a NaN addend -- udp_f16x2_overflow and the heat-maps are the same fused and unfused.
  * whole net: the mini HRNet (width 32) at 64x64, N in {1, 5}, flip test on and off: knob on = knob off, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from microprog import Micro, new_op
from test_gpu_program_ops import _env
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import PoseHighResolutionNetHip

pytestmark = pytest.mark.gpu

H2 = "f16x2"
LINE = "head chain "
BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))
BIG, W0 = 32736.0, 2.0              # BIG * W0 = 65472, both exact in fp16


class HeadMicro(Micro):
    """stem (udp_hrnet_create demands one), conv 32 -> 128 + three addends + ReLU, conv 128 -> 17 into the output."""

    def __init__(self, n, h, w, seed=0, plant=None, last=False):
        super().__init__(H2, n, in_h=4 * h, in_w=4 * w, seed=seed)
        q = lambda t: mp.quant(t, H2)
        x = self.randn(n, 32, h, w)
        w1 = self.randn(128, 32, 1, 1) * float(np.sqrt(2.0 / 32))
        b1 = self.randn(128) * 0.1
        ups = [self.randn(n, 128, h >> s, w >> s) for s in (1, 2, 3)]
        w2 = q(self.randn(17, 128, 1, 1) * float(np.sqrt(2.0 / 128)))
        b2 = self.randn(17) * 0.1
        self.at = (n - 1, 127, h - 1, w - 1) if last else (0, 0, 0, 0)
        n0, c0, y0, x0 = self.at
        if plant:
            # Y[c0] = bias[c0] everywhere but at the chosen pixel, where it is 2 * 32736 + bias[c0] (exact in fp32); no
            # other channel reads input channel 0 (tests/test_gpu_f16x2_range.py, "How an element lands exactly")
            x[:, 0] = 0
            w1[:, 0] = 0
            w1[c0] = 0
            for t in ups:
                t[:, c0] = 0
            if plant == "relu_neg":
                x[n0, 0, y0, x0], w1[c0, 0], b1[c0] = BIG, -3.0, 0.25
            elif plant == "nan_up":
                ups[0][n0, c0, y0 >> 1, x0 >> 1] = float("nan")
            else:
                x[n0, 0, y0, x0], w1[c0, 0] = BIG, W0
                b1[c0] = {"below": BELOW, "at": 65520.0}[plant] - BIG * W0
        self.w1, self.b1, self.w2, self.b2 = q(w1), b1, w2, b2
        self.bx, self.by = self.buf(h, w, 32), self.buf(h, w, 128)
        self.bu = [self.buf(h >> s, w >> s, 128) for s in (1, 2, 3)]
        self.xq = self.fill(self.bx, x)
        self.uq = [self.fill(b, t) for b, t in zip(self.bu, ups)]
        self.add(new_op(_lib.UDP_OP_CONV, relu=1, cin=32, cout=128, hin=h, win=w, hout=h, wout=w, in_buf=self.bx, out_buf=self.by,
                        n_up=3, up_buf=self.bu, up_shift=[1, 2, 3], **self.put_conv(self.w1, self.b1, ws=True)))
        self.add(new_op(_lib.UDP_OP_CONV, cin=128, cout=17, hin=h, win=w, hout=h, wout=w, in_buf=self.by,
                        out_buf=_lib.UDP_BUF_OUTPUT, **self.put_conv(self.w2, self.b2, ws=True)))

    def create(self):                       # (Micro.create appends its own 64 -> 17 head: this program ends on the pair)
        arr = (_lib.ConvOp * len(self.ops))(*self.ops)
        blob = np.zeros(mp.round_up(self._blob_size, 256), dtype=np.uint8)
        for off, raw in self._blob:
            blob[off:off + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        self.blob = torch.from_numpy(blob).cuda()
        bufs = (C.c_int64 * len(self.buf_elems))(*self.buf_elems)
        h = C.c_void_p()
        _lib.check(_lib.lib().udp_hrnet_create(arr, len(self.ops), bufs, len(self.buf_elems), _lib.ptr(self.blob), self.blob.numel(),
                                               _lib.DTYPES[H2], self.in_h, self.in_w, 17, C.byref(h)))
        return h

    def reference(self, dt):
        y = F.conv2d(self.xq.to(dt), self.w1.to(dt), self.b1.to(dt))
        for s, t in zip((1, 2, 3), self.uq):
            y = y + F.interpolate(t.to(dt), scale_factor=2 ** s, mode="nearest")
        y = mp.quant(F.relu(y), H2)                                  # Y as the format stores it
        return F.conv2d(y.to(dt), self.w2.to(dt), self.b2.to(dt))


def _run(capfd, fused, *args, **kw):
    """One eager forward of a fresh program with the knob on or off -> (program, the pair's debug line was printed)."""
    m = HeadMicro(*args, **kw)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_NO_HEAD_CHAIN="0" if fused else "1"):
        assert m.run() == 0, m.error
    taken = LINE in capfd.readouterr().err
    assert taken == fused, "the pair was %staken" % ("" if taken else "not ")
    return m


def _same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("n,h,w", [(3, 8, 8), (1, 16, 24)], ids=["8x8x3", "16x24x1"])
def test_head_pair_matches_fp64_and_the_two_launches(n, h, w, capfd):
    fused = _run(capfd, True, n, h, w, seed=h)
    e_hip, e_cpu, gate = mp.parity("head chain %dx%d x %d" % (h, w, n), fused.heat, fused.reference(torch.float64),
                                   fused.reference(torch.float32), mp.ULP[H2])
    assert e_hip <= gate, (e_hip, e_cpu, gate)
    fused.assert_untouched()              # (the intermediate buffer is not declared as written: it must stay poison)
    assert (fused.read_raw(fused.by) == np.int16(mp.POISON16)).all()
    plain = _run(capfd, False, n, h, w, seed=h)
    plain.wrote(plain.by)
    plain.assert_untouched()
    assert not torch.isnan(plain.read(plain.by)).any()
    assert torch.equal(fused.heat, plain.heat)


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("kind,raises", [("below", False), ("at", True), ("relu_neg", False), ("nan_up", False)])
def test_head_pair_range_guard(kind, raises, last, capfd):
    """The split of Y keeps the range check of the store that no longer happens.  ``nan_up``: under the ReLU the NaN is
    stored as max(NaN, 0) = 0 and nothing leaves the range, fused or not."""
    verdicts, heats = [], []
    for fused in (True, False):
        _lib.f16x2_overflow(reset=True)
        m = _run(capfd, fused, 3, 8, 8, seed=11, plant=kind, last=last)
        verdicts.append(_lib.f16x2_overflow(reset=False))
        assert _lib.f16x2_overflow(reset=True) == verdicts[-1]
        assert not _lib.f16x2_overflow(reset=True)
        heats.append(m.heat)
    assert verdicts == [raises, raises], (kind, verdicts)
    assert _same(heats[0], heats[1])
    if not raises:
        assert torch.isfinite(heats[0]).all()


def _net(seed=3):
    extra = synth.scaled_extra(32, modules=(1, 1, 1), blocks=1)
    cfg = {"MODEL": {"EXTRA": extra, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian"}}
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=seed)
    return PoseHighResolutionNetHip(cfg, dtype=H2).load_state_dict(sd).to("cuda:0")


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("n", [1, 5])
def test_whole_net_knob_on_equals_knob_off(n, flip, capfd):
    x = torch.from_numpy(synth.synth_crops(n, 64, 64, seed=9)).cuda()
    outs = []
    for fused in (True, False):
        capfd.readouterr()
        with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_NO_HEAD_CHAIN="0" if fused else "1"):
            net = _net()                                   # a fresh handle: the knob is read when a forward is described
            outs.append(net.raw_forward(x, flip_test=flip).clone())
            torch.cuda.synchronize()
        assert (LINE in capfd.readouterr().err) == fused
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
