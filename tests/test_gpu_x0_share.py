"""The shared-input launch of an exchange unit (csrc/conv_ws.hip: conv_ws_s2x_kernel; csrc/hrnet.hip: mark_x0_share):
the element-wise output 0 of a unit (fuse0) and the first stride-2 conv of every chain that leaves branch 0 read the
same 32-channel map, and run as ONE launch that stages each tile of it once.  UDP_POSE_NO_X0_SHARE=1 keeps the launches.

  * whole net (the mini HRNet of width 32 with modules (1, 1, 2): stage 2 gives fuse0 + one conv = 2 cout pairs, stage
    3 fuse0 + two convs = 3 pairs, the first module of stage 4 fuse0 + three convs = 4 pairs): knob on = knob off, bit
    for bit, at 64x64 (maps 16x16 .. 2x2) and 96x64 (24x16 .. 3x2: ragged tiles, odd low-resolution sizes), one image
    and five with the flip test, graph replay and eager; the UDP_POSE_DEBUG_TILES lines show that a 2-, a 3- and a
    4-pair set were formed with the knob on and none with it off;
  * the same nets, knob on, against the CPU oracle evaluated in fp64, under the gate tests/test_gpu_e2e.py applies to
    the mini fixtures (absolute 1e-3);
  * op level (a hand-made program in the manner of tests/microprog.py: the sum with two up-sampled addends, a conv
    32 -> 64 with residual and addend, a conv 32 -> 32 into a channel slice, a conv 32 -> 32): every output against
    fp64 under microprog's rule 3 x CPU-fp32 error + 4 ulp, bit-equal to the separate launches, nothing outside the
    declared outputs written;
  * range guard (the construction of tests/test_gpu_f16x2_range.py): one element of the sum, or of one conv's output,
    just below 65520 and at it: udp_f16x2_overflow and the stored outputs are what the separate launches give;
  * net.profile keeps working: the carried ops report 0, the carrying op the launch.
"""
import functools
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from microprog import Micro, new_op
from oracle import hrnet as ohrnet
from test_gpu_f16x2_range import BELOW, BIG, W0
from test_gpu_program_ops import _env
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import PoseHighResolutionNetHip

pytestmark = pytest.mark.gpu

H2 = "f16x2"
LINE = re.compile(r"^x0 share .* pairs=(\d) routes=\[([\d,]+)\] fuse0=(\d) ", re.M)
EXTRA = synth.scaled_extra(32, modules=(1, 1, 2), blocks=1)
SHAPES = {"64x64": (64, 64), "96x64": (96, 64)}


def _sets(err):
    return sorted(int(m.group(1)) for m in LINE.finditer(err))


@functools.lru_cache(maxsize=None)
def _case(shape, n):
    """Weights (BatchNorm statistics calibrated on the batch), crops and the fp64 oracle heat-maps of [crops | mirrored]."""
    h, w = SHAPES[shape]
    sd = synth.synth_state_dict(EXTRA, 17, "gaussian", seed=3)
    x = torch.from_numpy(synth.synth_crops(n, h, w, seed=9))
    ohrnet.hrnet_forward(sd, EXTRA, x, calibrate=True)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    both = torch.cat([x, torch.flip(x, dims=[3])]).double()
    return sd, x, ohrnet.hrnet_forward(sd64, EXTRA, both)


def _net(sd):
    cfg = {"MODEL": {"EXTRA": EXTRA, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian"}}
    return PoseHighResolutionNetHip(cfg, dtype=H2).load_state_dict(sd).to("cuda:0")


def _forward(capfd, sd, x, shared, flip, graph=True):
    """One forward of a fresh handle (the knob is read when a forward is described) -> (heat-maps, pair counts of the sets)."""
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_NO_X0_SHARE="0" if shared else "1"):
        net = _net(sd)
        net.use_graph = graph
        out = net.raw_forward(x.cuda(), flip_test=flip).clone()
        torch.cuda.synchronize()
    return out, _sets(capfd.readouterr().err)


@pytest.mark.parametrize("n,flip", [(1, False), (5, True)], ids=["n1", "n5flip"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_whole_net_knob_on_equals_knob_off_and_matches_fp64(shape, n, flip, capfd):
    sd, x, ref = _case(shape, n)
    on, sets_on = _forward(capfd, sd, x, True, flip)
    off, sets_off = _forward(capfd, sd, x, False, flip)
    assert sets_on == [2, 3, 4], "sets formed with the knob on: %s" % sets_on
    assert sets_off == [], "sets formed with the knob off: %s" % sets_off
    assert torch.isfinite(on).all()
    assert torch.equal(on, off)
    want = ref if flip else ref[:n]
    err = float((on.cpu().double() - want).abs().max())
    print("x0 share %s n=%d flip=%d: max abs err vs fp64 %.3g (max |ref| %.3g)" % (shape, n, flip, err, float(want.abs().max())))
    np.testing.assert_allclose(on.cpu().numpy(), want.numpy(), rtol=0, atol=1e-3)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_graph_replay_and_eager_run_equal_the_separate_launches(graph, capfd):
    sd, x, _ = _case("96x64", 5)
    on, sets_on = _forward(capfd, sd, x, True, True, graph=graph)
    off, sets_off = _forward(capfd, sd, x, False, True, graph=graph)
    assert sets_on == [2, 3, 4] and sets_off == []
    assert torch.equal(on, off)
    if graph:                                # the replay of the cached graph as well
        with _env(UDP_POSE_NO_X0_SHARE="0"):
            net = _net(sd)
            first = net.raw_forward(x.cuda(), flip_test=True).clone()
            again = net.raw_forward(x.cuda(), flip_test=True).clone()
        assert torch.equal(first, on) and torch.equal(again, on)


def test_profile_gives_the_whole_time_to_the_carrying_op(capfd):
    sd, x, _ = _case("64x64", 1)
    with _env(UDP_POSE_NO_X0_SHARE="0"):
        net = _net(sd)
        ms, table = net.profile(x.cuda())
    names = [t[0] for t in table]
    assert len(ms) == len(names) and (ms >= 0).all()
    fuse0 = [i for i, nm in enumerate(names) if nm.endswith(".fuse0")]
    assert len(fuse0) == 3 and all(ms[i] > 0 for i in fuse0)
    carried = [i for i, nm in enumerate(names) if re.search(r"fuse_layers\.[123]\.0\.0\.0$", nm)]      # (op name = conv name: chain step 0, ".0")
    assert len(carried) == 6 and all(ms[i] == 0 for i in carried), [(names[i], ms[i]) for i in carried]
    with _env(UDP_POSE_NO_X0_SHARE="1"):
        ms_off, _ = _net(sd).profile(x.cuda())
    assert all(ms_off[i] > 0 for i in carried + fuse0)


# ---------------------------------------------------------------- op level
class X0Micro(Micro):
    """stem, then over one pre-filled 32-channel map x0 [h, w]:  out0 = relu(x0 + up(u1, 2) + up(u2, 4));
    A = relu(conv_s2(x0) + res + up(ua, 2)), 64 channels;  B = relu(conv_s2(x0)) into channels 32..63 of a 64-channel
    tensor;  C = relu(conv_s2(x0)).  ``plant`` = (site, kind): one element of out0 (site "fuse") or of C (site "conv")
    lands on ``kind`` = "below" | "at" (tests/test_gpu_f16x2_range.py, "How an element lands exactly")."""

    def __init__(self, n, h, w, seed=0, plant=None, last=False):
        super().__init__(H2, n, in_h=4 * h, in_w=4 * w, seed=seed)
        q = lambda t: mp.quant(t, H2)
        ho, wo = h // 2, w // 2
        x = self.randn(n, 32, h, w)
        u1, u2 = self.randn(n, 32, h // 2, w // 2), self.randn(n, 32, h // 4, w // 4)
        res, ua = self.randn(n, 64, ho, wo), self.randn(n, 64, ho // 2, wo // 2)
        ws = [self.randn(c, 32, 3, 3) * float(np.sqrt(2.0 / 288)) for c in (64, 32, 32)]
        bs = [self.randn(c) * 0.1 for c in (64, 32, 32)]
        self.at = None
        if plant:
            site, kind = plant
            target = {"below": BELOW, "at": 65520.0}[kind]
            x[:, 0] = 0                                  # input channel 0 carries the planted value alone ...
            for wt in ws:
                wt[:, 0] = 0                             # ... and no conv output but the chosen one reads it
            if site == "fuse":
                n0, c0, y0, x0 = (n - 1, 0, h - 1, w - 1) if last else (0, 0, 0, 0)
                x[n0, 0, y0, x0] = BIG * W0              # 65472 + 47.99609375 (or 48): two stored values, the sum exact in fp32
                u1[n0, 0, y0 >> 1, x0 >> 1] = target - BIG * W0
                u2[n0, 0, y0 >> 2, x0 >> 2] = 0
            else:
                n0, c0, y0, x0 = (n - 1, 31, ho - 1, wo - 1) if last else (0, 0, 0, 0)
                x[n0, 0, 2 * y0, 2 * x0] = BIG
                ws[2][c0] = 0
                ws[2][c0, 0, 1, 1] = W0
                bs[2][c0] = target - BIG * W0
            self.at = (site, n0, c0, y0, x0)
        self.ws, self.bs = [q(t) for t in ws], bs
        self.bx, self.b0 = self.buf(h, w, 32), self.buf(h, w, 32)
        self.bu1, self.bu2 = self.buf(h // 2, w // 2, 32), self.buf(h // 4, w // 4, 32)
        self.br, self.bua = self.buf(ho, wo, 64), self.buf(ho // 2, wo // 2, 64)
        self.ba, self.bct, self.bc = self.buf(ho, wo, 64), self.buf(ho, wo, 64), self.buf(ho, wo, 32)
        self.xq, self.u1q, self.u2q = self.fill(self.bx, x), self.fill(self.bu1, u1), self.fill(self.bu2, u2)
        self.rq, self.uaq = self.fill(self.br, res), self.fill(self.bua, ua)
        geo = dict(ks=3, stride=2, cin=32, hin=h, win=w, hout=ho, wout=wo, in_buf=self.bx, relu=1)
        self.add(new_op(_lib.UDP_OP_FUSE, relu=1, cin=32, cout=32, hin=h, win=w, hout=h, wout=w, in_buf=self.bx, out_buf=self.b0,
                        n_up=2, up_buf=[self.bu1, self.bu2], up_shift=[1, 2]))
        self.add(new_op(_lib.UDP_OP_CONV, cout=64, out_buf=self.ba, res_buf=self.br, n_up=1, up_buf=[self.bua], up_shift=[1],
                        **geo, **self.put_conv(self.ws[0], self.bs[0], ws=True)))
        self.add(new_op(_lib.UDP_OP_CONV, cout=32, out_buf=self.bct, out_coff=32, out_pitch=64, **geo,
                        **self.put_conv(self.ws[1], self.bs[1], ws=True)))
        self.add(new_op(_lib.UDP_OP_CONV, cout=32, out_buf=self.bc, **geo, **self.put_conv(self.ws[2], self.bs[2], ws=True)))
        self.wrote(self.b0)
        self.wrote(self.ba)
        self.wrote(self.bct, 32, 32)
        self.wrote(self.bc)

    def outputs(self):
        return [self.read_raw(self.b0), self.read_raw(self.ba), self.read_raw(self.bct, 32, 32), self.read_raw(self.bc)]

    def decoded(self):
        return [self.read(self.b0), self.read(self.ba), self.read(self.bct, 32, 32), self.read(self.bc)]

    def reference(self, dt):
        up = lambda t, s: F.interpolate(t.to(dt), scale_factor=s, mode="nearest")
        conv = lambda k: F.conv2d(self.xq.to(dt), self.ws[k].to(dt), self.bs[k].to(dt), stride=2, padding=1)
        return [F.relu(self.xq.to(dt) + up(self.u1q, 2) + up(self.u2q, 4)), F.relu(conv(0) + self.rq.to(dt) + up(self.uaq, 2)),
                F.relu(conv(1)), F.relu(conv(2))]


def _run(capfd, shared, *args, **kw):
    m = X0Micro(*args, **kw)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_NO_X0_SHARE="0" if shared else "1"):
        assert m.run() == 0, m.error
    assert _sets(capfd.readouterr().err) == ([4] if shared else [])
    return m


@pytest.mark.parametrize("n,h,w", [(3, 8, 8), (1, 16, 24), (2, 24, 40)], ids=["8x8x3", "16x24x1", "24x40x2"])
def test_op_level_matches_fp64_and_the_separate_launches(n, h, w, capfd):
    """8x8 x 3: one tile of three images; 16x24: one image; 24x40 x 2 (outputs 12x20): several tiles per image."""
    shared = _run(capfd, True, n, h, w, seed=h + w)
    r64, r32 = shared.reference(torch.float64), shared.reference(torch.float32)
    for name, got, a, b in zip(("out0", "A", "B", "C"), shared.decoded(), r64, r32):
        e_hip, e_cpu, gate = mp.parity("x0 share %dx%d x %d %s" % (h, w, n, name), got, a, b, mp.ULP[H2])
        assert e_hip <= gate, (name, e_hip, e_cpu, gate)
    shared.assert_untouched()
    shared.check_head()
    plain = _run(capfd, False, n, h, w, seed=h + w)
    plain.assert_untouched()
    for a, b in zip(shared.outputs(), plain.outputs()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("last", [False, True], ids=["first", "last"])
@pytest.mark.parametrize("kind,raises", [("below", False), ("at", True)])
@pytest.mark.parametrize("site", ["fuse", "conv"])
def test_range_guard_reports_what_the_separate_launches_report(site, kind, raises, last, capfd):
    verdicts, outs = [], []
    for shared in (True, False):
        _lib.f16x2_overflow(reset=True)
        m = _run(capfd, shared, 3, 8, 8, seed=5, plant=(site, kind), last=last)
        verdicts.append(_lib.f16x2_overflow(reset=False))
        assert _lib.f16x2_overflow(reset=True) == verdicts[-1]
        assert not _lib.f16x2_overflow(reset=True)
        outs.append(m.outputs())
        _, n0, c0, y0, x0 = m.at
        v = float(m.decoded()[0 if site == "fuse" else 3][n0, c0, y0, x0])
        assert (np.isinf(v) or np.isnan(v)) if raises else v == 65520.0, v       # (below: what the format makes of it)
    assert verdicts == [raises, raises], (site, kind, verdicts)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
