"""The step structure of the 3x3 stride-1 weight-stationary body (csrc/conv_ws.hip: conv_ws_body, LATE), to the bit.

The body decodes its steps with running values (UDP_WS_INC_STEP: tap row, chunk, row offset in LDS, offset of the next A
fragments), and two of the three steps of a loop trip are straight-line code that the compiler schedules into the step
before.  The cases are the ones a B ring that runs on from step to step would need as well (built and measured next to
it, NOTES.md r11).  What all of that can get wrong is WHICH fragment meets which MFMA: a tap row, a stage buffer, a ring
slot or a clamped pixel row off by one.  The method is tests/test_gpu_ws_exact.py's: operands on a grid on which every partial sum
is exact in fp32 (proved per case by its ``_reference``), the expected planes = f16x2.encode of the fp64 reference, compared
bit for bit in a poisoned workspace.  On top of it every input pixel carries its own index in its leading channels
(``_distinct``): no two pixels of a case have the same channel vector, so a fragment read from the wrong tap or the wrong
stage cannot cancel.  Every 3x3 case has a residual and a ReLU (the peeled tail requests the residual late).

Cases, the smallest shapes that reach each path:
  pb8      32->32 on 2x32x16, the 8-block arm, one K chunk: the whole conv is two loop trips and the peeled tail
  c64      64->64 on 2x12x8, the (6, 2) arm, two K chunks: the chunk boundary inside the loop, both stage buffers
  merged   the two in one conv_ws_multi<3> launch: both phases in one kernel
  m240     32->32 on 1x20x12: 240 pixels, no multiple of 128 -- the last block of the tile is clamped rows.  The chooser
           gives the 8-block arm only tiles that fill all of its 512 pixels (ws_tile), and a 15-block tile is no member
           of a merged launch either: the shape runs the 4-block instantiation on its own
  m304     32->32 on 1x19x16: 19 blocks under the 6-block body of a merged launch -- the last wave has one real block,
           its block 1 and all behind it are clamped rows
  c96      96->64 on 1x12x8, three K chunks (the 3-block instantiation on its own); c80: 80->64 on 1x24x8, three K chunks
           with a ragged last one (96 has none), the (6, 2) arm, merged with m304
  sbuf     64->64 on 1x8x48 with one cout pair per workgroup: the one stride-1 shape with a single stage buffer, which
           the workgroup refills at the chunk boundary (asserted through the `ws conv` debug line)
  k1       1x1 96->64, three K chunks: every step is a chunk boundary (the body without the running values)
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import conv_arms as ca
import test_gpu_ws_exact as ex
from microprog import Micro, new_op, nhwc
from test_gpu_program_ops import _env
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

H2 = ex.H2
SBUF_LINE = re.compile(r"^ws conv k3 s1 .* CP=(\d+) PB=(\d+) lds=\d+ \(one stage buffer\)", re.M)


def _distinct(d, grid):
    """Overwrite the leading input channels with the digits of the pixel's index (over all images), on the case's grid."""
    x = d["x"]
    n, cin, h, w = x.shape
    base = 2 * grid["ximax"] + 1
    idx = torch.arange(n * h * w).reshape(n, h, w)
    digits = 1
    while base ** digits < n * h * w:
        digits += 1
    assert digits <= cin
    for k in range(digits):
        x[:, k] = ((idx // base ** k) % base - grid["ximax"]).to(torch.float32) * grid["xq"]
    flat = x.permute(0, 2, 3, 1).reshape(n * h * w, cin)
    assert len(torch.unique(flat, dim=0)) == n * h * w, "two input pixels carry the same values"
    return d


def _case(kind, seed, n, cin, cout, h, w, ks=3):
    grid = ex.ACT if kind == "act" else ex.WGT
    d = _distinct(ex._operands(grid, seed, n, cin, cout, h, w, ks, 1, ks == 3, True), grid)
    return d, ex._reference(d, kind)


# name: (kind, seed, n, cin, cout, h, w, the arm the case is about or None = whatever the chooser reports for a member)
MEMBERS = {
    "pb8": ("act", 101, 2, 32, 32, 32, 16, (8, 1)),
    "c64": ("wgt", 102, 2, 64, 64, 12, 8, (6, 2)),
    "m240": ("act", 103, 1, 32, 32, 20, 12, None),
    "c96": ("wgt", 104, 1, 96, 64, 12, 8, None),
    "c80": ("act", 105, 1, 80, 64, 24, 8, (6, 2)),
    "m304": ("wgt", 108, 1, 32, 32, 19, 16, (6, 1)),
}
_CASES = {}


def _member(name):
    if name not in _CASES:            # (computed once, shared by the merged run and the run alone, never modified)
        kind, seed, n, cin, cout, h, w, _ = MEMBERS[name]
        _CASES[name] = _case(kind, seed, n, cin, cout, h, w)
    return _CASES[name]


@pytest.mark.parametrize("names", [("pb8",), ("c64",), ("c64", "pb8"), ("m240",), ("c96",), ("c80", "m304")],
                         ids=["pb8", "c64", "merged-8-and-6", "m240", "c96", "merged-chunks-and-clamped"])
def test_launch_group(names, capfd):
    n = MEMBERS[names[0]][2]
    m = Micro(H2, n, seed=17)
    cases = []
    for name in names:
        kind, _, nn, cin, cout, h, w, arm = MEMBERS[name]
        assert nn == n
        d, ref = _member(name)
        if arm is None:
            t = ca.debug_tile(H2, 1, 3, 1, n, h, w, cin, cout, 0, 1)
            assert t is not None
            arm = t.arm
        bx, br, bo = m.buf(h, w, cin), m.buf(h, w, cout), m.buf(h, w, cout)
        assert torch.equal(m.fill(bx, d["x"]), d["x"]) and torch.equal(m.fill(br, d["r"]), d["r"])
        m.add(new_op(_lib.UDP_OP_CONV, ks=3, stride=1, relu=1, cin=cin, cout=cout, hin=h, win=w, hout=h, wout=w, in_buf=bx, res_buf=br,
                     out_buf=bo, group=1, **m.put_conv(d["wt"], d["bias"], ws=True)))
        m.wrote(bo)
        cases.append((name, ref, bo, (h, w, cin), arm))
    ex._flag(reset=True)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1"):
        assert m.run() == 0, m.error
    err = capfd.readouterr().err
    arms = {(int(g[2]), int(g[3]), int(g[4])): (int(g[10]), int(g[9])) for g in ex.WS_LINE.findall(err) if g[0] == "3"}
    assert arms == {geo: arm for _, _, _, geo, arm in cases}, arms
    assert [int(v) for v in ex.MULTI_LINE.findall(err)] == ([len(names)] if len(names) > 1 else []), err
    for name, ref, bo, _, _ in cases:
        got, want = m.read_raw(bo), m.raw_of(ref)
        assert np.array_equal(got, want), "%s: %d stored units differ" % (name, int((got != want).sum()))
    m.assert_untouched()
    m.check_head()
    assert not ex._flag()


def test_single_stage_buffer_refill(capfd):
    n, c, h, w = 1, 64, 8, 48
    knobs = {"UDP_POSE_WS_PB": "6", "UDP_POSE_WS_CP": "1"}
    with ca.env_knobs(**knobs):
        t = ca.debug_tile(H2, 1, 3, 1, n, h, w, c, c)
    # ws_tile's rule: two stage buffers of the 10 x 50 halo tile (2 x 64 KiB) exceed half the LDS, one does not
    assert t is not None and t.sbuf == 1 and t.arm == (6, 1) and t.TW == 48 and 2 * t.lds > 80 * 1024 >= t.lds, t
    d, ref = _case("act", 106, n, c, c, h, w)
    d_w, d_b, wexp = ex._weights(d, c)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 3, 1, 1
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = c, c, c, 1, wexp
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    d_x, d_r = f16x2.encode(nhwc(d["x"])).cuda(), f16x2.encode(nhwc(d["r"])).cuda()
    out = f16x2.encode(torch.full((n, h, w, c), ex.POISON)).cuda()
    ex._flag(reset=True)
    capfd.readouterr()
    with ca.env_knobs(UDP_POSE_DEBUG_TILES="1", **knobs):
        rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[H2], n, _lib.ptr(d_x), _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(d_r),
                                         None, None, None, _lib.ptr(out), _lib.stream_ptr())
    assert rc == 0, _lib.lib().udp_last_error()
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert SBUF_LINE.findall(err) == [("1", "6")], err          # the path was taken: one stage buffer, (6, 1)
    bad = ex._bits16(out.cpu()) != ex._bits16(f16x2.encode(nhwc(ref)))
    assert not bool(bad.any()), "%d stored units differ, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    assert not ex._flag()


def test_k1_three_chunks(capfd):
    n, cin, cout, h, w = 2, 96, 64, 13, 24
    d, ref = _case("act", 107, n, cin, cout, h, w, ks=1)
    ex._direct(d, ref, n, cin, cout, h, w, {"UDP_POSE_WS_PB": "6", "UDP_POSE_WS_CP": "2"}, (6, 2), capfd)
    assert not ex._flag()
