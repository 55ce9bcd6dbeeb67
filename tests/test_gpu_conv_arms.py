"""Every tile arm of both conv choosers on the GPU, each against the fp64 conv (table: tests/conv_arms.py).

A row is ONE udp_conv2d_fused call with the row's chooser knobs set around it.  For every row the test
  * captures the UDP_POSE_DEBUG_TILES line of the call and asserts it names the row's arm, with G, R, TW, the stage-buffer
    count, the LDS bytes and the workgroups equal to what the host-only diagnostic udp_debug_conv_tile returned
    (tests/test_conv_arms_cpu.py checks the table against that diagnostic without a GPU; this ties the report to the launch),
  * quantises the operands to the storage mode first (microprog.quant), pre-fills the output with NaN -- and with the
    POISON pattern outside an output view and behind the last image of an NCHW output, which must survive bit for bit,
  * asserts that no NaN is left and max |got - ref64| <= microprog.conv_tol: the shipped gates 1e-4 (f32) / 2e-5 (split
    fp16) / 6e-3 (bf16) x scale against torch's fp64 conv of the stored operands; hard-swish and SiLU rows use the
    reference and gate of their op tests (1.5 x / 1.1 x the conv gate of the pre-activation:
    tests/test_gpu_shufflenet_plus_ops.py, tests/test_gpu_mobilevitv2_ops.py),
  * with ReLU, that between 20 % and 80 % of the reference is clipped.
Rows of one group run on identical operands under different forced arms; their stored outputs must be bit-equal:
every accumulator sees the same K chunks and taps in the same order whatever the tile (tests/test_gpu_ws_pb8.py relies
on the same for 6 against 8 blocks).  That is far sharper than the fp64 gate: a wrong-but-small halo or mask error shows.
"""
import ctypes as C
import functools
import re
import zlib

import numpy as np
import pytest
import torch

import conv_arms as ca
import microprog as mp
from mobilevitv2_ref import silu
from shufflenet_plus_ref import hswish
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

POISON = -12345.0
WS_LINE = re.compile(r"^ws conv k(\d+) s(\d+) (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) CP=(\d+) PB=(\d+) lds=(\d+)( \(one stage buffer\))? wgs=(\d+)$", re.M)
LDS_LINE = re.compile(r"^conv k(\d+) s(\d+) (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) NB=(\d+) mbw=(\d+) lds=(\d+) wgs=(\d+)$", re.M)
GROUPS = sorted({r.group for r in ca.ROWS if r.group})


@functools.lru_cache(maxsize=None)
def _operands(dtype, ws, ks, stride, n, h, w, cin, cout, res, act):
    """Quantised operands, their device forms (host tensors) and the fp64 reference, once per distinct case."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((dtype, ws, ks, stride, n, h, w, cin, cout, res, act)).encode()))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    x = mp.quant(r(n, cin, h * stride, w * stride), dtype)
    if act >= ca.HS:      # pre-activations ~ N(0, 3^2): both knees of hard-swish, the dip and both tails of SiLU; fp16-exact weights
        wt, bias = (r(cout, cin, ks, ks) * (3.0 / np.sqrt(cin * ks * ks))).to(torch.float16).to(torch.float32), r(cout) * 0.5
    else:
        wt, bias = mp.quant(r(cout, cin, ks, ks) * float(np.sqrt(2.0 / (cin * ks * ks))), dtype), r(cout) * 0.1
    rs = mp.quant(r(n, cout, h, w), dtype) if res else None
    pre = mp.ref_conv(x.double(), wt, bias, stride=stride, res=None if rs is None else rs.double(), relu=act == 1)
    if act >= ca.HS:
        ref, tol = (hswish(pre), 1.5 * mp.conv_tol(dtype, pre)) if act == ca.HS else (silu(pre), 1.1 * mp.conv_tol(dtype, pre))
    else:
        ref, tol = pre, mp.conv_tol(dtype, pre)
    assert tuple(ref.shape) == (n, cout, h, w)
    cout_pad = mp.round_up(cout, 32)
    wp = torch.zeros(ks * ks, cout_pad, cin, dtype=torch.float32)
    wp[:, :cout] = wt.permute(2, 3, 0, 1).reshape(ks * ks, cout, cin)
    bp = torch.zeros(cout_pad, dtype=torch.float32)
    bp[:cout] = bias
    wexp = 0
    if ws:
        d_w, wexp = f16x2.pack_weights_ws(wp)
    else:
        d_w = f16x2.encode(wp) if dtype == "f16x2" else wp.to(torch.bfloat16) if dtype == "bf16" else wp
    return dict(x=x, rs=rs, ref=ref, tol=tol, d_w=d_w, d_b=bp, wexp=wexp, cout_pad=cout_pad)


def _store(t_nchw, dtype, view=None):
    """NCHW fp32 -> the device's NHWC storage; ``view`` = (coff, pitch): a channel slice of a wider tensor that is NaN elsewhere."""
    t = t_nchw.permute(0, 2, 3, 1)
    if view is not None:
        wide = torch.full(t.shape[:3] + (view[1],), float("nan"), dtype=torch.float32)
        wide[..., view[0]:view[0] + t.shape[3]] = t
        t = wide
    t = t.contiguous()
    return (f16x2.encode(t) if dtype == "f16x2" else t.to(torch.bfloat16) if dtype == "bf16" else t).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


_DONE = {}


def _run(row, capfd):
    """One udp_conv2d_fused call for ``row``; every per-row assertion.  Returns the stored output's bits (numpy)."""
    if row.id in _DONE:
        return _DONE[row.id]
    ws = row.fam != "lds"
    d = _operands(row.dtype, ws, row.ks, row.stride, row.n, row.h, row.w, row.cin, row.cout, row.res, row.act)
    want = ca.decide(row)
    assert want is not None and want.arm == row.arm, (row.id, want)
    n, h, w, cout, dtype = row.n, row.h, row.w, row.cout, row.dtype
    h2 = dtype == "f16x2"
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, row.ks, row.stride, row.act
    op.cin, op.cout, op.cout_pad = row.cin, cout, d["cout_pad"]
    op.hin, op.win, op.hout, op.wout = h * row.stride, w * row.stride, h, w
    op.wfmt, op.wexp = int(ws), d["wexp"]
    res_view, out_view = ((16, cout + 32), (32, cout + 64)) if row.views else (None, None)
    if res_view:
        op.res_coff, op.res_pitch = res_view
        op.out_coff, op.out_pitch = out_view
    ocoff, opitch = out_view or (0, cout)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    if row.nchw:
        # the images of an NCHW output are cout maps apart: a stored padded row (cout .. cout_pad - 1) of the last image
        # lands in the guard behind it, one of an earlier image in the next image's first maps
        op.out_buf = _lib.UDP_BUF_OUTPUT
        real = n * cout * h * w
        out = torch.full((real + (d["cout_pad"] - cout) * h * w,), float("nan"), dtype=torch.float32, device="cuda")
        out[real:] = POISON
    elif h2:
        out = torch.full((n, h, w, 2, opitch), float("nan"), dtype=torch.float16, device="cuda")
    else:
        out = torch.full((n, h, w, opitch), float("nan"), dtype=tdt, device="cuda")
    if out_view:
        out[...] = POISON
        out[..., ocoff:ocoff + cout] = float("nan")
    before = _bits(out).clone()
    d_x, d_w, d_b = _store(d["x"], dtype), d["d_w"].cuda(), d["d_b"].cuda()
    d_r = _store(d["rs"], dtype, res_view) if row.res else None
    torch.cuda.synchronize()
    capfd.readouterr()
    with ca.env_knobs(UDP_POSE_DEBUG_TILES="1", **row.env):
        rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(d_x), _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(d_r),
                                         None, None, None, _lib.ptr(out), _lib.stream_ptr())
    assert rc == 0, (row.id, _lib.lib().udp_last_error())
    torch.cuda.synchronize()
    err_text = capfd.readouterr().err
    # ---- the launch is the one the diagnostic reported
    if ws:
        m = WS_LINE.findall(err_text)
        assert len(m) == 1, (row.id, err_text)
        g = m[0]
        got_tile = ca.Tile((int(g[10]), int(g[9])), int(g[6]), int(g[7]), int(g[8]), int(bool(g[12])), int(g[11]), int(g[13]), 0)
        assert tuple(map(int, g[:6])) == (row.ks, row.stride, h, w, row.cin, cout), (row.id, g)
    else:
        m = LDS_LINE.findall(err_text)
        assert len(m) == 1, (row.id, err_text)
        g = m[0]
        got_tile = ca.Tile((int(g[9]), int(g[10])), int(g[6]), int(g[7]), int(g[8]), want.sbuf, want.lds if want.persist else int(g[11]),
                           int(g[12]), want.persist)
        assert tuple(map(int, g[:6])) == (row.ks, row.stride, h, w, row.cin, cout), (row.id, g)
    assert got_tile == want, (row.id, got_tile, want)
    assert all(ca.has_feature(row, got_tile, f) for f in row.feats), (row.id, got_tile)
    # ---- nothing outside the output was written
    after = _bits(out)
    if row.nchw:
        assert torch.equal(after[real:], before[real:]), "%s: a padded output row was stored behind the last image" % row.id
        got = out[:real].reshape(n, cout, h, w).cpu()
    else:
        if out_view:
            keep = torch.ones(opitch, dtype=torch.bool, device="cuda")
            keep[ocoff:ocoff + cout] = False
            assert torch.equal(after[..., keep], before[..., keep]), "%s: the conv wrote outside its output slice" % row.id
        sl = out[..., ocoff:ocoff + cout]
        got = (f16x2.decode(sl) if h2 else sl.float()).cpu().permute(0, 3, 1, 2)
    # ---- parity
    ref, tol = d["ref"], d["tol"]
    assert not torch.isnan(got).any(), "%s: output not fully written, or an unread NaN channel reached it" % row.id
    if row.act == 1:
        assert 0.2 < float((ref == 0).double().mean()) < 0.8, row.id          # the ReLU clips some and not all
    err = float((got.double() - ref).abs().max())
    print("%s arm %s  n%d %dx%d C%d->%d  G=%d R=%d TW=%d sbuf=%d  err %.3g (gate %.3g)" % (
        row.id, row.arm, n, h, w, row.cin, cout, want.G, want.R, want.TW, want.sbuf, err, tol))
    assert err <= tol, (row.id, err, tol)
    _DONE[row.id] = after.cpu().numpy() if row.group else None
    return _DONE[row.id]


@pytest.mark.parametrize("row", ca.ROWS, ids=lambda r: r.id)
def test_arm_matches_fp64(row, capfd):
    _run(row, capfd)


@pytest.mark.parametrize("group", GROUPS)
def test_forced_arms_store_bit_equal_outputs(group, capfd):
    """Same operands, different arms: the stored outputs are bit-equal (the order of K chunks and taps into every accumulator
    does not depend on PB, CP, G, R, TW or the stage-buffer count; NB, MBW for the LDS-staged kernels)."""
    rows = [r for r in ca.ROWS if r.group == group]
    outs = [_run(r, capfd) for r in rows]
    tiles = {ca.decide(r) for r in rows}
    assert len(tiles) > 1, group
    for r, o in zip(rows[1:], outs[1:]):
        diff = int((o != outs[0]).sum())
        assert diff == 0, "%s and %s differ in %d stored units (%s vs %s)" % (rows[0].id, r.id, diff, ca.decide(rows[0]), ca.decide(r))
    print("%s: %d runs over %d distinct tiles, bit-equal" % (group, len(rows), len(tiles)))
