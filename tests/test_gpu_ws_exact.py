"""Weight-stationary split-fp16 convs (csrc/conv_ws.hip: conv_ws_body) whose stored result is known to the bit.

The operands sit on a grid coarse enough that every product and every partial sum of the kernel is exact in fp32, in
any order: all terms of one output element are integer multiples of one quantum q, and the sum of their magnitudes
(the split pieces hi and lo of every operand counted apart, bias and residual included) stays below 2^24 q.  Each case
proves that of its own operands (``_reference``) and checks that the fp64 reference equals its own fp32 rounding.
The expected stored planes are then udp_pose_amd.f16x2.encode of that reference, compared bit for bit with what the
kernel wrote into a poisoned workspace -- any change to the epilogue's arithmetic (scale, bias, residual decode, ReLU,
hi / lo split), to the B-fragment addressing or to the tile decode shows as a wrong bit, not as a tolerance.

Both planes are exercised, never in the same product (the scheme drops lo x lo by design):
  kind "act"  activations (input, residual, addends) with non-zero lo planes, weights exactly representable in hi;
  kind "wgt"  weights with non-zero lo planes, activations exactly representable in hi.

Cases, the smallest shapes that reach each path of the body:
  merged   3x3 s1 32->32 on 2x32x16 + residual + ReLU (the 8-block arm, act) merged with 64->64 on 2x12x8 (the (6, 2)
           arm, wgt) in one conv_ws_multi launch, and each alone (conv_ws_pb8_kernel / conv_ws_h2_kernel)
  c128     3x3 s1 128->128 on 3x8x6 + residual (several images per tile, four K chunks), act
  s2       3x3 s2 32->64 on 2x26x40 -> 13x20 (row width no multiple of 16, edge tiles, one stage buffer), wgt
  k1       1x1 48->128 on 2x13x24 (ragged last K chunk, four cout pairs), act
  head     1x1 32->17 into the NCHW fp32 output on 1x7x37 (the head shape of tests/conv_arms.py), wgt
  x0       an x0-share set on 2x16x16: the element-wise side output and two stride-2 convs in one launch, act
  edge     3x3 s1 32->32 on 1x8x8 with one output element at 65520 (range flag raised, act) and at 65504 (clear, wgt)
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_arms as ca
from microprog import Micro, new_op, nhwc
from test_gpu_program_ops import _env
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

H2 = "f16x2"
POISON = -12345.0
WS_LINE = re.compile(r"^ws conv k(\d) s(\d) (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) CP=(\d+) PB=(\d+)", re.M)
MULTI_LINE = re.compile(r"^ws multi k3: members=(\d+) ", re.M)
SHARE_LINE = re.compile(r"^x0 share .* pairs=(\d) routes=\[([\d,]+)\] fuse0=(\d) ", re.M)

# grids: value = integer in [-imax, imax] x quantum.  13 significant bits = a non-zero lo plane; 3 bits = hi alone
ACT = dict(xq=2.0 ** -10, ximax=4095, wq=0.5, wimax=2)            # |x| < 4 in steps of 2^-10, w in {-1, -.5, 0, .5, 1}
WGT = dict(xq=1.0, ximax=2, wq=2.0 ** -11, wimax=4095)            # x in {-2 .. 2}, |w| < 2 in steps of 2^-11
ACT_EDGE = dict(xq=2.0 ** -4, ximax=4095, wq=1.0, wimax=1)        # (coarser: the planted element is 65520 = 2^20 quanta)
WGT_EDGE = dict(xq=1.0, ximax=2, wq=2.0 ** -6, wimax=4095)


def _ints(g, shape, imax):
    return torch.randint(-imax, imax + 1, shape, generator=g).to(torch.float32)


def _operands(grid, seed, n, cin, cout, h, w, ks, stride, res, relu):
    """x, weights, bias, residual on ``grid`` and the fp64 reference of act(conv + bias + res)."""
    g = torch.Generator().manual_seed(seed)
    q = grid["xq"] * grid["wq"]
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    d = dict(x=_ints(g, (n, cin, h, w), grid["ximax"]) * grid["xq"], wt=_ints(g, (cout, cin, ks, ks), grid["wimax"]) * grid["wq"],
             bias=_ints(g, (cout,), 4095) * q, r=_ints(g, (n, cout, ho, wo), grid["ximax"]) * grid["xq"] if res else None,
             q=q, ks=ks, stride=stride, relu=relu, ho=ho, wo=wo)
    return d


def _planes(t):
    """The two planes of a tensor in split-fp16 storage as fp64 values: (hi, lo * 2^-11)."""
    e = f16x2.encode(t.reshape(-1, 1))
    return e[:, 0, 0].double().reshape(t.shape), (e[:, 1, 0].double() / 2048.0).reshape(t.shape)


def _wplanes(wt):
    """The two planes of the weights as pack_weights_ws stores them (scaled by 2^wexp), descaled, fp64."""
    wexp = f16x2.weight_exponent(wt)
    s = torch.ldexp(wt.to(torch.float32), torch.tensor(wexp))
    hi = s.to(torch.float16).to(torch.float32)
    lo = (s - hi).to(torch.float16).to(torch.float32)
    assert torch.equal(hi + lo, s), "the weights are not exactly representable in their two planes"
    return torch.ldexp(hi.double(), torch.tensor(-wexp)), torch.ldexp(lo.double(), torch.tensor(-wexp))


def _reference(d, kind):
    """fp64 reference; proves the case exact (module docstring) and that the right planes carry the low bits."""
    x, wt, bias, r, q = d["x"], d["wt"], d["bias"], d["r"], d["q"]
    conv = lambda a, b: F.conv2d(a, b, None, stride=d["stride"], padding=d["ks"] // 2)
    xh, xl = _planes(x)
    wh, wl = _wplanes(wt)
    assert torch.equal(xh + xl, x.double()), "the activations are not exactly representable in split fp16"
    has_xlo, has_wlo = bool((xl != 0).any()), bool((wl != 0).any())
    assert (has_xlo, has_wlo) == ((True, False) if kind == "act" else (False, True)), (kind, has_xlo, has_wlo)
    if r is not None:
        rh, rl = _planes(r)
        assert torch.equal(rh + rl, r.double()) and bool((rl != 0).any()) == (kind == "act")
        assert torch.equal(torch.round(r.double() / q), r.double() / q)
    # every term of an output element is a multiple of q ...
    for a in (xh, xl):
        for b in (wh, wl):
            p = a.abs().max() * b.abs().max()
            assert p == 0 or torch.equal(torch.round(conv(a, b) / q), conv(a, b) / q)
    assert torch.equal(torch.round(bias.double() / q), bias.double() / q)
    # ... and the magnitudes of all of them together stay below 2^24 q: no partial sum, in any order, is ever rounded
    mass = conv(xh.abs() + xl.abs(), wh.abs() + wl.abs()) + bias.double().abs().view(1, -1, 1, 1)
    if r is not None:
        mass = mass + r.double().abs()
    assert float(mass.max()) < 2.0 ** 24 * q, (float(mass.max()), 2.0 ** 24 * q)
    y = conv(x.double(), wt.double()) + bias.double().view(1, -1, 1, 1)
    if r is not None:
        y = y + r.double()
    if d["relu"]:
        y = F.relu(y)
    assert torch.equal(y.float().double(), y), "the fp64 reference is not its own fp32 rounding"
    if d["relu"]:
        assert 0.1 < float((y == 0).double().mean()) < 0.9          # the ReLU clips some and not all
    return y.float()


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _weights(d, cout_pad):
    cout, cin, kh, kw = d["wt"].shape
    wp = torch.zeros(kh * kw, cout_pad, cin)
    wp[:, :cout] = d["wt"].permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    bp = torch.zeros(cout_pad)
    bp[:cout] = d["bias"]
    packed, wexp = f16x2.pack_weights_ws(wp)
    return packed.cuda(), bp.cuda(), wexp


def _direct(d, ref, n, cin, cout, h, w, env, want_arm, capfd, nchw=False):
    """One udp_conv2d_fused call on the weight-stationary kernels; the stored output against encode(ref), bit for bit."""
    cp = (cout + 31) // 32 * 32
    d_w, d_b, wexp = _weights(d, cp)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, d["ks"], d["stride"], int(d["relu"])
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cp, 1, wexp
    op.hin, op.win, op.hout, op.wout = h, w, d["ho"], d["wo"]
    d_x = f16x2.encode(nhwc(d["x"])).cuda()
    d_r = f16x2.encode(nhwc(d["r"])).cuda() if d["r"] is not None else None
    if nchw:
        op.out_buf = _lib.UDP_BUF_OUTPUT
        real = n * cout * d["ho"] * d["wo"]
        out = torch.full((real + (cp - cout) * d["ho"] * d["wo"],), POISON, dtype=torch.float32, device="cuda")
    else:
        out = f16x2.encode(torch.full((n, d["ho"], d["wo"], cout), POISON)).cuda()
    _lib.f16x2_overflow(reset=True)
    capfd.readouterr()
    with ca.env_knobs(UDP_POSE_DEBUG_TILES="1", **env):
        rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[H2], n, _lib.ptr(d_x), _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(d_r),
                                         None, None, None, _lib.ptr(out), _lib.stream_ptr())
    assert rc == 0, _lib.lib().udp_last_error()
    torch.cuda.synchronize()
    lines = WS_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1 and (int(lines[0][10]), int(lines[0][9])) == want_arm, (lines, want_arm)
    tile = dict(G=int(lines[0][6]), R=int(lines[0][7]), TW=int(lines[0][8]))
    if nchw:
        got = out[:real].reshape(n, cout, d["ho"], d["wo"]).cpu()
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), float((got - ref).abs().max())
        assert bool((out[real:] == POISON).all()), "a padded output row was stored behind the last image"
    else:
        want = f16x2.encode(nhwc(ref))
        bad = _bits16(out.cpu()) != _bits16(want)
        assert not bool(bad.any()), "%d stored units differ, first at %s" % (int(bad.sum()), bad.nonzero()[0].tolist())
    return tile


def _flag(reset=True):
    return bool(_lib.f16x2_overflow(reset=reset))


# ---------------------------------------------------------------- convs on a launch of their own
def test_c128_residual_across_images_and_chunks(capfd):
    n, c, h, w = 3, 128, 8, 6
    d = _operands(ACT, 1, n, c, c, h, w, 3, 1, True, True)
    ref = _reference(d, "act")
    tile = _direct(d, ref, n, c, c, h, w, {}, (2, 1), capfd)
    assert tile["G"] == 2, tile                     # two images per tile (the last tile holds one): indices cross image boundaries
    assert not _flag()


def test_s2_ragged_rows_edge_tiles_one_stage_buffer(capfd):
    n, cin, cout, h, w = 2, 32, 64, 26, 40
    d = _operands(WGT, 2, n, cin, cout, h, w, 3, 2, False, True)
    ref = _reference(d, "wgt")
    tile = _direct(d, ref, n, cin, cout, h, w, {}, (2, 1), capfd)
    assert (d["ho"], d["wo"]) == (13, 20) and tile["TW"] % 16 != 0 and d["ho"] % tile["R"] != 0, tile
    assert not _flag()


def test_k1_ragged_last_chunk_four_pairs(capfd):
    n, cin, cout, h, w = 2, 48, 128, 13, 24
    d = _operands(ACT, 3, n, cin, cout, h, w, 1, 1, False, True)
    ref = _reference(d, "act")
    _direct(d, ref, n, cin, cout, h, w, {"UDP_POSE_WS_PB": "6", "UDP_POSE_WS_CP": "4"}, (6, 4), capfd)
    assert not _flag()


def test_head_nchw_17_channels(capfd):
    n, cin, cout, h, w = 1, 32, 17, 7, 37
    d = _operands(WGT, 4, n, cin, cout, h, w, 1, 1, False, False)
    ref = _reference(d, "wgt")
    _direct(d, ref, n, cin, cout, h, w, {"UDP_POSE_WS_PB": "6", "UDP_POSE_WS_CP": "1"}, (6, 1), capfd, nchw=True)


@pytest.mark.parametrize("value,raises,kind,grid", [(65520.0, True, "act", ACT_EDGE), (65504.0, False, "wgt", WGT_EDGE)],
                         ids=["65520-raises", "65504-clear"])
def test_edge_of_fp16(value, raises, kind, grid, capfd):
    """One output element exactly at ``value``: x = 32736 at one pixel of input channel 0 (which nothing else reads),
    weight 2 on the centre tap, bias value - 65472; stored planes still encode(ref) -- hi = inf, lo = -inf at 65520."""
    n, c, h, w, c0 = 1, 32, 8, 8, 13
    d = _operands(grid, 5, n, c, c, h, w, 3, 1, False, True)
    d["x"][:, 0] = 0
    d["wt"][:, 0] = 0
    d["wt"][c0] = 0
    d["x"][0, 0, 5, 2], d["wt"][c0, 0, 1, 1], d["bias"][c0] = 32736.0, 2.0, value - 65472.0
    ref = _reference(d, kind)
    assert float(ref[0, c0, 5, 2]) == value and int((ref >= 65520.0).sum()) == int(raises)
    _flag(reset=True)
    _direct(d, ref, n, c, c, h, w, {}, (2, 1), capfd)
    assert _flag(reset=False) == raises
    assert _flag(reset=True) == raises and not _flag()


# ---------------------------------------------------------------- the merged launch and its members alone
MEMBERS = {          # name: (kind, grid, c, h, w, (PB, CP))
    "pb8": ("act", ACT, 32, 32, 16, (8, 1)),
    "c64": ("wgt", WGT, 64, 12, 8, (6, 2)),
}


@pytest.mark.parametrize("names", [("c64", "pb8"), ("pb8",), ("c64",)], ids=["merged", "pb8-alone", "c64-alone"])
def test_merged_launch_and_each_member_alone(names, capfd):
    n = 2
    m = Micro(H2, n, seed=11)
    cases = []
    for j, name in enumerate(names):
        kind, grid, c, h, w, arm = MEMBERS[name]
        d = _operands(grid, 20 + len(name) + c, n, c, c, h, w, 3, 1, True, True)
        ref = _reference(d, kind)
        bx, br, bo = m.buf(h, w, c), m.buf(h, w, c), m.buf(h, w, c)
        assert torch.equal(m.fill(bx, d["x"]), d["x"]) and torch.equal(m.fill(br, d["r"]), d["r"])
        m.add(new_op(_lib.UDP_OP_CONV, ks=3, stride=1, relu=1, cin=c, cout=c, hin=h, win=w, hout=h, wout=w, in_buf=bx, res_buf=br,
                     out_buf=bo, group=1, **m.put_conv(d["wt"], d["bias"], ws=True)))
        m.wrote(bo)
        cases.append((name, ref, bo, (h, w, c), arm))
    _flag(reset=True)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1"):
        assert m.run() == 0, m.error
    err = capfd.readouterr().err
    arms = {(int(g[2]), int(g[3]), int(g[4])): (int(g[10]), int(g[9])) for g in WS_LINE.findall(err) if g[0] == "3"}
    assert arms == {geo: arm for _, _, _, geo, arm in cases}, arms
    assert [int(v) for v in MULTI_LINE.findall(err)] == ([2] if len(names) == 2 else []), err
    for name, ref, bo, _, _ in cases:
        got, want = m.read_raw(bo), m.raw_of(ref)
        assert np.array_equal(got, want), "%s: %d stored units differ" % (name, int((got != want).sum()))
    m.assert_untouched()
    m.check_head()
    assert not _flag()


# ---------------------------------------------------------------- x0 share: side output + two stride-2 convs, one launch
def test_x0_share_set_with_side_output(capfd):
    n, h, w = 2, 16, 16
    ho, wo = h // 2, w // 2
    m = Micro(H2, n, in_h=4 * h, in_w=4 * w, seed=13)
    g = torch.Generator().manual_seed(31)
    d64 = _operands(ACT, 32, n, 32, 64, h, w, 3, 2, True, True)
    d32 = _operands(ACT, 33, n, 32, 32, h, w, 3, 2, False, True)
    d32["x"] = d64["x"]
    u1 = _ints(g, (n, 32, h // 2, w // 2), ACT["ximax"]) * ACT["xq"]
    refs = [_reference(d64, "act"), _reference(d32, "act")]
    side = F.relu(d64["x"].double() + F.interpolate(u1.double(), scale_factor=2, mode="nearest"))
    assert torch.equal(side.float().double(), side)
    bx, b0, bu = m.buf(h, w, 32), m.buf(h, w, 32), m.buf(h // 2, w // 2, 32)
    br, ba, bc = m.buf(ho, wo, 64), m.buf(ho, wo, 64), m.buf(ho, wo, 32)
    assert torch.equal(m.fill(bx, d64["x"]), d64["x"]) and torch.equal(m.fill(bu, u1), u1) and torch.equal(m.fill(br, d64["r"]), d64["r"])
    geo = dict(ks=3, stride=2, cin=32, hin=h, win=w, hout=ho, wout=wo, in_buf=bx, relu=1)
    m.add(new_op(_lib.UDP_OP_FUSE, relu=1, cin=32, cout=32, hin=h, win=w, hout=h, wout=w, in_buf=bx, out_buf=b0, n_up=1, up_buf=[bu],
                 up_shift=[1]))
    m.add(new_op(_lib.UDP_OP_CONV, cout=64, out_buf=ba, res_buf=br, **geo, **m.put_conv(d64["wt"], d64["bias"], ws=True)))
    m.add(new_op(_lib.UDP_OP_CONV, cout=32, out_buf=bc, **geo, **m.put_conv(d32["wt"], d32["bias"], ws=True)))
    for b in (b0, ba, bc):
        m.wrote(b)
    _flag(reset=True)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_NO_X0_SHARE="0"):
        assert m.run() == 0, m.error
    sets = [(int(s[0]), s[1], int(s[2])) for s in SHARE_LINE.findall(capfd.readouterr().err)]
    assert sets == [(3, "64,32", 1)], sets
    for name, b, ref in (("side", b0, side.float()), ("conv64", ba, refs[0]), ("conv32", bc, refs[1])):
        got, want = m.read_raw(b), m.raw_of(ref)
        assert np.array_equal(got, want), "%s: %d stored units differ" % (name, int((got != want).sum()))
    m.assert_untouched()
    m.check_head()
    assert not _flag()
