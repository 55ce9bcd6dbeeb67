"""What pose_mobilevit_pixel_shuffle adds to the op set, through udp_conv2d_fused (include/udp_pose_hip.h): UDP_OP_LNORM,
UDP_OP_MHATTN and UDP_OP_ACT; one micro-program runs the three kinds through the executor, eagerly and as a graph.

Outputs are pre-filled with NaN and operands are quantised to the storage mode first.  LNORM and MHATTN are gated by
|hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp relative to the tensor's max (microprog.parity; ulp = 2^-23 fp32, 2^-21 split
fp16), ACT by err_cpu_fp32 + 4 ulp."""
import ctypes as C

import numpy as np
import pytest
import torch

import microprog as mp
from mobilevit_ref import layer_norm_map, mha_core, silu
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21}
SILU = _lib.UDP_ACT_SILU
UNSUP, ARG = -3, -1
KEY_BLOCK = 32          # keys the attention kernel stages in LDS at a time (csrc/attn.hip, kMhaKB)


def _q(dtype):
    """Operands exactly as the device holds them (split fp16: 22-bit hi + lo pairs)."""
    return (lambda t: f16x2.decode(f16x2.encode(t))) if dtype == "f16x2" else (lambda t: t)


def _dev(t_nhwc, dtype):
    return (f16x2.encode(t_nhwc) if dtype == "f16x2" else t_nhwc.contiguous()).cuda()


def _nan(dtype, *shape):
    if dtype == "f16x2":
        return torch.full(shape[:-1] + (2, shape[-1]), float("nan"), dtype=torch.float16, device="cuda")
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _host(t, dtype):
    """device NHWC storage -> fp32 NHWC on the host"""
    return (f16x2.decode(t) if dtype == "f16x2" else t).cpu()


def _bits(t):
    """The stored bit patterns as [..., channel] (split fp16: [..., plane, channel])."""
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _call(op, dtype, n, x, w, b, out):
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), None, None, None, None,
                                     _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------ LayerNorm per pixel
def _ln_op(c, r, h, w):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_LNORM, 1, 1, 0
    op.cin, op.cout, op.cout_pad, op.chain_cout = c, c, c, r
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


def _ln_data(c, r, h, w, n, dtype):
    """Input mean 3, std 1: E[x^2] - E[x]^2 in fp32 loses what the variance is made of; zeros in the pad channels."""
    g = torch.Generator().manual_seed(c + 3 * r + 7 * h + n)
    x = torch.zeros(n, c, h, w)
    x[:, :r] = torch.randn(n, r, h, w, generator=g) + 3.0
    gam = torch.rand(r, generator=g) + 0.5
    bet = torch.randn(r, generator=g) * 0.5
    block = torch.zeros(2, c)
    block[0, :r], block[1, :r] = gam, bet
    return _q(dtype)(x), gam, bet, block.contiguous().cuda(), g


def _ln_ref(x, gam, bet, dt):
    r = gam.shape[0]
    return layer_norm_map(x[:, :r].to(dt), gam, bet)


LN_CR = [(32, 32), (64, 64), (96, 80), (160, 144), (256, 240)]
LN_HW = [(1, 1), (2, 2), (7, 5), (32, 24)]


def _ln_run(c, r, h, w, n, dtype, view=False, inplace=False):
    x, gam, bet, block, g = _ln_data(c, r, h, w, n, dtype)
    op = _ln_op(c, r, h, w)
    pitch, coff = (c + 96, 64) if view else (c, 0)
    if view:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = coff, pitch, coff, pitch
    xin = torch.randn(n, h, w, pitch, generator=g)                            # the channels outside the view are noise
    xin[..., coff:coff + c] = x.permute(0, 2, 3, 1)
    d_in = _dev(xin, dtype)
    out = d_in if inplace else _nan(dtype, n, h, w, pitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, d_in, block, None, out) == 0, _lib.lib().udp_last_error()
    return x, gam, bet, out, before, coff


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", LN_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cr", LN_CR, ids=lambda s: "C%d-r%d" % s)
def test_layer_norm_matches_fp64(cr, hw, n, dtype):
    (c, r), (h, w) = cr, hw
    x, gam, bet, out, _, _ = _ln_run(c, r, h, w, n, dtype)
    o = _host(out, dtype).permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("lnorm C%d(%d) %dx%d n%d %s" % (c, r, h, w, n, dtype), o[:, :r], _ln_ref(x, gam, bet, torch.float64),
                               _ln_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    if r < c:
        assert int(_bits(out)[..., r:].abs().max()) == 0                        # pad channels: exact zeros


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("cr", [(96, 80), (256, 240)], ids=lambda s: "C%d-r%d" % s)
def test_layer_norm_views_and_in_place(cr, dtype):
    """A view into a wider tensor leaves the rest of the tensor's bits alone; in place equals out of place, bit for bit."""
    (c, r), h, w, n = cr, 7, 5, 3
    x, gam, bet, out, before, coff = _ln_run(c, r, h, w, n, dtype, view=True)
    o = _host(out, dtype)[..., coff:coff + c].permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("lnorm view C%d(%d) %s" % (c, r, dtype), o[:, :r], _ln_ref(x, gam, bet, torch.float64),
                               _ln_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    ob = _bits(out)
    assert torch.equal(ob[..., :coff], before[..., :coff]) and torch.equal(ob[..., coff + c:], before[..., coff + c:])
    assert int(ob[..., coff + r:coff + c].abs().max()) == 0
    for view in (False, True):
        _, _, _, a, _, co = _ln_run(c, r, h, w, n, dtype, view=view)
        _, _, _, b, b_before, _ = _ln_run(c, r, h, w, n, dtype, view=view, inplace=True)
        bb = _bits(b)
        assert torch.equal(_bits(a)[..., co:co + c], bb[..., co:co + c])
        assert torch.equal(bb[..., :co], b_before[..., :co]) and torch.equal(bb[..., co + c:], b_before[..., co + c:])


# ------------------------------------------------------------------ multi-head attention core
def _mh_op(dp, d, heads, h, w):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_MHATTN, 2, 1, 0
    op.cin, op.cout, op.cout_pad, op.chain_cout = 3 * dp, dp, dp, d
    op.up_shift[0] = heads
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


def _mh_data(dp, d, h, w, n, dtype, qscale):
    g = torch.Generator().manual_seed(dp + 3 * d + 7 * h + n)
    qd = _q(dtype)
    q = qd(torch.randn(n, d, h, w, generator=g) * (0.5 * qscale))
    k = qd(torch.randn(n, d, h, w, generator=g))
    v = qd(torch.randn(n, d, h, w, generator=g) + 0.5)
    stored = torch.zeros(n, h, w, 3 * dp)                                       # q | k | v sections, zeros in the pads
    for s, t in enumerate((q, k, v)):
        stored[..., s * dp:s * dp + d] = t.permute(0, 2, 3, 1)
    return q, k, v, stored, g


def _mh_run(dp, d, heads, h, w, n, dtype, qscale=1.0, view=False):
    q, k, v, stored, g = _mh_data(dp, d, h, w, n, dtype, qscale)
    op = _mh_op(dp, d, heads, h, w)
    cin = 3 * dp
    ipitch, icoff, opitch, ocoff = (cin + 64, 32, dp + 96, 64) if view else (cin, 0, dp, 0)
    if view:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = icoff, ipitch, ocoff, opitch
    xin = torch.randn(n, h, w, ipitch, generator=g)
    xin[..., icoff:icoff + cin] = stored
    out = _nan(dtype, n, h, w, opitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, _dev(xin, dtype), None, None, out) == 0, _lib.lib().udp_last_error()
    return q, k, v, out, before, ocoff


MH_D = [(64, 64, 4), (96, 80, 4), (160, 144, 4), (256, 240, 4), (32, 32, 1)]
# 2x2: N = 1, out == v; 14x10: N = 35, a key block and 3 (not a multiple of anything); 32x24: N = 192, several waves of
# queries; 48x36: N = 432 -- K and V of one (class, head) no longer fit the LDS: reached only by walking key blocks
MH_HW = [(2, 2), (4, 2), (8, 6), (14, 10), (32, 24), (48, 36)]
WALKS_KEY_BLOCKS = (48, 36)
assert any((h * w // 4) > KEY_BLOCK and (h * w // 4) % KEY_BLOCK for h, w in MH_HW) and WALKS_KEY_BLOCKS in MH_HW


def _mh_check(name, q, k, v, got, d, heads, dtype):
    ref = lambda dt: mha_core(q.to(dt), k.to(dt), v.to(dt), heads)
    e_hip, _, gate = mp.parity(name, got[:, :d], ref(torch.float64), ref(torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", MH_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dh", MH_D, ids=lambda s: "dp%d-d%d-h%d" % s)
def test_multi_head_attention_matches_fp64(dh, hw, n, dtype):
    (dp, d, heads), (h, w) = dh, hw
    q, k, v, out, _, _ = _mh_run(dp, d, heads, h, w, n, dtype)
    got = _host(out, dtype).permute(0, 3, 1, 2)
    _mh_check("mhattn dp%d(%d) h%d %dx%d n%d %s" % (dp, d, heads, h, w, n, dtype), q, k, v, got, d, heads, dtype)
    if (h, w) == (2, 2):
        assert torch.equal(got[:, :d], v)                                       # one key: the soft-max is 1
    if d < dp:
        assert int(_bits(out)[..., d:].abs().max()) == 0                        # pad channels: exact zeros


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_multi_head_attention_large_scores_and_views(dtype):
    """q scaled x60: exp(s) overflows fp32 unless the row maximum is subtracted first.  Views: the rest of the output
    tensor keeps its bit pattern."""
    dp, d, heads, h, w, n = 96, 80, 4, 14, 10, 3
    q, k, v, out, _, _ = _mh_run(dp, d, heads, h, w, n, dtype, qscale=60.0)
    s = torch.einsum("nchw,ncij->nhwij", q[:, :20].double(), k[:, :20].double())
    assert float(s.abs().max()) > 100                                           # exp(100) is beyond fp32
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    _mh_check("mhattn q x60 %s" % dtype, q, k, v, got, d, heads, dtype)
    for dp, d in ((96, 80), (160, 144)):
        q, k, v, out, before, ocoff = _mh_run(dp, d, heads, 8, 6, n, dtype, view=True)
        _mh_check("mhattn views dp%d %s" % (dp, dtype), q, k, v, _host(out, dtype)[..., ocoff:ocoff + dp].permute(0, 3, 1, 2), d, heads, dtype)
        ob = _bits(out)
        assert torch.equal(ob[..., :ocoff], before[..., :ocoff]) and torch.equal(ob[..., ocoff + dp:], before[..., ocoff + dp:])
        assert int(ob[..., ocoff + d:ocoff + dp].abs().max()) == 0


# ------------------------------------------------------------------ the stand-alone activation
def _act_op(c, h, w, code=SILU):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_ACT, 1, 1, code
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("mode", ["plain", "inplace", "views"])
@pytest.mark.parametrize("c", [32, 160])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5), (16, 12)], ids=lambda s: "%dx%d" % s)
def test_act_silu(hw, c, mode, dtype):
    """Inputs ~ N(0, 3^2): both tails and the dip of SiLU."""
    (h, w), n = hw, 3
    g = torch.Generator().manual_seed(c + 7 * h)
    x = _q(dtype)(torch.randn(n, c, h, w, generator=g) * 3.0)
    op = _act_op(c, h, w)
    pitch, coff = (c + 96, 64) if mode == "views" else (c, 0)
    if mode == "views":
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = coff, pitch, coff, pitch
    xin = torch.randn(n, h, w, pitch, generator=g)
    xin[..., coff:coff + c] = x.permute(0, 2, 3, 1)
    d_in = _dev(xin, dtype)
    out = d_in if mode == "inplace" else _nan(dtype, n, h, w, pitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, d_in, None, None, out) == 0, _lib.lib().udp_last_error()
    got = _host(out, dtype)[..., coff:coff + c].permute(0, 3, 1, 2)
    e_hip, e_cpu, _ = mp.parity("act silu C%d %dx%d %s %s" % (c, h, w, mode, dtype), got, silu(x.double()), silu(x), ULP[dtype])
    assert e_hip <= e_cpu + 4 * ULP[dtype], (e_hip, e_cpu)
    ob = _bits(out)
    assert torch.equal(ob[..., :coff], before[..., :coff]) and torch.equal(ob[..., coff + c:], before[..., coff + c:])
    if mode == "plain":                                                         # hard-swish comes with the same kernel
        hs = _act_op(c, h, w, _lib.UDP_ACT_HSWISH)
        out = _nan(dtype, n, h, w, pitch)
        assert _call(hs, dtype, n, d_in, None, None, out) == 0, _lib.lib().udp_last_error()
        ref = lambda t: t * (torch.clamp(t + 3, 0, 6) / 6)
        e_hip, e_cpu, _ = mp.parity("act hswish C%d %dx%d %s" % (c, h, w, dtype), _host(out, dtype).permute(0, 3, 1, 2), ref(x.double()), ref(x), ULP[dtype])
        assert e_hip <= e_cpu + 4 * ULP[dtype], (e_hip, e_cpu)


# ------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_an_image_does_not_depend_on_its_batch(dtype):
    """Image 1 of a batch of 3 is bit-equal to the same image run alone (the sub-batch lanes split batches)."""
    c, r, h, w = 160, 144, 14, 10
    x, gam, bet, block, g = _ln_data(c, r, h, w, 3, dtype)
    d_in = _dev(x.permute(0, 2, 3, 1), dtype)
    out3, out1 = _nan(dtype, 3, h, w, c), _nan(dtype, 1, h, w, c)
    op = _ln_op(c, r, h, w)
    assert _call(op, dtype, 3, d_in, block, None, out3) == 0 and _call(op, dtype, 1, d_in[1:2].contiguous(), block, None, out1) == 0
    assert torch.equal(_bits(out3)[1:2], _bits(out1)) and not torch.isnan(_host(out1, dtype)).any()
    q, k, v, stored, g = _mh_data(c, r, h, w, 3, dtype, 1.0)
    d_in = _dev(stored, dtype)
    out3, out1 = _nan(dtype, 3, h, w, c), _nan(dtype, 1, h, w, c)
    op = _mh_op(c, r, 4, h, w)
    assert _call(op, dtype, 3, d_in, None, None, out3) == 0 and _call(op, dtype, 1, d_in[1:2].contiguous(), None, None, out1) == 0
    assert torch.equal(_bits(out3)[1:2], _bits(out1)) and not torch.isnan(_host(out1, dtype)).any()


# ------------------------------------------------------------------ the three kinds through the executor
def _replay(m):
    """The micro-program ``m`` (already run eagerly) once more as a graph replay: (workspace units, heat-maps)."""
    L = _lib.lib()
    h = m.create()
    try:
        ws = torch.from_numpy(m.before).cuda()
        x = m.x.cuda()
        heat = torch.full((m.B, 17, m.in_h // 4, m.in_w // 4), float("nan"), device="cuda")
        # ONE forward (it builds the graph and launches it): the activation runs in place, a second one would apply it twice
        rc = L.udp_hrnet_forward(h, _lib.ptr(x), m.n, int(m.flip), _lib.ptr(ws), ws.numel() * 2, _lib.ptr(heat), 1, _lib.stream_ptr())
        assert rc == 0, L.udp_last_error()
        torch.cuda.synchronize()
        return ws.cpu().numpy(), heat.cpu()
    finally:
        L.udp_hrnet_destroy(h)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_lnorm_mhattn_and_act_in_a_program(dtype):
    """udp_hrnet_create / udp_hrnet_forward: a layer norm (into a view of a wider tensor), an attention launch and an
    in-place activation between the stem and the head of a micro-program, with the flip-test half; nothing outside their
    outputs is touched, and the graph replay is bit-equal to the eager launches."""
    n, c, r, heads, h, w = 3, 64, 48, 4, 8, 8
    m = mp.Micro(dtype, n, 32, 32, flip=True, seed=77)
    B = m.B
    a, b = m.buf(h, w, c), m.buf(h, w, c + 32)
    xr = m.randn(B, c, h, w) + 3.0
    xr[:, r:] = 0
    x = m.fill(a, xr)
    gam, bet = torch.rand(r, generator=m.g) + 0.5, m.randn(r) * 0.5
    block = torch.zeros(2, c)
    block[0, :r], block[1, :r] = gam, bet
    m.add(mp.new_op(_lib.UDP_OP_LNORM, cin=c, cout=c, cout_pad=c, chain_cout=r, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=b,
                    out_coff=32, out_pitch=c + 32, w_off=m.put(block.numpy().tobytes())))
    m.wrote(b, 32, c)
    qkv, o = m.buf(h, w, 3 * c), m.buf(h, w, c)
    q, k, v = m.randn(B, c, h, w) * 0.5, m.randn(B, c, h, w), m.randn(B, c, h, w)
    q[:, r:], k[:, r:], v[:, r:] = 0, 0, 0
    st = m.fill(qkv, torch.cat([q, k, v], dim=1))
    at = mp.new_op(_lib.UDP_OP_MHATTN, ks=2, cin=3 * c, cout=c, cout_pad=c, chain_cout=r, hin=h, win=w, hout=h, wout=w, in_buf=qkv, out_buf=o)
    at.up_shift[0] = heads
    m.add(at)
    m.wrote(o)
    s = m.buf(h, w, c)
    xs = m.fill(s, m.randn(B, c, h, w) * 3.0)
    m.add(mp.new_op(_lib.UDP_OP_ACT, relu=SILU, cin=c, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w, in_buf=s, out_buf=s))
    m.wrote(s)
    assert m.run() == 0, m.error
    got = m.read(b, 32, c)
    e_hip, _, gate = mp.parity("program lnorm %s" % dtype, got[:, :r], _ln_ref(x, gam, bet, torch.float64), _ln_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate and float(got[:, r:].abs().max()) == 0.0
    _mh_check("program mhattn %s" % dtype, st[:, :r], st[:, c:c + r], st[:, 2 * c:2 * c + r], m.read(o), r, heads, dtype)
    assert float(m.read(o)[:, r:].abs().max()) == 0.0
    e_hip, e_cpu, _ = mp.parity("program act %s" % dtype, m.read(s), silu(xs.double()), silu(xs), ULP[dtype])
    assert e_hip <= e_cpu + 4 * ULP[dtype]
    m.assert_untouched()
    m.check_head()
    ws, heat = _replay(m)
    assert np.array_equal(ws, m.after) and torch.equal(heat.view(torch.int32), m.heat.view(torch.int32))


# ------------------------------------------------------------------ rejections
def test_rejections():
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    lib = _lib.lib()
    P = _lib.ptr

    def call(op, dtype=_lib.UDP_F32, res=None, out=None):
        rc = lib.udp_conv2d_fused(C.byref(op), dtype, 1, P(buf), P(buf[1 << 17:]), P(buf[1 << 18:]), res, None, None, None,
                                  P(buf[1 << 19:]) if out is None else out, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    # ---- UDP_OP_LNORM
    ln = _ln_op(64, 48, 8, 6)
    assert call(ln) == 0 and call(ln, _lib.UDP_F16X2) == 0 and call(ln, _lib.UDP_BF16) == UNSUP
    assert call(ln, out=P(buf)) == 0                                            # in place, same view
    for r in (0, 65, -1):
        assert call(_ln_op(64, r, 8, 6)) == ARG                                 # real channels outside 1 .. C
    assert call(_ln_op(48, 48, 8, 6)) == ARG and call(_ln_op(544, 544, 8, 6)) == ARG
    assert call(ln, res=P(buf[1 << 16:])) == ARG
    for code, rc in ((1, UNSUP), (2, UNSUP), (SILU, UNSUP), (3, ARG), (5, ARG)):
        ln.relu = code
        assert call(ln) == rc
    # ---- UDP_OP_MHATTN
    mh = _mh_op(64, 48, 4, 8, 6)
    assert call(mh) == 0 and call(mh, _lib.UDP_F16X2) == 0 and call(mh, _lib.UDP_BF16) == UNSUP
    for h, w in ((7, 6), (8, 5), (1, 1)):
        assert call(_mh_op(64, 48, 4, h, w)) == ARG                             # odd sizes
    for ks in (1, 3, 4):
        bad = _mh_op(64, 48, 4, 8, 6)
        bad.ks = ks
        assert call(bad) == ARG                                                 # the patch size
    bad = _mh_op(64, 48, 4, 8, 6)
    bad.cin = 2 * 64 + 32
    assert call(bad) == ARG                                                     # cin != 3 cout
    assert call(_mh_op(64, 50, 4, 8, 6)) == ARG                                 # d % heads
    assert call(_mh_op(64, 48, 0, 8, 6)) == ARG
    assert call(_mh_op(256, 240, 2, 8, 6)) == ARG                               # head width 120 > 64
    assert call(_mh_op(256, 256, 4, 8, 6)) == 0                                 # head width 64
    assert call(_mh_op(64, 0, 4, 8, 6)) == ARG and call(_mh_op(64, 68, 4, 8, 6)) == ARG
    assert call(_mh_op(288, 288, 8, 8, 6)) == ARG                               # dp > 256
    assert call(mh, out=P(buf)) == ARG                                          # out must not be in
    for code, rc in ((1, UNSUP), (SILU, UNSUP), (3, ARG)):
        mh.relu = code
        assert call(mh) == rc
    # ---- UDP_OP_ACT
    for dt in (_lib.UDP_F32, _lib.UDP_F16X2):
        assert call(_act_op(64, 8, 6), dt) == 0 and call(_act_op(64, 8, 6, _lib.UDP_ACT_HSWISH), dt) == 0
    assert call(_act_op(64, 8, 6), out=P(buf)) == 0                             # in place
    assert call(_act_op(64, 8, 6), _lib.UDP_BF16) == UNSUP
    for code in (0, 1, 3, 5):
        assert call(_act_op(64, 8, 6, code)) == ARG
    assert call(_act_op(48, 8, 6)) == ARG
    assert call(_act_op(64, 8, 6), res=P(buf[1 << 16:])) == ARG
    torch.cuda.synchronize()


def _program_rc(mutate):
    """udp_hrnet_create on a micro-program with a layer norm 64 -> 64 at H/4 (then altered)."""
    m = mp.Micro("f16x2", 1, 32, 32)
    a, b = m.buf(8, 8, 64), m.buf(8, 8, 64)
    m.fill(a, m.randn(1, 64, 8, 8))
    op = mp.new_op(_lib.UDP_OP_LNORM, cin=64, cout=64, cout_pad=64, chain_cout=64, hin=8, win=8, hout=8, wout=8, in_buf=a, out_buf=b,
                   w_off=m.put(torch.ones(128).numpy().tobytes()))
    mutate(m, op, a, b)
    m.add(op)
    try:
        h = m.create()
    except _lib.UdpPoseError as e:
        return e.code
    _lib.lib().udp_hrnet_destroy(h)
    return 0


def test_program_rejections():
    assert _program_rc(lambda m, op, a, b: None) == 0
    assert _program_rc(lambda m, op, a, b: setattr(op, "out_buf", a)) == 0                   # in place, same view
    assert _program_rc(lambda m, op, a, b: setattr(op, "relu", SILU)) == UNSUP
    assert _program_rc(lambda m, op, a, b: setattr(op, "chain_cout", 0)) == ARG
    assert _program_rc(lambda m, op, a, b: setattr(op, "res_buf", a)) == ARG
    assert _program_rc(lambda m, op, a, b: setattr(op, "w_off", 1 << 30)) == ARG

    def to_mhattn(in_place=False, **fields):
        def f(m, op, a, b):
            q = m.buf(8, 8, 192)
            m.fill(q, m.randn(1, 192, 8, 8))
            op.kind, op.ks, op.cin, op.chain_cout, op.in_buf, op.w_off = _lib.UDP_OP_MHATTN, 2, 192, 48, q, 0
            op.up_shift[0] = 4
            if in_place:
                op.out_buf = q
            for k, v in fields.items():
                setattr(op, k, v)
        return f
    assert _program_rc(to_mhattn()) == 0
    assert _program_rc(to_mhattn(True)) == ARG                                               # out must not be in
    assert _program_rc(to_mhattn(ks=3)) == ARG
    assert _program_rc(to_mhattn(chain_cout=50)) == ARG                                      # d % heads
    assert _program_rc(to_mhattn(hin=7, hout=7)) == ARG
    assert _program_rc(to_mhattn(relu=1)) == UNSUP

    def to_act(code, in_place=True):
        def f(m, op, a, b):
            op.kind, op.relu, op.chain_cout, op.w_off = _lib.UDP_OP_ACT, code, 0, 0
            if in_place:
                op.out_buf = a
        return f
    assert _program_rc(to_act(SILU)) == 0 and _program_rc(to_act(SILU, False)) == 0 and _program_rc(to_act(_lib.UDP_ACT_HSWISH)) == 0
    for code in (0, 1, 3, 5):
        assert _program_rc(to_act(code)) == ARG
