"""What pose_mobilevitv2_pixel_shuffle adds to the op set, through udp_conv2d_fused (include/udp_pose_hip.h): UDP_OP_GNORM,
UDP_OP_LINATTN and the SiLU activation code of the 1x1 conv, the stem and the depthwise conv; one micro-program runs the
two new kinds through the executor.

Outputs are pre-filled with NaN and operands are quantised to the storage mode first.  New arithmetic is gated by
|hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp relative to the tensor's max (microprog.parity; ulp = 2^-23 fp32, 2^-21 split
fp16), conv + SiLU by 1.1 x the shipped conv gate of the pre-activation (the slope of SiLU is below 1.1)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from mobilevitv2_ref import linear_attention_core, silu
from udp_pose_amd import _lib, f16x2
from udp_pose_amd.program import encode_weights

pytestmark = pytest.mark.gpu

ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21}
SILU = _lib.UDP_ACT_SILU
UNSUP, ARG = -3, -1


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


def _call(op, dtype, n, x, w, b, out, res=None, up0=None):
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(res),
                                     _lib.ptr(up0), None, None, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------ GroupNorm(1, C)
def _gn_op(c, r, h, w):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_GNORM, 1, 1, 0
    op.cin, op.cout, op.cout_pad, op.chain_cout = c, c, c, r
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


def _gn_data(c, r, h, w, n, dtype):
    """Input mean 3, std 1: E[x^2] - E[x]^2 in fp32 loses what the variance is made of; zeros in the pad channels."""
    g = torch.Generator().manual_seed(c + 3 * r + 7 * h + n)
    x = torch.zeros(n, c, h, w)
    x[:, :r] = torch.randn(n, r, h, w, generator=g) + 3.0
    gam = torch.rand(r, generator=g) + 0.5
    bet = torch.randn(r, generator=g) * 0.5
    block = torch.zeros(2, c)
    block[0, :r], block[1, :r] = gam, bet
    return _q(dtype)(x), gam, bet, block.contiguous().cuda(), g


def _gn_ref(x, gam, bet, dt):
    r = gam.shape[0]
    return F.group_norm(x[:, :r].to(dt), 1, gam.to(dt), bet.to(dt), 1e-5)


GN_CR = [(32, 32), (64, 64), (160, 144), (512, 512)]
GN_HW = [(1, 1), (2, 2), (4, 2), (8, 6), (32, 24)]


def _gn_run(c, r, h, w, n, dtype, view=False, inplace=False):
    x, gam, bet, block, g = _gn_data(c, r, h, w, n, dtype)
    op = _gn_op(c, r, h, w)
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
@pytest.mark.parametrize("hw", GN_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cr", GN_CR, ids=lambda s: "C%d-r%d" % s)
def test_group_norm_matches_fp64(cr, hw, n, dtype):
    (c, r), (h, w) = cr, hw
    x, gam, bet, out, _, _ = _gn_run(c, r, h, w, n, dtype)
    o = _host(out, dtype).permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("gnorm C%d(%d) %dx%d n%d %s" % (c, r, h, w, n, dtype), o[:, :r], _gn_ref(x, gam, bet, torch.float64),
                               _gn_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    if r < c:
        assert int(_bits(out)[..., r:].abs().max()) == 0                        # pad channels: exact zeros


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("cr", [(160, 144), (512, 512)], ids=lambda s: "C%d-r%d" % s)
def test_group_norm_views_and_in_place(cr, dtype):
    """A view into a wider tensor leaves the rest of the tensor's bits alone; in place equals out of place, bit for bit."""
    (c, r), h, w, n = cr, 8, 6, 3
    x, gam, bet, out, before, coff = _gn_run(c, r, h, w, n, dtype, view=True)
    o = _host(out, dtype)[..., coff:coff + c].permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("gnorm view C%d(%d) %s" % (c, r, dtype), o[:, :r], _gn_ref(x, gam, bet, torch.float64),
                               _gn_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    ob = _bits(out)
    assert torch.equal(ob[..., :coff], before[..., :coff]) and torch.equal(ob[..., coff + c:], before[..., coff + c:])
    if r < c:
        assert int(ob[..., coff + r:coff + c].abs().max()) == 0
    for view in (False, True):
        _, _, _, a, _, co = _gn_run(c, r, h, w, n, dtype, view=view)
        _, _, _, b, b_before, _ = _gn_run(c, r, h, w, n, dtype, view=view, inplace=True)
        bb = _bits(b)
        assert torch.equal(_bits(a)[..., co:co + c], bb[..., co:co + c])
        assert torch.equal(bb[..., :co], b_before[..., :co]) and torch.equal(bb[..., co + c:], b_before[..., co + c:])


# ------------------------------------------------------------------ separable self-attention core
def _la_op(c, h, w):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_LINATTN, 2, 1, 0
    op.cin, op.cout, op.cout_pad = 2 * c + 32, c, c
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


def _la_data(c, r, h, w, n, dtype, qscale):
    g = torch.Generator().manual_seed(c + 3 * r + 7 * h + n)
    q = torch.randn(n, 1, h, w, generator=g) * qscale
    k, v = torch.zeros(n, c, h, w), torch.zeros(n, c, h, w)
    k[:, :r] = torch.randn(n, r, h, w, generator=g) + 0.5
    v[:, :r] = torch.randn(n, r, h, w, generator=g)
    qd = _q(dtype)
    q, k, v = qd(q), qd(k), qd(v)
    stored = torch.zeros(n, h, w, 2 * c + 32)                                   # key | value | query, zeros behind it
    stored[..., :c], stored[..., c:2 * c], stored[..., 2 * c] = k.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), q[:, 0]
    return q, k, v, stored, g


def _la_run(c, r, h, w, n, dtype, qscale=1.0, view=False):
    q, k, v, stored, g = _la_data(c, r, h, w, n, dtype, qscale)
    op = _la_op(c, h, w)
    cin = 2 * c + 32
    ipitch, icoff, opitch, ocoff = (cin + 64, 32, c + 96, 64) if view else (cin, 0, c, 0)
    if view:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = icoff, ipitch, ocoff, opitch
    xin = torch.randn(n, h, w, ipitch, generator=g)
    xin[..., icoff:icoff + cin] = stored
    out = _nan(dtype, n, h, w, opitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, _dev(xin, dtype), None, None, out) == 0, _lib.lib().udp_last_error()
    return q, k, v, out, before, ocoff


LA_C = [(32, 32), (96, 96), (160, 144), (256, 256)]
LA_HW = [(2, 2), (4, 2), (8, 6), (32, 24)]


def _la_check(name, q, k, v, got, r, dtype):
    ref = lambda dt: linear_attention_core(q.to(dt), k[:, :r].to(dt), v[:, :r].to(dt))
    e_hip, _, gate = mp.parity(name, got[:, :r], ref(torch.float64), ref(torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", LA_HW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cr", LA_C, ids=lambda s: "C%d-r%d" % s)
def test_linear_attention_matches_fp64(cr, hw, n, dtype):
    """2x2 is one patch: the soft-max of one element."""
    (c, r), (h, w) = cr, hw
    q, k, v, out, _, _ = _la_run(c, r, h, w, n, dtype)
    _la_check("linattn C%d(%d) %dx%d n%d %s" % (c, r, h, w, n, dtype), q, k, v, _host(out, dtype).permute(0, 3, 1, 2), r, dtype)
    if r < c:
        assert int(_bits(out)[..., r:].abs().max()) == 0                        # k = v = 0 in the pad: exact zeros


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_linear_attention_large_queries_and_views(dtype):
    """q spread over +-100: exp(q) overflows fp32 unless the class maximum is subtracted first.  Views: the rest of the
    output tensor keeps its bit pattern."""
    c, r, h, w, n = 96, 96, 8, 6, 3
    q, k, v, out, _, _ = _la_run(c, r, h, w, n, dtype, qscale=60.0)
    assert float(q.abs().max()) > 100
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    _la_check("linattn q x60 %s" % dtype, q, k, v, got, r, dtype)
    for c, r in ((96, 96), (160, 144)):
        q, k, v, out, before, ocoff = _la_run(c, r, h, w, n, dtype, view=True)
        _la_check("linattn views C%d %s" % (c, dtype), q, k, v, _host(out, dtype)[..., ocoff:ocoff + c].permute(0, 3, 1, 2), r, dtype)
        ob = _bits(out)
        assert torch.equal(ob[..., :ocoff], before[..., :ocoff]) and torch.equal(ob[..., ocoff + c:], before[..., ocoff + c:])
        if r < c:
            assert int(ob[..., ocoff + r:ocoff + c].abs().max()) == 0


# ------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_an_image_does_not_depend_on_its_batch(dtype):
    """Image 1 of a batch of 3 is bit-equal to the same image run alone (the sub-batch lanes split batches)."""
    c, r, h, w = 160, 144, 8, 6
    x, gam, bet, block, g = _gn_data(c, r, h, w, 3, dtype)
    d_in = _dev(x.permute(0, 2, 3, 1), dtype)
    out3, out1 = _nan(dtype, 3, h, w, c), _nan(dtype, 1, h, w, c)
    op = _gn_op(c, r, h, w)
    assert _call(op, dtype, 3, d_in, block, None, out3) == 0 and _call(op, dtype, 1, d_in[1:2].contiguous(), block, None, out1) == 0
    assert torch.equal(_bits(out3)[1:2], _bits(out1)) and not torch.isnan(_host(out1, dtype)).any()
    q, k, v, stored, g = _la_data(c, r, h, w, 3, dtype, 1.0)
    d_in = _dev(stored, dtype)
    out3, out1 = _nan(dtype, 3, h, w, c), _nan(dtype, 1, h, w, c)
    op = _la_op(c, h, w)
    assert _call(op, dtype, 3, d_in, None, None, out3) == 0 and _call(op, dtype, 1, d_in[1:2].contiguous(), None, None, out1) == 0
    assert torch.equal(_bits(out3)[1:2], _bits(out1)) and not torch.isnan(_host(out1, dtype)).any()


# ------------------------------------------------------------------ SiLU
LAYOUTS = [("f32", 0), ("f16x2", 1), ("f16x2", 0)]       # (storage mode, wfmt): what the planner emits (f16x2, wfmt 0: UDP_POSE_WS=0)


def _pw_weights(wt, bt, dtype, wfmt):
    cout, cin = wt.shape[:2]
    cp = mp.round_up(cout, 32)
    wp = torch.zeros(1, cp, cin, dtype=torch.float32)
    wp[0, :cout] = wt.reshape(cout, cin)
    bp = torch.zeros(cp, dtype=torch.float32)
    bp[:cout] = bt
    wexp = 0
    if wfmt:
        packed, wexp = f16x2.pack_weights_ws(wp)
        raw = packed.numpy().tobytes()
    else:
        raw = encode_weights(wp, dtype)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda(), bp.cuda(), cp, wexp


@pytest.mark.parametrize("views", [False, True], ids=["plain", "views"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%s-wfmt%d" % l)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cc", [(32, 32), (128, 224)], ids=lambda s: "%d-%d" % s)
def test_conv1x1_silu(cc, hw, n, layout, views):
    """Pre-activations ~ N(0, 3^2): both tails and the dip of SiLU; the weights are exact in fp16, so every layout holds
    the same numbers."""
    (cin, cout), (h, w), (dtype, wfmt) = cc, hw, layout
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * h + n)
    x = _q(dtype)(torch.randn(n, cin, h, w, generator=g))
    wt = (torch.randn(cout, cin, 1, 1, generator=g) * (3.0 / np.sqrt(cin))).to(torch.float16).to(torch.float32)
    bt = torch.randn(cout, generator=g) * 0.5
    d_w, d_b, cp, wexp = _pw_weights(wt, bt, dtype, wfmt)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 1, 1, SILU
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cp, wfmt, wexp
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    ipitch, icoff, opitch, ocoff = (cin + 64, 32, cout + 96, 64) if views else (cin, 0, cout, 0)
    if views:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = icoff, ipitch, ocoff, opitch
    xin = torch.randn(n, h, w, ipitch, generator=g)                            # the channels outside the view are noise
    xin[..., icoff:icoff + cin] = x.permute(0, 2, 3, 1)
    out = _nan(dtype, n, h, w, opitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, _dev(xin, dtype), d_w, d_b, out) == 0, _lib.lib().udp_last_error()
    pre = F.conv2d(x.double(), wt.double(), bt.double())
    assert float((pre < -2).double().mean()) > 0.1 and float((pre > 2).double().mean()) > 0.1
    got = _host(out, dtype)[..., ocoff:ocoff + cout].permute(0, 3, 1, 2)
    assert not torch.isnan(got).any()
    err = float((got.double() - silu(pre)).abs().max())
    tol = 1.1 * mp.conv_tol(dtype, pre)
    print("1x1+silu C%d->%d %dx%d n%d %s wfmt%d views%d: err %.3g (gate %.3g)" % (cin, cout, h, w, n, dtype, wfmt, views, err, tol))
    assert err <= tol, (err, tol)
    if views:
        ob = _bits(out)
        assert torch.equal(ob[..., :ocoff], before[..., :ocoff]) and torch.equal(ob[..., ocoff + cout:], before[..., ocoff + cout:])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("variant", [("f32", {}), ("f16x2", {}), ("f16x2", {"UDP_POSE_STEM_VALU": "1"})], ids=["f32", "f16x2", "f16x2-valu"])
def test_stem_silu_matches_fp64(variant, n, monkeypatch):
    """UDP_OP_STEM with activation code 4 in a micro-program (with the flip-test half)."""
    mode, env = variant
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = mp.Micro(mode, n, 32, 32, flip=True, seed=400 + n)
    m.ops[0].relu = SILU
    assert m.run() == 0, m.error
    got = m.read(m.stem_buf)
    xx = torch.cat([m.x, torch.flip(m.x, [3])])
    p64 = mp.ref_conv(xx.double(), m.stem_w, m.stem_b, stride=2)
    assert not torch.isnan(got).any()
    err = float((got.double() - silu(p64)).abs().max())
    tol = 1.1 * mp.conv_tol(mode, p64)
    print("stem+silu %s n%d: err %.3g (gate %.3g)" % (mode, n, err, tol))
    assert err <= tol, (err, tol)
    m.assert_untouched()
    m.check_head()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_silu(ks, hw, stride, n, dtype):
    """Depthwise 3x3 (and one K > 3 form) + SiLU; pad channels (zero weights and bias) stay exact zeros."""
    c, r, (h, w) = 96, 80, hw
    rng = np.random.Generator(np.random.PCG64(10 * h + stride + n + 100 * ks))
    x = torch.zeros(n, c, h, w)
    x[:, :r] = torch.from_numpy(rng.standard_normal((n, r, h, w)).astype(np.float32))
    x = _q(dtype)(x)
    wt, bt = torch.zeros(c, 1, ks, ks), torch.zeros(c)
    wt[:r] = torch.from_numpy((rng.standard_normal((r, 1, ks, ks)) * 3.0 / ks).astype(np.float32))
    bt[:r] = torch.from_numpy((rng.standard_normal(r) * 0.5).astype(np.float32))
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, ks, stride, SILU
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, (h - 1) // stride + 1, (w - 1) // stride + 1
    out = _nan(dtype, n, op.hout, op.wout, c)
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), wt.reshape(c, ks * ks).t().contiguous().cuda(), bt.cuda(), out) == 0, \
        _lib.lib().udp_last_error()
    pre = F.conv2d(x.double(), wt.double(), bt.double(), stride=stride, padding=ks // 2, groups=c)
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert not torch.isnan(got).any()
    err = float((got.double() - silu(pre)).abs().max())
    tol = 1.1 * mp.conv_tol(dtype, pre)
    print("dw%d+silu %dx%d s%d n%d %s: err %.3g (gate %.3g)" % (ks, h, w, stride, n, dtype, err, tol))
    assert err <= tol, (err, tol)
    assert int(_bits(out)[..., r:].abs().max()) == 0


# ------------------------------------------------------------------ the two kinds through the executor
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_gnorm_and_linattn_in_a_program(dtype):
    """udp_hrnet_create / udp_hrnet_forward: a group norm (into a view of a wider tensor) and an attention launch between
    the stem and the head of a micro-program, with the flip-test half; nothing outside their outputs is touched."""
    n, c, r, h, w = 3, 64, 48, 8, 8
    m = mp.Micro(dtype, n, 32, 32, flip=True, seed=77)
    B = m.B
    a, b = m.buf(h, w, c), m.buf(h, w, c + 32)
    xr = m.randn(B, c, h, w) + 3.0
    xr[:, r:] = 0
    x = m.fill(a, xr)
    gam, bet = torch.rand(r, generator=m.g) + 0.5, m.randn(r) * 0.5
    block = torch.zeros(2, c)
    block[0, :r], block[1, :r] = gam, bet
    m.add(mp.new_op(_lib.UDP_OP_GNORM, cin=c, cout=c, cout_pad=c, chain_cout=r, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=b,
                    out_coff=32, out_pitch=c + 32, w_off=m.put(block.numpy().tobytes())))
    m.wrote(b, 32, c)
    qkv, o = m.buf(h, w, 2 * c + 32), m.buf(h, w, c)
    q, k, v = m.randn(B, 1, h, w), m.randn(B, c, h, w), m.randn(B, c, h, w)
    k[:, r:], v[:, r:] = 0, 0
    st = m.fill(qkv, torch.cat([k, v, q, torch.zeros(B, 31, h, w)], dim=1))
    m.add(mp.new_op(_lib.UDP_OP_LINATTN, ks=2, cin=2 * c + 32, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w, in_buf=qkv, out_buf=o))
    m.wrote(o)
    assert m.run() == 0, m.error
    got = m.read(b, 32, c)
    e_hip, _, gate = mp.parity("program gnorm %s" % dtype, got[:, :r], _gn_ref(x, gam, bet, torch.float64), _gn_ref(x, gam, bet, torch.float32), ULP[dtype])
    assert e_hip <= gate and float(got[:, r:].abs().max()) == 0.0
    _la_check("program linattn %s" % dtype, st[:, 2 * c:2 * c + 1], st[:, :c], st[:, c:2 * c], m.read(o), r, dtype)
    m.assert_untouched()
    m.check_head()


# ------------------------------------------------------------------ rejections
def _conv_op(ks=1, stride=1, relu=SILU, cin=32, cout=32, h=8, w=6):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, relu
    op.cin, op.cout, op.cout_pad = cin, cout, 32
    pad = ks // 2
    op.hin, op.win, op.hout, op.wout = h, w, (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    return op


def _dw_op(c, h, w, ks, stride, relu=0):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, ks, stride, relu
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, (h - 1) // stride + 1, (w - 1) // stride + 1
    return op


def test_rejections():
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    lib = _lib.lib()
    P = _lib.ptr

    def call(op, dtype=_lib.UDP_F32, res=None, up0=None):
        rc = lib.udp_conv2d_fused(C.byref(op), dtype, 1, P(buf), P(buf[1 << 17:]), P(buf[1 << 18:]), res, up0, None, None,
                                  P(buf[1 << 19:]), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    # ---- activation code 4: the forms that take it ...
    assert call(_conv_op()) == 0 and call(_conv_op(), _lib.UDP_F16X2) == 0
    ws = _conv_op()
    ws.wfmt = 1
    assert call(ws, _lib.UDP_F16X2) == 0
    for ks in (3, 5, 7):
        for stride in (1, 2):
            assert call(_dw_op(32, 8, 6, ks, stride, SILU)) == 0 and call(_dw_op(32, 8, 6, ks, stride, SILU), _lib.UDP_F16X2) == 0
    # ---- ... and the ones that do not
    assert call(_conv_op(ks=3)) == UNSUP                                        # 3x3
    assert call(_conv_op(stride=2)) == UNSUP                                    # stride 2
    assert call(_conv_op(), _lib.UDP_BF16) == UNSUP                             # bf16
    assert call(_dw_op(32, 8, 6, 3, 1, SILU), _lib.UDP_BF16) == UNSUP
    assert call(_conv_op(), res=P(buf[1 << 16:])) == UNSUP                      # residual addend
    up = _conv_op()
    up.n_up, up.up_shift[0] = 1, 1
    assert call(up, up0=P(buf[1 << 16:])) == UNSUP                              # up-sampled addend
    head = _conv_op(cout=17)
    head.out_buf = _lib.UDP_BUF_OUTPUT
    assert call(head) == UNSUP                                                  # NCHW head
    ws3 = _conv_op(ks=3)
    ws3.wfmt = 1
    assert call(ws3, _lib.UDP_F16X2) == UNSUP
    fuse = _conv_op()
    fuse.kind = _lib.UDP_OP_FUSE
    assert call(fuse) == UNSUP                                                  # UDP_OP_FUSE
    dec = _conv_op()
    dec.kind, dec.ks, dec.stride, dec.hout, dec.wout = _lib.UDP_OP_DECONV, 4, 2, 16, 12
    assert call(dec) == UNSUP                                                   # UDP_OP_DECONV
    se = _lib.ConvOp()
    se.kind, se.ks, se.stride, se.cin, se.cout, se.cout_pad, se.chain_cout = _lib.UDP_OP_SE, 1, 1, 32, 32, 32, 8
    se.hin, se.win, se.hout, se.wout = 8, 6, 8, 6
    se.relu = SILU
    assert call(se) == UNSUP                                                    # UDP_OP_SE
    ps = _lib.ConvOp()
    ps.kind, ps.ks, ps.stride, ps.cin, ps.cout, ps.cout_pad = _lib.UDP_OP_PIXSHUF, 1, 1, 128, 32, 32
    ps.hin, ps.win, ps.hout, ps.wout = 8, 6, 16, 12
    assert call(ps) == 0
    ps.relu = SILU
    assert call(ps) == UNSUP                                                    # UDP_OP_PIXSHUF
    # ---- codes 2 and 3 stay where they were; codes outside 0..4
    assert call(_dw_op(32, 8, 6, 3, 1, _lib.UDP_ACT_HSWISH)) == UNSUP
    assert call(_conv_op(relu=3)) == ARG and call(_dw_op(32, 8, 6, 3, 1, 3)) == ARG
    assert call(_conv_op(relu=5)) == ARG and call(_dw_op(32, 8, 6, 3, 1, 5)) == ARG and call(_conv_op(relu=-1)) == ARG
    # ---- UDP_OP_GNORM
    gn = _gn_op(64, 48, 8, 6)
    assert call(gn) == 0 and call(gn, _lib.UDP_F16X2) == 0 and call(gn, _lib.UDP_BF16) == UNSUP
    for r in (0, 65, -1):
        assert call(_gn_op(64, r, 8, 6)) == ARG                                 # real channels outside 1 .. C
    assert call(_gn_op(48, 48, 8, 6)) == ARG and call(_gn_op(544, 544, 8, 6)) == ARG
    gn.relu = SILU
    assert call(gn) == UNSUP
    gn.relu = 1
    assert call(gn) == UNSUP
    gn.relu = 3
    assert call(gn) == ARG
    # ---- UDP_OP_LINATTN
    la = _la_op(64, 8, 6)
    assert call(la) == 0 and call(la, _lib.UDP_F16X2) == 0 and call(la, _lib.UDP_BF16) == UNSUP
    for h, w in ((7, 6), (8, 5), (1, 1)):
        assert call(_la_op(64, h, w)) == ARG                                    # odd sizes
    for ks in (1, 3, 4):
        bad = _la_op(64, 8, 6)
        bad.ks = ks
        assert call(bad) == ARG                                                 # the patch size
    bad = _la_op(64, 8, 6)
    bad.cin = 2 * 64
    assert call(bad) == ARG
    la.relu = SILU
    assert call(la) == UNSUP
    torch.cuda.synchronize()


def _program_rc(mutate):
    """udp_hrnet_create on a micro-program with a group norm 64 -> 64 at H/4 (then altered)."""
    m = mp.Micro("f16x2", 1, 32, 32)
    a, b = m.buf(8, 8, 64), m.buf(8, 8, 64)
    m.fill(a, m.randn(1, 64, 8, 8))
    op = mp.new_op(_lib.UDP_OP_GNORM, cin=64, cout=64, cout_pad=64, chain_cout=64, hin=8, win=8, hout=8, wout=8, in_buf=a, out_buf=b,
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

    def to_linattn(in_place):
        def f(m, op, a, b):
            q = m.buf(8, 8, 160)
            m.fill(q, m.randn(1, 160, 8, 8))
            op.kind, op.ks, op.cin, op.chain_cout, op.in_buf, op.w_off = _lib.UDP_OP_LINATTN, 2, 160, 0, q, 0
            if in_place:
                op.out_buf = q
        return f
    assert _program_rc(to_linattn(False)) == 0
    assert _program_rc(to_linattn(True)) == ARG                                              # out must not be in
