"""What pose_shufflenetv2_plus_pixel_shuffle adds to the op set, through udp_conv2d_fused (include/udp_pose_hip.h): the
5x5 / 7x7 forms of UDP_OP_DWCONV, the hard-swish activation code of the 1x1 conv and of the stem, and UDP_OP_SE.

Outputs are pre-filled with NaN and operands are quantised to the storage mode first.  New arithmetic is gated by
|hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp relative to the tensor's max (microprog.parity; ulp = 2^-23 fp32, 2^-21 split
fp16), the conv + hard-swish by 1.5 x the shipped conv gate of the pre-activation (the slope of hard-swish is at most
1.5), the passthrough by bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from shufflenet_plus_ref import hswish
from udp_pose_amd import _lib, f16x2
from udp_pose_amd.program import encode_weights

pytestmark = pytest.mark.gpu

ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21}
HS = _lib.UDP_ACT_HSWISH


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
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _call(op, dtype, n, x, w, b, out, res=None, up0=None):
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(res),
                                     _lib.ptr(up0), None, None, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------ depthwise 5x5 / 7x7
def _dw_op(c, h, w, ks, stride):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, ks, stride, 0
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, (h - 1) // stride + 1, (w - 1) // stride + 1
    return op


def _dw_data(c, h, w, ks, n, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = _q(dtype)(torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32)))
    wt = torch.from_numpy((rng.standard_normal((c, 1, ks, ks)) * np.sqrt(2.0 / (ks * ks))).astype(np.float32))    # fp32 in every mode
    bt = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32))
    return x, wt, bt, wt.reshape(c, ks * ks).t().contiguous().cuda()                                              # [ks * ks][C], tap-major


def _dw_ref(x, wt, bt, stride, dt):
    return F.conv2d(x.to(dt), wt.to(dt), bt.to(dt), stride=stride, padding=wt.shape[2] // 2, groups=x.shape[1])


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(2, 2), (4, 4), (7, 5), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", [32, 96, 224])
@pytest.mark.parametrize("ks", [5, 7])
def test_dwconv_k5_k7_matches_conv2d_fp64(ks, c, hw, stride, n, dtype):
    """At 2x2 and 4x4 most taps are clipped (skipped, not multiplied by zero)."""
    h, w = hw
    x, wt, bt, d_w = _dw_data(c, h, w, ks, n, dtype, c + 10 * h + stride + n + 100 * ks)
    op = _dw_op(c, h, w, ks, stride)
    out = _nan(dtype, n, op.hout, op.wout, c)
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), d_w, bt.cuda(), out) == 0, _lib.lib().udp_last_error()
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert tuple(got.shape) == (n, c, (h - 1) // stride + 1, (w - 1) // stride + 1)
    e_hip, _, gate = mp.parity("dwconv k%d C%d %dx%d s%d n%d %s" % (ks, c, h, w, stride, n, dtype), got,
                               _dw_ref(x, wt, bt, stride, torch.float64), _dw_ref(x, wt, bt, stride, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_k5_channel_views(stride, dtype):
    """64 channels from offset 32 of a 128-pitch input into offset 64 of a 128-pitch output; the rest of the output
    tensor keeps its bit pattern."""
    c, h, w, n = 64, 7, 5, 3
    x, wt, bt, d_w = _dw_data(128, h, w, 5, n, dtype, 177 + stride)
    wt, bt, d_w = wt[:c], bt[:c], d_w[:, :c].contiguous()
    op = _dw_op(c, h, w, 5, stride)
    op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = 32, 128, 64, 128
    out = _nan(dtype, n, op.hout, op.wout, 128)
    before = _bits(out).clone()
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), d_w, bt.cuda(), out) == 0, _lib.lib().udp_last_error()
    got = _host(out, dtype)[..., 64:128].permute(0, 3, 1, 2)
    xs = x[:, 32:96]
    e_hip, _, gate = mp.parity("dwconv k5 views s%d %s" % (stride, dtype), got, _dw_ref(xs, wt, bt, stride, torch.float64),
                               _dw_ref(xs, wt, bt, stride, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    assert torch.equal(_bits(out)[..., :64], before[..., :64])


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("c,r", [(64, 52), (32, 18)])
def test_dwconv_k5_shuffle_passthrough_is_a_selection(c, r, dtype):
    """n_out2 = 1 on the 5x5 kernel: the even logical channels of the unit input go to the first half of the unit output
    bit for bit, zeros in the pad, nothing else touched; the conv of the same launch is unchanged."""
    h, w, n = 7, 5, 3
    x, wt, bt, d_w = _dw_data(c, h, w, 5, n, dtype, 5 * c + r)
    rng = np.random.Generator(np.random.PCG64(r))
    src = _dev(torch.from_numpy(rng.standard_normal((n, h, w, 2 * c)).astype(np.float32)), dtype)     # pads non-zero on purpose
    dst = _nan(dtype, n, h, w, 2 * c)
    before = _bits(dst).clone()
    op = _dw_op(c, h, w, 5, 1)
    op.n_out2, op.chain_cout = 1, r
    op.res_pitch = 2 * c
    op.out2_coff[0], op.out2_pitch[0] = 0, 2 * c
    out = _nan(dtype, n, h, w, c)
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), d_w, bt.cuda(), out, res=src, up0=dst) == 0, _lib.lib().udp_last_error()
    pos = [j if j < r else c + j - r for j in range(2 * r)]
    sel = torch.tensor([pos[2 * k] for k in range(r)])
    s_bits, d_bits = _bits(src), _bits(dst)
    assert torch.equal(d_bits[..., :r], s_bits[..., sel])
    assert int(d_bits[..., r:c].abs().max()) == 0
    assert torch.equal(d_bits[..., c:], before[..., c:])
    got = _host(out, dtype).permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("dwconv k5 + passthrough C%d %s" % (c, dtype), got, _dw_ref(x, wt, bt, 1, torch.float64),
                               _dw_ref(x, wt, bt, 1, torch.float32), ULP[dtype])
    assert e_hip <= gate


# ------------------------------------------------------------------ 1x1 conv + hard-swish
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


def _pw_data(cin, cout, h, w, n, dtype):
    """x, weight, bias, the generator.  Pre-activations ~ N(0, 3^2): a good share beyond both knees of hard-swish; the
    weights are exact in fp16, so every layout holds the same numbers."""
    g = torch.Generator().manual_seed(cin + 3 * cout + 7 * h + n)
    x = _q(dtype)(torch.randn(n, cin, h, w, generator=g))
    wt = (torch.randn(cout, cin, 1, 1, generator=g) * (3.0 / np.sqrt(cin))).to(torch.float16).to(torch.float32)
    return x, wt, torch.randn(cout, generator=g) * 0.5, g


def _pw_case(cin, cout, h, w, n, dtype, wfmt, views):
    x, wt, bt, g = _pw_data(cin, cout, h, w, n, dtype)
    d_w, d_b, cp, wexp = _pw_weights(wt, bt, dtype, wfmt)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 1, 1, HS
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
    share = [float((pre < -3).double().mean()), float(((pre > -3) & (pre < 3)).double().mean()), float((pre > 3).double().mean())]
    assert min(share) > 0.08, share                                             # not the linear part alone
    got = _host(out, dtype)[..., ocoff:ocoff + cout].permute(0, 3, 1, 2)
    assert not torch.isnan(got).any()
    err = float((got.double() - hswish(pre)).abs().max())
    tol = 1.5 * mp.conv_tol(dtype, pre)
    print("1x1+hs C%d->%d %dx%d n%d %s wfmt%d views%d: err %.3g (gate %.3g), shares %s" % (cin, cout, h, w, n, dtype, wfmt, views, err, tol,
                                                                                          ["%.2f" % s for s in share]))
    assert err <= tol, (err, tol)
    if views:
        ob = _bits(out)
        assert torch.equal(ob[..., :ocoff], before[..., :ocoff]) and torch.equal(ob[..., ocoff + cout:], before[..., ocoff + cout:])


@pytest.mark.parametrize("views", [False, True], ids=["plain", "views"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%s-wfmt%d" % l)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cc", [(32, 32), (128, 224)], ids=lambda s: "%d-%d" % s)
def test_conv1x1_hard_swish(cc, hw, n, layout, views):
    _pw_case(cc[0], cc[1], hw[0], hw[1], n, layout[0], layout[1], views)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_conv1x1_hard_swish_with_maps(dtype):
    """in_map / out_map are the host's weight scatter (Program._pack): 20 real inputs picked from a 64-channel tensor, 18
    real outputs spread over a 64-channel layout; the untouched output positions come out as hswish(0) = 0."""
    from udp_pose_amd.program import Program
    n, h, w = 3, 7, 5
    g = torch.Generator().manual_seed(5)
    x = _q(dtype)(torch.randn(n, 64, h, w, generator=g))
    wt = (torch.randn(18, 20, 1, 1, generator=g) * (3.0 / np.sqrt(20))).to(torch.float16).to(torch.float32)
    bt = torch.randn(18, generator=g) * 0.5
    in_map, out_map = list(range(1, 41, 2)), [j if j < 9 else 32 + j - 9 for j in range(18)]
    prog = Program.__new__(Program)
    prog.dtype, prog._blob, prog._blob_size = dtype, [], 0
    w_off, b_off, cout, cin, ks, cp, wexp = prog._pack(wt, bt, dtype == "f16x2", out_map=out_map, in_map=in_map, cout_t=64, cin_t=64)
    blob = torch.from_numpy(prog.weight_blob()).cuda()
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 1, 1, HS
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cp, int(dtype == "f16x2"), wexp
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    out = _nan(dtype, n, h, w, 64)
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), blob[w_off:], blob[b_off:].view(torch.float32), out) == 0, _lib.lib().udp_last_error()
    pre = F.conv2d(x[:, in_map].double(), wt.double(), bt.double())
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert float((got[:, out_map].double() - hswish(pre)).abs().max()) <= 1.5 * mp.conv_tol(dtype, pre)
    rest = [c for c in range(64) if c not in out_map]
    assert float(got[:, rest].abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("variant", [("f32", {}), ("f16x2", {}), ("f16x2", {"UDP_POSE_STEM_VALU": "1"})], ids=["f32", "f16x2", "f16x2-valu"])
def test_stem_hard_swish_matches_fp64(variant, n, monkeypatch):
    """UDP_OP_STEM with activation code 2 in a micro-program (with the flip-test half); the gate is 1.5 x the parity gate
    of the pre-activation (3 x the CPU fp32 error + 4 ulp of its max)."""
    mode, env = variant
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = mp.Micro(mode, n, 32, 32, flip=True, seed=300 + n)
    m.ops[0].relu = HS
    assert m.run() == 0, m.error
    got = m.read(m.stem_buf)
    xx = torch.cat([m.x, torch.flip(m.x, [3])])
    pre = lambda d: mp.ref_conv(xx.to(d), m.stem_w, m.stem_b, stride=2)
    p64 = pre(torch.float64)
    assert float((p64 < -3).double().mean()) > 0.001 and float((p64 > 3).double().mean()) > 0.001 and float((p64.abs() < 3).double().mean()) > 0.5
    tol = 1.5 * (3 * float((pre(torch.float32).double() - p64).abs().max()) + 4 * mp.ULP[mode] * float(p64.abs().max()))
    assert not torch.isnan(got).any()
    err = float((got.double() - hswish(p64)).abs().max())
    print("stem+hs %s n%d: err %.3g (gate %.3g)" % (mode, n, err, tol))
    assert err <= tol, (err, tol)
    m.assert_untouched()
    m.check_head()


# ------------------------------------------------------------------ squeeze-and-excitation
def _se_data(cs, real, h, w, n, dtype):
    hid = real // 4
    g = torch.Generator().manual_seed(cs + 5 * h + n)
    x = torch.zeros(n, cs, h, w)
    x[:, :real] = torch.randn(n, real, h, w, generator=g) + 0.5 * torch.randn(1, real, 1, 1, generator=g)      # channel means differ
    x = _q(dtype)(x)
    w1 = torch.randn(hid, real, generator=g) * (2.0 / np.sqrt(real))
    b1 = torch.randn(hid, generator=g) * 0.3
    w2 = torch.randn(real, hid, generator=g) * (6.0 / np.sqrt(hid))           # W2 h spreads over both knees of the hard-sigmoid
    return x, w1, b1, w2, g


def _se_ref(x, w1, b1, w2, dt):
    real = w1.shape[1]
    xr = x[:, :real].to(dt)
    hdn = F.relu(xr.mean(dim=(2, 3)) @ w1.to(dt).t() + b1.to(dt))
    m = torch.clamp(hdn @ w2.to(dt).t() + 3, 0, 6) / 6
    return xr * m[:, :, None, None], m


def _se_case(cs, real, h, w, n, dtype, view, inplace):
    hid = real // 4
    x, w1, b1, w2, g = _se_data(cs, real, h, w, n, dtype)
    w1t = torch.zeros(cs, hid)
    w1t[:real] = w1.t()
    w2t = torch.zeros(hid, cs)
    w2t[:, :real] = w2.t()
    block = torch.cat([w1t.reshape(-1), b1, w2t.reshape(-1)]).contiguous().cuda()
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_SE, 1, 1, 0
    op.cin, op.cout, op.cout_pad, op.chain_cout = cs, cs, cs, hid
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    pitch, coff = (2 * cs, cs) if view else (cs, 0)
    if view:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = coff, pitch, coff, pitch
    xin = torch.randn(n, h, w, pitch, generator=g)
    xin[..., coff:coff + cs] = x.permute(0, 2, 3, 1)
    d_in = _dev(xin, dtype)
    out = d_in if inplace else _nan(dtype, n, h, w, pitch)
    before = _bits(out).clone()
    assert _call(op, dtype, n, d_in, block, None, out) == 0, _lib.lib().udp_last_error()
    r64, m64 = _se_ref(x, w1, b1, w2, torch.float64)
    if n * real >= 64:
        assert float((m64 == 0).double().mean()) > 0.05 and float((m64 == 1).double().mean()) > 0.05 and \
            float(((m64 > 0) & (m64 < 1)).double().mean()) > 0.2, "the gate must not sit on one branch of the hard-sigmoid"
    o = _host(out, dtype)[..., coff:coff + cs].permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("se C%d(%d) %dx%d n%d %s view%d inplace%d" % (cs, real, h, w, n, dtype, view, inplace), o[:, :real], r64,
                               _se_ref(x, w1, b1, w2, torch.float32)[0], ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    ob = _bits(out)
    assert int(ob[..., coff + real:coff + cs].abs().max()) == 0                 # pad channels: exact zeros (0 * 0.5)
    if view:
        assert torch.equal(ob[..., :coff], before[..., :coff])                  # the other half keeps its bit pattern


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (8, 6), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cs,real", [(32, 26), (128, 104), (224, 208)])
@pytest.mark.parametrize("form", ["plain", "view", "view-inplace", "inplace"])
def test_squeeze_excitation_matches_fp64(form, cs, real, hw, n, dtype):
    _se_case(cs, real, hw[0], hw[1], n, dtype, form.startswith("view"), form.endswith("inplace"))


# ------------------------------------------------------------------ rejections
def _conv_op(ks=1, stride=1, relu=HS, cin=32, cout=32, h=8, w=6):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, relu
    op.cin, op.cout, op.cout_pad = cin, cout, 32
    pad = ks // 2
    op.hin, op.win, op.hout, op.wout = h, w, (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
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
    UNSUP, ARG = -3, -1
    assert call(_conv_op()) == 0 and call(_conv_op(), _lib.UDP_F16X2) == 0       # the accepted form
    assert call(_conv_op(ks=3)) == UNSUP                                        # 3x3
    assert call(_conv_op(stride=2)) == UNSUP                                    # stride 2
    assert call(_conv_op(), _lib.UDP_BF16) == UNSUP                             # bf16
    assert call(_conv_op(), res=P(buf[1 << 16:])) == UNSUP                      # residual addend
    up = _conv_op()
    up.n_up, up.up_shift[0] = 1, 1
    assert call(up, up0=P(buf[1 << 16:])) == UNSUP                              # up-sampled addend
    head = _conv_op(cout=17)
    head.out_buf = _lib.UDP_BUF_OUTPUT
    assert call(head) == UNSUP                                                  # NCHW head
    ws = _conv_op()
    ws.wfmt = 1
    assert call(ws, _lib.UDP_F16X2) == 0
    ws3 = _conv_op(ks=3)
    ws3.wfmt = 1
    assert call(ws3, _lib.UDP_F16X2) == UNSUP
    fuse = _conv_op()
    fuse.kind = _lib.UDP_OP_FUSE
    assert call(fuse) == UNSUP                                                  # UDP_OP_FUSE
    dec = _conv_op()
    dec.kind, dec.ks, dec.stride, dec.hout, dec.wout = _lib.UDP_OP_DECONV, 4, 2, 16, 12
    assert call(dec) == UNSUP                                                   # UDP_OP_DECONV
    dw = _dw_op(32, 8, 6, 5, 1)
    assert call(dw) == 0
    dw.relu = HS
    assert call(dw) == UNSUP                                                    # UDP_OP_DWCONV
    se = _lib.ConvOp()
    se.kind, se.ks, se.stride, se.cin, se.cout, se.cout_pad, se.chain_cout = _lib.UDP_OP_SE, 1, 1, 32, 32, 32, 8
    se.hin, se.win, se.hout, se.wout = 8, 6, 8, 6
    assert call(se) == 0 and call(se, _lib.UDP_BF16) == UNSUP
    se.relu = HS
    assert call(se) == UNSUP
    # activation codes above 2, kernel sizes outside {3, 5, 7}
    assert call(_conv_op(relu=3)) == ARG and call(_conv_op(relu=-1)) == ARG
    bad = _dw_op(32, 8, 6, 5, 1)
    bad.relu = 3
    assert call(bad) == ARG
    for ks in (4, 9):
        assert call(_dw_op(32, 8, 6, ks, 1)) == ARG
    torch.cuda.synchronize()


def _program_rc(mutate):
    """udp_hrnet_create on a micro-program whose middle op (a plain 1x1 conv + hard-swish, 64 -> 64 at H/4) was altered."""
    m = mp.Micro("f16x2", 1, 32, 32)
    a, b = m.buf(8, 8, 64), m.buf(8, 8, 64)
    m.fill(a, m.randn(1, 64, 8, 8))
    wt = mp.quant(m.randn(64, 64, 1, 1) * 0.1, "f16x2")
    op = mp.new_op(_lib.UDP_OP_CONV, relu=HS, cin=64, cout=64, hin=8, win=8, hout=8, wout=8, in_buf=a, out_buf=b,
                   **m.put_conv(wt, m.randn(64) * 0.1, ws=True))
    mutate(m, op, a, b)
    m.add(op)
    try:
        h = m.create()
    except _lib.UdpPoseError as e:
        return e.code
    _lib.lib().udp_hrnet_destroy(h)
    return 0


def test_program_rejections():
    """The forms only udp_hrnet programs have: launch groups, chains, second outputs, UDP_OP_BLOCK."""
    assert _program_rc(lambda m, op, a, b: None) == 0
    assert _program_rc(lambda m, op, a, b: setattr(op, "group", 1)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "chain_cout", 64)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "n_out2", 1)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "res_buf", a)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "kind", _lib.UDP_OP_BLOCK)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "kind", _lib.UDP_OP_MAXPOOL)) == -3
    assert _program_rc(lambda m, op, a, b: setattr(op, "relu", 3)) == -1
