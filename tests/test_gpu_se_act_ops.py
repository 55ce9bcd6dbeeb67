"""UDP_OP_SE_ACT (kind 23; include/udp_pose_hip.h): the activation + squeeze-and-excitation with both biases of a
MobileNetV3 InvertedResidual, through udp_conv2d_fused and through micro-programs (tests/microprog.py, workspace
poisoned), in f32 and f16x2 against an fp64 evaluation of the header's formula; and the project conv's form (a 1x1
UDP_OP_CONV with ``res`` and no activation, 96 -> 40 real channels).

Operands are quantised to the storage mode first.  The gate is the project's op rule (DESIGN section 5,
microprog.parity): |hip - ref64| <= 3 x the error of a CPU fp32 evaluation of the same formula + 4 ulp, relative to
the tensor's max (ulp = 2^-23 fp32, 2^-21 split fp16)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21}
KIND = _lib.UDP_OP_SE_ACT
UNSUP, ARG = -3, -1
# (stored C, real r, hidden Ch, h, w): the smallest shapes that reach each branch of se_act_kernel
SHAPES = [(32, 16, 8, 1, 1),        # one pixel, pad channels
          (32, 16, 8, 3, 5),        # fewer pixels than pixel groups (P = 32 fp32 / 64 split fp16 > 15)
          (96, 96, 24, 17, 19),     # a pixel-stride loop with a ragged tail (323 pixels over 10 / 21 groups)
          (256, 240, 64, 4, 3),     # pad channels behind 240 real ones
          (576, 576, 144, 2, 3),    # more than 128 channel groups (144 in fp32: one pixel group)
          (1024, 1024, 256, 1, 2)]  # both limits
IDS = ["C%d-r%d-Ch%d-%dx%d" % s for s in SHAPES]


def _q(dtype):
    return (lambda t: f16x2.decode(f16x2.encode(t))) if dtype == "f16x2" else (lambda t: t)


def _dev(t_nhwc, dtype):
    return (f16x2.encode(t_nhwc) if dtype == "f16x2" else t_nhwc.contiguous()).cuda()


def _nan(dtype, *shape):
    if dtype == "f16x2":
        return torch.full(shape[:-1] + (2, shape[-1]), float("nan"), dtype=torch.float16, device="cuda")
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _host(t, dtype):
    return (f16x2.decode(t) if dtype == "f16x2" else t).cpu()


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _call(op, dtype, n, x, w, out, res=None, up0=None, b=None):
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(res),
                                     _lib.ptr(up0), None, None, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def act(x, code):
    if code == 1:
        return F.relu(x)
    if code == 2:
        return x * (torch.clamp(x + 3, 0, 6) / 6)
    return x


def se_act_ref(x, P, code, dt):
    """The header's formula on the r real channels, in ``dt``: (out, m)."""
    w1, b1, w2, b2 = (t.to(dt) for t in P)
    a = act(x[:, :w1.shape[1]].to(dt), code)
    hdn = F.relu(a.mean(dim=(2, 3)) @ w1.t() + b1)
    m = torch.clamp(hdn @ w2.t() + b2 + 3, 0, 6) / 6
    return a * m[:, :, None, None], m


def _data(cs, real, hid, h, w, n, dtype, seed, scale=2.0):
    """x ~ N(0, scale^2) + per-channel offsets (both knees of hard-swish are crossed, channel means differ), pad
    channels zero; W2 and b2 spread the gate over both knees of the hard-sigmoid."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, cs, h, w)
    x[:, :real] = scale * torch.randn(n, real, h, w, generator=g) + torch.randn(1, real, 1, 1, generator=g)
    x = _q(dtype)(x)
    w1 = torch.randn(hid, real, generator=g) * (2.0 / np.sqrt(real))
    b1 = torch.randn(hid, generator=g) * 0.3
    w2 = torch.randn(real, hid, generator=g) * (4.0 / np.sqrt(hid))
    b2 = torch.randn(real, generator=g) * 1.5
    return x, (w1, b1, w2, b2), g


def block_of(P, cs):
    """W1 transposed [C][Ch], b1 [Ch], W2 transposed [Ch][C], b2 [C]: zeros at the pad channels."""
    w1, b1, w2, b2 = P
    hid, real = w1.shape
    w1t = torch.zeros(cs, hid)
    w1t[:real] = w1.t()
    w2t = torch.zeros(hid, cs)
    w2t[:, :real] = w2.t()
    b2p = torch.zeros(cs)
    b2p[:real] = b2
    return torch.cat([w1t.reshape(-1), b1, w2t.reshape(-1), b2p]).contiguous()


def _op(cs, hid, h, w, code):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = KIND, 1, 1, code
    op.cin, op.cout, op.cout_pad, op.chain_cout = cs, cs, cs, hid
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    return op


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_se_act_matches_fp64(shape, code, dtype):
    """Out of place with n = 3 against fp64; in place bit-equal to it; n = 1 bit-equal to image 0 of n = 3; pad
    channels exact zeros."""
    cs, real, hid, h, w = shape
    n = 3
    x, P, _ = _data(cs, real, hid, h, w, n, dtype, 7 * cs + 3 * h + w + code)
    block = block_of(P, cs).cuda()
    op = _op(cs, hid, h, w, code)
    d_in = _dev(x.permute(0, 2, 3, 1), dtype)
    out = _nan(dtype, n, h, w, cs)
    assert _call(op, dtype, n, d_in, block, out) == 0, _lib.lib().udp_last_error()
    r64, m64 = se_act_ref(x, P, code, torch.float64)
    if n * real >= 256:
        assert float((m64 == 0).double().mean()) > 0.02 and float((m64 == 1).double().mean()) > 0.02 and \
            float(((m64 > 0) & (m64 < 1)).double().mean()) > 0.2, "the gate must not sit on one branch of the hard-sigmoid"
    o = _host(out, dtype).permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("se_act C%d(%d) Ch%d %dx%d code%d %s" % (cs, real, hid, h, w, code, dtype), o[:, :real], r64,
                               se_act_ref(x, P, code, torch.float32)[0], ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    ob = _bits(out)
    if real < cs:
        assert int(ob[..., real:].abs().max()) == 0                             # pad channels: act(0) * 0.5 = exact zeros
    inplace = d_in.clone()
    assert _call(op, dtype, n, inplace, block, inplace) == 0, _lib.lib().udp_last_error()
    assert torch.equal(_bits(inplace), ob)                                      # in place == out of place, bit for bit
    one = _nan(dtype, 1, h, w, cs)
    assert _call(op, dtype, 1, d_in[:1].contiguous(), block, one) == 0, _lib.lib().udp_last_error()
    assert torch.equal(_bits(one)[0], ob[0])                                    # image 0 does not depend on its batch


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("inplace", [False, True], ids=["plain", "inplace"])
def test_se_act_channel_views(inplace, dtype):
    """C = 32 at coff 32 inside pitch 64: the neighbouring channels keep their bits."""
    cs, real, hid, h, w, n, code = 32, 16, 8, 3, 5, 3, 2
    x, P, g = _data(cs, real, hid, h, w, n, dtype, 99)
    op = _op(cs, hid, h, w, code)
    op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = 32, 64, 32, 64
    xin = torch.randn(n, h, w, 64, generator=g)
    xin[..., 32:] = x.permute(0, 2, 3, 1)
    d_in = _dev(xin, dtype)
    out = d_in if inplace else _nan(dtype, n, h, w, 64)
    before = _bits(out).clone()
    assert _call(op, dtype, n, d_in, block_of(P, cs).cuda(), out) == 0, _lib.lib().udp_last_error()
    o = _host(out, dtype)[..., 32:].permute(0, 3, 1, 2)
    e_hip, _, gate = mp.parity("se_act view inplace%d %s" % (inplace, dtype), o[:, :real], se_act_ref(x, P, code, torch.float64)[0],
                               se_act_ref(x, P, code, torch.float32)[0], ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    ob = _bits(out)
    assert torch.equal(ob[..., :32], before[..., :32])
    assert int(ob[..., 32 + real:].abs().max()) == 0


def _micro(dtype, shape, code, n=3, coff=0, pitch=None, mutate=None, short=0):
    """The op in place on a pre-filled buffer of a micro-program; returns (Micro, buffer, x, P)."""
    cs, real, hid, h, w = shape
    pitch = pitch or cs
    m = mp.Micro(dtype, n, 32, 32, seed=cs + code)
    x, P, _ = _data(cs, real, hid, h, w, n, dtype, 11 * cs + code)
    b = m.buf(h, w, pitch)
    m.fill(b, x, coff=coff)
    raw = block_of(P, cs).numpy().tobytes()
    op = mp.new_op(KIND, relu=code, cin=cs, cout=cs, cout_pad=cs, chain_cout=hid, hin=h, win=w, hout=h, wout=w, in_buf=b, out_buf=b,
                   w_off=m.put(raw[:len(raw) - short]))
    if pitch != cs:
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = coff, pitch, coff, pitch
    if mutate:
        mutate(m, op, b)
    m.add(op)
    m.wrote(b, coff, cs)
    return m, b, x, P


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("code", [0, 2])
@pytest.mark.parametrize("shape,coff,pitch", [(SHAPES[2], 0, None), (SHAPES[4], 0, None), (SHAPES[1], 32, 64)],
                         ids=["C96-17x19", "C576-2x3", "C32-view"])
def test_se_act_in_a_program(shape, coff, pitch, code, dtype):
    """udp_hrnet_create / forward: in place on a poisoned workspace, nothing outside the view touched."""
    cs, real = shape[0], shape[1]
    m, b, x, P = _micro(dtype, shape, code, coff=coff, pitch=pitch)
    assert m.run() == 0, m.error
    got = m.read(b, coff, cs)
    e_hip, _, gate = mp.parity("se_act program C%d code%d %s" % (cs, code, dtype), got[:, :real], se_act_ref(x, P, code, torch.float64)[0],
                               se_act_ref(x, P, code, torch.float32)[0], ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    if real < cs:
        assert float(got[:, real:].abs().max()) == 0.0
    m.assert_untouched()
    m.check_head()


def test_se_act_range_guard():
    """A scaled result beyond fp16's range raises udp_f16x2_overflow; an in-range case leaves it clear.  The gate is 1
    everywhere (b2 = 6), so the element comes out as it went in: 60000 in range; hi = 65504 with lo = 65504 decodes to
    65504 + 65504 * 2^-11 = 65535.98 >= 65520, which no fp16 holds."""
    cs, real, hid, h, w, n = 32, 16, 8, 3, 5, 1
    P = (torch.zeros(hid, real), torch.zeros(hid), torch.zeros(real, hid), torch.full((real,), 6.0))
    block = block_of(P, cs).cuda()
    _lib.f16x2_overflow(reset=True)
    for hi, lo, want in ((60000.0, 0.0, False), (65504.0, 65504.0, True)):
        x = torch.zeros(n, cs, h, w)
        x[:, :real] = 1.0
        xin = _dev(x.permute(0, 2, 3, 1), "f16x2")                    # [n, h, w, plane, C]
        xin[0, 1, 2, 0, 3], xin[0, 1, 2, 1, 3] = hi, lo
        out = _nan("f16x2", n, h, w, cs)
        assert _call(_op(cs, hid, h, w, 0), "f16x2", n, xin, block, out) == 0, _lib.lib().udp_last_error()
        assert bool(_lib.f16x2_overflow(reset=True)) == want, (hi, lo)


# ------------------------------------------------------------------ rejections
def _rc_fused(mutate, dtype=_lib.UDP_F32, res=None, alias=None):
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    op = _op(32, 8, 8, 6, 2)
    if mutate:
        mutate(op)
    P = _lib.ptr
    out = buf[1 << 19:] if alias is None else buf[alias:]
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), dtype, 1, P(buf), P(buf[1 << 17:]), None, res and P(buf[1 << 16:]), None, None, None,
                                     P(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _set(**kw):
    def f(op):
        for k, v in kw.items():
            setattr(op, k, v)
    return f


def test_rejections_conv2d_fused():
    assert _rc_fused(None) == 0 and _rc_fused(None, _lib.UDP_F16X2) == 0        # the accepted form
    for code in (0, 1):
        assert _rc_fused(_set(relu=code)) == 0
    assert _rc_fused(None, _lib.UDP_BF16) == UNSUP
    assert _rc_fused(_set(relu=4)) == UNSUP
    assert _rc_fused(_set(relu=3)) == ARG and _rc_fused(_set(relu=5)) == ARG and _rc_fused(_set(relu=-1)) == ARG
    assert _rc_fused(_set(cin=1056, cout=1056, cout_pad=1056)) == ARG
    assert _rc_fused(_set(cin=48, cout=48, cout_pad=48)) == ARG                  # C % 32 != 0
    assert _rc_fused(_set(chain_cout=0)) == ARG and _rc_fused(_set(chain_cout=33)) == ARG
    assert _rc_fused(_set(cin=512, cout=512, cout_pad=512, chain_cout=257)) == ARG
    assert _rc_fused(None, res=True) == ARG                                     # res
    assert _rc_fused(_set(n_up=1)) == UNSUP
    assert _rc_fused(_set(n_out2=1)) == UNSUP and _rc_fused(_set(group=1)) == UNSUP and _rc_fused(_set(wfmt=1)) == UNSUP
    assert _rc_fused(_set(hout=4)) == ARG
    assert _rc_fused(_set(in_coff=4, in_pitch=64)) == ARG                       # views in multiples of 8
    # `out` is `in` but another view of it
    assert _rc_fused(_set(in_coff=0, in_pitch=64, out_coff=32, out_pitch=64), alias=0) == ARG
    assert _rc_fused(_set(in_coff=32, in_pitch=64, out_coff=32, out_pitch=64), alias=0) == 0


def _program_rc(mutate=None, dtype="f32", short=0):
    m, b, _, _ = _micro(dtype, SHAPES[1], 2, n=1, mutate=mutate, short=short)
    try:
        h = m.create()
    except _lib.UdpPoseError as e:
        return e.code
    _lib.lib().udp_hrnet_destroy(h)
    return 0


def test_rejections_program():
    assert _program_rc() == 0 and _program_rc(dtype="f16x2") == 0
    assert _program_rc(dtype="bf16") == UNSUP
    assert _program_rc(lambda m, op, b: setattr(op, "relu", 4)) == UNSUP
    assert _program_rc(lambda m, op, b: setattr(op, "relu", 3)) == ARG
    assert _program_rc(_wide(1056)) == ARG
    assert _program_rc(_wide(48)) == ARG
    assert _program_rc(lambda m, op, b: setattr(op, "chain_cout", 0)) == ARG
    assert _program_rc(lambda m, op, b: setattr(op, "chain_cout", 33)) == ARG
    assert _program_rc(lambda m, op, b: setattr(op, "res_buf", m.head_buf)) == ARG
    assert _program_rc(lambda m, op, b: setattr(op, "n_up", 1)) == UNSUP

    def other_view(m, op, b):            # the same buffer through two different views
        wide = m.buf(3, 5, 64)
        op.in_buf = op.out_buf = wide
        op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = 0, 64, 32, 64
    assert _program_rc(other_view) == ARG
    # the parameter block, (2 C Ch + Ch + C) * 4 = 2208 bytes, is the last entry of the blob, which is rounded up to 256
    # bytes (96 here): a block cut by 256 bytes ends beyond the blob (a cut inside the rounding cannot be seen)
    assert _program_rc(short=256) == ARG


def _wide(c):
    def f(m, op, b):
        op.cin = op.cout = op.cout_pad = c
        op.in_buf = op.out_buf = m.buf(3, 5, c)
    return f


# ------------------------------------------------------------------ the project conv's form
@pytest.mark.parametrize("dtype,ws", [("f32", False), ("f16x2", True), ("f16x2", False)], ids=["f32", "f16x2-ws", "f16x2-lds"])
def test_project_conv_with_residual_and_no_activation(dtype, ws):
    """1x1 UDP_OP_CONV with ``res`` and activation 0 at 96 -> 40 real channels (stored 96 -> 64), in a micro-program."""
    n, h, w, cin, cout, cs = 3, 8, 8, 96, 40, 64
    m = mp.Micro(dtype, n, 32, 32, seed=5)
    a, r, o = m.buf(h, w, cin), m.buf(h, w, cs), m.buf(h, w, cs)
    x = m.fill(a, m.randn(n, cin, h, w))
    rz = torch.zeros(n, cs, h, w)
    rz[:, :cout] = m.randn(n, cout, h, w)
    res = m.fill(r, rz)
    wt = mp.quant(m.randn(cout, cin, 1, 1) * float(np.sqrt(1.0 / cin)), dtype)
    bt = m.randn(cout) * 0.1
    m.add(mp.new_op(_lib.UDP_OP_CONV, relu=0, cin=cin, cout=cs, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=o, res_buf=r,
                    **m.put_conv(torch.cat([wt, torch.zeros(cs - cout, cin, 1, 1)]), torch.cat([bt, torch.zeros(cs - cout)]), ws=ws)))
    m.wrote(o)
    assert m.run() == 0, m.error
    got = m.read(o)
    ref = mp.ref_conv(x.double(), wt.double(), bt.double(), res=res[:, :cout].double())
    assert float((ref < 0).double().mean()) > 0.2                               # no ReLU was applied
    err = float((got[:, :cout].double() - ref).abs().max())
    assert err <= mp.conv_tol(dtype, ref), (err, mp.conv_tol(dtype, ref))
    assert float(got[:, cout:].abs().max()) == 0.0
    m.assert_untouched()
    m.check_head()
