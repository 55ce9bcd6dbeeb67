"""The three op kinds of RSN-18 "se + prm" (include/udp_pose_hip.h, kinds 20 - 22; csrc/rsn_gate.hip) against fp64:
UDP_OP_SE_RES (the SELayer that closes a Bottleneck, with the shortcut and the ReLU), UDP_OP_PRM_GATE (the channel gate
of the Pose Refine Machine) and UDP_OP_PRM_DW9 (its depthwise 9x9 spatial gate and the combine).

Every parity case is a micro-program (tests/microprog.py): the workspace is poisoned, the operands are stored quantised
to the storage mode, ONE eager forward runs, and every 16-bit unit outside the op's declared outputs must keep its bits.
The gate is the project's rule for new arithmetic, |hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp relative to the tensor's max
(microprog.parity; ulp = 2^-23 fp32, 2^-21 split fp16)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from udp_pose_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16x2"]
SE, GATE, DW9 = _lib.UDP_OP_SE_RES, _lib.UDP_OP_PRM_GATE, _lib.UDP_OP_PRM_DW9


def _gen(*key):
    return torch.Generator().manual_seed(sum((31 ** i) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _prefill_rows(m, b, rows):
    """Pre-fill the fp32 side buffer ``b`` (Micro.buf_rows) with ``rows`` [B, floats]: raw fp32 in every storage mode."""
    orig = m.host_workspace

    def host_workspace():
        ws = orig()
        u = rows.to(torch.float32).contiguous().numpy().view(np.int16).reshape(-1)
        ws[m.offs[b] // 2:m.offs[b] // 2 + u.size] = u
        return ws
    m.host_workspace = host_workspace


# ------------------------------------------------------------------ (a) squeeze-and-excitation + residual
def se_ref(x, w1, w2, res, relu, dt):
    """network.py:62-66 and :137-143: x * sigmoid(W2 relu(W1 mean x)) [+ shortcut] [ReLU]."""
    x = x.to(dt)
    m = torch.sigmoid(F.relu(x.mean(dim=(2, 3)) @ w1.to(dt).t()) @ w2.to(dt).t())
    y = x * m[:, :, None, None]
    if res is not None:
        y = y + res.to(dt)
    return F.relu(y) if relu else y


def _se_case(c, ch, h, w, n, dtype, res, relu, inplace, view):
    g = _gen(c, ch, h, w, res, relu, inplace, view)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    m = mp.Micro(dtype, n, 32, 32, seed=7)
    pitch, coff = (c + 64, 32) if view else (c, 0)
    a = m.buf(h, w, pitch)
    x = m.fill(a, r(n, c, h, w) + 0.5 * r(1, c, 1, 1), coff)                    # channel means differ
    o = a if inplace else m.buf(h, w, pitch)
    rb, xr = _lib.UDP_BUF_NONE, None
    if res:
        rb = m.buf(h, w, pitch)
        xr = m.fill(rb, r(n, c, h, w), coff)
    w1 = r(ch, c) * (2.0 / np.sqrt(c))
    w2 = r(c, ch) * (3.0 / np.sqrt(ch))                                         # the gate spreads over (0, 1)
    w_off = m.put(torch.cat([w1.t().reshape(-1), w2.t().reshape(-1)]).contiguous().numpy().tobytes())
    m.add(mp.new_op(SE, relu=relu, cin=c, cout=c, cout_pad=c, chain_cout=ch, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=o, res_buf=rb,
                    in_coff=coff, out_coff=coff, res_coff=coff, in_pitch=pitch, out_pitch=pitch, res_pitch=pitch, w_off=w_off))
    m.wrote(o, coff, c)
    assert m.run() == 0, m.error
    r64 = se_ref(x, w1, w2, xr, relu, torch.float64)
    gate = torch.sigmoid(F.relu(x.double().mean(dim=(2, 3)) @ w1.double().t()) @ w2.double().t())
    assert float(gate.std()) > 0.05, "a flat gate would hide the op"
    name = "se+res C%d/%d %dx%d %s res%d relu%d inplace%d view%d" % (c, ch, h, w, dtype, res, relu, inplace, view)
    e_hip, _, tol = mp.parity(name, m.read(o, coff, c), r64, se_ref(x, w1, w2, xr, relu, torch.float32), mp.ULP[dtype])
    assert e_hip <= tol, (e_hip, tol)
    m.assert_untouched()
    m.check_head()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 6)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("cc", [(64, 8), (512, 64)], ids=lambda s: "%d-%d" % s)
def test_se_res_matches_fp64(cc, hw, res, relu, inplace, dtype):
    _se_case(cc[0], cc[1], hw[0], hw[1], 3, dtype, res, relu, inplace, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inplace", [0, 1])
def test_se_res_channel_view(inplace, dtype):
    """64 channels from offset 32 of 128-pitch tensors (in, res and out): the neighbours hold NaN / poison and keep it."""
    _se_case(64, 8, 3, 5, 3, dtype, 1, 1, inplace, 1)


# ------------------------------------------------------------------ (b) PRM channel gate
def gate_ref(x, w1, b1, w2, b2, dt):
    """network.py:293-296 with the conv bias + BatchNorm folded: sigmoid(relu(W2 relu(W1 mean x + b1) + b2))."""
    hid = F.relu(x.to(dt).mean(dim=(2, 3)) @ w1.to(dt).t() + b1.to(dt))
    return torch.sigmoid(F.relu(hid @ w2.to(dt).t() + b2.to(dt)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", [32, 256])
def test_prm_channel_gate_matches_fp64(c, hw, dtype):
    h, w = hw
    n = 3
    g = _gen(c, h, w, 11)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    m = mp.Micro(dtype, n, 32, 32, seed=8)
    pitch, coff = c + 32, 8                                                     # a view, so that the pitch matters
    a = m.buf(h, w, pitch)
    x = m.fill(a, r(n, c, h, w) + 0.5 * r(1, c, 1, 1), coff)
    rows = m.buf_rows(c)
    w1, b1 = r(c, c) * (2.0 / np.sqrt(c)), r(c) * 0.3
    w2, b2 = r(c, c) * (3.0 / np.sqrt(c)), r(c) * 0.3
    w_off = m.put(torch.cat([w1.t().reshape(-1), b1, w2.t().reshape(-1), b2]).contiguous().numpy().tobytes())
    m.add(mp.new_op(GATE, cin=c, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=rows, in_coff=coff, in_pitch=pitch,
                    w_off=w_off))
    m.wrote(rows)
    assert m.run() == 0, m.error
    r64 = gate_ref(x, w1, b1, w2, b2, torch.float64)
    assert float(r64.std()) > 0.05 and float((r64 == 0.5).double().mean()) > 0.1, "both branches of the ReLU before the sigmoid"
    e_hip, _, tol = mp.parity("prm gate C%d %dx%d %s" % (c, h, w, dtype), m.read_rows(rows), r64, gate_ref(x, w1, b1, w2, b2, torch.float32),
                              mp.ULP["f32"])                                    # the row is fp32 in every storage mode
    assert e_hip <= tol, (e_hip, tol)
    m.assert_untouched()
    m.check_head()


# ------------------------------------------------------------------ (c) PRM spatial gate: depthwise 9x9 + combine
def dw9_ref(t, wt, bt, a, res, dt):
    """network.py:298-300: out_1 * (1 + a * sigmoid(relu(dw9(t) + b)))."""
    s = torch.sigmoid(F.relu(F.conv2d(t.to(dt), wt.to(dt), bt.to(dt), padding=4, groups=t.shape[1])))
    return res.to(dt) * (1 + a.to(dt)[:, :, None, None] * s)


def _dw9_data(c, h, w, n, dtype, seed=0):
    g = _gen(c, h, w, seed, 5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    return dict(t=mp.quant(r(n, c, h, w), dtype), res=mp.quant(r(n, c, h, w), dtype), a=torch.rand(n, c, generator=g, dtype=torch.float32),
                wt=r(c, 1, 9, 9) * float(np.sqrt(2.0 / 81)), bt=r(c) * 0.1)


def _dw9_run(d, dtype, view=False):
    """One micro-program around one UDP_OP_PRM_DW9; returns (Micro, output buffer, channel offset)."""
    n, c, h, w = d["t"].shape
    m = mp.Micro(dtype, n, 32, 32, seed=9)
    pitch, coff = (c + 64, 32) if view else (c, 0)
    tb, rb, o, rows = m.buf(h, w, pitch), m.buf(h, w, pitch), m.buf(h, w, pitch), m.buf_rows(c)
    m.fill(tb, d["t"], coff)
    m.fill(rb, d["res"], coff)
    _prefill_rows(m, rows, d["a"])
    w_off = m.put(d["wt"].reshape(c, 81).t().contiguous().numpy().tobytes())    # [81][C], tap-major
    b_off = m.put(d["bt"].numpy().tobytes())
    m.add(mp.new_op(DW9, ks=9, cin=c, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w, in_buf=tb, res_buf=rb, out_buf=o, n_up=1, up_buf=[rows],
                    in_coff=coff, out_coff=coff, res_coff=coff, in_pitch=pitch, out_pitch=pitch, res_pitch=pitch, w_off=w_off, b_off=b_off))
    m.wrote(o, coff, c)
    assert m.run() == 0, m.error
    return m, o, coff


def _dw9_check(name, d, dtype, view=False):
    c = d["t"].shape[1]
    m, o, coff = _dw9_run(d, dtype, view)
    args = (d["t"], d["wt"], d["bt"], d["a"], d["res"])
    pre = F.conv2d(d["t"].double(), d["wt"].double(), d["bt"].double(), padding=4, groups=c)
    if pre.shape[2] * pre.shape[3] >= 81:      # (on the all-halo maps few taps count and the pre-activation is small by construction)
        assert 0.2 < float((pre > 0).double().mean()) < 0.8 and float(torch.sigmoid(F.relu(pre)).std()) > 0.05, "the gate must not be flat"
    e_hip, _, tol = mp.parity(name, m.read(o, coff, c), dw9_ref(*args, torch.float64), dw9_ref(*args, torch.float32), mp.ULP[dtype])
    assert e_hip <= tol, (e_hip, tol)
    m.assert_untouched()
    m.check_head()
    return m, o


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(1, 1), (3, 2), (9, 9), (13, 11), (64, 48)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", [32, 256])
def test_prm_dw9_matches_fp64(c, hw, dtype):
    """1x1 and 3x2 are all halo (most taps skipped), 9x9 is the window, 13x11 is no multiple of the 8 x 16 tile or of the
    4-pixel run, 64x48 is the map of the net (several tiles in both directions, interior threads on the fast path)."""
    _dw9_check("prm dw9 C%d %dx%d %s" % (c, hw[0], hw[1], dtype), _dw9_data(c, hw[0], hw[1], 1, dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [32, 256])
def test_prm_dw9_batch_and_views(c, dtype):
    """n = 3 at 13x11 through channel views; image 1 of the batch is bit-equal to the same image run alone."""
    d = _dw9_data(c, 13, 11, 3, dtype, seed=1)
    m3, o3 = _dw9_check("prm dw9 C%d 13x11 n3 views %s" % (c, dtype), d, dtype, view=True)
    one = {k: (v[1:2] if k in ("t", "res", "a") else v) for k, v in d.items()}
    m1, o1, coff = _dw9_run(one, dtype, view=True)
    assert np.array_equal(m3.read_raw(o3, coff, c)[1], m1.read_raw(o1, coff, c)[0])


def test_prm_dw9_skips_taps_outside_the_image():
    """A tap outside the image is skipped, not multiplied by zero: with inf weights on every tap but the centre, a 1x1
    map (whose 80 other taps all fall outside) still comes out finite, and equal to the centre tap alone."""
    d = _dw9_data(32, 1, 1, 2, "f32", seed=2)
    wt = torch.full_like(d["wt"], float("inf"))
    wt[:, :, 4, 4] = d["wt"][:, :, 4, 4]
    m, o, _ = _dw9_run(dict(d, wt=wt), "f32")
    centre = torch.zeros_like(d["wt"])
    centre[:, :, 4, 4] = d["wt"][:, :, 4, 4]
    args = (d["t"], centre, d["bt"], d["a"], d["res"])
    got = m.read(o)
    assert torch.isfinite(got).all()
    e_hip, _, tol = mp.parity("prm dw9 1x1, inf off-centre taps", got, dw9_ref(*args, torch.float64), dw9_ref(*args, torch.float32), mp.ULP["f32"])
    assert e_hip <= tol, (e_hip, tol)


# ------------------------------------------------------------------ refusals
def _op(kind, c=32, h=8, w=6, **fields):
    base = dict(cin=c, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w)
    if kind == SE:
        base.update(chain_cout=8)
    if kind == DW9:
        base.update(ks=9, n_up=1)
    base.update(fields)
    return mp.new_op(kind, **base)


def test_refusals_of_the_single_op_entry():
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    lib, P = _lib.lib(), _lib.ptr
    x, wgt, bias, res, up0, out = (P(buf[k << 16:]) for k in range(6))

    def call(op, dtype=_lib.UDP_F32, inp=x, res=None, up0=None, out=out):
        rc = lib.udp_conv2d_fused(C.byref(op), dtype, 1, inp, wgt, bias, res, up0, None, None, out, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    UNSUP, ARG = -3, -1
    # the accepted forms
    assert call(_op(SE)) == 0 and call(_op(SE), _lib.UDP_F16X2) == 0 and call(_op(SE, relu=1), res=res) == 0 and call(_op(SE), out=x) == 0
    assert call(_op(GATE)) == 0 and call(_op(GATE), _lib.UDP_F16X2) == 0
    assert call(_op(DW9), res=res, up0=up0) == 0 and call(_op(DW9), _lib.UDP_F16X2, res=res, up0=up0) == 0
    # bf16
    assert call(_op(SE), _lib.UDP_BF16) == UNSUP and call(_op(GATE), _lib.UDP_BF16) == UNSUP
    assert call(_op(DW9), _lib.UDP_BF16, res=res, up0=up0) == UNSUP
    # (c): stride 2, another kernel size, out aliasing in / res, a missing operand
    assert call(_op(DW9, stride=2, hout=4, wout=3), res=res, up0=up0) == ARG
    assert call(_op(DW9, ks=7), res=res, up0=up0) == ARG
    assert call(_op(DW9), res=res, up0=up0, out=x) == ARG and call(_op(DW9), res=res, up0=up0, out=res) == ARG
    assert call(_op(DW9), res=res) == ARG and call(_op(DW9), up0=up0) == ARG and call(_op(DW9, n_up=0), res=res, up0=up0) == ARG
    # C not a multiple of 32; hidden width 0 or > 256; C beyond the kernels' reach
    for kind, kw in ((SE, {}), (GATE, {}), (DW9, dict(res=res, up0=up0))):
        assert call(_op(kind, c=48, cout_pad=64), **kw) == ARG
    assert call(_op(SE, chain_cout=0)) == ARG and call(_op(SE, c=512, chain_cout=257)) == ARG and call(_op(SE, c=544)) == ARG
    assert call(_op(SE, c=512, chain_cout=256)) == 0
    assert call(_op(GATE, c=288)) == ARG and call(_op(GATE, chain_cout=8)) == ARG and call(_op(GATE), res=res) == ARG
    # activation codes: ReLU on (a) only; hard-swish / SiLU nowhere; the in-place rule of (a)
    assert call(_op(GATE, relu=1)) == UNSUP and call(_op(DW9, relu=1), res=res, up0=up0) == UNSUP
    assert call(_op(SE, relu=2)) == UNSUP and call(_op(SE, relu=4)) == UNSUP and call(_op(SE, relu=3)) == ARG
    assert call(_op(SE, c=32, in_pitch=64, out_pitch=64, out_coff=32), out=x) == ARG
    assert call(_op(SE), res=x) == ARG
    torch.cuda.synchronize()


def _program_rc(kind, mutate):
    """udp_hrnet_create on a micro-program around one op of ``kind`` (32 channels, 8x6), altered by ``mutate``."""
    m = mp.Micro("f32", 1, 32, 32)
    a, r, o, rows = m.buf(8, 6, 32), m.buf(8, 6, 32), m.buf(8, 6, 32), m.buf_rows(32)
    w_off = m.put(np.zeros(81 * 32 * 4 + 2 * 32 * 32 * 4 + 256, dtype=np.uint8).tobytes())
    b_off = m.put(np.zeros(32 * 4, dtype=np.uint8).tobytes())
    op = _op(kind, in_buf=a, out_buf=rows if kind == GATE else o, w_off=w_off, b_off=b_off)
    if kind == DW9:
        op.res_buf, op.up_buf[0] = r, rows
    mutate(op, a, r, o, rows)
    m.add(op)
    try:
        h = m.create()
    except _lib.UdpPoseError as e:
        return e.code
    _lib.lib().udp_hrnet_destroy(h)
    return 0


def test_refusals_of_the_program():
    ok = lambda *_: None
    assert _program_rc(SE, ok) == 0 and _program_rc(GATE, ok) == 0 and _program_rc(DW9, ok) == 0
    assert _program_rc(SE, lambda op, a, r, o, rows: setattr(op, "out_buf", a)) == 0                      # in place
    assert _program_rc(SE, lambda op, a, r, o, rows: setattr(op, "res_buf", a)) == -1                     # res in the buffer of in
    assert _program_rc(DW9, lambda op, a, r, o, rows: setattr(op, "out_buf", a)) == -1
    assert _program_rc(DW9, lambda op, a, r, o, rows: setattr(op, "out_buf", r)) == -1
    assert _program_rc(DW9, lambda op, a, r, o, rows: setattr(op, "res_buf", _lib.UDP_BUF_NONE)) == -1
    assert _program_rc(DW9, lambda op, a, r, o, rows: setattr(op, "stride", 2)) == -1
    assert _program_rc(GATE, lambda op, a, r, o, rows: setattr(op, "out_buf", a)) == -1
    assert _program_rc(GATE, lambda op, a, r, o, rows: setattr(op, "res_buf", r)) == -1
    assert _program_rc(SE, lambda op, a, r, o, rows: setattr(op, "w_off", 1 << 30)) == -1                 # block outside the blob
    assert _program_rc(SE, lambda op, a, r, o, rows: setattr(op, "chain_cout", 300)) == -1


# ------------------------------------------------------------------ split-fp16 range guard of the two writers
@pytest.mark.parametrize("kind", ["se", "dw9"])
def test_f16x2_range_guard_sees_the_new_writers(kind):
    """udp_f16x2_overflow ORs the flag of csrc/rsn_gate.hip: a result of magnitude >= 65520 about to be split raises it,
    the same launch on small operands leaves it clear.  SE: in = 40000, gate 0.5 (zero weights), res = 50000 -> 70000;
    dw9: res = 60000, a = 1, spatial gate 0.5 (zero weights and bias) -> 90000."""
    n, c, h, w = 2, 32, 3, 5
    for big in (False, True):
        _lib.f16x2_overflow(reset=True)
        m = mp.Micro("f16x2", n, 32, 32, seed=3)
        a, r, o = m.buf(h, w, c), m.buf(h, w, c), m.buf(h, w, c)
        scale = 1.0 if big else 1e-3
        if kind == "se":
            m.fill(a, torch.full((n, c, h, w), 40000.0 * scale))
            m.fill(r, torch.full((n, c, h, w), 50000.0 * scale))
            w_off = m.put(np.zeros(2 * c * 8 * 4, dtype=np.uint8).tobytes())
            m.add(mp.new_op(SE, cin=c, cout=c, cout_pad=c, chain_cout=8, hin=h, win=w, hout=h, wout=w, in_buf=a, out_buf=o, res_buf=r, w_off=w_off))
            want = 70000.0 * scale
        else:
            rows = m.buf_rows(c)
            m.fill(a, torch.zeros(n, c, h, w))
            m.fill(r, torch.full((n, c, h, w), 60000.0 * scale))
            _prefill_rows(m, rows, torch.ones(n, c))
            w_off = m.put(np.zeros(81 * c * 4, dtype=np.uint8).tobytes())
            b_off = m.put(np.zeros(c * 4, dtype=np.uint8).tobytes())
            m.add(mp.new_op(DW9, ks=9, cin=c, cout=c, cout_pad=c, hin=h, win=w, hout=h, wout=w, in_buf=a, res_buf=r, out_buf=o, n_up=1,
                            up_buf=[rows], w_off=w_off, b_off=b_off))
            want = 90000.0 * scale
        m.wrote(o)
        assert m.run() == 0, m.error
        assert _lib.f16x2_overflow(reset=True) == big
        if not big:
            assert float((m.read(o) - want).abs().max()) <= 1e-4 * want
