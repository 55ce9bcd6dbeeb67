"""The MobileViTv2 training kernels (csrc/mobilevitv2_train.hip), one entry point at a time through ctypes, against fp64
autograd of the same op on the CPU: SiLU (tests/mobilevitv2_ref.silu), GroupNorm(1, C) in train mode (F.group_norm) and
the separable self-attention core (tests/mobilevitv2_ref.linear_attention_core), at the smallest shapes where each can
go wrong and at the largest maps of the real 256x192 step.

Every output lives in an arena of one NaN bit pattern between two guards (tests/test_gpu_train_arms.py): it must come
back fully written and the guards untouched.  The gate is measured, not chosen: ours may be at most 4 x as far from fp64
as torch's fp32 CPU run of the same op is, or 1e-6 * max|ref| where that is more (fp32 CPU error can be zero on tiny
tensors).  Pads of every output are exactly zero -- the inputs' pads hold garbage, so nothing may count them --, two
runs are bit-identical."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mobilevitv2_ref as R                               # noqa: E402
from test_gpu_train_arms import GUARD, Arena              # noqa: E402
from udp_pose_amd import _lib                             # noqa: E402

F32 = _lib.UDP_F32
GN_EPS = 1e-5


def _s():
    return _lib.stream_ptr()


def _ok(rc):
    assert rc == 0, _lib.lib().udp_last_error()


def _nhwc(t, pitch, pad=0.0):
    """NCHW fp64 (exactly fp32-representable values) -> device NHWC fp32, channels c..pitch holding ``pad``."""
    n, c, h, w = t.shape
    o = torch.full((n, h, w, pitch), pad, dtype=torch.float32)
    o[..., :c] = t.permute(0, 2, 3, 1).float()
    return o.cuda()


def _nchw(t, n, h, w, pitch, real):
    return t.view(n, h, w, pitch)[..., :real].permute(0, 3, 1, 2)


def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen).double()     # fp32 draws: exact in every precision used here


def _gate(name, got, ref64, ref32):
    mx = float(ref64.abs().max())
    assert mx > 0, "%s: the reference is zero, the gate would be vacuous" % name
    e_ours = float((got.double() - ref64).abs().max())
    e_f32 = float((ref32.double() - ref64).abs().max())
    gate = max(4 * e_f32, 1e-6 * mx)
    print("%-52s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (name, mx, e_f32, e_ours, gate))
    assert e_ours <= gate, (name, e_ours, gate)


def _pads_zero(t, pitch, real):
    return pitch == real or float(t.view(-1, pitch)[:, real:].abs().max()) == 0.0


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ SiLU
def test_silu_forward_and_backward():
    """3 x 5 x 7 x 16 = 1680 values (not a multiple of 1024), among them 0, +-1e-6, +-20 and +-90: exp(-x) overflows to
    +inf at -90 and the kernel must give 0 / x and 0 / dy, not NaN.  Arbiter: the restated silu under fp64 autograd
    (finite there: exp(90) fits fp64).  Yardstick: F.silu in fp32 -- fp32 autograd through the restated form is inf * 0 =
    NaN at -90, which is why the kernel states its derivative in s = sigmoid(x)."""
    L = _lib.lib()
    count = 3 * 5 * 7 * 16
    gen = torch.Generator().manual_seed(5)
    special = torch.tensor([0.0, 1e-6, -1e-6, 20.0, -20.0, 90.0, -90.0, 88.0, -88.0, 89.5, -89.5, 3.0])
    x = torch.cat([special, torch.randn(count - special.numel(), generator=gen) * 4]).float()
    dy = torch.randn(count, generator=gen)
    xr = x.double().requires_grad_(True)
    y64 = R.silu(xr)
    dx64 = torch.autograd.grad(y64, xr, dy.double())[0]
    y64 = y64.detach()
    assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(dx64).all())
    xs = x.double().requires_grad_(True)                           # the restatement IS nn.SiLU
    ys = F.silu(xs)
    assert float((ys.detach() - y64).abs().max()) <= 1e-12 * 90 and \
        float((torch.autograd.grad(ys, xs, dy.double())[0] - dx64).abs().max()) <= 1e-12 * float(dx64.abs().max())
    x32 = x.clone().requires_grad_(True)
    y32 = F.silu(x32)
    dx32 = torch.autograd.grad(y32, x32, dy)[0]
    xd, dd = x.cuda(), dy.cuda()
    runs = []
    for _ in range(2):
        y, dx = Arena(count), Arena(count)
        _ok(L.udp_silu_fwd(xd.data_ptr(), y.ptr(), count, _s()))
        _ok(L.udp_silu_bwd(dd.data_ptr(), xd.data_ptr(), dx.ptr(), count, _s()))
        runs.append((y.get("silu fwd"), dx.get("silu bwd")))
    (y, dx), again = runs
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    _gate("silu fwd", y, y64, y32.detach())
    _gate("silu bwd", dx, dx64, dx32)
    assert _same_bits(again[0], y) and _same_bits(again[1], dx)
    assert float(y[0]) == 0.0 and float(dx[0]) == float(0.5 * dy[0])                       # silu(0) = 0, silu'(0) = 1/2
    assert float(y[5]) == 90.0 and float(dx[5]) == float(dy[5]) and float(y[6]) == 0.0 and float(dx[6]) == 0.0


# ------------------------------------------------------------------ GroupNorm(1, C)
def _gn_ref(x, g, b, dy, dtype):
    n, c, h, w = x.shape
    x = x.to(dtype).requires_grad_(True)
    g, b = g.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    y = F.group_norm(x, 1, g, b, GN_EPS)
    dx, dg, db = torch.autograd.grad(y, [x, g, b], dy.to(dtype))
    _, mean, rstd = torch.native_group_norm(x.detach(), g.detach(), b.detach(), n, c, h * w, 1, GN_EPS)
    return dict(y=y.detach(), dx=dx, dg=dg, db=db, mu=mean.reshape(n), r=rstd.reshape(n))


def _gn_run(x, g, b, dy, cs, prev=None):
    """Pads of x and dy hold 3.0 / -2.0: a kernel that counted them would miss every gate."""
    L = _lib.lib()
    n, cr, h, w = x.shape
    xd, dd = _nhwc(x, cs, 3.0), _nhwc(dy, cs, -2.0)
    gd, bd = g.float().cuda(), b.float().cuda()                    # c_real entries only: nothing behind them may be read
    nbytes = int(L.udp_gnorm_train_workspace_bytes(n, h, w, cs))
    y, save, ws = Arena(n * h * w * cs), Arena(2 * n), Arena(nbytes // 4)
    _ok(L.udp_gnorm_train_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), n, h, w, cs, cr, F32, GN_EPS, y.ptr(), save.ptr(),
                              ws.ptr(), nbytes, _s()))
    ws.check("gnorm fwd workspace")
    out = dict(y=y.get("gnorm y"), save=save.get("gnorm save"))
    dx, dgm, dbt, ws2 = Arena(n * h * w * cs), Arena(cs), Arena(cs), Arena(nbytes // 4)
    if prev is not None:
        dx.t.copy_(_nhwc(prev, cs).reshape(-1))
    _ok(L.udp_gnorm_train_bwd(dd.data_ptr(), xd.data_ptr(), gd.data_ptr(), save.ptr(), n, h, w, cs, cr, F32, int(prev is not None),
                              dx.ptr(), dgm.ptr(), dbt.ptr(), ws2.ptr(), nbytes, _s()))
    ws2.check("gnorm bwd workspace")
    out["dx"] = dx.get("gnorm dx")
    for k, a in (("dg", dgm), ("db", dbt)):
        a.check("gnorm " + k)
        # only c_real entries are written: the rest of the stored row keeps the arena's pattern
        assert bool((a.raw[GUARD + cr:GUARD + cs] == a.pat).all()), "gnorm %s: wrote behind c_real" % k
        t = a.t[:cr].clone().cpu()
        assert not torch.isnan(t).any(), "gnorm %s: not fully written" % k
        out[k] = t
    return out


GN_CASES = [(3, 2, 2, 32, 24, 0.0), (2, 6, 4, 64, 64, 0.0), (2, 8, 6, 144, 144, 0.0), (2, 8, 6, 144, 144, 1000.0),
            (2, 32, 24, 64, 64, 0.0)]


@pytest.mark.parametrize("n,h,w,cs,cr,mean", GN_CASES)
def test_gnorm_forward_and_backward_against_fp64(n, h, w, cs, cr, mean):
    L = _lib.lib()
    split = int(L.udp_gnorm_train_split(h, w, cs))
    assert int(L.udp_gnorm_train_workspace_bytes(n, h, w, cs)) == n * split * (16 + 8 * cs)
    if (h, w) == (32, 24):
        assert split == 12                          # the largest map of the real step takes the multi-workgroup split
    if (h, w, cs) == (8, 6, 144):
        assert split == 2                           # 48 pixels in runs of 29 and 19: a ragged last run
    if (h, w) in ((2, 2), (6, 4)):
        assert split == 1
    gen = torch.Generator().manual_seed(7 * h + cs + int(mean))
    x = (_rand(gen, n, cr, h, w) + mean).float().double()          # mean 1000, standard deviation 1: E[x^2] - mu^2 in fp32 is noise
    g = (_rand(gen, cr) * 0.3 + 1).float().double()
    b, dy, prev = _rand(gen, cr) * 0.2, _rand(gen, n, cr, h, w), _rand(gen, n, cr, h, w)
    r64, r32 = _gn_ref(x, g, b, dy, torch.float64), _gn_ref(x, g, b, dy, torch.float32)
    tag = "C%d(%d) %dx%dx%d mean %g split %d" % (cs, cr, n, h, w, mean, split)
    for acc in (0, 1):
        got = _gn_run(x, g, b, dy, cs, prev if acc else None)
        if not acc:
            _gate("gnorm y " + tag, _nchw(got["y"], n, h, w, cs, cr), r64["y"], r32["y"])
            _gate("gnorm mu " + tag, got["save"].view(n, 2)[:, 0], r64["mu"], r32["mu"])
            _gate("gnorm r " + tag, got["save"].view(n, 2)[:, 1], r64["r"], r32["r"])
            _gate("gnorm dgamma " + tag, got["dg"], r64["dg"], r32["dg"])
            _gate("gnorm dbeta " + tag, got["db"], r64["db"], r32["db"])
        want64, want32 = (r64["dx"] + prev, r32["dx"] + prev.float()) if acc else (r64["dx"], r32["dx"])
        _gate("gnorm dx acc%d %s" % (acc, tag), _nchw(got["dx"], n, h, w, cs, cr), want64, want32)
        assert _pads_zero(got["y"], cs, cr) and _pads_zero(got["dx"], cs, cr), tag
        again = _gn_run(x, g, b, dy, cs, prev if acc else None)
        assert all(_same_bits(again[k], got[k]) for k in got), tag


# ------------------------------------------------------------------ the separable self-attention core
def _core(q, k, v):
    """tests/mobilevitv2_ref.linear_attention_core with its intermediates: (out, scores [B,4,M], ctx [B,4,C])."""
    b, c, h, w = k.shape
    cls = lambda t: t.reshape(b, t.shape[1], h // 2, 2, w // 2, 2)
    s = torch.softmax(cls(q).permute(0, 1, 3, 5, 2, 4).reshape(b, 1, 2, 2, -1), dim=-1)
    kk = cls(k).permute(0, 1, 3, 5, 2, 4).reshape(b, c, 2, 2, -1)
    ctx = (kk * s).sum(dim=-1)
    out = F.relu(cls(v)) * ctx[:, :, None, :, None, :]
    return out.reshape(b, c, h, w), s.reshape(b, 4, -1), ctx.permute(0, 2, 3, 1).reshape(b, 4, c)


def _la_ref(qkv, d, dout, dtype):
    qkv = qkv.to(dtype).requires_grad_(True)
    out, s, ctx = _core(qkv[:, :1], qkv[:, 1:1 + d], qkv[:, 1 + d:])
    assert torch.equal(out, R.linear_attention_core(qkv[:, :1], qkv[:, 1:1 + d], qkv[:, 1 + d:]))
    dqkv = torch.autograd.grad(out, qkv, dout.to(dtype))[0]
    return dict(out=out.detach(), s=s.detach(), ctx=ctx.detach(), dqkv=dqkv)


def _la_run(qkv, d, dout):
    L = _lib.lib()
    n, _, h, w = qkv.shape
    cq, m = (1 + 2 * d + 15) // 16 * 16, h * w // 4
    qd, dd = _nhwc(qkv, cq, 5.0), _nhwc(dout, d)
    out, scores, ctx, dqkv = Arena(n * h * w * d), Arena(n * 4 * m), Arena(n * 4 * d), Arena(n * h * w * cq)
    _ok(L.udp_linattn_train_fwd(qd.data_ptr(), n, h, w, cq, d, F32, out.ptr(), d, scores.ptr(), ctx.ptr(), _s()))
    _ok(L.udp_linattn_train_bwd(dd.data_ptr(), qd.data_ptr(), scores.ptr(), ctx.ptr(), n, h, w, cq, d, d, F32, dqkv.ptr(), _s()))
    return dict(out=out.get("linattn out"), s=scores.get("linattn scores"), ctx=ctx.get("linattn ctx"), dqkv=dqkv.get("linattn dqkv"))


@pytest.mark.parametrize("d,h,w", [(64, 2, 2), (64, 4, 2), (96, 8, 6), (144, 4, 4), (64, 32, 24)])
def test_linattn_forward_and_backward_against_fp64(d, h, w):
    n, cq = 2, (1 + 2 * d + 15) // 16 * 16
    assert d != 144 or cq == 304                                             # 289 channels are stored as 304
    gen = torch.Generator().manual_seed(d + h)
    qkv, dout = _rand(gen, n, 1 + 2 * d, h, w), _rand(gen, n, d, h, w)
    qkv[:, 0] = (qkv[:, 0] * 25).clamp(-80, 80).float().double()            # queries up to +-80: no overflow, no NaN
    qkv[0, 0, 0, 0], qkv[0, 0, -1, -1] = 80.0, -80.0
    zero = torch.rand(n, d, h, w, generator=gen) < 0.1
    qkv[:, 1 + d:][zero] = 0.0                                              # exact zeros among the values: dv = 0 there
    r64, r32 = _la_ref(qkv, d, dout, torch.float64), _la_ref(qkv, d, dout, torch.float32)
    got = _la_run(qkv, d, dout)
    tag = "d%d %dx%dx%d" % (d, n, h, w)
    assert all(bool(torch.isfinite(got[k]).all()) for k in got), tag
    _gate("linattn out " + tag, _nchw(got["out"], n, h, w, d, d), r64["out"], r32["out"])
    _gate("linattn scores " + tag, got["s"].view(n, 4, -1), r64["s"], r32["s"])
    _gate("linattn ctx " + tag, got["ctx"].view(n, 4, d), r64["ctx"], r32["ctx"])
    dq = _nchw(got["dqkv"], n, h, w, cq, 1 + 2 * d)
    if h * w == 4:                                  # one pixel per class: every score is exactly 1 and dq exactly 0
        assert float((got["s"] - 1).abs().max()) == 0.0 and float(dq[:, 0].abs().max()) == 0.0
        assert float(r64["dqkv"][:, 0].abs().max()) == 0.0
    else:
        _gate("linattn dq " + tag, dq[:, :1], r64["dqkv"][:, :1], r32["dqkv"][:, :1])
    _gate("linattn dk " + tag, dq[:, 1:1 + d], r64["dqkv"][:, 1:1 + d], r32["dqkv"][:, 1:1 + d])
    _gate("linattn dv " + tag, dq[:, 1 + d:], r64["dqkv"][:, 1 + d:], r32["dqkv"][:, 1 + d:])
    assert int(zero.sum()) > 0 and float(dq[:, 1 + d:][zero].abs().max()) == 0.0
    assert _pads_zero(got["dqkv"], cq, 1 + 2 * d) and cq > 1 + 2 * d, tag    # all stored channels of dqkv, pads zero
    again = _la_run(qkv, d, dout)
    assert all(_same_bits(again[k], got[k]) for k in got), tag
