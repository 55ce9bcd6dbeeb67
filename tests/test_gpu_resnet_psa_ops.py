"""Op-level fp64 parity of what pose_resnet_psa (ResNet-18 / 34) adds below the planner: the C = 512 arm of the four
PSA ops (csrc/psa.hip, the *_wide kernels), the BasicBlock conv shapes no other net here runs, and the deconv head
starting from 512 channels.

The PSA cases follow tests/test_gpu_program_ops.py::_psa: a hand-made micro-program (tests/microprog.py), one op under
test at a time against the reference on the operands AS STORED by the op before it, the gate
|hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp (errors relative to the tensor's max; the side rows are fp32 in every mode),
then every 16-bit unit outside the declared outputs unchanged and the head conv intact.  The conv and deconv cases use
the recipe and gate of tests/test_gpu_pose_resnet.py::test_wide_convs (1e-4 x scale, 2e-5 x scale for split fp16).
Each test prints its measured errors (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from microprog import Micro, new_op
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x2", "bf16"]
WIDE = 512
TOP = 65504.0                       # the largest value split fp16 holds exactly


# ------------------------------------------------------------------ PSA at C = 512
def _psa_program(mode, x, theta, P, h, w, n, seed):
    c = WIDE
    m = Micro(mode, n, seed=seed)
    bx, bpool, bmask = m.buf(h, w, c), m.buf_rows(2 * c), m.buf_rows(c + c // 2)
    bx1, bth, bx2 = m.buf(h, w, c), m.buf(h, w, c // 2), m.buf(h, w, c)
    xq, thq = m.fill(bx, x), m.fill(bth, theta)
    geom = dict(cin=c, cout=c, hin=h, win=w, hout=h, wout=w, w_off=m.put(mp.psa_block_bytes(P)))
    m.add(new_op(_lib.UDP_OP_PSA_POOL, in_buf=bx, out_buf=bpool, **geom))
    m.add(new_op(_lib.UDP_OP_PSA_MLP, in_buf=bpool, out_buf=bmask, **geom))
    m.add(new_op(_lib.UDP_OP_PSA_SCALE, in_buf=bx, res_buf=bmask, out_buf=bx1, **geom))
    m.add(new_op(_lib.UDP_OP_PSA_SP, in_buf=bth, res_buf=bx1, n_up=1, up_buf=[bmask], out_buf=bx2, **dict(geom, cin=c // 2)))
    for b in (bpool, bmask, bx1, bx2):
        m.wrote(b)
    assert m.run() == 0, m.error
    return m, xq, thq, m.read_rows(bpool), m.read_rows(bmask), m.read(bx1), m.read(bx2)


def _gate(name, got, ref64, ref32, ulp):
    e_hip, e_cpu, gate = mp.parity(name, got, ref64, ref32, ulp)
    assert e_hip <= gate, (name, e_hip, e_cpu, gate)


def _psa(mode, h, w, n=3, spread=4.0):
    c = WIDE
    x, theta, P = mp.psa_inputs(c, h, w, n, spread)
    P64 = {k: v.double() for k, v in P.items()}
    m, xq, thq, pool, mask, x1, x2 = _psa_program(mode, x, theta, P, h, w, n, seed=c + h)
    tag = "psa %s C%d %dx%d s%g " % (mode, c, h, w, spread)
    f32u = mp.ULP["f32"]
    _gate(tag + "pool.xbar", pool[:, :c], mp.psa_pool(xq.double(), P64)[:, :c], mp.psa_pool(xq, P)[:, :c], f32u)
    _gate(tag + "pool.xmean", pool[:, c:], mp.psa_pool(xq.double(), P64)[:, c:], mp.psa_pool(xq, P)[:, c:], f32u)
    _gate(tag + "mlp.m", mask[:, :c], mp.psa_mlp(pool.double(), P64)[:, :c], mp.psa_mlp(pool, P)[:, :c], f32u)
    _gate(tag + "mlp.gbar", mask[:, c:], mp.psa_mlp(pool.double(), P64)[:, c:], mp.psa_mlp(pool, P)[:, c:], f32u)
    _gate(tag + "scale", x1, mp.psa_scale(xq.double(), mask.double()), mp.psa_scale(xq, mask), mp.ULP[mode])
    _gate(tag + "sp", x2, mp.psa_sp(thq.double(), x1.double(), mask.double()), mp.psa_sp(thq, x1, mask), mp.ULP[mode])
    # the gates are not flat at this width (a mask or a spatial gate stuck at 0.5 would hide its op)
    sgate = torch.sigmoid(torch.einsum("nj,njp->np", mask[:, c:].double(),
                                       torch.softmax(thq.double().reshape(n, c // 2, h * w), dim=2)))
    assert float(mask[:, :c].max() - mask[:, :c].min()) > 0.5 and float(sgate.max() - sgate.min()) > 0.2
    m.assert_untouched()
    m.check_head()


# 8x6: layer 4 at 256x192.  12x9: at 384x288, 108 pixels, no multiple of 64 nor of the 8 waves.  4x3: at 128x96, fewer
# pixels than lanes.  2x2: fewer pixels than waves.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", [(8, 6), (12, 9), (4, 3), (2, 2)])
def test_psa_c512_ops_match_fp64(mode, h, w):
    _psa(mode, h, w)


@pytest.mark.parametrize("mode", MODES)
def test_psa_c512_peaked_softmax(mode):
    """Logit spread about 40: without the max-subtraction exp() overflows."""
    _psa(mode, 8, 6, spread=40.0)


def test_psa_c512_stays_silent_and_propagates_nan():
    """The split-fp16 writers of the wide arm (psa_scale_kernel, psa_sp_wide_kernel: both store through stx<H2>), as
    tests/test_gpu_f16x2_range.py::test_psa_stays_silent_and_propagates_nan has them at the narrower widths: x reaches
    +-65504 on a few elements and the range flag stays silent; a NaN element of x makes that image's pooled rows NaN
    and with them the spatial gate of every pixel of the image, the other images stay finite, and the NaN-proof guard
    reports it."""
    n, c, h, w = 3, WIDE, 8, 6
    x, theta, P = mp.psa_inputs(c, h, w, n)
    x[0, 0, 0, 0], x[n - 1, c - 1, h - 1, w - 1], x[n // 2, c // 2, h // 2, w // 2] = TOP, -TOP, TOP
    _lib.f16x2_overflow(reset=True)
    m, xq, thq, _, mask, x1, x2 = _psa_program("f16x2", x, theta, P, h, w, n, seed=c + h)
    m.assert_untouched()
    _gate("psa scale at the edge C512", x1, mp.psa_scale(xq.double(), mask.double()), mp.psa_scale(xq, mask), mp.ULP["f16x2"])
    _gate("psa sp at the edge C512", x2, mp.psa_sp(thq.double(), x1.double(), mask.double()), mp.psa_sp(thq, x1, mask),
          mp.ULP["f16x2"])
    assert float(x1.abs().max()) <= TOP and float(x2.abs().max()) <= TOP
    assert not _lib.f16x2_overflow(reset=True)
    x[n - 1, c - 1, h - 1, w - 1] = float("nan")
    m, _, _, _, _, x1, x2 = _psa_program("f16x2", x, theta, P, h, w, n, seed=c + h)
    m.assert_untouched()
    # (the mask itself survives: relu() of the NaN LayerNorm output is 0; the image's channel mean and so gbar are NaN)
    assert torch.isnan(x1[n - 1]).any() and torch.isnan(x2[n - 1]).all()
    assert torch.isfinite(x1[:n - 1]).all() and torch.isfinite(x2[:n - 1]).all()
    assert _lib.f16x2_overflow(reset=True) and not _lib.f16x2_overflow(reset=True)


@pytest.mark.parametrize("c", [1024, 384, 48])
def test_psa_still_refuses_other_widths(c):
    """Only the set of accepted widths grew by 512: every other one is refused at the first forward as before."""
    m = Micro("f32", 1)
    h = w = 2
    bx, bpool = m.buf(h, w, c), m.buf_rows(2 * c)
    m.fill(bx, m.randn(1, c, h, w))
    nw = c + c // 2 * c + c // 8 * (c // 2) + 3 * (c // 8) + c * (c // 8) + c + c // 2 * c
    m.add(new_op(_lib.UDP_OP_PSA_POOL, in_buf=bx, out_buf=bpool, cin=c, cout=c, hin=h, win=w, hout=h, wout=w,
                 w_off=m.put(np.zeros(nw, np.float32).tobytes())))
    assert m.run() == -3 and "must divide 256" in m.error and "512" in m.error, m.error
    m.written = []
    m.assert_untouched()
    assert torch.isnan(m.heat).all()


# ------------------------------------------------------------------ convs / deconvs of the BasicBlock ResNet
def _q(dtype):
    """Operands exactly as the device holds them (split fp16: 22-bit hi + lo pairs)."""
    return (lambda t: f16x2.decode(f16x2.encode(t))) if dtype == "f16x2" else (lambda t: t)


def _nhwc(t, dtype):
    t = t.permute(0, 2, 3, 1)
    return (f16x2.encode(t) if dtype == "f16x2" else t.contiguous()).cuda()


def _run(op, dtype, n, x, w, b, out, res=None):
    _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b),
                                           _lib.ptr(res), None, None, None, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()


def _nan_out(dtype, n, h, w, c):
    if dtype == "f16x2":
        return torch.full((n, h, w, 2, c), float("nan"), dtype=torch.float16, device="cuda")
    return torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device="cuda")


def _read(out, dtype):
    return (f16x2.decode(out) if dtype == "f16x2" else out).cpu().permute(0, 3, 1, 2).double().numpy()


def _conv_gate(name, got, ref, dtype):
    assert not np.isnan(got).any(), "output not fully written"
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print("%-36s err %.3g (scale %.3g)" % (name, err, scale))
    assert err <= 1e-4 * scale, (err, scale)
    if dtype == "f16x2":
        assert err <= 2e-5 * scale, (err, scale)


BASIC_CASES = [
    # ks, stride, cin, cout, h, w (input), residual, relu
    (3, 2, 64, 128, 64, 48, False, True),      # layer2.0 conv1
    (3, 2, 256, 512, 16, 12, False, True),     # layer4.0 conv1
    (3, 1, 64, 64, 64, 48, True, True),        # layer1 conv2 + identity shortcut
    (1, 2, 64, 128, 64, 48, False, False),     # layer2.0 downsample
    (1, 1, 512, 256, 8, 6, False, False),      # layer4 theta (deattn.conv_v_left)
]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("case", BASIC_CASES, ids=lambda c: "k%ds%d_%d-%d_%dx%d" % c[:6])
def test_basic_block_convs(case, dtype):
    ks, stride, cin, cout, h, w, res, relu = case
    n = 3
    rng = np.random.Generator(np.random.PCG64(cin + cout + h))
    q = _q(dtype)
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    x = q(torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)))
    wt = q(torch.from_numpy((rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2.0 / (cin * ks * ks))).astype(np.float32)))
    bt = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32))
    r = q(torch.from_numpy(rng.standard_normal((n, cout, ho, wo)).astype(np.float32))) if res else None
    ref = F.conv2d(x.double(), wt.double(), bt.double(), stride=stride, padding=pad)
    if r is not None:
        ref = ref + r.double()
    if relu:
        ref = F.relu(ref)
    else:
        assert float(ref.min()) < 0
    wp = wt.permute(2, 3, 0, 1).reshape(ks * ks, cout, cin).contiguous()
    if dtype == "f16x2":                                   # the weight-stationary kernels, as the planner packs them
        packed, wexp = f16x2.pack_weights_ws(wp)
        d_w = packed.cuda()
    else:
        d_w, wexp = wp.cuda(), 0
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, int(relu)
    op.cin, op.cout, op.cout_pad = cin, cout, cout
    op.hin, op.win, op.hout, op.wout = h, w, ho, wo
    op.wfmt, op.wexp = int(dtype == "f16x2"), wexp
    out = _nan_out(dtype, n, ho, wo, cout)
    _run(op, dtype, n, _nhwc(x, dtype), d_w, bt.cuda(), out, res=_nhwc(r, dtype) if res else None)
    _conv_gate("conv k%ds%d %d-%d %dx%d %s" % (ks, stride, cin, cout, h, w, dtype), _read(out, dtype), ref.numpy(), dtype)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("h,w", [(8, 6), (4, 3)])
def test_deconv_from_512_channels(h, w, dtype):
    cin, cout, n = 512, 256, 3
    rng = np.random.Generator(np.random.PCG64(cin + h))
    q = _q(dtype)
    x = q(torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)))
    wt = q(torch.from_numpy((rng.standard_normal((cin, cout, 4, 4)) * np.sqrt(2.0 / (cin * 4))).astype(np.float32)))
    ref = F.relu(F.conv_transpose2d(x.double(), wt.double(), None, stride=2, padding=1))
    if dtype == "f16x2":
        packed, wexp = f16x2.pack_deconv_weights_ws(wt, cout)
        d_w = packed.cuda()
    else:
        d_w, wexp = f16x2.deconv_phase_taps(wt, cout).contiguous().cuda(), 0
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DECONV, 4, 2, 1
    op.cin, op.cout, op.cout_pad = cin, cout, cout
    op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
    op.wfmt, op.wexp = int(dtype == "f16x2"), wexp
    out = _nan_out(dtype, n, 2 * h, 2 * w, cout)
    _run(op, dtype, n, _nhwc(x, dtype), d_w, torch.zeros(cout).cuda(), out)
    _conv_gate("deconv 512-256 %dx%d %s" % (h, w, dtype), _read(out, dtype), ref.numpy(), dtype)
