"""The kernels pose_resnet's training step adds (csrc/resnet_train.hip and the ks 4 / 7 arms of csrc/train.hip), op by
op against torch in fp64 on the CPU: the transposed conv's forward from packed raw weights, its input gradient
(udp_deconv4s2_dgrad) and weight gradient (udp_conv2d_wgrad, ks 4), the max-pool pair, the 7x7 stem on unfolded weights
with its weight gradient (ks 7), and the 1x1 stride-2 projection shortcut's two gradients.

Tolerances are those of tests/test_gpu_train.py: forward 1e-4 * max|ref|, input gradient 2e-4 * max|ref|, weight
gradient 1e-4 * max|ref| (3e-4 for the accumulate = 1 second call against 2 * ref).  Every output buffer starts as NaN,
so an element no kernel writes fails the comparison."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from udp_pose_amd import _lib, f16x2                                 # noqa: E402

F32 = _lib.UDP_F32


def _rup(x, m):
    return (x + m - 1) // m * m


def _rand(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _nhwc(t, pitch=None):
    """NCHW host tensor -> NHWC fp32 on the device, channels zero-padded to ``pitch``."""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, pitch or c, dtype=torch.float32)
    out[..., :c] = t.permute(0, 2, 3, 1).to(torch.float32)
    return out.cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _nchw(t, c=None):
    """NHWC device tensor -> NCHW fp64 on the host (the first ``c`` channels)."""
    t = t.cpu().double()
    return (t if c is None else t[..., :c]).permute(0, 3, 1, 2).numpy()


def _gate(got, ref, rel, what):
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), "%s: output not fully written" % what
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max err %.3g, max|ref| %.3g, gate %.3g" % (what, err, scale, rel * scale))
    assert err <= rel * scale, (what, err, scale)


def _wgrad(x, dy, n, hin, win, cin_k, hout, wout, cout_k, ks, stride, cout, cin, dw, accumulate):
    L = _lib.lib()
    nbytes = int(L.udp_conv2d_wgrad_workspace_bytes(cout, cin, ks))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.udp_conv2d_wgrad(_lib.ptr(x), _lib.ptr(dy), n, hin, win, cin_k, hout, wout, cout_k, ks, stride, cout, cin,
                                  F32, _lib.ptr(dw), accumulate, _lib.ptr(ws), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()


def _conv_op(kind, ks, stride, cin, cout, hin, win, hout, wout):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = kind, ks, stride, 0
    op.cin, op.cout, op.cout_pad = cin, cout, _rup(cout, 32)
    op.hin, op.win, op.hout, op.wout = hin, win, hout, wout
    op.in_buf = op.res_buf = _lib.UDP_BUF_NONE
    return op


def _fused(op, n, x, w, b, out):
    _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), F32, n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), None, None, None, None,
                                           _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the transposed conv
#                (cin, cout, h, w, n)
DECONV_CASES = [(16, 8, 1, 1, 1),          # one pixel: every tap meets the border
                (32, 40, 3, 5, 2),         # cout not a multiple of 32, odd sizes
                (64, 32, 8, 6, 2),
                (272, 24, 4, 3, 1),        # K-chunk tails on both sides
                (2048, 256, 2, 2, 1)]      # the real channel counts
_ids = lambda s: "%d-%d_%dx%d_n%d" % s     # noqa: E731


@functools.lru_cache(maxsize=None)
def _deconv_ref(case, bias):
    cin, cout, h, w, n = case
    rng = np.random.Generator(np.random.PCG64(cin * 7 + cout + h))
    x = _rand(rng, n, cin, h, w)
    wt = _rand(rng, cin, cout, 4, 4, scale=np.sqrt(2.0 / (cin * 4)))
    bt = _rand(rng, cout, scale=0.1) if bias else None
    dy = _rand(rng, n, cout, 2 * h, 2 * w)
    xd, wd = x.double().requires_grad_(), wt.double().requires_grad_()
    bd = bt.double().requires_grad_() if bias else None
    y = F.conv_transpose2d(xd, wd, bd, stride=2, padding=1)
    y.backward(dy.double())
    ref = {"y": y.detach().numpy(), "dx": xd.grad.numpy(), "dw": wd.grad.numpy(), "db": bd.grad.numpy() if bias else None}
    return x, wt, bt, dy, ref


def _deconv_pack(wt):
    cin, cout = wt.shape[:2]
    fwd = _nan(16 * _rup(cout, 32) * cin)
    dg = _nan(16 * _rup(cin, 32) * _rup(cout, 16))
    wdev = wt.contiguous().cuda()
    _lib.check(_lib.lib().udp_pack_conv_weights(_lib.ptr(wdev), cout, cin, 4, F32, _lib.ptr(fwd), _lib.ptr(dg), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return fwd, dg


@pytest.mark.parametrize("case", DECONV_CASES, ids=_ids)
def test_deconv_pack_layouts(case):
    """Both packed operands against their definitions (include/udp_pose_hip.h), bit for bit, padding zero."""
    cin, cout = case[:2]
    _, wt, _, _, _ = _deconv_ref(case, False)
    fwd, dg = _deconv_pack(wt)
    want = f16x2.deconv_phase_taps(wt, _rup(cout, 32))
    assert torch.equal(fwd.cpu().view_as(want), want)
    wd = torch.zeros(16, _rup(cin, 32), _rup(cout, 16))
    wd[:, :cin, :cout] = wt.permute(2, 3, 0, 1).reshape(16, cin, cout)
    assert torch.equal(dg.cpu().view_as(wd), wd)


def _deconv_forward(case, bias):
    cin, cout, h, w, n = case
    x, wt, bt, dy, ref = _deconv_ref(case, bias)
    fwd, _ = _deconv_pack(wt)
    bp = torch.zeros(_rup(cout, 32))
    if bias:
        bp[:cout] = bt
    out = _nan(n, 2 * h, 2 * w, cout)
    _fused(_conv_op(_lib.UDP_OP_DECONV, 4, 2, cin, cout, h, w, 2 * h, 2 * w), n, _nhwc(x), fwd, bp.cuda(), out)
    _gate(_nchw(out), ref["y"], 1e-4, "deconv forward")


@pytest.mark.parametrize("case", DECONV_CASES, ids=_ids)
def test_deconv_forward_from_packed_raw_weights(case):
    _deconv_forward(case, False)


def test_deconv_with_bias_and_its_gradient():
    """DECONV_WITH_BIAS: the bias row in the forward, udp_bias_grad over dY for its gradient."""
    case = DECONV_CASES[2]
    cin, cout, h, w, n = case
    _deconv_forward(case, True)
    _, _, _, dy, ref = _deconv_ref(case, True)
    db = _nan(cout)
    g = _nhwc(dy)
    _lib.check(_lib.lib().udp_bias_grad(_lib.ptr(g), n * 4 * h * w, cout, cout, _lib.ptr(db), F32, _lib.stream_ptr()))
    torch.cuda.synchronize()
    _gate(db.cpu().double().numpy(), ref["db"], 1e-4, "deconv bias gradient")


@pytest.mark.parametrize("case", DECONV_CASES, ids=_ids)
def test_deconv_input_gradient(case):
    cin, cout, h, w, n = case
    x, wt, _, dy, ref = _deconv_ref(case, False)
    _, dg = _deconv_pack(wt)
    dx = _nan(n, h, w, cin)
    g = _nhwc(dy)
    _lib.check(_lib.lib().udp_deconv4s2_dgrad(_lib.ptr(g), _lib.ptr(dg), n, h, w, cin, cin, cout, cout, F32, _lib.ptr(dx),
                                              _lib.stream_ptr()))
    torch.cuda.synchronize()
    _gate(_nchw(dx), ref["dx"], 2e-4, "deconv input gradient")


def test_deconv_input_gradient_padded_pitches():
    """dy in a pitch of 48 for 40 channels (the trainer's NHWC16 maps): the pad is never read as data."""
    case = DECONV_CASES[1]
    cin, cout, h, w, n = case
    x, wt, _, dy, ref = _deconv_ref(case, False)
    _, dg = _deconv_pack(wt)
    g = _nhwc(dy, 48)
    g[..., cout:] = 1e30
    dx = _nan(n, h, w, cin)
    _lib.check(_lib.lib().udp_deconv4s2_dgrad(_lib.ptr(g), _lib.ptr(dg), n, h, w, cin, cin, cout, 48, F32, _lib.ptr(dx),
                                              _lib.stream_ptr()))
    torch.cuda.synchronize()
    _gate(_nchw(dx), ref["dx"], 2e-4, "deconv input gradient (pitch 48)")


@pytest.mark.parametrize("case", DECONV_CASES, ids=_ids)
def test_deconv_weight_gradient(case):
    """udp_conv2d_wgrad with ks 4: `x` = dY, `dy` = the deconv's input; the result is ConvTranspose2d.weight's layout."""
    cin, cout, h, w, n = case
    x, wt, _, dy, ref = _deconv_ref(case, False)
    dw = _nan(cin, cout, 4, 4)
    g, xi = _nhwc(dy), _nhwc(x)
    _wgrad(g, xi, n, 2 * h, 2 * w, cout, h, w, cin, 4, 2, cin, cout, dw, 0)
    _gate(dw.cpu().double().numpy(), ref["dw"], 1e-4, "deconv weight gradient")
    _wgrad(g, xi, n, 2 * h, 2 * w, cout, h, w, cin, 4, 2, cin, cout, dw, 1)
    _gate(dw.cpu().double().numpy(), 2 * ref["dw"], 3e-4, "deconv weight gradient, accumulated")


# ------------------------------------------------------------------ max-pool
@pytest.mark.parametrize("shape", [(8, 6, 16, 2), (7, 5, 16, 1), (2, 2, 64, 1), (1, 9, 16, 1)], ids=lambda s: "%dx%dx%d_n%d" % s)
def test_maxpool_forward_and_backward_equal_torch(shape):
    """Integers 0..3 after a ReLU: most windows hold ties, so the first-maximum rule decides where dy goes."""
    h, w, c, n = shape
    rng = np.random.Generator(np.random.PCG64(h * 31 + w))
    x = torch.from_numpy(rng.integers(-3, 4, (n, c, h, w)).clip(0, 3).astype(np.float32))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.from_numpy(rng.integers(-4, 5, (n, c, ho, wo)).astype(np.float32))
    xd = x.double().requires_grad_()
    yr = F.max_pool2d(xd, 3, 2, 1)
    yr.backward(dy.double())
    L = _lib.lib()
    xg, y, dx = _nhwc(x), _nan(n, ho, wo, c), _nan(n, h, w, c)
    _lib.check(L.udp_maxpool3s2_fwd(_lib.ptr(xg), n, h, w, c, F32, _lib.ptr(y), _lib.stream_ptr()))
    g = _nhwc(dy)
    _lib.check(L.udp_maxpool3s2_bwd(_lib.ptr(xg), _lib.ptr(g), n, h, w, c, F32, _lib.ptr(dx), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(_nchw(y), yr.detach().numpy())
    assert np.array_equal(_nchw(dx), xd.grad.numpy())


# ------------------------------------------------------------------ the stem
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 3, 64, 32)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_stem_forward_and_weight_gradient(shape):
    n, _, h, w = shape
    rng = np.random.Generator(np.random.PCG64(h + w))
    x = _rand(rng, n, 3, h, w)
    wt = _rand(rng, 64, 3, 7, 7, scale=np.sqrt(2.0 / 147))
    ho, wo = h // 2, w // 2
    dy = _rand(rng, n, 64, ho, wo)
    wd = wt.double().requires_grad_()
    yr = F.conv2d(x.double(), wd, None, stride=2, padding=3)
    yr.backward(dy.double())
    L = _lib.lib()
    img = _nan(n, h, w, 16)
    xdev = x.contiguous().cuda()
    _lib.check(L.udp_nchw_to_nhwc(_lib.ptr(xdev), n, 3, h, w, 16, _lib.ptr(img), F32, _lib.stream_ptr()))
    wdev, wf = wt.contiguous().cuda(), _nan(49 * 64 * 16)
    _lib.check(L.udp_pack_conv_weights(_lib.ptr(wdev), 64, 3, 7, F32, _lib.ptr(wf), None, _lib.stream_ptr()))
    y = _nan(n, ho, wo, 64)
    _lib.check(L.udp_stem7_train_fwd(_lib.ptr(img), _lib.ptr(wf), n, h, w, 16, 64, F32, _lib.ptr(y), _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = torch.zeros(49, 64, 16)
    want[:, :, :3] = wt.permute(2, 3, 0, 1).reshape(49, 64, 3)
    assert torch.equal(wf.cpu().view_as(want), want)
    _gate(_nchw(y), yr.detach().numpy(), 1e-4, "stem forward")
    dw = _nan(64, 3, 7, 7)
    _wgrad(img, _nhwc(dy), n, h, w, 16, ho, wo, 64, 7, 2, 64, 3, dw, 0)
    _gate(dw.cpu().double().numpy(), wd.grad.numpy(), 1e-4, "stem weight gradient")


# ------------------------------------------------------------------ the 1x1 stride-2 projection shortcut
@pytest.mark.parametrize("case", [(32, 64, 6, 4, 2), (64, 128, 8, 8, 2)], ids=_ids)
def test_conv1x1_stride2_gradients(case):
    """downsample.0 of a strided Bottleneck (pose_resnet.py:136-141): the input gradient is a 1x1 conv over dy read as
    its zero-stuffed image (udp_conv_op.in_stuff2), the weight gradient udp_conv2d_wgrad with ks 1, stride 2."""
    cin, cout, h, w, n = case
    rng = np.random.Generator(np.random.PCG64(cin + cout))
    x = _rand(rng, n, cin, h, w)
    wt = _rand(rng, cout, cin, 1, 1, scale=np.sqrt(2.0 / cin))
    ho, wo = h // 2, w // 2
    dy = _rand(rng, n, cout, ho, wo)
    xd, wd = x.double().requires_grad_(), wt.double().requires_grad_()
    yr = F.conv2d(xd, wd, None, stride=2)
    yr.backward(dy.double())
    L = _lib.lib()
    wdev = wt.contiguous().cuda()
    wf, wg = _nan(_rup(cout, 32) * _rup(cin, 16)), _nan(_rup(cin, 32) * _rup(cout, 16))
    _lib.check(L.udp_pack_conv_weights(_lib.ptr(wdev), cout, cin, 1, F32, _lib.ptr(wf), _lib.ptr(wg), _lib.stream_ptr()))
    xg, g = _nhwc(x), _nhwc(dy)
    y = _nan(n, ho, wo, cout)
    zeros = torch.zeros(max(_rup(cout, 32), _rup(cin, 32)), device="cuda")
    _fused(_conv_op(_lib.UDP_OP_CONV, 1, 2, cin, cout, h, w, ho, wo), n, xg, wf, zeros, y)
    _gate(_nchw(y), yr.detach().numpy(), 1e-4, "1x1 stride-2 forward")
    dx = _nan(n, h, w, cin)
    dop = _conv_op(_lib.UDP_OP_CONV, 1, 1, cout, cin, 2 * ho, 2 * wo, h, w)
    dop.in_stuff2 = 1
    _fused(dop, n, g, wg, zeros, dx)
    _gate(_nchw(dx), xd.grad.numpy(), 2e-4, "1x1 stride-2 input gradient")
    dw = _nan(cout, cin, 1, 1)
    _wgrad(xg, g, n, h, w, cin, ho, wo, cout, 1, 2, cout, cin, dw, 0)
    _gate(dw.cpu().double().numpy(), wd.grad.numpy(), 1e-4, "1x1 stride-2 weight gradient")
