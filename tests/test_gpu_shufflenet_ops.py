"""The two ops pose_shufflenetv2_10x_pixel_shuffle adds, through udp_conv2d_fused: UDP_OP_DWCONV (depthwise 3x3 conv +
folded BatchNorm, with the ShuffleV2 passthrough) and UDP_OP_PIXSHUF (PixelShuffle(2)), include/udp_pose_hip.h.

Outputs are pre-filled with NaN and operands are quantised to the storage mode first.  The conv is new arithmetic:
|hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp relative to the tensor's max (tests/test_gpu_program_ops.py), ulp = 2^-23
(fp32) / 2^-21 (split fp16).  The passthrough and the pixel shuffle move bit patterns: equality."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21}


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


def _dw_op(c, h, w, stride, relu):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, 3, stride, int(relu)
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, (h - 1) // stride + 1, (w - 1) // stride + 1
    return op


def _dw_data(c, h, w, n, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = _q(dtype)(torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32)))
    wt = torch.from_numpy((rng.standard_normal((c, 1, 3, 3)) * np.sqrt(2.0 / 9)).astype(np.float32))    # fp32 in every mode
    bt = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32))
    return x, wt, bt, wt.reshape(c, 9).t().contiguous().cuda()                                             # [9][C], tap-major


def _dw_ref(x, wt, bt, stride, relu, dt):
    y = F.conv2d(x.to(dt), wt.to(dt), bt.to(dt), stride=stride, padding=1, groups=x.shape[1])
    return F.relu(y) if relu else y


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5), (8, 6), (16, 12)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", [32, 64, 96, 256])
def test_dwconv_matches_conv2d_fp64(c, hw, stride, n, relu, dtype):
    h, w = hw
    x, wt, bt, d_w = _dw_data(c, h, w, n, dtype, c + 10 * h + stride + n)
    op = _dw_op(c, h, w, stride, relu)
    out = _nan(dtype, n, op.hout, op.wout, c)
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), d_w, bt.cuda(), out) == 0, _lib.lib().udp_last_error()
    got = _host(out, dtype).permute(0, 3, 1, 2)
    assert tuple(got.shape) == (n, c, (h - 1) // stride + 1, (w - 1) // stride + 1)
    e_hip, _, gate = mp.parity("dwconv C%d %dx%d s%d n%d relu%d %s" % (c, h, w, stride, n, relu, dtype), got,
                               _dw_ref(x, wt, bt, stride, relu, torch.float64), _dw_ref(x, wt, bt, stride, relu, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_channel_views(stride, dtype):
    """64 channels from offset 32 of a 128-pitch input into offset 64 of a 128-pitch output; the rest of the output
    tensor keeps its bit pattern."""
    c, h, w, n = 64, 7, 5, 3
    x, wt, bt, d_w = _dw_data(128, h, w, n, dtype, 77 + stride)
    wt, bt, d_w = wt[:c], bt[:c], d_w[:, :c].contiguous()
    op = _dw_op(c, h, w, stride, False)
    op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = 32, 128, 64, 128
    out = _nan(dtype, n, op.hout, op.wout, 128)
    before = _bits(out).clone()
    assert _call(op, dtype, n, _dev(x.permute(0, 2, 3, 1), dtype), d_w, bt.cuda(), out) == 0, _lib.lib().udp_last_error()
    got = _host(out, dtype)[..., 64:128].permute(0, 3, 1, 2)
    xs = x[:, 32:96]
    e_hip, _, gate = mp.parity("dwconv views s%d %s" % (stride, dtype), got, _dw_ref(xs, wt, bt, stride, False, torch.float64),
                               _dw_ref(xs, wt, bt, stride, False, torch.float32), ULP[dtype])
    assert e_hip <= gate, (e_hip, gate)
    assert torch.equal(_bits(out)[..., :64], before[..., :64])


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("c,r", [(64, 58), (32, 24)])
def test_dwconv_shuffle_passthrough_is_a_selection(c, r, dtype):
    """n_out2 = 1: the launch also copies the even logical channels of the unit input (two halves of c stored channels,
    r real ones each) to the first half of the unit output -- bit for bit, zeros in the pad, nothing else touched."""
    h, w, n = 7, 5, 3
    x, wt, bt, d_w = _dw_data(c, h, w, n, dtype, 5 * c + r)
    rng = np.random.Generator(np.random.PCG64(r))
    src = _dev(torch.from_numpy(rng.standard_normal((n, h, w, 2 * c)).astype(np.float32)), dtype)     # pads non-zero on purpose
    dst = _nan(dtype, n, h, w, 2 * c)
    before = _bits(dst).clone()
    op = _dw_op(c, h, w, 1, False)
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
    got = _host(out, dtype).permute(0, 3, 1, 2)                              # the conv of the same launch is unchanged
    e_hip, _, gate = mp.parity("dwconv + passthrough C%d %s" % (c, dtype), got, _dw_ref(x, wt, bt, 1, False, torch.float64),
                               _dw_ref(x, wt, bt, 1, False, torch.float32), ULP[dtype])
    assert e_hip <= gate


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("case", [(128, 4, 3), (512, 8, 6), (128, 1, 1)], ids=lambda s: "%d_%dx%d" % s)
def test_pixel_shuffle_bit_for_bit(case, dtype):
    cin, h, w = case
    n, cq = 3, cin // 4
    rng = np.random.Generator(np.random.PCG64(cin + h))
    x = _q(dtype)(torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)))
    want = F.pixel_shuffle(x, 2)                                             # of the un-permuted tensor
    perm = torch.tensor([4 * (p % cq) + p // cq for p in range(cin)])        # stored position g * cq + c holds channel 4c + g
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride = _lib.UDP_OP_PIXSHUF, 1, 1
    op.cin, op.cout, op.cout_pad = cin, cq, (cq + 31) // 32 * 32
    op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
    out = _nan(dtype, n, 2 * h, 2 * w, cq)
    assert _call(op, dtype, n, _dev(x[:, perm].permute(0, 2, 3, 1), dtype), None, None, out) == 0, _lib.lib().udp_last_error()
    assert torch.equal(_bits(out), _bits(_dev(want.permute(0, 2, 3, 1), dtype)))


def test_rejections():
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    args = (1, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), None, None, None, None, _lib.ptr(buf[1 << 19:]), _lib.stream_ptr())
    lib = _lib.lib()
    op = _dw_op(64, 8, 6, 2, False)
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_BF16, *args) == -3                 # UDP_ERR_UNSUPPORTED
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_F32, *args) == 0
    op.hout = 5
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_F32, *args) == -1                  # UDP_ERR_ARG: hout != (hin - 1) / 2 + 1
    op = _dw_op(48, 8, 6, 1, False)
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_F32, *args) == -1                  # C is no multiple of 32
    ps = _lib.ConvOp()
    ps.kind, ps.ks, ps.stride, ps.cin, ps.cout, ps.cout_pad, ps.hin, ps.win, ps.hout, ps.wout = _lib.UDP_OP_PIXSHUF, 1, 1, 128, 32, 32, 4, 3, 8, 6
    assert lib.udp_conv2d_fused(C.byref(ps), _lib.UDP_BF16, *args) == -3
    ps.hout = 7
    assert lib.udp_conv2d_fused(C.byref(ps), _lib.UDP_F16X2, *args) == -1
    torch.cuda.synchronize()
