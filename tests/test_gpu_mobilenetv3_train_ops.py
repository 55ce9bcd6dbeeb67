"""The MobileNetV3 training kernels (csrc/dw_train.hip, csrc/mobilenetv3_train.hip), one entry point at a time, against fp64 autograd of
the same op on the CPU: depthwise 3x3 / 5x5 forward, input gradient and weight gradient (F.conv2d(groups=C)), hard-swish
(x * clamp(x + 3, 0, 6) / 6, which is F.hardswish) and the squeeze-and-excitation with biases (the formula of tests/mobilenetv3_ref.py:squeeze_excitation;
torchvision is not installed, so its own module cannot be the arbiter), at the smallest shapes where each can go wrong.

Every output lives in an arena of one NaN bit pattern between two guards (tests/test_gpu_train_arms.py): it must come
back fully written and the guards untouched.  The gate is the rule of tests/test_gpu_shufflenet_train.py, measured and
not chosen: ours may be at most 4 x as far from fp64 as torch's fp32 CPU run of the same op is, or 1e-4 * max|ref| where
that is more (fp32 CPU error can be zero on tiny tensors).  Pads of every output are exactly zero, two runs are
bit-identical."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_gpu_train_arms import Arena                     # noqa: E402
from udp_pose_amd import _lib                             # noqa: E402

F32 = _lib.UDP_F32
CHANNELS = [(48, 40), (80, 72), (16, 16)]                  # stored / real
MAPS = [(1, 1), (2, 3), (7, 9)]                            # 2x3: smaller than the kernel's reach; 7x9 -> 4x5: the odd stride-2 case


def _s():
    return _lib.stream_ptr()


def _ok(rc):
    assert rc == 0, _lib.lib().udp_last_error()


def _nhwc(t, pitch):
    """NCHW fp64 (exactly fp32-representable values) -> device NHWC fp32 with zero pads."""
    n, c, h, w = t.shape
    o = torch.zeros(n, h, w, pitch, dtype=torch.float32)
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
    gate = max(4 * e_f32, 1e-4 * mx)
    print("%-46s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (name, mx, e_f32, e_ours, gate))
    assert e_ours <= gate, (name, e_ours, gate)


def _pads_zero(t, pitch, real):
    return pitch == real or float(t.view(-1, pitch)[:, real:].abs().max()) == 0.0


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ depthwise K x K
def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _dw_fwd(x, wt, cs, ks, s):
    n, cr, h, w = x.shape
    ho, wo = _out_hw(h, w, s)
    out = Arena(n * ho * wo * cs)
    xd, wd = _nhwc(x, cs), wt.float().contiguous().cuda()          # (held until the result has been read)
    _ok(_lib.lib().udp_dwconvk_train_fwd(xd.data_ptr(), wd.data_ptr(), n, h, w, cs, cr, ks, s, F32, out.ptr(), _s()))
    return out.get("dwk fwd")


def _dw_dgrad(dy, wt, cs, ks, s, h, w, prev=None):
    n, cr, ho, wo = dy.shape
    out = Arena(n * h * w * cs)
    if prev is not None:
        out.t.copy_(_nhwc(prev, cs).reshape(-1))
    dd, wd = _nhwc(dy, cs), wt.float().contiguous().cuda()
    _ok(_lib.lib().udp_dwconvk_dgrad(dd.data_ptr(), wd.data_ptr(), n, h, w, cs, cr, ks, s, int(prev is not None), F32,
                                     out.ptr(), _s()))
    return out.get("dwk dgrad")


def _dw_wgrad(x, dy, cs, ks, s, ws_bytes=None):
    n, cr, h, w = x.shape
    ho, wo = dy.shape[2:]
    L = _lib.lib()
    full = int(L.udp_dwconvk_wgrad_workspace_bytes(n, ho, wo, cs, ks))
    rows = -(-n * ho // min(n * ho, 256))
    assert full == -(-n * ho // rows) * ks * ks * cs * 4                # partials = ceil(n*hout / rows) of [ks^2][c] floats
    if ws_bytes is None:
        ws_bytes = full
    ws = Arena(ws_bytes // 4)
    out = Arena(cr * ks * ks)
    xd, dd = _nhwc(x, cs), _nhwc(dy, cs)
    _ok(L.udp_dwconvk_wgrad(xd.data_ptr(), dd.data_ptr(), n, h, w, cs, cr, ks, s, F32, out.ptr(), ws.ptr(), ws_bytes, _s()))
    ws.check("dwk wgrad workspace")
    return out.get("dwk wgrad").view(cr, 1, ks, ks)


def _dw_ref(x, wt, dy, s, dtype):
    """(y, dx, dw) of F.conv2d(groups=C) + autograd in ``dtype`` on the CPU."""
    x = x.to(dtype).requires_grad_(True)
    wt = wt.to(dtype).requires_grad_(True)
    y = F.conv2d(x, wt, None, stride=s, padding=wt.shape[2] // 2, groups=x.shape[1])
    dx, dw = torch.autograd.grad(y, [x, wt], dy.to(dtype))
    return y.detach(), dx, dw


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ks", [3, 5])
def test_dw_forward_dgrad_and_wgrad_against_fp64(ks, stride):
    gen = torch.Generator().manual_seed(100 * ks + stride)
    for cs, cr in CHANNELS:
        for h, w in MAPS:
            for n in (1, 3):
                ho, wo = _out_hw(h, w, stride)
                x, wt = _rand(gen, n, cr, h, w), _rand(gen, cr, 1, ks, ks)
                dy, prev = _rand(gen, n, cr, ho, wo), _rand(gen, n, cr, h, w)
                y64, dx64, dw64 = _dw_ref(x, wt, dy, stride, torch.float64)
                y32, dx32, dw32 = _dw_ref(x, wt, dy, stride, torch.float32)
                tag = "k%d s%d C%d(%d) %dx%dx%d" % (ks, stride, cs, cr, n, h, w)
                y = _dw_fwd(x, wt, cs, ks, stride)
                _gate("dwk fwd " + tag, _nchw(y, n, ho, wo, cs, cr), y64, y32)
                assert _pads_zero(y, cs, cr), tag
                assert _same_bits(_dw_fwd(x, wt, cs, ks, stride), y), tag
                for acc in (0, 1):
                    dx = _dw_dgrad(dy, wt, cs, ks, stride, h, w, prev if acc else None)
                    want64, want32 = (dx64 + prev, dx32 + prev.float()) if acc else (dx64, dx32)
                    _gate("dwk dgrad acc%d %s" % (acc, tag), _nchw(dx, n, h, w, cs, cr), want64, want32)
                    assert _pads_zero(dx, cs, cr), tag
                    assert _same_bits(_dw_dgrad(dy, wt, cs, ks, stride, h, w, prev if acc else None), dx), tag
                for ws_bytes in (None, 2 * ks * ks * cs * 4):          # the full split; room for two partials
                    dw = _dw_wgrad(x, dy, cs, ks, stride, ws_bytes)
                    _gate("dwk wgrad ws %s %s" % (ws_bytes, tag), dw, dw64, dw32)
                    assert _same_bits(_dw_wgrad(x, dy, cs, ks, stride, ws_bytes), dw), tag


def _replay_parent_bits(g):
    """udp_dwconvk_*(ks=3) on the recorded inputs of tests/golden/dw3_train_parent_bits.npz (tools/gen_golden_dw3_parent.py:
    int32 bit patterns of NHWC fp32 buffers): {name: int32 array} under the fixture's own output names."""
    L = _lib.lib()

    def dev(name):
        return torch.from_numpy(g[name]).cuda().view(torch.float32)

    def bits(arena, what):
        return arena.get(what).view(torch.int32).numpy().reshape(-1)

    got = {}
    n, h, w, cs, cr = 3, 7, 9, 32, 24
    x, prev, wt = dev("a_x"), dev("a_prev"), dev("a_w")
    for s in (1, 2):
        ho, wo = _out_hw(h, w, s)
        dy = dev("a_dy_s%d" % s)
        y, dx0, dx1, dw = Arena(n * ho * wo * cs), Arena(n * h * w * cs), Arena(n * h * w * cs), Arena(cr * 9)
        dx1.t.copy_(prev.reshape(-1))
        ws_bytes = int(L.udp_dwconvk_wgrad_workspace_bytes(n, ho, wo, cs, 3))
        ws = Arena(ws_bytes // 4)
        _ok(L.udp_dwconvk_train_fwd(x.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, 3, s, F32, y.ptr(), _s()))
        _ok(L.udp_dwconvk_dgrad(dy.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, 3, s, 0, F32, dx0.ptr(), _s()))
        _ok(L.udp_dwconvk_dgrad(dy.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, 3, s, 1, F32, dx1.ptr(), _s()))
        _ok(L.udp_dwconvk_wgrad(x.data_ptr(), dy.data_ptr(), n, h, w, cs, cr, 3, s, F32, dw.ptr(), ws.ptr(), ws_bytes, _s()))
        ws.check("dwk wgrad workspace")
        got.update({"a_y_s%d" % s: bits(y, "fwd"), "a_dx_acc0_s%d" % s: bits(dx0, "dgrad"), "a_dx_acc1_s%d" % s: bits(dx1, "dgrad acc"),
                    "a_dw_s%d" % s: bits(dw, "wgrad")})
    cs, cr = 64, 58
    x, dy, dw, ws_bytes = dev("b_x"), dev("b_dy"), Arena(cr * 9), 5 * 9 * cs * 4           # 21 rows in runs of 5, 5, 5, 5, 1
    ws = Arena(ws_bytes // 4)
    _ok(L.udp_dwconvk_wgrad(x.data_ptr(), dy.data_ptr(), n, h, w, cs, cr, 3, 1, F32, dw.ptr(), ws.ptr(), ws_bytes, _s()))
    ws.check("dwk wgrad workspace")
    got["b_dw_ws5"] = bits(dw, "wgrad ws5")
    return got


@pytest.mark.parametrize("ks", [3, 5])
def test_dw_k3_arm_is_the_3x3_kernel_and_many_rows_split(ks, golden_dir):
    """More output rows than partials fit (320 rows: the 256 cap -> runs of 2), several blocks of strips; and for K = 3
    the recorded outputs of the one-pixel-per-thread 3x3 kernels this family replaced (udp_dwconv3_*, recorded from the
    library that had them), bit for bit: forward, input gradient with and without accumulation and weight gradient at
    both strides, and the weight gradient under a workspace that limits the split (the same fmaf order per element, the
    same lane-order and index-order sums)."""
    gen = torch.Generator().manual_seed(7 + ks)
    cs, cr, n, h, w = 48, 40, 40, 8, 10
    x, wt, dy = _rand(gen, n, cr, h, w), _rand(gen, cr, 1, ks, ks), _rand(gen, n, cr, h, w)
    y64, dx64, dw64 = _dw_ref(x, wt, dy, 1, torch.float64)
    y32, dx32, dw32 = _dw_ref(x, wt, dy, 1, torch.float32)
    y, dx, dw = _dw_fwd(x, wt, cs, ks, 1), _dw_dgrad(dy, wt, cs, ks, 1, h, w), _dw_wgrad(x, dy, cs, ks, 1)
    _gate("dwk fwd k%d 40x8x10" % ks, _nchw(y, n, h, w, cs, cr), y64, y32)
    _gate("dwk dgrad k%d 40x8x10" % ks, _nchw(dx, n, h, w, cs, cr), dx64, dx32)
    _gate("dwk wgrad k%d 40x8x10" % ks, dw, dw64, dw32)
    if ks == 3:
        g = np.load(os.path.join(golden_dir, "dw3_train_parent_bits.npz"))
        got = _replay_parent_bits(g)
        assert len(got) == 9 and all(float(np.abs(g[k].view(np.float32)).max()) > 0 for k in got)       # a record of something
        differ = [(k, int((got[k] != g[k].reshape(-1)).sum())) for k in got if not np.array_equal(got[k], g[k].reshape(-1))]
        assert not differ, differ


# ------------------------------------------------------------------ hard-swish
def _hswish_vector():
    three = torch.tensor(3.0)
    edge = [torch.nextafter(three, torch.tensor(0.0)), torch.nextafter(three, torch.tensor(9.0))]
    special = torch.tensor([-3.0, 0.0, 3.0, float(edge[0]), float(edge[1]), -float(edge[0]), -float(edge[1]), 1e4, -1e4, 65536.0,
                            -7.5, 2.5])
    gen = torch.Generator().manual_seed(3)
    return torch.cat([special, torch.randn(1004 - special.numel(), generator=gen) * 3])        # 1004 = 4 * 251, not a multiple of 256


@pytest.mark.parametrize("count", [4, 1004])
def test_hswish_forward_and_backward(count):
    L = _lib.lib()
    x = _hswish_vector()[:count].clone()
    dy = torch.randn(count, generator=torch.Generator().manual_seed(4))
    refs = []
    for dtype in (torch.float64, torch.float32):                  # the op as the header states it: x * clamp(x + 3, 0, 6) / 6
        xr = x.to(dtype).requires_grad_(True)
        yr = xr * torch.clamp(xr + 3, 0, 6) / 6
        refs.append((yr.detach(), torch.autograd.grad(yr, xr, dy.to(dtype))[0]))
    # F.hardswish is the same function, and the same derivative away from the two kinks; AT x = -3 and x = 3 this torch's
    # hardswish_backward takes the outer pieces (0 and dy) where the clamp form, the kernel and the restatement of the
    # net (tests/mobilenetv3_train_ref.py) take the inner one
    xr = x.double().requires_grad_(True)
    yh = F.hardswish(xr)
    dh = torch.autograd.grad(yh, xr, dy.double())[0]
    off_kink = x.abs() != 3
    assert float((yh.detach() - refs[0][0]).abs().max()) <= 1e-12 * float(refs[0][0].abs().max())
    assert float((dh - refs[0][1])[off_kink].abs().max()) <= 1e-12
    xd, dd = x.cuda(), dy.cuda()
    runs = []
    for _ in range(2):
        y, dx = Arena(count), Arena(count)
        _ok(L.udp_hswish_fwd(xd.data_ptr(), y.ptr(), count, _s()))
        _ok(L.udp_hswish_bwd(dd.data_ptr(), xd.data_ptr(), dx.ptr(), count, _s()))
        runs.append((y.get("hswish fwd"), dx.get("hswish bwd")))
    (y, dx), again = runs
    _gate("hswish fwd %d" % count, y, refs[0][0], refs[1][0])
    _gate("hswish bwd %d" % count, dx, refs[0][1], refs[1][1])
    assert _same_bits(again[0], y) and _same_bits(again[1], dx)
    # the three pieces at the kinks themselves: x = -3 -> (0, -0.5 dy), 0 -> (0, 0.5 dy), 3 -> (3, 1.5 dy)
    assert y[:3].tolist() == [0.0, 0.0, 3.0]
    assert dx[:3].tolist() == [float(-0.5 * dy[0]), float(0.5 * dy[1]), float(1.5 * dy[2])]
    if count > 8:
        assert float(dx[7]) == float(dy[7]) and float(dx[8]) == 0.0 and float(y[8]) == 0.0 and float(y[7]) == 1e4


# ------------------------------------------------------------------ squeeze-and-excitation
def _se_params(gen, cr, sq):
    """fc1 / fc2 with biases; b2 sweeps the gate pre-activation through all three pieces of the hardsigmoid."""
    w1 = _rand(gen, sq, cr, 1, 1) * (2.0 / cr) ** 0.5
    b1 = _rand(gen, sq) * 0.5
    w2 = _rand(gen, cr, sq, 1, 1) * (0.5 / sq) ** 0.5
    b2 = (torch.linspace(-4.7, 4.9, cr)[torch.randperm(cr, generator=gen)] + torch.randn(cr, generator=gen) * 0.05).float().double()
    return w1.float().double(), b1, w2.float().double(), b2


def _se_ref(x, params, dy, dtype):
    x = x.to(dtype).requires_grad_(True)
    w1, b1, w2, b2 = [p.to(dtype).requires_grad_(True) for p in params]
    pool = x.mean(dim=(2, 3), keepdim=True)
    hid = F.relu(F.conv2d(pool, w1, b1))
    s = F.conv2d(hid, w2, b2)
    y = x * (torch.clamp(s + 3, 0, 6) / 6)
    gs = torch.autograd.grad(y, [x, w1, b1, w2, b2], dy.to(dtype))
    return dict(y=y.detach(), pool=pool.detach().flatten(1), hid=hid.detach().flatten(1), s=s.detach().flatten(1), dx=gs[0],
                dw1=gs[1], db1=gs[2], dw2=gs[3], db2=gs[4])


def _se_run(x, params, dy, cs, prev=None):
    L = _lib.lib()
    n, cr, h, w = x.shape
    sq = params[0].shape[0]
    xd, dd = _nhwc(x, cs), _nhwc(dy, cs)
    pd = [p.float().contiguous().cuda() for p in params]
    pool, hid, s, y = Arena(n * cs), Arena(n * sq), Arena(n * cs), Arena(n * h * w * cs)
    _ok(L.udp_se_train_fwd(xd.data_ptr(), *[p.data_ptr() for p in pd], n, h, w, cs, cr, sq, F32, pool.ptr(), hid.ptr(), s.ptr(),
                           y.ptr(), _s()))
    out = dict(y=y.get("se y"), pool=pool.get("se pool"), hid=hid.get("se hid"), s=s.get("se s"))
    ws_bytes = int(L.udp_se_train_workspace_bytes(n, cs, sq))
    ws, dx = Arena(ws_bytes // 4), Arena(n * h * w * cs)
    if prev is not None:
        dx.t.copy_(_nhwc(prev, cs).reshape(-1))
    g = dict(dw1=Arena(sq * cr), db1=Arena(sq), dw2=Arena(cr * sq), db2=Arena(cr))
    _ok(L.udp_se_train_bwd(dd.data_ptr(), xd.data_ptr(), pd[0].data_ptr(), pd[2].data_ptr(), pool.ptr(), hid.ptr(), s.ptr(), n, h, w,
                           cs, cr, sq, int(prev is not None), F32, dx.ptr(), g["dw1"].ptr(), g["db1"].ptr(), g["dw2"].ptr(),
                           g["db2"].ptr(), ws.ptr(), ws_bytes, _s()))
    ws.check("se workspace")
    out["dx"] = dx.get("se dx")
    for k, a in g.items():
        out[k] = a.get("se " + k)
    return out


@pytest.mark.parametrize("cs,cr,sq", [(16, 16, 8), (128, 120, 32), (576, 576, 144)])
def test_se_forward_and_backward_against_fp64(cs, cr, sq):
    gen = torch.Generator().manual_seed(1000 + cr)
    for h, w in [(1, 1), (2, 2), (7, 3)]:
        for n in (1, 3):
            params = _se_params(gen, cr, sq)
            x, dy, prev = _rand(gen, n, cr, h, w), _rand(gen, n, cr, h, w), _rand(gen, n, cr, h, w)
            r64, r32 = _se_ref(x, params, dy, torch.float64), _se_ref(x, params, dy, torch.float32)
            assert bool((r64["s"] < -3).any()) and bool((r64["s"] > 3).any()) and bool(((r64["s"] > -3) & (r64["s"] < 3)).any())
            assert bool((r64["hid"] == 0).any()) and bool((r64["hid"] > 0).any())
            tag = "C%d(%d) S%d %dx%dx%d" % (cs, cr, sq, n, h, w)
            for acc in (0, 1):
                got = _se_run(x, params, dy, cs, prev if acc else None)
                if not acc:
                    _gate("se y " + tag, _nchw(got["y"], n, h, w, cs, cr), r64["y"], r32["y"])
                    _gate("se pool " + tag, got["pool"].view(n, cs)[:, :cr], r64["pool"], r32["pool"])
                    _gate("se hid " + tag, got["hid"].view(n, sq), r64["hid"], r32["hid"])
                    _gate("se s " + tag, got["s"].view(n, cs)[:, :cr], r64["s"], r32["s"])
                    for k in ("dw1", "db1", "dw2", "db2"):
                        _gate("se %s %s" % (k, tag), got[k].view(r64[k].shape), r64[k], r32[k])
                want64, want32 = (r64["dx"] + prev, r32["dx"] + prev.float()) if acc else (r64["dx"], r32["dx"])
                _gate("se dx acc%d %s" % (acc, tag), _nchw(got["dx"], n, h, w, cs, cr), want64, want32)
                for k in ("y", "dx"):
                    assert _pads_zero(got[k], cs, cr), (tag, k)
                for k in ("pool", "s"):
                    assert _pads_zero(got[k], cs, cr), (tag, k)
                again = _se_run(x, params, dy, cs, prev if acc else None)
                assert all(_same_bits(again[k], got[k]) for k in got), tag
