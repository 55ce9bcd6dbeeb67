"""The ShuffleNetV2 training kernels (csrc/dw_train.hip at ks = 3, csrc/shufflenet_train.hip), one entry point at a time,
against fp64 torch on the CPU: depthwise 3x3 forward / input gradient / weight gradient (F.conv2d(groups=C) + autograd),
pixel shuffle (F.pixel_shuffle), the channel shuffle on pairs of halves and the concat (indexing).

Every output lives in an arena of one NaN bit pattern between two guards (tests/test_gpu_train_arms.py): it must come back
fully written and the guards untouched.  Gates: forward and input gradient 3 x (the error of the fp32 CPU evaluation) +
4 x 2^-23 relative to the tensor's max (microprog.parity); weight gradient 1e-4 x max|ref| (tests/train_arms.py).  The
data movers are compared bit for bit."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import microprog as mp                                    # noqa: E402
from test_gpu_train_arms import Arena                     # noqa: E402
from udp_pose_amd import _lib                             # noqa: E402

F32, BF16 = _lib.UDP_F32, _lib.UDP_BF16
ARG, UNSUP, WORKSPACE = -1, -3, -4
CHANNELS = [(4, 4), (32, 24), (64, 58), (96, 88)]          # stored / real
SHAPES = [(1, 1, 1), (1, 1, 5), (3, 7, 9), (2, 8, 10)]     # (n, h, w); 7x9 -> 4x5 is the odd stride-2 case


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


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _dw_fwd(x, wt, cs, s):
    n, cr, h, w = x.shape
    ho, wo = _out_hw(h, w, s)
    out = Arena(n * ho * wo * cs)
    xd, wd = _nhwc(x, cs), wt.float().contiguous().cuda()          # (held until the result has been read)
    _ok(_lib.lib().udp_dwconvk_train_fwd(xd.data_ptr(), wd.data_ptr(), n, h, w, cs, cr, 3, s, F32, out.ptr(), _s()))
    return out.get("dw fwd"), (n, ho, wo)


def _dw_dgrad(dy, wt, cs, s, h, w, prev=None):
    n, cr, ho, wo = dy.shape
    out = Arena(n * h * w * cs)
    if prev is not None:
        out.t.copy_(_nhwc(prev, cs).reshape(-1))
    dd, wd = _nhwc(dy, cs), wt.float().contiguous().cuda()
    _ok(_lib.lib().udp_dwconvk_dgrad(dd.data_ptr(), wd.data_ptr(), n, h, w, cs, cr, 3, s, int(prev is not None), F32,
                                     out.ptr(), _s()))
    return out.get("dw dgrad")


def _plan(n, ho, wo, cs, ws):
    out = (C.c_int * 4)()
    _ok(_lib.lib().udp_debug_dw_wgrad_plan(n, ho, wo, cs, 3, ws, out))
    return list(out)


def _dw_wgrad(x, dy, cs, s, ws_bytes=None):
    n, cr, h, w = x.shape
    ho, wo = dy.shape[2:]
    L = _lib.lib()
    if ws_bytes is None:
        ws_bytes = int(L.udp_dwconvk_wgrad_workspace_bytes(n, ho, wo, cs, 3))
    ws = Arena(ws_bytes // 4)
    out = Arena(cr * 9)
    xd, dd = _nhwc(x, cs), _nhwc(dy, cs)
    _ok(L.udp_dwconvk_wgrad(xd.data_ptr(), dd.data_ptr(), n, h, w, cs, cr, 3, s, F32, out.ptr(), ws.ptr(), ws_bytes, _s()))
    ws.check("dw wgrad workspace")
    return out.get("dw wgrad").view(cr, 1, 3, 3), _plan(n, ho, wo, cs, ws_bytes)


def _ref(x, wt, dy, s, dtype):
    """(y, dx, dw) of F.conv2d(groups=C) + autograd in ``dtype`` on the CPU."""
    x = x.to(dtype).requires_grad_(True)
    wt = wt.to(dtype).requires_grad_(True)
    y = F.conv2d(x, wt, None, stride=s, padding=1, groups=x.shape[1])
    if dy is None:
        return y.detach(), None, None
    dx, dw = torch.autograd.grad(y, [x, wt], dy.to(dtype))
    return y.detach(), dx, dw


# ------------------------------------------------------------------ depthwise 3x3
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cs,cr", CHANNELS)
def test_dw_forward_dgrad_and_wgrad_against_fp64(cs, cr, stride):
    gen = torch.Generator().manual_seed(100 * cs + stride)
    for n, h, w in SHAPES:
        ho, wo = _out_hw(h, w, stride)
        x, wt, dy, prev = _rand(gen, n, cr, h, w), _rand(gen, cr, 1, 3, 3), _rand(gen, n, cr, ho, wo), _rand(gen, n, cr, h, w)
        y64, dx64, dw64 = _ref(x, wt, dy, stride, torch.float64)
        y32, dx32, dw32 = _ref(x, wt, dy, stride, torch.float32)
        tag = "C%d(%d) s%d %dx%dx%d" % (cs, cr, stride, n, h, w)
        y, (_, gho, gwo) = _dw_fwd(x, wt, cs, stride)
        assert (gho, gwo) == (ho, wo)
        e, _, gate = mp.parity("dw fwd " + tag, _nchw(y, n, ho, wo, cs, cr), y64, y32, 2.0 ** -23)
        assert e <= gate, (tag, e, gate)
        assert cr == cs or float(y.view(-1, cs)[:, cr:].abs().max()) == 0.0            # pads: exactly zero
        for acc in (0, 1):
            dx = _dw_dgrad(dy, wt, cs, stride, h, w, prev if acc else None)
            want64, want32 = (dx64 + prev, dx32 + prev.float()) if acc else (dx64, dx32)
            e, _, gate = mp.parity("dw dgrad acc%d %s" % (acc, tag), _nchw(dx, n, h, w, cs, cr), want64, want32, 2.0 ** -23)
            assert e <= gate, (tag, acc, e, gate)
            assert cr == cs or float(dx.view(-1, cs)[:, cr:].abs().max()) == 0.0
        dw, plan = _dw_wgrad(x, dy, cs, stride)
        mx = float(dw64.abs().max())
        e_ours, e_f32 = float((dw.double() - dw64).abs().max()), float((dw32.double() - dw64).abs().max())
        print("dw wgrad %-26s plan %s  max|ref| %.3e  ours %.3e  fp32-CPU %.3e  gate %.3e" % (tag, plan, mx, e_ours, e_f32, 1e-4 * mx))
        assert e_ours <= 1e-4 * mx, (tag, e_ours, mx)


def test_dw_wgrad_splits():
    """One partial; >= 3 partials with a shorter last workgroup; a workspace that limits the split.  Same gate, and two
    runs are bit-equal."""
    gen = torch.Generator().manual_seed(7)
    cs, cr = 64, 58
    for (n, h, w, stride), ws_bytes, want_plan in (((1, 1, 5, 1), None, (1, 1)),                 # 1 output row: one partial
                                                   ((3, 7, 9, 1), 5 * 9 * cs * 4, (5, 5)),        # 21 rows in runs of 5: 5,5,5,5,1
                                                   ((3, 7, 9, 2), 2 * 9 * cs * 4 + 8, (6, 2)),    # 12 rows, room for 2 partials
                                                   ((40, 8, 10, 1), None, (2, 160))):             # 320 rows: the 256 cap -> runs of 2
        ho, wo = _out_hw(h, w, stride)
        x, dy = _rand(gen, n, cr, h, w), _rand(gen, n, cr, ho, wo)
        _, _, dw64 = _ref(x, _rand(gen, cr, 1, 3, 3), dy, stride, torch.float64)
        dw, plan = _dw_wgrad(x, dy, cs, stride, ws_bytes)
        assert (plan[0], plan[2]) == want_plan, plan
        mx = float(dw64.abs().max())
        e = float((dw.double() - dw64).abs().max())
        print("dw wgrad split %dx%dx%d s%d plan %s: ours %.3e gate %.3e" % (n, h, w, stride, plan, e, 1e-4 * mx))
        assert e <= 1e-4 * mx
        again, _ = _dw_wgrad(x, dy, cs, stride, ws_bytes)
        assert torch.equal(again.view(torch.int32), dw.view(torch.int32))


@pytest.mark.parametrize("stride", [1, 2])
def test_dw_image_zero_of_three_is_the_single_image(stride):
    gen = torch.Generator().manual_seed(11)
    cs, cr, h, w = 32, 24, 7, 9
    ho, wo = _out_hw(h, w, stride)
    x, wt, dy = _rand(gen, 3, cr, h, w), _rand(gen, cr, 1, 3, 3), _rand(gen, 3, cr, ho, wo)
    y3, _ = _dw_fwd(x, wt, cs, stride)
    y1, _ = _dw_fwd(x[:1], wt, cs, stride)
    assert torch.equal(y3.view(3, -1)[0].view(torch.int32), y1.view(-1).view(torch.int32))
    d3, d1 = _dw_dgrad(dy, wt, cs, stride, h, w), _dw_dgrad(dy[:1], wt, cs, stride, h, w)
    assert torch.equal(d3.view(3, -1)[0].view(torch.int32), d1.view(-1).view(torch.int32))


@pytest.mark.parametrize("stride", [1, 2])
def test_dw_one_hot_places_every_tap(stride):
    """Weights 1..9 per tap (times channel + 1): a one-hot x shows each tap at its output pixel, a one-hot dy at its input
    pixel, and the weight gradient of one-hot x . one-hot dy is a single tap.  Exact: every product is a small integer."""
    cs, cr, h, w = 32, 24, 7, 9
    ho, wo = _out_hw(h, w, stride)
    wt = (torch.arange(1, 10).double().view(1, 1, 3, 3) * torch.arange(1, cr + 1).double().view(cr, 1, 1, 1))
    for (py, px) in ((0, 0), (3, 4), (6, 8), (5, 3)):
        x = torch.zeros(1, cr, h, w, dtype=torch.float64)
        x[0, :, py, px] = 1.0
        y, _ = _dw_fwd(x, wt, cs, stride)
        assert torch.equal(_nchw(y, 1, ho, wo, cs, cr).double(), _ref(x, wt, None, stride, torch.float64)[0])
    for (qy, qx) in ((0, 0), (ho - 1, wo - 1), (ho // 2, wo // 2)):
        dy = torch.zeros(1, cr, ho, wo, dtype=torch.float64)
        dy[0, :, qy, qx] = 1.0
        x = torch.zeros(1, cr, h, w, dtype=torch.float64)
        _, dx64, _ = _ref(x, wt, dy, stride, torch.float64)
        dx = _dw_dgrad(dy, wt, cs, stride, h, w)
        assert torch.equal(_nchw(dx, 1, h, w, cs, cr).double(), dx64)
        for ky in range(3):
            for kx in range(3):
                iy, ix = qy * stride + ky - 1, qx * stride + kx - 1
                if not (0 <= iy < h and 0 <= ix < w):
                    continue
                x = torch.zeros(1, cr, h, w, dtype=torch.float64)
                x[0, :, iy, ix] = 2.0
                dw, _ = _dw_wgrad(x, dy, cs, stride)
                want = torch.zeros(cr, 1, 3, 3, dtype=torch.float64)
                want[:, 0, ky, kx] = 2.0
                assert torch.equal(dw.double(), want), (qy, qx, ky, kx)
    # stride 2, 7 -> 4: the last input row receives from ky = 1 only (row 6 = 2 * 3 + 1 - 1)
    if stride == 2:
        dy = torch.ones(1, cr, ho, wo, dtype=torch.float64)
        dx = _nchw(_dw_dgrad(dy, wt, cs, stride, h, w), 1, h, w, cs, cr).double()
        assert torch.equal(dx[0, :, 6, 1], wt[:, 0, 1, 0] + wt[:, 0, 1, 2])          # odd column: kx = 0 and 2 of row ky = 1
        assert torch.equal(dx[0, :, 6, 2], wt[:, 0, 1, 1])                          # even column: the centre tap alone


# ------------------------------------------------------------------ pixel shuffle
def _patterns(numel, seed):
    """Distinct int32 bit patterns, among them -0.0, NaNs (quiet and signalling payloads) and subnormals."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randperm(numel, generator=g).to(torch.int64) * 7919 + 12345
    special = torch.tensor([0x80000000, 0x7FC00001, 0x7F800123, 0xFFC00000, 0x00000001, 0x807FFFFF, 0x7F800000], dtype=torch.int64)
    k = min(len(special), numel)
    bits[:k] = special[:k]
    bits = bits & 0xFFFFFFFF
    return torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)


@pytest.mark.parametrize("cin", [64, 128])
def test_pixel_shuffle_forward_and_backward_bit_exact(cin):
    L = _lib.lib()
    for n, h, w in ((1, 1, 1), (1, 3, 5), (3, 6, 4), (3, 1, 1)):
        bits = _patterns(n * h * w * cin, cin + n)                                  # NHWC [n,h,w,cin]
        x = bits.view(n, h, w, cin)
        # F.pixel_shuffle moves floats; do it on the bit patterns as int64 -> exact, then compare patterns
        want = F.pixel_shuffle(x.permute(0, 3, 1, 2).to(torch.int64).double(), 2).to(torch.int64).to(torch.int32).permute(0, 2, 3, 1).contiguous()
        out = Arena(n * h * w * cin)
        xd, wantd = x.cuda(), want.cuda()
        _ok(L.udp_pixshuf2_train_fwd(xd.data_ptr(), n, h, w, cin, F32, out.ptr(), _s()))
        got = out.check("pixshuf fwd").t.view(torch.int32).cpu().view(n, 2 * h, 2 * w, cin // 4)
        assert torch.equal(got, want), (n, h, w)
        back = Arena(n * h * w * cin)
        _ok(L.udp_pixshuf2_train_bwd(wantd.data_ptr(), n, h, w, cin, F32, back.ptr(), _s()))
        assert torch.equal(back.check("pixshuf bwd").t.view(torch.int32).cpu().view(n, h, w, cin), x), (n, h, w)


# ------------------------------------------------------------------ channel shuffle on pairs, concat
@pytest.mark.parametrize("r,cp", [(24, 32), (58, 64), (88, 96), (2, 16)])
def test_shuffle_pair_and_cat_bit_exact(r, cp):
    L = _lib.lib()
    for m in (1, 7, 257):
        a, b = _patterns(m * cp, r + m).view(m, cp), _patterns(m * cp, 2 * r + m).view(m, cp) ^ 0x55
        a[:, r:], b[:, r:] = 0, 0
        logical = torch.cat((a[:, :r], b[:, :r]), 1)
        even, odd = Arena(m * cp), Arena(m * cp)
        ad, bd = a.cuda(), b.cuda()
        _ok(L.udp_shuffle_pair_fwd(ad.data_ptr(), bd.data_ptr(), m, r, cp, cp, F32, even.ptr(), odd.ptr(), _s()))
        ge = even.check("shuffle even").t.view(torch.int32).cpu().view(m, cp)
        go = odd.check("shuffle odd").t.view(torch.int32).cpu().view(m, cp)
        assert torch.equal(ge[:, :r], logical[:, 0::2]) and torch.equal(go[:, :r], logical[:, 1::2])
        assert int(ge[:, r:].abs().max()) == 0 and int(go[:, r:].abs().max()) == 0
        da, db = Arena(m * cp), Arena(m * cp)
        ged, god = ge.cuda(), go.cuda()
        _ok(L.udp_shuffle_pair_bwd(ged.data_ptr(), god.data_ptr(), m, r, cp, cp, F32, da.ptr(), db.ptr(), _s()))
        assert torch.equal(da.check("shuffle d_a").t.view(torch.int32).cpu().view(m, cp), a)       # backward o forward = identity,
        assert torch.equal(db.check("shuffle d_b").t.view(torch.int32).cpu().view(m, cp), b)       # pads zero
        # the concat, with halves of different widths (the first unit: 24 + 92 at 1.0x) and its inverse
        rb = max(2, r // 2)
        pb = (rb + 15) // 16 * 16
        b2 = _patterns(m * pb, r + 3).view(m, pb)
        b2[:, rb:] = 0
        cw = (r + rb + 15) // 16 * 16
        y = Arena(m * cw)
        b2d = b2.cuda()
        _ok(L.udp_chan_cat2(ad.data_ptr(), cp, r, b2d.data_ptr(), pb, rb, m, cw, F32, y.ptr(), _s()))
        gy = y.check("cat2").t.view(torch.int32).cpu().view(m, cw)
        assert torch.equal(gy[:, :r + rb], torch.cat((a[:, :r], b2[:, :rb]), 1)) and (cw == r + rb or int(gy[:, r + rb:].abs().max()) == 0)
        ua, ub = Arena(m * cp), Arena(m * pb)
        gyd = gy.cuda()
        _ok(L.udp_chan_uncat2(gyd.data_ptr(), cw, m, F32, ua.ptr(), cp, r, ub.ptr(), pb, rb, _s()))
        assert torch.equal(ua.check("uncat2 a").t.view(torch.int32).cpu().view(m, cp), a)
        assert torch.equal(ub.check("uncat2 b").t.view(torch.int32).cpu().view(m, pb), b2)


# ------------------------------------------------------------------ refusals
def test_refusals_return_their_code_with_a_message():
    L = _lib.lib()
    buf = torch.zeros(4096, device="cuda")
    p = buf.data_ptr()
    cases = [
        (L.udp_dwconvk_train_fwd, (p, p, 1, 4, 4, 32, 24, 3, 1, BF16, p, _s()), UNSUP),
        (L.udp_dwconvk_train_fwd, (p, p, 1, 4, 4, 32, 24, 3, 3, F32, p, _s()), UNSUP),
        (L.udp_dwconvk_train_fwd, (p, p, 1, 4, 4, 30, 24, 3, 1, F32, p, _s()), ARG),
        (L.udp_dwconvk_train_fwd, (p, p, 1, 4, 4, 32, 33, 3, 1, F32, p, _s()), ARG),
        (L.udp_dwconvk_train_fwd, (None, p, 1, 4, 4, 32, 24, 3, 1, F32, p, _s()), ARG),
        (L.udp_dwconvk_dgrad, (p, p, 1, 4, 4, 32, 24, 3, 1, 0, BF16, p, _s()), UNSUP),
        (L.udp_dwconvk_dgrad, (p, p, 1, 4, 4, 32, 24, 3, 3, 0, F32, p, _s()), UNSUP),
        (L.udp_dwconvk_dgrad, (p, p, 1, 4, 4, 34, 24, 3, 1, 0, F32, p, _s()), ARG),
        (L.udp_dwconvk_dgrad, (p, p, 1, 4, 4, 32, 24, 3, 1, 0, F32, None, _s()), ARG),
        (L.udp_dwconvk_wgrad, (p, p, 1, 4, 4, 32, 24, 3, 1, BF16, p, p, 4096, _s()), UNSUP),
        (L.udp_dwconvk_wgrad, (p, p, 1, 4, 4, 32, 24, 3, 3, F32, p, p, 4096, _s()), UNSUP),
        (L.udp_dwconvk_wgrad, (p, p, 1, 4, 4, 32, 24, 3, 1, F32, p, None, 4096, _s()), ARG),
        (L.udp_dwconvk_wgrad, (p, p, 1, 4, 4, 32, 24, 3, 1, F32, p, p, 9 * 32 * 4 - 4, _s()), WORKSPACE),
        (L.udp_pixshuf2_train_fwd, (p, 1, 2, 2, 64, BF16, p, _s()), UNSUP),
        (L.udp_pixshuf2_train_fwd, (p, 1, 2, 2, 32, F32, p, _s()), ARG),
        (L.udp_pixshuf2_train_bwd, (p, 1, 2, 2, 64, F32, None, _s()), ARG),
        (L.udp_pixshuf2_train_bwd, (p, 1, 2, 2, 96, F32, p, _s()), ARG),
        (L.udp_shuffle_pair_fwd, (p, p, 4, 24, 32, 32, BF16, p, p, _s()), UNSUP),
        (L.udp_shuffle_pair_fwd, (p, p, 4, 24, 32, 30, F32, p, p, _s()), ARG),
        (L.udp_shuffle_pair_fwd, (p, p, 4, 24, 16, 32, F32, p, p, _s()), ARG),
        (L.udp_shuffle_pair_fwd, (p, None, 4, 24, 32, 32, F32, p, p, _s()), ARG),
        (L.udp_shuffle_pair_bwd, (p, p, 4, 24, 32, 32, BF16, p, p, _s()), UNSUP),
        (L.udp_shuffle_pair_bwd, (p, p, 4, 24, 32, 32, F32, p, None, _s()), ARG),
        (L.udp_chan_cat2, (p, 32, 24, p, 32, 24, 4, 48, BF16, p, _s()), UNSUP),
        (L.udp_chan_cat2, (p, 32, 24, p, 32, 24, 4, 44, F32, p, _s()), ARG),
        (L.udp_chan_cat2, (p, 32, 24, p, 32, 24, 4, 48, F32, None, _s()), ARG),
        (L.udp_chan_uncat2, (p, 48, 4, BF16, p, 32, 24, p, 32, 24, _s()), UNSUP),
        (L.udp_chan_uncat2, (p, 48, 4, F32, p, 30, 24, p, 32, 24, _s()), ARG),
        (L.udp_chan_uncat2, (None, 48, 4, F32, p, 32, 24, p, 32, 24, _s()), ARG),
    ]
    for fn, args, code in cases:
        assert fn(*args) == code, (fn.__name__, args)
        assert L.udp_last_error(), fn.__name__
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                     # a refused call launches nothing
