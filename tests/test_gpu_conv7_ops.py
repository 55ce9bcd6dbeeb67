"""UDP_OP_CONV with ks = 7 (csrc/conv7.hip: stride 1, pad 3, NHWC, f32 and split fp16) at op level, through
udp_conv2d_fused, against the fp64 ``microprog.ref_conv`` under the shipped conv gate ``microprog.conv_tol`` (which
tests/test_gpu_ops.py holds at K = 3456; here K = 49 * cin <= 3136).

Every operand -- input, weights, bias, output -- lies in ONE device arena that is filled with the NaN pattern
``microprog.POISON16`` beforehand, 512 bytes of it between any two of them; inputs and weights are quantised with
``microprog.quant`` so that device and reference see the same numbers.  After a run the output holds no NaN, the gaps and
the operands hold what they held before, and (channel views) so do the output channels outside the view.

``out_skip`` of the "refused" list is an argument of the whole-net forward, not a udp_conv_op field: udp_conv2d_fused
cannot express it; describe_conv7 refuses it for the programs (ConvParams.out_skip)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from udp_pose_amd import _lib
from udp_pose_amd.program import encode_weights

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x2"]
UNSUP = -3
GAP = 512                                   # bytes of poison between two operands
BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))


def _tile(dtype, n, h, w, cin, cout):
    out = (C.c_int * 9)()
    _lib.check(_lib.lib().udp_debug_conv_tile(_lib.DTYPES[dtype], 0, 7, 1, n, h, w, cin, cout, 0, 0, out))
    return dict(nb=out[0], mbw=out[1], g=out[2], r=out[3], tw=out[4], one_halo=out[5], lds=out[6], wgs=out[7])


def _units(t_nhwc, dtype):
    """fp32 NHWC (NaN allowed) -> the int16 units of its device form."""
    return torch.from_numpy(mp.to_units(t_nhwc, dtype).copy())


class Arena:
    """Operands inside one poisoned device allocation."""

    def __init__(self, parts):
        """``parts``: [(name, int16 tensor or number of int16 units)] -- a number reserves poison (the output)."""
        self.off, run = {}, GAP // 2
        for name, p in parts:
            cnt = p if isinstance(p, int) else p.numel()
            self.off[name] = (run, cnt)
            run += (cnt + 127) // 128 * 128 + GAP // 2
        host = torch.full((run,), mp.POISON16, dtype=torch.int16)
        for name, p in parts:
            if not isinstance(p, int):
                a, cnt = self.off[name]
                host[a:a + cnt] = p.reshape(-1)
        self.before = host
        self.dev = host.cuda()

    def ptr(self, name):
        return C.c_void_p(self.dev.data_ptr() + 2 * self.off[name][0])

    def after(self, name):
        a, cnt = self.off[name]
        return self.dev.cpu()[a:a + cnt]

    def assert_rest_untouched(self, written="out"):
        now = self.dev.cpu()
        a, cnt = self.off[written]
        same = now == self.before
        same[a:a + cnt] = True
        bad = torch.nonzero(~same)
        assert bad.numel() == 0, "%d units outside the output changed, first at unit %d" % (bad.shape[0], int(bad[0]))


def _pack(w, b, dtype):
    """[cout, cin, 7, 7] (quantised) + bias -> wfmt 0 weights [49][cout_pad][cin] in the storage form, padded bias."""
    cout, cin = w.shape[:2]
    cp = mp.round_up(cout, 32)
    wp = torch.zeros(w.shape[2] * w.shape[3], cp, cin)
    wp[:, :cout] = w.permute(2, 3, 0, 1).reshape(-1, cout, cin)
    bp = torch.zeros(cp)
    bp[:cout] = b
    wu = torch.from_numpy(np.frombuffer(encode_weights(wp, dtype), dtype=np.int16).copy())
    bu = torch.from_numpy(bp.numpy().view(np.int16).copy())
    return wu, bu


def _run(dtype, x, w, b, relu=False, in_view=None, out_view=None):
    """x [n, cin, h, w] (quantised), w [cout, cin, k, k] (quantised), b fp32.  ``in_view`` = (coff, pitch): the input sits
    in channels [coff, coff + cin) of a ``pitch``-channel tensor whose other channels are NaN; ``out_view`` likewise for
    the output.  Returns (rc, output NCHW fp32 of the view, the whole output buffer as int16 units [n, h, w, pitch, per],
    the arena)."""
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    icoff, ipitch = in_view or (0, cin)
    ocoff, opitch = out_view or (0, cout)
    wide = torch.full((n, h, wd, ipitch), float("nan"))
    wide[..., icoff:icoff + cin] = mp.nhwc(x)
    wu, bu = _pack(w, b, dtype)
    per = 2                                                   # int16 units per stored element (fp32: 2, split fp16: hi + lo)
    arena = Arena([("in", _units(wide, dtype)), ("w", wu), ("b", bu), ("out", n * h * wd * opitch * per)])
    fields = dict(in_coff=icoff, in_pitch=ipitch if in_view else 0, out_coff=ocoff, out_pitch=opitch if out_view else 0)
    op = mp.new_op(_lib.UDP_OP_CONV, ks=w.shape[2], stride=1, relu=int(relu), cin=cin, cout=cout, hin=h, win=wd, hout=h, wout=wd, **fields)
    rc = _lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, arena.ptr("in"), arena.ptr("w"), arena.ptr("b"), None,
                                     None, None, None, arena.ptr("out"), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.UDP_OK, (rc, _lib.lib().udp_last_error().decode())
    raw = arena.after("out").numpy()
    out = mp.nchw(mp.from_units(raw, dtype, (n, h, wd, opitch)))[:, ocoff:ocoff + cout]
    units = raw.reshape(n, h, wd, 2, opitch).transpose(0, 1, 2, 4, 3) if dtype == "f16x2" else raw.reshape(n, h, wd, opitch, 2)
    return rc, out, units, arena


def _data(n, h, w, cin, cout, dtype, seed, k=7):
    g = torch.Generator().manual_seed(seed)
    x = mp.quant(torch.randn(n, cin, h, w, generator=g), dtype)
    wt = mp.quant(torch.randn(cout, cin, k, k, generator=g) * float(np.sqrt(2.0 / (cin * k * k))), dtype)
    b = torch.randn(cout, generator=g) * 0.5
    return x, wt, b


def _check(name, dtype, got, x, wt, b, relu):
    ref = mp.ref_conv(x.double(), wt.double(), b.double(), relu=relu)
    assert not torch.isnan(got).any(), "%s: output not fully written" % name
    err = float((got.double() - ref).abs().max())
    tol = mp.conv_tol(dtype, ref)
    print("%-28s %-5s |hip - fp64| %.3g (gate %.3g, max %.3g)" % (name, dtype, err, tol, float(ref.abs().max())))
    assert err <= tol, (name, err, tol)
    return ref


@pytest.fixture(scope="module")
def batch3():
    """The 3 x 9 x 7 case of both modes, run once: (x, w, b, output, units)."""
    res = {}
    for dtype in MODES:
        x, wt, b = _data(3, 9, 7, 64, 64, dtype, seed=1)
        _, out, units, arena = _run(dtype, x, wt, b)
        arena.assert_rest_untouched()
        res[dtype] = (x, wt, b, out, units)
    return res


@pytest.mark.parametrize("dtype", MODES)
def test_map_smaller_than_the_window(batch3, dtype):
    """3 x 9 x 7, 64 -> 64: the window reaches past both borders from every output pixel."""
    x, wt, b, out, _ = batch3[dtype]
    _check("3x9x7 64->64", dtype, out, x, wt, b, False)


@pytest.mark.parametrize("dtype", MODES)
def test_image_of_a_batch_equals_the_image_alone(batch3, dtype):
    """Image 1 of the 3-image run (fp32: three images share one tile) equals the same image run alone, bit for bit."""
    x, wt, b, _, units = batch3[dtype]
    _, _, alone, _ = _run(dtype, x[1:2], wt, b)
    assert np.array_equal(alone[0], units[1])
    assert _tile(dtype, 3, 9, 7, 64, 64)["g"] != _tile(dtype, 1, 9, 7, 64, 64)["g"] or dtype == "f16x2"


@pytest.mark.parametrize("dtype", MODES)
def test_ragged_chunk_rows_and_columns(dtype):
    """2 x 13 x 37, 48 -> 48: a 32 + 16 K chunk in split fp16, tile rows and columns that do not divide the map, cout
    below the 64-channel block (cout_pad 64, the last 16 lanes' channels masked)."""
    x, wt, b = _data(2, 13, 37, 48, 48, dtype, seed=2)
    _, out, _, arena = _run(dtype, x, wt, b, relu=True)
    arena.assert_rest_untouched()
    _check("2x13x37 48->48 relu", dtype, out, x, wt, b, True)
    t = _tile(dtype, 2, 13, 37, 48, 48)
    assert 37 % t["tw"] != 0 and t["nb"] == 4


@pytest.mark.parametrize("dtype", MODES)
def test_single_pixel_is_the_centre_tap(dtype):
    """1 x 1 x 1, 16 -> 16: only the centre tap sees the image; the result also equals the 1x1 conv with those weights."""
    x, wt, b = _data(1, 1, 1, 16, 16, dtype, seed=3)
    _, out, _, arena = _run(dtype, x, wt, b)
    arena.assert_rest_untouched()
    ref = _check("1x1x1 16->16", dtype, out, x, wt, b, False)
    w1 = wt[:, :, 3:4, 3:4].contiguous()
    _, out1, _, _ = _run(dtype, x, w1, b)
    assert float((out1.double() - ref).abs().max()) <= mp.conv_tol(dtype, ref)
    assert float((out1.double() - out.double()).abs().max()) <= mp.conv_tol(dtype, ref)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", MODES)
def test_interior_and_border_tiles(dtype, relu):
    """A map of at least 3 x 3 tiles (24 x 40, enlarged by 8 until the chooser's report says so): corner, edge and
    interior tiles, ReLU off and on."""
    h, w = 24, 40
    for _ in range(16):
        t = _tile(dtype, 1, h, w, 64, 64)
        ty, tx = -(-h // t["r"]), -(-w // t["tw"])
        if ty >= 3 and tx >= 3:
            break
        h, w = h + (8 if ty < 3 else 0), w + (8 if tx < 3 else 0)
    assert ty >= 3 and tx >= 3 and t["g"] == 1, (h, w, t)
    print("interior case %s: %dx%d, tile %dx%d, %d workgroups, lds %d" % (dtype, h, w, t["r"], t["tw"], t["wgs"], t["lds"]))
    x, wt, b = _data(1, h, w, 64, 64, dtype, seed=4)
    _, out, _, arena = _run(dtype, x, wt, b, relu=relu)
    arena.assert_rest_untouched()
    ref = _check("1x%dx%d 64->64 relu=%d" % (h, w, relu), dtype, out, x, wt, b, relu)
    assert not relu or (float(ref.min()) == 0.0 and float((ref == 0).double().mean()) > 0.2)


@pytest.mark.parametrize("dtype", MODES)
def test_exact_tap_placement(dtype):
    """Output channel c = 1.0 * (input channel c shifted by tap c % 49), zero bias, small integers: every channel is the
    zero-padded shift of its input channel, bit for bit, at 13 x 37."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (2, 64, 13, 37), generator=g).float()
    wt = torch.zeros(64, 64, 7, 7)
    for c in range(64):
        wt[c, c, (c % 49) // 7, (c % 49) % 7] = 1.0
    _, out, units, _ = _run(dtype, x, wt, torch.zeros(64))
    want = torch.zeros_like(x)
    xp = F.pad(x, (3, 3, 3, 3))
    for c in range(64):
        ky, kx = (c % 49) // 7, (c % 49) % 7
        want[:, c] = xp[:, c, ky:ky + 13, kx:kx + 37]
    assert torch.equal(want, F.conv2d(x.double(), wt.double(), padding=3).float())
    assert torch.equal(out, want)
    exp = mp.to_units(mp.nhwc(want), dtype)
    exp = exp.reshape(2, 13, 37, 2, 64).transpose(0, 1, 2, 4, 3) if dtype == "f16x2" else exp.reshape(2, 13, 37, 64, 2)
    assert np.array_equal(units, exp)


@pytest.mark.parametrize("dtype", MODES)
def test_channel_views(batch3, dtype):
    """Input = channels 16..79 of a 96-channel tensor (NaN elsewhere), output = channels 32..95 of a 128-channel one: the
    dense run's bits, and the other output channels still hold the poison."""
    x, wt, b, _, dense = batch3[dtype]
    _, _, units, arena = _run(dtype, x, wt, b, in_view=(16, 96), out_view=(32, 128))
    arena.assert_rest_untouched()
    assert np.array_equal(units[:, :, :, 32:96], dense)
    assert np.all(units[:, :, :, :32].view(np.uint16) == mp.POISON16) and np.all(units[:, :, :, 96:].view(np.uint16) == mp.POISON16)


@pytest.mark.parametrize("dtype", MODES)
def test_refusals_write_nothing(dtype):
    """What the 7x7 conv does not do is refused with UDP_ERR_UNSUPPORTED before anything is launched."""
    x, wt, b = _data(1, 8, 8, 64, 64, dtype, seed=6)
    L = _lib.lib()

    def refused(what, dt=None, res=False, up0=False, **fields):
        side = _units(torch.zeros(1, 8, 8, 64), dtype)
        wide = mp.nhwc(x)
        wu, bu = _pack(wt, b, dtype)
        arena = Arena([("in", _units(wide, dtype)), ("w", wu), ("b", bu), ("side", side), ("out", 8 * 8 * 64 * 2)])
        geo = dict(hout=8, wout=8)
        geo.update(fields)
        op = mp.new_op(_lib.UDP_OP_CONV, ks=7, cin=64, cout=64, hin=8, win=8, **dict(dict(stride=1), **geo))
        rc = L.udp_conv2d_fused(C.byref(op), _lib.DTYPES[dt or dtype], 1, arena.ptr("in"), arena.ptr("w"), arena.ptr("b"),
                                arena.ptr("side") if res else None, arena.ptr("side") if up0 else None, None, None, arena.ptr("out"),
                                _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == UNSUP, (what, rc, L.udp_last_error().decode())
        assert torch.equal(arena.dev.cpu(), arena.before), "%s: a refused call wrote something" % what

    refused("bf16", dt="bf16")
    refused("res", res=True)
    refused("n_up", up0=True, n_up=1, up_shift=[1, 0, 0])
    refused("n_out2", n_out2=1)
    refused("out_nchw_f32", out_buf=_lib.UDP_BUF_OUTPUT)
    refused("in_stuff2", in_stuff2=1)
    refused("hard-swish", relu=_lib.UDP_ACT_HSWISH)
    refused("SiLU", relu=_lib.UDP_ACT_SILU)
    refused("chain_cout", chain_cout=64)
    refused("group", group=1)
    refused("wfmt 1", wfmt=1)
    refused("stride 2", stride=2, hout=4, wout=4)


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("kind", ["below", "at"])
def test_range_guard(kind, where):
    """The construction of tests/test_gpu_f16x2_range.py: 32736 at one pixel of input channel 0, 2.0 on the centre tap of
    that channel in ONE output row, bias = T - 65472 there -> that element is T.  ``below`` (T = nextafter(65520, 0)) leaves
    udp_f16x2_overflow clear and stores 65520.0; ``at`` (T = 65520) raises it and reset=True clears it."""
    dtype = "f16x2"
    n, h, w, c = 3, 9, 7, 64
    img, c0, py, px = (0, 0, 0, 0) if where == "first" else (n - 1, c - 1, h - 1, w - 1)
    T = BELOW if kind == "below" else 65520.0
    x, wt, b = _data(n, h, w, c, c, dtype, seed=7)
    x[:, 0] = 0.0
    x[img, 0, py, px] = 32736.0
    wt[:, 0] = 0.0
    wt[c0] = 0.0
    wt[c0, 0, 3, 3] = 2.0
    b[c0] = float(np.float32(T) - np.float32(65472.0))
    assert not _lib.f16x2_overflow(reset=True)
    _, out, _, arena = _run(dtype, x, wt, b)
    arena.assert_rest_untouched()
    if kind == "below":
        assert not _lib.f16x2_overflow(reset=False), "below the edge raised the range flag"
        assert float(out[img, c0, py, px]) == 65520.0
        rest = torch.ones(c, dtype=torch.bool)
        rest[c0] = False
        ref = mp.ref_conv(x.double(), wt.double(), b.double())
        assert float((out[:, rest].double() - ref[:, rest]).abs().max()) <= mp.conv_tol(dtype, ref[:, rest])
        mask = torch.ones(n, h, w, dtype=torch.bool)
        mask[img, py, px] = False
        assert torch.equal(out[:, c0][mask], mp.quant(b[c0:c0 + 1], dtype).expand(int(mask.sum())))
    else:
        assert _lib.f16x2_overflow(reset=False), "at the edge: flag not raised"
        assert _lib.f16x2_overflow(reset=True)
        assert not _lib.f16x2_overflow(reset=True), "reset=True did not clear the flag"
        x2, w2, b2 = _data(n, h, w, c, c, dtype, seed=8)
        _run(dtype, x2, w2, b2)
        assert not _lib.f16x2_overflow(reset=True), "a clean run raised the flag"
