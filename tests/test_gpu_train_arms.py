"""Op-level fp64 parity of the training kernels (csrc/train.hip and the in_stuff2 read path of csrc/conv.hip) at the
shapes where their branches turn: every row of tests/train_arms.py in every weight-gradient kernel family, the stride-2
input gradient over the zero-stuffed view, train-mode BatchNorm at C = 4 .. 1028 and m = 1 .. 100, the element-wise
nodes and Adam, in fp32 and bf16.

Every test quantises its operands to the storage type first and compares with the same operation in fp64 on those
stored operands.  Every output lives inside a larger buffer filled with a NaN bit pattern: the output must come back
without a NaN where it is declared written, and the bytes around it must be unchanged.

Gates (none is fitted to what the kernels give):
  * weight gradient   1e-4 x max|ref|, input gradient 2e-4 x max|ref|: the gates of tests/test_gpu_train.py.  A bf16
    input gradient is stored in bf16, which rounds each element by up to half of bf16's eps (2^-8) of its own magnitude:
    that rounding of the gated value is added element by element, nothing else;
  * BatchNorm, element-wise nodes, Adam   |hip - ref64| <= 3 x err_cpu_fp32 + 4 ulp of the tensor's max
    (tests/microprog.py parity): err_cpu_fp32 = the same reference in fp32 on the CPU against its fp64 self, ulp = 2^-23
    for fp32 outputs (dw, dgamma, dbeta, db, statistics, Adam state), 2^-8 for tensors stored in bf16;
  * copies and masks (udp_zero_stuff2, udp_nchw_to_nhwc, udp_relu_bwd) and every "same result as the single call"
    claim: bit for bit.
"""
import ctypes as C
import functools
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import microprog as mp                                    # noqa: E402
import train_arms as ta                                   # noqa: E402
from udp_pose_amd import _lib                             # noqa: E402

NAN = float("nan")
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 256                                               # elements of NaN pattern on either side of an output


def _s():
    return _lib.stream_ptr()


class Arena:
    """``numel`` elements of ``tdt`` between two guards, all of it one NaN bit pattern until someone writes."""

    def __init__(self, numel, tdt=torch.float32):
        self.it, self.pat = (torch.int32, 0x7FC12345) if tdt == torch.float32 else (torch.int16, 0x7FC1)
        self.n = int(numel)
        self.raw = torch.full((GUARD + self.n + GUARD,), self.pat, dtype=self.it, device="cuda")
        self.t = self.raw[GUARD:GUARD + self.n].view(tdt)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        lo, hi = self.raw[:GUARD], self.raw[GUARD + self.n:]
        assert bool((lo == self.pat).all()) and bool((hi == self.pat).all()), "%s: a store outside the declared output" % what
        return self

    def get(self, what):
        self.check(what)
        out = self.t.clone()
        assert not torch.isnan(out).any(), "%s: output not fully written, or an unread NaN reached it" % what
        return out.cpu()


def _dev(t64, dtype):
    """fp64 CPU tensor of already-quantised values -> device tensor of the storage type (exact)."""
    return t64.to(TDT[dtype]).contiguous().cuda()


def _nhwc_padded(t64, pitch, dtype, pad=NAN):
    """NCHW fp64 -> device NHWC of the storage type with channels c..pitch holding ``pad``."""
    n, c, h, w = t64.shape
    o = torch.full((n, h, w, pitch), pad, dtype=torch.float64)
    o[..., :c] = t64.permute(0, 2, 3, 1)
    return _dev(o, dtype)


def _rand(g, dtype, *shape, scale=1.0, shift=0.0):
    """Random values as the device stores them, in fp64."""
    return mp.quant(torch.randn(*shape, generator=g) * scale + shift, dtype).double()


def _f32(v):
    """A scalar argument as the fp32 the ABI passes holds it."""
    return float(torch.tensor(v, dtype=torch.float32))


def _gate(name, got, ref64, ref32, ulp):
    """microprog.parity; a reference that is exactly zero (m = 1) must be met exactly."""
    if float(ref64.abs().max()) == 0.0:
        assert not torch.isnan(got).any() and float(got.abs().max()) == 0.0, "%s: expected exact zeros" % name
        print("%-40s exact zeros" % name)
        return 0.0
    e_hip, e_cpu, gate = mp.parity(name, got, ref64, ref32, ulp)
    assert e_hip <= gate, "%s: error %.3g above the gate %.3g (cpu fp32 %.3g)" % (name, e_hip, gate, e_cpu)
    return e_hip


# ------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=None)
def _wgrad_case(ks, stride, cin, cout, h, w, n, dtype):
    """Stored operands and the fp64 / fp32 CPU weight gradients of one conv (shared by the families and the groups)."""
    g = torch.Generator().manual_seed(1000 * ks + 100 * stride + cin + 7 * cout + 13 * h + w + n)
    x = _rand(g, dtype, n, cin, h, w)
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    dy = _rand(g, dtype, n, cout, ho, wo)
    shape = (cout, cin, ks, ks)
    ref64 = torch.nn.grad.conv2d_weight(x, shape, dy, stride=stride, padding=pad)
    ref32 = torch.nn.grad.conv2d_weight(x.float(), shape, dy.float(), stride=stride, padding=pad)
    dw0 = torch.randn(shape, generator=g) * float(ref64.abs().max()) * 0.5       # what accumulate = 1 adds to
    return x, dy, ref64, ref32, dw0


def _row_case(row, fam):
    return _wgrad_case(row.ks, row.stride, row.cin, row.cout, row.h, row.w, row.n, ta.dtype_of(fam))


def _run_wgrad(row, fam, x, dy, dw0):
    """One udp_conv2d_wgrad call of the row in its family: NaN in the padded channels, dw in an arena."""
    L, dtype = _lib.lib(), ta.dtype_of(fam)
    ho, wo = ta.out_hw(row)
    xd, dyd = _nhwc_padded(x, row.cin_k, dtype), _nhwc_padded(dy, row.cout_k, dtype)
    dw = Arena(row.cout * row.cin * row.ks * row.ks)
    if row.accumulate:
        dw.t.copy_(dw0.reshape(-1))
    ws = Arena(ta.workspace_bytes(row) // 4)
    with ta.family_env(fam):
        _lib.check(L.udp_conv2d_wgrad(xd.data_ptr(), dyd.data_ptr(), row.n, row.h, row.w, row.cin_k, ho, wo, row.cout_k,
                                      row.ks, row.stride, row.cout, row.cin, _lib.DTYPES[dtype], dw.ptr(), row.accumulate,
                                      ws.ptr(), ws.n * 4, _s()))
    ws.check(row.id + ": workspace")
    return dw.get("%s / %s: dw" % (row.id, fam)).reshape(row.cout, row.cin, row.ks, row.ks)


@pytest.mark.parametrize("row,fam", ta.cases(), ids=["%s-%s" % (r.id, f) for r, f in ta.cases()])
def test_wgrad_row_matches_fp64(row, fam):
    """udp_conv2d_wgrad against conv2d's weight gradient in fp64, 1e-4 x max|ref| (the gate of test_gpu_train.py).
    x and dy hold NaN in their padded channels: an MFMA row / column sees its own channel only and rows >= cout,
    columns >= cin are never stored, so no real output may notice."""
    x, dy, ref64, ref32, dw0 = _row_case(row, fam)
    p = ta.plan(row, fam)
    got = _run_wgrad(row, fam, x, dy, dw0).double()
    ref = ref64 + dw0.double() if row.accumulate else ref64
    mx = float(ref.abs().max())
    assert mx > 0
    err = float((got - ref).abs().max()) / mx
    e_cpu = float((ref32.double() - ref64).abs().max()) / float(ref64.abs().max())
    print("wgrad %-34s %-8s tw %3d th %2d upw %2d splits %2d  err %.3g  cpu fp32 %.3g  (gate 1e-4)"
          % (row.id, fam, p.tw, p.th, p.upw, p.splits, err, e_cpu))
    assert err <= 1e-4, "%s / %s: %.3g of max|ref|" % (row.id, fam, err)


GROUP_IDS = ("k3s1-16to16-1x5x65", "k1s2-32to48-3x7x9", "k3s2-17to3-2x7x5")


@pytest.mark.parametrize("fam", ta.FAMILIES)
@pytest.mark.parametrize("members", [1, 2, 3])
def test_wgrad_group_equals_single_calls(fam, members):
    """udp_conv2d_wgrad_group with 1, 2 and 3 members of mixed ks, stride and accumulate (wgrad_reduce_multi with the
    0xFFFFFFFF start sentinels of the absent members) against udp_conv2d_wgrad per member: bit for bit."""
    L, dtype = _lib.lib(), ta.dtype_of(fam)
    rows = [next(r for r in ta.ROWS if r.id == i) for i in GROUP_IDS][:members]
    rows = [r._replace(accumulate=int(j == 1)) for j, r in enumerate(rows)]
    items = (_lib.WgradItem * members)()
    keep, single = [], []
    for it, row in zip(items, rows):
        x, dy, ref64, _, dw0 = _row_case(row, fam)
        single.append(_run_wgrad(row, fam, x, dy, dw0))
        ho, wo = ta.out_hw(row)
        xd, dyd = _nhwc_padded(x, row.cin_k, dtype), _nhwc_padded(dy, row.cout_k, dtype)
        dw, ws = Arena(row.cout * row.cin * row.ks * row.ks), Arena(ta.workspace_bytes(row) // 4)
        if row.accumulate:
            dw.t.copy_(dw0.reshape(-1))
        keep.append((xd, dyd, dw, ws))
        it.x, it.dy, it.dw, it.workspace, it.workspace_bytes = xd.data_ptr(), dyd.data_ptr(), dw.ptr(), ws.ptr(), ws.n * 4
        it.n, it.hin, it.win, it.cin_k, it.hout, it.wout, it.cout_k = row.n, row.h, row.w, row.cin_k, ho, wo, row.cout_k
        it.ks, it.stride, it.cout, it.cin, it.accumulate = row.ks, row.stride, row.cout, row.cin, row.accumulate
    with ta.family_env(fam):
        _lib.check(L.udp_conv2d_wgrad_group(items, members, _lib.DTYPES[dtype], _s()))
    for row, (_, _, dw, ws), one in zip(rows, keep, single):
        ws.check(row.id + ": workspace")
        got = dw.get("group member %s" % row.id).reshape(one.shape)
        assert torch.equal(got, one), "%s: the group's result differs from the single call" % row.id


# ------------------------------------------------------------------------------------------ input gradient
def _conv_op(ks, cin, cout, hin, win, hout, wout, stuffed):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, 1, 0
    op.cin, op.cout, op.cout_pad = cin, cout, mp.round_up(cout, 32)
    op.hin, op.win, op.hout, op.wout = hin, win, hout, wout
    op.in_buf = op.res_buf = _lib.UDP_BUF_NONE
    op.in_stuff2 = stuffed
    return op


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _scratch(dtype, numel):
    return torch.empty(numel, dtype=TDT[dtype], device="cuda")


def _zero_stuff_ref(t):
    """Index reference of udp_zero_stuff2 on an NHWC tensor."""
    n, h, w, c = t.shape
    o = torch.zeros(n, 2 * h, 2 * w, c, dtype=t.dtype)
    o[:, ::2, ::2] = t
    return o


# (dy rows, dy columns, forward cin, forward cout, UDP_POSE_MAXM): under MAXM 64 the 10 x 14 map splits into tiles of 4
# rows (3 per image, the last with 2 rows); under 128 into tiles of 5 rows, so the second tile starts on an ODD row of
# the stuffed image; the 12 x 18 map takes the chooser's own tile (several workgroups)
DGRAD = [(5, 7, 16, 32, "64"), (5, 7, 16, 32, "128"), (6, 9, 48, 16, None)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("hy,wy,cin,cout,maxm", DGRAD)
def test_stride2_input_gradient_over_the_stuffed_view(dtype, ks, hy, wy, cin, cout, maxm):
    """udp_conv2d_fused with in_stuff2 = 1 (dy read as its zero-stuffed image) against the fp64 input gradient of the
    stride-2 conv, and bit-equal to the same launch over the udp_zero_stuff2 copy -- once writing a fresh dx, once
    accumulating in place onto a non-zero dx."""
    L, dt, n = _lib.lib(), _lib.DTYPES[dtype], 3
    h, w = 2 * hy, 2 * wy
    cin_k, cout_k = mp.round_up(cin, 16), mp.round_up(cout, 16)
    g = torch.Generator().manual_seed(hy * 100 + cin + ks)
    wt = _rand(g, dtype, cout, cin, ks, ks, scale=(cin * ks * ks) ** -0.5)
    dy = _rand(g, dtype, n, cout, hy, wy)
    prev = _rand(g, dtype, n, cin, h, w)
    ref64 = torch.nn.grad.conv2d_input((n, cin, h, w), wt, dy, stride=2, padding=ks // 2)
    assert ref64.shape == (n, cin, h, w)
    ref32 = torch.nn.grad.conv2d_input((n, cin, h, w), wt.float(), dy.float(), stride=2, padding=ks // 2)
    wd = Arena(ks * ks * mp.round_up(cin, 32) * cout_k, TDT[dtype])
    wdev = wt.float().contiguous().cuda()
    _lib.check(L.udp_pack_conv_weights(wdev.data_ptr(), cout, cin, ks, dt, _scratch(dtype, ks * ks * mp.round_up(cout, 32) * cin_k).data_ptr(),
                                       wd.ptr(), _s()))
    wd.get("packed dgrad weights")
    dyd = _nhwc_padded(dy, cout_k, dtype, pad=0.0)
    stuffed = Arena(n * h * w * cout_k, TDT[dtype])
    _lib.check(L.udp_zero_stuff2(dyd.data_ptr(), n, hy, wy, cout_k, dt, stuffed.ptr(), _s()))
    got_stuffed = stuffed.get("udp_zero_stuff2").reshape(n, h, w, cout_k)
    assert torch.equal(got_stuffed, _zero_stuff_ref(dyd.cpu())), "udp_zero_stuff2 differs from the index reference"
    zeros = torch.zeros(mp.round_up(cin_k, 32), device="cuda")
    tile = (C.c_int * 9)()
    with _Env(UDP_POSE_MAXM=maxm):
        _lib.check(L.udp_debug_conv_tile(dt, 0, ks, 1, n, h, w, cout_k, cin_k, 0, 0, tile))
        assert tile[7] > 1, "one workgroup only"
        if maxm == "64":
            assert h % tile[3], "the tile's %d rows divide the %d-row map: no ragged tile" % (tile[3], h)
        if maxm == "128":
            assert tile[3] % 2 and tile[3] < h, "no tile starts on an odd row of the stuffed image"
        outs = {}
        for with_res in (0, 1):
            for view in ("stuffed", "copy"):
                dx = Arena(n * h * w * cin_k, TDT[dtype])
                if with_res:
                    dx.t.copy_(_nhwc_padded(prev, cin_k, dtype, pad=0.0).reshape(-1))
                op = _conv_op(ks, cout_k, cin_k, h, w, h, w, int(view == "stuffed"))
                src = dyd.data_ptr() if view == "stuffed" else stuffed.ptr()
                _lib.check(L.udp_conv2d_fused(C.byref(op), dt, n, src, wd.ptr(), zeros.data_ptr(), dx.ptr() if with_res else None,
                                              None, None, None, dx.ptr(), _s()))
                outs[with_res, view] = dx.get("dx (%s, res %d)" % (view, with_res)).reshape(n, h, w, cin_k).float()
    for with_res in (0, 1):
        a, b = outs[with_res, "stuffed"], outs[with_res, "copy"]
        assert torch.equal(a, b), "in_stuff2 differs from the launch over the materialised copy (res %d)" % with_res
        ref = ref64 + prev if with_res else ref64
        got = a[..., :cin].permute(0, 3, 1, 2).double()
        mx = float(ref.abs().max())
        tol = torch.full_like(ref, 2e-4 * mx)
        if dtype == "bf16":
            # the bf16 store of a value within the gate: round to nearest, half of eps = 2^-7 of its magnitude
            tol = tol + 0.5 * torch.finfo(torch.bfloat16).eps * (ref.abs() + 2e-4 * mx)
        over = ((got - ref).abs() - tol).max()
        e_cpu = float((ref32.double() - ref64).abs().max()) / float(ref64.abs().max())
        print("dgrad %s k%d %dx%d %d->%d maxm %s res %d: err %.3g of max  cpu fp32 %.3g  (gate 2e-4%s)"
              % (dtype, ks, hy, wy, cin, cout, maxm, with_res, float((got - ref).abs().max()) / mx, e_cpu,
                 " + bf16 store" if dtype == "bf16" else ""))
        assert float(over) <= 0, "input gradient: %.3g above the gate" % float(over)
        assert float(a[..., cin:].abs().max() if cin_k > cin else 0.0) == 0.0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_stuff2_is_exact_at_odd_sizes(dtype):
    g = torch.Generator().manual_seed(3)
    for n, h, w, c in ((3, 5, 7, 8), (1, 1, 1, 4), (2, 3, 1, 20)):
        t = _dev(_rand(g, dtype, n, h, w, c), dtype)
        out = Arena(n * 4 * h * w * c, TDT[dtype])
        _lib.check(_lib.lib().udp_zero_stuff2(t.data_ptr(), n, h, w, c, _lib.DTYPES[dtype], out.ptr(), _s()))
        assert torch.equal(out.get("udp_zero_stuff2").reshape(n, 2 * h, 2 * w, c), _zero_stuff_ref(t.cpu()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stuffed_view_of_an_odd_sized_forward_input_is_refused(dtype):
    """udp_conv_op.in_stuff2 promises "hin, win even".  A stride-2 conv over a 7 x 9 input has a 4 x 5 output whose
    stuffed image is 8 x 10: declared as 7 x 9 the op is refused as unsupported (the kernel would read past dy),
    declared as 8 x 10 it no longer matches the 7 x 9 gradient it has to write.  Both are host-side returns; the
    trainer therefore raises on such a layer instead of computing something else."""
    L, dt = _lib.lib(), _lib.DTYPES[dtype]
    t = torch.zeros(8 * 10 * 16 * 2, dtype=TDT[dtype], device="cuda")
    wd, zeros = torch.zeros(9 * 32 * 16, dtype=TDT[dtype], device="cuda"), torch.zeros(32, device="cuda")
    op = _conv_op(3, 16, 16, 7, 9, 7, 9, 1)
    assert L.udp_conv2d_fused(C.byref(op), dt, 1, t.data_ptr(), wd.data_ptr(), zeros.data_ptr(), None, None, None, None,
                              t.data_ptr(), _s()) == -3
    assert b"even-sized stuffed image" in L.udp_last_error()
    op = _conv_op(3, 16, 16, 8, 10, 7, 9, 1)
    assert L.udp_conv2d_fused(C.byref(op), dt, 1, t.data_ptr(), wd.data_ptr(), zeros.data_ptr(), None, None, None, None,
                              t.data_ptr(), _s()) == -1
    assert b"output size" in L.udp_last_error()
    op = _conv_op(3, 16, 16, 8, 10, 8, 10, 1)
    op.stride, op.hout, op.wout = 2, 4, 5
    assert L.udp_conv2d_fused(C.byref(op), dt, 1, t.data_ptr(), wd.data_ptr(), zeros.data_ptr(), None, None, None, None,
                              t.data_ptr(), _s()) == -3


# ------------------------------------------------------------------------------------------ BatchNorm
def _bn_fwd_ref(x, gamma, beta, rm, rv, res, relu, eps, mom):
    """nn.BatchNorm2d.forward in train mode as a plain formula, in the dtype of its arguments ([m, C] rows)."""
    m = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * invstd * gamma + beta
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    unbiased = var * m / (m - 1) if m > 1 else var
    return y, mean, invstd, (1 - mom) * rm + mom * mean, (1 - mom) * rv + mom * unbiased


def _bn_bwd_ref(x, dy, y_relu, gamma, mean, invstd):
    m = x.shape[0]
    g = dy if y_relu is None else torch.where(y_relu > 0, dy, torch.zeros_like(dy))
    xhat = (x - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    return gamma * invstd * (g - dbeta / m - xhat * dgamma / m), g, dgamma, dbeta


BN_SHAPES = list(itertools.product((4, 12, 48, 1028), (1, 7, 100)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c,m", BN_SHAPES)
def test_batchnorm_train_matches_fp64(dtype, c, m):
    """udp_bn_train_fwd / _bwd against the fp64 formula: C = 4 and 12 leave threads of the partial-sum workgroup idle,
    C = 1028 (257 channel quads) takes the channel loop a second time, m = 1 meets the unbiased-variance guard.  The
    options rotate over the shapes: residual and ReLU in all four combinations, null running statistics, a second
    eps / momentum.  The backward masks with an arbitrary stored y_relu (exact 0, -0.0 and tiny positives included)."""
    L, dt, ulp_t = _lib.lib(), _lib.DTYPES[dtype], mp.ULP[dtype]
    i = BN_SHAPES.index((c, m))
    relu, with_res, null_running = i % 2, (i // 2) % 2, i % 3 == 0
    eps, mom = (_f32(1e-5), _f32(0.1)) if i % 4 else (_f32(1e-3), _f32(0.3))
    g = torch.Generator().manual_seed(17 * c + m)
    x = _rand(g, dtype, m, c, scale=1.5, shift=0.3)
    res = _rand(g, dtype, m, c) if with_res else None
    gamma, beta = (torch.rand(c, generator=g) + 0.5).double(), torch.randn(c, generator=g).double()
    rm, rv = torch.randn(c, generator=g).double(), (torch.rand(c, generator=g) + 0.5).double()
    f32 = lambda *ts: [None if t is None else t.float() for t in ts]
    ref = _bn_fwd_ref(x, gamma, beta, rm, rv, res, relu, eps, mom)
    ref32 = _bn_fwd_ref(*f32(x, gamma, beta, rm, rv, res), relu, eps, mom)
    if m > 1:                                              # the formula is torch's batch_norm
        t_rm, t_rv = rm.clone(), rv.clone()
        t_y = F.batch_norm(x.t()[None], t_rm, t_rv, gamma, beta, training=True, momentum=mom, eps=eps)[0].t()
        t_y = t_y + res if with_res else t_y
        torch.testing.assert_close(torch.relu(t_y) if relu else t_y, ref[0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(t_rm, ref[3], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(t_rv, ref[4], rtol=1e-12, atol=1e-12)
    xd = _dev(x, dtype)
    resd = _dev(res, dtype) if with_res else None
    gd, bd = gamma.float().cuda(), beta.float().cuda()
    rmd, rvd = Arena(c), Arena(c)
    rmd.t.copy_(rm.float())
    rvd.t.copy_(rv.float())
    smean, sinv, y = Arena(c), Arena(c), Arena(m * c, TDT[dtype])
    ws = torch.zeros(L.udp_bn_workspace_doubles(c), dtype=torch.float64, device="cuda")
    _lib.check(L.udp_bn_train_fwd(xd.data_ptr(), m, c, gd.data_ptr(), bd.data_ptr(), eps, mom,
                                  None if null_running else rmd.ptr(), None if null_running else rvd.ptr(), smean.ptr(),
                                  sinv.ptr(), None if resd is None else resd.data_ptr(), relu, y.ptr(), dt, ws.data_ptr(), _s()))
    tag = "bn %s C%d m%d" % (dtype, c, m)
    _gate(tag + " y", y.get(tag + " y").reshape(m, c).float(), ref[0], ref32[0], ulp_t)
    _gate(tag + " mean", smean.get(tag + " mean"), ref[1], ref32[1], mp.ULP["f32"])
    _gate(tag + " invstd", sinv.get(tag + " invstd"), ref[2], ref32[2], mp.ULP["f32"])
    if null_running:
        rmd.check(tag + " running_mean (null)")
        rvd.check(tag + " running_var (null)")
    else:
        _gate(tag + " running_mean", rmd.get(tag + " running_mean"), ref[3], ref32[3], mp.ULP["f32"])
        _gate(tag + " running_var", rvd.get(tag + " running_var"), ref[4], ref32[4], mp.ULP["f32"])
    # backward on stored operands of its own: the statistics as fp32 holds them, an arbitrary y_relu
    mean, invstd = ref[1].float().double(), ref[2].float().double()
    dy = _rand(g, dtype, m, c)
    yr = None
    if relu:
        yr = _rand(g, dtype, m, c)
        flat = yr.reshape(-1)
        tiny = float(torch.finfo(TDT[dtype]).tiny)
        specials = torch.tensor([0.0, -0.0, tiny, -tiny], dtype=torch.float64)
        idx = torch.randperm(flat.numel(), generator=g)[:flat.numel() // 2]      # half the map: the special values
        flat[idx] = specials.repeat(idx.numel() // 4 + 1)[:idx.numel()]
    bref = _bn_bwd_ref(x, dy, yr, gamma, mean, invstd)
    bref32 = _bn_bwd_ref(*f32(x, dy, yr, gamma, mean, invstd))
    dyd, yrd = _dev(dy, dtype), (None if yr is None else _dev(yr, dtype))
    dgam, dbet, dx = Arena(c), Arena(c), Arena(m * c, TDT[dtype])
    gout = Arena(m * c, TDT[dtype])
    md, isd = mean.float().cuda(), invstd.float().cuda()
    _lib.check(L.udp_bn_train_bwd(xd.data_ptr(), dyd.data_ptr(), None if yrd is None else yrd.data_ptr(), m, c, gd.data_ptr(),
                                  md.data_ptr(), isd.data_ptr(), dgam.ptr(), dbet.ptr(), dx.ptr(),
                                  gout.ptr() if with_res else None, dt, ws.data_ptr(), _s()))
    _gate(tag + " dx", dx.get(tag + " dx").reshape(m, c).float(), bref[0], bref32[0], ulp_t)
    _gate(tag + " dgamma", dgam.get(tag + " dgamma"), bref[2], bref32[2], mp.ULP["f32"])
    _gate(tag + " dbeta", dbet.get(tag + " dbeta"), bref[3], bref32[3], mp.ULP["f32"])
    if with_res:
        assert torch.equal(gout.get(tag + " g_out").reshape(m, c).double(), bref[1]), tag + ": g_out is a masked copy of dy"
    else:
        gout.check(tag + " g_out (null)")


def _bn_item(it, t, relu, rows):
    c = t["c"]
    it.x, it.dy, it.y, it.dx, it.g_out = t["x"].data_ptr(), t["dy"].data_ptr(), t["y"].ptr(), t["dx"].ptr(), t["gout"].ptr()
    it.y_relu = t["y"].ptr() if relu else None
    it.res = None if t["res"] is None else t["res"].data_ptr()
    it.gamma, it.beta = t["gamma"].data_ptr(), t["beta"].data_ptr()
    it.running_mean, it.running_var = t["rm"].ptr(), t["rv"].ptr()
    it.save_mean, it.save_invstd = t["smean"].ptr(), t["sinv"].ptr()
    it.dgamma, it.dbeta, it.ws = t["dgam"].ptr(), t["dbet"].ptr(), t["ws"].data_ptr()
    it.m, it.c, it.rows, it.relu = t["m"], c, rows, relu


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("count", [1, 2, 3])
def test_batchnorm_multi_equals_single_calls(dtype, count):
    """udp_bn_train_fwd_multi / _bwd_multi over 1, 2 and 3 tensors -- the first with the partial rows of a conv
    epilogue (udp_conv2d_fused_bn), the others with rows = 0 -- against the single-tensor entry points, bit for bit."""
    L, dt, tdt = _lib.lib(), _lib.DTYPES[dtype], TDT[dtype]
    specs = [(60, 16, 1, True), (7, 12, 0, False), (7, 1028, 1, False)][:count]       # (m, C, relu, with_res)
    n, h, w, cin = 2, 6, 5, 16

    def build():
        g = torch.Generator().manual_seed(23)
        ts = []
        for j, (m, c, relu, wr) in enumerate(specs):
            t = dict(m=m, c=c)
            t["x"] = _dev(_rand(g, dtype, m, c, scale=1.5, shift=0.3), dtype)
            t["dy"] = _dev(_rand(g, dtype, m, c), dtype)
            t["res"] = _dev(_rand(g, dtype, m, c), dtype) if wr else None
            t["gamma"], t["beta"] = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()
            for k in ("rm", "rv", "smean", "sinv", "dgam", "dbet"):
                t[k] = Arena(c)
            t["rm"].t.copy_(torch.randn(c, generator=g))
            t["rv"].t.copy_(torch.rand(c, generator=g) + 0.5)
            for k in ("y", "dx", "gout"):
                t[k] = Arena(m * c, tdt)
            t["ws"] = torch.zeros(L.udp_bn_workspace_doubles(c), dtype=torch.float64, device="cuda")
            t["rows"] = 0
            if j == 0:                                     # x = a small conv's output, statistics from its epilogue
                xin = _dev(_rand(g, dtype, n, h, w, cin), dtype)
                wt = _rand(g, dtype, c, cin, 3, 3, scale=0.1).float().cuda()
                wf = torch.empty(9 * 32 * cin, dtype=tdt, device="cuda")
                _lib.check(L.udp_pack_conv_weights(wt.data_ptr(), c, cin, 3, dt, wf.data_ptr(), None, _s()))
                op = _conv_op(3, cin, c, h, w, h, w, 0)
                rows = C.c_int(0)
                zeros = torch.zeros(32, device="cuda")
                _lib.check(L.udp_conv2d_fused_bn(C.byref(op), dt, n, xin.data_ptr(), wf.data_ptr(), zeros.data_ptr(),
                                                 t["x"].data_ptr(), t["ws"].data_ptr(), t["ws"].numel(), C.byref(rows), _s()))
                assert 0 < rows.value <= L.udp_bn_rows_max()
                t["rows"] = rows.value
            ts.append(t)
        return ts
    single, multi = build(), build()
    eps, mom = _f32(1e-5), _f32(0.1)
    for t, (m, c, relu, wr) in zip(single, specs):
        args = (t["x"].data_ptr(), m, c, t["gamma"].data_ptr(), t["beta"].data_ptr(), eps, mom, t["rm"].ptr(), t["rv"].ptr(),
                t["smean"].ptr(), t["sinv"].ptr(), None if t["res"] is None else t["res"].data_ptr(), relu, t["y"].ptr(), dt,
                t["ws"].data_ptr())
        if t["rows"]:
            _lib.check(L.udp_bn_train_fwd_from_sums(*args, t["rows"], _s()))
        else:
            _lib.check(L.udp_bn_train_fwd(*args, _s()))
        _lib.check(L.udp_bn_train_bwd(t["x"].data_ptr(), t["dy"].data_ptr(), t["y"].ptr() if relu else None, m, c,
                                      t["gamma"].data_ptr(), t["smean"].ptr(), t["sinv"].ptr(), t["dgam"].ptr(), t["dbet"].ptr(),
                                      t["dx"].ptr(), t["gout"].ptr(), dt, t["ws"].data_ptr(), _s()))
    items = (_lib.BnItem * count)()
    for it, t, (m, c, relu, wr) in zip(items, multi, specs):
        _bn_item(it, t, relu, t["rows"])
    _lib.check(L.udp_bn_train_fwd_multi(items, count, eps, mom, dt, _s()))
    _lib.check(L.udp_bn_train_bwd_multi(items, count, dt, _s()))
    for a, b, spec in zip(single, multi, specs):
        assert torch.equal(a["x"], b["x"]), "the two conv epilogues differ"
        for k in ("y", "smean", "sinv", "rm", "rv", "dx", "gout", "dgam", "dbet"):
            what = "bn multi %s %s %s" % (dtype, spec, k)
            assert torch.equal(a[k].get(what).float(), b[k].get(what).float()), what


# ------------------------------------------------------------------------------------------ element-wise nodes
def _up(t, shift):
    return t.repeat_interleave(1 << shift, 1).repeat_interleave(1 << shift, 2) if shift else t


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shift", [0, 1, 3, 5])
def test_ew_accumulate_matches_fp64(dtype, shift):
    """acc (= | +=) src[y >> shift, x >> shift], optional ReLU, on a 32 x 32 map (shift 5: one source pixel)."""
    L, dt, n, h, w, c = _lib.lib(), _lib.DTYPES[dtype], 2, 32, 32, 4
    g = torch.Generator().manual_seed(shift)
    src = _rand(g, dtype, n, h >> shift, w >> shift, c)
    acc0 = _rand(g, dtype, n, h, w, c)
    srcd = _dev(src, dtype)
    for init, relu in itertools.product((1, 0), (0, 1)):
        def ref(s, a):
            v = _up(s, shift) if init else _up(s, shift) + a
            return torch.relu(v) if relu else v
        acc = Arena(n * h * w * c, TDT[dtype])
        if not init:
            acc.t.copy_(_dev(acc0, dtype).reshape(-1))
        _lib.check(L.udp_ew_accumulate(acc.ptr(), srcd.data_ptr(), n, h, w, c, shift, init, relu, dt, _s()))
        what = "ew_accumulate %s shift %d init %d relu %d" % (dtype, shift, init, relu)
        _gate(what, acc.get(what).reshape(n, h, w, c).float(), ref(src, acc0), ref(src.float(), acc0.float()), mp.ULP[dtype])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_relu_bwd_at_zero_and_the_smallest_positive_values(dtype):
    """g = dy where y > 0, else 0: exact, with y = 0, -0.0, the smallest positive normal and subnormal numbers of the
    storage type and their negatives in the map (count not a multiple of the block)."""
    fi = torch.finfo(TDT[dtype])
    sub = float(fi.tiny) * float(fi.eps)                   # the smallest subnormal
    specials = torch.tensor([0.0, -0.0, fi.tiny, -fi.tiny, sub, -sub, 1.0, -1.0], dtype=torch.float64)
    g = torch.Generator().manual_seed(2)
    count = 8 * 333 + 5
    y = _rand(g, dtype, count)
    y[:8 * 200] = specials.repeat(200)
    y = y[torch.randperm(count, generator=g)]
    dy = _rand(g, dtype, count)
    yd, dyd = _dev(y, dtype), _dev(dy, dtype)
    assert torch.equal(yd.cpu().double(), y), "the special values survive the storage type"
    out = Arena(count, TDT[dtype])
    _lib.check(_lib.lib().udp_relu_bwd(dyd.data_ptr(), yd.data_ptr(), out.ptr(), count, _lib.DTYPES[dtype], _s()))
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    assert torch.equal(out.get("udp_relu_bwd").double(), ref)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shift", [1, 3])
def test_upsample_bwd_matches_fp64(dtype, shift):
    L, dt, n, h, w, c = _lib.lib(), _lib.DTYPES[dtype], 2, 16, 24, 4
    g = torch.Generator().manual_seed(40 + shift)
    gr = _rand(g, dtype, n, h, w, c)
    du0 = _rand(g, dtype, n, h >> shift, w >> shift, c)
    grd = _dev(gr, dtype)
    f = 1 << shift

    def ref(t, a, accumulate):
        s = t.reshape(n, h // f, f, w // f, f, c).sum(dim=(2, 4))
        return s + a if accumulate else s
    for accumulate in (0, 1):
        du = Arena(du0.numel(), TDT[dtype])
        if accumulate:
            du.t.copy_(_dev(du0, dtype).reshape(-1))
        _lib.check(L.udp_upsample_bwd(grd.data_ptr(), n, h, w, c, shift, du.ptr(), accumulate, dt, _s()))
        what = "upsample_bwd %s shift %d acc %d" % (dtype, shift, accumulate)
        _gate(what, du.get(what).reshape(du0.shape).float(), ref(gr, du0, accumulate), ref(gr.float(), du0.float(), accumulate),
              mp.ULP[dtype])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("m", [1, 255, 257])
def test_bias_grad_with_a_channel_pitch(dtype, m):
    """db[c] = column sums of 17 channels in a pitch of 32 (NaN in the padding), m around the 256-thread block."""
    c, pitch = 17, 32
    g = torch.Generator().manual_seed(m)
    gr = _rand(g, dtype, m, c)
    wide = torch.full((m, pitch), NAN, dtype=torch.float64)
    wide[:, :c] = gr
    grd = _dev(wide, dtype)
    db = Arena(c)
    _lib.check(_lib.lib().udp_bias_grad(grd.data_ptr(), m, pitch, c, db.ptr(), _lib.DTYPES[dtype], _s()))
    what = "bias_grad %s m %d" % (dtype, m)
    _gate(what, db.get(what), gr.sum(0), gr.float().sum(0), mp.ULP["f32"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c,c_pad", [(3, 16), (17, 32)])
def test_nchw_to_nhwc_pads_with_zeros(dtype, c, c_pad):
    n, h, w = 2, 5, 7
    g = torch.Generator().manual_seed(c)
    src = torch.randn(n, c, h, w, generator=g)
    dst = Arena(n * h * w * c_pad, TDT[dtype])
    srcd = src.cuda()
    _lib.check(_lib.lib().udp_nchw_to_nhwc(srcd.data_ptr(), n, c, h, w, c_pad, dst.ptr(), _lib.DTYPES[dtype], _s()))
    ref = torch.zeros(n, h, w, c_pad)
    ref[..., :c] = src.permute(0, 2, 3, 1)
    assert torch.equal(dst.get("udp_nchw_to_nhwc").reshape(n, h, w, c_pad), ref.to(TDT[dtype]))


# ------------------------------------------------------------------------------------------ Adam
def _adam_ref(p, gr, m, v, lr, b1, b2, eps, step, scale):
    """torch.optim.Adam's single-tensor rule in the dtype of its arguments."""
    gr = gr * scale
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - (lr / bc1) * (m / (torch.sqrt(v) / bc2 ** 0.5 + eps)), m, v


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step_matches_fp64_and_its_device_coefficient_form(step):
    """udp_adam_step over 3 x 1024 + 37 elements with grad_scale 0.5 against an fp64 Adam; udp_adam_step_dev with the
    coefficients of udp_adam_coefficients in device memory gives the same bits."""
    L, count = _lib.lib(), 3 * 1024 + 37
    lr, b1, b2, eps, scale = _f32(1e-3), _f32(0.9), _f32(0.999), _f32(1e-8), 0.5      # 1 - b2 is what fp32 makes of it
    g = torch.Generator().manual_seed(step)
    p, gr = torch.randn(count, generator=g).double(), torch.randn(count, generator=g).double()
    m = (torch.randn(count, generator=g) * (0.0 if step == 1 else 0.3)).double()
    v = (torch.rand(count, generator=g) * (0.0 if step == 1 else 0.2)).double()
    ref = _adam_ref(p, gr, m, v, lr, b1, b2, eps, step, scale)
    ref32 = _adam_ref(p.float(), gr.float(), m.float(), v.float(), lr, b1, b2, eps, step, scale)
    grd = gr.float().cuda()
    outs = []
    for form in ("host", "dev"):
        pa, ma, va = Arena(count), Arena(count), Arena(count)
        for a, t in ((pa, p), (ma, m), (va, v)):
            a.t.copy_(t.float())
        if form == "host":
            _lib.check(L.udp_adam_step(pa.ptr(), grd.data_ptr(), ma.ptr(), va.ptr(), count, lr, b1, b2, eps, step, scale, _s()))
        else:
            coef = (C.c_float * 2)()
            _lib.check(L.udp_adam_coefficients(lr, b1, b2, step, coef))
            cd = torch.tensor([coef[0], coef[1]], dtype=torch.float32).cuda()
            _lib.check(L.udp_adam_step_dev(pa.ptr(), grd.data_ptr(), ma.ptr(), va.ptr(), count, b1, b2, eps, cd.data_ptr(), scale, _s()))
        outs.append([a.get("adam %s %s" % (form, k)) for a, k in ((pa, "p"), (ma, "m"), (va, "v"))])
    for k, a, b, r, r32 in zip("pmv", outs[0], outs[1], ref, ref32):
        assert torch.equal(a, b), "udp_adam_step_dev differs from udp_adam_step in %s" % k
        _gate("adam step %d %s" % (step, k), a, r, r32, mp.ULP["f32"])
    # the step moves p by about lr = 1e-3 of its size: on p alone the gate above would pass a kernel that does nothing.
    # The update itself: fp32 arithmetic on it (1e-3 of its size is generous) + the store of p (half an ulp of p;
    # 2^-22 x max|p| covers it four times)
    upd, upd_ref = outs[0][0].double() - p.float().double(), ref[0] - p
    assert float((upd - upd_ref).abs().max()) <= 1e-3 * float(upd_ref.abs().max()) + 2.0 ** -22 * float(p.abs().max())
