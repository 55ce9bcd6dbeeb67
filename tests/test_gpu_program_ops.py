"""Op-level fp64 parity of the inference ops that only whole nets reach: max-pool, bilinear resize, the 3x3 / 7x7
stems, the four PSA ops, second outputs, the chained 1x1 conv and UDP_OP_FUSE -- each in a hand-made micro-program
(tests/microprog.py) at the smallest shapes where its edges exist, one op under test at a time.

Every case asserts that the output is fully written, that every 16-bit unit of the workspace outside the declared
outputs (untouched buffers, padding, the channels outside an output slice, the operands) holds what it held before
the run, and the tolerance:
  * selections and copies (max-pool, identity resize, second outputs, the poison): bit-equal;
  * convs with a shipped gate: that of test_fused_conv_matches_torch_fp32 (1e-4 / 2e-5 / 6e-3 x scale);
  * new arithmetic (stems, bilinear, FUSE, the PSA tensors): |hip - ref64| <= 3 * err_cpu_fp32 + 4 ulp, errors
    relative to the tensor's max, err_cpu_fp32 = the same reference in fp32 on the CPU against its fp64 self,
    ulp = one unit of the storage format (fp32 2^-23, split fp16 2^-21, bf16 2^-8; the PSA side rows are fp32).
Each test prints its measured errors (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import microprog as mp
from microprog import Micro, new_op
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x2", "bf16"]


class _env:
    """Set environment knobs around a run and restore them (describe_stem / describe_stem7 read them per forward)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _gate(name, got, ref64, ref32, ulp):
    e_hip, e_cpu, gate = mp.parity(name, got, ref64, ref32, ulp)
    assert e_hip <= gate, (name, e_hip, e_cpu, gate)
    return e_hip


def _finish(m):
    m.assert_untouched()
    m.check_head()


# ------------------------------------------------------------------ max-pool
def _pool_input(m, n, c, h, w):
    """Image 0: negative only.  Image 1: negative with the maximum of channel k planted on corner / border k % 8.
    The others: mixed sign."""
    x = m.randn(n, c, h, w)
    x[0] = -x[0].abs() - 0.1
    if n > 1:
        x[1] = -x[1].abs() - 0.1
        spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
        for ch in range(c):
            y0, x0 = spots[ch % 8]
            x[1, ch, y0, x0] = 5.0 + ch
    return x


def _maxpool(mode, c, h, w, n, in_view=None, out_view=None):
    m = Micro(mode, n, seed=c + h)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ic, ip = in_view or (0, c)
    oc, op_ = out_view or (0, c)
    bi, bo = m.buf(h, w, ip), m.buf(ho, wo, op_)
    xq = m.fill(bi, _pool_input(m, n, c, h, w), coff=ic)
    m.add(new_op(_lib.UDP_OP_MAXPOOL, ks=3, stride=2, cin=c, cout=c, hin=h, win=w, hout=ho, wout=wo, in_buf=bi, out_buf=bo,
                 in_coff=ic, in_pitch=ip if in_view else 0, out_coff=oc, out_pitch=op_ if out_view else 0))
    m.wrote(bo, oc, c)
    assert m.run() == 0, m.error
    got, ref = m.read(bo, oc, c), mp.ref_maxpool(xq.double())
    assert not torch.isnan(got).any(), "output not fully written"
    assert (ref[0] < 0).all()                                   # padding that wins with 0 would show
    assert torch.equal(got.double(), ref), float((got.double() - ref).abs().max())     # a selection: bit-equal
    _finish(m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,h,w,n", [(64, 16, 16, 3), (64, 15, 9, 3), (16, 2, 2, 3), (64, 32, 24, 5)])
def test_maxpool_equals_torch(mode, c, h, w, n):
    _maxpool(mode, c, h, w, n)


@pytest.mark.parametrize("mode", MODES)
def test_maxpool_channel_slices(mode):
    """Reads channels 32.. of a 96-channel tensor (NaN elsewhere), writes channels 16.. of a 64-channel one."""
    _maxpool(mode, 32, 15, 9, 3, in_view=(32, 96), out_view=(16, 64))


# ------------------------------------------------------------------ bilinear, align_corners=True
def _bilinear(mode, c, hi, wi, ho, wo, n=3, in_view=None, out_view=None):
    m = Micro(mode, n, seed=hi * 7 + wo)
    ic, ip = in_view or (0, c)
    oc, op_ = out_view or (0, c)
    bi, bo = m.buf(hi, wi, ip), m.buf(ho, wo, op_)
    xq = m.fill(bi, m.randn(n, c, hi, wi), coff=ic)
    m.add(new_op(_lib.UDP_OP_BILINEAR, cin=c, cout=c, hin=hi, win=wi, hout=ho, wout=wo, in_buf=bi, out_buf=bo,
                 in_coff=ic, in_pitch=ip if in_view else 0, out_coff=oc, out_pitch=op_ if out_view else 0))
    m.wrote(bo, oc, c)
    assert m.run() == 0, m.error
    got = m.read(bo, oc, c)
    name = "bilinear %s c%d %dx%d->%dx%d" % (mode, c, hi, wi, ho, wo)
    if (hi, wi) == (ho, wo):
        assert torch.equal(got, xq), name                       # identity size: a copy, bit-equal
    _gate(name, got, mp.ref_bilinear(xq.double(), ho, wo), mp.ref_bilinear(xq, ho, wo), mp.ULP[mode])
    _finish(m)


BILINEAR = [(8, 6, 64, 48), (16, 12, 64, 48), (7, 5, 13, 9), (64, 48, 8, 6), (5, 5, 5, 5), (4, 4, 1, 7)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [16, 64])
@pytest.mark.parametrize("hi,wi,ho,wo", BILINEAR)
def test_bilinear_matches_torch_fp64(mode, c, hi, wi, ho, wo):
    _bilinear(mode, c, hi, wi, ho, wo)


@pytest.mark.parametrize("mode", MODES)
def test_bilinear_channel_slices(mode):
    _bilinear(mode, 32, 7, 5, 13, 9, in_view=(32, 96), out_view=(16, 64))


# ------------------------------------------------------------------ stems
def _stem(mode, ks, n, in_h, in_w, env, positive_bias):
    m = Micro(mode, n, in_h, in_w, flip=True, stem_ks=ks, seed=ks * 100 + in_h + n, positive_bias=positive_bias)
    with _env(**env):
        assert m.run() == 0, m.error
    got = m.read(m.stem_buf)
    xx = torch.cat([m.x, torch.flip(m.x, [3])])                 # rows n..2n-1: the mirrored inputs
    ref = lambda d: mp.ref_conv(xx.to(d), m.stem_w, m.stem_b, stride=2, relu=True)
    r64 = ref(torch.float64)
    if positive_bias:
        assert float(r64.min()) > 0                             # the ReLU clips nothing
    else:
        assert 0.2 < float((r64 == 0).double().mean()) < 0.8
    name = "stem%d %s%s %dx%d n%d %s" % (ks, mode, "".join("+" + k[9:] for k in env), in_h, in_w, n, "pos" if positive_bias else "mix")
    _gate(name, got, r64, ref(torch.float32), mp.ULP[mode])
    _finish(m)


STEM3 = [("f32", {}), ("f16x2", {}), ("bf16", {}), ("f16x2", {"UDP_POSE_STEM_VALU": "1"}), ("bf16", {"UDP_POSE_STEM_VALU": "1"})]
STEM7 = STEM3 + [("f16x2", {"UDP_POSE_STEM7_GATHER": "1"}), ("bf16", {"UDP_POSE_STEM7_GATHER": "1"})]
_vid = lambda v: v[0] + "".join("+" + k[9:].lower() for k in v[1])


@pytest.mark.parametrize("positive_bias", [False, True], ids=["mixbias", "posbias"])
@pytest.mark.parametrize("in_h,in_w", [(32, 32), (64, 96), (96, 32)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("variant", STEM3, ids=_vid)
def test_stem3_with_flip_matches_fp64(variant, n, in_h, in_w, positive_bias):
    _stem(variant[0], 3, n, in_h, in_w, variant[1], positive_bias)


@pytest.mark.parametrize("positive_bias", [False, True], ids=["mixbias", "posbias"])
@pytest.mark.parametrize("in_h,in_w", [(32, 32), (64, 96), (96, 32)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("variant", STEM7, ids=_vid)
def test_stem7_with_flip_matches_fp64(variant, n, in_h, in_w, positive_bias):
    """64x96 -> Wout = 48: a full and a ragged 32-column tile of stem7_lds_kernel; 96x32 -> Wout = 16: half a tile."""
    _stem(variant[0], 7, n, in_h, in_w, variant[1], positive_bias)


# The persistent stem kernels cap their grid (describe_stem / describe_stem7): a workgroup takes a second tile only
# beyond cap x tiles-per-pass.  With 32x32 inputs (256 output pixels per image) and flip_test (B = 2n images):
#   stem_mfma_kernel (3x3 bf16)     4096 workgroups x 4 waves x 16 pixels -> B > 1024 -> n = 513
#   stem_mfma_k<H2,3> (3x3 f16x2)   2048 x 4 x 16                         -> B > 512  -> n = 257
#   stem7_lds_kernel                1024 tiles of 2 x 32 pixels, 8 / image -> B > 128  -> n = 65
#   stem_mfma_k<.,7> (GATHER)       1024 x 4 x 16                         -> B > 256  -> n = 129
# (40 images, 80 with the mirrored half, reach none of these caps.)  The VALU kernels launch one workgroup per 64 pixels.
MANY = [(3, "bf16", {}, 513), (3, "f16x2", {}, 257), (7, "bf16", {}, 65), (7, "f16x2", {}, 65),
        (7, "bf16", {"UDP_POSE_STEM7_GATHER": "1"}, 129), (7, "f16x2", {"UDP_POSE_STEM7_GATHER": "1"}, 129)]


@pytest.mark.parametrize("ks,mode,env,n", MANY, ids=lambda v: None if isinstance(v, dict) else str(v))
def test_stem_persistent_workgroup_takes_a_second_tile(ks, mode, env, n):
    _stem(mode, ks, n, 32, 32, env, False)


# ------------------------------------------------------------------ PSA ops
def _psa(mode, c, h, w, n=3, spread=4.0):
    m = Micro(mode, n, seed=c + h)
    x, theta, P = mp.psa_inputs(c, h, w, n, spread)
    P64 = {k: v.double() for k, v in P.items()}
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
    # each op against the reference on the operands AS STORED by the op before it
    pool, mask, x1, x2 = m.read_rows(bpool), m.read_rows(bmask), m.read(bx1), m.read(bx2)
    tag = "psa %s C%d %dx%d s%g " % (mode, c, h, w, spread)
    f32u = mp.ULP["f32"]                                         # the side rows are fp32 in every mode
    _gate(tag + "pool.xbar", pool[:, :c], mp.psa_pool(xq.double(), P64)[:, :c], mp.psa_pool(xq, P)[:, :c], f32u)
    _gate(tag + "pool.xmean", pool[:, c:], mp.psa_pool(xq.double(), P64)[:, c:], mp.psa_pool(xq, P)[:, c:], f32u)
    _gate(tag + "mlp.m", mask[:, :c], mp.psa_mlp(pool.double(), P64)[:, :c], mp.psa_mlp(pool, P)[:, :c], f32u)
    _gate(tag + "mlp.gbar", mask[:, c:], mp.psa_mlp(pool.double(), P64)[:, c:], mp.psa_mlp(pool, P)[:, c:], f32u)
    _gate(tag + "scale", x1, mp.psa_scale(xq.double(), mask.double()), mp.psa_scale(xq, mask), mp.ULP[mode])
    _gate(tag + "sp", x2, mp.psa_sp(thq.double(), x1.double(), mask.double()), mp.psa_sp(thq, x1, mask), mp.ULP[mode])
    _finish(m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,h,w", [(16, 8, 6), (32, 16, 12), (64, 9, 7), (128, 8, 6), (256, 8, 6), (32, 64, 48)])
def test_psa_ops_match_fp64(mode, c, h, w):
    _psa(mode, c, h, w)


@pytest.mark.parametrize("mode", MODES)
def test_psa_ops_peaked_softmax(mode):
    """Logit spread about 40: without the max-subtraction exp() overflows."""
    _psa(mode, 32, 16, 12, spread=40.0)


def test_psa_refuses_c48_at_first_forward():
    """C = 48 passes udp_hrnet_create (a multiple of 16) and is refused by check_psa_c at the first forward."""
    m = Micro("f32", 1)
    c, h, w = 48, 4, 4
    x, _, _ = mp.psa_inputs(32, h, w, 1)
    bx, bpool = m.buf(h, w, c), m.buf_rows(2 * c)
    m.fill(bx, torch.cat([x, x[:, :16]], dim=1))
    nw = c + c // 2 * c + c // 8 * (c // 2) + 3 * (c // 8) + c * (c // 8) + c + c // 2 * c
    m.add(new_op(_lib.UDP_OP_PSA_POOL, in_buf=bx, out_buf=bpool, cin=c, cout=c, hin=h, win=w, hout=h, wout=w,
                 w_off=m.put(np.zeros(nw, np.float32).tobytes())))
    assert m.run() == -3 and "must divide 256" in m.error, m.error
    m.written = []
    m.assert_untouched()                                        # nothing ran
    assert torch.isnan(m.heat).all()


# ------------------------------------------------------------------ second outputs (split fp16, fragment-major weights)
@pytest.mark.parametrize("c,h,w", [(32, 16, 12), (64, 9, 7)])
def test_second_outputs_equal_stored_out_plus_addend(c, h, w):
    """3x3 stride-1 conv with n_out2 = 2, once with a real out_buf and once with UDP_BUF_NONE.  add2_k / out2_k are
    slices at channel offsets 32 and 64 of wider tensors: pitch 96 for 32 channels, pitch 128 for 64 channels (a
    64-channel slice at offset 64 does not fit pitch 96).  out2_k == encode(decode(out as stored) + decode(add2_k)),
    bit for bit, as the header promises."""
    n, pitch, coffs = 3, 96 if c == 32 else 128, (32, 64)
    out_ref = None
    for with_out in (True, False):
        m = Micro("f16x2", n, seed=c)
        bi, bo = m.buf(h, w, c), m.buf(h, w, c)
        ba, b2 = [m.buf(h, w, pitch) for _ in range(2)], [m.buf(h, w, pitch) for _ in range(2)]
        xq = m.fill(bi, m.randn(n, c, h, w))
        aq = [m.fill(ba[k], m.randn(n, c, h, w), coff=coffs[k]) for k in range(2)]
        wq = mp.quant(m.randn(c, c, 3, 3) * float(np.sqrt(2.0 / (9 * c))), "f16x2")
        bias = m.randn(c) * 0.1
        m.add(new_op(_lib.UDP_OP_CONV, ks=3, stride=1, relu=1, cin=c, cout=c, hin=h, win=w, hout=h, wout=w, in_buf=bi,
                     out_buf=bo if with_out else _lib.UDP_BUF_NONE, n_out2=2, out2_buf=b2, out2_coff=coffs, out2_pitch=[pitch] * 2,
                     add2_buf=ba, add2_coff=coffs, add2_pitch=[pitch] * 2, **m.put_conv(wq, bias, ws=True)))
        if with_out:
            m.wrote(bo)
        for k in range(2):
            m.wrote(b2[k], coffs[k], c)
        assert m.run() == 0, m.error
        if with_out:
            out_ref = m.read(bo)
            ref = mp.ref_conv(xq.double(), wq, bias, relu=True)
            assert not torch.isnan(out_ref).any()
            err = float((out_ref.double() - ref).abs().max())
            print("out2 c%d conv err %.3g" % (c, err))
            assert err <= mp.conv_tol("f16x2", ref), err
        for k in range(2):
            want = m.raw_of(out_ref + aq[k])                    # fp32 sum of the decoded operands, re-encoded
            assert np.array_equal(m.read_raw(b2[k], coffs[k], c), want), (with_out, k)
        _finish(m)                                              # without out_buf: its buffer keeps the poison


# ------------------------------------------------------------------ chained 1x1 conv (split fp16)
@pytest.mark.parametrize("chain_relu", [1, 0])
@pytest.mark.parametrize("h,w,n", [(8, 8, 1), (9, 7, 3)])
@pytest.mark.parametrize("cin", [64, 128])
def test_chained_1x1_conv_matches_fp64(cin, h, w, n, chain_relu):
    """conv 1x1 cin -> 256 + residual + ReLU, chained into a 1x1 conv 256 -> 64: `out` against the fp64 conv, chain_buf
    against the fp64 1x1 conv of the STORED out.  64 pixels (less than one 128-pixel workgroup) and 189 (ragged)."""
    m = Micro("f16x2", n, seed=cin + h)
    bi, br, bo, bc = m.buf(h, w, cin), m.buf(h, w, 256), m.buf(h, w, 256), m.buf(h, w, 64)
    xq, rq = m.fill(bi, m.randn(n, cin, h, w)), m.fill(br, m.randn(n, 256, h, w))
    w1 = mp.quant(m.randn(256, cin, 1, 1) * float(np.sqrt(2.0 / cin)), "f16x2")
    w2 = mp.quant(m.randn(64, 256, 1, 1) * float(np.sqrt(2.0 / 256)), "f16x2")
    b1, b2 = m.randn(256) * 0.1, m.randn(64) * 0.1
    packed, wexp2 = f16x2.pack_weights_ws(w2.reshape(1, 64, 256))
    m.add(new_op(_lib.UDP_OP_CONV, relu=1, cin=cin, cout=256, hin=h, win=w, hout=h, wout=w, in_buf=bi, res_buf=br, out_buf=bo,
                 chain_cout=64, chain_buf=bc, chain_relu=chain_relu, chain_wexp=wexp2, w2_off=m.put(packed.numpy().tobytes()),
                 b2_off=m.put(b2.numpy().tobytes()), **m.put_conv(w1, b1, ws=True)))
    m.wrote(bo)
    m.wrote(bc)
    assert m.run() == 0, m.error
    out, chained = m.read(bo), m.read(bc)
    assert not torch.isnan(out).any() and not torch.isnan(chained).any(), "outputs not fully written"
    ref = mp.ref_conv(xq.double(), w1, b1, res=rq.double(), relu=True)
    ref2 = mp.ref_conv(out.double(), w2, b2, relu=bool(chain_relu))
    e1, e2 = float((out.double() - ref).abs().max()), float((chained.double() - ref2).abs().max())
    print("chain cin%d %dx%d n%d relu%d: out err %.3g  chained err %.3g" % (cin, h, w, n, chain_relu, e1, e2))
    assert e1 <= mp.conv_tol("f16x2", ref), e1
    assert e2 <= mp.conv_tol("f16x2", ref2), e2
    if not chain_relu:
        assert float(ref2.min()) < 0 and float(chained.min()) < 0
    _finish(m)


# ------------------------------------------------------------------ UDP_OP_FUSE in a program
@pytest.mark.parametrize("mode", MODES)
def test_fuse_with_views_and_three_upsampled_addends(mode):
    """in + res + up(shift 1) + up(shift 2) + up(shift 3) + ReLU on 16 x 16 x 32, n = 3; in, res and out are channel
    slices.  Besides the parity rule: every element within one rounding of the storage format plus the four fp32
    additions (each within 2^-24 of the magnitudes summed) of the fp64 sum.  One rounding to p significant bits is at
    most 2^-p of the value: fp32 p = 24, split fp16 p = 22 (hi and lo carry 11 bits each), bf16 p = 8."""
    n, c, h, w = 3, 32, 16, 16
    m = Micro(mode, n, seed=11)
    bi, br, bo = m.buf(h, w, 96), m.buf(h, w, 64), m.buf(h, w, 128)
    bu = [m.buf(h >> s, w >> s, c) for s in (1, 2, 3)]
    xq, rq = m.fill(bi, m.randn(n, c, h, w), coff=32), m.fill(br, m.randn(n, c, h, w), coff=16)
    uq = [m.fill(bu[k], m.randn(n, c, h >> (k + 1), w >> (k + 1))) for k in range(3)]
    m.add(new_op(_lib.UDP_OP_FUSE, relu=1, cin=c, cout=c, hin=h, win=w, hout=h, wout=w, in_buf=bi, res_buf=br, out_buf=bo,
                 in_coff=32, in_pitch=96, res_coff=16, res_pitch=64, out_coff=64, out_pitch=128,
                 n_up=3, up_buf=bu, up_shift=[1, 2, 3]))
    m.wrote(bo, 64, c)
    assert m.run() == 0, m.error
    got = m.read(bo, 64, c)
    ref = lambda d: mp.ref_fuse(xq.to(d), rq.to(d), [(uq[k].to(d), k + 1) for k in range(3)], True)
    r64 = ref(torch.float64)
    _gate("fuse %s" % mode, got, r64, ref(torch.float32), mp.ULP[mode])
    mags = mp.ref_fuse(xq.double().abs(), rq.double().abs(), [(uq[k].double().abs(), k + 1) for k in range(3)], False)
    bound = {"f32": 2.0 ** -24, "f16x2": 2.0 ** -22, "bf16": 2.0 ** -8}[mode] * r64.abs() + 4 * 2.0 ** -24 * mags
    over = (got.double() - r64).abs() - bound
    assert float(over.max()) <= 0, float(over.max())
    _finish(m)
