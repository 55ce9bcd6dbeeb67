"""The split-fp16 ("f16x2") range guard, op by op, and the format away from unit scale.

Split fp16 has fp16's range: a value of magnitude >= 65520 splits into hi = inf.  Every kernel that writes split fp16
raises a flag at the store (csrc/common.h: g_h2_overflow, one per translation unit, udp_f16x2_overflow ORs them); the
stems, which split the fp32 image in registers, also check the pixels they load.  Section 1 puts ONE element of one
op's output on the edge and reads the flag; section 2 repeats fp64 parity checks with the activations scaled by 2^-10
and 2^+12, and with weights whose output channels span 2^0 .. 2^-12.

How an element lands exactly.  Only an fp32 operand carries the 24 bits of T = nextafter(65520, 0): the bias (or an
affine beta).  So a conv gets input channel 0 all zero but for 32736 (exact in fp16) at one pixel, output channel c0's
weight row all zero but for 2.0 on the centre tap of input channel 0, and no other row reads input channel 0:
  out[c0, p0] = 2 * 32736 + bias[c0] = 65472 + bias[c0]     (both products and the one addition are exact in fp32)
with bias[c0] = T - 65472 = 47.99609375 or 48.0; every other pixel of channel c0 holds bias[c0], every other channel is
an ordinary conv of N(0,1) activations with He-scaled weights.  "res" / "up" plant the 65472 in the residual or in
an upsampled addend instead.  Ops without a bias get their operands at +-65504 (the largest value that is exact in
the format), or a beta.  The chosen element sits at (image 0, channel 0, pixel 0) and at (last image, last real channel,
last pixel): with n = 3 images of 9 x 7 pixels the last pixel is in a ragged tile of every kernel.

Expectations (KINDS):
  below / -below   T = +-nextafter(65520, 0): flag clear; the element is stored as decode(encode(T)) = +-65520.0, bit for
                   bit (6e-8 relative); the other elements meet the op's fp64 gate, taken against THEIR maximum
  at / -at         +-65520.0: flag raised; reset=False reads it without clearing, reset=True reads and clears it, the
                   next read is clear, and a clean call of the same op leaves it clear
  relu_neg         pre-activation -98208 under a ReLU: stored 0, flag clear
  nan_res / nan_up one NaN in the residual / an upsampled addend (fuse: nan_up0, nan_up1 = each addend in turn), no
                   ReLU: ONE output lane is NaN, the 3 or 7 siblings
                   of its st4 / h2_split8 group are finite -- the flag is raised
  nan_in           one NaN input element, no ReLU (a ReLU stores max(NaN, 0) = 0: the writer of the NaN raised the
                   flag, the reader has nothing out of range to store)

Writers (search: kLoScale|h2_split8|st4< in csrc/).  ``site``: the store, file:line; st4 and h2_split8 (conv_dev.h:160
/ :173) hold the check of 4 / 8 values, store_vec_buf (conv_dev.h:311) and dw_store (dw_dev.h:54) go through h2_split8.
TU = the translation unit whose flag the case raises (all six: conv, conv_ws, deconv, dwconv, attn, psa).
  kernel              site                   over the edge by / why it cannot leave the range                      TU
  conv_mfma_kernel    conv.hip:359           test_conv_edge[mfma-k*]: 3x3 s1, 3x3 s2, 1x1, 1x1 s2 at NB = 2 (32 / 48 / 64 ch) conv
                                             and [mfma-k1*-nb4]: 1x1 s1 (views) and 1x1 s2 at NB = 4, the only split-fp16 NB = 4
                                             forms the chooser reaches (3x3: see NB4 below); the arm is asserted from the report
  conv1x1_hs_kernel   conv.hip:359           test_conv_edge[mfma-hs-*], [mfma-silu-*] (NB = 2), [mfma-silu-*-nb4] (NB = 4) conv
  conv_mfma_multi     conv.hip:359           test_grouped_convs_edge[mfma-multi] (NB = 2, its only form; membership asserted) conv
  conv_mfma_persist1  conv.hip:624           bf16 only (describe_conv_persist): writes no split fp16                  --
  stem_mfma_k<3>      conv.hip:1090          test_stem_output_edge[3-mfma], test_stem_input_pixel[3-mfma] (:1068)     conv
  stem_conv_kernel    conv.hip:887 (st4)     test_stem_output_edge[3-valu], test_stem_input_pixel[3-valu] (:875)      conv
  stem7_lds_kernel    conv.hip:1883          test_stem_output_edge[7-lds], test_stem_input_pixel[7-lds] (:1819)       conv
  stem7_conv_kernel   conv.hip:1197 (st4)    test_stem_output_edge[7-valu], test_stem_input_pixel[7-valu] (:1189)     conv
  stem_mfma_k<7>      conv.hip:1090          test_stem_output_edge[7-gather], test_stem_input_pixel[7-gather]         conv
  fuse_sum_kernel     conv.hip:1136 (st4)    test_fuse_edge                                                           conv
  maxpool3_kernel     conv.hip:1225 (st4)    a selection of stored values: test_selections_stay_silent[maxpool]       conv
  bilinear_ac_kernel  conv.hip:1257 (st4)    a convex combination of stored values: ...[bilinear-same / -up]          conv
  conv_ws_h2_kernel   conv_ws.hip:418        test_conv_edge[ws-k*]                                                    conv_ws
  (second outputs)    conv_ws.hip:422, :442  test_second_output_edge: out + addend reaches the edge, out does not     conv_ws
  conv_ws_hs_kernel   conv_ws.hip:418        test_conv_edge[ws-hs-*], [ws-silu-*]                                     conv_ws
  conv_ws_multi       conv_ws.hip:418        test_grouped_convs_edge[ws-multi] (PB 6 + 6), [ws-multi-pb8-member] (6 + 8)  conv_ws
  conv_ws_pb8_kernel  conv_ws.hip:418        test_grouped_convs_edge[ws-pb8] (PB 8 beside a PB 4 sibling; arms asserted)  conv_ws
  conv_chain_kernel   conv_ws.hip:1140,:1183 test_chain_edge[out-*] (:1140), test_chain_edge[chained-*] (:1183)       conv_ws
  deconv4s2_kernel    deconv.hip:253         test_deconv_edge                                                         deconv
  dwconv3_kernel      dwconv.hip:121         test_dwconv_edge[3-*]                                                    dwconv
  dwconvk_kernel      dwconv.hip:212         test_dwconv_edge[5-*], [7-*]                                             dwconv
  se_kernel           dwconv.hip:299         a gate in [0, 1] times a stored value; NaN: test_se_stays_silent_...     dwconv
  pixshuf2_kernel     dwconv.hip:306         moves bit patterns, no arithmetic: test_selections_stay_silent[pixshuf]  --
  gnorm_kernel        attn.hip:95            test_norm_edge[gnorm] (beta)                                             attn
  linattn_kernel      attn.hip:194           relu(v) * context: a product of stored values -- test_linattn_edge       attn
  lnorm_kernel        attn.hip:265           test_norm_edge[lnorm] (beta)                                             attn
  act_kernel          attn.hip:284           |silu(x)|, |hswish(x)| <= |x|; NaN: test_act_stays_silent_...            attn
  mhattn_kernel       attn.hip:293           a convex sum of values; NaN: test_mhattn_stays_silent_...                attn
  psa_scale_kernel    psa.hip:43             a sigmoid times a stored value; NaN: test_psa_stays_silent_...           psa
  psa_sp_kernel       psa.hip:43             the same                                                                 psa
(psa_train.hip's st4 is its own fp32 / bf16 helper: the training kernels write no split fp16.)
"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import microprog as mp
from microprog import Micro, new_op
from test_gpu_mobilevit_ops import _act_op, _ln_data, _ln_op, _ln_ref, _mh_check, _mh_data, _mh_op, LN_CR, MH_D
from test_gpu_mobilevitv2_ops import _gn_data, _gn_op, _gn_ref, _la_data, _la_op, GN_CR, LA_C
from test_gpu_program_ops import _env
from test_gpu_shufflenet_ops import _call, _dev, _host, _nan
from test_gpu_shufflenet_plus_ops import _se_ref
from mobilevitv2_ref import linear_attention_core
from udp_pose_amd import _lib, f16x2

pytestmark = pytest.mark.gpu

H2 = "f16x2"
BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))
TOP = 65504.0                       # the largest value the format holds exactly
BIG, W0 = 32736.0, 2.0              # BIG * W0 = 65472, both exact in fp16
SILENT = ("below", "-below", "relu_neg")
RAISES = ("at", "-at")
EDGES = SILENT + RAISES
POISON = -12345.0
HS, SILU = _lib.UDP_ACT_HSWISH, _lib.UDP_ACT_SILU


def _q(t):
    return f16x2.decode(f16x2.encode(t))


def _flag(reset=True):
    return bool(_lib.f16x2_overflow(reset=reset))


def _target(kind):
    return {"below": BELOW, "-below": -BELOW, "at": 65520.0, "-at": -65520.0}[kind]


def _verdict(kind, run):
    """``run(kind)`` executes the op once and checks its output.  Around it: the flag protocol of the module docstring."""
    _flag(reset=True)
    run(kind)
    if kind in SILENT or kind == "clean":
        assert not _flag(reset=False), "%s raised the range flag" % kind
        assert not _flag(reset=True)
        return
    assert _flag(reset=False), "%s left the range flag clear" % kind
    assert _flag(reset=False), "reset=False cleared the flag"
    assert _flag(reset=True)
    assert not _flag(reset=True), "reset=True did not clear the flag"
    run("clean")                                                # the same op on clean data
    assert not _flag(reset=True), "a clean call raised the flag"


def _others(name, got, ref, mask, tol_of):
    """Every element outside ``mask`` against ``ref`` (fp64), the gate taken against the maximum of THOSE elements."""
    keep = ~mask
    g, r = got.double()[keep], ref.double()[keep]
    assert torch.isfinite(g).all(), "%s: non-finite or unwritten element beside the chosen one" % name
    err, tol = float((g - r).abs().max()), tol_of(r)
    print("%-44s others: err %.3g (gate %.3g, max %.3g)" % (name, err, tol, float(r.abs().max())))
    assert err <= tol, (name, err, tol)


def _chosen(name, kind, v):
    """The stored value of the chosen element."""
    v = float(v)
    print("%-44s chosen element stored as %r" % (name, v))
    if kind in ("below", "-below"):
        want = float(_q(torch.tensor([_target(kind)]))[0])
        assert want == math.copysign(65520.0, want)                                 # what the format makes of T
        assert v == want, (name, v, want)
        assert abs(v - _target(kind)) <= 2.0 ** -22 * 65520.0
    elif kind == "relu_neg":
        assert v == 0.0, (name, v)


# =================================================================== convs
def _plant_conv(kind, last, ks, stride, cin, cout, real, h, w, n, res, nup, relu, seed, via="w", transposed=False):
    """The operands of one conv case (NCHW, quantised) with the chosen element planted as the docstring describes."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    if transposed:
        ho, wo = 2 * h, 2 * w
    else:
        pad = ks // 2
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    x = rn(n, cin, h, w)
    wt = rn(cout, cin, ks, ks) * float(np.sqrt(2.0 / (cin * ks * ks)))
    wt[real:] = 0                                               # pad channels: zero weights and bias, as the planner packs them
    bias = rn(cout) * 0.1
    bias[real:] = 0
    r = rn(n, cout, ho, wo) if res else None
    ups = [rn(n, cout, ho >> (u + 1), wo >> (u + 1)) for u in range(nup)]
    n0, c0, yo, xo = (n - 1, real - 1, ho - 1, wo - 1) if last else (0, 0, 0, 0)
    if kind != "clean":
        x[:, 0] = 0
        wt[:, 0] = 0
        wt[c0] = 0
        if r is not None:
            r[:, c0] = 0
        for t in ups:
            t[:, c0] = 0
    if transposed:                                              # ConvTranspose2d(4, 2, 1): out[2i + ky - 1] += x[i] w[ky]
        iy, ix, ky, kx = yo // 2, xo // 2, 1 + yo % 2, 1 + xo % 2
    else:
        iy, ix, ky, kx = stride * yo, stride * xo, ks // 2, ks // 2
    if kind in EDGES:
        sign = -1.0 if kind.startswith("-") else 1.0
        if kind == "relu_neg":
            assert relu == 1
            x[n0, 0, iy, ix], wt[c0, 0, ky, kx], bias[c0] = BIG, -3.0, 0.25          # -98208 + 0.25
        elif via == "w":
            x[n0, 0, iy, ix], wt[c0, 0, ky, kx] = BIG, sign * W0
        elif via == "res":
            r[n0, c0, yo, xo] = sign * BIG * W0
        else:
            ups[0][n0, c0, yo >> 1, xo >> 1] = sign * BIG * W0                        # lands on a 2 x 2 block of the output
        if kind != "relu_neg":
            bias[c0] = sign * (abs(_target(kind)) - BIG * W0)
    elif kind == "nan_res":
        r[n0, c0, yo, xo] = float("nan")
    elif kind == "nan_up":
        ups[0][n0, c0, yo >> 1, xo >> 1] = float("nan")
    elif kind == "nan_in":
        x[n0, 1, iy, ix] = float("nan")
    x, wt = _q(x), _q(wt)
    r = _q(r) if r is not None else None
    ups = [_q(t) for t in ups]
    if transposed:
        wt = wt.permute(1, 0, 2, 3).contiguous()                # [cin, cout, 4, 4]
        y = F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2, padding=1)
    else:
        y = F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=ks // 2)
    if r is not None:
        y = y + r.double()
    for u, t in enumerate(ups):
        y = y + F.interpolate(t.double(), scale_factor=2 ** (u + 1), mode="nearest")
    if relu == 1:
        y = F.relu(y)
    elif relu == HS:
        y = y * torch.clamp(y + 3, 0, 6) / 6
    elif relu == SILU:
        y = y * torch.sigmoid(y)
    mask = torch.zeros(y.shape, dtype=torch.bool)
    if kind != "clean":
        if via == "up" and kind in EDGES and kind != "relu_neg" or kind == "nan_up":
            mask[n0, c0, yo & ~1:(yo & ~1) + 2, xo & ~1:(xo & ~1) + 2] = True
        elif kind == "nan_in":
            mask[n0, :, max(0, yo - 1):yo + 2, max(0, xo - 1):xo + 2] = True          # every channel of the pixels that read it
            if transposed:
                mask[n0, :, max(0, yo - 2):yo + 3, max(0, xo - 2):xo + 3] = True
        else:
            mask[n0, c0, yo, xo] = True
    return dict(x=x, wt=wt, bias=bias, r=r, ups=ups, ref=y, mask=mask, at=(n0, c0, yo, xo), ho=ho, wo=wo)


def _wide(t_nchw, view, outside):
    t = t_nchw.permute(0, 2, 3, 1)
    if view is None:
        return t.contiguous()
    wide = torch.full(t.shape[:3] + (view[1],), outside, dtype=torch.float32)
    wide[..., view[0]:view[0] + t.shape[3]] = t
    return wide


def _conv_weights(wt, bias, ws):
    cout, cin, kh, kw = wt.shape
    cp = mp.round_up(cout, 32)
    wp = torch.zeros(kh * kw, cp, cin)
    wp[:, :cout] = wt.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
    bp = torch.zeros(cp)
    bp[:cout] = bias
    if ws:
        packed, wexp = f16x2.pack_weights_ws(wp)
        return packed.cuda(), bp.cuda(), cp, wexp
    return f16x2.encode(wp).cuda(), bp.cuda(), cp, 0


def _conv_direct(name, kind, last, ks, stride, cin, cout, real, h, w, n, ws, relu, res, nup, views, via="w", seed=0):
    """One UDP_OP_CONV through udp_conv2d_fused (as tests/test_gpu_ops.py: _conv_case), operands from _plant_conv."""
    nan_kind = kind.startswith("nan")
    act = 0 if nan_kind and relu == 1 else relu
    d = _plant_conv(kind, last, ks, stride, cin, cout, real, h, w, n, res, nup, act, seed, via)
    in_view, out_view, res_view = ((32, cin + 64), (64, cout + 96), (16, cout + 32)) if views else (None, None, None)
    d_w, d_b, cp, wexp = _conv_weights(d["wt"], d["bias"], ws)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, act
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cp, int(ws), wexp
    op.hin, op.win, op.hout, op.wout = h, w, d["ho"], d["wo"]
    op.n_up = nup
    for u in range(nup):
        op.up_shift[u] = u + 1
    if views:
        op.in_coff, op.in_pitch = in_view
        op.out_coff, op.out_pitch = out_view
        if res:
            op.res_coff, op.res_pitch = res_view
    ocoff, opitch = out_view or (0, cout)
    d_x = f16x2.encode(_wide(d["x"], in_view, float("nan"))).cuda()     # NaN outside the input slice must not be seen
    d_r = f16x2.encode(_wide(d["r"], res_view, float("nan"))).cuda() if res else None
    d_u = [f16x2.encode(_wide(t, None, 0.0)).cuda() for t in d["ups"]] + [None] * (3 - nup)
    out = f16x2.encode(torch.full((n, d["ho"], d["wo"], opitch), POISON)).cuda()
    before = out.clone()
    _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[H2], n, _lib.ptr(d_x), _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(d_r),
                                           _lib.ptr(d_u[0]), _lib.ptr(d_u[1]), _lib.ptr(d_u[2]), _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    if views:
        keep = torch.ones(opitch, dtype=torch.bool, device="cuda")
        keep[ocoff:ocoff + cout] = False
        assert torch.equal(out[..., keep].view(torch.int16), before[..., keep].view(torch.int16)), "wrote outside the output slice"
    got = f16x2.decode(out).cpu()[..., ocoff:ocoff + cout].permute(0, 3, 1, 2)
    _judge(name, kind, d, got, relu)


def _judge(name, kind, d, got, relu=0):
    tol = lambda r: (1.5 if relu in (HS, SILU) else 1.0) * mp.conv_tol(H2, r)
    _others(name + " " + kind, got, d["ref"], d["mask"], tol)
    if kind in EDGES:
        _chosen(name + " " + kind, kind, got[d["at"]])
    if kind.startswith("nan") and kind != "nan_in":
        n0, c0, yo, xo = d["at"]
        assert torch.isnan(got[n0, c0, yo, xo])
        sib = got[n0, c0 & ~7:(c0 & ~7) + 8, yo, xo]
        assert int(torch.isnan(sib).sum()) == 1, "the NaN lane is meant to sit among finite siblings"


# name: (ks, stride, cin, cout, real, h, w, n, ws, relu, res, nup, views)
CONVS = {
    "mfma-k3s1-32": (3, 1, 32, 32, 32, 8, 8, 1, False, 1, True, 0, False),
    "mfma-k3s1-64-ragged": (3, 1, 64, 64, 64, 9, 7, 3, False, 1, True, 0, False),
    "mfma-k3s1-48-ragged": (3, 1, 48, 48, 48, 9, 7, 3, False, 1, True, 0, False),       # ragged K chunk 48 = 32 + 16
    "mfma-k3s1-26of32-views": (3, 1, 32, 32, 26, 9, 7, 3, False, 1, True, 0, True),     # pad channels + channel views
    "mfma-k3s2-32-64-up": (3, 2, 32, 64, 64, 16, 12, 3, False, 1, True, 1, False),      # 8 x 6 out, + an upsampled addend
    "mfma-k1s1-64-32": (1, 1, 64, 32, 32, 9, 7, 3, False, 0, True, 0, False),            # no activation: the negative targets
    "mfma-k1s1-32-64-views": (1, 1, 32, 64, 64, 9, 7, 3, False, 0, False, 0, True),
    "mfma-k1s2-32-64": (1, 2, 32, 64, 64, 9, 7, 3, False, 1, False, 0, False),
    "mfma-hs-k1-32": (1, 1, 32, 32, 32, 7, 5, 3, False, HS, False, 0, False),
    "mfma-silu-k1-64-views": (1, 1, 64, 64, 64, 7, 5, 3, False, SILU, False, 0, True),
    "ws-k3s1-32": (3, 1, 32, 32, 32, 8, 8, 1, True, 1, True, 0, False),
    "ws-k3s1-64-ragged": (3, 1, 64, 64, 64, 9, 7, 3, True, 1, True, 0, False),
    "ws-k3s1-48-ragged": (3, 1, 48, 48, 48, 9, 7, 3, True, 1, True, 0, False),
    "ws-k3s1-26of32-views": (3, 1, 32, 32, 26, 9, 7, 3, True, 1, True, 0, True),
    "ws-k3s2-32-64-up": (3, 2, 32, 64, 64, 16, 12, 3, True, 1, True, 1, False),
    "ws-k1s1-64-32": (1, 1, 64, 32, 32, 9, 7, 3, True, 0, True, 0, False),
    "ws-k1s2-32-64": (1, 2, 32, 64, 64, 9, 7, 3, True, 1, False, 0, False),
    "ws-hs-k1-32": (1, 1, 32, 32, 32, 7, 5, 3, True, HS, False, 0, False),
    "ws-silu-k1-64-views": (1, 1, 64, 64, 64, 7, 5, 3, True, SILU, False, 0, True),
}
# conv_mfma_kernel / conv1x1_hs_kernel come in NB = 2 and NB = 4 (cout blocks of 16 per workgroup; store_vec_buf<H2, NB>
# splits NB / 2 groups of 8 channels, the last real channel sits in the second one at NB = 4).  conv_choose_tile starts at
# NB = 4 when CoutPad % 64 == 0 and drops to 2 below UDP_POSE_MINWGS = 512 workgroups, which every shape above is.  The
# 64-output-channel 1x1 cases run again with UDP_POSE_MINWGS=0 (read at every describe): NB = 4 at the same shapes.
# A 3x3 conv never takes NB = 4 in split fp16: its weight stage alone is 9 taps x 64 rows x 64 B x 2 planes = 72 KB of the
# 76 KB the chooser allows (conv.hip: kLimit), so with any input tile it falls back to NB = 2 (measured: the report of
# the 64-channel 3x3 cases says NB=2 with UDP_POSE_MINWGS=0 too); test_conv_edge asserts NB=2 for them.
NB4 = ["mfma-k1s1-32-64-views", "mfma-k1s2-32-64", "mfma-silu-k1-64-views"]
CONVS.update({name + "-nb4": CONVS[name] for name in NB4})
TILE_MFMA = re.compile(r"^conv k(\d) s(\d) (\d+)x(\d+) C(\d+)->(\d+): G=\d+ R=\d+ TW=\d+ NB=(\d)", re.M)
TILE_WS = re.compile(r"^ws conv k(\d) s(\d) (\d+)x(\d+) C(\d+)->(\d+): G=\d+ R=\d+ TW=\d+ CP=\d+ PB=(\d+)", re.M)
TILE_GROUPED = re.compile(r"^grouped conv (\d+)x(\d+) C(\d+)->(\d+): ", re.M)


def _conv_kinds(case):
    """(kind, via) of one conv case.  Negative targets only without an activation: under a ReLU they are the relu_neg
    case, and hard-swish / SiLU send a large negative pre-activation to -0."""
    relu, res, nup = case[9], case[10], case[11]
    kinds = [("below", "w"), ("at", "w"), ("nan_in", "w")]
    if relu == 0:
        kinds += [("-below", "w"), ("-at", "w")]
    if relu == 1:
        kinds.append(("relu_neg", "w"))
    if res:
        kinds += [("below", "res"), ("at", "res"), ("nan_res", "w")]
    if nup:
        kinds += [("below", "up"), ("at", "up"), ("nan_up", "w")]
    return kinds


_ids = lambda v: ("last" if v else "first") if isinstance(v, bool) else str(v)
CONV_PARAMS = [(name, kind, via, last) for name, case in CONVS.items() for kind, via in _conv_kinds(case) for last in (False, True)]


@pytest.mark.parametrize("name,kind,via,last", CONV_PARAMS, ids=_ids)
def test_conv_edge(name, kind, via, last, capfd):
    """conv_mfma_kernel / conv1x1_hs_kernel (plain weights, NB = 2 and the -nb4 cases NB = 4) and conv_ws_h2_kernel /
    conv_ws_hs_kernel (fragment-major).  The UDP_POSE_DEBUG_TILES report names the arm every launch took."""
    ks, stride, cin, cout, real, h, w, n, ws, relu, res, nup, views = CONVS[name]
    nb4 = name.endswith("-nb4")
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", **({"UDP_POSE_MINWGS": "0"} if nb4 else {})):
        _verdict(kind, lambda k: _conv_direct(name, k, last, ks, stride, cin, cout, real, h, w, n, ws, relu, res, nup, views, via,
                                              seed=len(name)))
    err = capfd.readouterr().err
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
    geom = tuple(str(v) for v in (ks, stride, ho, wo, cin, cout))
    if ws:
        arms = [g[6:] for g in TILE_WS.findall(err) if g[:6] == geom]
        assert arms and not TILE_MFMA.findall(err), "not on the weight-stationary kernels: %s" % err
    else:
        arms = [g[6] for g in TILE_MFMA.findall(err) if g[:6] == geom]
        assert arms and set(arms) == {"4" if nb4 else "2"} and not TILE_WS.findall(err), (name, arms, err)


# ------------------------------------------------------------------ deconv
@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("kind", ["below", "-below", "at", "-at", "nan_in", "relu_neg"])
def test_deconv_edge(kind, last):
    """deconv4s2_kernel, 256 -> 64 on 8 x 6 -> 16 x 12, n = 3 (no addends, no views: describe_deconv refuses them)."""
    cin, cout, h, w, n = 256, 64, 8, 6, 3
    relu = 1 if kind == "relu_neg" else 0

    def run(k):
        d = _plant_conv(k, last, 4, 2, cin, cout, cout, h, w, n, False, 0, relu, 77, transposed=True)
        packed, wexp = f16x2.pack_deconv_weights_ws(d["wt"], cout)
        bp = d["bias"].clone()
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DECONV, 4, 2, relu
        op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cout, 1, wexp
        op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
        out = _nan(H2, n, 2 * h, 2 * w, cout)
        assert _call(op, H2, n, _dev(d["x"].permute(0, 2, 3, 1), H2), packed.cuda(), bp.cuda(), out) == 0, _lib.lib().udp_last_error()
        _judge("deconv", k, d, _host(out, H2).permute(0, 3, 1, 2), relu)
    _verdict(kind, run)


# ------------------------------------------------------------------ grouped convs, second outputs, chained 1x1 (programs)
def _micro_conv(m, d, c, h, w, ws, group=0, relu=1, **extra):
    """One planted 3x3 stride-1 conv c -> c + residual in the micro-program ``m``; returns its output buffer."""
    bx, br, bo = m.buf(h, w, c), m.buf(h, w, c), m.buf(h, w, c)
    m.fill(bx, d["x"])
    m.fill(br, d["r"])
    m.add(new_op(_lib.UDP_OP_CONV, ks=3, stride=1, relu=relu, cin=c, cout=c, hin=h, win=w, hout=h, wout=w, in_buf=bx, res_buf=br,
                 out_buf=bo, group=group, **extra, **m.put_conv(d["wt"], d["bias"], ws=ws)))
    m.wrote(bo)
    return bo


GROUPED = {
    # name: (ws, n, maps deepest-K first, the planted member, {(h, w, c): PB the report must show}): the cases of
    # tests/test_gpu_ws_pb8.py.  A weight-stationary conv joins the merged launch (conv_ws_multi) exactly when it reports
    # PB = 6 or 8 (describe_conv_ws -> groupable); PB = 8 beside a PB = 4 sibling runs alone, on conv_ws_pb8_kernel.  A
    # plain-weight conv is a member of conv_mfma_multi exactly when describe_conv_grouped reports it ("grouped conv").
    "ws-multi": (True, 2, [(64, 24, 8), (32, 48, 16)], 0, {(24, 8, 64): 6, (48, 16, 32): 6}),
    "ws-multi-pb8-member": (True, 3, [(64, 24, 8), (32, 32, 16)], 1, {(24, 8, 64): 6, (32, 16, 32): 8}),
    "ws-pb8": (True, 3, [(64, 16, 8), (32, 32, 16)], 1, {(16, 8, 64): 4, (32, 16, 32): 8}),
    "mfma-multi": (False, 3, [(64, 24, 8), (32, 32, 16)], 1, None),
}


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("kind", ["below", "at", "relu_neg", "nan_res"])
@pytest.mark.parametrize("name", sorted(GROUPED))
def test_grouped_convs_edge(name, kind, last, capfd):
    ws, n, maps, planted, want = GROUPED[name]
    relu = 0 if kind == "nan_res" else 1

    def run(k):
        m = Micro(H2, n, seed=5)
        ds, bufs = [], []
        for j, (c, h, w) in enumerate(maps):
            d = _plant_conv(k if j == planted else "clean", last, 3, 1, c, c, c, h, w, n, True, 0, relu, 100 + j)
            ds.append(d)
            bufs.append(_micro_conv(m, d, c, h, w, ws, group=1, relu=relu))
        capfd.readouterr()
        with _env(UDP_POSE_DEBUG_TILES="1"):
            assert m.run() == 0, m.error
        err = capfd.readouterr().err
        if ws:
            arms = {(int(g[2]), int(g[3]), int(g[4])): int(g[6]) for g in TILE_WS.findall(err) if g[0] == "3"}
            assert arms == want, (name, arms, want)
        else:
            members = {(int(g[0]), int(g[1]), int(g[2])) for g in TILE_GROUPED.findall(err)}
            assert members == {(h, w, c) for c, h, w in maps}, (name, members, err)
        for j, d in enumerate(ds):
            _judge("%s member %d" % (name, j), k if j == planted else "clean", d, m.read(bufs[j]), relu)
        m.assert_untouched()
        m.check_head()
    _verdict(kind, run)


@pytest.mark.parametrize("kind", ["below", "at", "nan_add2"])
def test_second_output_edge(kind):
    """conv_ws.hip:422 / :442: out stays small, out2 = out (as stored) + add2 is what reaches the edge.  add2 holds 65472
    at one element and out holds bias[c0] = 47.99609375 or 48 there (exact in the format: 22 bits), so the sum is T or 65520
    exactly; ``nan_add2``: a NaN in the addend."""
    c, h, w, n = 32, 9, 7, 3

    def run(k):
        m = Micro(H2, n, seed=9)
        d = _plant_conv("below" if k != "clean" else "clean", True, 3, 1, c, c, c, h, w, n, False, 0, 1, 31)
        n0, c0, yo, xo = d["at"]
        if k != "clean":
            d["x"][n0, 0, yo, xo] = 0                              # no 65472 from the conv: out[c0, p0] = bias[c0]
            d["bias"][c0] = 48.0 if k == "at" else BELOW - 65472.0
        add = m.randn(n, c, h, w)
        if k in ("below", "at"):
            add[n0, c0, yo, xo] = 65472.0
        elif k == "nan_add2":
            add[n0, c0, yo, xo] = float("nan")
        bx, bo, ba, b2 = m.buf(h, w, c), m.buf(h, w, c), m.buf(h, w, 96), m.buf(h, w, 96)
        xq, aq = m.fill(bx, d["x"]), m.fill(ba, add, coff=32)
        m.add(new_op(_lib.UDP_OP_CONV, ks=3, stride=1, relu=1, cin=c, cout=c, hin=h, win=w, hout=h, wout=w, in_buf=bx, out_buf=bo,
                     n_out2=1, out2_buf=[b2], out2_coff=[32], out2_pitch=[96], add2_buf=[ba], add2_coff=[32], add2_pitch=[96],
                     **m.put_conv(d["wt"], d["bias"], ws=True)))
        m.wrote(bo)
        m.wrote(b2, 32, c)
        assert m.run() == 0, m.error
        out, out2 = m.read(bo), m.read(b2, 32, c)
        ref = mp.ref_conv(xq.double(), d["wt"], d["bias"], relu=True)
        assert float((out.double() - ref).abs().max()) <= mp.conv_tol(H2, ref)
        assert float(out.abs().max()) < 100
        mask = torch.zeros(out.shape, dtype=torch.bool)
        if k != "clean":
            mask[n0, c0, yo, xo] = True
        assert torch.equal(out2[~mask], _q(out + aq)[~mask])        # bit for bit, as the header promises
        if k in ("below", "at"):
            _chosen("out2", k, out2[n0, c0, yo, xo])
        m.assert_untouched()
    _verdict(kind, run)


CHAIN = [("out", k) for k in ("below", "at", "relu_neg", "nan_res")] + [("chained", k) for k in ("below", "at", "relu_neg")]


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("site,kind", CHAIN)
def test_chain_edge(site, kind, last):
    """conv_chain_kernel: 1x1 conv 64 -> 256 + residual (+ ReLU) at conv_ws.hip:1140, chained into a 1x1 conv 256 -> 64 at
    :1183.  ``chained``: the first conv's output holds 32736 at one element of channel 0 and the second conv doubles it."""
    cin, h, w, n = 64, 9, 7, 3                     # (the chained conv has no residual of its own: no nan_res there)

    def run(k):
        m = Micro(H2, n, seed=3)
        relu1 = 0 if k == "nan_res" else 1
        k1, k2 = (k, "clean") if site == "out" else ("clean", k)
        d1 = _plant_conv(k1, last, 1, 1, cin, 256, 256, h, w, n, True, 0, relu1, 41)
        bi, br, bo, bc = m.buf(h, w, cin), m.buf(h, w, 256), m.buf(h, w, 256), m.buf(h, w, 64)
        if site == "chained" and k != "clean":
            # the first conv delivers the second one's operand: out1[:, 0] = 0 but for 32736 at the chosen pixel
            d1["wt"][0] = 0
            d1["bias"][0] = 0
            d1["r"][:, 0] = 0
            n0, _, yo, xo = _plant_conv(k2, last, 1, 1, 256, 64, 64, h, w, n, False, 0, 1, 42)["at"]
            d1["r"][n0, 0, yo, xo] = BIG
        xq, rq = m.fill(bi, d1["x"]), m.fill(br, d1["r"])
        d2 = _plant_conv(k2, last, 1, 1, 256, 64, 64, h, w, n, False, 0, 1, 42)
        packed, wexp2 = f16x2.pack_weights_ws(d2["wt"].reshape(1, 64, 256))
        m.add(new_op(_lib.UDP_OP_CONV, relu=relu1, cin=cin, cout=256, hin=h, win=w, hout=h, wout=w, in_buf=bi, res_buf=br, out_buf=bo,
                     chain_cout=64, chain_buf=bc, chain_relu=1, chain_wexp=wexp2, w2_off=m.put(packed.numpy().tobytes()),
                     b2_off=m.put(d2["bias"].numpy().tobytes()), **m.put_conv(d1["wt"], d1["bias"], ws=True)))
        m.wrote(bo)
        m.wrote(bc)
        assert m.run() == 0, m.error
        out, chained = m.read(bo), m.read(bc)
        ref1 = mp.ref_conv(xq.double(), d1["wt"], d1["bias"], res=rq.double(), relu=bool(relu1))
        _judge("chain.out", k1, dict(d1, ref=ref1), out, relu1)
        src = torch.where(torch.isfinite(out), out, torch.zeros(())).double()
        ref2 = mp.ref_conv(src, d2["wt"], d2["bias"], relu=True)                      # of the first conv's output AS STORED
        mask2 = d2["mask"] | (~torch.isfinite(out)).any(dim=1, keepdim=True).expand_as(ref2)   # pixels that read a non-finite value
        _judge("chain.chained", k2, dict(d2, ref=ref2, mask=mask2), chained, 1)
        m.assert_untouched()
    _verdict(kind, run)


# =================================================================== per-pixel ops with a bias or a beta
@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("kind", ["below", "-below", "at", "-at", "relu_neg", "nan_in"])
@pytest.mark.parametrize("view", [False, True], ids=["plain", "views"])
@pytest.mark.parametrize("hw", [(2, 2), (7, 5)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ks", [3, 5, 7])
def test_dwconv_edge(ks, hw, view, kind, last):
    """dwconv3_kernel / dwconvk_kernel: depthwise, so x = 32736 at one element, the centre tap of its channel = 2 and
    the channel's other taps 0; the NaN of ``nan_in`` reaches one channel only -- its h2_split8 siblings are finite."""
    (h, w), c, n = hw, 64, 3
    relu = 1 if kind == "relu_neg" else 0

    def run(k):
        g = torch.Generator().manual_seed(ks + h)
        x = torch.randn(n, c, h, w, generator=g)
        wt = torch.randn(c, 1, ks, ks, generator=g) * float(np.sqrt(2.0 / (ks * ks)))
        bt = torch.randn(c, generator=g) * 0.1
        n0, c0, y0, x0 = (n - 1, c - 1, h - 1, w - 1) if last else (0, 0, 0, 0)
        mask = torch.zeros(n, c, h, w, dtype=torch.bool)
        if k in EDGES:
            sign = -1.0 if k.startswith("-") else 1.0
            x[:, c0] = 0
            wt[c0] = 0
            x[n0, c0, y0, x0] = BIG
            wt[c0, 0, ks // 2, ks // 2], bt[c0] = (-3.0, 0.25) if k == "relu_neg" else (sign * W0, sign * (abs(_target(k)) - BIG * W0))
            mask[n0, c0, y0, x0] = True
        elif k == "nan_in":
            x[n0, c0, y0, x0] = float("nan")
            mask[n0, c0] = True
        x = _q(x)
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, ks, 1, relu
        op.cin, op.cout, op.cout_pad = c, c, c
        op.hin, op.win, op.hout, op.wout = h, w, h, w
        ip, ic, opi, oc = (128, 32, 160, 64) if view else (c, 0, c, 0)
        if view:
            op.in_coff, op.in_pitch, op.out_coff, op.out_pitch = ic, ip, oc, opi
        xin = torch.full((n, h, w, ip), float("nan"))                               # NaN outside the slice must not be seen
        xin[..., ic:ic + c] = x.permute(0, 2, 3, 1)
        out = _dev(torch.full((n, h, w, opi), POISON), H2)
        before = out.clone()
        assert _call(op, H2, n, _dev(xin, H2), wt.reshape(c, ks * ks).t().contiguous().cuda(), bt.cuda(), out) == 0, _lib.lib().udp_last_error()
        keep = torch.ones(opi, dtype=torch.bool)
        keep[oc:oc + c] = False
        assert torch.equal(out.cpu()[..., keep].view(torch.int16), before.cpu()[..., keep].view(torch.int16))
        got = _host(out, H2)[..., oc:oc + c].permute(0, 3, 1, 2)
        ref = lambda dt: (F.relu if relu else (lambda t: t))(F.conv2d(torch.nan_to_num(x).to(dt), wt.to(dt), bt.to(dt), padding=ks // 2, groups=c))
        r64, r32 = ref(torch.float64), ref(torch.float32)
        e32 = float((r32.double() - r64)[~mask].abs().max())
        _others("dwconv k%d %s" % (ks, k), got, r64, mask, lambda r: 3 * e32 + 4 * mp.ULP[H2] * float(r.abs().max()))
        if k in EDGES:
            _chosen("dwconv k%d %s" % (ks, k), k, got[n0, c0, y0, x0])
        if k == "nan_in":
            sib = got[n0, c0 & ~7:(c0 & ~7) + 8, y0, x0]
            assert int(torch.isnan(sib).sum()) == 1
    _verdict(kind, run)


def _norm_case(which, k, last):
    """GroupNorm(1, C) / LayerNorm: out = gamma * xhat + beta.  gamma[c0] = 0 makes channel c0's output beta[c0] itself
    (0 * xhat is exact), an fp32 operand; every pixel of that channel lands on the target."""
    c, r = (GN_CR[2] if which == "gnorm" else LN_CR[2])                            # 160 stored / 144 real, 96 / 80
    h, w, n = 7, 5, 3
    data, mk, ref = (_gn_data, _gn_op, _gn_ref) if which == "gnorm" else (_ln_data, _ln_op, _ln_ref)
    x, gam, bet, block, g = data(c, r, h, w, n, H2)
    c0 = r - 1 if last else 0
    mask = torch.zeros(n, r, h, w, dtype=torch.bool)
    if k in EDGES:
        gam[c0], bet[c0] = 0.0, _target(k)
        block[0, c0], block[1, c0] = 0.0, _target(k)                                 # the device's [gamma; beta] rows
        mask[:, c0] = True
    elif k == "nan_in":
        x[n - 1 if last else 0, c0, h - 1 if last else 0, w - 1 if last else 0] = float("nan")
        mask[n - 1 if last else 0] = True                                            # gnorm: the image; lnorm: the pixel (a subset)
    out = _nan(H2, n, h, w, c)
    assert _call(mk(c, r, h, w), H2, n, _dev(x.permute(0, 2, 3, 1), H2), block, None, out) == 0, _lib.lib().udp_last_error()
    got = _host(out, H2).permute(0, 3, 1, 2)[:, :r]
    xs = torch.nan_to_num(x, nan=3.0)
    r64, r32 = ref(xs, gam, bet, torch.float64), ref(xs, gam, bet, torch.float32)
    e32 = float((r32.double() - r64)[~mask].abs().max())
    _others("%s %s" % (which, k), got, r64, mask, lambda t: 3 * e32 + 4 * mp.ULP[H2] * float(t.abs().max()))
    if k in EDGES:
        for v in (got[0, c0, 0, 0], got[n - 1, c0, h - 1, w - 1]):
            _chosen("%s %s" % (which, k), k, v)
    if k != "nan_in":
        assert int(_host(out, H2)[..., r:].abs().max()) == 0                         # the pad channels: exact zeros


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("kind", ["below", "-below", "at", "-at", "nan_in"])
@pytest.mark.parametrize("which", ["gnorm", "lnorm"])
def test_norm_edge(which, kind, last):
    _verdict(kind, lambda k: _norm_case(which, k, last))


# =================================================================== UDP_OP_FUSE
FUSE_KINDS = ["below", "-below", "at", "-at", "relu_neg", "nan_in", "nan_res", "nan_up0", "nan_up1"]      # nan_up<u>: addend u
FUSE = [(h, w, nup, k) for h, w, nup in [(2, 2, 1), (7, 5, 0), (8, 12, 2)] for k in FUSE_KINDS
        if not k.startswith("nan_up") or int(k[-1]) < nup]


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("h,w,nup,kind", FUSE)
def test_fuse_edge(h, w, nup, kind, last):
    """fuse_sum_kernel: in + res (+ upsampled addends), every operand a channel slice.  All operands are stored values
    (22 bits), so T is the exact fp32 sum of two of them: in = 65472 and res = 47.99609375 (or 48)."""
    c, n = 32, 3
    relu = 1 if kind == "relu_neg" else 0

    def run(k):
        g = torch.Generator().manual_seed(h * 10 + w)
        x, r = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
        ups = [torch.randn(n, c, h >> (u + 1), w >> (u + 1), generator=g) for u in range(nup)]
        n0, c0, y0, x0 = (n - 1, c - 1, h - 1, w - 1) if last else (0, 0, 0, 0)
        mask = torch.zeros(n, c, h, w, dtype=torch.bool)
        if k != "clean":
            mask[n0, c0, y0, x0] = True
            for u, t in enumerate(ups):
                t[n0, c0, y0 >> (u + 1), x0 >> (u + 1)] = 0
        if k in EDGES:
            sign = -1.0 if k.startswith("-") else 1.0
            x[n0, c0, y0, x0], r[n0, c0, y0, x0] = (-BIG * W0, -BIG) if k == "relu_neg" else (sign * BIG * W0, sign * (abs(_target(k)) - BIG * W0))
        elif k == "nan_in":
            x[n0, c0, y0, x0] = float("nan")
        elif k == "nan_res":
            r[n0, c0, y0, x0] = float("nan")
        elif k.startswith("nan_up"):
            u = int(k[-1])
            ups[u][n0, c0, y0 >> (u + 1), x0 >> (u + 1)] = float("nan")
            mask[n0, c0] = True
        x, r, ups = _q(x), _q(r), [_q(t) for t in ups]
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_FUSE, 1, 1, relu
        op.cin, op.cout, op.cout_pad = c, c, c
        op.hin, op.win, op.hout, op.wout = h, w, h, w
        op.in_coff, op.in_pitch, op.res_coff, op.res_pitch, op.out_coff, op.out_pitch = 32, 96, 16, 64, 64, 128
        op.n_up = nup
        for u in range(nup):
            op.up_shift[u] = u + 1
        d_u = [_dev(t.permute(0, 2, 3, 1), H2) for t in ups] + [None] * (3 - nup)
        d_x, d_r = _dev(_wide(x, (32, 96), float("nan")), H2), _dev(_wide(r, (16, 64), float("nan")), H2)    # NaN outside the slices
        out = _dev(torch.full((n, h, w, 128), POISON), H2)
        before = out.clone()
        _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[H2], n, _lib.ptr(d_x), None, None, _lib.ptr(d_r), _lib.ptr(d_u[0]),
                                               _lib.ptr(d_u[1]), _lib.ptr(d_u[2]), _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        keep = torch.ones(128, dtype=torch.bool)
        keep[64:96] = False
        assert torch.equal(out.cpu()[..., keep].view(torch.int16), before.cpu()[..., keep].view(torch.int16))
        got = _host(out, H2)[..., 64:96].permute(0, 3, 1, 2)
        clean = lambda t: torch.nan_to_num(t)
        ref = lambda dt: mp.ref_fuse(clean(x).to(dt), clean(r).to(dt), [(clean(t).to(dt), u + 1) for u, t in enumerate(ups)], bool(relu))
        r64 = ref(torch.float64)
        e32 = float((ref(torch.float32).double() - r64)[~mask].abs().max())
        _others("fuse %dx%d %s" % (h, w, k), got, r64, mask, lambda t: 3 * e32 + 4 * mp.ULP[H2] * float(t.abs().max()))
        if k in EDGES:
            _chosen("fuse %dx%d %s" % (h, w, k), k, got[n0, c0, y0, x0])
        if k.startswith("nan"):
            sib = got[n0, c0 & ~3:(c0 & ~3) + 4, y0, x0]
            assert int(torch.isnan(sib).sum()) == 1, "the NaN lane is meant to sit among 3 finite st4 siblings"
    _verdict(kind, run)


# =================================================================== stems
STEMS = {
    "3-mfma": (3, {}), "3-valu": (3, {"UDP_POSE_STEM_VALU": "1"}),
    "7-lds": (7, {}), "7-valu": (7, {"UDP_POSE_STEM_VALU": "1"}), "7-gather": (7, {"UDP_POSE_STEM7_GATHER": "1"}),
}


def _stem_micro(ks, n, in_h, in_w, flip, c0=None, bias=None):
    """A micro-program whose stem has output channel c0's weights zeroed and its bias set: that channel's output is
    relu(bias) at every pixel."""
    m = Micro(H2, n, in_h, in_w, flip=flip, stem_ks=ks, seed=ks + n)
    if c0 is not None:
        m.stem_w[c0] = 0
        m.stem_b[c0] = bias
        m._blob[0] = (m._blob[0][0], m.stem_w.permute(2, 3, 1, 0).contiguous().numpy().tobytes())
        m._blob[1] = (m._blob[1][0], m.stem_b.numpy().tobytes())
    return m


@pytest.mark.parametrize("c0", [0, 63])
@pytest.mark.parametrize("kind", ["below", "at", "relu_neg"])
@pytest.mark.parametrize("variant", sorted(STEMS))
def test_stem_output_edge(variant, kind, c0):
    """The stems' own stores (h2_split8 in the MFMA kernels, st4 in the VALU ones): 64 x 96 input, Wout = 48 = a full and
    a ragged 32-column tile of stem7_lds_kernel, n = 3 with the flip-test half."""
    ks, env = STEMS[variant]
    n, in_h, in_w = 3, 64, 96

    def run(k):
        m = _stem_micro(ks, n, in_h, in_w, True, *((None, None) if k == "clean" else (c0, -1e5 if k == "relu_neg" else _target(k))))
        with _env(**env):
            assert m.run() == 0, m.error
        got = m.read(m.stem_buf)
        xx = torch.cat([m.x, torch.flip(m.x, [3])])
        ref = lambda d: mp.ref_conv(xx.to(d), m.stem_w, m.stem_b, stride=2, relu=True)
        r64 = ref(torch.float64)
        mask = torch.zeros(r64.shape, dtype=torch.bool)
        if k != "clean":
            mask[:, c0] = True
        e32 = float((ref(torch.float32).double() - r64)[~mask].abs().max())
        _others("stem %s %s" % (variant, k), got, r64, mask, lambda t: 3 * e32 + 4 * mp.ULP[H2] * float(t.abs().max()))
        if k != "clean":
            for v in (got[0, c0, 0, 0], got[-1, c0, -1, -1]):
                _chosen("stem %s %s" % (variant, k), k, v)
        m.assert_untouched()
        m.check_head()
    _verdict(kind, run)


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("pixel", [7e4, -7e4, float("nan")], ids=["7e4", "-7e4", "nan"])
@pytest.mark.parametrize("variant", sorted(STEMS))
def test_stem_input_pixel(variant, pixel, flip, last):
    """One pixel of the fp32 image outside fp16's range, or NaN.  The MFMA stems split the image in registers: hi = inf,
    lo = -inf, the products are NaN and the ReLU stores 0 -- nothing a downstream check could see.  The flag is raised
    where the pixel is loaded; the VALU stems give the same verdict."""
    ks, env = STEMS[variant]
    n = 3

    def run(k):
        m = _stem_micro(ks, n, 32, 32, flip)
        if k != "clean":
            m.x[(n - 1, 2, 31, 31) if last else (0, 0, 0, 0)] = pixel
        with _env(**env):
            assert m.run() == 0, m.error
        if k == "clean":
            m.assert_untouched()
            m.check_head()
    _verdict("at", run)


# =================================================================== ops that cannot leave the range from in-range inputs
def _extremes(t, last):
    """+-65504 on a few elements of ``t`` [n, c, h, w], among them the first and the last element."""
    n, c, h, w = t.shape
    t[0, 0, 0, 0], t[n - 1, c - 1, h - 1, w - 1] = TOP, -TOP
    t[n // 2, c // 2, h // 2, w // 2] = -TOP if last else TOP
    return t


@pytest.mark.parametrize("h,w", [(2, 2), (7, 5)])
@pytest.mark.parametrize("op_name", ["maxpool", "bilinear-same", "bilinear-up", "pixshuf"])
def test_selections_stay_silent(op_name, h, w):
    """Max-pool, bilinear resize and PixelShuffle of inputs that reach +-65504: no flag; selections bit-equal."""
    n, c = 3, 64
    _flag(reset=True)
    if op_name == "pixshuf":
        g = torch.Generator().manual_seed(h)
        x = _q(_extremes(torch.randn(n, 128, h, w, generator=g), False))
        cq = 32
        perm = torch.tensor([4 * (p % cq) + p // cq for p in range(128)])
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride = _lib.UDP_OP_PIXSHUF, 1, 1
        op.cin, op.cout, op.cout_pad = 128, cq, 32
        op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
        out = _nan(H2, n, 2 * h, 2 * w, cq)
        assert _call(op, H2, n, _dev(x[:, perm].permute(0, 2, 3, 1), H2), None, None, out) == 0, _lib.lib().udp_last_error()
        assert torch.equal(_host(out, H2).permute(0, 3, 1, 2), F.pixel_shuffle(x, 2))
    else:
        m = Micro(H2, n, seed=h)
        ho, wo = {"maxpool": ((h - 1) // 2 + 1, (w - 1) // 2 + 1), "bilinear-same": (h, w), "bilinear-up": (2 * h + 1, 2 * w - 1)}[op_name]
        bi, bo = m.buf(h, w, c), m.buf(ho, wo, c)
        x = m.randn(n, c, h, w)
        x[1] = TOP                                              # a whole image at the top: every interpolation weight sums there
        x[2, :, ::2] = -TOP
        xq = m.fill(bi, _extremes(x, False))
        kind = _lib.UDP_OP_MAXPOOL if op_name == "maxpool" else _lib.UDP_OP_BILINEAR
        m.add(new_op(kind, ks=3 if op_name == "maxpool" else 1, stride=2 if op_name == "maxpool" else 1, cin=c, cout=c, hin=h, win=w,
                     hout=ho, wout=wo, in_buf=bi, out_buf=bo))
        m.wrote(bo)
        assert m.run() == 0, m.error
        got = m.read(bo)
        if op_name == "maxpool":
            assert torch.equal(got, mp.ref_maxpool(xq))
        elif op_name == "bilinear-same":
            assert torch.equal(got, xq)
        else:
            ref = mp.ref_bilinear(xq.double(), ho, wo)
            # four fp32 roundings of the weights and sums: within 2^-21 of 65504, far from 65520
            assert torch.isfinite(got).all() and float(got.abs().max()) <= TOP * (1 + 2.0 ** -21)
            e32 = float((mp.ref_bilinear(xq, ho, wo).double() - ref).abs().max())
            assert float((got.double() - ref).abs().max()) <= 3 * e32 + 4 * mp.ULP[H2] * TOP
        m.assert_untouched()
    assert not _flag(reset=True), "%s raised the range flag on in-range inputs" % op_name


def _se_run(x, w1, b1, w2, cs, real, h, w, n):
    hid = real // 4
    w1t, w2t = torch.zeros(cs, hid), torch.zeros(hid, cs)
    w1t[:real], w2t[:, :real] = w1.t(), w2.t()
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_SE, 1, 1, 0
    op.cin, op.cout, op.cout_pad, op.chain_cout = cs, cs, cs, hid
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    out = _nan(H2, n, h, w, cs)
    assert _call(op, H2, n, _dev(x.permute(0, 2, 3, 1), H2), torch.cat([w1t.reshape(-1), b1, w2t.reshape(-1)]).cuda(), None, out) == 0, \
        _lib.lib().udp_last_error()
    return _host(out, H2).permute(0, 3, 1, 2)


@pytest.mark.parametrize("h,w", [(2, 2), (7, 5)])
def test_se_stays_silent_and_propagates_nan(h, w):
    """se_kernel: out = x * gate with a hard-sigmoid gate in [0, 1]: one multiplication by at most 1 cannot leave the
    range that x = +-65504 is in, and the flag stays clear.  A NaN element is stored as NaN and raises it."""
    cs, real, n = 32, 26, 3
    g = torch.Generator().manual_seed(h)
    x = torch.zeros(n, cs, h, w)
    x[:, :real] = torch.randn(n, real, h, w, generator=g)
    x[:, :real] = _extremes(x[:, :real].clone(), False)
    x = _q(x)
    w1 = torch.randn(real // 4, real, generator=g) * 0.3
    b1 = torch.randn(real // 4, generator=g) * 0.3
    w2 = torch.randn(real, real // 4, generator=g)
    _flag(reset=True)
    got = _se_run(x, w1, b1, w2, cs, real, h, w, n)
    r64, m64 = _se_ref(x, w1, b1, w2, torch.float64)
    r32, _ = _se_ref(x, w1, b1, w2, torch.float32)
    e_hip, e_cpu, gate = mp.parity("se at the edge %dx%d" % (h, w), got[:, :real], r64, r32, mp.ULP[H2])
    assert e_hip <= gate and float(got.abs().max()) <= TOP
    assert not _flag(reset=True)
    x[n - 1, real - 1, h - 1, w - 1] = float("nan")
    got = _se_run(x, w1, b1, w2, cs, real, h, w, n)
    assert torch.isnan(got[n - 1, real - 1, h - 1, w - 1]) and torch.isfinite(got[:n - 1]).all()
    assert _flag(reset=True) and not _flag(reset=True)


@pytest.mark.parametrize("code", [SILU, HS], ids=["silu", "hswish"])
@pytest.mark.parametrize("h,w", [(2, 2), (7, 5)])
def test_act_stays_silent_and_propagates_nan(h, w, code):
    """act_kernel: |silu(x)| <= |x| and |hswish(x)| <= |x|, and both are x itself at +65504 and -0 at -65504.  One NaN
    element gives ONE NaN lane among 7 finite h2_split8 siblings."""
    n, c = 3, 32
    g = torch.Generator().manual_seed(h + code)
    x = _q(_extremes(torch.randn(n, c, h, w, generator=g) * 3.0, False))
    f = (lambda t: t * (1 / (1 + torch.exp(-t)))) if code == SILU else (lambda t: t * (torch.clamp(t + 3, 0, 6) / 6))
    run = lambda t: _host(_act_call(t, c, h, w, n, code), H2).permute(0, 3, 1, 2)
    _flag(reset=True)
    got = run(x)
    e_hip, e_cpu, _ = mp.parity("act %d at the edge %dx%d" % (code, h, w), got, f(x.double()), f(x), mp.ULP[H2])
    assert e_hip <= e_cpu + 4 * mp.ULP[H2]
    assert float(got[0, 0, 0, 0]) == TOP and float(got[n - 1, c - 1, h - 1, w - 1]) == 0.0
    assert not _flag(reset=True)
    for at in ((0, 0, 0, 0), (n - 1, c - 1, h - 1, w - 1)):
        y = x.clone()
        y[at] = float("nan")
        got = run(y)
        assert int(torch.isnan(got).sum()) == 1 and torch.isnan(got[at])
        assert _flag(reset=False) and _flag(reset=True) and not _flag(reset=True), at
    run(x)
    assert not _flag(reset=True)


def _act_call(x, c, h, w, n, code):
    out = _nan(H2, n, h, w, c)
    assert _call(_act_op(c, h, w, code), H2, n, _dev(x.permute(0, 2, 3, 1), H2), None, None, out) == 0, _lib.lib().udp_last_error()
    return out


@pytest.mark.parametrize("last", [False, True], ids=_ids)
@pytest.mark.parametrize("kind", ["below", "at", "nan_in"])
@pytest.mark.parametrize("h,w", [(2, 2), (4, 2)])
def test_linattn_edge(h, w, kind, last):
    """linattn_kernel: out = relu(v) * ctx, ctx = the soft-max-weighted mean of the keys of the pixel's parity class -- a
    product of two stored values, so it CAN leave the range.  The query puts all the weight of the chosen pixel's class on
    it (the others at -200: exp underflows to 0, the weights are exactly 1 and 0), so out[c0, p0] = v * k exactly, with
    v = 2 and k = 32760 - 2^-7 -> 65519.984375 (the largest product under 65520 these operands reach; exact in the
    format), or k = 32760 -> 65520.  ``nan_in``: a NaN key: every pixel of its class in ONE channel."""
    c, r = LA_C[0]
    n = 3

    def run(k):
        q, key, v, stored, g = _la_data(c, r, h, w, n, H2, 1.0)
        n0, c0, y0, x0 = (n - 1, r - 1, h - 1, w - 1) if last else (0, 0, 0, 0)
        mask = torch.zeros(n, r, h, w, dtype=torch.bool)
        if k != "clean":
            q[n0, 0, y0 & 1::2, x0 & 1::2] = -200.0
            q[n0, 0, y0, x0] = 0.0
            v[n0, c0, y0 & 1::2, x0 & 1::2] = 0.0
            v[n0, c0, y0, x0] = 2.0
            key[n0, c0, y0, x0] = {"below": 32760.0 - 2.0 ** -7, "at": 32760.0, "nan_in": float("nan")}[k]
            mask[n0, c0, y0 & 1::2, x0 & 1::2] = True
        stored = torch.zeros(n, h, w, 2 * c + 32)
        stored[..., :c], stored[..., c:2 * c], stored[..., 2 * c] = key.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), q[:, 0]
        out = _nan(H2, n, h, w, c)
        assert _call(_la_op(c, h, w), H2, n, _dev(stored, H2), None, None, out) == 0, _lib.lib().udp_last_error()
        got = _host(out, H2).permute(0, 3, 1, 2)[:, :r]
        kk = torch.nan_to_num(key)
        ref = lambda dt: linear_attention_core(q.to(dt), kk[:, :r].to(dt), v[:, :r].to(dt))
        r64 = ref(torch.float64)
        e32 = float((ref(torch.float32).double() - r64)[~mask].abs().max())
        _others("linattn %dx%d %s" % (h, w, k), got, r64, mask, lambda t: 3 * e32 + 4 * mp.ULP[H2] * float(t.abs().max()))
        if k == "below":
            assert float(got[n0, c0, y0, x0]) == 65519.984375, float(got[n0, c0, y0, x0])
        if k == "nan_in":
            sib = got[n0, c0 & ~7:(c0 & ~7) + 8, y0, x0]
            assert torch.isnan(got[n0, c0, y0, x0]) and int(torch.isnan(sib).sum()) == 1
    _verdict(kind, run)


@pytest.mark.parametrize("h,w", [(2, 2), (4, 2)])
@pytest.mark.parametrize("dh", [MH_D[4], MH_D[0]], ids=lambda s: "dp%d-d%d-h%d" % s)
def test_mhattn_stays_silent_and_propagates_nan(dh, h, w):
    """mhattn_kernel (attn.hip:293, a per-value check): a convex sum of values that reach +-65504 stays in range; a NaN
    value raises the flag."""
    dp, d, heads = dh
    n = 3
    q, k, v, stored, g = _mh_data(dp, d, h, w, n, H2, 1.0)
    v = _q(_extremes(v, False))

    def run(vv):
        st = torch.zeros(n, h, w, 3 * dp)
        for s, t in enumerate((q, k, vv)):
            st[..., s * dp:s * dp + d] = t.permute(0, 2, 3, 1)
        out = _nan(H2, n, h, w, dp)
        assert _call(_mh_op(dp, d, heads, h, w), H2, n, _dev(st, H2), None, None, out) == 0, _lib.lib().udp_last_error()
        return _host(out, H2).permute(0, 3, 1, 2)
    _flag(reset=True)
    got = run(v)
    _mh_check("mhattn at the edge dp%d %dx%d" % (dp, h, w), q, k, v, got, d, heads, H2)
    assert float(got.abs().max()) <= TOP * (1 + 2.0 ** -20)        # soft-max weights sum to 1 within a few fp32 roundings
    assert not _flag(reset=True)
    v2 = v.clone()
    v2[n - 1, d - 1, h - 1, w - 1] = float("nan")
    got = run(v2)
    assert torch.isnan(got[n - 1, d - 1]).any() and torch.isfinite(got[:n - 1]).all()
    assert _flag(reset=True) and not _flag(reset=True)
    run(v)
    assert not _flag(reset=True)


def _psa_run(x, theta, P, c, h, w, n):
    m = Micro(H2, n, seed=c + h)
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
    m.assert_untouched()
    return xq, thq, m.read_rows(bmask), m.read(bx1), m.read(bx2)


@pytest.mark.parametrize("c,h,w", [(16, 8, 6), (64, 9, 7)])
def test_psa_stays_silent_and_propagates_nan(c, h, w):
    """psa_scale_kernel / psa_sp_kernel (psa.hip:43, per-value checks): a sigmoid times a stored value.  x reaches
    +-65504 on a few elements; a NaN element of x makes the image's pooled rows NaN and with them every lane."""
    n = 3
    x, theta, P = mp.psa_inputs(c, h, w, n)
    x = _extremes(x, False)
    _flag(reset=True)
    xq, thq, mask, x1, x2 = _psa_run(x, theta, P, c, h, w, n)
    ref1 = mp.psa_scale(xq.double(), mask.double())
    ref2 = mp.psa_sp(thq.double(), x1.double(), mask.double())
    for name, got, ref, r32 in (("scale", x1, ref1, mp.psa_scale(xq, mask)), ("sp", x2, ref2, mp.psa_sp(thq, x1, mask))):
        e_hip, e_cpu, gate = mp.parity("psa %s at the edge C%d" % (name, c), got, ref, r32, mp.ULP[H2])
        assert e_hip <= gate and float(got.abs().max()) <= TOP
    assert not _flag(reset=True)
    x[n - 1, c - 1, h - 1, w - 1] = float("nan")
    _, _, _, x1, x2 = _psa_run(x, theta, P, c, h, w, n)
    assert torch.isnan(x1[n - 1]).any() and torch.isfinite(x1[:n - 1]).all() and torch.isfinite(x2[:n - 1]).all()
    assert _flag(reset=True) and not _flag(reset=True)


# =================================================================== section 2: away from unit scale
# The existing gates floor their scale at 1.0; here every gate is taken against |ref|max itself: the conv gate
# (microprog.conv_tol: 2e-5 for split fp16) for the convs, 3 * err_cpu_fp32 + 4 ulp (microprog.parity) for the rest.  The
# format's own error relative to the tensor maximum is 1.05e-7 at every one of these scales.
SCALE_EXP = [-10, 12]
CONV_REL = 2e-5


def _rel_gate(name, got, ref, rel=CONV_REL):
    mx = float(ref.abs().max())
    assert 0 < mx < 6e4, (name, mx)
    assert torch.isfinite(got).all(), "%s: output not fully written, or out of range" % name
    err = float((got.double() - ref.double()).abs().max()) / mx
    print("%-44s |ref|max %.4g  err / max %.3g (gate %.3g)" % (name, mx, err, rel))
    assert err <= rel, (name, err, rel)
    return err


def _parity_gate(name, got, r64, r32):
    assert float(r64.abs().max()) < 6e4, name
    e_hip, e_cpu, gate = mp.parity(name, got, r64, r32, mp.ULP[H2])
    assert e_hip <= gate, (name, e_hip, e_cpu, gate)


def _conv_call(d, ks, stride, cin, cout, h, w, n, ws, relu, kind=_lib.UDP_OP_CONV):
    d_w, d_b, cp, wexp = _conv_weights(d["wt"], d["bias"], ws)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = kind, ks, stride, relu
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cp, int(ws), wexp
    op.hin, op.win, op.hout, op.wout = h, w, d["ho"], d["wo"]
    out = _nan(H2, n, d["ho"], d["wo"], cout)
    res = _dev(d["r"].permute(0, 2, 3, 1), H2) if d["r"] is not None else None
    assert _call(op, H2, n, _dev(d["x"].permute(0, 2, 3, 1), H2), d_w, d_b, out, res=res) == 0, _lib.lib().udp_last_error()
    return _host(out, H2).permute(0, 3, 1, 2)


@pytest.mark.parametrize("e", SCALE_EXP)
@pytest.mark.parametrize("family", ["mfma-k3", "mfma-k1", "ws-k3", "ws-k1"])
def test_conv_away_from_unit_scale(family, e):
    """conv + residual + ReLU, 64 -> 64 on 9 x 7, n = 3; activations, residual and bias scaled by 2^e."""
    ws, ks = family.startswith("ws"), int(family[-1])
    s = 2.0 ** e
    d = _plant_conv("clean", False, ks, 1, 64, 64, 64, 9, 7, 3, True, 0, 1, 7 + ks)
    d["x"], d["r"], d["bias"] = _q(d["x"] * s), _q(d["r"] * s), d["bias"] * s
    _flag(reset=True)
    got = _conv_call(d, ks, 1, 64, 64, 9, 7, 3, ws, 1)
    ref = mp.ref_conv(d["x"].double(), d["wt"], d["bias"], res=d["r"].double(), relu=True)
    _rel_gate("conv %s 2^%d" % (family, e), got, ref)
    assert not _flag(reset=True)


@pytest.mark.parametrize("e", SCALE_EXP)
def test_deconv_away_from_unit_scale(e):
    s = 2.0 ** e
    cin, cout, h, w, n = 256, 64, 8, 6, 3
    d = _plant_conv("clean", False, 4, 2, cin, cout, cout, h, w, n, False, 0, 1, 78, transposed=True)
    x, bias = _q(d["x"] * s), d["bias"] * s
    packed, wexp = f16x2.pack_deconv_weights_ws(d["wt"], cout)
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DECONV, 4, 2, 1
    op.cin, op.cout, op.cout_pad, op.wfmt, op.wexp = cin, cout, cout, 1, wexp
    op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
    out = _nan(H2, n, 2 * h, 2 * w, cout)
    _flag(reset=True)
    assert _call(op, H2, n, _dev(x.permute(0, 2, 3, 1), H2), packed.cuda(), bias.cuda(), out) == 0, _lib.lib().udp_last_error()
    ref = F.relu(F.conv_transpose2d(x.double(), d["wt"].double(), bias.double(), stride=2, padding=1))
    _rel_gate("deconv 2^%d" % e, _host(out, H2).permute(0, 3, 1, 2), ref)
    assert not _flag(reset=True)


@pytest.mark.parametrize("e", SCALE_EXP)
def test_chained_conv_away_from_unit_scale(e):
    """The case of test_chained_1x1_conv_matches_fp64 (cin 64, 9 x 7, n = 3) with x, the residual and both biases scaled."""
    s = 2.0 ** e
    cin, h, w, n = 64, 9, 7, 3
    m = Micro(H2, n, seed=cin + h)
    bi, br, bo, bc = m.buf(h, w, cin), m.buf(h, w, 256), m.buf(h, w, 256), m.buf(h, w, 64)
    xq, rq = m.fill(bi, m.randn(n, cin, h, w) * s), m.fill(br, m.randn(n, 256, h, w) * s)
    w1 = mp.quant(m.randn(256, cin, 1, 1) * float(np.sqrt(2.0 / cin)), H2)
    w2 = mp.quant(m.randn(64, 256, 1, 1) * float(np.sqrt(2.0 / 256)), H2)
    b1, b2 = m.randn(256) * 0.1 * s, m.randn(64) * 0.1 * s
    packed, wexp2 = f16x2.pack_weights_ws(w2.reshape(1, 64, 256))
    m.add(new_op(_lib.UDP_OP_CONV, relu=1, cin=cin, cout=256, hin=h, win=w, hout=h, wout=w, in_buf=bi, res_buf=br, out_buf=bo,
                 chain_cout=64, chain_buf=bc, chain_relu=1, chain_wexp=wexp2, w2_off=m.put(packed.numpy().tobytes()),
                 b2_off=m.put(b2.numpy().tobytes()), **m.put_conv(w1, b1, ws=True)))
    m.wrote(bo)
    m.wrote(bc)
    _flag(reset=True)
    assert m.run() == 0, m.error
    out, chained = m.read(bo), m.read(bc)
    _rel_gate("chain out 2^%d" % e, out, mp.ref_conv(xq.double(), w1, b1, res=rq.double(), relu=True))
    _rel_gate("chain chained 2^%d" % e, chained, mp.ref_conv(out.double(), w2, b2, relu=True))
    assert not _flag(reset=True)
    m.assert_untouched()


@pytest.mark.parametrize("e", SCALE_EXP)
@pytest.mark.parametrize("ks", [3, 5])
def test_dwconv_away_from_unit_scale(ks, e):
    s = 2.0 ** e
    c, h, w, n = 64, 7, 5, 3
    g = torch.Generator().manual_seed(ks)
    x = _q(torch.randn(n, c, h, w, generator=g) * s)
    wt = torch.randn(c, 1, ks, ks, generator=g) * float(np.sqrt(2.0 / (ks * ks)))
    bt = torch.randn(c, generator=g) * 0.1 * s
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DWCONV, ks, 1, 0
    op.cin, op.cout, op.cout_pad = c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    out = _nan(H2, n, h, w, c)
    _flag(reset=True)
    assert _call(op, H2, n, _dev(x.permute(0, 2, 3, 1), H2), wt.reshape(c, ks * ks).t().contiguous().cuda(), bt.cuda(), out) == 0
    ref = lambda dt: F.conv2d(x.to(dt), wt.to(dt), bt.to(dt), padding=ks // 2, groups=c)
    _parity_gate("dwconv k%d 2^%d" % (ks, e), _host(out, H2).permute(0, 3, 1, 2), ref(torch.float64), ref(torch.float32))
    assert not _flag(reset=True)


@pytest.mark.parametrize("e", SCALE_EXP)
@pytest.mark.parametrize("which", ["se", "gnorm", "lnorm", "act", "linattn", "mhattn"])
def test_per_pixel_ops_away_from_unit_scale(which, e):
    """SE, both norms, the stand-alone SiLU and both attentions with the activations scaled by 2^e.  The attentions scale
    the VALUE operand: the logits are products of activations, and at 2^12 a soft-max over logits of 1e8 is decided by the
    last bit of an fp32 dot product in any implementation, the reference's fp32 self included."""
    s = 2.0 ** e
    n, h, w = 3, 8, 6
    name = "%s 2^%d" % (which, e)
    _flag(reset=True)
    if which == "se":
        cs, real = 32, 26
        g = torch.Generator().manual_seed(3)
        x = torch.zeros(n, cs, h, w)
        x[:, :real] = (torch.randn(n, real, h, w, generator=g) + 0.5 * torch.randn(1, real, 1, 1, generator=g)) * s
        x = _q(x)
        w1 = torch.randn(real // 4, real, generator=g) * (2.0 / np.sqrt(real)) / s          # the squeeze sees unit-scale means
        b1 = torch.randn(real // 4, generator=g) * 0.3
        w2 = torch.randn(real, real // 4, generator=g) * (6.0 / np.sqrt(real // 4))
        got = _se_run(x, w1, b1, w2, cs, real, h, w, n)[:, :real]
        _parity_gate(name, got, _se_ref(x, w1, b1, w2, torch.float64)[0], _se_ref(x, w1, b1, w2, torch.float32)[0])
    elif which in ("gnorm", "lnorm"):
        c, r = (GN_CR[2] if which == "gnorm" else LN_CR[2])
        data, mk, ref = (_gn_data, _gn_op, _gn_ref) if which == "gnorm" else (_ln_data, _ln_op, _ln_ref)
        x, gam, bet, block, g = data(c, r, h, w, n, H2)
        x = _q(x * s)
        out = _nan(H2, n, h, w, c)
        assert _call(mk(c, r, h, w), H2, n, _dev(x.permute(0, 2, 3, 1), H2), block, None, out) == 0, _lib.lib().udp_last_error()
        _parity_gate(name, _host(out, H2).permute(0, 3, 1, 2)[:, :r], ref(x, gam, bet, torch.float64), ref(x, gam, bet, torch.float32))
    elif which == "act":
        g = torch.Generator().manual_seed(4)
        x = _q(torch.randn(n, 32, h, w, generator=g) * 3.0 * s)
        f = lambda t: t * (1 / (1 + torch.exp(-t)))
        got = _host(_act_call(x, 32, h, w, n, SILU), H2).permute(0, 3, 1, 2)
        assert float(x.abs().max()) < 6e4
        e_hip, e_cpu, _ = mp.parity(name, got, f(x.double()), f(x), mp.ULP[H2])
        assert e_hip <= e_cpu + 4 * mp.ULP[H2]
    elif which == "linattn":
        c, r = LA_C[0]
        q, k, v, _, g = _la_data(c, r, h, w, n, H2, 1.0)
        v = _q(v * s)
        stored = torch.zeros(n, h, w, 2 * c + 32)
        stored[..., :c], stored[..., c:2 * c], stored[..., 2 * c] = k.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), q[:, 0]
        out = _nan(H2, n, h, w, c)
        assert _call(_la_op(c, h, w), H2, n, _dev(stored, H2), None, None, out) == 0, _lib.lib().udp_last_error()
        ref = lambda dt: linear_attention_core(q.to(dt), k[:, :r].to(dt), v[:, :r].to(dt))
        _parity_gate(name, _host(out, H2).permute(0, 3, 1, 2)[:, :r], ref(torch.float64), ref(torch.float32))
    else:
        dp, d, heads = MH_D[0]
        q, k, v, _, g = _mh_data(dp, d, h, w, n, H2, 1.0)
        v = _q(v * s)
        st = torch.zeros(n, h, w, 3 * dp)
        for j, t in enumerate((q, k, v)):
            st[..., j * dp:j * dp + d] = t.permute(0, 2, 3, 1)
        out = _nan(H2, n, h, w, dp)
        assert _call(_mh_op(dp, d, heads, h, w), H2, n, _dev(st, H2), None, None, out) == 0, _lib.lib().udp_last_error()
        assert float(v.abs().max()) < 6e4
        _mh_check(name, q, k, v, _host(out, H2).permute(0, 3, 1, 2), d, heads, H2)
    assert not _flag(reset=True), name


@pytest.mark.parametrize("e", SCALE_EXP)
def test_psa_away_from_unit_scale(e):
    s = 2.0 ** e
    c, h, w, n = 16, 8, 6, 3
    x, theta, P = mp.psa_inputs(c, h, w, n)
    P = dict(P, wq=P["wq"] / s)                                   # the pooling logits stay at unit scale (see the attentions)
    _flag(reset=True)
    xq, thq, mask, x1, x2 = _psa_run(x * s, theta, P, c, h, w, n)
    _parity_gate("psa scale 2^%d" % e, x1, mp.psa_scale(xq.double(), mask.double()), mp.psa_scale(xq, mask))
    _parity_gate("psa sp 2^%d" % e, x2, mp.psa_sp(thq.double(), x1.double(), mask.double()), mp.psa_sp(thq, x1, mask))
    assert not _flag(reset=True)


@pytest.mark.parametrize("e", SCALE_EXP)
@pytest.mark.parametrize("variant", sorted(STEMS))
def test_stem_away_from_unit_scale(variant, e):
    """The image and the stem's bias scaled by 2^e (64 x 96, n = 3, with the flip-test half)."""
    ks, env = STEMS[variant]
    s = 2.0 ** e
    m = Micro(H2, 3, 64, 96, flip=True, stem_ks=ks, seed=ks)
    m.x = m.x * s
    m.stem_b = m.stem_b * s
    m._blob[1] = (m._blob[1][0], m.stem_b.numpy().tobytes())
    _flag(reset=True)
    with _env(**env):
        assert m.run() == 0, m.error
    xx = torch.cat([m.x, torch.flip(m.x, [3])])
    ref = lambda d: mp.ref_conv(xx.to(d), m.stem_w, m.stem_b, stride=2, relu=True)
    _parity_gate("stem %s 2^%d" % (variant, e), m.read(m.stem_buf), ref(torch.float64), ref(torch.float32))
    assert not _flag(reset=True)
    m.assert_untouched()
    m.check_head()


@pytest.mark.parametrize("fmt,kmax", [("ws", 12), ("plain", 6)])
def test_weight_range_per_output_channel(fmt, kmax):
    """Output channel c of a 3x3 conv 64 -> 64 (9 x 7, n = 3, no activation) has its weights and bias scaled by 2^-(c mod
    (kmax + 1)): 0..12 for the fragment-major weights, whose block exponent keeps 22 bits down to 2^-16 of the largest
    weight (f16x2.pack_weights_ws), 0..6 for the plain format, which keeps hi a normal fp16 for He-scaled weights.  Every
    channel meets the conv gate against ITS OWN maximum.

    Measured on an MI355X, worst channel error / its own |ref|max per k (gate 2e-5), k = 0 upward:
      fragment-major 4.78e-7 4.73e-7 4.99e-7 4.60e-7 6.64e-7 4.34e-7 4.67e-7 6.41e-7 3.72e-7 5.50e-7 4.07e-7 4.27e-7 5.69e-7
      plain          3.37e-7 3.69e-7 2.61e-7 3.21e-7 4.13e-7 4.57e-7 2.76e-7"""
    d = _plant_conv("clean", False, 3, 1, 64, 64, 64, 9, 7, 3, False, 0, 0, 21)
    k = torch.arange(64) % (kmax + 1)
    sc = torch.ldexp(torch.ones(64), -k)
    d["wt"], d["bias"] = _q(d["wt"] * sc[:, None, None, None]), d["bias"] * sc
    _flag(reset=True)
    got = _conv_call(d, 3, 1, 64, 64, 9, 7, 3, fmt == "ws", 0)
    ref = mp.ref_conv(d["x"].double(), d["wt"], d["bias"])
    assert torch.isfinite(got).all()
    err = (got.double() - ref).abs().amax(dim=(0, 2, 3)) / ref.abs().amax(dim=(0, 2, 3))
    for kk in range(kmax + 1):
        print("weights %-5s 2^-%-2d  worst channel err / its max %.3g (gate %.3g)" % (fmt, kk, float(err[k == kk].max()), CONV_REL))
    assert float(err.max()) <= CONV_REL, err
    assert not _flag(reset=True)
