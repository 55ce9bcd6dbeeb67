/*
 * udp_pose_hip.h -- C ABI of the MI355X-native UDP-Pose hot path (gfx950).
 *
 * One shared library (libudp_pose_hip.so), extern "C", plain pointers and sizes,
 * no torch types.  Every pointer is a DEVICE pointer unless the name ends in
 * `_host`.  Every entry point returns UDP_OK (0) or a negative error code and
 * never throws; udp_last_error() gives the message for the calling thread.
 * The caller owns all buffers; nothing is allocated after udp_hrnet_create().
 * All work is enqueued on the hipStream_t the caller passes (`stream`, a
 * hipStream_t cast to void*; NULL = the default stream) and is asynchronous.
 * A handle is single-stream; distinct handles are independent (one per GPU).
 *
 * The reference (realphongha/UDP-Pose) has no FFI layer: its seam is Python
 * call contracts.  Each entry below names the reference function (file:line
 * under /root/reference) whose arithmetic it replaces; INTEGRATION.md shows
 * the ctypes binding a maintainer would add on the reference side.
 */
#ifndef UDP_POSE_HIP_H
#define UDP_POSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UDP_POSE_ABI_VERSION 20

enum udp_status {
  UDP_OK = 0,
  UDP_ERR_ARG = -1,          /* bad argument (null pointer, shape, enum) */
  UDP_ERR_HIP = -2,          /* a HIP runtime call failed */
  UDP_ERR_UNSUPPORTED = -3,  /* shape / config outside what the kernels cover */
  UDP_ERR_WORKSPACE = -4     /* workspace too small */
};

/* Storage type of activations + weights.
 *   UDP_F32   fp32, exact fp32 MFMA (v_mfma_f32_16x16x4_f32): the reference's arithmetic.
 *   UDP_BF16  bf16 storage, fp32 accumulate: reduced precision (does NOT meet the 1e-3 parity contract).
 *   UDP_F16X2 split fp16: a value is the pair (hi, lo) with x ~= hi + lo * 2^-11 (22 significant bits),
 *             4 bytes per element laid out per pixel as [C hi][C lo]; products run as three fp16 MFMAs
 *             with fp32 accumulation.  The parity-grade throughput mode (fp32-level results, fp16 matrix
 *             pipe).  |x| >= 65520 overflows to NaN (never silently). */
enum udp_dtype { UDP_F32 = 0, UDP_BF16 = 1, UDP_F16X2 = 2 };

/* ABI version of the loaded library (== UDP_POSE_ABI_VERSION it was built with). */
int udp_abi_version(void);
/* UDP_F16X2 range guard.  Split-fp16 storage has fp16's range: a value of magnitude >= 65520 (or a NaN) about to be
 * stored raises a device-side flag in the kernel that produced it -- at the source, because a NaN does not survive
 * the next ReLU and a finiteness test of the heat-maps can miss the event.  Waits for `stream`, then returns 1 if
 * any split-fp16 store since the last reset left the range, 0 if none, < 0 on error; reset != 0 clears the flag.
 * The stems raise it for a pixel of the fp32 input image outside that range (or NaN) too: they split the image in
 * registers, and what grows out of such a pixel is stored as 0 by their ReLU.  The flag is one per process, not per
 * handle or stream: clear it before the forward whose verdict is wanted.
 * The caller re-runs such a batch in UDP_F32 (udp_pose_amd.pose_engine does; the reference engine is fp32,
 * deep_hrnet/pose_engine.py:99-127). */
int udp_f16x2_overflow(void* stream, int reset);
/* Message of the last error on this thread ("" if none). */
const char* udp_last_error(void);

/* ------------------------------------------------------------------------- *
 * HRNet forward.  Replaces PoseHighResolutionNet.forward
 * (deep_hrnet/lib/models/pose_hrnet.py:436-471) incl. BasicBlock :29-59,
 * Bottleneck :62-100, HighResolutionModule.forward :260-273 with its fuse
 * layers :189-255 and the transitions :344-383; with flip_test != 0 also the
 * second forward on the W-mirrored batch of validate()
 * (deep_hrnet/lib/core/function.py:151-156).
 *
 * The network is handed over as a flat program of fused ops (one kernel launch
 * each) that the host builds from the reference's YAML + state_dict:
 * BatchNorm (eval) is folded into the conv weights/bias, so an op is
 *   out = act( conv(in) + bias [+ res] [+ sum_k nearest_up(up_k, 2^shift_k)] ).
 * Activations are NHWC in `dtype`; buffer b holds buf_elems[b] elements per
 * image and lives in the caller's workspace.
 * ------------------------------------------------------------------------- */
enum udp_op_kind {
  UDP_OP_STEM = 0, /* 3x3 s2 conv, Cin=3, reads the NCHW fp32 network input    */
  UDP_OP_CONV = 1, /* implicit-GEMM conv on MFMA, ks 1|3, stride 1|2; ks 7: stride 1 (below) */
  /* UDP_OP_CONV with ks = 7 (csrc/conv7.hip; the 7x7 stride-1 64 -> 64 conv of the stem of RSN-18 "se + prm"): stride 1,
   * pad 3, NHWC in and out, UDP_F32 (v_mfma_f32_16x16x4_f32) and UDP_F16X2 (the three-MFMA split-fp16 product, fp32
   * accumulation) -- UDP_BF16 is UDP_ERR_UNSUPPORTED.  Weights wfmt 0, [49 taps][cout_pad][cin] (tap = 7 ky + kx), bias
   * folded, relu 0 | 1.  cin and cout multiples of 16; in_coff / in_pitch / out_coff / out_pitch are honoured under the
   * 16-byte rule of every UDP_OP_CONV.  Pixels outside the image contribute exact zeros; a pixel's sum runs in one fixed
   * order (K chunk, ky, kx) whatever tile or image group it falls into, so results do not depend on the batch.  Refused
   * with UDP_ERR_UNSUPPORTED, never ignored: res, n_up, n_out2, the NCHW output (out_buf = UDP_BUF_OUTPUT), in_stuff2,
   * an output placed for a sub-batch lane (out_skip), UDP_ACT_HSWISH / UDP_ACT_SILU, chain_cout, group, wfmt 1, stride 2. */
  UDP_OP_FUSE = 2, /* no conv: out = act(in [+ res] + sum_k nearest_up(up_k))  */
  UDP_OP_STEM7 = 3,   /* 7x7 s2 p3 conv, Cin=3, reads the NCHW fp32 network input (RSN top) */
  UDP_OP_MAXPOOL = 4, /* MaxPool2d(3, stride 2, pad 1) */
  UDP_OP_BILINEAR = 5, /* bilinear resize, align_corners=True, hin x win -> hout x wout */
  /* Polarized self-attention PSA_s (deep_hrnet/lib/models/PSA.py:190-269) of pose_hrnet_psa and pose_resnet_psa, per
   * image.  C divides 256 and is a multiple of 16, or C = 512 (layer 4 of ResNet-18 / 34: a separate set of kernels with
   * the wave's lanes along the channels / along the weight rows); any other C is UDP_ERR_UNSUPPORTED at the first
   * forward.  Accepting 512 added no symbol and no field: UDP_POSE_ABI_VERSION stays as it is.
   * w_off = fp32 block wq[C] | Wv[C/2][C] | W1[C/8][C/2] | b1 | ln_g | ln_b | W2[C][C/8] | b2[C] | Wg[C/2][C] */
  UDP_OP_PSA_POOL = 6,  /* in = x [C];   out = fp32 {sum_p softmax(wq.x)_p x_p, mean_p x_p}  (2C floats) */
  UDP_OP_PSA_MLP = 7,   /* in = POOL out; out = fp32 {channel mask m[C], gbar[C/2]}            (3C/2 floats) */
  UDP_OP_PSA_SCALE = 8, /* in = x, res = MLP out; out = x * m[c] */
  UDP_OP_BLOCK = 10,    /* fused BasicBlock, bf16, 32 channels: out = relu(conv3x3(relu(conv3x3(in)+b)) + b2 + in);
                           w_off/b_off = first conv, w2_off/b2_off = second conv (pose_hrnet.py:43-59) */
  UDP_OP_PSA_SP = 9,    /* in = theta [C/2] (1x1 conv of the scaled map), res = scaled map [C], up_buf[0] = MLP out;
                           out = res * sigmoid(sum_j gbar_j softmax_HW(theta_j)) */
  /* ConvTranspose2d(k=4, stride=2, pad=1) + folded BatchNorm (+ ReLU): the deconv head of pose_resnet
   * (deep_hrnet/lib/models/pose_resnet.py:155-193).  ks = 4, stride = 2, hin x win -> hout = 2 hin x wout = 2 win,
   * UDP_F32 (cin % 16 == 0) and UDP_F16X2 (cin % 32 == 0), cout % 8 == 0, no addends.  Output row 2m+a (a in {0,1})
   * takes input rows m-1+a+t with ky = 3-a-2t (t in {0,1}), columns alike: phase (a,b) is a 2x2 conv over the 3x3
   * input window around (m,n), 4*cin*cout MACs per output pixel.  Weights: 16 "taps" pt = 4*(2a+b) + (2t+u) holding
   * w[ci][co][3-a-2t][3-b-2u] (PyTorch's [cin][cout][kh][kw] with the BatchNorm scale folded along dim 1, the deconv
   * bias folded into `bias`), laid out as a 16-tap conv: wfmt 0 (UDP_F32) fp32 [pt][cout_pad][cin]; wfmt 1
   * (UDP_F16X2, required there) the fragment-major blocks described at `wfmt` with tap = pt, scaled by 2^wexp
   * (udp_pose_amd.f16x2.pack_deconv_weights_ws builds it). */
  UDP_OP_DECONV = 11,
  /* Depthwise Conv2d(C, C, ks, stride, ks / 2, groups=C, bias=False) + folded BatchNorm (+ ReLU if `relu` == 1, SiLU
   * if `relu` == 4 -- MobileViTv2, backbones/mobilevitv2.py:210-214, :898-908; activation code 2 is refused with
   * UDP_ERR_UNSUPPORTED): the dw convs of the ShuffleV2 units (deep_hrnet/lib/models/backbones/
   * shufflenetv2.py:54-55, :66-67; the reference never puts a ReLU behind one, the field is honoured all the same) and
   * the 5x5 / 7x7 ones of ShuffleNetV2+ (backbones/shufflenetv2_plus.py:97, :119).  Per image, NHWC, UDP_F32 and
   * UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED).  ks = 3 | 5 | 7 (anything else: UDP_ERR_ARG), stride 1 | 2,
   * cin == cout == cout_pad = C, a multiple of 32; any hin, win >= 1;
   * hout = (hin - 1) / stride + 1, wout alike (integer division).  in_coff / in_pitch / out_coff / out_pitch are
   * honoured (multiples of 8).  No addends, no group, wfmt 0.
   * Weights: fp32 [ks * ks][C], tap-major (tap = ks * ky + kx), the BatchNorm scale folded in (in fp64 on the host),
   * in EVERY storage mode; bias fp32 [C].
   * Arithmetic per output element, fp32: acc = bias; then for ky = 0..ks-1, kx = 0..ks-1 in that order
   * acc = fmaf(x[stride*oy + ky - ks/2][stride*ox + kx - ks/2], w[ks ky + kx], acc), where a tap outside the image is
   * skipped (not read, not multiplied by zero).  UDP_F16X2 inputs are decoded hi + lo * 2^-11 first and the result is
   * split again on store, with the udp_f16x2_overflow range guard.  A memory-bound VALU kernel: no MFMA.
   *
   * Shuffle passthrough (n_out2 = 1, stride 1 only).  A stride-1 ShuffleV2 unit (shufflenetv2.py:77-92) keeps the
   * even logical channels of its input as x_proj and runs branch_main on the odd ones; its output is
   * cat(x_proj, branch_main).  Unit tensors hold 2r logical channels as two halves of C stored channels each, the r
   * real ones first and C - r zeros behind them: logical channel j lives at j (j < r) or C + j - r.  The dw launch of
   * the unit copies x_proj while it is at it:
   *   source       `res`:  res_buf, res_coff, res_pitch (>= res_coff + 2C) -- the unit's input, same h x w as the output
   *   destination  out2_buf[0], out2_coff[0], out2_pitch[0] (>= out2_coff[0] + C) -- the first half of the unit's output
   *   chain_cout = r, the real channels per half (even, 2 <= r <= C)
   *   dst[k] = src[2k < r ? 2k : C + 2k - r] for k < r, and 0 for r <= k < C.
   * It is a selection of stored bit patterns (both planes in UDP_F16X2), never decoded: bit for bit.  add2_* are not
   * read.  udp_conv2d_fused: the source is `res`, the destination (written) is `up0`.  Without a passthrough
   * (n_out2 = 0) res_buf must be UDP_BUF_NONE and chain_cout 0. */
  UDP_OP_DWCONV = 12,
  /* nn.PixelShuffle(2) on NHWC (deep_hrnet/lib/models/decoders/DUC.py:21,27), UDP_F32 and UDP_F16X2.  cin = 4 cout,
   * cout % 8 == 0, hout = 2 hin, wout = 2 win; views honoured.  PyTorch takes out[c][2h+i][2w+j] from input channel
   * 4c + 2i + j; here the PRODUCER (the DUC conv, through its output-channel permutation) stores that channel at
   * (2i + j) * cout + c, so the four sub-pixel groups are contiguous per pixel and the op copies channels
   * [g * cout, (g + 1) * cout) of pixel (h, w), g = 2i + j, to pixel (2h + i, 2w + j).  Pure data movement of the
   * stored bit patterns: bit for bit, no weights / bias (may be NULL), no ReLU. */
  UDP_OP_PIXSHUF = 13,
  /* Squeeze-and-excitation (SELayer, deep_hrnet/lib/models/backbones/shufflenetv2_plus.py:34-60) on an NHWC view of
   * C stored channels, UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED); one launch, one workgroup per image:
   *   mean[c] = (1 / HW) sum_p in[p][c]          h = relu(W1 mean + b1)   (BatchNorm folded into W1 / b1)
   *   m[c] = clamp((W2 h)[c] + 3, 0, 6) / 6      out[p][c] = in[p][c] * m[c]
   * cin == cout == cout_pad = C, a multiple of 32 up to 512; hout == hin, wout == win (any size >= 1);
   * chain_cout = the hidden width Ch (rows of W1), 1 <= Ch <= min(256, C) -- the way it carries r for the passthrough
   * of UDP_OP_DWCONV; no chained conv.  in_coff / in_pitch / out_coff / out_pitch are honoured (multiples of 8, as
   * for kinds 12 and 13).  `out` MAY be `in` (same buffer, same view): the pool is complete before the first store
   * and every element is read and written by one thread; any other overlap of the two is refused.  relu must be 0;
   * no addends, second outputs, group, wfmt.  Parameter block at w_off (udp_conv2d_fused: `weights`; `bias` may be
   * NULL), fp32 in EVERY storage mode: W1 transposed [C][Ch], b1 [Ch], W2 transposed [Ch][C].  Pad channels carry
   * zero weights: m = 0.5 there and the stored zeros stay exact zeros.  All sums are fp32 in a fixed order that
   * depends on (C, Ch, HW) only, nothing is atomic: an image's result does not depend on the batch it arrives in. */
  UDP_OP_SE = 14,
  /* nn.GroupNorm(1, C), eps 1e-5 -- what the reference calls "layer_norm_2d" (deep_hrnet/lib/models/backbones/
   * mobilevitv2.py:139-140; the norms of LinearAttnFFN :783-794 and the closing one of MobileViTBlockv2 :1018-1022) --
   * on an NHWC view of C stored channels, UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED); one launch, one
   * workgroup per image.  The reference applies it to the unfolded [B, C, P, N] tensor; the statistics run over the
   * whole sample, so on the NHWC map it is the same op (unfold / fold only re-index pixels).
   *   mean = (1 / (r HW)) sum in[p][c]     var = (1 / (r HW)) sum (in[p][c] - mean)^2     (over the r real channels)
   *   out[p][c] = fmaf((in[p][c] - mean) * rstd, gamma[c], beta[c]),  rstd = 1 / sqrt(var + 1e-5)      for c < r
   *     (mean and the subtraction in fp64, the difference and rstd rounded to fp32, the rest in fp32)
   *   out[p][c] = 0                                                                                     for r <= c < C
   * cin == cout == cout_pad = C, a multiple of 32 up to 512; chain_cout = r, the real channels (1 <= r <= C; the first
   * r of the view) -- the field carries a count here as it does for kinds 12 and 14, no chained conv; hout == hin,
   * wout == win, any size >= 1.  in_coff / in_pitch / out_coff / out_pitch are honoured (multiples of 8).  relu must
   * be 0; no addends, second outputs, group, wfmt.  `out` MAY be `in` (same buffer, same view -- the rule of kind 14):
   * both statistics are complete before the first store and every element is read and written by one thread.
   * Parameter block at w_off (udp_conv2d_fused: `weights`; `bias` may be NULL), fp32 in EVERY storage mode: gamma [C],
   * beta [C], zeros at the pad channels.  The variance is two-pass (the mean first, then the squared deviations of a
   * second read of the map): never E[x^2] - E[x]^2.  A thread accumulates in fp64 over its pixels in ascending order
   * and the workgroup adds the per-thread sums in a fixed tree; the order depends on (C, r, HW) only, nothing is
   * atomic: an image's result does not depend on the batch it arrives in.  Not counted in udp_hrnet_flops_per_image. */
  UDP_OP_GNORM = 15,
  /* The core of the separable ("linear") self-attention of MobileViTv2 for 2x2 patches: LinearSelfAttention.
   * _forward_self_attn between qkv_proj and out_proj (backbones/mobilevitv2.py:671-689), with the F.unfold / F.fold
   * around it (:1026-1055) folded into indexing: pixel (y, x) of the NHWC map is position p = 2 (y & 1) + (x & 1) of
   * patch (y / 2, x / 2), and the soft-max over the patches runs separately for each of the four positions.
   * UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED); one launch, one workgroup per image.  ks = 2 carries the
   * patch size (anything else: UDP_ERR_ARG).  cout == cout_pad = C, a multiple of 32 up to 512; cin = 2C + 32: the
   * output of the qkv conv as the planner stores it (through the conv's output-channel map) -- key at [0, C), value at
   * [C, 2C), the query's single channel at 2C, zeros behind it.  hin == hout, win == wout, both even and hin * win <=
   * 16384 (odd sizes: UDP_ERR_ARG; the reference resizes such maps bilinearly, :1095-1103).  Views are honoured
   * (multiples of 8); `out` must not be `in`.  relu must be 0; no weights / bias (may be NULL), addends, second
   * outputs, group, wfmt.  Per image and position class p:
   *   m = max q over the class's pixels        s = exp(q - m) / sum exp(q - m)
   *   ctx[p][c] = sum s k[.][c]                out[y][x][c] = max(v[y][x][c], 0) * ctx[p(y, x)][c]
   * All fp32; UDP_F16X2 operands are decoded hi + lo * 2^-11 first and the result is split again on store, with the
   * udp_f16x2_overflow range guard.  q is staged in LDS, so the map is read once (k, then v).  The class maximum and
   * sum are reduced by one wave per class in a fixed butterfly; ctx is accumulated with fmaf by G pixel groups per
   * class (class pixels g, g + G, ... in raster order) that are then added in the order g = 0 .. G-1; G depends on C
   * only, nothing is atomic: an image's result does not depend on the batch it arrives in.  Pad channels have
   * k = v = 0 and stay exact zeros.  udp_hrnet_flops_per_image counts 2 C HW (the weighted sum) for it. */
  UDP_OP_LINATTN = 16,
  /* nn.LayerNorm(d), eps 1e-5, per token -- the norms of MobileViT's pre-norm TransformerEncoder and the one that closes
   * a MobileViTBlock's global_rep (deep_hrnet/lib/models/backbones/mobilevit.py:112-113, :480-488, :566-568).  The
   * reference applies it to the unfolded [B P, N, d] tensor (:593-632); a token is a pixel, so on the NHWC map it
   * is a reduction over one pixel's contiguous channels and the map is never rearranged.  UDP_F32 and UDP_F16X2
   * (UDP_BF16: UDP_ERR_UNSUPPORTED).  cin == cout == cout_pad = C, a multiple of 32 up to 512; chain_cout = r, the real
   * channels (1 <= r <= C; the first r of the view) -- the field carries a count as it does for kind 15, no chained
   * conv; hout == hin, wout == win, any size >= 1.  in_coff / in_pitch / out_coff / out_pitch are honoured (multiples
   * of 8).  relu must be 0; no addends, second outputs, group, wfmt.  `out` MAY be `in` (same buffer, same view): a
   * pixel's row sits in registers before its first store and every element is read and written by one thread.
   * Parameter block at w_off (udp_conv2d_fused: `weights`; `bias` may be NULL), fp32 in EVERY storage mode: gamma [C],
   * beta [C], zeros at the pad channels.  Per pixel:
   *   mean = (1 / r) sum_c in[c]     var = (1 / r) sum_c (in[c] - mean)^2     (two-pass, never E[x^2] - E[x]^2)
   *   out[c] = fmaf((in[c] - mean) * rstd, gamma[c], beta[c]),  rstd = 1 / sqrt(var + 1e-5)      for c < r
   *     (mean and the subtraction in fp64, the difference and rstd rounded to fp32, the rest in fp32)
   *   out[c] = 0                                                                                 for r <= c < C
   * 16 lanes share a pixel: lane l adds the real channels of its 16-byte groups l, l + 16, ... in ascending order in
   * fp64, then a butterfly over the 16 lanes.  The order depends on (C, r) only, nothing is atomic: an image's result
   * does not depend on the batch it arrives in.  Not counted in udp_hrnet_flops_per_image. */
  UDP_OP_LNORM = 17,
  /* Soft-max multi-head self-attention for 2x2 patches: MultiHeadAttention.forward_other between qkv_proj and out_proj
   * (backbones/mobilevit.py:436-457), with MobileViTBlock.unfolding / folding (:593-655) folded into indexing: pixel
   * (y, x) of the NHWC map is position p = 2 (y & 1) + (x & 1) of patch (y / 2, x / 2), and the reference's [B P, N, d]
   * token tensor means that attention mixes only the N = HW / 4 pixels of one position class of one image, in patch
   * raster order.  UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED).  ks = 2 carries the patch size (anything
   * else: UDP_ERR_ARG).  cout == cout_pad = dp, a multiple of 32 up to 256; cin = 3 dp: the output of the qkv conv as
   * the planner stores it (through the conv's output-channel map) -- q real channels at [0, d), k at [dp, dp + d), v at
   * [2 dp, 2 dp + d), zeros in the pads.  chain_cout = d, the real width (1 <= d <= dp; a count, no chained conv).
   * up_shift[0] = the head count (with n_up == 0 the field is free for this kind): d % heads == 0 and head width
   * hd = d / heads <= 64, else UDP_ERR_ARG.  Head h owns the REAL channels [h hd, (h + 1) hd) of q, k and v: padding
   * never moves a head boundary.  hin == hout, win == wout, both even (odd sizes: UDP_ERR_ARG; the reference resizes such
   * maps bilinearly, :598-605).  Views are honoured (multiples of 8); `out` must not be `in`.  relu must be 0; no
   * weights / bias (may be NULL), addends, second outputs, group, wfmt.  The hd^-0.5 scaling of q (:441) is NOT applied:
   * the planner folds it into the q rows of qkv_proj's weight and bias (in fp64, before packing).  Per image, class p,
   * head h, over the class's N pixels:
   *   s_ij = q_i . k_j        m_i = max_j s_ij        out_i = sum_j exp(s_ij - m_i) v_j / sum_j exp(s_ij - m_i)
   * All fp32; UDP_F16X2 operands are decoded hi + lo * 2^-11 first and the result is split again on store, with the
   * udp_f16x2_overflow range guard.  One thread per query row; the keys are walked in blocks of 32 staged in LDS (any N
   * runs on the one code path), 8 keys per soft-max update: s_ij by fmaf over the head's channels in ascending order
   * from 0; m' = max(m, max of the 8); l and the accumulator are multiplied by exp(m - m'); then for j ascending
   * e = exp(s_ij - m'), l += e, acc = fmaf(e, v_j, acc); out = acc / l.  Keys past N are skipped.  For N <= 64 / 128 a
   * workgroup runs 4 / 2 (class, head) pairs, a whole number of waves each.  The order depends on (N, hd) only, nothing
   * is atomic: an image's result does not depend on the batch it arrives in.  Pad channels of the output are written
   * as exact zeros.  udp_hrnet_flops_per_image counts 2 d N MACs per pixel (q k^T and the weighted sum). */
  UDP_OP_MHATTN = 18,
  /* out = act(in) element-wise, act = `relu` = UDP_ACT_SILU or UDP_ACT_HSWISH (0 and 1: UDP_ERR_ARG, as every code
   * outside 0..4 and code 3; a ReLU rides in its producer's epilogue).  The two full 3x3 convs of a MobileViTBlock
   * (backbones/mobilevit.py:531-534, :546-549) are followed by SiLU, and the 3x3 conv kernels have no SiLU epilogue:
   * they run with code 0 and one of these follows.  UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED).
   * cin == cout == cout_pad = C, a multiple of 32; hout == hin, wout == win, any size >= 1; views honoured (multiples
   * of 8); `out` MAY be `in` (same buffer, same view): every element is read and written by one thread.  No weights /
   * bias (may be NULL), addends, second outputs, chain, group, wfmt.  The arithmetic is that of the activation codes
   * below, fp32; act(0) = 0, so zero pad channels stay exact zeros.  Not counted in udp_hrnet_flops_per_image. */
  UDP_OP_ACT = 19,
  /* Kinds 20 - 22: the gates of RSN-18 "se + prm" (RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py).  All three:
   * UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED); inputs decoded hi + lo * 2^-11, results split again on store
   * with the udp_f16x2_overflow range guard; parameters fp32 in EVERY storage mode; per image, nothing atomic, every
   * sum in an order that depends on the shape only: an image's result does not depend on the batch it arrives in, on
   * the lane or on graph replay.  sigmoid(v) = 1 / (1 + expf(-v)) in fp32.  They add kinds and no field or symbol:
   * UDP_POSE_ABI_VERSION stays as it is.
   *
   * Squeeze-and-excitation with the block's shortcut (SELayer, reduction 8, no biases, no BatchNorm: network.py:51-66;
   * `out = se(out); out += x; relu`, :137-143) on an NHWC view of C stored channels; one launch, one workgroup per image:
   *   mean[c] = (1 / HW) sum_p in[p][c]      h = relu(W1 mean)      m = sigmoid(W2 h)
   *   out[p][c] = act(fmaf(in[p][c], m[c], res[p][c]))         (res_buf == UDP_BUF_NONE: in[p][c] * m[c])
   * cin == cout == cout_pad = C, a multiple of 32 up to 512; hout == hin, wout == win (any size >= 1); chain_cout = the
   * hidden width Ch (rows of W1), 1 <= Ch <= 256 -- a count, as for kind 14, no chained conv.  relu = UDP_ACT_NONE or
   * UDP_ACT_RELU (codes 2 and 4: UDP_ERR_UNSUPPORTED).  in / out / res views are honoured (multiples of 8).  `out` MAY
   * be `in` (same buffer, same view -- the rule of kind 14): the pool is complete before the first store and every
   * element is read and written by one thread; any other overlap of the two, and `res` in the buffer of `in` or `out`,
   * is refused.  No up-sampled addends, second outputs, group, wfmt.  Parameter block at w_off (udp_conv2d_fused:
   * `weights`; `bias` may be NULL): W1 transposed [C][Ch], W2 transposed [Ch][C]; zero weights at pad channels give
   * m = 0.5 there, and act(0 * 0.5 + 0) = 0 keeps them exact zeros.  Sums as kind 14: the pool by P pixel groups per
   * channel added in group order, W1 mean by Q channel parts (fmaf from 0 in channel order) added in part order, W2 h by
   * fmaf from 0 in the order j = 0 .. Ch-1; P, Q depend on (C, Ch) only.  udp_hrnet_flops_per_image counts 4 C Ch. */
  UDP_OP_SE_RES = 20,
  /* Channel gate of the Pose Refine Machine (PRM.forward, network.py:293-296): in = out_1 on an NHWC view of C stored
   * channels; out = ONE fp32 row a[C] per image in a side buffer of C floats (counted in `dtype` elements, the way
   * UDP_OP_PSA_MLP leaves its vector); one launch, one workgroup per image:
   *   a = sigmoid(relu(W2 relu(W1 mean_p in + b1) + b2))
   * -- the ReLU in front of the sigmoid is the reference's (conv_bn_relu(..., has_relu=True), :278-281).  The conv biases
   * and BatchNorms of prm_2_1 / prm_2_2 are folded into W / b on the host (in fp64).  cin == cout == cout_pad = C, a
   * multiple of 32 up to 256 (the hidden layer is C wide); hin x win = the map, hout == hin, wout == win; the input view
   * is honoured, the output takes none; chain_cout 0, relu 0, no res / addends / second outputs / group / wfmt; `out`
   * must not be `in`.  Parameter block at w_off (udp_conv2d_fused: `weights`; `bias` may be NULL): W1 transposed [C][C],
   * b1 [C], W2 transposed [C][C], b2 [C].  Sums as kind 20, onto b1 / from b2.  Counts 4 C C in udp_hrnet_flops_per_image. */
  UDP_OP_PRM_GATE = 21,
  /* Spatial gate of the Pose Refine Machine and the combine (network.py:297-300): a depthwise Conv2d(C, C, 9, 1, 4,
   * groups=C) with bias + folded BatchNorm + ReLU + sigmoid, then out_1 * (1 + channel gate * spatial gate):
   *   in = t (the output of the 1x1 prm_3_1), res = out_1, n_up = 1 with up_buf[0] = the fp32 rows of kind 21 and
   *   up_shift[0] = 0 (udp_conv2d_fused: `res`, `up0`)
   *   out[p][c] = res[p][c] * fmaf(a[c], sigmoid(max(dw9(t)[p][c], 0)), 1)
   * dw9 has the arithmetic contract of kind 12: acc = bias, then one fmaf per tap in the order ky = 0..8, kx = 0..8,
   * a tap outside the image skipped (not read, not multiplied by zero) -- so the result does not depend on the tiling.
   * Weights fp32 [81][C], tap-major (tap = 9 ky + kx), the BatchNorm scale folded in; bias fp32 [C] (conv bias and
   * BatchNorm folded).  ks = 9, stride = 1 (anything else: UDP_ERR_ARG); cin == cout == cout_pad = C, a multiple of 32;
   * hout == hin, wout == win, any size >= 1 (maps smaller than the window included).  in / out / res views are
   * honoured (multiples of 8).  `out` must not be `in` or `res`.  relu 0; no second outputs, chain, group, wfmt.  An
   * LDS-tiled VALU kernel (csrc/rsn_gate.hip): the 16 x 24 pixel input tile of an 8 x 16 output tile is staged once.
   * udp_hrnet_flops_per_image counts the 81 MACs per output element. */
  UDP_OP_PRM_DW9 = 22,
  /* Activation + squeeze-and-excitation with both biases: what follows `depthwise conv -> BatchNorm` in a MobileNetV3
   * InvertedResidual (torchvision's mobilenet_v3_small().features -- the backbone of pose_mobilenetv3_small and
   * pose_mobilenetv3_small_pixel_shuffle, deep_hrnet/lib/models/backbones/mobilenetv3.py:5-16): the block's activation,
   * then SqueezeExcitation = fc1 (with bias) + ReLU + fc2 (with bias) + Hardsigmoid.  On an NHWC view of C stored
   * channels, UDP_F32 and UDP_F16X2 (UDP_BF16: UDP_ERR_UNSUPPORTED); one launch, one workgroup per image:
   *   a[p][c] = act(in[p][c])                 act = `relu`: UDP_ACT_NONE | UDP_ACT_RELU | UDP_ACT_HSWISH
   *   mean[c] = (1 / HW) sum_p a[p][c]        h = relu(W1 mean + b1)                 (Ch = chain_cout rows)
   *   m[c] = clamp((W2 h)[c] + b2[c] + 3, 0, 6) / 6                                  (torch Hardsigmoid)
   *   out[p][c] = a[p][c] * m[c]
   * The activation is applied while the map is pooled and again while it is scaled, so the map is read twice and
   * written once -- where UDP_OP_DWCONV (no hard-swish epilogue) + UDP_OP_ACT + UDP_OP_SE would read and write it
   * twice and still lack b2.  cin == cout == cout_pad = C, a multiple of 32, 32 <= C <= 1024; chain_cout = Ch,
   * 1 <= Ch <= min(256, C) -- a count, as for kind 14, no chained conv; hout == hin, wout == win, any size >= 1.
   * Activation code 4 (SiLU): UDP_ERR_UNSUPPORTED; code 3 and codes outside 0..4: UDP_ERR_ARG.  in_coff / in_pitch /
   * out_coff / out_pitch are honoured (multiples of 8).  `out` MAY be `in` (same buffer, same view -- the rule of kind
   * 14): the pool is complete before the first store and every element is read and written by one thread; any other
   * overlap of the two is refused.  No res, addends, second outputs, group, wfmt.  Parameter block at w_off
   * (udp_conv2d_fused: `weights`; `bias` may be NULL), fp32 in EVERY storage mode: W1 transposed [C][Ch], b1 [Ch], W2
   * transposed [Ch][C], b2 [C]; udp_hrnet_create checks its (2 C Ch + Ch + C) * 4 bytes against the blob.  Pad
   * channels carry zero weights and zero b2: m = 0.5 there, and act(0) * 0.5 = 0 keeps them exact zeros.  All
   * arithmetic is fp32, hard-swish exactly the formula at UDP_ACT_HSWISH below; UDP_F16X2 inputs are decoded hi + lo *
   * 2^-11 and the result is split again on store, with the udp_f16x2_overflow range guard.  Sums as kind 14: the pool
   * by P = max(1, 256 / (C / V)) pixel groups per channel (V = 4 fp32 / 8 split-fp16 channels per thread) added in
   * group order, W1 mean by Q channel parts (fmaf from 0 in channel order) added in part order onto b1, W2 h by fmaf
   * from 0 in the order j = 0 .. Ch-1, then + b2 + 3; P, Q depend on (C, Ch) only, nothing is atomic: an image's
   * result does not depend on the batch it arrives in, on the lane or on graph replay.  The dynamic LDS is sized from
   * C.  It adds a kind and no field or symbol: UDP_POSE_ABI_VERSION stays as it is.  udp_hrnet_flops_per_image counts
   * 4 C Ch (the two small products), as for kind 14. */
  UDP_OP_SE_ACT = UDP_OP_PRM_DW9 + 1 /* kind 23 */
};

/* udp_conv_op.relu is an activation code.  UDP_ACT_HSWISH: v * (clamp(v + 3, 0, 6) / 6) in fp32, applied where the
 * ReLU is applied, before the value is stored -- in UDP_OP_STEM and in a 1x1 stride-1 UDP_OP_CONV writing NHWC
 * without addends (res / up), second outputs, a chain or a group, in UDP_F32 and UDP_F16X2 (wfmt 0 and 1, channel
 * views honoured).  Every other op and conv form answers it with UDP_ERR_UNSUPPORTED.
 * UDP_ACT_SILU ("swish", nn.SiLU: the activation of every ConvLayer of MobileViTv2, backbones/mobilevitv2.py:78-79):
 * v * (1 / (1 + expf(-v))) in fp32, in the same place -- honoured by the two forms above and by UDP_OP_DWCONV (every
 * ks / stride it has); every other op and conv form answers it with UDP_ERR_UNSUPPORTED.  silu(0) = 0, so zero pad
 * channels stay exact zeros.  Code 3 is not assigned and stays refused with UDP_ERR_ARG, as every code outside 0..4.
 * UDP_OP_SE_ACT reads the field as the activation of its INPUT (codes 0, 1 and 2; kind 23 above). */
#define UDP_ACT_NONE 0
#define UDP_ACT_RELU 1
#define UDP_ACT_HSWISH 2
#define UDP_ACT_SILU 4

#define UDP_MAX_LANES 4
#define UDP_MAX_WAIT 8
#define UDP_BUF_NONE (-1)
#define UDP_BUF_OUTPUT (-2) /* out_buf: the NCHW fp32 heat-map output of the net */

typedef struct udp_conv_op {
  int32_t kind;            /* enum udp_op_kind */
  int32_t ks, stride;      /* kernel size 1|3, UDP_OP_CONV also 7 at stride 1 (see UDP_OP_CONV) (UDP_OP_DWCONV: 3|5|7, UDP_OP_PRM_DW9: 9; pad = ks/2; UDP_OP_LINATTN / UDP_OP_MHATTN: 2 = the patch size), stride 1|2 */
  int32_t relu;            /* activation of the epilogue: UDP_ACT_NONE / UDP_ACT_RELU / UDP_ACT_HSWISH / UDP_ACT_SILU (see there) */
  int32_t cin, cout;       /* real channel counts (cin multiple of 16 for UDP_OP_CONV) */
  int32_t cout_pad;        /* cout rounded up to a multiple of 32: rows of `weights`/`bias` */
  int32_t hin, win, hout, wout;
  int32_t in_buf, out_buf, res_buf; /* activation buffer ids; UDP_BUF_NONE / UDP_BUF_OUTPUT */
  int32_t n_up;            /* 0..3 nearest-upsampled addends */
  int32_t up_buf[3];
  int32_t up_shift[3];     /* up_k has (hout>>shift) x (wout>>shift) pixels, cout channels */
  int64_t w_off;           /* byte offset in the weight blob: [ks*ks][cout_pad][cin] in dtype
                              (UDP_OP_STEM: fp32 [27][cout]) */
  int64_t b_off;           /* byte offset of the fp32 bias [cout_pad] */
  /* Channel-slice views (elements; 0 pitch = dense): the op reads channels [in_coff, in_coff+cin) of
   * a tensor stored with in_pitch channels per pixel, writes [out_coff, out_coff+cout) of a tensor with
   * out_pitch channels, likewise for res.  torch.split / torch.cat of the RSN bottleneck
   * (RSN/exps/RSN18.coco/network.py:102-114) become views, never copies. */
  int32_t in_coff, in_pitch, out_coff, out_pitch, res_coff, res_pitch;
  int32_t lane;            /* 0..UDP_MAX_LANES-1: ops of different lanes may run concurrently
                              (HRNet branches); lane 0 runs on the caller's stream */
  int32_t n_wait;          /* cross-lane dependencies: this op starts after ops wait_op[0..n_wait) */
  int32_t wait_op[UDP_MAX_WAIT];
  int64_t w2_off, b2_off;  /* UDP_OP_BLOCK / chain_cout: the second conv's weights / bias in the blob */
  int32_t group;           /* != 0: consecutive UDP_OP_CONV ops with the same group id are independent of each
                              other (same-depth convs of different HRNet branches) and may share one launch */
  int32_t wfmt;            /* weight layout of a UDP_OP_CONV.  0: [tap][cout_pad][cin] in dtype (UDP_F16X2: per row the
                              cin hi values, then the cin lo values).  1 (UDP_F16X2 only): fragment-major for the
                              weight-stationary kernel -- 1 KiB blocks [tap][cin chunk of 32][cout pair of 32]
                              [block nb of 16][plane hi|lo], a block = 64 lanes x 8 fp16: lane kg*16 + li holds
                              w[tap][32*pair + 8*(li>>2) + 4*nb + (li&3)][32*chunk + 8*kg .. +7] (cin zero-padded to
                              a multiple of 32).  UDP_OP_DECONV: the same over its 16 phase/tap pairs (see there).  The stored numbers are the weights times 2^wexp: plane hi =
                              fp16(w * 2^wexp), plane lo = fp16(w * 2^wexp - hi) (the plain residual, NOT scaled by 2^11
                              as activations are).  udp_pose_amd.f16x2.pack_weights_ws builds it. */
  int32_t wexp;            /* wfmt 1: power-of-two scale of the stored weights, chosen so that max |w| * 2^wexp lies in
                              [2^13, 2^14) (|wexp| <= 40; 0 for an all-zero tensor).  The kernel keeps one fp32
                              accumulator of conv * 2^wexp and multiplies by 2^-wexp in its epilogue. */
  int32_t in_stuff2;       /* udp_conv2d_fused / _group, fp32 and bf16 storage: 1 = the input tensor is [n][hin/2][win/2][cin] and is read
                              as its zero-stuffed image (pixel (2i, 2j) = tensor pixel (i, j), zeros elsewhere): the input gradient of
                              a stride-2 conv = this stride-1 conv over the stuffed output gradient, without materialising it
                              (udp_zero_stuff2 + 4x the bytes); hin, win even.  0 elsewhere. */
  /* Second outputs (udp_hrnet_* programs, UDP_F16X2 convs with wfmt 1 and an NHWC output): besides `out`, the epilogue
   * writes out2_k = out + add2_k for k < n_out2 (0..2) -- the value AS STORED in `out` (22-bit split) plus channels
   * [add2_coff, add2_coff + cout) of another tensor of the output's resolution -- into channels [out2_coff, +cout) of a
   * third one.  The RSN bottleneck's element-wise sums between its 3x3 convs (RSN/exps/RSN18.coco/network.py:102-114:
   * `out_2_1 = conv(spx[1] + out_1_1)` ...) ride in the epilogue of the conv that produces their second operand instead of
   * being launches of their own; the numbers are those of UDP_OP_FUSE on the stored tensors, bit for bit.  With
   * n_out2 > 0, out_buf may be UDP_BUF_NONE: only the sums are stored. */
  int32_t n_out2;
  int32_t out2_buf[2], out2_coff[2], out2_pitch[2];
  int32_t add2_buf[2], add2_coff[2], add2_pitch[2];
  /* Chained 1x1 conv (udp_hrnet_* programs; chain_cout == 0: none).  A UDP_F16X2 1x1 stride-1 UDP_OP_CONV with wfmt 1,
   * cin 64 | 128, cout 256, a dense-or-sliced NHWC `out`, no up-sampled addends and no second outputs feeds
   * its result -- the value AS STORED in `out` -- straight into a second 1x1 conv + bias (+ ReLU if chain_relu) of
   * chain_cout (= 64) output channels, written densely to chain_buf: the Bottleneck chain of pose_hrnet.py:80-100
   * (conv3 + bn3 + shortcut + ReLU of one block, conv1 + bn1 + ReLU of the next) in one launch, the 4 * planes-channel
   * map written once and not read back.  The second conv's weights are fragment-major ([cout / 32 chunks][chain_cout / 32
   * pairs], scaled by 2^chain_wexp) at w2_off, its fp32 bias [chain_cout] at b2_off.  Both results equal those of the
   * two separate convs bit for bit. */
  int32_t chain_cout, chain_buf, chain_relu, chain_wexp;
} udp_conv_op;

typedef struct udp_hrnet udp_hrnet; /* opaque */

/* weights_dev: device blob (caller-owned, must outlive the handle).  ops and
 * buf_elems are host arrays, copied.  in_h/in_w: network input size. */
int udp_hrnet_create(const udp_conv_op* ops_host, int n_ops, const int64_t* buf_elems_host,
                     int n_bufs, const void* weights_dev, size_t weights_bytes, int dtype,
                     int in_h, int in_w, int out_channels, udp_hrnet** out);
/* Bytes of workspace udp_hrnet_forward needs for `n` input images (flip_test doubles it; with two sub-batch lanes:
 * both lanes' buffers plus, under flip_test, their heat-maps before they are copied into place). */
size_t udp_hrnet_workspace_bytes(const udp_hrnet* h, int n, int flip_test);
/* Sub-batch lanes udp_hrnet_forward(use_graph != 0) runs a batch of `n` images in: 2 = the batch is cut in two halves,
 * each replayed as its own hipGraph, the second on an internal stream beside the first (fork / join on the caller's
 * stream; results are those of one lane, images are independent); 1 otherwise.  Two lanes: UDP_F16X2 / UDP_BF16, inputs
 * up to 256x192, n >= 16 (environment UDP_POSE_LANES=1 / 2 forces one / two). */
int udp_hrnet_lanes(const udp_hrnet* h, int n);
/* in_nchw: fp32 [n,3,in_h,in_w].  heatmaps_nchw: fp32 [n*(flip_test?2:1), C, in_h/4, in_w/4];
 * with flip_test rows n..2n-1 are the raw outputs for the mirrored inputs (fuse them with
 * udp_flip_fuse).  use_graph != 0 replays a cached hipGraph of the launch sequence. */
int udp_hrnet_forward(udp_hrnet* h, const float* in_nchw, int n, int flip_test, void* workspace,
                      size_t workspace_bytes, float* heatmaps_nchw, int use_graph, void* stream);
/* Same launches as udp_hrnet_forward (eager, no graph) with a hipEvent pair around every launch on
 * `stream`; waits for completion and writes the elapsed milliseconds of op i to ms_per_op_host[i]
 * (udp_hrnet_num_launches entries; the time of a merged launch -- ops sharing a `group` -- is split over
 * its members in proportion to their FLOPs).  Measurement aid for bench.py's roofline section. */
int udp_hrnet_profile(udp_hrnet* h, const float* in_nchw, int n, int flip_test, void* workspace,
                      size_t workspace_bytes, float* heatmaps_nchw, float* ms_per_op_host, void* stream);
int udp_hrnet_destroy(udp_hrnet* h);
/* Number of kernel launches of one forward, and algorithmic FLOPs (2*MAC) per image. */
int udp_hrnet_num_launches(const udp_hrnet* h);
double udp_hrnet_flops_per_image(const udp_hrnet* h);

/* One fused conv launch on raw pointers (the operator the program above is made of; used by
 * the per-layer parity tests and kernel benchmarks).  `op` supplies kind (UDP_OP_CONV, UDP_OP_FUSE,
 * UDP_OP_DECONV, UDP_OP_DWCONV, UDP_OP_PIXSHUF, UDP_OP_SE, UDP_OP_GNORM, UDP_OP_LINATTN, UDP_OP_LNORM, UDP_OP_MHATTN, UDP_OP_ACT, UDP_OP_SE_RES, UDP_OP_PRM_GATE, UDP_OP_PRM_DW9 or UDP_OP_SE_ACT: NHWC in / out, weights as documented there, no res / up -- except the
 * passthrough of UDP_OP_DWCONV: source `res`, destination `up0`; UDP_OP_SE / UDP_OP_SE_ACT / UDP_OP_GNORM: `weights` = the parameter block, chain_cout = hidden width / real channels;
 * UDP_OP_LNORM: `weights` = the parameter block, chain_cout = real channels; UDP_OP_MHATTN: no weights, chain_cout = real width, up_shift[0] = heads;
 * UDP_OP_LINATTN / UDP_OP_ACT: no weights; UDP_OP_SE_RES: `weights` = the parameter block, chain_cout = hidden width, `res` = the shortcut or NULL;
 * UDP_OP_PRM_GATE: `weights` = the parameter block, `out` = fp32 [n][C]; UDP_OP_PRM_DW9: `res` = out_1, `up0` = the fp32 rows of UDP_OP_PRM_GATE), ks, stride, relu, cin, cout, cout_pad, hin, win, hout, wout, n_up, up_shift;
 * its buffer ids and blob offsets are ignored except out_buf == UDP_BUF_OUTPUT, which selects
 * the NCHW fp32 output form.  in/res/ups/out: NHWC `dtype`; weights [ks*ks][cout_pad][cin]
 * `dtype`; bias fp32 [cout_pad].  Replaces conv+BN(+add)(+ReLU), pose_hrnet.py:43-59.
 * UDP_OP_FUSE: out = act(in [+ res] + sum_k nearest_up(up_k, up_shift[k])), added in that order; up_shift 0 = an addend
 * of the output's own resolution (the training step's exchange-unit sums, pose_hrnet.py:266-272, have up to four terms);
 * weights / bias are ignored (may be NULL). */
int udp_conv2d_fused(const udp_conv_op* op_host, int dtype, int n, const void* in, const void* weights,
                     const float* bias, const void* res, const void* up0, const void* up1,
                     const void* up2, void* out, void* stream);
/* Training form of a plain conv (fp32 / bf16 NHWC, no addends, no ReLU): additionally leaves the statistics
 * pass of the BatchNorm2d that follows it (pose_hrnet.py:46, :83 ...: `bn(conv(x))` in train mode) in `bn_ws`:
 * one row of 2*cout doubles per workgroup tile -- sum x and sum x*x of the output AS STORED -- summed in the
 * conv epilogue instead of a separate pass over the tensor.  *bn_rows receives the row count
 * (<= udp_bn_rows_max()); feed both to udp_bn_train_fwd_from_sums. */
int udp_conv2d_fused_bn(const udp_conv_op* op_host, int dtype, int n, const void* in, const void* weights,
                        const float* bias, void* out, double* bn_ws, size_t bn_ws_doubles, int* bn_rows,
                        void* stream);

/* ------------------------------------------------------------------------- *
 * Flip-test fuse.  Replaces flip_back / flip_back_offset
 * (deep_hrnet/lib/utils/transforms.py:15-29 / :31-47) and
 * output = (output + output_flipped) * 0.5 (deep_hrnet/lib/core/function.py:161-171).
 * out[n,c,y,x] = 0.5f * (a[n,c,y,x] + sign[c] * b[n,src_ch[c],y,w-1-x]).
 * src_ch / sign: device arrays of length c (channel permutation and +-1).
 * out may alias a.
 * ------------------------------------------------------------------------- */
int udp_flip_fuse(const float* a, const float* b, const int32_t* src_ch, const float* sign,
                  int n, int c, int h, int w, float* out, void* stream);
/* Same, followed by a division: out = ((a + flip_back(b)) * 0.5f) / divisor.  The RSN test loop
 * divides the fused maps by 255 before decoding (RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/test.py:174-185). */
int udp_flip_fuse_scaled(const float* a, const float* b, const int32_t* src_ch, const float* sign,
                         int n, int c, int h, int w, float divisor, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * UDP decode.  Replaces get_final_preds (deep_hrnet/lib/core/inference.py:149-186):
 * get_max_preds :30-58, post (DARK/Taylor) :60-145, the offset branch :156-174 and
 * transform_preds :20-27.  heatmaps: fp32 [n, j*(offset?3:1), h, w] (not modified).
 * center, scale: fp64 [n,2]; cs_is_f32 != 0 says the caller's arrays were float32
 * (the reference then rounds scale*200, scale/(w-1) and scale*0.5 to fp32).
 * Outputs: preds fp64 [n,j,2] (image pixels), maxvals fp32 [n,j], preds_in fp64
 * [n,j,2] (preds_in_input_space), argidx int32 [n,j] (flat arg-max index; may be NULL).
 * ------------------------------------------------------------------------- */
int udp_decode_gaussian(const float* heatmaps, int n, int j, int h, int w, const double* center,
                        const double* scale, int cs_is_f32, int post_process, double* preds,
                        float* maxvals, double* preds_in, int32_t* argidx, void* stream);
int udp_decode_offset(const float* heatmaps, int n, int j, int h, int w, const double* center,
                      const double* scale, int cs_is_f32, float kpd, double* preds, float* maxvals,
                      double* preds_in, int32_t* argidx, void* stream);
/* Host helper: the 1-D Gaussian taps cv2.GaussianBlur(ksize, sigma=0) uses (fp32). */
int udp_gaussian_taps_host(int ksize, float* taps_host);

/* ------------------------------------------------------------------------- *
 * UDP data path.
 * udp_warp_affine: cv2.warpAffine(INTER_LINEAR, constant-0 border) on a uint8
 * HxWx3 frame + ToTensor + Normalize, one 2x3 dst->src matrix per crop
 * (deep_hrnet/pose_engine.py:69-85,40-43 with the inverse of
 * tools/infer_utils/utils.py:157-177; deep_hrnet/lib/dataset/JointsDataset.py:226-227
 * with get_warpmatrix :29-49).  mats: fp64 [n,6] dst->src.  out: fp32 [n,3,oh,ow].
 * ------------------------------------------------------------------------- */
int udp_warp_affine(const uint8_t* frame, int fh, int fw, int row_stride_bytes, const double* mats,
                    int n, int oh, int ow, const float* mean3, const float* std3, float* out,
                    void* stream);
/* Same warp with the training loader's two source transforms folded in: flip_lr = the frame is read
 * mirrored left-right (data_numpy[:, ::-1, :], JointsDataset.py:218-219; same fixed-point taps),
 * swap_rb = cv2.COLOR_BGR2RGB (:195-196).  mats: the get_warpmatrix dst->src matrix (:226-227). */
int udp_warp_affine_ex(const uint8_t* frame, int fh, int fw, int row_stride_bytes, const double* mats,
                       int n, int oh, int ow, const float* mean3, const float* std3, int flip_lr,
                       int swap_rb, float* out, void* stream);
/* AID information dropping (Cutout / HideAndSeek, deep_hrnet/lib/utils/transforms.py:144-224) on
 * normalized crops img fp32 [n,3,h,w]: dropped pixels become (0-mean)/std.  cutout: fp64
 * [n,n_patch,4] = (cx, cy, rx, ry) per ellipse (rx <= 0: unused).  hs_grid int32 [n] (0 = off) and
 * hs_mask uint8 [n,mask_x,mask_y]: cell (i,j) drops rows [i*g,(i+1)*g) for i*g < w and columns
 * [j*g,(j+1)*g) for j*g < h -- the reference's x/y-swapped indexing (:172-177), kept.  NULL = off. */
int udp_aid_apply(float* img, int n, int h, int w, const double* cutout, int n_patch,
                  const int32_t* hs_grid, const uint8_t* hs_mask, int mask_x, int mask_y,
                  const float* mean3, const float* std3, void* stream);
/* generate_target (JointsDataset.py:291-385).  joints fp32 [n,j,2] in crop pixels,
 * vis fp32 [n,j].  gaussian: target [n,j,h,w]; offset: [n,3j,h,w].  weight [n,j]. */
int udp_target_gaussian(const float* joints, const float* vis, int n, int j, int img_w, int img_h,
                        int hm_w, int hm_h, float sigma, float* target, float* weight, void* stream);
int udp_target_offset(const float* joints, const float* vis, int n, int j, int img_w, int img_h,
                      int hm_w, int hm_h, float kpd, float* target, float* weight, void* stream);

/* ------------------------------------------------------------------------- *
 * JointsMSELoss / JointsMSELoss_offset forward + gradient
 * (deep_hrnet/lib/core/loss.py:15-39 / :41-76).  pred, target: fp32 [b,c,hw];
 * weight fp32 [b,j].  loss_out: fp64 [2] = (L_hm, L_offset) (L_offset = 0 for the
 * plain loss); grad: fp32 like pred (d(L_hm+L_offset)/d pred), may be NULL.
 * The two scalars are accumulated with fp64 atomic adds of per-workgroup partial sums, so
 * their last bits may differ from run to run (~1e-16 relative); the gradient is computed per
 * element and does not depend on them.
 * ------------------------------------------------------------------------- */
int udp_mse_loss(const float* pred, const float* target, const float* weight, int b, int j, int hw,
                 int is_offset, double* loss_out, float* grad, void* stream);

/* ------------------------------------------------------------------------- *
 * Keypoint rescoring + OKS-NMS: deep_hrnet/lib/dataset/coco.py:321-356 with
 * oks_iou / oks_nms of deep_hrnet/lib/nms/nms.py:75-124, all images in one launch.
 * Persons of image i are rows img_offsets[i] .. img_offsets[i+1] (both a device and a host copy of the
 * int32 [n_images+1] offsets are passed; at most 1024 persons per image).  kpts fp32 [P,J,3] (x, y,
 * score) in image pixels, areas / box_scores fp64 [P], vars fp64 [J] = (2*sigma_j)^2.
 * rescore != 0: score = mean(joint scores > in_vis_thre) * box_score (coco.py:326-341), else box_score.
 * use_vis != 0 reproduces oks_iou's in_vis_thre branch (only joints of the candidate above
 * oks_vis_thre count).  scores_out fp64 [P]; keep_rank int32 [P]: position in the keep list (selection
 * order = descending score) or -1 when suppressed (overlap > oks_thre with a kept pose).
 * soft != 0: soft_oks_nms (nms.py:139-175, TEST.SOFT_NMS): instead of suppressing, the remaining scores
 * are multiplied by exp(-oks^2 / oks_thre) after every pick; at most 20 picks per image.  scores_out still
 * holds the (re)scores before NMS, as the reference never writes the decayed scores back.
 * ------------------------------------------------------------------------- */
int udp_oks_nms(const float* kpts, const double* areas, const double* box_scores,
                const int32_t* img_offsets, const int32_t* img_offsets_host, int n_images, int num_joints,
                const double* vars_dev, double in_vis_thre, int rescore, double oks_thre, int use_vis,
                double oks_vis_thre, int soft, double* scores_out, int32_t* keep_rank, void* stream);

/* ------------------------------------------------------------------------- *
 * Training step (deep_hrnet/lib/core/function.py:38-77: model.train(), forward,
 * criterion, zero_grad / backward / step; optimizer lib/utils/utils.py:70-74).
 * Activations are NHWC `dtype` with the channel count rounded up to 16 (zero
 * filled); parameters, gradients and optimizer state are fp32 in the reference's
 * state_dict layouts.  The host (udp-pose_amd/train.py) keeps the tape.
 * ------------------------------------------------------------------------- */
/* conv weight [cout][cin][ks][ks] fp32 -> operand layouts of udp_conv2d_fused:
 *   w_fwd   [ks*ks][cout_pad=ceil32(cout)][cin_k=ceil16(cin)]                      (forward)
 *   w_dgrad [ks*ks][ceil32(cin)][ceil16(cout)], taps mirrored, Cin/Cout swapped  (input gradient;
 *           may be NULL).  conv2d backward w.r.t. the input of a stride-1 conv is
 *   udp_conv2d_fused(dy, w_dgrad); for stride 2 apply it to udp_zero_stuff2(dy).
 * ks in {1, 3, 7}: that; ks 7 is the stem of pose_resnet.py:112 (w_dgrad NULL: the image needs no gradient).
 * ks == 4 is ConvTranspose2d(4, 2, 1) (pose_resnet.py:155-193), fp32 only: w is the module's [cin][cout][4][4] and
 *   w_fwd   [16][ceil32(cout)][cin], entry 4*(2a+b) + 2t+u = w[ci][co][3-a-2t][3-b-2u]  (UDP_OP_DECONV, wfmt 0; cin % 16 == 0)
 *   w_dgrad [16][ceil32(cin)][ceil16(cout)], entry 4*ky+kx = w[ci][co][ky][kx], zero filled  (udp_deconv4s2_dgrad; may be NULL) */
int udp_pack_conv_weights(const float* w, int cout, int cin, int ks, int dtype, void* w_fwd,
                          void* w_dgrad, void* stream);
/* The same for every conv of a model in one launch: a device array of n descriptors (shapes are
 * validated by the host that builds the table; ks in {1,3,7}).  reserved == 1 marks a transposed conv (ks 4): w, cout,
 * cin and both layouts as udp_pack_conv_weights(ks = 4) documents them; reserved == 0 everywhere else. */
typedef struct udp_pack_desc {
  const float* w;
  void* w_fwd;
  void* w_dgrad; /* may be NULL */
  int32_t cout, cin, ks, reserved;
} udp_pack_desc;
int udp_pack_conv_weights_batch(const udp_pack_desc* descs_dev, int n, int dtype, void* stream);
/* out[n][2y][2x][c] = dy[n][y][x][c], zero elsewhere (out: [n][2h][2w][c]). */
int udp_zero_stuff2(const void* dy, int n, int h, int w, int c, int dtype, void* out, void* stream);
/* dW[co][ci][ky][kx] (+)= sum_{n,y,x} dy[n,y,x,co] * x[n, y*s+ky-ks/2, x*s+kx-ks/2, ci]
 * (torch.nn.functional.conv2d backward w.r.t. weight).  x: [n,hin,win,cin_k], dy: [n,hout,wout,cout_k].
 * workspace: split-K partials, at least ks*ks*cout*cin*4 bytes (udp_conv2d_wgrad_workspace_bytes
 * suggests a size that keeps the chip full).
 * (ks, padding) is one of (1, 0), (3, 1), (7, 3) -- the stem of pose_resnet.py:112, stride 2, cin 3 in cin_k 16 -- and
 * (4, 1).  ks == 4 is the weight gradient of ConvTranspose2d(4, 2, 1) (pose_resnet.py:155-193) with the roles swapped:
 * `x` is the gradient of its OUTPUT [n,2h,2w,cin_k], `dy` its INPUT [n,h,w,cout_k], cout / cin the module's input /
 * output channels, and dW [cout][cin][4][4] is then ConvTranspose2d.weight's own layout; it needs stride == 2,
 * hin == 2*hout and win == 2*wout (anything else: UDP_ERR_ARG).  ks 4 and 7 are fp32 only (UDP_ERR_UNSUPPORTED in bf16). */
size_t udp_conv2d_wgrad_workspace_bytes(int cout, int cin, int ks);
int udp_conv2d_wgrad(const void* x, const void* dy, int n, int hin, int win, int cin_k, int hout,
                     int wout, int cout_k, int ks, int stride, int cout, int cin, int dtype, float* dw,
                     int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Diagnostic, host only (no GPU, no HIP call): the kernel, tile and split-K choice udp_conv2d_wgrad makes for these
 * arguments and this workspace size -- the launch path calls the same function, so a launch runs exactly what is
 * reported here.  out[0] = kernel family (0: fp32 MFMA on fp32 tensors, 1: bf16 MFMA on bf16 tensors, 2: bf16 tensors
 * on the fp32 MFMA kernel, which is what UDP_POSE_WGRAD_F32MFMA selects; the variable is read at every call),
 * out[1..2] = TW, TH (a unit = TH x TW output pixels of one image), out[3..5] = units per row, per column, in all,
 * out[6] = upw (units a workgroup walks; the last workgroup may have fewer), out[7] = splits (partials; grid.y),
 * out[8] = PXP (TH*TW rounded up to 4, family 1: to 16), out[9] = staged rows (PXP + input patch rows),
 * out[10] = dynamic LDS bytes.  splits = min(target workgroups / channel tiles, units, workspace_bytes / bytes of one
 * partial), so a caller steers the split count through workspace_bytes.  Returns UDP_OK or the error udp_conv2d_wgrad
 * would return after its pointer check (shape, output size, workspace smaller than one partial, bf16 pitch, tile
 * limits).  Channels cin..cin_k of x and cout..cout_k of dy are read but reach no stored element: an MFMA row /
 * column depends on its own channel only and rows >= cout, columns >= cin are never stored, so the padding need
 * not be zero.  Adds a symbol only: UDP_POSE_ABI_VERSION stays as it is. */
int udp_debug_wgrad_tile(int n, int hin, int win, int cin_k, int hout, int wout, int cout_k, int ks, int stride,
                         int cout, int cin, int dtype, size_t workspace_bytes, int* out);
/* The weight gradients of up to 4 convs (the same-depth convs of the HRNet branches): the partial-sum kernels run
 * one per member, the fixed-order reduces of all members as ONE launch; results are those of udp_conv2d_wgrad per
 * member, bit for bit.  Every member needs its own workspace. */
typedef struct udp_wgrad_item {
  const void* x;
  const void* dy;
  float* dw;
  void* workspace;
  size_t workspace_bytes;
  int32_t n, hin, win, cin_k, hout, wout, cout_k, ks, stride, cout, cin, accumulate;
} udp_wgrad_item;
/* Diagnostic, host only (no GPU): the dispatch order of a merged weight-stationary launch whose member j has
 * tiles[j] pixel tiles x ncby[j] cout blocks and kernel variant code[j] (1, 2 or 4): for every flat workgroup
 * b < total the member, tile and cout block it computes, resolved as the kernel resolves them.  Returns total
 * (<= cap), -1 on error; *used_table = 1 when the one-load lookup table applies.  Tests check that every
 * (member, tile, cout block) is computed exactly once. */
int udp_debug_multi_order(const unsigned* tiles, const unsigned* ncby, const int* code, int n, unsigned cap,
                          unsigned* out_member, unsigned* out_tile, unsigned* out_cby, int* used_table);
/* Diagnostic, host only (no GPU, no HIP call): the tile and kernel arm the library's choosers pick for one UDP_OP_CONV
 * without channel views -- ks 1 | 3, stride 1 | 2, batch n, output map hout x wout, cin -> cout channels, nchw_out = the
 * net's NCHW fp32 output, grouped = as a member of a launch group.  wfmt 1 (UDP_F16X2): the weight-stationary chooser,
 * out[0] = PB (pixel blocks per wave of the instantiation that runs), out[1] = CP (cout pairs per workgroup).  wfmt 0:
 * the LDS-staged chooser, out[0] = NB (16-channel cout blocks per workgroup), out[1] = MBW (pixel blocks per wave).
 * Then out[2..7] = G, R, TW (tile = G images x R rows x TW columns), one stage buffer (0 | 1), dynamic LDS bytes,
 * workgroups; out[8] = grid.x of the persistent bf16 form when that is what runs (every workgroup then strides over
 * ceil(tiles / out[8]) tiles), else 0.  ks 7 (wfmt 0, stride 1, UDP_F32 | UDP_F16X2; csrc/conv7.hip): out[0] = NB, out[1] =
 * MBW, out[2..4] = G, R, TW, out[5] = 1 when the input halo tile has ONE LDS buffer (split fp16, or a single K chunk) and
 * 0 when it has two, out[6] = dynamic LDS bytes (halo buffers + the two buffers of one kernel row of weights),
 * out[7] = workgroups, out[8] = 0; grouped: 1.  The choosers read UDP_POSE_WS_PB, UDP_POSE_WS_CP, UDP_POSE_MINWGS and
 * UDP_POSE_MAXM at every call, so a test can force an arm around one call.  Returns UDP_OK, 1 when grouped is set and
 * the conv is no member of a merged launch, or the error udp_conv2d_fused would return.  Adds a symbol only:
 * UDP_POSE_ABI_VERSION stays as it is.
 * With UDP_POSE_DEBUG_TILES set, describing a conv prints the same decision to stderr, one line per conv ("ws conv k..",
 * "conv k..", "grouped conv ..", "x0 share .."), and every merged launch of a program adds one line when it is described
 * (at every eager forward and when a graph is built):
 *   ws multi k<3|1>: members=<n> wgs=<workgroups> codes=[c0,..] dispatch=<table|search>
 *   lds multi <bf16|f16x2> k<3|1>: members=<n> wgs=<workgroups> codes=[m0,..] MBW=<3|4>
 * codes of "ws multi": each member's kernel variant in launch order (CP 1, 2 or 4; 8 = the 8-pixel-block arm); dispatch: whether
 * the kernel resolves a workgroup through the per-8 lookup table or the segment search.  codes of "lds multi": the MBW each
 * member was described for; MBW: that of the conv_mfma_multi instantiation that runs them all (the largest). */
int udp_debug_conv_tile(int dtype, int wfmt, int ks, int stride, int n, int hout, int wout, int cin, int cout,
                        int nchw_out, int grouped, int* out);
/* Diagnostic, host only (no GPU, no HIP call): the shared-input sets the executor forms over an op list in UDP_F16X2
 * (csrc/hrnet.hip, find_share_sets): the 3x3 stride-2 convs with 32 input channels and the 32-channel UDP_OP_FUSE that
 * read one input view run as ONE launch at the position of the earliest of them, where the buffer ids allow it.
 * carrier[i] = the op whose launch does op i's work (i itself for the carrying op), -1 for an op outside every set.
 * The ops are not validated and UDP_POSE_NO_X0_SHARE is not read.  Returns the number of sets, -1 on a null argument.
 * Adds a symbol only: UDP_POSE_ABI_VERSION stays as it is. */
int udp_debug_x0_share(const udp_conv_op* ops, int n_ops, int* carrier);
int udp_conv2d_wgrad_group(const udp_wgrad_item* items, int n_items, int dtype, void* stream);
/* Up to 4 independent plain convs (same dtype and batch n) in as few launches as possible -- the same-depth convs
 * of the HRNet branches in the training step (pose_hrnet.py:253-256): members whose tile fits the merged kernel run
 * as ONE launch, the rest on their own; per-member results are those of udp_conv2d_fused / udp_conv2d_fused_bn.
 * res (optional) is accumulated as in udp_conv2d_fused; bn_ws != NULL (then no res / ReLU): BatchNorm partial rows
 * as udp_conv2d_fused_bn leaves them, their count in bn_rows. */
typedef struct udp_conv_item {
  const udp_conv_op* op;
  const void* in;
  const void* weights;
  const float* bias;
  const void* res;
  void* out;
  double* bn_ws;
  size_t bn_ws_doubles;
  int32_t bn_rows;     /* out */
  int32_t reserved;
} udp_conv_item;
int udp_conv2d_fused_group(udp_conv_item* items, int n_items, int dtype, int n, void* stream);
/* nn.BatchNorm2d in train mode over x [m = N*H*W rows][c]: batch mean / biased variance (fp64 sums),
 * running_mean/var <- (1-momentum)*running + momentum*batch (unbiased variance), either may be NULL;
 * y = [relu](xhat*gamma + beta [+ res]).  save_mean / save_invstd fp32 [c] feed the backward.
 * c must be a multiple of 4.  ws: udp_bn_workspace_doubles(c) doubles of scratch (per-block partial
 * sums, summed in a fixed order: results are run-to-run deterministic).  A workspace serves one
 * stream at a time. */
size_t udp_bn_workspace_doubles(int c);
int udp_bn_train_fwd(const void* x, int64_t m, int c, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, float* save_mean,
                     float* save_invstd, const void* res, int relu, void* y, int dtype, double* ws,
                     void* stream);
/* The same with the statistics pass already done: `ws` holds `rows` partial rows of 2*c doubles
 * ([row][0..c) = sum x, [row][c..2c) = sum x*x), as udp_conv2d_fused_bn leaves them.  rows <= udp_bn_rows_max(). */
int udp_bn_rows_max(void);
int udp_bn_train_fwd_from_sums(const void* x, int64_t m, int c, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, float* save_mean,
                               float* save_invstd, const void* res, int relu, void* y, int dtype, double* ws,
                               int rows, void* stream);
/* Backward of the above.  g = dy * (y_relu > 0) when y_relu != NULL (the ReLU that followed), else dy.
 * dgamma = sum g*xhat, dbeta = sum g, dx = gamma*invstd*(g - dbeta/m - xhat*dgamma/m);
 * g_out (optional) receives g -- the gradient of the residual input. */
int udp_bn_train_bwd(const void* x, const void* dy, const void* y_relu, int64_t m, int c,
                     const float* gamma, const float* save_mean, const float* save_invstd, float* dgamma,
                     float* dbeta, void* dx, void* g_out, int dtype, double* ws, void* stream);
/* Up to 4 BatchNorms per call (the bn1 / bn2 of one block depth of every HRNet branch are independent,
 * pose_hrnet.py:253-256: train.py runs the branches in lock step): each pass is ONE launch over all tensors,
 * per-tensor arithmetic and results are those of the single-tensor entry points above, bit for bit.
 * Forward reads x, gamma, beta, running_*, res, relu, rows (> 0: `ws` already holds that many partial rows from
 * udp_conv2d_fused_bn; 0: the partial sums are computed here) and writes save_*, y.  Backward reads x, dy, y_relu,
 * gamma, save_* and writes dgamma, dbeta, dx, g_out (optional).  Every tensor needs its own `ws`
 * (udp_bn_workspace_doubles(c) doubles). */
typedef struct udp_bn_item {
  const void* x;
  const void* dy;
  const void* y_relu;
  const void* res;
  void* y;
  void* dx;
  void* g_out;
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float* save_mean;
  float* save_invstd;
  float* dgamma;
  float* dbeta;
  double* ws;
  int64_t m;
  int32_t c, rows, relu, reserved;
} udp_bn_item;
int udp_bn_train_fwd_multi(const udp_bn_item* items, int n, float eps, float momentum, int dtype, void* stream);
int udp_bn_train_bwd_multi(const udp_bn_item* items, int n, int dtype, void* stream);
/* acc[n,y,x,c] (init ? = : +=) src[n, y>>shift, x>>shift, c], optional ReLU: the sum nodes of
 * HighResolutionModule.forward (pose_hrnet.py:266-272) with nn.Upsample(mode='nearest'). */
int udp_ew_accumulate(void* acc, const void* src, int n, int h, int w, int c, int shift, int init,
                      int relu, int dtype, void* stream);
/* g = dy * (y > 0). */
int udp_relu_bwd(const void* dy, const void* y, void* g, int64_t count, int dtype, void* stream);
/* Backward of nearest upsampling by 2^shift: du[n,y,x,c] (+)= sum of the 2^shift x 2^shift block of g
 * (g: [n,h,w,c], du: [n,h>>shift,w>>shift,c]). */
int udp_upsample_bwd(const void* g, int n, int h, int w, int c, int shift, void* du, int accumulate,
                     int dtype, void* stream);
/* db[c] = sum over the m rows of g[row*c_pitch + c] (conv bias gradient). */
int udp_bias_grad(const void* g, int64_t m, int c_pitch, int c, float* db, int dtype, void* stream);
/* NCHW fp32 [n,c,h,w] -> NHWC `dtype` [n,h,w,c_pad], channels c..c_pad zero. */
int udp_nchw_to_nhwc(const float* src, int n, int c, int h, int w, int c_pad, void* dst, int dtype,
                     void* stream);
/* torch.optim.Adam (no weight decay, no amsgrad) over flat fp32 buffers; step counts from 1.
 * The gradient is read as g*grad_scale (1/world_size after a SUM all-reduce; 1 otherwise). */
int udp_adam_step(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1,
                  float beta2, float eps, int step, float grad_scale, void* stream);
/* The same for a captured training step (hipGraph replay): the two step-dependent scalars
 * coef = {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step)} -- exactly the values udp_adam_step uses, as
 * udp_adam_coefficients computes them on the host -- are read from device memory at run time, so the host only
 * refreshes those 8 bytes before each replay. */
int udp_adam_coefficients(float lr, float beta1, float beta2, int step, float* coef_host);
int udp_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t count, float beta1, float beta2,
                      float eps, const float* coef_dev, float grad_scale, void* stream);

/* ------------------------------------------------------------------------- *
 * Training of pose_resnet (SimpleBaseline, deep_hrnet/lib/models/pose_resnet.py;
 * recipe experiments/coco/resnet/res50_256x192_d256x3_adam_lr1e-3.yaml): the ops
 * its graph has beyond the HRNet step above.  fp32 only (UDP_F32; anything else
 * is UDP_ERR_UNSUPPORTED).  Symbols only: UDP_POSE_ABI_VERSION stays as it is.
 * The weight gradients of the transposed conv and of the stem are
 * udp_conv2d_wgrad with ks 4 / 7; their packed operands come from
 * udp_pack_conv_weights(_batch).
 * ------------------------------------------------------------------------- */
/* Input gradient of ConvTranspose2d(4, 2, 1) (pose_resnet.py:155-193, deconv_layers; autograd's backward of :203):
 *   dx[n,iy,ix,ci] = sum_{co,ky,kx} dy[n, 2iy-1+ky, 2ix-1+kx, co] * w[ci][co][ky][kx]
 * dy: NHWC [n, 2hin, 2win, cout_pitch], dx: NHWC [n, hin, win, cin_pitch] (channels 0..cin of every pixel are written,
 * nothing is accumulated), w_dgrad: the [16][ceil32(cin)][ceil16(cout)] operand of udp_pack_conv_weights(ks = 4).
 * cin % 16 == 0, cin <= 2048, cout % 8 == 0, pitches % 4 == 0.  One MFMA launch over an LDS-staged halo tile of dy: no
 * atomics, no zero-stuffed copy; a pixel's sum has one fixed order whatever the tiling. */
int udp_deconv4s2_dgrad(const void* dy, const void* w_dgrad, int n, int hin, int win, int cin, int cin_pitch,
                        int cout, int cout_pitch, int dtype, void* dx, void* stream);
/* MaxPool2d(kernel 3, stride 2, padding 1) (pose_resnet.py:116, :199) on NHWC [n,h,w,c], c % 4 == 0:
 * y [n, (h-1)/2+1, (w-1)/2+1, c].  The backward recomputes every window's arg-max -- its first maximum in row-major
 * window order, torch.max_pool2d's rule -- and gathers: dx [n,h,w,c] is written everywhere, no index tensor, no
 * atomics, a fixed order of the at most four addends. */
int udp_maxpool3s2_fwd(const void* x, int n, int h, int w, int c, int dtype, void* y, void* stream);
int udp_maxpool3s2_bwd(const void* x, const void* dy, int n, int h, int w, int c, int dtype, void* dx, void* stream);
/* conv1 of pose_resnet.py:112 in train mode (3 -> 64, 7x7, stride 2, padding 3, no bias, no ReLU; bn1 follows
 * unfolded, :113): x = the NHWC [n,h,w,cin_k] image of udp_nchw_to_nhwc (channels 3.. are not read), w_fwd = the
 * [49][64][cin_k] operand of udp_pack_conv_weights(cout 64, cin 3, ks 7) -- so cin_k must be 16 --,
 * y: NHWC [n, (h-1)/2+1, (w-1)/2+1, 64]. */
int udp_stem7_train_fwd(const void* x, const void* w_fwd, int n, int h, int w, int cin_k, int cout, int dtype,
                        void* y, void* stream);

/* ------------------------------------------------------------------------- *
 * Training of the ShuffleNetV2 pose nets (pose_shufflenetv2_10x_pixel_shuffle,
 * pose_shufflenetv2_10x; recipes experiments/coco/shufflenetv2/): the ops their
 * graph has beyond the two steps above (csrc/dw_train.hip, csrc/shufflenet_train.hip).
 * fp32 only (UDP_F32; anything else is UDP_ERR_UNSUPPORTED).
 *
 * All tensors are NHWC with a stored channel count that is a multiple of 4 (a thread owns 4 consecutive channels and
 * moves 16 bytes).  Every entry point writes EVERY stored channel of its outputs -- padded channels come out as zeros
 * computed from zeros --, uses no atomics, and sums in one order that depends on the shape alone: eager and captured
 * steps are bit-equal, and so are two runs.
 * ------------------------------------------------------------------------- */
/* Depthwise ks x ks conv (ks = 3 | 5), stride 1 | 2, padding ks/2, no bias, no activation (csrc/dw_train.hip;
 * shufflenetv2.py:54 branch_main.3, :66 branch_proj.0 and the depthwise member of a MobileNetV3 InvertedResidual, BLOCKS
 * columns `kernel`, `stride`, under model.train(); the BatchNorm that follows stays unfolded):
 *   y[n,oy,ox,ch] = sum_{ky,kx} x[n, oy*s+ky-ks/2, ox*s+kx-ks/2, ch] * w[ch][0][ky][kx]
 * as fmaf in (ky, kx) order with the taps outside the image skipped -- the contract of the inference kernel
 * (UDP_OP_DWCONV).  x: [n,hin,win,c]; w: the parameter itself, [c_real][1][ks][ks] fp32, read in place (no pack step),
 * 16-byte aligned; c_real <= c, channels c_real..c of y are written as zero.  y: [n,hout,wout,c] with
 * hout = (hin-1)/s + 1 (odd sizes allowed).  A thread owns a strip of consecutive output pixels of one row (2 for 3x3, 4
 * for 5x5) x 4 channels and loads each input column of a kernel row once for the whole strip.  ks other than 3 | 5,
 * stride other than 1 | 2: UDP_ERR_UNSUPPORTED. */
int udp_dwconvk_train_fwd(const void* x, const void* w, int n, int hin, int win, int c, int c_real, int ks, int stride,
                          int dtype, void* y, void* stream);
/* Its input gradient (autograd's backward w.r.t. the input), a gather over a strip of input pixels:
 *   dx[n,iy,ix,ch] (+)= sum_{ky,kx} dy[n, (iy+ks/2-ky)/s, (ix+ks/2-kx)/s, ch] * w[ch][ky][kx]
 * over the taps where both divisions are exact and the index lies inside dy [n,hout,wout,c]; (ky, kx) order from 0.
 * `accumulate` != 0 adds the sum to dx last (the input of a stride-2 ShuffleNetV2 unit feeds both branches, :81-84);
 * otherwise every element of dx [n,hin,win,c] is overwritten. */
int udp_dwconvk_dgrad(const void* dy, const void* w, int n, int hin, int win, int c, int c_real, int ks, int stride,
                      int accumulate, int dtype, void* dx, void* stream);
/* Its weight gradient, written in the parameter layout [c_real][1][ks][ks] (nothing is accumulated):
 *   dw[ch][ky][kx] = sum_{n,y,x} dy[n,y,x,ch] * x[n, y*s+ky-ks/2, x*s+kx-ks/2, ch]
 * Two launches.  The n*hout output rows are cut into `partials` runs of `rows` consecutive rows; a workgroup takes one
 * run and up to 64 channel groups (lanes along channels, ks^2 taps x 4 channels of fp32 accumulators per thread, its
 * pixel lanes combined through LDS in lane order, one kernel row at a time) and leaves a [ks^2][c] partial in the
 * workspace; the second launch adds the partials in index order.  partials = min(n*hout, 256, workspace_bytes /
 * (4 ks^2 c)), rows = ceil(n*hout / partials), partials = ceil(n*hout / rows): a pure function of the shape and the
 * workspace size.  A workspace that holds no partial: UDP_ERR_WORKSPACE.  udp_dwconvk_wgrad_workspace_bytes: what the
 * unconstrained split needs (0: bad shape or ks; udp_last_error() is left as it was), never more than 256 * 4 ks^2 c
 * bytes, which (n = 256, hout = 1) returns. */
size_t udp_dwconvk_wgrad_workspace_bytes(int n, int hout, int wout, int c, int ks);
int udp_dwconvk_wgrad(const void* x, const void* dy, int n, int hin, int win, int c, int c_real, int ks, int stride, int dtype,
                      void* dw, void* workspace, size_t workspace_bytes, void* stream);
/* Host only: the split udp_dwconvk_wgrad would use (it calls the same function).  out[0] = output rows per workgroup,
 * out[1] = workgroups of the first launch (partials x channel blocks), out[2] = partials, out[3] = LDS bytes of a
 * workgroup (256 * ks * 16).  Returns what the launch would return for this shape, ks and workspace. */
int udp_debug_dw_wgrad_plan(int n, int hout, int wout, int c, int ks, size_t workspace_bytes, int* out);
/* nn.PixelShuffle(2) in torch's own channel order (decoders/DUC.py:27 under model.train()) and its backward:
 *   y[n, 2h+i, 2w+j, ch] = x[n, h, w, 4ch + 2i + j]          x: [n,h,w,cin], y: [n,2h,2w,cin/4]
 * _bwd is the inverse: dy [n,2h,2w,cin/4] -> dx [n,h,w,cin]; h, w, cin describe the LOW-resolution tensor in both.
 * (The inference op UDP_OP_PIXSHUF assumes the planner's permuted conv groups; a trainer keeps the parameter order.)
 * cin % 64 == 0.  Pure data movement: bit patterns are never decoded. */
int udp_pixshuf2_train_fwd(const void* x, int n, int h, int w, int cin, int dtype, void* y, void* stream);
int udp_pixshuf2_train_bwd(const void* dy, int n, int h, int w, int cin, int dtype, void* dx, void* stream);
/* torch.cat + channel_shuffle of ShuffleV2Block.forward (shufflenetv2.py:77-92) without the concat.  A unit's output is
 * a pair (a, b) of [m][in_pitch] tensors with r real channels each; logical channel j of the concat is a[j] for j < r,
 * else b[j-r].  even[k] = logical[2k], odd[k] = logical[2k+1] for k < r and zeros for r <= k < cp; even / odd:
 * [m][cp], cp % 4 == 0.  r need not be a multiple of 4 (58 at 1.0x): elements are read one by one, stores are 16 bytes.
 * _bwd is the inverse permutation of (d_even, d_odd) [m][cp] into (d_a, d_b) [m][out_pitch], pads zero. */
int udp_shuffle_pair_fwd(const void* a, const void* b, int64_t m, int r, int in_pitch, int cp, int dtype, void* even,
                         void* odd, void* stream);
int udp_shuffle_pair_bwd(const void* d_even, const void* d_odd, int64_t m, int r, int cp, int out_pitch, int dtype,
                         void* d_a, void* d_b, void* stream);
/* The materialised concat where a whole unit tensor is read (the input of a stride-2 unit, :81-84, and of conv_last,
 * :143): y[:, :ra] = a, y[:, ra:ra+rb] = b, zeros up to c; a: [m][pa], b: [m][pb], y: [m][c], c % 4 == 0.
 * udp_chan_uncat2 is its inverse (and its backward): a = y[:, :ra], b = y[:, ra:ra+rb], pads zero; pa, pb % 4 == 0. */
int udp_chan_cat2(const void* a, int pa, int ra, const void* b, int pb, int rb, int64_t m, int c, int dtype, void* y,
                  void* stream);
int udp_chan_uncat2(const void* y, int c, int64_t m, int dtype, void* a, int pa, int ra, void* b, int pb, int rb,
                    void* stream);

/* ------------------------------------------------------------------------- *
 * Training of the MobileNetV3-small pose nets (pose_mobilenetv3_small_pixel_shuffle,
 * pose_mobilenetv3_small; recipes experiments/coco/mobilenetv3/): what their
 * backbone -- torchvision's mobilenet_v3_small().features,
 * deep_hrnet/lib/models/backbones/mobilenetv3.py:5-16; the block table is
 * udp_pose_amd/synth_mobilenetv3.py BLOCKS -- adds to a ShuffleNetV2 step
 * (csrc/mobilenetv3_train.hip).  fp32 only (UDP_F32; anything else is
 * UDP_ERR_UNSUPPORTED).
 *
 * The conventions of the section above hold: NHWC tensors with a stored channel count c % 4 == 0, c_real <= c real
 * channels first; every stored channel of every output is written and the padded ones are exact zeros; no atomics, one
 * summation order per shape (two runs, and eager and captured steps, are bit-equal); no host synchronisation and no
 * allocation (capturable in a hipGraph); every argument check comes before anything touches the device.
 * ------------------------------------------------------------------------- */
/* The depthwise convs of the InvertedResiduals are the udp_dwconvk_* of the section above. */
/* nn.Hardswish (BLOCKS column `activation` = "HS", and behind the stem and the last conv) over `count` fp32 values,
 * count a positive multiple of 4:  y = x * clamp(x + 3, 0, 6) / 6;
 *   dx = 0 (x < -3) | dy * (x / 3 + 0.5) (-3 <= x <= 3) | dy (x > 3)      (x: the forward's INPUT).
 * That is autograd's derivative of the clamp form.  At exactly x = -3 and x = 3 it differs from torch's
 * hardswish_backward (nn.Hardswish, the reference backbone's layer), which takes the outer pieces there: 0 and dy
 * instead of -0.5 dy and 1.5 dy.  Everywhere else the two are the same function.
 * A BatchNorm with relu = 0 followed by this launch is BatchNorm + Hardswish; 0 maps to 0, so pads stay zero. */
int udp_hswish_fwd(const void* x, void* y, int64_t count, void* stream);
int udp_hswish_bwd(const void* dy, const void* x, void* dx, int64_t count, void* stream);
/* torchvision.ops.SqueezeExcitation under model.train() (BLOCKS column `squeeze-excitation`; restated in
 * tests/mobilenetv3_ref.py:squeeze_excitation):  y = x * hardsigmoid(W2 relu(W1 mean_hw(x) + b1) + b2)  per image.
 * x, y: [n,h,w,c]; w1 = fc1.weight [sq][c_real][1][1], b1 [sq], w2 = fc2.weight [c_real][sq][1][1], b2 [c_real], fp32,
 * read as they are.  Kept for the backward: pool [n][c] = mean_hw(x) (fp32, pixels added in a fixed order), hid [n][sq]
 * after the ReLU, s [n][c] the gate pre-activation (pads of pool and s: 0).  Four launches: pool, fc1, fc2, scale. */
int udp_se_train_fwd(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, int n, int h, int w,
                     int c, int c_real, int sq, int dtype, float* pool, float* hid, float* s, void* y, void* stream);
/* Its backward.  A map pass reduces dgate[n][ch] = sum_hw dy * x and leaves ds = dgate / 6 where -3 <= s <= 3, else 0;
 * on the [n][.] rows: dh = (ds W2) (hid > 0), dpool = dh W1, and dW2 = ds^T hid, db2 = sum_n ds, dW1 = dh^T pool,
 * db1 = sum_n dh (parameter layouts, overwritten, images in index order); a second map pass writes
 * dx (+)= dy * hardsigmoid(s) + dpool / (h w).  workspace: udp_se_train_workspace_bytes(n, c, sq) bytes (0: bad shape);
 * less is UDP_ERR_WORKSPACE. */
size_t udp_se_train_workspace_bytes(int n, int c, int sq);
int udp_se_train_bwd(const void* dy, const void* x, const float* w1, const float* w2, const float* pool, const float* hid,
                     const float* s, int n, int h, int w, int c, int c_real, int sq, int accumulate, int dtype, void* dx,
                     float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Training of pose_mobilevitv2_pixel_shuffle (recipes experiments/coco/mobilevitv2/): what its backbone --
 * deep_hrnet/lib/models/backbones/mobilevitv2.py, restated in tests/mobilevitv2_ref.py -- adds to a MobileNetV3 step
 * (csrc/mobilevitv2_train.hip).  fp32 only (UDP_F32; anything else is UDP_ERR_UNSUPPORTED, "fp32 only").
 *
 * The conventions of the two sections above hold: NHWC tensors with a stored channel count that is a multiple of 4
 * (the trainer stores ceil16 of the real count), real channels first; every stored channel of every output is written
 * and the padded ones are exact zeros; no atomics, one summation order per shape (two runs, and eager and captured
 * steps, are bit-equal); no host synchronisation and no allocation; every argument check comes before any launch.
 * New symbols only, so UDP_POSE_ABI_VERSION stays as it is.
 * ------------------------------------------------------------------------- */
/* nn.SiLU (mobilevitv2.py:78-79, get_activation_fn 'swish') over `count` fp32 values, count a positive multiple of 4:
 *   y = x * (1 / (1 + exp(-x)))  (the arithmetic of UDP_ACT_SILU);   dx = dy * s * (1 + x * (1 - s)), s = 1 / (1 + exp(-x))
 * (x: the forward's INPUT).  Finite for every finite x: where exp(-x) overflows s is 0 (y = -0, dx = 0), where it
 * underflows s is 1 (y = x, dx = dy).  0 maps to 0, so pads stay zero. */
int udp_silu_fwd(const void* x, void* y, int64_t count, void* stream);
int udp_silu_bwd(const void* dy, const void* x, void* dx, int64_t count, void* stream);
/* GroupNorm(num_groups = 1, C) under model.train() -- "layer_norm_2d", mobilevitv2.py:139-140 (pre_norm_attn.0,
 * pre_norm_ffn.0 of every LinearAttnFFN :779-817 and the block's last norm :932-934).  x, y: [n,h,w,ck]; gamma, beta:
 * c_real floats.  Per image over its c_real*h*w REAL elements (pads are not counted):
 *   mu = mean(x)   r = 1 / sqrt(mean((x - mu)^2) + eps)   y = (x - mu) * r * gamma[c] + beta[c]   (pads of y: 0)
 * save: [n][2] = (mu, r).  The statistics are shifted sums in fp64, sum(x - x0) and sum((x - x0)^2) with x0 the image's
 * first element, so a map whose mean is 1000 x its standard deviation keeps its variance.  An image's pixels are cut
 * into `split` runs of consecutive pixels, one workgroup each, split = udp_gnorm_train_split(h, w, ck): a pure function
 * of the shape (a run holds at least 1024 16-byte channel groups, at most 64 runs); the runs' partial sums go through the
 * workspace and are added in index order.  Two launches.  workspace: udp_gnorm_train_workspace_bytes(n, h, w, ck) =
 * n * split * (16 + 8 ck) bytes, for the forward and the backward alike (0: bad shape); less is UDP_ERR_WORKSPACE. */
int udp_gnorm_train_split(int h, int w, int ck);
size_t udp_gnorm_train_workspace_bytes(int n, int h, int w, int ck);
int udp_gnorm_train_fwd(const void* x, const float* gamma, const float* beta, int n, int h, int w, int ck, int c_real,
                        int dtype, float eps, void* y, float* save, void* workspace, size_t workspace_bytes, void* stream);
/* Its backward (autograd through F.group_norm), with g^ = dy * gamma[c] and x^ = (x - mu) * r:
 *   dx (+)= r * (g^ - mean(g^) - x^ * mean(g^ x^))      (means over the image's real elements; pads of dx: 0)
 *   dgamma[c] = sum_{n,h,w} dy x^     dbeta[c] = sum_{n,h,w} dy      (c < c_real only; overwritten)
 * `accumulate` != 0 adds into an existing dx (the input of every GroupNorm also feeds the residual).  Three launches:
 * per run the two image sums (fp64) and the per-channel sums (fp32, the run's pixels in a fixed order), the dx pass,
 * and dgamma / dbeta = the (image, run) partials added in index order. */
int udp_gnorm_train_bwd(const void* dy, const void* x, const float* gamma, const float* save, int n, int h, int w, int ck,
                        int c_real, int dtype, int accumulate, void* dx, float* dgamma, float* dbeta, void* workspace,
                        size_t workspace_bytes, void* stream);
/* The separable ("linear") self-attention core between qkv_proj and out_proj under model.train():
 * LinearSelfAttention._forward_self_attn, mobilevitv2.py:671-689, in the map form of
 * tests/mobilevitv2_ref.py:linear_attention_core -- the four patch positions are the parity classes (y & 1, x & 1) of
 * the map, M = h*w/4 pixels each, in row-major order of the (h/2, w/2) grid.  qkv: [n,h,w,ck_qkv], the qkv conv's
 * output in the PARAMETER's channel order (channel 0 the query, 1..d the keys, d+1..2d the values; not the key | value
 * | query order of the packed inference weights), ck_qkv = ceil16(1 + 2d).  Per image and class:
 *   s_i = softmax_i(q_i) (maximum subtracted)   ctx[c] = sum_i s_i k_ic   out_ic = relu(v_ic) * ctx[c]
 * out: [n,h,w,ck_out], ck_out >= d, channels d.. zero.  Kept for the backward: scores [n][4][M], ctx [n][4][d]
 * (class = (y & 1) * 2 + (x & 1)).  One launch, a workgroup per (image, class).  h and w even, d % 16 == 0, d <= 512,
 * M <= 2048: otherwise UDP_ERR_UNSUPPORTED; ck_qkv or ck_out that do not fit d: UDP_ERR_ARG. */
int udp_linattn_train_fwd(const void* qkv, int n, int h, int w, int ck_qkv, int d, int dtype, void* out, int ck_out,
                          float* scores, float* ctx, void* stream);
/* Its backward, g = dout:
 *   dv_ic = g_ic ctx[c] [v_ic > 0]  (0 at v = 0, torch's rule)    dctx[c] = sum_i g_ic relu(v_ic)    dk_ic = s_i dctx[c]
 *   e_i = sum_c k_ic dctx[c]        dq_i = s_i (e_i - sum_j s_j e_j)
 * All ck_qkv channels of dqkv [n,h,w,ck_qkv] are written, the pads as zero (qkv has one consumer: nothing accumulates). */
int udp_linattn_train_bwd(const void* dout, const void* qkv, const float* scores, const float* ctx, int n, int h, int w,
                          int ck_qkv, int d, int ck_out, int dtype, void* dqkv, void* stream);

/* ------------------------------------------------------------------------- *
 * Training of the polarized self-attention block of pose_hrnet_psa.  Replaces
 * PSA_s.forward (deep_hrnet/lib/models/PSA.py:190-269: spatial_pool :190-222,
 * channel_pool :224-258) under model.train() and its autograd backward.
 *
 * New symbols rather than new udp_conv_op kinds: the backward reads and writes more tensors (gradient maps, ten
 * parameter gradients, a save area) than udp_conv2d_fused has arguments for.  They are an addition old callers never
 * see, so UDP_POSE_ABI_VERSION stays as it is.
 *
 * One block, per image on an NHWC map x [h*w][c] of `dtype` (UDP_F32 | UDP_BF16; c divides 256, a multiple of 16,
 * at least 32 -- the inference ops UDP_OP_PSA_* also take c = 512, training does not):
 *   a = softmax_HW(wq.x_p)   xbar = sum_p a_p x_p   m = sigmoid(W2 relu(LN(W1 Wv xbar + b1)) + b2)   x1 = x * m[c]
 *   gbar = Wg mean_p(x1)     theta = Wt x1          s_p = sigmoid(sum_j gbar_j softmax_HW(theta_j)_p) x2 = x1 * s_p
 * theta (c/2 channels) and its backward (dWt, dx1 += Wt^T dtheta) are the caller's 1x1 conv: udp_conv2d_fused,
 * udp_conv2d_wgrad.  Call order of a step:
 *   udp_psa_train_fwd_pool   reads x, w               writes x1
 *   (theta = conv1x1(x1, conv_v_left))
 *   udp_psa_train_fwd_sp     reads x1, theta          writes x2
 *   ...
 *   udp_psa_train_bwd_sp     reads dx2, x1, theta, w  writes dtheta, dx1 (= dx2 * s_p + Wg^T dgbar / HW)
 *   (dx1 += conv1x1(dtheta, conv_v_left^T); d conv_v_left = wgrad(x1, dtheta))
 *   udp_psa_train_bwd_pool   reads dx1, x, w          writes dx
 *   udp_psa_train_bwd_params                          writes dw (overwritten, not accumulated; may run on another
 *                                                     stream ordered behind udp_psa_train_bwd_pool)
 * `save` (udp_psa_train_save_floats(n, h, w, c) floats, 0 for an unsupported shape) carries what the forward keeps
 * for the backward (soft-max logits and statistics, LayerNorm statistics, r, m, gbar, s_p) and the per-image partial
 * sums; it belongs to one block from its fwd_pool to its bwd_params.  All reductions are fp32 in a fixed order
 * (partial rows per pixel chunk added in row order, images in image order): no atomics, bit-identical reruns.
 * w / dw: fp32, the reference's tensors flattened, in registration order without conv_v_left --
 *   0 conv_q_right.weight [c]       1 conv_v_right.weight [c/2][c]  2 conv_up.0.weight [c/8][c/2]  3 conv_up.0.bias [c/8]
 *   4 conv_up.1.weight (LN) [c/8]   5 conv_up.1.bias (LN) [c/8]     6 conv_up.3.weight [c][c/8]    7 conv_up.3.bias [c]
 *   8 conv_q_left.weight [c/2][c]   -- each 16-byte aligned.
 * Every call checks the pointers it uses (UDP_ERR_ARG), the shape and dtype (UDP_ERR_UNSUPPORTED for a channel count
 * outside the range above and for UDP_F16X2) and the size of `save` (UDP_ERR_WORKSPACE) before it launches anything.
 * ------------------------------------------------------------------------- */
typedef struct udp_psa_train_args {
  const float* w[9];
  float* dw[9];
  const void* x;       /* [n][h*w][c]   block input */
  void* x1;            /* [n][h*w][c]   x * m            (written by fwd_pool, read by fwd_sp / bwd_sp) */
  const void* theta;   /* [n][h*w][c/2] conv_v_left(x1) */
  void* x2;            /* [n][h*w][c]   block output */
  const void* dx2;     /* gradient of x2 */
  void* dtheta;        /* gradient of theta */
  void* dx1;           /* gradient of x1: written by bwd_sp, completed by the caller's conv, read by bwd_pool */
  void* dx;            /* gradient of x */
  float* save;
  size_t save_floats;
  int32_t n, h, w_px, c;   /* images, map height, map width, channels */
} udp_psa_train_args;
size_t udp_psa_train_save_floats(int n, int h, int w, int c);
int udp_psa_train_fwd_pool(const udp_psa_train_args* args, int dtype, void* stream);
int udp_psa_train_fwd_sp(const udp_psa_train_args* args, int dtype, void* stream);
int udp_psa_train_bwd_sp(const udp_psa_train_args* args, int dtype, void* stream);
int udp_psa_train_bwd_pool(const udp_psa_train_args* args, int dtype, void* stream);
int udp_psa_train_bwd_params(const udp_psa_train_args* args, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UDP_POSE_HIP_H */
