// GroupNorm(1, C) (UDP_OP_GNORM) and the separable self-attention core (UDP_OP_LINATTN) of MobileViTv2 for gfx950
// (MI355X): the two ops of pose_mobilevitv2_pixel_shuffle between the 1x1 convs of an attention unit
// (deep_hrnet/lib/models/backbones/mobilevitv2.py:139-140 "layer_norm_2d", :664-691 LinearSelfAttention).
//
// Both are reductions over one image followed by an element-wise pass, on maps of at most a few hundred KB that stay
// in the L2 between the passes: ONE workgroup of 1024 threads per image (as se_kernel has one of 256), lanes along the
// channels with 16-byte loads (dw_dev.h), no atomics, every sum in an order that depends on the op's shape only -- so
// an image's result does not depend on the batch, the sub-batch lane or graph replay.
//
// The reference unfolds the map into [B, C, P = 4, N] patches before the attention units and folds it back after them
// (:1026-1055).  Nothing between the two looks across P except through these two ops, so the NHWC map is never
// rearranged: GroupNorm runs over the whole sample anyway, and the attention takes position p = 2 (y & 1) + (x & 1)
// of pixel (y, x) as the soft-max class.
//
// Further down: the three ops pose_mobilevit_pixel_shuffle adds (MobileViT v1) -- LayerNorm per pixel (UDP_OP_LNORM),
// soft-max multi-head self-attention over a position class (UDP_OP_MHATTN) and the stand-alone activation (UDP_OP_ACT).
// Those are per-pixel / per-query kernels with many workgroups per image, under the same rules: no atomics, fixed order.
#include "dw_dev.h"

namespace udp {

constexpr int kAttnThreads = 1024;

// sum of `v` over the workgroup, fp64, a fixed tree over the thread index; `red`: kAttnThreads doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                       // the previous use of `red` is over
  red[tid] = v;
  __syncthreads();
  for (int s = kAttnThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// UDP_OP_GNORM (udp_pose_hip.h).  thread = (pixel group g, channel group cg): it owns channels cg * V .. + V-1 of the
// pixels g, g + P, ... (P = 1024 / (C / V) groups).  Three reads of the map: the sum, the squared deviations from
// the mean (two-pass variance; fp64 per-thread partials), the normalisation.  Only the r = p.up_shift[0] real channels
// count; the pad channels are written as zeros.  An element is read and written by the same thread and both
// statistics are complete (block_sum ends in a barrier) before the first store: `out` may be the very view `in` is.
// Parameter block (fp32): gamma [C], beta [C].
template <typename T>
__global__ __launch_bounds__(kAttnThreads) void gnorm_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  __shared__ double red[kAttnThreads];
  const int C = p.Cin, r = p.up_shift[0], HW = p.Hin * p.Win;
  const int tid = threadIdx.x;
  const size_t img = (size_t)blockIdx.x * HW;
  const int cgs = C / V;
  const int P = kAttnThreads / cgs;                       // cgs <= 128 (gnorm_validate: C <= 512)
  const int cg = tid % cgs, g = tid / cgs, c0 = cg * V;
  const bool active = g < P && c0 < r;
  const double cnt = (double)r * (double)HW;

  double s = 0.0;
  if (active)
    for (int px = g; px < HW; px += P) {
      float x[V];
      dw_load<T, V>(p, img + px, c0, x);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (c0 + k < r) s += (double)x[k];
    }
  const double mean = block_sum(s, red) / cnt;      // kept in fp64: x - mean is then exact to the rounding of the result

  double q = 0.0;
  if (active)
    for (int px = g; px < HW; px += P) {
      float x[V];
      dw_load<T, V>(p, img + px, c0, x);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (c0 + k < r) {
          const double d = (double)x[k] - mean;
          q += d * d;
        }
    }
  const float rstd = (float)(1.0 / sqrt(block_sum(q, red) / cnt + 1e-5));

  if (g < P) {
    const float* gam = reinterpret_cast<const float*>(p.wgt) + c0;
    float ga[V], be[V];
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(gam + k), b = *reinterpret_cast<const f32x4*>(gam + C + k);
      ga[k] = a[0], ga[k + 1] = a[1], ga[k + 2] = a[2], ga[k + 3] = a[3];
      be[k] = b[0], be[k + 1] = b[1], be[k + 2] = b[2], be[k + 3] = b[3];
    }
    for (int px = g; px < HW; px += P) {
      float x[V];
      dw_load<T, V>(p, img + px, c0, x);
#pragma unroll
      for (int k = 0; k < V; ++k) x[k] = c0 + k < r ? __builtin_fmaf((float)((double)x[k] - mean) * rstd, ga[k], be[k]) : 0.f;
      dw_store<T, V>(p, img + px, c0, x);                 // (p.relu == 0: gnorm_validate)
    }
  }
}

// the single channel `c` of pixel `pix` of the input view, decoded to fp32
template <typename T>
__device__ __forceinline__ float attn_load1(const ConvParams& p, size_t pix, int c) {
  if constexpr (std::is_same<T, float>::value) {
    return reinterpret_cast<const float*>(p.in)[pix * (size_t)p.in_pitch + p.in_coff + c];
  } else {
    const _Float16* q = reinterpret_cast<const _Float16*>(p.in) + pix * (2 * (size_t)p.in_pitch) + p.in_coff + c;
    return (float)q[0] + (float)q[p.in_pitch] * kLoInv;
  }
}

// UDP_OP_LINATTN (udp_pose_hip.h).  Input pixel: key [0, C), value [C, 2C), query at 2C (C = p.Cout).  Phases,
// separated by barriers:
//   1. q of every pixel -> LDS (qs[HW]);
//   2. wave p (p = 0..3) owns position class p: the class maximum, then e = exp(q - max) and its sum, both by a
//      lane loop over the class's pixels j = lane, lane + 64, ... and a butterfly over the wave; qs <- e / sum;
//   3. thread = (pixel group g, channel group cg), g = 4 sg + p: ctx partial of class p over the class pixels
//      sg, sg + SG, ... (raster order inside the class), fmaf from 0 -> part[g][C]; then thread (p, c) adds the SG
//      partials of its class in the order sg = 0 .. SG-1 -> ctx[p][C];
//   4. out = max(v, 0) * ctx[class of the pixel], every element by one thread.
// Class pixel j of class p is pixel (2 (j / (W/2)) + (p >> 1), 2 (j % (W/2)) + (p & 1)).
// Dynamic LDS: (HW + 4 SG C + 4 C) floats, SG = (1024 / (C / V)) / 4.
template <typename T>
__global__ __launch_bounds__(kAttnThreads) void linattn_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  extern __shared__ __attribute__((aligned(16))) float la_s[];
  const int C = p.Cout, H = p.Hin, W = p.Win, HW = H * W, W2 = W >> 1, NC = HW >> 2;
  const int cgs = C / V;
  const int SG = (kAttnThreads / cgs) >> 2;               // cgs <= 128 (linattn_validate: C <= 512): SG >= 2
  float* qs = la_s;                                        // [HW]
  float* part = qs + HW;                                   // [4 SG][C]
  float* ctx = part + 4 * SG * C;                          // [4][C]
  const int tid = threadIdx.x;
  const size_t img = (size_t)blockIdx.x * HW;
  auto class_pixel = [&](int cls, int j) { return (2 * (j / W2) + (cls >> 1)) * W + 2 * (j % W2) + (cls & 1); };

  for (int px = tid; px < HW; px += kAttnThreads) qs[px] = attn_load1<T>(p, img + px, 2 * C);
  __syncthreads();
  if (tid < 256) {
    const int cls = tid >> 6, lane = tid & 63;
    float m = -INFINITY;
    for (int j = lane; j < NC; j += 64) m = __builtin_fmaxf(m, qs[class_pixel(cls, j)]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
    for (int j = lane; j < NC; j += 64) {
      const int px = class_pixel(cls, j);
      const float e = expf(qs[px] - m);
      qs[px] = e;
      s += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);     // (a + b on both sides: every lane holds the same sum)
    for (int j = lane; j < NC; j += 64) {
      const int px = class_pixel(cls, j);
      qs[px] = qs[px] / s;
    }
  }
  __syncthreads();
  {
    const int cg = tid % cgs, g = tid / cgs;
    if (g < 4 * SG) {
      const int cls = g & 3, sg = g >> 2;
      float a[V];
#pragma unroll
      for (int k = 0; k < V; ++k) a[k] = 0.f;
      for (int j = sg; j < NC; j += SG) {
        const int px = class_pixel(cls, j);
        const float sc = qs[px];
        float x[V];
        dw_load<T, V>(p, img + px, cg * V, x);            // the key
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = __builtin_fmaf(sc, x[k], a[k]);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) part[g * C + cg * V + k] = a[k];
    }
  }
  __syncthreads();
  for (int e = tid; e < 4 * C; e += kAttnThreads) {
    const int cls = e / C, c = e % C;
    float s = part[cls * C + c];
    for (int sg = 1; sg < SG; ++sg) s += part[(4 * sg + cls) * C + c];
    ctx[e] = s;
  }
  __syncthreads();
  for (int e = tid; e < HW * cgs; e += kAttnThreads) {
    const int cg = e % cgs, px = e / cgs;
    const int y = px / W, x0 = px % W;
    const float* cx = ctx + (2 * (y & 1) + (x0 & 1)) * C + cg * V;
    float v[V];
    dw_load<T, V>(p, img + px, C + cg * V, v);             // the value
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = __builtin_fmaxf(v[k], 0.f) * cx[k];
    dw_store<T, V>(p, img + px, cg * V, v);                // (p.relu == 0: linattn_validate)
  }
}

// ---------------------------------------------------------------------------------------------- MobileViT (v1)
// LayerNorm per token (UDP_OP_LNORM), soft-max multi-head self-attention (UDP_OP_MHATTN) and the stand-alone activation
// (UDP_OP_ACT) of pose_mobilevit_pixel_shuffle (deep_hrnet/lib/models/backbones/mobilevit.py:369-514, :517-677).  A token
// is a pixel of the NHWC map, so LayerNorm is a reduction over one pixel's contiguous channels; the attention mixes the
// N = HW / 4 pixels of one 2x2-position class of one image (the [B P, N, C] tensor of :593-632 is never built).

constexpr int kLnLanes = 16;       // lanes that share one pixel's channels
constexpr int kLnThreads = 256;    // 16 pixels per workgroup

// UDP_OP_LNORM (udp_pose_hip.h).  kLnLanes lanes per pixel; lane l owns the channel groups l, l + 16, ... of V channels
// (at most MG of them: C <= 512), held in registers between the passes.  mean: the lane adds its real channels in
// ascending order in fp64, then a butterfly over the 16 lanes (a + b on both sides: every lane holds the same sum);
// variance: the same over (x - mean)^2.  An element is read and written by the same thread and the pixel's row is in
// registers before the first store: `out` may be the very view `in` is.  Parameter block (fp32): gamma [C], beta [C].
template <typename T>
__global__ __launch_bounds__(kLnThreads) void lnorm_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  constexpr int MG = 512 / V / kLnLanes;                     // 8 (fp32) / 4 (split fp16) channel groups per lane
  const int C = p.Cin, r = p.up_shift[0];
  const int ngroups = C / V;
  const int l = threadIdx.x % kLnLanes;
  const long pix = (long)blockIdx.x * (kLnThreads / kLnLanes) + threadIdx.x / kLnLanes;
  const bool live = pix < (long)p.N * p.Hin * p.Win;                              // (the shuffles below need every lane of the wave)
  float x[MG][V];
  double s = 0.0;
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    const int c0 = (l + g * kLnLanes) * V;
    if (live && l + g * kLnLanes < ngroups) {
      dw_load<T, V>(p, (size_t)pix, c0, x[g]);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (c0 + k < r) s += (double)x[g][k];
    }
  }
#pragma unroll
  for (int o = kLnLanes / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const double mean = s / (double)r;
  double q = 0.0;
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    const int c0 = (l + g * kLnLanes) * V;
    if (live && l + g * kLnLanes < ngroups) {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (c0 + k < r) {
          const double d = (double)x[g][k] - mean;
          q += d * d;
        }
    }
  }
#pragma unroll
  for (int o = kLnLanes / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = (float)(1.0 / sqrt(q / (double)r + 1e-5));
  const float* gam = reinterpret_cast<const float*>(p.wgt);
#pragma unroll
  for (int g = 0; g < MG; ++g) {
    const int c0 = (l + g * kLnLanes) * V;
    if (live && l + g * kLnLanes < ngroups) {
      float y[V];
#pragma unroll
      for (int k = 0; k < V; k += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(gam + c0 + k), b = *reinterpret_cast<const f32x4*>(gam + C + c0 + k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          y[k + j] = c0 + k + j < r ? __builtin_fmaf((float)((double)x[g][k + j] - mean) * rstd, a[j], b[j]) : 0.f;
      }
      dw_store<T, V>(p, (size_t)pix, c0, y);                 // (p.relu == 0: lnorm_validate)
    }
  }
}

// UDP_OP_ACT (udp_pose_hip.h): out = act(in), thread = (pixel, channel group); ACT = UDP_ACT_HSWISH | UDP_ACT_SILU.
// An element is read and written by the same thread: `out` may be `in`.
template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int cgs = p.Cin / V;
  if (e >= (long)p.N * p.Hin * p.Win * cgs) return;
  const size_t pix = (size_t)(e / cgs);
  const int c0 = (int)(e % cgs) * V;
  float x[V];
  dw_load<T, V>(p, pix, c0, x);
#pragma unroll
  for (int k = 0; k < V; ++k) x[k] = act_hs<ACT>(x[k]);
  dw_store<T, V>(p, pix, c0, x);                            // (p.relu == 0 here: describe_act moved the code into ACT)
}

// the single channel `c` of pixel `pix` of the output view <- v (split again in the split-fp16 mode, with the range guard)
template <typename T>
__device__ __forceinline__ void attn_store1(const ConvParams& p, size_t pix, int c, float v) {
  if constexpr (std::is_same<T, float>::value) {
    reinterpret_cast<float*>(p.out)[pix * (size_t)p.out_pitch + p.out_coff + c] = v;
  } else {
    h2_range_check(__builtin_fabsf(v));
    _Float16* q = reinterpret_cast<_Float16*>(p.out) + pix * (2 * (size_t)p.out_pitch) + p.out_coff + c;
    const _Float16 hi = (_Float16)v;
    q[0] = hi;
    q[p.out_pitch] = (_Float16)((v - (float)hi) * kLoScale);
  }
}

constexpr int kMhaThreads = 256;
constexpr int kMhaKB = 32;         // keys staged in LDS at a time
constexpr int kMhaSub = 8;         // keys per soft-max update

// units (class, head) that share a workgroup: N <= 64 queries fill one wave, so four units take a wave each
static inline __host__ __device__ int mha_units_per_wg(int N) { return N <= 64 ? 4 : N <= 128 ? 2 : 1; }

// UDP_OP_MHATTN (udp_pose_hip.h).  Input pixel: q [0, dp), k [dp, 2 dp), v [2 dp, 3 dp) (dp = p.Cout), d = p.up_shift[0]
// real channels in each, heads = p.up_shift[1], hd = d / heads <= HDP (the instantiation's padded head width).
// A unit = (position class cls, head h) of one image; its N = HW / 4 queries and keys are the class's pixels in patch
// raster order.  A workgroup runs U = mha_units_per_wg(N) units with T = 256 / U threads each (whole waves) on one
// chunk of T queries: blockIdx.x = (unit group, query chunk), blockIdx.y = image.  thread = one query row: q and the
// accumulator in registers.  Keys are walked in blocks of kMhaKB, K and V rows staged in LDS as [key][HDP] fp32 (zeros
// past hd and past N) and read as broadcasts; inside a block, kMhaSub keys at a time:
//   s_j = fmaf chain over the head's channels in ascending order from 0;  m' = max(m, max_j s_j);
//   a = exp(m - m');  l = l a;  acc = acc a;  then for j ascending: e = exp(s_j - m'), l += e, acc = fmaf(e, v_j, acc)
// and out = acc / l at the end.  Keys past N are skipped (never exponentiated).  The order depends on (N, hd) only.
template <typename T, int HDP>
__global__ __launch_bounds__(kMhaThreads) void mhattn_kernel(const ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) float mha_s[];
  const int dp = p.Cout, d = p.up_shift[0], heads = p.up_shift[1], hd = d / heads;
  const int H = p.Hin, W = p.Win, HW = H * W, W2 = W >> 1, N = HW >> 2;
  const int U = mha_units_per_wg(N), TPU = kMhaThreads / U;
  const int ugroups = 4 * heads / U;
  const int ug = blockIdx.x % ugroups, chunk = blockIdx.x / ugroups;
  const int tid = threadIdx.x, ul = tid / TPU, t = tid % TPU;
  const int unit = ug * U + ul, cls = unit / heads, h = unit % heads;
  const size_t img = (size_t)blockIdx.y * HW;
  auto class_pixel = [&](int j) { return (2 * (j / W2) + (cls >> 1)) * W + 2 * (j % W2) + (cls & 1); };
  float* Ks = mha_s + (size_t)ul * (2 * kMhaKB * HDP);     // [kMhaKB][HDP]
  float* Vs = Ks + kMhaKB * HDP;
  const int i = chunk * TPU + t;
  const bool live = i < N;
  const size_t qpix = img + class_pixel(live ? i : 0);
  const int ch0 = h * hd;

  float q[HDP], acc[HDP];
#pragma unroll
  for (int c = 0; c < HDP; ++c) {
    q[c] = live && c < hd ? attn_load1<T>(p, qpix, ch0 + c) : 0.f;
    acc[c] = 0.f;
  }
  float m = -INFINITY, l = 0.f;

  for (int j0 = 0; j0 < N; j0 += kMhaKB) {
    __syncthreads();                                         // the previous block has been read
    for (int e = t; e < kMhaKB * HDP; e += TPU) {
      const int j = e / HDP, c = e % HDP;
      float kv = 0.f, vv = 0.f;
      if (j0 + j < N && c < hd) {
        const size_t px = img + class_pixel(j0 + j);
        kv = attn_load1<T>(p, px, dp + ch0 + c);
        vv = attn_load1<T>(p, px, 2 * dp + ch0 + c);
      }
      Ks[e] = kv;
      Vs[e] = vv;
    }
    __syncthreads();
    for (int js = 0; js < kMhaKB && j0 + js < N; js += kMhaSub) {
      float s[kMhaSub];
      float mb = m;
#pragma unroll
      for (int jj = 0; jj < kMhaSub; ++jj) {
        const f32x4* kr = reinterpret_cast<const f32x4*>(Ks + (js + jj) * HDP);
        float a = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < HDP / 4; ++c4) {
          const f32x4 k4 = kr[c4];
          a = __builtin_fmaf(q[4 * c4], k4[0], a);
          a = __builtin_fmaf(q[4 * c4 + 1], k4[1], a);
          a = __builtin_fmaf(q[4 * c4 + 2], k4[2], a);
          a = __builtin_fmaf(q[4 * c4 + 3], k4[3], a);
        }
        s[jj] = a;
        if (j0 + js + jj < N) mb = __builtin_fmaxf(mb, a);
      }
      const float alpha = expf(m - mb);                     // first block: exp(-inf) = 0 on l = 0, acc = 0
      m = mb;
      l *= alpha;
#pragma unroll
      for (int c = 0; c < HDP; ++c) acc[c] *= alpha;
#pragma unroll
      for (int jj = 0; jj < kMhaSub; ++jj) {
        if (j0 + js + jj < N) {
          const float e = expf(s[jj] - m);
          l += e;
          const f32x4* vr = reinterpret_cast<const f32x4*>(Vs + (js + jj) * HDP);
#pragma unroll
          for (int c4 = 0; c4 < HDP / 4; ++c4) {
            const f32x4 v4 = vr[c4];
            acc[4 * c4] = __builtin_fmaf(e, v4[0], acc[4 * c4]);
            acc[4 * c4 + 1] = __builtin_fmaf(e, v4[1], acc[4 * c4 + 1]);
            acc[4 * c4 + 2] = __builtin_fmaf(e, v4[2], acc[4 * c4 + 2]);
            acc[4 * c4 + 3] = __builtin_fmaf(e, v4[3], acc[4 * c4 + 3]);
          }
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < HDP; ++c)
    if (c < hd) attn_store1<T>(p, qpix, ch0 + c, acc[c] / l);
  if (h == heads - 1)                                        // the pad channels of the pixel: exact zeros
    for (int c = d; c < dp; ++c) attn_store1<T>(p, qpix, c, 0.f);
}

// ---------------------------------------------------------------------------------------------- host side
// Shape / field rules of the two kinds (udp_pose_hip.h), shared by udp_hrnet_create and udp_conv2d_fused.
int gnorm_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "group norm: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "group norm: dtype %d", dtype);
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cin > 512 || o.cout_pad != o.cout || o.chain_cout < 1 || o.chain_cout > o.cin ||
      o.hin < 1 || o.win < 1 || o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "group norm: cin == cout == cout_pad, a multiple of 32 up to 512, real channels (chain_cout) 1 .. cin, "
                "output = input size (C%d->%d, real %d)", o.cin, o.cout, o.chain_cout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "group norm: channel views");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "group norm: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "group norm: no addends, activation, second outputs, groups or NCHW output");
  return UDP_OK;
}

int linattn_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "linear attention: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "linear attention: dtype %d", dtype);
  if (o.ks != 2) return fail(UDP_ERR_ARG, "linear attention: ks %d (the patch size; 2 x 2 patches only)", o.ks);
  if (o.cout <= 0 || o.cout % 32 || o.cout > 512 || o.cout_pad != o.cout || o.cin != 2 * o.cout + 32)
    return fail(UDP_ERR_ARG, "linear attention: cout == cout_pad = C, a multiple of 32 up to 512, cin = 2C + 32 (C%d->%d)", o.cin, o.cout);
  if (o.hin < 2 || o.win < 2 || (o.hin & 1) || (o.win & 1) || o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "linear attention: %dx%d -> %dx%d (even sizes, output = input size)", o.hin, o.win, o.hout, o.wout);
  if ((long)o.hin * o.win > 16384) return fail(UDP_ERR_UNSUPPORTED, "linear attention: %dx%d pixels; the query of at most 16384 is staged in LDS", o.hin, o.win);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "linear attention: channel views");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "linear attention: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.chain_cout || o.group || o.in_stuff2 || o.wfmt || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "linear attention: no addends, activation, second outputs, chain, groups or NCHW output");
  return UDP_OK;
}

// p: geometry, views, in / out, wgt = the parameter block, up_shift[0] = real channels.  One workgroup per image.
int describe_gnorm(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "group norm: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt) return fail(UDP_ERR_ARG, "group norm: null pointer");
  const int r = p.up_shift[0];
  if (p.Cin <= 0 || p.Cin % 32 || p.Cin > 512 || r < 1 || r > p.Cin || p.N <= 0 || p.relu) return fail(UDP_ERR_ARG, "group norm: C %d, real %d", p.Cin, r);
  out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&gnorm_kernel<float>) : reinterpret_cast<const void*>(&gnorm_kernel<H2>);
  out->grid = dim3((unsigned)p.N);
  out->block = dim3(kAttnThreads);
  out->lds = 0;
  out->p = p;
  return UDP_OK;
}

// p: geometry (Cout = C), views, in / out.  One workgroup per image.
int describe_linattn(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "linear attention: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || p.in == p.out) return fail(UDP_ERR_ARG, "linear attention: null pointer, or out == in");
  const int V = dtype == UDP_F32 ? 4 : 8, C = p.Cout;
  const long HW = (long)p.Hin * p.Win;
  if (C <= 0 || C % 32 || C > 512 || p.Cin != 2 * C + 32 || (p.Hin & 1) || (p.Win & 1) || HW < 4 || HW > 16384 || p.N <= 0 || p.relu)
    return fail(UDP_ERR_ARG, "linear attention: C %d, %dx%d", C, p.Hin, p.Win);
  const int SG = (kAttnThreads / (C / V)) / 4;
  const size_t lds = ((size_t)HW + (size_t)4 * SG * C + (size_t)4 * C) * sizeof(float);       // <= 64 K + 32 K + 8 K
  const void* kern = dtype == UDP_F32 ? reinterpret_cast<const void*>(&linattn_kernel<float>) : reinterpret_cast<const void*>(&linattn_kernel<H2>);
  static bool attr_set[2] = {false, false};
  if (!attr_set[dtype == UDP_F32]) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 112 * 1024));
    attr_set[dtype == UDP_F32] = true;
  }
  out->fn = kern;
  out->grid = dim3((unsigned)p.N);
  out->block = dim3(kAttnThreads);
  out->lds = (unsigned)lds;
  out->p = p;
  return UDP_OK;
}

// Field rules the three MobileViT kinds share: storage mode, views, and what they refuse.
static int vit_common_validate(const udp_conv_op& o, int dtype, const char* what) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "%s: storage modes f32 and f16x2 only", what);
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "%s: dtype %d", what, dtype);
  if (o.hin < 1 || o.win < 1 || o.hout != o.hin || o.wout != o.win || o.cin <= 0 || o.cout <= 0)
    return fail(UDP_ERR_ARG, "%s: %dx%d -> %dx%d (output = input size)", what, o.hin, o.win, o.hout, o.wout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "%s: channel views", what);
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "%s: no addends, second outputs, groups, wfmt or NCHW output", what);
  return UDP_OK;
}

int lnorm_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "layer norm: storage modes f32 and f16x2 only");
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cin > 512 || o.cout_pad != o.cout || o.chain_cout < 1 || o.chain_cout > o.cin)
    return fail(UDP_ERR_ARG, "layer norm: cin == cout == cout_pad, a multiple of 32 up to 512, real channels (chain_cout) 1 .. cin "
                "(C%d->%d, real %d)", o.cin, o.cout, o.chain_cout);
  if (const int rc = vit_common_validate(o, dtype, "layer norm")) return rc;
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "layer norm: activation code %d", o.relu);
  if (o.relu) return fail(UDP_ERR_UNSUPPORTED, "layer norm: no activation");
  return UDP_OK;
}

int mhattn_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "multi-head attention: storage modes f32 and f16x2 only");
  if (o.ks != 2) return fail(UDP_ERR_ARG, "multi-head attention: ks %d (the patch size; 2 x 2 patches only)", o.ks);
  if (o.cout <= 0 || o.cout % 32 || o.cout > 256 || o.cout_pad != o.cout || o.cin != 3 * o.cout)
    return fail(UDP_ERR_ARG, "multi-head attention: cout == cout_pad = dp, a multiple of 32 up to 256, cin = 3 dp (C%d->%d)", o.cin, o.cout);
  const int d = o.chain_cout, heads = o.up_shift[0];
  if (d < 1 || d > o.cout || heads < 1 || d % heads || d / heads > 64)
    return fail(UDP_ERR_ARG, "multi-head attention: real width (chain_cout) %d of %d, %d heads (up_shift[0]): d %% heads == 0, head width <= 64",
                d, o.cout, heads);
  if (o.hin < 2 || o.win < 2 || (o.hin & 1) || (o.win & 1))
    return fail(UDP_ERR_ARG, "multi-head attention: a %dx%d map (even sizes)", o.hin, o.win);
  if ((long)o.hin * o.win > (1L << 20)) return fail(UDP_ERR_UNSUPPORTED, "multi-head attention: %dx%d pixels (at most 2^20)", o.hin, o.win);
  if (o.n_up) return fail(UDP_ERR_UNSUPPORTED, "multi-head attention: no addends (up_shift[0] carries the head count with n_up == 0)");
  if (const int rc = vit_common_validate(o, dtype, "multi-head attention")) return rc;
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "multi-head attention: activation code %d", o.relu);
  if (o.relu) return fail(UDP_ERR_UNSUPPORTED, "multi-head attention: no activation");
  return UDP_OK;
}

int act_op_validate(const udp_conv_op& o, int dtype) {
  if (o.relu != UDP_ACT_HSWISH && o.relu != UDP_ACT_SILU)
    return fail(UDP_ERR_ARG, "activation op: code %d (2 hard-swish or 4 SiLU; a ReLU rides in its producer's epilogue)", o.relu);
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "activation op: storage modes f32 and f16x2 only");
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cout_pad != o.cout)
    return fail(UDP_ERR_ARG, "activation op: cin == cout == cout_pad, a multiple of 32 (C%d->%d)", o.cin, o.cout);
  if (const int rc = vit_common_validate(o, dtype, "activation op")) return rc;
  if (o.chain_cout) return fail(UDP_ERR_UNSUPPORTED, "activation op: no chain");
  return UDP_OK;
}

// p: geometry, views, in / out, wgt = the parameter block, up_shift[0] = real channels.  16 pixels per workgroup.
int describe_lnorm(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "layer norm: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt) return fail(UDP_ERR_ARG, "layer norm: null pointer");
  const int r = p.up_shift[0];
  const long npix = (long)p.N * p.Hin * p.Win;
  if (p.Cin <= 0 || p.Cin % 32 || p.Cin > 512 || r < 1 || r > p.Cin || p.N <= 0 || p.relu || npix > (1L << 30))
    return fail(UDP_ERR_ARG, "layer norm: C %d, real %d, %ld pixels", p.Cin, r, npix);
  out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&lnorm_kernel<float>) : reinterpret_cast<const void*>(&lnorm_kernel<H2>);
  out->grid = dim3((unsigned)((npix + kLnThreads / kLnLanes - 1) / (kLnThreads / kLnLanes)));
  out->block = dim3(kLnThreads);
  out->lds = 0;
  out->p = p;
  return UDP_OK;
}

// p: geometry (Cin = C), views, in / out, relu = the activation code.  One thread per 16-byte channel group.
int describe_act(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "activation op: storage modes f32 and f16x2 only");
  if (!p.in || !p.out) return fail(UDP_ERR_ARG, "activation op: null pointer");
  if (p.relu != UDP_ACT_HSWISH && p.relu != UDP_ACT_SILU) return fail(UDP_ERR_ARG, "activation op: code %d", p.relu);
  const int V = dtype == UDP_F32 ? 4 : 8;
  const long groups = (long)p.N * p.Hin * p.Win * (p.Cin / V);
  if (p.Cin <= 0 || p.Cin % 32 || p.N <= 0 || groups > (1L << 31) * 255) return fail(UDP_ERR_ARG, "activation op: C %d", p.Cin);
  const bool s = p.relu == UDP_ACT_SILU;
  out->fn = dtype == UDP_F32 ? (s ? reinterpret_cast<const void*>(&act_kernel<float, UDP_ACT_SILU>) : reinterpret_cast<const void*>(&act_kernel<float, UDP_ACT_HSWISH>))
                             : (s ? reinterpret_cast<const void*>(&act_kernel<H2, UDP_ACT_SILU>) : reinterpret_cast<const void*>(&act_kernel<H2, UDP_ACT_HSWISH>));
  out->grid = dim3((unsigned)((groups + 255) / 256));
  out->block = dim3(256);
  out->lds = 0;
  p.relu = 0;                                               // the code is the kernel's template argument
  out->p = p;
  return UDP_OK;
}

template <typename T, int HDP>
static int describe_mha_one(const ConvParams& p, unsigned grid_x, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&mhattn_kernel<T, HDP>);
  if (!attr_set) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    attr_set = true;
  }
  out->fn = kern;
  out->grid = dim3(grid_x, (unsigned)p.N);
  out->block = dim3(kMhaThreads);
  out->lds = (unsigned)lds;
  out->p = p;
  return UDP_OK;
}

// p: geometry (Cout = dp), views, in / out, up_shift[0] = real width d, up_shift[1] = heads.
int describe_mhattn(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "multi-head attention: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || p.in == p.out) return fail(UDP_ERR_ARG, "multi-head attention: null pointer, or out == in");
  const int dp = p.Cout, d = p.up_shift[0], heads = p.up_shift[1];
  const long HW = (long)p.Hin * p.Win;
  if (dp <= 0 || dp % 32 || dp > 256 || p.Cin != 3 * dp || d < 1 || d > dp || heads < 1 || d % heads || d / heads > 64 || (p.Hin & 1) || (p.Win & 1) ||
      HW < 4 || HW > (1L << 20) || p.N <= 0 || p.N > 65535 || p.relu)
    return fail(UDP_ERR_ARG, "multi-head attention: dp %d, d %d, %d heads, %dx%d, n %d", dp, d, heads, p.Hin, p.Win, p.N);
  const int hd = d / heads, N = (int)(HW / 4);
  const int U = mha_units_per_wg(N), TPU = kMhaThreads / U;
  const int hdp = (hd + 15) / 16 * 16;
  const unsigned grid_x = (unsigned)(4 * heads / U) * (unsigned)((N + TPU - 1) / TPU);       // (4 heads is a multiple of U <= 4)
  const size_t lds = (size_t)U * 2 * kMhaKB * hdp * sizeof(float);                            // <= 64 KB
  const bool f = dtype == UDP_F32;
  switch (hdp) {
    case 16: return f ? describe_mha_one<float, 16>(p, grid_x, lds, out) : describe_mha_one<H2, 16>(p, grid_x, lds, out);
    case 32: return f ? describe_mha_one<float, 32>(p, grid_x, lds, out) : describe_mha_one<H2, 32>(p, grid_x, lds, out);
    case 48: return f ? describe_mha_one<float, 48>(p, grid_x, lds, out) : describe_mha_one<H2, 48>(p, grid_x, lds, out);
    default: return f ? describe_mha_one<float, 64>(p, grid_x, lds, out) : describe_mha_one<H2, 64>(p, grid_x, lds, out);
  }
}

int attn_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
