// Training kernels of pose_mobilevitv2_pixel_shuffle (deep_hrnet/lib/models/backbones/mobilevitv2.py) for gfx950 that the
// MobileNetV3 step (dw_train.hip, shufflenet_train.hip, mobilenetv3_train.hip) does not have:
//
//   udp_silu_fwd / _bwd            nn.SiLU (:78-79) and its derivative
//   udp_gnorm_train_fwd / _bwd     GroupNorm(1, C), "layer_norm_2d" (:139-140), in train mode
//   udp_linattn_train_fwd / _bwd   the separable self-attention core, LinearSelfAttention._forward_self_attn (:671-689)
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4.  Every kernel writes EVERY stored channel of
// its outputs (padded channels: exact zeros), there are no atomics, and every sum has one order that depends on the shape
// alone.  Dot products are explicit fmaf (the file is compiled without fp contraction, like dw_train.hip).
#include "common.h"

namespace udp {

// one fixed butterfly: every lane ends with the same sum, the order depends on nothing but the lane count
__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
  return a;
}
__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
  return a;
}
__device__ __forceinline__ float wave_max(float a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a = fmaxf(a, __shfl_xor(a, m, 64));
  return a;
}
// sum over the 256 threads of a workgroup: butterfly per wave, the four waves in index order.  red: 4 values of LDS.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------------------------------------
// SiLU.  y = x * (1 / (1 + exp(-x))) -- the arithmetic of UDP_ACT_SILU and of tests/mobilevitv2_ref.silu;
// dx = dy * s * (1 + x * (1 - s)), s = 1 / (1 + exp(-x)).  exp(-x) = +inf for x < -88.7: s = 0, y = -0, dx = 0; exp(-x) = 0
// for x > 88.7 (or a denormal the hardware flushes): s = 1, y = x, dx = dy.  Nothing is NaN for finite x.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

__global__ __launch_bounds__(256) void silu_fwd_kernel(const float* __restrict__ x, long total4, float* __restrict__ y) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e] * sigm(v[e]);
    *reinterpret_cast<f32x4*>(y + i * 4) = o;
  }
}

__global__ __launch_bounds__(256) void silu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, long total4,
                                                      float* __restrict__ dx) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + i * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = sigm(v[e]);
      o[e] = d[e] * s * (1.f + v[e] * (1.f - s));
    }
    *reinterpret_cast<f32x4*>(dx + i * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// GroupNorm(1, C), train mode.  An image's h*w pixels are cut into `split` runs of `ppw` consecutive pixels (gn_split: a
// pure function of h, w and the stored channel count); workgroup (run, image).  Statistics are SHIFTED sums in fp64,
// sum(x - x0) and sum((x - x0)^2) with x0 = the image's first element, over the c_real real channels only: a map whose
// mean is 1000 x its standard deviation keeps its variance (the shift removes the mean's magnitude, fp64 the rest).
// The runs' partial sums land in the workspace and every reader adds them in index order.
// ---------------------------------------------------------------------------------------------
constexpr int kGnGroupsPerWg = 1024;     // 16-byte channel groups a workgroup takes at least (4 per thread)
constexpr int kGnMaxSplit = 64;

static void gn_split(int h, int w, int ck, int* ppw, int* split) {
  const long P = (long)h * w;
  long per = (kGnGroupsPerWg + ck / 4 - 1) / (ck / 4);
  if (per < 1) per = 1;
  long s = (P + per - 1) / per;
  if (s > kGnMaxSplit) {
    per = (P + kGnMaxSplit - 1) / kGnMaxSplit;
    s = (P + per - 1) / per;
  }
  *ppw = (int)per, *split = (int)s;
}

// part[n][run][2] (fp64) = sum(x - x0), sum((x - x0)^2) over the run's real elements
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, int HW, int C, int Creal, int ppw,
                                                      double* __restrict__ part) {
  __shared__ double red[4];
  const int n = blockIdx.y, run = blockIdx.x, C4 = C >> 2;
  const float* xi = x + (size_t)n * HW * C;
  const float x0 = xi[0];
  const int p0 = run * ppw, p1 = min(HW, p0 + ppw);
  const long lo = (long)p0 * C4, hi = (long)p1 * C4;
  double s1 = 0.0, s2 = 0.0;
  for (long g = lo + threadIdx.x; g < hi; g += 256) {
    const int c = (int)(g % C4) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(xi + g * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e < Creal) {
        const double d = (double)(v[e] - x0);
        s1 += d;
        s2 = __builtin_fma(d, d, s2);
      }
    }
  }
  s1 = block_sum(s1, red);
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    part[((size_t)n * gridDim.x + run) * 2] = s1;
    part[((size_t)n * gridDim.x + run) * 2 + 1] = s2;
  }
}

// y = (x - mu) * r * gamma + beta on the real channels, 0 on the pads; run 0 leaves (mu, r) in save[n]
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const double* __restrict__ part, int HW, int C,
                                                      int Creal, int ppw, float eps, float* __restrict__ y, float* __restrict__ save) {
  const int n = blockIdx.y, run = blockIdx.x, C4 = C >> 2;
  const float* xi = x + (size_t)n * HW * C;
  float* yi = y + (size_t)n * HW * C;
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < (int)gridDim.x; ++k) {
    s1 += part[((size_t)n * gridDim.x + k) * 2];
    s2 += part[((size_t)n * gridDim.x + k) * 2 + 1];
  }
  const double cnt = (double)HW * Creal;
  const double m = s1 / cnt;
  double var = s2 / cnt - m * m;
  if (var < 0.0) var = 0.0;
  const float mu = (float)((double)xi[0] + m);
  const float r = (float)(1.0 / sqrt(var + (double)eps));
  if (run == 0 && threadIdx.x == 0) {
    save[2 * n] = mu;
    save[2 * n + 1] = r;
  }
  const int p0 = run * ppw, p1 = min(HW, p0 + ppw);
  const long lo = (long)p0 * C4, hi = (long)p1 * C4;
  for (long g = lo + threadIdx.x; g < hi; g += 256) {
    const int c = (int)(g % C4) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(xi + g * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = c + e < Creal ? __builtin_fmaf((v[e] - mu) * r, gamma[c + e], beta[c + e]) : 0.f;
    *reinterpret_cast<f32x4*>(yi + g * 4) = o;
  }
}

// Backward, pass 1.  Workgroup (run, image): cgw channel-group lanes x 256 / cgw pixel lanes; pixel lane l takes the
// run's pixels l, l + PL, ... in order.  Leaves
//   part[n][run][2] (fp64)  = sum(g^), sum(g^ x^)  over the run's real elements (g^ = dy gamma, x^ = (x - mu) r)
//   cpart[n][run][2][C]     = per channel sum(dy x^), sum(dy)  over the run's pixels, pixel lanes combined in lane order
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ save, int HW,
                                                           int C, int Creal, int ppw, int cgw, int cgw_shift,
                                                           double* __restrict__ part, float* __restrict__ cpart) {
  __shared__ float sAcc[256 * 8];
  __shared__ double red[4];
  const int n = blockIdx.y, run = blockIdx.x, C4 = C >> 2, t = threadIdx.x;
  const int lc = t & (cgw - 1), lp = t >> cgw_shift, PL = 256 >> cgw_shift;
  const float mu = save[2 * n], r = save[2 * n + 1];
  const int p0 = run * ppw, p1 = min(HW, p0 + ppw);
  const size_t img = (size_t)n * HW * C;
  float* cp = cpart + ((size_t)n * gridDim.x + run) * 2 * C;
  double a1 = 0.0, a2 = 0.0;
  for (int cb = 0; cb * cgw < C4; ++cb) {
    const int cg = cb * cgw + lc;
    f32x4 dg = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
    if (cg < C4) {
      f32x4 gm;
#pragma unroll
      for (int e = 0; e < 4; ++e) gm[e] = cg * 4 + e < Creal ? gamma[cg * 4 + e] : 0.f;
      for (int q = p0 + lp; q < p1; q += PL) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + img + (size_t)q * C + cg * 4);
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + img + (size_t)q * C + cg * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (cg * 4 + e < Creal) {
            const float xh = (v[e] - mu) * r;
            dg[e] = __builtin_fmaf(d[e], xh, dg[e]);
            db[e] += d[e];
            const double gh = (double)(d[e] * gm[e]);
            a1 += gh;
            a2 = __builtin_fma(gh, (double)xh, a2);
          }
        }
      }
    }
    const int span = cgw * 4;
    __syncthreads();
    *reinterpret_cast<f32x4*>(sAcc + (lp * span + lc * 4) * 2) = dg;
    *reinterpret_cast<f32x4*>(sAcc + (lp * span + lc * 4) * 2 + 4) = db;
    __syncthreads();
    for (int o = t; o < span; o += 256) {
      const int ch = cb * span + o;
      if (ch >= C) continue;
      const int base = ((o >> 2) * 4) * 2 + (o & 3);
      float vg = sAcc[base], vb = sAcc[base + 4];
      for (int l = 1; l < PL; ++l) {
        vg += sAcc[l * span * 2 + base];
        vb += sAcc[l * span * 2 + base + 4];
      }
      cp[ch] = vg;
      cp[C + ch] = vb;
    }
  }
  a1 = block_sum(a1, red);
  a2 = block_sum(a2, red);
  if (t == 0) {
    part[((size_t)n * gridDim.x + run) * 2] = a1;
    part[((size_t)n * gridDim.x + run) * 2 + 1] = a2;
  }
}

// Backward, pass 2: dx (+)= r (g^ - mean(g^) - x^ mean(g^ x^)) on the real channels, 0 on the pads
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ save,
                                                          const double* __restrict__ part, int HW, int C, int Creal, int ppw,
                                                          int accumulate, float* __restrict__ dx) {
  const int n = blockIdx.y, run = blockIdx.x, C4 = C >> 2;
  const size_t img = (size_t)n * HW * C;
  double a1 = 0.0, a2 = 0.0;
  for (int k = 0; k < (int)gridDim.x; ++k) {
    a1 += part[((size_t)n * gridDim.x + k) * 2];
    a2 += part[((size_t)n * gridDim.x + k) * 2 + 1];
  }
  const double cnt = (double)HW * Creal;
  const float m1 = (float)(a1 / cnt), m2 = (float)(a2 / cnt);
  const float mu = save[2 * n], r = save[2 * n + 1];
  const int p0 = run * ppw, p1 = min(HW, p0 + ppw);
  const long lo = (long)p0 * C4, hi = (long)p1 * C4;
  for (long g = lo + threadIdx.x; g < hi; g += 256) {
    const int c = (int)(g % C4) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + img + g * 4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + img + g * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (c + e < Creal) {
        const float xh = (v[e] - mu) * r;
        o[e] = r * ((d[e] * gamma[c + e] - m1) - xh * m2);
      } else {
        o[e] = 0.f;
      }
    }
    if (accumulate) {
      const f32x4 old = *reinterpret_cast<const f32x4*>(dx + img + g * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = old[e] + o[e];
    }
    *reinterpret_cast<f32x4*>(dx + img + g * 4) = o;
  }
}

// Backward, pass 3: dgamma[c] / dbeta[c] = the (image, run) partials added in index order, c < c_real
__global__ __launch_bounds__(256) void gn_param_grad_kernel(const float* __restrict__ cpart, int rows, int C, int Creal,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * Creal) return;
  const int which = i >= Creal, c = i - which * Creal;
  float a = 0.f;
  for (int k = 0; k < rows; ++k) a += cpart[((size_t)k * 2 + which) * C + c];
  (which ? dbeta : dgamma)[c] = a;
}

static int gn_check(const char* who, int n, int h, int w, int ck, int c_real, int dtype) {
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (n <= 0 || h <= 0 || w <= 0 || ck <= 0 || (ck & 3) || c_real <= 0 || c_real > ck)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, ck %d (ck %% 4), c_real %d (1..ck)", who, h, w, n, ck, c_real);
  if ((long)h * w * (ck / 4) >= (1L << 31) || n > 65535 || (long)n * h * w * ck >= (1L << 40))
    return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d x%d ck %d is too large", who, h, w, n, ck);
  return UDP_OK;
}

static size_t gn_workspace(int n, int split, int ck) { return (size_t)n * split * (2 * sizeof(double) + 2 * (size_t)ck * sizeof(float)); }

// channel-group lanes of gn_bwd_reduce_kernel: the power of two in 8..64 that covers ck / 4
static void gn_lanes(int ck, int* cgw, int* shift) {
  const int C4 = ck >> 2;
  int g = 8, sh = 3;
  while (g < 64 && g < C4) g *= 2, ++sh;
  *cgw = g, *shift = sh;
}

// ---------------------------------------------------------------------------------------------
// Separable self-attention core.  Workgroup (class, image); class = (y & 1) * 2 + (x & 1), its M = h w / 4 pixels in
// row-major order of the (h / 2, w / 2) grid.  qkv channels: 0 the query, 1..d the keys, d+1..2d the values (the
// parameter's own order), so the key / value rows are 4-byte aligned only and are read with scalar loads, consecutive
// lanes on consecutive channels.
// ---------------------------------------------------------------------------------------------
constexpr int kLaMaxM = 2048, kLaMaxD = 512;

__device__ __forceinline__ size_t la_pixel(int i, int cls, int w2, int W) {
  const int yy = i / w2, xx = i - yy * w2;
  return (size_t)(2 * yy + (cls >> 1)) * W + (2 * xx + (cls & 1));
}

__global__ __launch_bounds__(256) void linattn_fwd_kernel(const float* __restrict__ qkv, int H, int W, int CQ, int d,
                                                         float* __restrict__ out, int CO, float* __restrict__ scores,
                                                         float* __restrict__ ctx) {
  __shared__ float sS[kLaMaxM];
  __shared__ float sCtx[kLaMaxD];
  __shared__ float sPart[4 * kLaMaxD];
  __shared__ float red[4];
  const int cls = blockIdx.x, n = blockIdx.y, t = threadIdx.x, w2 = W >> 1, M = (H >> 1) * w2;
  const float* base = qkv + (size_t)n * H * W * CQ;
  float* ob = out + (size_t)n * H * W * CO;
  // soft-max of the queries, the maximum subtracted
  float mx = -INFINITY;
  for (int i = t; i < M; i += 256) {
    const float q = base[la_pixel(i, cls, w2, W) * CQ];
    sS[i] = q;
    mx = fmaxf(mx, q);
  }
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int i = t; i < M; i += 256) {
    const float e = expf(sS[i] - mx);
    sS[i] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  float* sc = scores + ((size_t)n * 4 + cls) * M;
  for (int i = t; i < M; i += 256) {
    const float s = sS[i] / sum;
    sS[i] = s;
    sc[i] = s;
  }
  __syncthreads();
  // ctx[c] = sum_i s_i k_ic: wave l takes pixels l, l + 4, ... in order, the four waves are combined in index order
  const int wave = t >> 6, lane = t & 63;
  for (int c = lane; c < d; c += 64) {
    float a = 0.f;
    for (int i = wave; i < M; i += 4) a = __builtin_fmaf(sS[i], base[la_pixel(i, cls, w2, W) * CQ + 1 + c], a);
    sPart[wave * d + c] = a;
  }
  __syncthreads();
  for (int c = t; c < d; c += 256) {
    const float a = ((sPart[c] + sPart[d + c]) + sPart[2 * d + c]) + sPart[3 * d + c];
    sCtx[c] = a;
    ctx[((size_t)n * 4 + cls) * d + c] = a;
  }
  __syncthreads();
  // out = relu(v) * ctx, pads 0
  for (int idx = t; idx < M * CO; idx += 256) {
    const int i = idx / CO, c = idx - i * CO;
    const size_t p = la_pixel(i, cls, w2, W);
    ob[p * CO + c] = c < d ? fmaxf(base[p * CQ + 1 + d + c], 0.f) * sCtx[c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void linattn_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ qkv,
                                                         const float* __restrict__ scores, const float* __restrict__ ctx, int H, int W,
                                                         int CQ, int d, int CO, float* __restrict__ dqkv) {
  __shared__ float sS[kLaMaxM];
  __shared__ float sE[kLaMaxM];
  __shared__ float sCtx[kLaMaxD];
  __shared__ float sDctx[kLaMaxD];
  __shared__ float sPart[4 * kLaMaxD];
  __shared__ float red[4];
  const int cls = blockIdx.x, n = blockIdx.y, t = threadIdx.x, w2 = W >> 1, M = (H >> 1) * w2;
  const int wave = t >> 6, lane = t & 63;
  const float* base = qkv + (size_t)n * H * W * CQ;
  const float* gb = dout + (size_t)n * H * W * CO;
  float* db = dqkv + (size_t)n * H * W * CQ;
  for (int i = t; i < M; i += 256) sS[i] = scores[((size_t)n * 4 + cls) * M + i];
  for (int c = t; c < d; c += 256) sCtx[c] = ctx[((size_t)n * 4 + cls) * d + c];
  // dctx[c] = sum_i g_ic relu(v_ic): the forward's layout and order
  for (int c = lane; c < d; c += 64) {
    float a = 0.f;
    for (int i = wave; i < M; i += 4) {
      const size_t p = la_pixel(i, cls, w2, W);
      a = __builtin_fmaf(gb[p * CO + c], fmaxf(base[p * CQ + 1 + d + c], 0.f), a);
    }
    sPart[wave * d + c] = a;
  }
  __syncthreads();
  for (int c = t; c < d; c += 256) sDctx[c] = ((sPart[c] + sPart[d + c]) + sPart[2 * d + c]) + sPart[3 * d + c];
  __syncthreads();
  // e_i = sum_c k_ic dctx_c: a wave per pixel, lanes stride over the channels
  for (int i = wave; i < M; i += 4) {
    const size_t p = la_pixel(i, cls, w2, W);
    float a = 0.f;
    for (int c = lane; c < d; c += 64) a = __builtin_fmaf(base[p * CQ + 1 + c], sDctx[c], a);
    a = wave_sum(a);
    if (lane == 0) sE[i] = a;
  }
  __syncthreads();
  float se = 0.f;
  for (int i = t; i < M; i += 256) se = __builtin_fmaf(sS[i], sE[i], se);
  se = block_sum(se, red);
  // every stored channel of dqkv: dq | dk | dv | zeros
  for (int idx = t; idx < M * CQ; idx += 256) {
    const int i = idx / CQ, c = idx - i * CQ;
    const size_t p = la_pixel(i, cls, w2, W);
    float o;
    if (c == 0) {
      o = sS[i] * (sE[i] - se);
    } else if (c <= d) {
      o = sS[i] * sDctx[c - 1];
    } else if (c <= 2 * d) {
      o = base[p * CQ + c] > 0.f ? gb[p * CO + c - 1 - d] * sCtx[c - 1 - d] : 0.f;
    } else {
      o = 0.f;
    }
    db[p * CQ + c] = o;
  }
}

static int la_check(const char* who, int n, int h, int w, int ck_qkv, int d, int ck_out, int dtype) {
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (n <= 0 || h <= 0 || w <= 0 || d <= 0 || ck_out <= 0)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, d %d, ck_out %d (all > 0)", who, h, w, n, d, ck_out);
  if ((h & 1) || (w & 1)) return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d -- 2x2 patches need an even height and width", who, h, w);
  if (d % 16) return fail(UDP_ERR_UNSUPPORTED, "%s: d %d (d %% 16 == 0)", who, d);
  if (ck_qkv != (1 + 2 * d + 15) / 16 * 16)
    return fail(UDP_ERR_ARG, "%s: ck_qkv %d, ceil16(1 + 2 d) = %d expected", who, ck_qkv, (1 + 2 * d + 15) / 16 * 16);
  if (ck_out < d || ck_out > ck_qkv || (ck_out & 3))
    return fail(UDP_ERR_ARG, "%s: ck_out %d (d = %d <= ck_out <= ck_qkv, ck_out %% 4)", who, ck_out, d);
  if (d > kLaMaxD || (long)h * w / 4 > kLaMaxM || n > 65535 || (long)(h * w / 4) * ck_qkv >= (1L << 31))
    return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d x%d d %d is too large (d <= %d, h w / 4 <= %d)", who, h, w, n, d, kLaMaxD, kLaMaxM);
  return UDP_OK;
}

}  // namespace udp

using namespace udp;

static int silu_check(const char* who, const void* a, const void* b, const void* c, int64_t count) {
  if (!a || !b || !c) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (count <= 0 || (count & 3)) return fail(UDP_ERR_ARG, "%s: count %lld (a positive multiple of 4)", who, (long long)count);
  return UDP_OK;
}

extern "C" int udp_silu_fwd(const void* x, void* y, int64_t count, void* stream) {
  if (const int rc = silu_check("udp_silu_fwd", x, y, y, count)) return rc;
  silu_fwd_kernel<<<blocks_for(count / 4, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(x), count / 4, reinterpret_cast<float*>(y));
  return launched("udp_silu_fwd");
}

extern "C" int udp_silu_bwd(const void* dy, const void* x, void* dx, int64_t count, void* stream) {
  if (const int rc = silu_check("udp_silu_bwd", dy, x, dx, count)) return rc;
  silu_bwd_kernel<<<blocks_for(count / 4, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(dy), reinterpret_cast<const float*>(x), count / 4, reinterpret_cast<float*>(dx));
  return launched("udp_silu_bwd");
}

extern "C" int udp_gnorm_train_split(int h, int w, int ck) {
  if (h <= 0 || w <= 0 || ck <= 0 || (ck & 3)) return 0;
  int ppw, split;
  gn_split(h, w, ck, &ppw, &split);
  return split;
}

extern "C" size_t udp_gnorm_train_workspace_bytes(int n, int h, int w, int ck) {
  if (n <= 0 || h <= 0 || w <= 0 || ck <= 0 || (ck & 3)) return 0;
  int ppw, split;
  gn_split(h, w, ck, &ppw, &split);
  return gn_workspace(n, split, ck);
}

extern "C" int udp_gnorm_train_fwd(const void* x, const float* gamma, const float* beta, int n, int h, int w, int ck, int c_real,
                                   int dtype, float eps, void* y, float* save, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (!x || !gamma || !beta || !y || !save || !workspace) return fail(UDP_ERR_ARG, "udp_gnorm_train_fwd: null pointer");
  if (const int rc = gn_check("udp_gnorm_train_fwd", n, h, w, ck, c_real, dtype)) return rc;
  if (!(eps > 0.f)) return fail(UDP_ERR_ARG, "udp_gnorm_train_fwd: eps %g (> 0)", (double)eps);
  int ppw, split;
  gn_split(h, w, ck, &ppw, &split);
  const size_t need = gn_workspace(n, split, ck);
  if (workspace_bytes < need)
    return fail(UDP_ERR_WORKSPACE, "udp_gnorm_train_fwd: workspace %zu B, %zu B needed", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace);
  const float* xp = reinterpret_cast<const float*>(x);
  gn_stats_kernel<<<dim3(split, n), 256, 0, st>>>(xp, h * w, ck, c_real, ppw, part);
  gn_apply_kernel<<<dim3(split, n), 256, 0, st>>>(xp, gamma, beta, part, h * w, ck, c_real, ppw, eps, reinterpret_cast<float*>(y), save);
  return launched("udp_gnorm_train_fwd");
}

extern "C" int udp_gnorm_train_bwd(const void* dy, const void* x, const float* gamma, const float* save, int n, int h, int w,
                                   int ck, int c_real, int dtype, int accumulate, void* dx, float* dgamma, float* dbeta,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!dy || !x || !gamma || !save || !dx || !dgamma || !dbeta || !workspace)
    return fail(UDP_ERR_ARG, "udp_gnorm_train_bwd: null pointer");
  if (const int rc = gn_check("udp_gnorm_train_bwd", n, h, w, ck, c_real, dtype)) return rc;
  int ppw, split;
  gn_split(h, w, ck, &ppw, &split);
  const size_t need = gn_workspace(n, split, ck);
  if (workspace_bytes < need)
    return fail(UDP_ERR_WORKSPACE, "udp_gnorm_train_bwd: workspace %zu B, %zu B needed", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(workspace);                       // [n][split][2]
  float* cpart = reinterpret_cast<float*>(part + (size_t)n * split * 2);     // [n][split][2][ck]
  int cgw, shift;
  gn_lanes(ck, &cgw, &shift);
  const float *dyp = reinterpret_cast<const float*>(dy), *xp = reinterpret_cast<const float*>(x);
  gn_bwd_reduce_kernel<<<dim3(split, n), 256, 0, st>>>(dyp, xp, gamma, save, h * w, ck, c_real, ppw, cgw, shift, part, cpart);
  gn_bwd_apply_kernel<<<dim3(split, n), 256, 0, st>>>(dyp, xp, gamma, save, part, h * w, ck, c_real, ppw, accumulate != 0,
                                                      reinterpret_cast<float*>(dx));
  gn_param_grad_kernel<<<ceil_div(2 * c_real, 256), 256, 0, st>>>(cpart, n * split, ck, c_real, dgamma, dbeta);
  return launched("udp_gnorm_train_bwd");
}

extern "C" int udp_linattn_train_fwd(const void* qkv, int n, int h, int w, int ck_qkv, int d, int dtype, void* out, int ck_out,
                                     float* scores, float* ctx, void* stream) {
  if (!qkv || !out || !scores || !ctx) return fail(UDP_ERR_ARG, "udp_linattn_train_fwd: null pointer");
  if (const int rc = la_check("udp_linattn_train_fwd", n, h, w, ck_qkv, d, ck_out, dtype)) return rc;
  linattn_fwd_kernel<<<dim3(4, n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(qkv), h, w, ck_qkv, d, reinterpret_cast<float*>(out), ck_out, scores, ctx);
  return launched("udp_linattn_train_fwd");
}

extern "C" int udp_linattn_train_bwd(const void* dout, const void* qkv, const float* scores, const float* ctx, int n, int h, int w,
                                     int ck_qkv, int d, int ck_out, int dtype, void* dqkv, void* stream) {
  if (!dout || !qkv || !scores || !ctx || !dqkv) return fail(UDP_ERR_ARG, "udp_linattn_train_bwd: null pointer");
  if (const int rc = la_check("udp_linattn_train_bwd", n, h, w, ck_qkv, d, ck_out, dtype)) return rc;
  linattn_bwd_kernel<<<dim3(4, n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(dout), reinterpret_cast<const float*>(qkv), scores, ctx, h, w, ck_qkv, d, ck_out,
      reinterpret_cast<float*>(dqkv));
  return launched("udp_linattn_train_bwd");
}
