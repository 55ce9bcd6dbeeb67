// Polarized self-attention (PSA_s) of the fork's pose_hrnet_psa and pose_resnet_psa models on gfx950.
//
// Replaces PSA_s.forward, deep_hrnet/lib/models/PSA.py:190-269 (spatial_pool :190-222,
// channel_pool :224-258), inserted after relu(bn1(conv1)) of every BasicBlock
// (deep_hrnet/lib/models/pose_hrnet_psa.py:37,49).  Per image, on an NHWC map x [HW][C]:
//
//   spatial_pool: q = softmax_HW(wq . x_p);  ctx = Wv (sum_p q_p x_p)        (the C/2-channel
//                 conv_v_right never has to be materialised: Wv is linear)
//                 m = sigmoid(W2 relu(LN(W1 ctx + b1)) + b2);  x1 = x * m[c]
//   channel_pool: gbar = Wg mean_p(x1) = Wg (m * mean_p x);  theta = Wt x1_p (1x1 conv, MFMA kernel)
//                 s_p = sigmoid(sum_j gbar_j softmax_HW(theta_.j)_p);  x2 = x1 * s_p
//
// Four small HBM-bound kernels (one workgroup per image; the maps are re-read from L2) + the
// existing conv kernel for theta.  All reductions in fp32.  C divides 256 (the kernels below), or C = 512 (the
// *_wide kernels further down; SCALE is element-wise with the lanes along the channels and serves every width).
#include <type_traits>

#include "common.h"

namespace udp {

// Split-fp16 storage (UDP_F16X2, csrc/conv.hip): per pixel the C hi values, then the C lo values (fp16),
// x = hi + lo * 2^-11.
struct H2 {};
constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;

// channel c of pixel px of a [pixels][C] map stored as T
template <typename T>
__device__ __forceinline__ float ldx(const void* base, size_t px, int C, int c) {
  if constexpr (std::is_same<T, H2>::value) {
    const _Float16* q = reinterpret_cast<const _Float16*>(base) + px * 2 * C + c;
    return (float)q[0] + (float)q[C] * kLoInv;
  } else {
    return (float)reinterpret_cast<const T*>(base)[px * C + c];
  }
}
template <typename T>
__device__ __forceinline__ void stx(void* base, size_t px, int C, int c, float v) {
  if constexpr (std::is_same<T, H2>::value) {
    _Float16* q = reinterpret_cast<_Float16*>(base) + px * 2 * C + c;
    const _Float16 hi = (_Float16)v;
    h2_range_check(__builtin_fabsf(v));
    q[0] = hi;
    q[C] = (_Float16)((v - (float)hi) * kLoScale);
  } else {
    reinterpret_cast<T*>(base)[px * C + c] = (T)v;
  }
}

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_down(v, off);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
  return r;
}

// PSA fp32 parameter block: wq[C] | Wv[C/2][C] | W1[C/8][C/2] | b1[C/8] | ln_g[C/8] | ln_b[C/8] |
// W2[C][C/8] | b2[C] | Wg[C/2][C]
struct PsaW {
  const float *wq, *wv, *w1, *b1, *lg, *lb, *w2, *b2, *wg;
  __device__ PsaW(const float* p, int C) {
    wq = p;
    wv = wq + C;
    w1 = wv + (C / 2) * C;
    b1 = w1 + (C / 8) * (C / 2);
    lg = b1 + C / 8;
    lb = lg + C / 8;
    w2 = lb + C / 8;
    b2 = w2 + C * (C / 8);
    wg = b2 + C;
  }
};

// out[n] = { xbar[C] = sum_p softmax(q)_p x_p , xmean[C] }   (fp32)
template <typename T>
__global__ __launch_bounds__(256) void psa_pool_kernel(const ConvParams p) {
  extern __shared__ float sm[];   // e[HW] | part[256 * 2]
  __shared__ float red[4];
  const int C = p.Cin, HW = p.Hin * p.Win;
  const int n = blockIdx.x;
  const size_t px0 = (size_t)n * HW;
  const PsaW w(reinterpret_cast<const float*>(p.wgt), C);
  float* e = sm;
  float* part = sm + HW;
  float lmax = -INFINITY;
  for (int px = threadIdx.x; px < HW; px += 256) {
    float q = 0.f;
    for (int c = 0; c < C; ++c) q = fmaf(ldx<T>(p.in, px0 + px, C, c), w.wq[c], q);
    e[px] = q;
    lmax = fmaxf(lmax, q);
  }
  const float gmax = block_reduce(lmax, true, red);
  float lsum = 0.f;
  for (int px = threadIdx.x; px < HW; px += 256) {
    const float v = expf(e[px] - gmax);
    e[px] = v;
    lsum += v;
  }
  const float gsum = block_reduce(lsum, false, red);
  // channel c = tid % C, pixel group = tid / C (256 % C == 0)
  const int c = threadIdx.x % C, grp = threadIdx.x / C, ngrp = 256 / C;
  float a = 0.f, m = 0.f;
  for (int px = grp; px < HW; px += ngrp) {
    const float v = ldx<T>(p.in, px0 + px, C, c);
    a = fmaf(e[px], v, a);
    m += v;
  }
  part[threadIdx.x] = a;
  part[256 + threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x < C) {
    float sa = 0.f, smn = 0.f;
    for (int g = 0; g < ngrp; ++g) {
      sa += part[g * C + threadIdx.x];
      smn += part[256 + g * C + threadIdx.x];
    }
    float* o = reinterpret_cast<float*>(p.out) + (size_t)n * 2 * C;
    o[threadIdx.x] = sa / gsum;
    o[C + threadIdx.x] = smn / (float)HW;
  }
}

// out[n] = { m[C] = sigmoid(W2 relu(LN(W1 Wv xbar + b1)) + b2) , gbar[C/2] = Wg (m * xmean) }
__global__ __launch_bounds__(256) void psa_mlp_kernel(const ConvParams p) {
  __shared__ float xb[256], xm[256], ctx[128], h[32], msk[256];
  __shared__ float stat[2];
  const int C = p.Cin, C2 = C / 2, C8 = C / 8;
  const int n = blockIdx.x, t = threadIdx.x;
  const PsaW w(reinterpret_cast<const float*>(p.wgt), C);
  const float* s = reinterpret_cast<const float*>(p.in) + (size_t)n * 2 * C;
  if (t < C) {
    xb[t] = s[t];
    xm[t] = s[C + t];
  }
  __syncthreads();
  if (t < C2) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(w.wv[t * C + c], xb[c], a);
    ctx[t] = a;
  }
  __syncthreads();
  if (t < C8) {
    float a = w.b1[t];
    for (int j = 0; j < C2; ++j) a = fmaf(w.w1[t * C2 + j], ctx[j], a);
    h[t] = a;
  }
  __syncthreads();
  if (t == 0) {
    float mu = 0.f;
    for (int k = 0; k < C8; ++k) mu += h[k];
    mu /= (float)C8;
    float var = 0.f;
    for (int k = 0; k < C8; ++k) var += (h[k] - mu) * (h[k] - mu);
    stat[0] = mu;
    stat[1] = rsqrtf(var / (float)C8 + 1e-5f);
  }
  __syncthreads();
  if (t < C8) h[t] = fmaxf((h[t] - stat[0]) * stat[1] * w.lg[t] + w.lb[t], 0.f);
  __syncthreads();
  float* o = reinterpret_cast<float*>(p.out) + (size_t)n * (C + C2);
  if (t < C) {
    float a = w.b2[t];
    for (int k = 0; k < C8; ++k) a = fmaf(w.w2[t * C8 + k], h[k], a);
    const float m = 1.f / (1.f + expf(-a));
    msk[t] = m * xm[t];
    o[t] = m;
  }
  __syncthreads();
  if (t < C2) {
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(w.wg[t * C + c], msk[c], a);
    o[C + t] = a;
  }
}

// out[n,p,c] = in[n,p,c] * mask[n][c]     (mask: fp32 rows of `res`, pitch = res_pitch floats)
template <typename T>
__global__ __launch_bounds__(256) void psa_scale_kernel(const ConvParams p) {
  const int C = p.Cin, HW = p.Hin * p.Win;
  const long total = (long)p.N * HW * C;
  const float* mask = reinterpret_cast<const float*>(p.res);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = i % C;
    const long n = i / ((long)HW * C);
    const size_t px = (size_t)(i / C);
    stx<T>(p.out, px, C, c, ldx<T>(p.in, px, C, c) * mask[n * p.res_pitch + c]);
  }
}

// in = theta [N][HW][C/2], res = x1 [N][HW][C], up[0] = {m, gbar} fp32 rows; out = x1 * sigmoid(ctx_p)
template <typename T>
__global__ __launch_bounds__(256) void psa_sp_kernel(const ConvParams p) {
  extern __shared__ float sm[];   // msp[HW] | part[256] | M[C2] | S[C2] | g[C2]
  const int C = p.Cout, C2 = p.Cin, HW = p.Hin * p.Win;
  const int n = blockIdx.x, t = threadIdx.x;
  const size_t px0 = (size_t)n * HW;
  float* msp = sm;
  float* part = sm + HW;
  float* M = part + 256;
  float* S = M + C2;
  float* g = S + C2;
  const int j = t % C2, grp = t / C2, ngrp = 256 / C2;
  float lm = -INFINITY;
  for (int px = grp; px < HW; px += ngrp) lm = fmaxf(lm, ldx<T>(p.in, px0 + px, C2, j));
  part[t] = lm;
  __syncthreads();
  if (t < C2) {
    float m = part[t];
    for (int k = 1; k < ngrp; ++k) m = fmaxf(m, part[k * C2 + t]);
    M[t] = m;
    g[t] = reinterpret_cast<const float*>(p.up[0])[(size_t)n * (C + C2) + C + t];
  }
  __syncthreads();
  float ls = 0.f;
  for (int px = grp; px < HW; px += ngrp) ls += expf(ldx<T>(p.in, px0 + px, C2, j) - M[j]);
  part[t] = ls;
  __syncthreads();
  if (t < C2) {
    float s = part[t];
    for (int k = 1; k < ngrp; ++k) s += part[k * C2 + t];
    S[t] = s;
  }
  __syncthreads();
  for (int px = t; px < HW; px += 256) {
    float ctx = 0.f;
    for (int k = 0; k < C2; ++k) ctx = fmaf(g[k], expf(ldx<T>(p.in, px0 + px, C2, k) - M[k]) / S[k], ctx);
    msp[px] = 1.f / (1.f + expf(-ctx));
  }
  __syncthreads();
  for (int i = t; i < HW * C; i += 256) stx<T>(p.out, px0 + i / C, C, i % C, ldx<T>(p.res, px0 + i / C, C, i % C) * msp[i / C]);
}

// ---------------------------------------------------------------------------------------------------------------
// The wide arm: C = 512 (layer 4 of pose_resnet_psa's ResNet-18 / 34, deep_hrnet/lib/models/pose_resnet_psa.py:39,121).
// Its maps are tiny (8x6 at 256x192, 12x9 at 384x288, 4x3 at 128x96) while a weight row is 2 KB, so one thread per
// pixel or per weight row would leave the workgroup idle and every lane on its own cache line.  Here the lanes of a
// wave always run along the contiguous dimension -- the channels of a pixel of x / theta, the input channels of a
// weight row -- and a dot product is reduced across the wave by a butterfly of __shfl_xor (the same bits in every lane,
// a fixed order), across waves through LDS.  One workgroup of 8 waves per image, no atomics: an image's result depends
// on nothing but the image.
constexpr int kWideC = 512, kWideThreads = 512, kWideWaves = kWideThreads / 64;

__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// y[r] (+ bias[r]) = W[r][0 .. 256 NV) . v for the rows r = wave, wave + 8, ...: lane l holds v[4l .. 4l + 3] of every
// 256-column panel and reads the same columns of the row (a float4 per panel: 1 KB per wave instruction).  Eight rows
// at a time: their loads are issued together and their eight butterflies interleave, so a wave waits for memory and
// for the cross-lane network once per eight rows, not once per row; lane k then stores row k of the eight.
template <int NV, int ROWS>
__device__ __forceinline__ void wide_matvec(const float* __restrict__ W, const float* v, const float* __restrict__ bias, float* y,
                                            int lane, int wave) {
  constexpr int B = 8, PER_WAVE = ROWS / kWideWaves;
  static_assert(ROWS % (B * kWideWaves) == 0, "rows in whole batches per wave");
  f32x4 vv[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) vv[j] = *reinterpret_cast<const f32x4*>(v + 256 * j + 4 * lane);
  for (int b0 = 0; b0 < PER_WAVE; b0 += B) {
    f32x4 a[B][NV];
#pragma unroll
    for (int k = 0; k < B; ++k)
#pragma unroll
      for (int j = 0; j < NV; ++j)
        a[k][j] = *reinterpret_cast<const f32x4*>(W + (size_t)(wave + kWideWaves * (b0 + k)) * (256 * NV) + 256 * j + 4 * lane);
    float s[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
      s[k] = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        s[k] = fmaf(a[k][j].x, vv[j].x, s[k]);
        s[k] = fmaf(a[k][j].y, vv[j].y, s[k]);
        s[k] = fmaf(a[k][j].z, vv[j].z, s[k]);
        s[k] = fmaf(a[k][j].w, vv[j].w, s[k]);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < B; ++k) s[k] += __shfl_xor(s[k], off);
    float mine = s[0];
#pragma unroll
    for (int k = 1; k < B; ++k) mine = lane == k ? s[k] : mine;
    if (lane < B) {
      const int r = wave + kWideWaves * (b0 + lane);
      y[r] = bias ? mine + bias[r] : mine;
    }
  }
}

// POOL at C = 512: the logit of a pixel is one wave's dot product (lane l: channels l, l + 64, ..), the two pooled
// rows are one thread per channel over the pixels (a wave reads 64 consecutive channels of a pixel)
template <typename T>
__global__ __launch_bounds__(kWideThreads) void psa_pool_wide_kernel(const ConvParams p) {
  extern __shared__ float sm[];   // e[HW]
  __shared__ float red[kWideWaves];
  constexpr int C = kWideC;
  const int HW = p.Hin * p.Win;
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t px0 = (size_t)n * HW;
  const PsaW w(reinterpret_cast<const float*>(p.wgt), C);
  float* e = sm;
  float wq[C / 64];
#pragma unroll
  for (int k = 0; k < C / 64; ++k) wq[k] = w.wq[lane + 64 * k];
  for (int px = wave; px < HW; px += kWideWaves) {
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < C / 64; ++k) q = fmaf(ldx<T>(p.in, px0 + px, C, lane + 64 * k), wq[k], q);
    q = wave_sum(q);
    if (lane == 0) e[px] = q;
  }
  __syncthreads();
  float lmax = -INFINITY;
  for (int px = t; px < HW; px += kWideThreads) lmax = fmaxf(lmax, e[px]);
  const float gmax = block_reduce(lmax, true, red);
  float lsum = 0.f;
  for (int px = t; px < HW; px += kWideThreads) {
    const float v = expf(e[px] - gmax);
    e[px] = v;
    lsum += v;
  }
  const float gsum = block_reduce(lsum, false, red);   // (its barriers also publish e[])
  float a = 0.f, m = 0.f;
#pragma unroll 4
  for (int px = 0; px < HW; ++px) {
    const float v = ldx<T>(p.in, px0 + px, C, t);
    a = fmaf(e[px], v, a);
    m += v;
  }
  float* o = reinterpret_cast<float*>(p.out) + (size_t)n * 2 * C;
  o[t] = a / gsum;
  o[C + t] = m / (float)HW;
}

// MLP at C = 512: every matrix-vector product with the input-channel index along the lanes.  Wv / Wg rows (512 floats)
// and W1 rows (256) are one wave each, a W2 row (64 floats) is 16 lanes, four rows per wave instruction; the LayerNorm
// over C/8 = 64 values is one wave with one value per lane.
__global__ __launch_bounds__(kWideThreads) void psa_mlp_wide_kernel(const ConvParams p) {
  constexpr int C = kWideC, C2 = C / 2, C8 = C / 8;
  __shared__ __attribute__((aligned(16))) float xb[C], xm[C], ctx[C2], h[C8], msk[C];
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const PsaW w(reinterpret_cast<const float*>(p.wgt), C);
  const float* s = reinterpret_cast<const float*>(p.in) + (size_t)n * 2 * C;
  xb[t] = s[t];
  xm[t] = s[C + t];
  __syncthreads();
  wide_matvec<2, C2>(w.wv, xb, nullptr, ctx, lane, wave);
  __syncthreads();
  wide_matvec<1, C8>(w.w1, ctx, w.b1, h, lane, wave);
  __syncthreads();
  if (wave == 0) {
    const float v = h[lane];
    const float mu = wave_sum(v) / (float)C8;
    const float d = v - mu;
    const float rstd = rsqrtf(wave_sum(d * d) / (float)C8 + 1e-5f);
    h[lane] = fmaxf(d * rstd * w.lg[lane] + w.lb[lane], 0.f);
  }
  __syncthreads();
  float* o = reinterpret_cast<float*>(p.out) + (size_t)n * (C + C2);
  {
    constexpr int B = 4;                 // wave instructions (of four rows each) in flight
    const int sub = lane & 15, quad = lane >> 4;
    const f32x4 hv = *reinterpret_cast<const f32x4*>(h + 4 * sub);
    for (int b0 = 0; b0 < C / (4 * kWideWaves); b0 += B) {
      f32x4 a[B];
#pragma unroll
      for (int k = 0; k < B; ++k)
        a[k] = *reinterpret_cast<const f32x4*>(w.w2 + (size_t)(4 * (wave + kWideWaves * (b0 + k)) + quad) * C8 + 4 * sub);
      float v[B];
#pragma unroll
      for (int k = 0; k < B; ++k) v[k] = fmaf(a[k].w, hv.w, fmaf(a[k].z, hv.z, fmaf(a[k].y, hv.y, a[k].x * hv.x)));
#pragma unroll
      for (int off = 8; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < B; ++k) v[k] += __shfl_xor(v[k], off);
      if (sub == 0) {
#pragma unroll
        for (int k = 0; k < B; ++k) {
          const int r = 4 * (wave + kWideWaves * (b0 + k)) + quad;
          const float m = 1.f / (1.f + expf(-(v[k] + w.b2[r])));
          msk[r] = m * xm[r];
          o[r] = m;
        }
      }
    }
  }
  __syncthreads();
  wide_matvec<2, C2>(w.wg, msk, nullptr, o + C, lane, wave);
}

// SP at C = 512 (theta has 256 channels): the soft-max statistics per theta channel are one thread per channel over
// the pixels of its half (even / odd pixels, combined through LDS); the gate of a pixel is one wave's dot product
// over the 256 channels; the product with x1 is one thread per channel.
template <typename T>
__global__ __launch_bounds__(kWideThreads) void psa_sp_wide_kernel(const ConvParams p) {
  extern __shared__ float sm[];   // msp[HW] | part[512] | M[256] | gs[256]
  constexpr int C = kWideC, C2 = C / 2;
  const int HW = p.Hin * p.Win;
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t px0 = (size_t)n * HW;
  float* msp = sm;
  float* part = sm + HW;
  float* M = part + kWideThreads;
  float* gs = M + C2;
  const int j = t & (C2 - 1), half = t >> 8;
  float lm = -INFINITY;
  for (int px = half; px < HW; px += 2) lm = fmaxf(lm, ldx<T>(p.in, px0 + px, C2, j));
  part[t] = lm;
  __syncthreads();
  if (t < C2) M[t] = fmaxf(part[t], part[C2 + t]);
  __syncthreads();
  float ls = 0.f;
  for (int px = half; px < HW; px += 2) ls += expf(ldx<T>(p.in, px0 + px, C2, j) - M[j]);
  part[t] = ls;
  __syncthreads();
  if (t < C2) gs[t] = reinterpret_cast<const float*>(p.up[0])[(size_t)n * (C + C2) + C + t] / (part[t] + part[C2 + t]);
  __syncthreads();
  float mj[C2 / 64], gj[C2 / 64];
#pragma unroll
  for (int k = 0; k < C2 / 64; ++k) {
    mj[k] = M[lane + 64 * k];
    gj[k] = gs[lane + 64 * k];
  }
  for (int px = wave; px < HW; px += kWideWaves) {
    float ctx = 0.f;
#pragma unroll
    for (int k = 0; k < C2 / 64; ++k) ctx = fmaf(gj[k], expf(ldx<T>(p.in, px0 + px, C2, lane + 64 * k) - mj[k]), ctx);
    ctx = wave_sum(ctx);
    if (lane == 0) msp[px] = 1.f / (1.f + expf(-ctx));
  }
  __syncthreads();
#pragma unroll 4
  for (int px = 0; px < HW; ++px) stx<T>(p.out, px0 + px, C, t, ldx<T>(p.res, px0 + px, C, t) * msp[px]);
}

static int check_psa_c(int C) {
  if (C == kWideC) return UDP_OK;
  if (C < 16 || C > 256 || (256 % C) != 0 || (C % 16) != 0)
    return fail(UDP_ERR_UNSUPPORTED, "PSA: C=%d must divide 256 and be a multiple of 16, or be 512", C);
  return UDP_OK;
}

// the wide kernels keep one float per pixel (and the soft-max statistics) in LDS
static int check_wide_hw(int HW) {
  if (HW > 8192) return fail(UDP_ERR_UNSUPPORTED, "PSA: C=512 on a map of %d pixels (at most 8192)", HW);
  return UDP_OK;
}

int describe_psa(const ConvParams& p, int dtype, int kind, Launch* out) {
  const int HW = p.Hin * p.Win;
  out->block = dim3(256);
  out->p = p;
  out->lds = 0;
  if (dtype != UDP_F32 && dtype != UDP_BF16 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "polarized self-attention ops: dtype %d", dtype);
  auto pick = [&](const void* kf, const void* kb, const void* kh) { return dtype == UDP_F32 ? kf : dtype == UDP_BF16 ? kb : kh; };
  switch (kind) {
    case UDP_OP_PSA_POOL: {
      const int rc = check_psa_c(p.Cin);
      if (rc) return rc;
      out->grid = dim3(p.N);
      if (p.Cin == kWideC) {
        if (check_wide_hw(HW)) return UDP_ERR_UNSUPPORTED;
        out->fn = pick(reinterpret_cast<const void*>(&psa_pool_wide_kernel<float>), reinterpret_cast<const void*>(&psa_pool_wide_kernel<__bf16>),
                       reinterpret_cast<const void*>(&psa_pool_wide_kernel<H2>));
        out->block = dim3(kWideThreads);
        out->lds = (unsigned)(HW * sizeof(float));
        return UDP_OK;
      }
      out->fn = pick(reinterpret_cast<const void*>(&psa_pool_kernel<float>), reinterpret_cast<const void*>(&psa_pool_kernel<__bf16>),
                     reinterpret_cast<const void*>(&psa_pool_kernel<H2>));
      out->lds = (unsigned)((HW + 512) * sizeof(float));
      return UDP_OK;
    }
    case UDP_OP_PSA_MLP: {
      const int rc = check_psa_c(p.Cin);
      if (rc) return rc;
      out->grid = dim3(p.N);
      if (p.Cin == kWideC) {
        out->fn = reinterpret_cast<const void*>(&psa_mlp_wide_kernel);
        out->block = dim3(kWideThreads);
        return UDP_OK;
      }
      out->fn = reinterpret_cast<const void*>(&psa_mlp_kernel);
      return UDP_OK;
    }
    case UDP_OP_PSA_SCALE: {
      out->fn = pick(reinterpret_cast<const void*>(&psa_scale_kernel<float>), reinterpret_cast<const void*>(&psa_scale_kernel<__bf16>),
                     reinterpret_cast<const void*>(&psa_scale_kernel<H2>));
      long blocks = ((long)p.N * HW * p.Cin + 255) / 256;
      out->grid = dim3((unsigned)(blocks > 8192 ? 8192 : blocks));
      return UDP_OK;
    }
    case UDP_OP_PSA_SP: {
      const int rc = check_psa_c(p.Cout);
      if (rc) return rc;
      out->grid = dim3(p.N);
      if (p.Cout == kWideC) {
        if (p.Cin != kWideC / 2) return fail(UDP_ERR_ARG, "PSA_SP: theta has %d channels, the map %d", p.Cin, p.Cout);
        if (check_wide_hw(HW)) return UDP_ERR_UNSUPPORTED;
        out->fn = pick(reinterpret_cast<const void*>(&psa_sp_wide_kernel<float>), reinterpret_cast<const void*>(&psa_sp_wide_kernel<__bf16>),
                       reinterpret_cast<const void*>(&psa_sp_wide_kernel<H2>));
        out->block = dim3(kWideThreads);
        out->lds = (unsigned)((HW + kWideThreads + kWideC) * sizeof(float));
        return UDP_OK;
      }
      out->fn = pick(reinterpret_cast<const void*>(&psa_sp_kernel<float>), reinterpret_cast<const void*>(&psa_sp_kernel<__bf16>),
                     reinterpret_cast<const void*>(&psa_sp_kernel<H2>));
      out->lds = (unsigned)((HW + 256 + 3 * p.Cin) * sizeof(float));
      return UDP_OK;
    }
  }
  return fail(UDP_ERR_ARG, "describe_psa: kind %d", kind);
}

int psa_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
