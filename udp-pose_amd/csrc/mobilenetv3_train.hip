// Training kernels of the MobileNetV3-small pose nets (deep_hrnet/lib/models/backbones/mobilenetv3.py:5-16: torchvision's
// mobilenet_v3_small().features; the block table is udp_pose_amd/synth_mobilenetv3.py BLOCKS) for gfx950 that the
// ShuffleNetV2 step (shufflenet_train.hip) does not have:
//
//   udp_dwconvk_train_fwd    depthwise K x K (K = 3 | 5), stride 1 | 2, on the parameter's own [C_real][1][K][K] layout
//   udp_dwconvk_dgrad        its input gradient as a gather (optionally accumulating)
//   udp_dwconvk_wgrad        its weight gradient: per-workgroup partials over a fixed row split, reduced in index order
//   udp_hswish_fwd / _bwd    nn.Hardswish and its derivative
//   udp_se_train_fwd / _bwd  torchvision.ops.SqueezeExcitation (fc1 / fc2 with biases, ReLU, Hardsigmoid) in train mode
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4: a thread owns 4 consecutive channels and
// moves 16 bytes.  Every kernel writes EVERY stored channel of its outputs (padded channels: exact zeros), there are no
// atomics, and every sum has one order that depends on the shape alone.  The tap sums and dot products are explicit fmaf
// (the file is compiled without fp contraction, like shufflenet_train.hip).
#include "common.h"

namespace udp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The 4 x KK weights of channels c .. c+3 from the [C_real][KK] parameter; channels >= C_real read as 0.  KK * c floats
// is a multiple of 16 bytes for c % 4 == 0, so a full group is KK 16-byte loads.
template <int KK>
__device__ __forceinline__ void dwk_load_w(const float* __restrict__ w, int c, int Creal, float (&wv)[4][KK]) {
  if (c + 4 <= Creal) {
    float flat[4 * KK];
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + (size_t)c * KK + 4 * q);
      flat[4 * q] = v[0], flat[4 * q + 1] = v[1], flat[4 * q + 2] = v[2], flat[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < KK; ++t) wv[e][t] = flat[e * KK + t];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < KK; ++t) wv[e][t] = c + e < Creal ? w[(size_t)(c + e) * KK + t] : 0.f;
  }
}

// thread = a strip of TW consecutive output pixels of one row x 4 channels.  Per kernel row the (TW - 1) S + K input
// columns the strip reaches are loaded once and serve all its outputs (K = 5, TW = 4, stride 1: 8 loads for 20 taps).
// Every output still sums its taps by fmaf in (ky, kx) order with the taps outside the image skipped.
template <int K, int S, int TW>
__global__ __launch_bounds__(256) void dwk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int H, int W,
                                                     int C, int Creal, int Ho, int Wo, float* __restrict__ y) {
  constexpr int P = K / 2, NC = (TW - 1) * S + K;
  const int C4 = C >> 2, WS = (Wo + TW - 1) / TW;
  const long total = (long)N * Ho * WS * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    long r = idx / C4;
    const int ox0 = (int)(r % WS) * TW;
    r /= WS;
    const int oy = (int)(r % Ho);
    const long n = r / Ho;
    const int ix0 = ox0 * S - P;
    float wv[4][K * K];
    dwk_load_w<K * K>(w, c, Creal, wv);
    f32x4 acc[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = oy * S + ky - P;
      if (iy < 0 || iy >= H) continue;
      const float* row = x + ((n * H + iy) * W) * C + c;
      f32x4 col[NC];
      bool ok[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const int ix = ix0 + q;
        ok[q] = ix >= 0 && ix < W;
        col[q] = ok[q] ? *reinterpret_cast<const f32x4*>(row + (long)ix * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < TW; ++j)
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
          if (ok[j * S + kx]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] = __builtin_fmaf(col[j * S + kx][e], wv[e][ky * K + kx], acc[j][e]);
          }
    }
    float* out = y + ((n * Ho + oy) * Wo) * C + c;
#pragma unroll
    for (int j = 0; j < TW; ++j)
      if (ox0 + j < Wo) *reinterpret_cast<f32x4*>(out + (long)(ox0 + j) * C) = acc[j];
  }
}

// thread = a strip of TW consecutive INPUT pixels of one row x 4 channels.  Tap (ky, kx) of input pixel ix0 + j reads
// dy at ((iy + P - ky) / S, (ix0 + j + P - kx) / S) when both divisions are exact and the index lies inside dy.  ix0 is a
// multiple of TW (even for stride 2), so which kx contribute to which j, and from which of the strip's dy columns, is
// known when the kernel is compiled.  The sum of an input pixel runs in (ky, kx) order from 0 and is added to dx last
// when accumulating.
template <int K, int S, int TW>
__global__ __launch_bounds__(256) void dwk_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int H, int W,
                                                       int C, int Creal, int Ho, int Wo, int accumulate, float* __restrict__ dx) {
  static_assert(S == 1 || TW % 2 == 0, "a stride-2 strip starts at an even column");
  constexpr int P = K / 2;
  constexpr int DMIN = S == 1 ? -P : -(P / 2), DMAX = S == 1 ? TW - 1 + P : (TW - 1 + P) / 2, NC = DMAX - DMIN + 1;
  const int C4 = C >> 2, WS = (W + TW - 1) / TW;
  const long total = (long)N * H * WS * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    long r = idx / C4;
    const int ix0 = (int)(r % WS) * TW;
    r /= WS;
    const int iy = (int)(r % H);
    const long n = r / H;
    const int ob = ix0 / S + DMIN;                         // dy column of col[0]
    float wv[4][K * K];
    dwk_load_w<K * K>(w, c, Creal, wv);
    f32x4 g[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j) g[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int ty = iy + P - ky;
      if (ty < 0 || (S == 2 && (ty & 1))) continue;
      const int oy = ty / S;
      if (oy >= Ho) continue;
      const float* row = dy + ((n * Ho + oy) * Wo) * C + c;
      f32x4 col[NC];
      bool ok[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const int ox = ob + q;
        ok[q] = ox >= 0 && ox < Wo;
        col[q] = ok[q] ? *reinterpret_cast<const f32x4*>(row + (long)ox * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < TW; ++j)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int t = j + P - kx;                        // = tx - ix0
          if (S == 2 && (t & 1)) continue;
          const int q = (S == 1 ? t : t / 2) - DMIN;
          if (ok[q]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[j][e] = __builtin_fmaf(col[q][e], wv[e][ky * K + kx], g[j][e]);
          }
        }
    }
    float* out = dx + ((n * H + iy) * W) * C + c;
#pragma unroll
    for (int j = 0; j < TW; ++j) {
      if (ix0 + j >= W) continue;
      f32x4* o = reinterpret_cast<f32x4*>(out + (long)(ix0 + j) * C);
      f32x4 v = g[j];
      if (accumulate) {
        const f32x4 old = *o;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = old[e] + v[e];
      }
      *o = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Weight gradient: the row split of udp_dwconv3_wgrad.  The n * hout output rows are cut into `partials` runs of `rows`
// consecutive rows; workgroup (p, cb) owns run p and `cgw` channel groups from cb * cgw.  Its 256 threads are cgw channel
// lanes x 256 / cgw pixel lanes; pixel lane l visits pixels l, l + PL, ... of the run in order, keeping K*K taps x 4
// channels in registers.  The pixel lanes are combined through LDS in lane order, one kernel row at a time (K x 4 KiB),
// and the partial goes to the workspace as [p][K*K][C]; dwk_wgrad_reduce_kernel adds the partials in index order and
// writes the parameter layout [C_real][K*K].
// ---------------------------------------------------------------------------------------------
constexpr int kDwkMaxPartials = 256;     // a split never has more runs: one per CU of an MI355X

struct DwkWgradPlan {
  int rows, partials, cgw, cblocks;
};

static int dwk_wgrad_plan(int n, int hout, int wout, int C, int kk, size_t workspace_bytes, DwkWgradPlan* pl) {
  if (n <= 0 || hout <= 0 || wout <= 0 || C <= 0 || (C & 3))
    return fail(UDP_ERR_ARG, "udp_dwconvk_wgrad: %dx%d x%d C%d (C %% 4)", hout, wout, n, C);
  const long R = (long)n * hout;
  if (R >= (1L << 31) || R * wout >= (1L << 31)) return fail(UDP_ERR_UNSUPPORTED, "udp_dwconvk_wgrad: %ld output rows", R);
  const size_t per = (size_t)kk * C * sizeof(float);
  long pmax = (long)(workspace_bytes / per);
  if (pmax < 1)
    return fail(UDP_ERR_WORKSPACE, "udp_dwconvk_wgrad: workspace %zu B holds no [%d][%d] partial (%zu B)", workspace_bytes, kk, C, per);
  if (pmax > kDwkMaxPartials) pmax = kDwkMaxPartials;
  if (pmax > R) pmax = R;
  pl->rows = (int)((R + pmax - 1) / pmax);
  pl->partials = (int)((R + pl->rows - 1) / pl->rows);
  const int C4 = C >> 2;
  int cgw = 8;
  while (cgw < 64 && cgw < C4) cgw *= 2;
  pl->cgw = cgw;
  pl->cblocks = (C4 + cgw - 1) / cgw;
  return UDP_OK;
}

template <int K, int S>
__global__ __launch_bounds__(256) void dwk_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N, int H,
                                                               int W, int C, int Ho, int Wo, int rows, int cgw, int cgw_shift,
                                                               float* __restrict__ ws) {
  constexpr int P = K / 2, KK = K * K;
  __shared__ float sAcc[256 * K * 4];
  const int t = threadIdx.x;
  const int lc = t & (cgw - 1), lp = t >> cgw_shift, PL = 256 >> cgw_shift;
  const int cg = blockIdx.y * cgw + lc;                   // channel group of this thread
  const bool live = cg < (C >> 2);
  const int c = cg * 4;
  const long R = (long)N * Ho;
  const long r0 = (long)blockIdx.x * rows;
  const long r1 = r0 + rows < R ? r0 + rows : R;
  const int npix = (int)(r1 - r0) * Wo;
  float acc[KK][4];
#pragma unroll
  for (int k = 0; k < KK; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
  if (live) {
    for (int q = lp; q < npix; q += PL) {
      const long row = r0 + q / Wo;
      const int ox = q % Wo;
      const int oy = (int)(row % Ho);
      const long n = row / Ho;
      const f32x4 d = *reinterpret_cast<const f32x4*>(dy + (row * Wo + ox) * C + c);
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int iy = oy * S + ky - P;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int ix = ox * S + kx - P;
          if (ix < 0 || ix >= W) continue;
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + iy) * W + ix) * C + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ky * K + kx][e] = __builtin_fmaf(d[e], v[e], acc[ky * K + kx][e]);
        }
      }
    }
  }
  // sAcc[lp][kx][lc * 4 + e] for one ky at a time: the combining threads below read consecutive floats
  const int span = cgw * 4;
  float* out = ws + (size_t)blockIdx.x * KK * C;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
#pragma unroll
    for (int kx = 0; kx < K; ++kx)
      *reinterpret_cast<f32x4*>(sAcc + (lp * K + kx) * span + lc * 4) =
          f32x4{acc[ky * K + kx][0], acc[ky * K + kx][1], acc[ky * K + kx][2], acc[ky * K + kx][3]};
    __syncthreads();
    for (int o = t; o < K * span; o += 256) {
      const int kx = o / span, cc = o - kx * span;
      const int ch = blockIdx.y * span + cc;
      if (ch >= C) continue;
      float s = sAcc[kx * span + cc];
      for (int l = 1; l < PL; ++l) s += sAcc[(l * K + kx) * span + cc];
      out[(ky * K + kx) * C + ch] = s;
    }
    __syncthreads();
  }
}

// thread = one element of the [KK][C] workspace layout (a wave reads consecutive floats of every partial); the sum goes
// to its place c * KK + tap of the parameter layout
__global__ __launch_bounds__(256) void dwk_wgrad_reduce_kernel(const float* __restrict__ ws, int partials, int C, int Creal, int KK,
                                                              float* __restrict__ dw) {
  const int o = blockIdx.x * 256 + threadIdx.x;           // = tap * C + c
  if (o >= KK * C) return;
  const int k = o / C, c = o - k * C;
  if (c >= Creal) return;
  const size_t pitch = (size_t)KK * C;
  float s = ws[o];
#pragma unroll 4
  for (int p = 1; p < partials; ++p) s += ws[p * pitch + o];
  dw[c * KK + k] = s;
}

// ---------------------------------------------------------------------------------------------
// Hard-swish.  y = x * clamp(x + 3, 0, 6) / 6;  dx = 0 (x < -3) | dy * (x / 3 + 0.5) (-3 <= x <= 3) | dy (x > 3): the
// derivative autograd gives the clamp form.  AT x = -3 and x = 3 torch's own hardswish_backward (nn.Hardswish, which the
// reference's backbone uses) takes the outer pieces, 0 and dy, instead of -0.5 dy and 1.5 dy; everywhere else they agree.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float hsig(float s) { return fminf(fmaxf(s + 3.f, 0.f), 6.f) / 6.f; }

__global__ __launch_bounds__(256) void hswish_fwd_kernel(const float* __restrict__ x, long total4, float* __restrict__ y) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e] * fminf(fmaxf(v[e] + 3.f, 0.f), 6.f) / 6.f;
    *reinterpret_cast<f32x4*>(y + i * 4) = o;
  }
}

__global__ __launch_bounds__(256) void hswish_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, long total4,
                                                        float* __restrict__ dx) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
    const f32x4 d = *reinterpret_cast<const f32x4*>(dy + i * 4);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e] < -3.f ? 0.f : (v[e] > 3.f ? d[e] : d[e] * (v[e] / 3.f + 0.5f));
    *reinterpret_cast<f32x4*>(dx + i * 4) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// Squeeze-and-excitation.
// ---------------------------------------------------------------------------------------------
// Per-image, per-channel sum over the map.  Workgroup (cb, n): cgw channel lanes x 256 / cgw pixel lanes; pixel lane l
// adds pixels l, l + PL, ... in order, the lanes are combined through LDS in lane order.  MODE 0: out = sum(a) / div (the
// pool);  MODE 1: sum(a * b) by fmaf, turned into the gradient of the gate pre-activation: out = (-3 <= s <= 3) ? sum / 6 : 0.
template <int MODE>
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       const float* __restrict__ s, int HW, int C, int cgw, int cgw_shift, float div,
                                                       float* __restrict__ out) {
  __shared__ float sAcc[256 * 4];
  const int t = threadIdx.x;
  const int lc = t & (cgw - 1), lp = t >> cgw_shift, PL = 256 >> cgw_shift;
  const int cg = blockIdx.x * cgw + lc;
  const int n = blockIdx.y;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (cg < (C >> 2)) {
    const size_t base = (size_t)n * HW * C + cg * 4;
#pragma unroll 4
    for (int q = lp; q < HW; q += PL) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(a + base + (size_t)q * C);
      if (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
      } else {
        const f32x4 d = *reinterpret_cast<const f32x4*>(b + base + (size_t)q * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(v[e], d[e], acc[e]);
      }
    }
  }
  const int span = cgw * 4;
  *reinterpret_cast<f32x4*>(sAcc + lp * span + lc * 4) = acc;
  __syncthreads();
  for (int o = t; o < span; o += 256) {
    const int ch = blockIdx.x * span + o;
    if (ch >= C) continue;
    float v = sAcc[o];
    for (int l = 1; l < PL; ++l) v += sAcc[l * span + o];
    if (MODE == 0) {
      v = v / div;
    } else {
      const float z = s[(size_t)n * C + ch];
      v = (z >= -3.f && z <= 3.f) ? v / 6.f : 0.f;
    }
    out[(size_t)n * C + ch] = v;
  }
}

constexpr int kSeRows = 16;              // rows of se_matvec_kernel per workgroup, columns of se_matvec_t_kernel

// one fixed butterfly: every lane ends with the same sum, the order depends on nothing but the lane count
__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m, 64);
  return a;
}

// out[n][r] = act(bias[r] + sum_k Wm[r][k] * in[n][k]) for r < R, zeros for R <= r < out_pitch.  Workgroup (rb, n): 16
// rows, a wave per row at a time, lanes stride over k.
template <int RELU>
__global__ __launch_bounds__(256) void se_matvec_kernel(const float* __restrict__ in, int in_pitch, const float* __restrict__ Wm,
                                                       const float* __restrict__ bias, int R, int K, float* __restrict__ out,
                                                       int out_pitch) {
  const int n = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* v = in + (size_t)n * in_pitch;
  for (int rr = wave; rr < kSeRows; rr += 4) {
    const int r = blockIdx.x * kSeRows + rr;
    if (r >= out_pitch) break;
    float a = 0.f;
    if (r < R) {
      const float* wr = Wm + (size_t)r * K;
      for (int k = lane; k < K; k += 64) a = __builtin_fmaf(wr[k], v[k], a);
      a = wave_sum(a) + bias[r];
      if (RELU) a = fmaxf(a, 0.f);
    }
    if (lane == 0) out[(size_t)n * out_pitch + r] = a;
  }
}

// out[n][k] = sum_r g[n][r] * Wm[r][k] for k < K (zeroed where mask[n][k] <= 0 when a mask is given), zeros for
// K <= k < out_pitch.  Workgroup (kb, n): 16 columns x 16 row lanes; row lane l adds rows l, l + 16, ... in order (16
// lanes read 64 consecutive bytes of a weight row), the lanes are combined through LDS in lane order.
__global__ __launch_bounds__(256) void se_matvec_t_kernel(const float* __restrict__ g, int g_pitch, const float* __restrict__ Wm, int R,
                                                         int K, const float* __restrict__ mask, float* __restrict__ out,
                                                         int out_pitch) {
  __shared__ float sAcc[256];
  const int n = blockIdx.y, kl = threadIdx.x & (kSeRows - 1), rl = threadIdx.x >> 4;
  const int k = blockIdx.x * kSeRows + kl;
  float a = 0.f;
  if (k < K) {
    const float* gv = g + (size_t)n * g_pitch;
#pragma unroll 4
    for (int r = rl; r < R; r += 16) a = __builtin_fmaf(gv[r], Wm[(size_t)r * K + k], a);
  }
  sAcc[rl * kSeRows + kl] = a;
  __syncthreads();
  if (rl != 0 || k >= out_pitch) return;
  for (int l = 1; l < 16; ++l) a += sAcc[l * kSeRows + kl];
  if (k < K && mask && !(mask[(size_t)n * out_pitch + k] > 0.f)) a = 0.f;
  out[(size_t)n * out_pitch + k] = a;
}

// The four parameter gradients, every sum over the images in index order:
//   dW2[c][j] = sum_n ds[n][c] h[n][j]   dW1[j][c] = sum_n dh[n][j] pool[n][c]   db2[c] = sum_n ds[n][c]   db1[j] = sum_n dh[n][j]
__global__ __launch_bounds__(256) void se_param_grad_kernel(const float* __restrict__ ds, const float* __restrict__ dh,
                                                           const float* __restrict__ pool, const float* __restrict__ h, int N, int C,
                                                           int Creal, int S, float* __restrict__ dw1, float* __restrict__ db1,
                                                           float* __restrict__ dw2, float* __restrict__ db2) {
  const int CS = Creal * S;
  int i = blockIdx.x * 256 + threadIdx.x;
  float a = 0.f;
  if (i < CS) {
    const int c = i / S, j = i - c * S;
    for (int n = 0; n < N; ++n) a = __builtin_fmaf(ds[(size_t)n * C + c], h[(size_t)n * S + j], a);
    dw2[i] = a;
    return;
  }
  i -= CS;
  if (i < CS) {
    const int j = i / Creal, c = i - j * Creal;
    for (int n = 0; n < N; ++n) a = __builtin_fmaf(dh[(size_t)n * S + j], pool[(size_t)n * C + c], a);
    dw1[i] = a;
    return;
  }
  i -= CS;
  if (i < Creal) {
    for (int n = 0; n < N; ++n) a += ds[(size_t)n * C + i];
    db2[i] = a;
    return;
  }
  i -= Creal;
  if (i < S) {
    for (int n = 0; n < N; ++n) a += dh[(size_t)n * S + i];
    db1[i] = a;
  }
}

// BWD 0: y = x * gate;  BWD 1: dx (+)= dy * gate + dpool / HW, with gate = hardsigmoid(s[n][c]).  Channels >= C_real: 0.
template <int BWD>
__global__ __launch_bounds__(256) void se_scale_kernel(const float* __restrict__ a, const float* __restrict__ s,
                                                      const float* __restrict__ dpool, long M, int HW, int C, int Creal, int accumulate,
                                                      float* __restrict__ out) {
  const int C4 = C >> 2;
  const long total = M * C4;
  const float hw = (float)HW;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const long n = pix / HW;
    const f32x4 v = *reinterpret_cast<const f32x4*>(a + pix * C + c);
    const f32x4 z = *reinterpret_cast<const f32x4*>(s + n * C + c);
    f32x4 o;
    if (BWD) {
      const f32x4 dp = *reinterpret_cast<const f32x4*>(dpool + n * C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = c + e < Creal ? __builtin_fmaf(v[e], hsig(z[e]), dp[e] / hw) : 0.f;
      if (accumulate) {
        const f32x4 old = *reinterpret_cast<const f32x4*>(out + pix * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = old[e] + o[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = c + e < Creal ? v[e] * hsig(z[e]) : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + pix * C + c) = o;
  }
}

static unsigned blocks_for(long total, int per, long cap) {
  long b = (total + per - 1) / per;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}
static int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return UDP_OK;
}

static int dwk_check(const char* who, const void* a, const void* b, const void* c, int n, int hin, int win, int C, int Creal, int ks,
                     int stride, int dtype) {
  if (!a || !b || !c) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (ks != 3 && ks != 5) return fail(UDP_ERR_UNSUPPORTED, "%s: kernel size %d (3 or 5)", who, ks);
  if (stride != 1 && stride != 2) return fail(UDP_ERR_UNSUPPORTED, "%s: stride %d (1 or 2)", who, stride);
  if (n <= 0 || hin <= 0 || win <= 0 || C <= 0 || (C & 3) || Creal <= 0 || Creal > C)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, C %d (C %% 4), C_real %d (1..C)", who, hin, win, n, C, Creal);
  if ((long)n * hin * win * C >= (1L << 40)) return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d x%d C%d is too large", who, hin, win, n, C);
  return UDP_OK;
}

static int se_check(const char* who, int n, int h, int w, int C, int Creal, int S, int dtype) {
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (n <= 0 || h <= 0 || w <= 0 || C <= 0 || (C & 3) || Creal <= 0 || Creal > C || S <= 0)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, C %d (C %% 4), C_real %d (1..C), squeeze %d (> 0)", who, h, w, n, C, Creal, S);
  if ((long)h * w >= (1L << 31) || n > 65535 || (long)n * h * w * C >= (1L << 40))
    return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d x%d C%d is too large", who, h, w, n, C);
  return UDP_OK;
}

// channel lanes of se_reduce_kernel: the power of two in 8..64 that covers C / 4
static void se_lanes(int C, int* cgw, int* shift, int* cblocks) {
  const int C4 = C >> 2;
  int g = 8, sh = 3;
  while (g < 64 && g < C4) g *= 2, ++sh;
  *cgw = g, *shift = sh, *cblocks = (C4 + g - 1) / g;
}

static size_t rup4(size_t v) { return (v + 3) & ~(size_t)3; }

}  // namespace udp

using namespace udp;

// TW: output (input) pixels of a thread's strip -- 2 for 3x3, 4 for 5x5
#define UDP_DWK_DISPATCH(KERNEL, ...)                                                  \
  do {                                                                                 \
    if (ks == 3 && stride == 1) KERNEL<3, 1, 2><<<blocks, 256, 0, s>>>(__VA_ARGS__);   \
    else if (ks == 3) KERNEL<3, 2, 2><<<blocks, 256, 0, s>>>(__VA_ARGS__);             \
    else if (stride == 1) KERNEL<5, 1, 4><<<blocks, 256, 0, s>>>(__VA_ARGS__);         \
    else KERNEL<5, 2, 4><<<blocks, 256, 0, s>>>(__VA_ARGS__);                          \
  } while (0)

extern "C" int udp_dwconvk_train_fwd(const void* x, const void* w, int n, int hin, int win, int c, int c_real, int ks, int stride,
                                     int dtype, void* y, void* stream) {
  if (const int rc = dwk_check("udp_dwconvk_train_fwd", x, w, y, n, hin, win, c, c_real, ks, stride, dtype)) return rc;
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  const int tw = ks == 3 ? 2 : 4;
  const long total = (long)n * ho * ((wo + tw - 1) / tw) * (c / 4);
  const unsigned blocks = blocks_for(total, 256, 1 << 20);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *xp = reinterpret_cast<const float*>(x), *wp = reinterpret_cast<const float*>(w);
  UDP_DWK_DISPATCH(dwk_fwd_kernel, xp, wp, n, hin, win, c, c_real, ho, wo, reinterpret_cast<float*>(y));
  return launched("udp_dwconvk_train_fwd");
}

extern "C" int udp_dwconvk_dgrad(const void* dy, const void* w, int n, int hin, int win, int c, int c_real, int ks, int stride,
                                 int accumulate, int dtype, void* dx, void* stream) {
  if (const int rc = dwk_check("udp_dwconvk_dgrad", dy, w, dx, n, hin, win, c, c_real, ks, stride, dtype)) return rc;
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  const int tw = ks == 3 ? 2 : 4;
  const long total = (long)n * hin * ((win + tw - 1) / tw) * (c / 4);
  const unsigned blocks = blocks_for(total, 256, 1 << 20);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *dp = reinterpret_cast<const float*>(dy), *wp = reinterpret_cast<const float*>(w);
  UDP_DWK_DISPATCH(dwk_dgrad_kernel, dp, wp, n, hin, win, c, c_real, ho, wo, accumulate != 0, reinterpret_cast<float*>(dx));
  return launched("udp_dwconvk_dgrad");
}

extern "C" size_t udp_dwconvk_wgrad_workspace_bytes(int n, int hout, int wout, int c, int ks) {
  // a size query: the plan's arithmetic without its fail(), so that udp_last_error() keeps the message of the last real call
  if ((ks != 3 && ks != 5) || n <= 0 || hout <= 0 || wout <= 0 || c <= 0 || (c & 3)) return 0;
  const long R = (long)n * hout;
  if (R >= (1L << 31) || R * wout >= (1L << 31)) return 0;
  const long pmax = R < kDwkMaxPartials ? R : kDwkMaxPartials;
  const long rows = (R + pmax - 1) / pmax;
  return (size_t)((R + rows - 1) / rows) * ks * ks * c * sizeof(float);
}

extern "C" int udp_dwconvk_wgrad(const void* x, const void* dy, int n, int hin, int win, int c, int c_real, int ks, int stride,
                                 int dtype, void* dw, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = dwk_check("udp_dwconvk_wgrad", x, dy, dw, n, hin, win, c, c_real, ks, stride, dtype)) return rc;
  if (!workspace) return fail(UDP_ERR_ARG, "udp_dwconvk_wgrad: null pointer");
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  DwkWgradPlan pl;
  if (const int rc = dwk_wgrad_plan(n, ho, wo, c, ks * ks, workspace_bytes, &pl)) return rc;
  int shift = 3;
  while ((1 << shift) < pl.cgw) ++shift;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *xp = reinterpret_cast<const float*>(x), *dp = reinterpret_cast<const float*>(dy);
  float* ws = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)pl.partials, (unsigned)pl.cblocks);
  if (ks == 3 && stride == 1) dwk_wgrad_partial_kernel<3, 1><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  else if (ks == 3) dwk_wgrad_partial_kernel<3, 2><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  else if (stride == 1) dwk_wgrad_partial_kernel<5, 1><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  else dwk_wgrad_partial_kernel<5, 2><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  if (const int rc = launched("udp_dwconvk_wgrad")) return rc;
  dwk_wgrad_reduce_kernel<<<ceil_div(c * ks * ks, 256), 256, 0, s>>>(ws, pl.partials, c, c_real, ks * ks, reinterpret_cast<float*>(dw));
  return launched("udp_dwconvk_wgrad");
}

static int hswish_check(const char* who, const void* a, const void* b, const void* c, int64_t count) {
  if (!a || !b || !c) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (count <= 0 || (count & 3)) return fail(UDP_ERR_ARG, "%s: count %lld (a positive multiple of 4)", who, (long long)count);
  return UDP_OK;
}

extern "C" int udp_hswish_fwd(const void* x, void* y, int64_t count, void* stream) {
  if (const int rc = hswish_check("udp_hswish_fwd", x, y, y, count)) return rc;
  hswish_fwd_kernel<<<blocks_for(count / 4, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(x), count / 4, reinterpret_cast<float*>(y));
  return launched("udp_hswish_fwd");
}

extern "C" int udp_hswish_bwd(const void* dy, const void* x, void* dx, int64_t count, void* stream) {
  if (const int rc = hswish_check("udp_hswish_bwd", dy, x, dx, count)) return rc;
  hswish_bwd_kernel<<<blocks_for(count / 4, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(dy), reinterpret_cast<const float*>(x), count / 4, reinterpret_cast<float*>(dx));
  return launched("udp_hswish_bwd");
}

extern "C" int udp_se_train_fwd(const void* x, const float* w1, const float* b1, const float* w2, const float* b2, int n, int h,
                                int w, int c, int c_real, int sq, int dtype, float* pool, float* hid, float* s, void* y,
                                void* stream) {
  if (!x || !w1 || !b1 || !w2 || !b2 || !pool || !hid || !s || !y) return fail(UDP_ERR_ARG, "udp_se_train_fwd: null pointer");
  if (const int rc = se_check("udp_se_train_fwd", n, h, w, c, c_real, sq, dtype)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int hw = h * w;
  int cgw, shift, cblocks;
  se_lanes(c, &cgw, &shift, &cblocks);
  const float* xp = reinterpret_cast<const float*>(x);
  se_reduce_kernel<0><<<dim3(cblocks, n), 256, 0, st>>>(xp, nullptr, nullptr, hw, c, cgw, shift, (float)hw, pool);
  se_matvec_kernel<1><<<dim3(ceil_div(sq, kSeRows), n), 256, 0, st>>>(pool, c, w1, b1, sq, c_real, hid, sq);
  se_matvec_kernel<0><<<dim3(ceil_div(c, kSeRows), n), 256, 0, st>>>(hid, sq, w2, b2, c_real, sq, s, c);
  const long m = (long)n * hw;
  se_scale_kernel<0><<<blocks_for(m * (c / 4), 256, 1 << 20), 256, 0, st>>>(xp, s, nullptr, m, hw, c, c_real, 0,
                                                                            reinterpret_cast<float*>(y));
  return launched("udp_se_train_fwd");
}

extern "C" size_t udp_se_train_workspace_bytes(int n, int c, int sq) {
  if (n <= 0 || c <= 0 || (c & 3) || sq <= 0) return 0;
  return (2 * rup4((size_t)n * c) + rup4((size_t)n * sq)) * sizeof(float);
}

extern "C" int udp_se_train_bwd(const void* dy, const void* x, const float* w1, const float* w2, const float* pool, const float* hid,
                                const float* s, int n, int h, int w, int c, int c_real, int sq, int accumulate, int dtype, void* dx,
                                float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!dy || !x || !w1 || !w2 || !pool || !hid || !s || !dx || !dw1 || !db1 || !dw2 || !db2 || !workspace)
    return fail(UDP_ERR_ARG, "udp_se_train_bwd: null pointer");
  if (const int rc = se_check("udp_se_train_bwd", n, h, w, c, c_real, sq, dtype)) return rc;
  const size_t need = udp_se_train_workspace_bytes(n, c, sq);
  if (workspace_bytes < need)
    return fail(UDP_ERR_WORKSPACE, "udp_se_train_bwd: workspace %zu B, %zu B needed", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int hw = h * w;
  float* ds = reinterpret_cast<float*>(workspace);       // [n][c]   gradient of the gate pre-activation
  float* dpool = ds + rup4((size_t)n * c);               // [n][c]
  float* dh = dpool + rup4((size_t)n * c);               // [n][sq]
  int cgw, shift, cblocks;
  se_lanes(c, &cgw, &shift, &cblocks);
  const float *dyp = reinterpret_cast<const float*>(dy), *xp = reinterpret_cast<const float*>(x);
  se_reduce_kernel<1><<<dim3(cblocks, n), 256, 0, st>>>(dyp, xp, s, hw, c, cgw, shift, 1.f, ds);
  se_matvec_t_kernel<<<dim3(ceil_div(sq, kSeRows), n), 256, 0, st>>>(ds, c, w2, c_real, sq, hid, dh, sq);
  se_matvec_t_kernel<<<dim3(ceil_div(c, kSeRows), n), 256, 0, st>>>(dh, sq, w1, sq, c_real, nullptr, dpool, c);
  se_param_grad_kernel<<<ceil_div(2 * c_real * sq + c_real + sq, 256), 256, 0, st>>>(ds, dh, pool, hid, n, c, c_real, sq, dw1, db1, dw2, db2);
  const long m = (long)n * hw;
  se_scale_kernel<1><<<blocks_for(m * (c / 4), 256, 1 << 20), 256, 0, st>>>(dyp, s, dpool, m, hw, c, c_real, accumulate != 0,
                                                                            reinterpret_cast<float*>(dx));
  return launched("udp_se_train_bwd");
}
