// The depthwise training kernels for gfx950, one family for every net that trains with a depthwise conv (ShuffleNetV2:
// deep_hrnet/lib/models/backbones/shufflenetv2.py:54, :66; MobileNetV3-small: the depthwise member of every
// InvertedResidual of udp_pose_amd/synth_mobilenetv3.py BLOCKS):
//
//   udp_dwconvk_train_fwd    depthwise K x K (K = 3 | 5), stride 1 | 2, on the parameter's own [C_real][1][K][K] layout
//   udp_dwconvk_dgrad        its input gradient as a gather (optionally accumulating: a stride-2 ShuffleNetV2 unit's input
//                            feeds two branches)
//   udp_dwconvk_wgrad        its weight gradient: per-workgroup partials over a fixed row split, reduced in index order
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4: a thread owns 4 consecutive channels and
// moves 16 bytes.  Every kernel writes EVERY stored channel of its outputs (padded channels: zeros computed from zeros),
// there are no atomics, and every sum has one order that depends on the shape alone.  The tap sums are explicit fmaf
// (the file is compiled without fp contraction, like dwconv.hip).
#include "common.h"

namespace udp {

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
// Every output still sums its taps by fmaf in (ky, kx) order with the taps outside the image skipped (the contract of
// dwconv3_kernel).
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
// Weight gradient.  The n * hout output rows are cut into `partials` runs of `rows` consecutive rows (the last may be
// shorter); workgroup (p, cb) owns run p and `cgw` channel groups from cb * cgw.  Its 256 threads are cgw channel lanes
// (lanes run along channels: a wave's loads are contiguous) x 256 / cgw pixel lanes; pixel lane l visits pixels l,
// l + PL, ... of the run in order, keeping K*K taps x 4 channels in registers.  The pixel lanes are combined through LDS
// in lane order, one kernel row at a time (K x 4 KiB), and the partial goes to the workspace as [p][K*K][C];
// dwk_wgrad_reduce_kernel adds the partials in index order and writes the parameter layout [C_real][K*K].  (A 3x3
// form that combined all 9 taps at once, 36 KiB of LDS, with a reduce thread per parameter element took 1756 us over the
// 3x3 convs of the two steps where this takes 752 us: tools/bench_dw_train.py, NOTES.md.)
// ---------------------------------------------------------------------------------------------
constexpr int kDwkMaxPartials = 256;     // a split never has more runs: one per CU of an MI355X

struct DwkWgradPlan {
  int rows, partials, cgw, cblocks;
};

// The split as a pure function of the shape and the workspace size: host arithmetic that returns its refusal as a code
// and leaves the message to the caller, because the size query calls it too.
static int dwk_wgrad_split(int n, int hout, int wout, int C, int kk, size_t workspace_bytes, DwkWgradPlan* pl) {
  if (n <= 0 || hout <= 0 || wout <= 0 || C <= 0 || (C & 3)) return UDP_ERR_ARG;
  const long R = (long)n * hout;
  if (R >= (1L << 31) || R * wout >= (1L << 31)) return UDP_ERR_UNSUPPORTED;
  long pmax = (long)(workspace_bytes / ((size_t)kk * C * sizeof(float)));
  if (pmax < 1) return UDP_ERR_WORKSPACE;
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

static int dwk_wgrad_plan(const char* who, int n, int hout, int wout, int C, int kk, size_t workspace_bytes, DwkWgradPlan* pl) {
  const int rc = dwk_wgrad_split(n, hout, wout, C, kk, workspace_bytes, pl);
  if (rc == UDP_ERR_ARG) return fail(rc, "%s: %dx%d x%d C%d (C %% 4)", who, hout, wout, n, C);
  if (rc == UDP_ERR_UNSUPPORTED) return fail(rc, "%s: %ld output rows", who, (long)n * hout);
  if (rc == UDP_ERR_WORKSPACE)
    return fail(rc, "%s: workspace %zu B holds no [%d][%d] partial (%zu B)", who, workspace_bytes, kk, C, (size_t)kk * C * sizeof(float));
  return rc;
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

}  // namespace udp

using namespace udp;

// TW: output (input) pixels of a thread's strip -- 2 for 3x3, 4 for 5x5.  At K = 3 a strip of 2 takes 125 / 152 us where
// one pixel per thread takes 158 / 210 us (forward / input gradient over all 3x3 depthwise convs of a 256x192 batch-32
// ShuffleNetV2 1.0x + MobileNetV3-small step: tools/bench_dw_train.py, NOTES.md).
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

// a size query: the split without a message, so that udp_last_error() keeps the message of the last real call
extern "C" size_t udp_dwconvk_wgrad_workspace_bytes(int n, int hout, int wout, int c, int ks) {
  DwkWgradPlan pl;
  if ((ks != 3 && ks != 5) || dwk_wgrad_split(n, hout, wout, c, ks * ks, ~(size_t)0, &pl)) return 0;
  return (size_t)pl.partials * ks * ks * c * sizeof(float);
}

extern "C" int udp_debug_dw_wgrad_plan(int n, int hout, int wout, int c, int ks, size_t workspace_bytes, int* out) {
  if (!out) return fail(UDP_ERR_ARG, "udp_debug_dw_wgrad_plan: null pointer");
  if (ks != 3 && ks != 5) return fail(UDP_ERR_UNSUPPORTED, "udp_debug_dw_wgrad_plan: kernel size %d (3 or 5)", ks);
  DwkWgradPlan pl;
  if (const int rc = dwk_wgrad_plan("udp_debug_dw_wgrad_plan", n, hout, wout, c, ks * ks, workspace_bytes, &pl)) return rc;
  out[0] = pl.rows;
  out[1] = pl.partials * pl.cblocks;
  out[2] = pl.partials;
  out[3] = 256 * ks * 4 * (int)sizeof(float);             // sAcc of dwk_wgrad_partial_kernel<ks, .>
  return UDP_OK;
}

extern "C" int udp_dwconvk_wgrad(const void* x, const void* dy, int n, int hin, int win, int c, int c_real, int ks, int stride,
                                 int dtype, void* dw, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = dwk_check("udp_dwconvk_wgrad", x, dy, dw, n, hin, win, c, c_real, ks, stride, dtype)) return rc;
  if (!workspace) return fail(UDP_ERR_ARG, "udp_dwconvk_wgrad: null pointer");
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  DwkWgradPlan pl;
  if (const int rc = dwk_wgrad_plan("udp_dwconvk_wgrad", n, ho, wo, c, ks * ks, workspace_bytes, &pl)) return rc;
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
