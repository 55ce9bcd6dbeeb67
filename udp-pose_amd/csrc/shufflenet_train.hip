// Training kernels of the ShuffleNetV2 pose nets (deep_hrnet/lib/models/backbones/shufflenetv2.py, decoders/DUC.py)
// for gfx950 that the HRNet / pose_resnet steps (train.hip, resnet_train.hip) do not have:
//
//   udp_dwconv3_train_fwd    depthwise 3x3, stride 1 | 2, on the parameter's own [C_real][1][3][3] layout (:54, :66)
//   udp_dwconv3_dgrad        its input gradient as a gather (optionally accumulating: a stride-2 unit's input feeds two branches)
//   udp_dwconv3_wgrad        its weight gradient: per-workgroup partials over a fixed row split, reduced in index order
//   udp_pixshuf2_train_fwd   nn.PixelShuffle(2) in torch's channel order (DUC.py:27) and
//   udp_pixshuf2_train_bwd   its inverse
//   udp_shuffle_pair_fwd     torch.cat + channel_shuffle (:77-92) on a unit output kept as a pair of halves, and
//   udp_shuffle_pair_bwd     the inverse permutation
//   udp_chan_cat2 / _uncat2  the materialised concat where the whole tensor is read, and its inverse
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4: a thread owns 4 consecutive channels and
// moves 16 bytes.  Every kernel writes EVERY stored channel of its output (padded channels: zeros computed from zeros),
// there are no atomics, and every sum has one order that depends on the shape alone.  The tap sums are explicit fmaf
// (the file is compiled without fp contraction, like dwconv.hip).
#include "common.h"

namespace udp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The 4 x 9 weights of channels c .. c+3 from the [C_real][9] parameter; channels >= C_real read as 0.  9c floats is a
// multiple of 16 bytes for c % 4 == 0, so a full group is nine 16-byte loads.
__device__ __forceinline__ void dw_train_load_w(const float* __restrict__ w, int c, int Creal, float (&wv)[4][9]) {
  if (c + 4 <= Creal) {
    float flat[36];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + (size_t)c * 9 + 4 * q);
      flat[4 * q] = v[0], flat[4 * q + 1] = v[1], flat[4 * q + 2] = v[2], flat[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 9; ++t) wv[e][t] = flat[e * 9 + t];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 9; ++t) wv[e][t] = c + e < Creal ? w[(size_t)(c + e) * 9 + t] : 0.f;
  }
}

// thread = one output pixel x 4 channels: nine fmaf in (ky, kx) order, taps outside the image skipped (the contract of
// dwconv3_kernel)
template <int S>
__global__ __launch_bounds__(256) void dw3_train_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, int N, int H,
                                                           int W, int C, int Creal, int Ho, int Wo, float* __restrict__ y) {
  const int C4 = C >> 2;
  const long total = (long)N * Ho * Wo * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const int ox = (int)(pix % Wo);
    const long r = pix / Wo;
    const int oy = (int)(r % Ho);
    const long n = r / Ho;
    float wv[4][9];
    dw_train_load_w(w, c, Creal, wv);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * S + ky - 1;
      if (iy < 0 || iy >= H) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * S + kx - 1;
        if (ix < 0 || ix >= W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + iy) * W + ix) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(v[e], wv[e][ky * 3 + kx], acc[e]);
      }
    }
    *reinterpret_cast<f32x4*>(y + pix * C + c) = acc;
  }
}

// thread = one INPUT pixel x 4 channels; tap (ky, kx) contributes when (iy + 1 - ky) is a multiple of the stride and the
// quotient lies inside dy.  The sum runs in (ky, kx) order from 0 and is added to dx last when accumulating.
template <int S>
__global__ __launch_bounds__(256) void dw3_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int H,
                                                       int W, int C, int Creal, int Ho, int Wo, int accumulate,
                                                       float* __restrict__ dx) {
  const int C4 = C >> 2;
  const long total = (long)N * H * W * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (int)(idx % C4) * 4;
    const long pix = idx / C4;
    const int ix = (int)(pix % W);
    const long r = pix / W;
    const int iy = (int)(r % H);
    const long n = r / H;
    float wv[4][9];
    dw_train_load_w(w, c, Creal, wv);
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = iy + 1 - ky;
      if (ty < 0 || (S == 2 && (ty & 1))) continue;
      const int oy = ty / S;
      if (oy >= Ho) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int tx = ix + 1 - kx;
        if (tx < 0 || (S == 2 && (tx & 1))) continue;
        const int ox = tx / S;
        if (ox >= Wo) continue;
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((n * Ho + oy) * Wo + ox) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = __builtin_fmaf(d[e], wv[e][ky * 3 + kx], g[e]);
      }
    }
    f32x4* out = reinterpret_cast<f32x4*>(dx + pix * C + c);
    if (accumulate) {
      const f32x4 o = *out;
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = o[e] + g[e];
    }
    *out = g;
  }
}

// ---------------------------------------------------------------------------------------------
// Weight gradient.  The n * hout output rows are cut into `partials` runs of `rows` consecutive rows (the last may be
// shorter); workgroup (p, cb) owns run p and `cgw` channel groups from cb * cgw.  Its 256 threads are cgw channel lanes
// (lanes run along channels: a wave's loads are contiguous) x 256 / cgw pixel lanes; pixel lane l visits pixels l,
// l + PL, ... of the run in order, keeping 9 taps x 4 channels in registers.  The pixel lanes are then combined through
// LDS in lane order and the partial goes to the workspace as [p][9][C]; dw3_wgrad_reduce_kernel adds the partials in
// index order and writes the parameter layout [C_real][9].
// ---------------------------------------------------------------------------------------------
constexpr int kDwMaxPartials = 256;      // a split never has more runs: one per CU of an MI355X
constexpr int kDwLdsBytes = 256 * 36 * 4;

struct DwWgradPlan {
  int rows, partials, cgw, cblocks;
};

// The split as a pure function of the shape and the workspace size (host arithmetic only; udp_debug_dw_wgrad_plan
// reports it).  UDP_ERR_WORKSPACE when not even one partial fits.
static int dw_wgrad_plan(int n, int hout, int wout, int C, size_t workspace_bytes, DwWgradPlan* pl) {
  if (n <= 0 || hout <= 0 || wout <= 0 || C <= 0 || (C & 3)) return fail(UDP_ERR_ARG, "dw wgrad plan: %dx%d x%d C%d (C %% 4)", hout, wout, n, C);
  const long R = (long)n * hout;
  if (R >= (1L << 31) || R * wout >= (1L << 31)) return fail(UDP_ERR_UNSUPPORTED, "dw wgrad plan: %ld output rows", R);
  const size_t per = (size_t)9 * C * sizeof(float);
  long pmax = (long)(workspace_bytes / per);
  if (pmax < 1) return fail(UDP_ERR_WORKSPACE, "dw wgrad plan: workspace %zu B holds no [9][%d] partial (%zu B)", workspace_bytes, C, per);
  if (pmax > kDwMaxPartials) pmax = kDwMaxPartials;
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

template <int S>
__global__ __launch_bounds__(256) void dw3_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N,
                                                               int H, int W, int C, int Ho, int Wo, int rows, int cgw, int cgw_shift,
                                                               float* __restrict__ ws) {
  __shared__ float sAcc[256 * 36];
  const int t = threadIdx.x;
  const int lc = t & (cgw - 1), lp = t >> cgw_shift, PL = 256 >> cgw_shift;
  const int cg = blockIdx.y * cgw + lc;                   // channel group of this thread
  const bool live = cg < (C >> 2);
  const int c = cg * 4;
  const long R = (long)N * Ho;
  const long r0 = (long)blockIdx.x * rows;
  const long r1 = r0 + rows < R ? r0 + rows : R;
  const int npix = (int)(r1 - r0) * Wo;
  float acc[9][4];
#pragma unroll
  for (int k = 0; k < 9; ++k)
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
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * S + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * S + kx - 1;
          if (ix < 0 || ix >= W) continue;
          const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + iy) * W + ix) * C + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ky * 3 + kx][e] = __builtin_fmaf(d[e], v[e], acc[ky * 3 + kx][e]);
        }
      }
    }
  }
  // sAcc[lp][tap][lc * 4 + e]: the combining threads below read consecutive floats
  const int span = cgw * 4;
#pragma unroll
  for (int k = 0; k < 9; ++k)
    *reinterpret_cast<f32x4*>(sAcc + (lp * 9 + k) * span + lc * 4) = f32x4{acc[k][0], acc[k][1], acc[k][2], acc[k][3]};
  __syncthreads();
  float* out = ws + (size_t)blockIdx.x * 9 * C;
  for (int o = t; o < 9 * span; o += 256) {
    const int k = o / span, cc = o - k * span;
    const int ch = blockIdx.y * span + cc;
    if (ch >= C) continue;
    float s = sAcc[k * span + cc];
    for (int l = 1; l < PL; ++l) s += sAcc[(l * 9 + k) * span + cc];
    out[k * C + ch] = s;
  }
}

__global__ __launch_bounds__(256) void dw3_wgrad_reduce_kernel(const float* __restrict__ ws, int partials, int C, int Creal,
                                                              float* __restrict__ dw) {
  const int o = blockIdx.x * 256 + threadIdx.x;           // = c * 9 + tap of the parameter layout
  if (o >= Creal * 9) return;
  const int c = o / 9, k = o - c * 9;
  float s = ws[k * C + c];
  for (int p = 1; p < partials; ++p) s += ws[((size_t)p * 9 + k) * C + c];
  dw[o] = s;
}

// ---------------------------------------------------------------------------------------------
// PixelShuffle(2), torch's order: out[n, 2h+i, 2w+j, c] = in[n, h, w, 4c + 2i + j].  thread = one input pixel x 16
// input channels = 4 output channels of each of the four output pixels: four 16-byte loads, a 4x4 transpose in
// registers, four 16-byte stores.  Integer registers: bit patterns are moved, never decoded.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pixshuf2_train_kernel(const unsigned* __restrict__ src, int N, int H, int W, int Cin,
                                                            unsigned* __restrict__ dst, int backward) {
  const int G = Cin >> 4, Co = Cin >> 2;
  const long total = (long)N * H * W * G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx % G);
    const long pix = idx / G;
    const int wx = (int)(pix % W);
    const long r = pix / W;                               // = n * H + h
    const size_t lo = (size_t)pix * Cin + 16 * g;         // the 16 channels of the low-resolution pixel
    u32x4 a[4], b[4];
    if (!backward) {
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = *reinterpret_cast<const u32x4*>(src + lo + 4 * e);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        a[q] = *reinterpret_cast<const u32x4*>(src + ((2 * r + (q >> 1)) * (size_t)(2 * W) + 2 * wx + (q & 1)) * Co + 4 * g);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) b[q][e] = a[e][q];
    if (!backward) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<u32x4*>(dst + ((2 * r + (q >> 1)) * (size_t)(2 * W) + 2 * wx + (q & 1)) * Co + 4 * g) = b[q];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) *reinterpret_cast<u32x4*>(dst + lo + 4 * e) = b[e];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// cat + channel_shuffle on a pair of halves.  logical[j] = a[j] (j < r) | b[j - r]; even[k] = logical[2k],
// odd[k] = logical[2k + 1] for k < r, zeros up to cp.  Scalar element reads (r need not be a multiple of 4), 16-byte
// stores.  Integer registers again.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shuffle_pair_fwd_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b, long M,
                                                              int r, int in_pitch, int cp, unsigned* __restrict__ even,
                                                              unsigned* __restrict__ odd) {
  const int G = cp >> 2;
  const long total = M * G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int k0 = (int)(idx % G) * 4;
    const long pix = idx / G;
    const unsigned* pa = a + (size_t)pix * in_pitch;
    const unsigned* pb = b + (size_t)pix * in_pitch;
    u32x4 ve = {0u, 0u, 0u, 0u}, vo = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + e;
      if (k < r) {
        const int j0 = 2 * k, j1 = 2 * k + 1;
        ve[e] = j0 < r ? pa[j0] : pb[j0 - r];
        vo[e] = j1 < r ? pa[j1] : pb[j1 - r];
      }
    }
    *reinterpret_cast<u32x4*>(even + (size_t)pix * cp + k0) = ve;
    *reinterpret_cast<u32x4*>(odd + (size_t)pix * cp + k0) = vo;
  }
}

// d_logical[j] = (j even ? d_even : d_odd)[j / 2]; d_a[j] = d_logical[j], d_b[j] = d_logical[r + j] for j < r, zeros up
// to out_pitch.
__global__ __launch_bounds__(256) void shuffle_pair_bwd_kernel(const unsigned* __restrict__ d_even, const unsigned* __restrict__ d_odd,
                                                              long M, int r, int cp, int out_pitch, unsigned* __restrict__ d_a,
                                                              unsigned* __restrict__ d_b) {
  const int G = out_pitch >> 2;
  const long total = M * G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int j0 = (int)(idx % G) * 4;
    const long pix = idx / G;
    const unsigned* pe = d_even + (size_t)pix * cp;
    const unsigned* po = d_odd + (size_t)pix * cp;
    u32x4 va = {0u, 0u, 0u, 0u}, vb = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      if (j < r) {
        const int ja = j, jb = r + j;
        va[e] = (ja & 1) ? po[ja >> 1] : pe[ja >> 1];
        vb[e] = (jb & 1) ? po[jb >> 1] : pe[jb >> 1];
      }
    }
    *reinterpret_cast<u32x4*>(d_a + (size_t)pix * out_pitch + j0) = va;
    *reinterpret_cast<u32x4*>(d_b + (size_t)pix * out_pitch + j0) = vb;
  }
}

// y[:, :ra] = a, y[:, ra:ra+rb] = b, zeros up to C
__global__ __launch_bounds__(256) void chan_cat2_kernel(const unsigned* __restrict__ a, int pa, int ra, const unsigned* __restrict__ b,
                                                       int pb, int rb, long M, int C, unsigned* __restrict__ y) {
  const int G = C >> 2;
  const long total = M * G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c0 = (int)(idx % G) * 4;
    const long pix = idx / G;
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      if (c < ra) v[e] = a[(size_t)pix * pa + c];
      else if (c < ra + rb) v[e] = b[(size_t)pix * pb + c - ra];
    }
    *reinterpret_cast<u32x4*>(y + (size_t)pix * C + c0) = v;
  }
}

// a = y[:, :ra] (zeros up to pa), b = y[:, ra:ra+rb] (zeros up to pb); the first pa / 4 groups of a pixel write a
__global__ __launch_bounds__(256) void chan_uncat2_kernel(const unsigned* __restrict__ y, int C, long M, unsigned* __restrict__ a, int pa,
                                                         int ra, unsigned* __restrict__ b, int pb, int rb) {
  const int Ga = pa >> 2, G = (pa + pb) >> 2;
  const long total = M * G;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx % G);
    const long pix = idx / G;
    const bool first = g < Ga;
    const int c0 = (first ? g : g - Ga) * 4;
    const int real = first ? ra : rb, base = first ? 0 : ra;
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c0 + e < real) v[e] = y[(size_t)pix * C + base + c0 + e];
    unsigned* dst = first ? a + (size_t)pix * pa : b + (size_t)pix * pb;
    *reinterpret_cast<u32x4*>(dst + c0) = v;
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

static int dw_check(const char* who, const void* a, const void* b, const void* c, int n, int hin, int win, int C, int Creal,
                    int stride, int dtype) {
  if (!a || !b || !c) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (stride != 1 && stride != 2) return fail(UDP_ERR_UNSUPPORTED, "%s: stride %d (1 or 2)", who, stride);
  if (n <= 0 || hin <= 0 || win <= 0 || C <= 0 || (C & 3) || Creal <= 0 || Creal > C)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, C %d (C %% 4), C_real %d (1..C)", who, hin, win, n, C, Creal);
  if ((long)n * hin * win * C >= (1L << 40)) return fail(UDP_ERR_UNSUPPORTED, "%s: %dx%d x%d C%d is too large", who, hin, win, n, C);
  return UDP_OK;
}

static int move_check(const char* who, const void* a, const void* b, int dtype) {
  if (!a || !b) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  return UDP_OK;
}

}  // namespace udp

using namespace udp;

extern "C" int udp_dwconv3_train_fwd(const void* x, const void* w, int n, int hin, int win, int c, int c_real, int stride,
                                     int dtype, void* y, void* stream) {
  if (const int rc = dw_check("udp_dwconv3_train_fwd", x, w, y, n, hin, win, c, c_real, stride, dtype)) return rc;
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  const long total = (long)n * ho * wo * (c / 4);
  const unsigned blocks = blocks_for(total, 256, 1 << 20);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *xp = reinterpret_cast<const float*>(x), *wp = reinterpret_cast<const float*>(w);
  if (stride == 1) dw3_train_fwd_kernel<1><<<blocks, 256, 0, s>>>(xp, wp, n, hin, win, c, c_real, ho, wo, reinterpret_cast<float*>(y));
  else dw3_train_fwd_kernel<2><<<blocks, 256, 0, s>>>(xp, wp, n, hin, win, c, c_real, ho, wo, reinterpret_cast<float*>(y));
  return launched("udp_dwconv3_train_fwd");
}

extern "C" int udp_dwconv3_dgrad(const void* dy, const void* w, int n, int hin, int win, int c, int c_real, int stride,
                                 int accumulate, int dtype, void* dx, void* stream) {
  if (const int rc = dw_check("udp_dwconv3_dgrad", dy, w, dx, n, hin, win, c, c_real, stride, dtype)) return rc;
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  const long total = (long)n * hin * win * (c / 4);
  const unsigned blocks = blocks_for(total, 256, 1 << 20);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *dp = reinterpret_cast<const float*>(dy), *wp = reinterpret_cast<const float*>(w);
  if (stride == 1) dw3_dgrad_kernel<1><<<blocks, 256, 0, s>>>(dp, wp, n, hin, win, c, c_real, ho, wo, accumulate != 0, reinterpret_cast<float*>(dx));
  else dw3_dgrad_kernel<2><<<blocks, 256, 0, s>>>(dp, wp, n, hin, win, c, c_real, ho, wo, accumulate != 0, reinterpret_cast<float*>(dx));
  return launched("udp_dwconv3_dgrad");
}

extern "C" size_t udp_dwconv3_wgrad_workspace_bytes(int n, int hout, int wout, int c) {
  DwWgradPlan pl;
  if (dw_wgrad_plan(n, hout, wout, c, (size_t)kDwMaxPartials * 9 * (c > 0 ? c : 1) * sizeof(float), &pl)) return 0;
  return (size_t)pl.partials * 9 * c * sizeof(float);
}

extern "C" int udp_debug_dw_wgrad_plan(int n, int hout, int wout, int c, size_t workspace_bytes, int* out) {
  if (!out) return fail(UDP_ERR_ARG, "udp_debug_dw_wgrad_plan: null pointer");
  DwWgradPlan pl;
  if (const int rc = dw_wgrad_plan(n, hout, wout, c, workspace_bytes, &pl)) return rc;
  out[0] = pl.rows;
  out[1] = pl.partials * pl.cblocks;
  out[2] = pl.partials;
  out[3] = kDwLdsBytes;
  return UDP_OK;
}

extern "C" int udp_dwconv3_wgrad(const void* x, const void* dy, int n, int hin, int win, int c, int c_real, int stride, int dtype,
                                 void* dw, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = dw_check("udp_dwconv3_wgrad", x, dy, dw, n, hin, win, c, c_real, stride, dtype)) return rc;
  if (!workspace) return fail(UDP_ERR_ARG, "udp_dwconv3_wgrad: null pointer");
  const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;
  DwWgradPlan pl;
  if (const int rc = dw_wgrad_plan(n, ho, wo, c, workspace_bytes, &pl)) return rc;
  int shift = 3;
  while ((1 << shift) < pl.cgw) ++shift;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float *xp = reinterpret_cast<const float*>(x), *dp = reinterpret_cast<const float*>(dy);
  float* ws = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)pl.partials, (unsigned)pl.cblocks);
  if (stride == 1) dw3_wgrad_partial_kernel<1><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  else dw3_wgrad_partial_kernel<2><<<grid, 256, 0, s>>>(xp, dp, n, hin, win, c, ho, wo, pl.rows, pl.cgw, shift, ws);
  if (const int rc = launched("udp_dwconv3_wgrad")) return rc;
  dw3_wgrad_reduce_kernel<<<ceil_div(c_real * 9, 256), 256, 0, s>>>(ws, pl.partials, c, c_real, reinterpret_cast<float*>(dw));
  return launched("udp_dwconv3_wgrad");
}

static int pixshuf_train(const char* who, const void* src, int n, int h, int w, int cin, int dtype, void* dst, int backward, void* stream) {
  if (const int rc = move_check(who, src, dst, dtype)) return rc;
  if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin % 64)
    return fail(UDP_ERR_ARG, "%s: %dx%d x%d, %d channels before the shuffle (a multiple of 64)", who, h, w, n, cin);
  const long total = (long)n * h * w * (cin / 16);
  pixshuf2_train_kernel<<<blocks_for(total, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const unsigned*>(src), n, h, w, cin, reinterpret_cast<unsigned*>(dst), backward);
  return launched(who);
}

extern "C" int udp_pixshuf2_train_fwd(const void* x, int n, int h, int w, int cin, int dtype, void* y, void* stream) {
  return pixshuf_train("udp_pixshuf2_train_fwd", x, n, h, w, cin, dtype, y, 0, stream);
}

extern "C" int udp_pixshuf2_train_bwd(const void* dy, int n, int h, int w, int cin, int dtype, void* dx, void* stream) {
  return pixshuf_train("udp_pixshuf2_train_bwd", dy, n, h, w, cin, dtype, dx, 1, stream);
}

extern "C" int udp_shuffle_pair_fwd(const void* a, const void* b, int64_t m, int r, int in_pitch, int cp, int dtype, void* even,
                                    void* odd, void* stream) {
  if (const int rc = move_check("udp_shuffle_pair_fwd", a, b, dtype)) return rc;
  if (!even || !odd) return fail(UDP_ERR_ARG, "udp_shuffle_pair_fwd: null pointer");
  if (m <= 0 || r <= 0 || in_pitch < r || cp < r || (cp & 3))
    return fail(UDP_ERR_ARG, "udp_shuffle_pair_fwd: m %ld, r %d, pitches %d -> %d (>= r, out %% 4)", m, r, in_pitch, cp);
  shuffle_pair_fwd_kernel<<<blocks_for(m * (cp / 4), 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const unsigned*>(a), reinterpret_cast<const unsigned*>(b), m, r, in_pitch, cp,
      reinterpret_cast<unsigned*>(even), reinterpret_cast<unsigned*>(odd));
  return launched("udp_shuffle_pair_fwd");
}

extern "C" int udp_shuffle_pair_bwd(const void* d_even, const void* d_odd, int64_t m, int r, int cp, int out_pitch, int dtype,
                                    void* d_a, void* d_b, void* stream) {
  if (const int rc = move_check("udp_shuffle_pair_bwd", d_even, d_odd, dtype)) return rc;
  if (!d_a || !d_b) return fail(UDP_ERR_ARG, "udp_shuffle_pair_bwd: null pointer");
  if (m <= 0 || r <= 0 || cp < r || out_pitch < r || (out_pitch & 3))
    return fail(UDP_ERR_ARG, "udp_shuffle_pair_bwd: m %ld, r %d, pitches %d -> %d (>= r, out %% 4)", m, r, cp, out_pitch);
  shuffle_pair_bwd_kernel<<<blocks_for(m * (out_pitch / 4), 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const unsigned*>(d_even), reinterpret_cast<const unsigned*>(d_odd), m, r, cp, out_pitch,
      reinterpret_cast<unsigned*>(d_a), reinterpret_cast<unsigned*>(d_b));
  return launched("udp_shuffle_pair_bwd");
}

static int cat_check(const char* who, long m, int pa, int ra, int pb, int rb, int c) {
  if (m <= 0 || ra <= 0 || rb <= 0 || pa < ra || pb < rb || c < ra + rb || (c & 3))
    return fail(UDP_ERR_ARG, "%s: m %ld, %d(%d) + %d(%d) <-> %d (pitches >= channels, whole %% 4)", who, m, ra, pa, rb, pb, c);
  return UDP_OK;
}

extern "C" int udp_chan_cat2(const void* a, int pa, int ra, const void* b, int pb, int rb, int64_t m, int c, int dtype, void* y,
                             void* stream) {
  if (const int rc = move_check("udp_chan_cat2", a, b, dtype)) return rc;
  if (!y) return fail(UDP_ERR_ARG, "udp_chan_cat2: null pointer");
  if (const int rc = cat_check("udp_chan_cat2", m, pa, ra, pb, rb, c)) return rc;
  chan_cat2_kernel<<<blocks_for(m * (c / 4), 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const unsigned*>(a), pa, ra, reinterpret_cast<const unsigned*>(b), pb, rb, m, c, reinterpret_cast<unsigned*>(y));
  return launched("udp_chan_cat2");
}

extern "C" int udp_chan_uncat2(const void* y, int c, int64_t m, int dtype, void* a, int pa, int ra, void* b, int pb, int rb,
                               void* stream) {
  if (const int rc = move_check("udp_chan_uncat2", a, b, dtype)) return rc;
  if (!y) return fail(UDP_ERR_ARG, "udp_chan_uncat2: null pointer");
  if (const int rc = cat_check("udp_chan_uncat2", m, pa, ra, pb, rb, c)) return rc;
  if ((pa & 3) || (pb & 3)) return fail(UDP_ERR_ARG, "udp_chan_uncat2: pitches %d, %d (%% 4)", pa, pb);
  chan_uncat2_kernel<<<blocks_for(m * ((pa + pb) / 4), 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const unsigned*>(y), c, m, reinterpret_cast<unsigned*>(a), pa, ra, reinterpret_cast<unsigned*>(b), pb, rb);
  return launched("udp_chan_uncat2");
}
