// Training kernels of the MobileNetV3-small pose nets (deep_hrnet/lib/models/backbones/mobilenetv3.py:5-16: torchvision's
// mobilenet_v3_small().features; the block table is udp_pose_amd/synth_mobilenetv3.py BLOCKS) for gfx950 that the
// ShuffleNetV2 step (dw_train.hip, shufflenet_train.hip) does not have:
//
//   udp_hswish_fwd / _bwd    nn.Hardswish and its derivative
//   udp_se_train_fwd / _bwd  torchvision.ops.SqueezeExcitation (fc1 / fc2 with biases, ReLU, Hardsigmoid) in train mode
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4: a thread owns 4 consecutive channels and
// moves 16 bytes.  Every kernel writes EVERY stored channel of its outputs (padded channels: exact zeros), there are no
// atomics, and every sum has one order that depends on the shape alone.  The pools and dot products are explicit fmaf
// (the file is compiled without fp contraction, like dw_train.hip).
#include "common.h"

namespace udp {

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
