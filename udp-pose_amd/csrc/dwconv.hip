// Depthwise 3x3 conv + folded BatchNorm (UDP_OP_DWCONV) and PixelShuffle(2) (UDP_OP_PIXSHUF) for gfx950 (MI355X):
// the two ops of pose_shufflenetv2_10x_pixel_shuffle that the conv kernels do not cover
// (deep_hrnet/lib/models/backbones/shufflenetv2.py:54-55, :66-67; decoders/DUC.py:21).  Further down: the 5x5 / 7x7
// depthwise form (dwconvk_kernel) and squeeze-and-excitation (UDP_OP_SE, se_kernel) of the ShuffleNetV2+ backbone.
//
// A depthwise conv has no GEMM in it (9 MACs per output element): it is memory-bound and runs on the VALU.  Lanes run
// along the channels -- a thread owns V consecutive channels (fp32: 4 = one 16-byte load; split fp16: 8 = one 16-byte
// load per plane of the [C hi][C lo] pixel) of one output column and walks DOWN a strip of output rows, so a wave
// reads 64 * 16 contiguous bytes of a pixel (row) at a time.  Vertical reuse is in registers:
//   stride 1: three accumulators are in flight (the output rows iy-1, iy, iy+1 that input row iy feeds with ky = 2,
//             1, 0); an input row is loaded once per strip and leaves with the accumulator it completes;
//   stride 2: input row 2oy+1 is kept for the next output row (its ky = 0 taps), rows 2oy are used once.
// A strip of R output rows loads R + 2 (stride 2: 2R + 1) input rows, so neighbouring strips re-read their halo rows:
// (R + 2) / R of the input per launch -- 1x only when one strip covers the image, 2x at the floor R = 2 that
// describe_dwconv reaches when a small launch needs the threads more than the reuse.
// The three columns of a row are loaded by the thread itself; the neighbouring columns' threads sit in the same
// workgroup and read the same lines at about the same time, so that 3x is expected to hit the L1 / L2 (not measured
// with counters; NOTES.md has the achieved bytes/s against an element-wise kernel moving the same map).  Per output
// element the arithmetic is: bias, then nine fmaf in the order ky, kx -- whatever the strip height, so the result
// does not depend on the launch geometry.  Taps outside the image are SKIPPED (never read, never multiplied by 0).
//
// The shuffle passthrough of a stride-1 ShuffleV2 unit (shufflenetv2.py:77-92) rides in the same launch: the thread
// that stores output pixel (n, y, x), channels c..c+V-1 also copies the V selected channels of the unit's input to
// the unit's output (udp_pose_hip.h, UDP_OP_DWCONV).  A selection: bit patterns are moved, never decoded.
#include "dw_dev.h"

namespace udp {

// the three taps of kernel row KY on one input row; v0 / v2: the left / right column lies inside the image
template <int KY, int V>
__device__ __forceinline__ void dw_row(float (&acc)[V], const float (&x)[3][V], const float (&w)[9][V], bool v0, bool v2) {
  if (v0) {
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = __builtin_fmaf(x[0][k], w[3 * KY][k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = __builtin_fmaf(x[1][k], w[3 * KY + 1][k], acc[k]);
  if (v2) {
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = __builtin_fmaf(x[2][k], w[3 * KY + 2][k], acc[k]);
  }
}

// Shuffle passthrough: destination channels c..c+V-1 (of cin) of pixel `pix` take the even logical channels of the
// source.  The source pixel holds 2r logical channels as two halves of cin (= Cp) stored channels, r real ones
// first: logical j sits at j (j < r) or Cp + j - r.  Destination k < r takes logical 2k, k >= r is zero.
template <typename T>
__device__ __forceinline__ void dw_passthrough(const ConvParams& p, size_t pix, int c) {
  using E = typename DwTr<T>::E;
  using Vec = typename DwTr<T>::Vec;
  constexpr int V = DwTr<T>::V, PL = DwTr<T>::PL;
  const int r = p.up_shift[0], Cp = p.Cin;
#pragma unroll
  for (int pl = 0; pl < PL; ++pl) {
    const E* src = reinterpret_cast<const E*>(p.res) + pix * ((size_t)PL * p.res_pitch) + (size_t)pl * p.res_pitch + p.res_coff;
    E* dst = reinterpret_cast<E*>(p.out2[0]) + pix * ((size_t)PL * p.out2_pitch[0]) + (size_t)pl * p.out2_pitch[0] + p.out2_coff[0] + c;
    Vec o;
    if (2 * c + 2 * V <= r) {           // the whole span lies in the first half: two aligned 16-byte loads
      const Vec a = *reinterpret_cast<const Vec*>(src + 2 * c), b = *reinterpret_cast<const Vec*>(src + 2 * c + V);
#pragma unroll
      for (int e = 0; e < V / 2; ++e) {
        o[e] = a[2 * e];
        o[V / 2 + e] = b[2 * e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int k = c + e, j = 2 * k;
        o[e] = k < r ? src[j < r ? j : Cp + j - r] : (E)0;
      }
    }
    *reinterpret_cast<Vec*>(dst) = o;
  }
}

// thread = (image, row strip, output column, channel group); p.R output rows per strip, p.tiles_y strips per image,
// p.ntiles threads in all
template <typename T, int S, bool SILU = false>      // SILU: + SiLU instead of the ReLU (UDP_ACT_SILU)
__global__ __launch_bounds__(256) void dwconv3_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)p.ntiles) return;
  const int cgs = p.Cin / V;
  const int c = (int)(idx % cgs) * V;
  idx /= cgs;
  const int ox = (int)(idx % p.Wout);
  idx /= p.Wout;
  const int st = (int)(idx % p.tiles_y);
  const int n = (int)(idx / p.tiles_y);
  const int oy0 = st * p.R;
  const int oy1 = oy0 + p.R < p.Hout ? oy0 + p.R : p.Hout;

  float w[9][V], b[V];
  const float* wg = reinterpret_cast<const float*>(p.wgt);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(wg + (size_t)t * p.Cin + c + q);
      w[t][q] = v[0], w[t][q + 1] = v[1], w[t][q + 2] = v[2], w[t][q + 3] = v[3];
    }
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.bias + c + q);
    b[q] = v[0], b[q + 1] = v[1], b[q + 2] = v[2], b[q + 3] = v[3];
  }

  const int ix0 = ox * S - 1;                       // column of tap kx = 0; kx = 1 is always inside
  const bool v0 = ix0 >= 0, v2 = ix0 + 2 < p.Win;
  const size_t img_in = (size_t)n * p.Hin * p.Win, img_out = (size_t)n * p.Hout * p.Wout;
  auto load_row = [&](int iy, float (&x)[3][V]) __attribute__((always_inline)) {
    const size_t pix = img_in + (size_t)iy * p.Win + ox * S;      // the centre column
#pragma unroll
    for (int k = 0; k < V; ++k) x[0][k] = x[2][k] = 0.f;          // never used when outside (dw_row skips the tap)
    if (v0) dw_load<T, V>(p, pix - 1, c, x[0]);
    dw_load<T, V>(p, pix, c, x[1]);
    if (v2) dw_load<T, V>(p, pix + 1, c, x[2]);
  };
  auto finish = [&](int oy, const float (&a)[V]) __attribute__((always_inline)) {
    const size_t pix = img_out + (size_t)oy * p.Wout + ox;
    dw_store<T, V, SILU>(p, pix, c, a);
    if (p.nout2) dw_passthrough<T>(p, pix, c);
  };

  if constexpr (S == 1) {
    float a0[V], a1[V], a2[V];                      // output rows iy-1 (ky = 2 next), iy (ky = 1), iy+1 (ky = 0)
#pragma unroll
    for (int k = 0; k < V; ++k) a0[k] = a1[k] = a2[k] = b[k];
    for (int iy = oy0 - 1; iy <= oy1; ++iy) {
      if (iy >= 0 && iy < p.Hin) {
        float x[3][V];
        load_row(iy, x);
        dw_row<2, V>(a0, x, w, v0, v2);
        dw_row<1, V>(a1, x, w, v0, v2);
        dw_row<0, V>(a2, x, w, v0, v2);
      }
      if (iy - 1 >= oy0) finish(iy - 1, a0);        // (iy - 1 < oy1 by the loop bound)
#pragma unroll
      for (int k = 0; k < V; ++k) a0[k] = a1[k], a1[k] = a2[k], a2[k] = b[k];
    }
  } else {
    float xp[3][V];                                 // input row 2oy-1: ky = 2 of row oy-1, ky = 0 of row oy
    bool have = 2 * oy0 - 1 >= 0;
    if (have) load_row(2 * oy0 - 1, xp);
    for (int oy = oy0; oy < oy1; ++oy) {
      float a[V], x[3][V];
#pragma unroll
      for (int k = 0; k < V; ++k) a[k] = b[k];
      if (have) dw_row<0, V>(a, xp, w, v0, v2);
      load_row(2 * oy, x);                          // 2oy <= Hin - 1 by hout = (hin - 1) / 2 + 1
      dw_row<1, V>(a, x, w, v0, v2);
      have = 2 * oy + 1 < p.Hin;
      if (have) {
        load_row(2 * oy + 1, xp);
        dw_row<2, V>(a, xp, w, v0, v2);
      }
      finish(oy, a);
    }
  }
}

// Depthwise K x K, K = 5 | 7 (ShuffleNetV2+ units, backbones/shufflenetv2_plus.py:97, :119).  The register scheme of
// dwconv3_kernel does not stretch: 49 taps x 8 channels of weights alone are 392 VGPRs.  Here a thread owns ONE
// output pixel x V channels and holds ONE kernel row of weights (K x V <= 56 registers) at a time: the ky loop is
// rolled, the kx loop unrolled; a tap costs PL input loads + V / 4 weight loads of 16 bytes, all of which hit the
// L1 / L2 (the maps where K > 3 occurs are 64 x 48 and smaller, the weights K * K * C * 4 bytes).  Same arithmetic
// contract as above: bias, then one fmaf per tap in the order ky, kx, taps outside the image skipped.
// thread = (image, output row, output column, channel group); p.ntiles threads in all
template <typename T, int S, int K, bool SILU = false>
__global__ __launch_bounds__(256) void dwconvk_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V, PAD = K / 2;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)p.ntiles) return;
  const int cgs = p.Cin / V;
  const int c = (int)(idx % cgs) * V;
  idx /= cgs;
  const int ox = (int)(idx % p.Wout);
  idx /= p.Wout;
  const int oy = (int)(idx % p.Hout);
  const int n = (int)(idx / p.Hout);
  const float* wg = reinterpret_cast<const float*>(p.wgt) + c;
  float a[V];
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p.bias + c + q);
    a[q] = v[0], a[q + 1] = v[1], a[q + 2] = v[2], a[q + 3] = v[3];
  }
  const int ix0 = ox * S - PAD;
  const size_t img_in = (size_t)n * p.Hin * p.Win;
#pragma unroll 1
  for (int ky = 0; ky < K; ++ky) {
    const int iy = oy * S - PAD + ky;
    if (iy < 0 || iy >= p.Hin) continue;
    const size_t row = img_in + (size_t)iy * p.Win;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = ix0 + kx;
      if (ix >= 0 && ix < p.Win) {
        float x[V], w[V];
        dw_load<T, V>(p, row + ix, c, x);
#pragma unroll
        for (int q = 0; q < V; q += 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(wg + (size_t)(ky * K + kx) * p.Cin + q);
          w[q] = v[0], w[q + 1] = v[1], w[q + 2] = v[2], w[q + 3] = v[3];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = __builtin_fmaf(x[k], w[k], a[k]);
      }
    }
  }
  const size_t pix = ((size_t)n * p.Hout + oy) * p.Wout + ox;
  dw_store<T, V, SILU>(p, pix, c, a);
  if (p.nout2) dw_passthrough<T>(p, pix, c);
}

// Squeeze-and-excitation (UDP_OP_SE; SELayer, backbones/shufflenetv2_plus.py:34-60) on an NHWC view of C = p.Cin
// stored channels: one workgroup per image, four phases separated by barriers --
//   1. mean[c] over the HW pixels: thread (pixel group g, channel group) adds pixels g, g + P, ... in that order,
//      then the P partial sums of a channel are added in the order g = 0 .. P-1 and multiplied by 1 / HW;
//   2. h[j] = relu(b1[j] + sum_c W1[c][j] mean[c]), j < Ch = p.up_shift[0]: the channel range is cut into Q equal
//      parts, thread (part, j) runs its part with fmaf in channel order, the parts are added in order onto b1[j];
//   3. m[c] = clamp(sum_j W2[j][c] h[j] + 3, 0, 6) / 6, fmaf from 0 in the order j = 0 .. Ch-1;
//   4. out = in * m[c], every element by one thread.
// P and Q depend on (C, Ch) only and nothing is atomic: an image's result does not depend on the batch, the lane
// or graph replay.  The pool is complete before the first store, and an element is read and written by the same
// thread, so `out` may be the very view `in` is.  Parameter block (fp32): W1 [C][Ch], b1 [Ch], W2 [Ch][C].
// Dynamic LDS: (256 * V + 2 * C + 256 + Ch) floats.
template <typename T>
__global__ __launch_bounds__(256) void se_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  extern __shared__ __attribute__((aligned(16))) float se_s[];
  const int C = p.Cin, Ch = p.up_shift[0], HW = p.Hin * p.Win;
  float* part = se_s;                  // [P][C], P * C <= 256 * V
  float* mean = part + 256 * V;        // [C]
  float* mul = mean + C;               // [C]
  float* hpart = mul + C;              // [Q][Ch], Q * Ch <= 256
  float* hid = hpart + 256;            // [Ch]
  const int tid = threadIdx.x;
  const size_t img = (size_t)blockIdx.x * HW;
  const int cgs = C / V;
  const int P = 256 / cgs < HW ? 256 / cgs : HW;        // cgs <= 128 (dwconv_validate / se_validate: C <= 512)
  {
    const int cg = tid % cgs, g = tid / cgs;
    if (g < P) {
      float s[V];
#pragma unroll
      for (int k = 0; k < V; ++k) s[k] = 0.f;
      for (int px = g; px < HW; px += P) {
        float x[V];
        dw_load<T, V>(p, img + px, cg * V, x);
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] += x[k];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) part[g * C + cg * V + k] = s[k];
    }
  }
  __syncthreads();
  const float inv = 1.f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    float s = part[c];
    for (int g = 1; g < P; ++g) s += part[g * C + c];
    mean[c] = s * inv;
  }
  __syncthreads();
  const float* w1 = reinterpret_cast<const float*>(p.wgt);
  const float* b1 = w1 + (size_t)C * Ch;
  const float* w2 = b1 + Ch;
  const int Q = 256 / Ch < C ? 256 / Ch : C;            // Ch <= 256
  const int L = (C + Q - 1) / Q;
  {
    const int j = tid % Ch, q = tid / Ch;
    if (q < Q) {
      const int c1 = (q + 1) * L < C ? (q + 1) * L : C;
      float s = 0.f;
      for (int c = q * L; c < c1; ++c) s = __builtin_fmaf(w1[(size_t)c * Ch + j], mean[c], s);
      hpart[q * Ch + j] = s;
    }
  }
  __syncthreads();
  if (tid < Ch) {
    float s = b1[tid];
    for (int q = 0; q < Q; ++q) s += hpart[q * Ch + tid];
    hid[tid] = __builtin_fmaxf(s, 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int j = 0; j < Ch; ++j) s = __builtin_fmaf(w2[(size_t)j * C + c], hid[j], s);
    mul[c] = __builtin_fminf(__builtin_fmaxf(s + 3.f, 0.f), 6.f) / 6.f;
  }
  __syncthreads();
  for (int e = tid; e < HW * cgs; e += 256) {
    const int cg = e % cgs, px = e / cgs;
    float x[V];
    dw_load<T, V>(p, img + px, cg * V, x);
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] *= mul[cg * V + k];
    dw_store<T, V>(p, img + px, cg * V, x);
  }
}

// Activation + squeeze-and-excitation with both biases (UDP_OP_SE_ACT; torchvision's SqueezeExcitation behind the
// depthwise conv + BatchNorm + activation of a MobileNetV3 InvertedResidual) on an NHWC view of C = p.Cin stored
// channels, C up to 1024: se_kernel's four phases with a[p][c] = act(in[p][c]) in place of in[p][c] in the pool and
// in the scale, b2 added in phase 3, and the pool's partial sums sized from C --
//   1. P = max(1, 256 / (C / V)) pixel groups (at most HW): thread (g, channel group) adds act(in) of pixels g, g + P,
//      ... in that order; the P partial sums of a channel are added in the order g = 0 .. P-1, times 1 / HW.  Beyond
//      128 channel groups (C = 576 in fp32: 144) P is 1: a thread walks every pixel and the other threads sit idle;
//   2. h[j] = relu(b1[j] + sum_c W1[c][j] mean[c]) exactly as se_kernel (Q channel parts, added in part order);
//   3. m[c] = clamp((sum_j W2[j][c] h[j]) + b2[c] + 3, 0, 6) / 6, fmaf from 0 in the order j = 0 .. Ch-1;
//   4. out = act(in) * m[c], every element by one thread (so `out` may be the very view `in` is).
// ACT = udp_conv_op.relu: UDP_ACT_NONE | UDP_ACT_RELU | UDP_ACT_HSWISH (describe_se_act clears p.relu: dw_store must not
// put a ReLU behind the product -- hswish(v) * m is negative for -3 < v < 0).  Parameter block (fp32): W1 [C][Ch],
// b1 [Ch], W2 [Ch][C], b2 [C].  Dynamic LDS: (P * C + 2 * C + 256 + Ch) floats, P before the clamp to HW.
static_assert(UDP_OP_SE_ACT == 23, "udp_pose_hip.h: UDP_OP_SE_ACT follows UDP_OP_PRM_DW9 (_lib.py binds 23)");

template <int ACT>
__device__ __forceinline__ float se_act_in(float v) {
  if constexpr (ACT == UDP_ACT_RELU) return __builtin_fmaxf(v, 0.f);
  else if constexpr (ACT == UDP_ACT_HSWISH) return hswish(v);
  else return v;
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void se_act_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  extern __shared__ __attribute__((aligned(16))) float se_s[];
  const int C = p.Cin, Ch = p.up_shift[0], HW = p.Hin * p.Win;
  const int cgs = C / V;                                    // <= 256 (se_act_validate: C <= 1024)
  const int P0 = 256 / cgs > 1 ? 256 / cgs : 1;
  float* part = se_s;                  // [P0][C]
  float* mean = part + (size_t)P0 * C; // [C]
  float* mul = mean + C;               // [C]
  float* hpart = mul + C;              // [Q][Ch], Q * Ch <= 256
  float* hid = hpart + 256;            // [Ch]
  const int tid = threadIdx.x;
  const size_t img = (size_t)blockIdx.x * HW;
  const int P = P0 < HW ? P0 : HW;
  {
    const int cg = tid % cgs, g = tid / cgs;
    if (g < P) {
      float s[V];
#pragma unroll
      for (int k = 0; k < V; ++k) s[k] = 0.f;
      for (int px = g; px < HW; px += P) {
        float x[V];
        dw_load<T, V>(p, img + px, cg * V, x);
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] += se_act_in<ACT>(x[k]);
      }
#pragma unroll
      for (int k = 0; k < V; ++k) part[g * C + cg * V + k] = s[k];
    }
  }
  __syncthreads();
  const float inv = 1.f / (float)HW;
  for (int c = tid; c < C; c += 256) {
    float s = part[c];
    for (int g = 1; g < P; ++g) s += part[g * C + c];
    mean[c] = s * inv;
  }
  __syncthreads();
  const float* w1 = reinterpret_cast<const float*>(p.wgt);
  const float* b1 = w1 + (size_t)C * Ch;
  const float* w2 = b1 + Ch;
  const float* b2 = w2 + (size_t)Ch * C;
  const int Q = 256 / Ch < C ? 256 / Ch : C;            // Ch <= 256
  const int L = (C + Q - 1) / Q;
  {
    const int j = tid % Ch, q = tid / Ch;
    if (q < Q) {
      const int c0 = q * L < C ? q * L : C, c1 = (q + 1) * L < C ? (q + 1) * L : C;
      float s = 0.f;
      for (int c = c0; c < c1; ++c) s = __builtin_fmaf(w1[(size_t)c * Ch + j], mean[c], s);
      hpart[q * Ch + j] = s;
    }
  }
  __syncthreads();
  if (tid < Ch) {
    float s = b1[tid];
    for (int q = 0; q < Q; ++q) s += hpart[q * Ch + tid];
    hid[tid] = __builtin_fmaxf(s, 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int j = 0; j < Ch; ++j) s = __builtin_fmaf(w2[(size_t)j * C + c], hid[j], s);
    mul[c] = __builtin_fminf(__builtin_fmaxf(s + b2[c] + 3.f, 0.f), 6.f) / 6.f;
  }
  __syncthreads();
  for (int e = tid; e < HW * cgs; e += 256) {
    const int cg = e % cgs, px = e / cgs;
    float x[V];
    dw_load<T, V>(p, img + px, cg * V, x);
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] = se_act_in<ACT>(x[k]) * mul[cg * V + k];
    dw_store<T, V>(p, img + px, cg * V, x);
  }
}

// PixelShuffle(2) on NHWC with the four sub-pixel groups contiguous per pixel: group g = 2i + j (cout channels from
// g * cout) of input pixel (h, w) -> output pixel (2h + i, 2w + j).  thread = (image, h, w, g, channel group).
template <typename T>
__global__ __launch_bounds__(256) void pixshuf2_kernel(const ConvParams p) {
  using E = typename DwTr<T>::E;
  using Vec = typename DwTr<T>::Vec;
  constexpr int V = DwTr<T>::V, PL = DwTr<T>::PL;
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)p.ntiles) return;
  const int cgs = p.Cout / V;
  const int c = (int)(idx % cgs) * V;
  idx /= cgs;
  const int g = (int)(idx & 3);
  idx >>= 2;
  const int x = (int)(idx % p.Win);
  idx /= p.Win;
  const int y = (int)(idx % p.Hin);
  const int n = (int)(idx / p.Hin);
  const size_t pin = ((size_t)n * p.Hin + y) * p.Win + x;
  const size_t pout = ((size_t)n * p.Hout + 2 * y + (g >> 1)) * p.Wout + 2 * x + (g & 1);
#pragma unroll
  for (int pl = 0; pl < PL; ++pl) {
    const E* src = reinterpret_cast<const E*>(p.in) + pin * ((size_t)PL * p.in_pitch) + (size_t)pl * p.in_pitch + p.in_coff + g * p.Cout + c;
    E* dst = reinterpret_cast<E*>(p.out) + pout * ((size_t)PL * p.out_pitch) + (size_t)pl * p.out_pitch + p.out_coff + c;
    *reinterpret_cast<Vec*>(dst) = *reinterpret_cast<const Vec*>(src);
  }
}

// ---------------------------------------------------------------------------------------------- host side
// Shape / field rules of the two kinds (udp_pose_hip.h), shared by udp_hrnet_create and udp_conv2d_fused.
int dwconv_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "depthwise conv: dtype %d", dtype);
  if ((o.ks != 3 && o.ks != 5 && o.ks != 7) || (o.stride != 1 && o.stride != 2) || o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cout_pad != o.cout)
    return fail(UDP_ERR_ARG, "depthwise conv: 3x3 | 5x5 | 7x7, stride 1 | 2, cin == cout == cout_pad, a multiple of 32 (k%d C%d->%d)", o.ks, o.cin, o.cout);
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "depthwise conv: activation code %d", o.relu);
  if (o.relu == UDP_ACT_HSWISH) return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: no hard-swish epilogue (activation code 2)");
  if (o.hin < 1 || o.win < 1 || o.hout != (o.hin - 1) / o.stride + 1 || o.wout != (o.win - 1) / o.stride + 1)
    return fail(UDP_ERR_ARG, "depthwise conv: %dx%d -> %dx%d does not match stride %d", o.hin, o.win, o.hout, o.wout, o.stride);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "depthwise conv: channel views");
  if (o.n_up || o.group || o.in_stuff2 || o.wfmt || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: no addends, groups or NCHW output; weights fp32 [ks * ks][C] (wfmt 0)");
  if (o.n_out2 == 0) {
    if (o.chain_cout) return fail(UDP_ERR_ARG, "depthwise conv: chain_cout without a passthrough (n_out2 = 1)");
    return UDP_OK;
  }
  // shuffle passthrough
  const int r = o.chain_cout, rpitch = o.res_pitch, dpitch = o.out2_pitch[0];
  if (o.n_out2 != 1 || o.stride != 1) return fail(UDP_ERR_ARG, "depthwise conv: the passthrough is one second output of a stride-1 launch");
  if (r < 2 || r > o.cin || (r & 1)) return fail(UDP_ERR_ARG, "depthwise conv: passthrough of %d real channels per half of %d", r, o.cin);
  if (o.res_coff < 0 || o.res_coff + 2 * o.cin > rpitch || o.out2_coff[0] < 0 || o.out2_coff[0] + o.cin > dpitch ||
      (o.res_coff | rpitch | o.out2_coff[0] | dpitch) % 8)
    return fail(UDP_ERR_ARG, "depthwise conv: passthrough views (res: 2 x %d channels, out2[0]: %d channels, pitches given)", o.cin, o.cin);
  return UDP_OK;
}

// UDP_OP_SE: cin == cout stored channels (a multiple of 32, at most 512), chain_cout = hidden width (1 .. 256)
int se_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "squeeze-excitation: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "squeeze-excitation: dtype %d", dtype);
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cin > 512 || o.cout_pad != o.cout || o.chain_cout < 1 || o.chain_cout > 256 ||
      o.chain_cout > o.cin || o.hin < 1 || o.win < 1 || o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "squeeze-excitation: cin == cout == cout_pad, a multiple of 32 up to 512, hidden width (chain_cout) 1 .. min(256, cin), "
                "output = input size (C%d->%d, hidden %d)", o.cin, o.cout, o.chain_cout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "squeeze-excitation: channel views");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "squeeze-excitation: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "squeeze-excitation: no addends, activation, second outputs, groups or NCHW output");
  return UDP_OK;
}

// UDP_OP_SE_ACT: cin == cout stored channels (a multiple of 32, 32 .. 1024), chain_cout = hidden width (1 .. min(256, C)),
// relu = the activation applied to the input: 0 | 1 | 2 (hrnet.hip's act_validate has refused code 3 and codes outside 0..4)
int se_act_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "activation + squeeze-excitation: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "activation + squeeze-excitation: dtype %d", dtype);
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "activation + squeeze-excitation: activation code %d", o.relu);
  if (o.relu == UDP_ACT_SILU) return fail(UDP_ERR_UNSUPPORTED, "activation + squeeze-excitation: no SiLU form (activation code 4)");
  if (o.cin < 32 || o.cin != o.cout || o.cin % 32 || o.cin > 1024 || o.cout_pad != o.cout || o.chain_cout < 1 || o.chain_cout > 256 ||
      o.chain_cout > o.cin || o.hin < 1 || o.win < 1 || o.hout != o.hin || o.wout != o.win ||
      (int64_t)o.hin * o.win * (o.cin / 4) >= (1LL << 31))
    return fail(UDP_ERR_ARG, "activation + squeeze-excitation: cin == cout == cout_pad, a multiple of 32 from 32 to 1024, hidden width "
                "(chain_cout) 1 .. min(256, cin), output = input size (C%d->%d, hidden %d)", o.cin, o.cout, o.chain_cout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "activation + squeeze-excitation: channel views");
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "activation + squeeze-excitation: no addends, second outputs, groups, wfmt or NCHW output");
  return UDP_OK;
}

int pixshuf_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "pixel shuffle: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "pixel shuffle: dtype %d", dtype);
  if (o.cout <= 0 || o.cout % 8 || o.cin != 4 * o.cout || o.hin < 1 || o.win < 1 || o.hout != 2 * o.hin || o.wout != 2 * o.win)
    return fail(UDP_ERR_ARG, "pixel shuffle: C%d %dx%d -> C%d %dx%d (cin = 4 cout, cout %% 8 == 0, output = 2x the input)", o.cin, o.hin,
                o.win, o.cout, o.hout, o.wout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
    return fail(UDP_ERR_ARG, "pixel shuffle: channel views");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "pixel shuffle: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.chain_cout || o.group || o.in_stuff2 || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "pixel shuffle: pure data movement (no addends, ReLU, second outputs or NCHW output)");
  return UDP_OK;
}

// p: geometry, views, in / out / wgt / bias set; passthrough: nout2 = 1, res, res_pitch / res_coff, out2[0],
// out2_pitch[0] / out2_coff[0], up_shift[0] = real channels per half.
int describe_dwconv(ConvParams p, int dtype, int ks, int stride, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt || !p.bias || (p.nout2 && (!p.res || !p.out2[0])) || (!p.nout2 && p.res))
    return fail(UDP_ERR_ARG, "depthwise conv: null pointer (or a residual without a passthrough)");
  const int V = dtype == UDP_F32 ? 4 : 8;
  const bool si = p.relu == UDP_ACT_SILU;      // the SiLU instantiations
  if (ks != 3) {      // 5x5 / 7x7: one output pixel x V channels per thread (dwconvk_kernel)
    if ((ks != 5 && ks != 7) || (stride != 1 && stride != 2)) return fail(UDP_ERR_ARG, "depthwise conv: ks %d stride %d", ks, stride);
    const long total = (long)p.N * p.Hout * p.Wout * (p.Cin / V);
    if (total <= 0 || total >= (1L << 31) - 256) return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: %ld threads; split the batch", total);
    p.ntiles = (int)total;
#define UDP_DWK(T, S, K) (si ? reinterpret_cast<const void*>(&dwconvk_kernel<T, S, K, true>) : reinterpret_cast<const void*>(&dwconvk_kernel<T, S, K>))
    out->fn = dtype == UDP_F32 ? (ks == 5 ? (stride == 1 ? UDP_DWK(float, 1, 5) : UDP_DWK(float, 2, 5)) : (stride == 1 ? UDP_DWK(float, 1, 7) : UDP_DWK(float, 2, 7)))
                               : (ks == 5 ? (stride == 1 ? UDP_DWK(H2, 1, 5) : UDP_DWK(H2, 2, 5)) : (stride == 1 ? UDP_DWK(H2, 1, 7) : UDP_DWK(H2, 2, 7)));
#undef UDP_DWK
    out->grid = dim3((unsigned)((total + 255) / 256));
    out->block = dim3(256);
    out->lds = 0;
    out->p = p;
    return UDP_OK;
  }
  const long per_row = (long)p.N * p.Wout * (p.Cin / V);
  // rows per strip: the whole height if that still fills the chip (256 CUs x 8 waves), else halved down to 2
  int R = p.Hout;
  while (R > 2 && per_row * ((p.Hout + R - 1) / R) < 131072) R = (R + 1) / 2;
  p.R = R;
  p.tiles_y = (p.Hout + R - 1) / R;
  const long total = per_row * p.tiles_y;
  if (total <= 0 || total >= (1L << 31) - 256) return fail(UDP_ERR_UNSUPPORTED, "depthwise conv: %ld threads; split the batch", total);
  p.ntiles = (int)total;
#define UDP_DW3(T, S) (si ? reinterpret_cast<const void*>(&dwconv3_kernel<T, S, true>) : reinterpret_cast<const void*>(&dwconv3_kernel<T, S>))
  out->fn = dtype == UDP_F32 ? (stride == 1 ? UDP_DW3(float, 1) : UDP_DW3(float, 2)) : (stride == 1 ? UDP_DW3(H2, 1) : UDP_DW3(H2, 2));
#undef UDP_DW3
  out->grid = dim3((unsigned)((total + 255) / 256));
  out->block = dim3(256);
  out->lds = 0;
  out->p = p;
  return UDP_OK;
}

// p: geometry, views, in / out, wgt = the parameter block, up_shift[0] = hidden width.  One workgroup per image.
int describe_se(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "squeeze-excitation: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt) return fail(UDP_ERR_ARG, "squeeze-excitation: null pointer");
  const int V = dtype == UDP_F32 ? 4 : 8, Ch = p.up_shift[0];
  if (p.Cin <= 0 || p.Cin % 32 || p.Cin > 512 || Ch < 1 || Ch > 256 || p.N <= 0) return fail(UDP_ERR_ARG, "squeeze-excitation: C %d, hidden %d", p.Cin, Ch);
  out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&se_kernel<float>) : reinterpret_cast<const void*>(&se_kernel<H2>);
  out->grid = dim3((unsigned)p.N);
  out->block = dim3(256);
  out->lds = (unsigned)((256 * V + 2 * p.Cin + 256 + Ch) * sizeof(float));
  out->p = p;
  return UDP_OK;
}

// p: geometry, views, in / out, wgt = the parameter block, up_shift[0] = hidden width, relu = the activation applied to
// the INPUT (it picks the instantiation; the store applies none).  One workgroup per image, LDS sized from C.
int describe_se_act(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "activation + squeeze-excitation: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt) return fail(UDP_ERR_ARG, "activation + squeeze-excitation: null pointer");
  const int V = dtype == UDP_F32 ? 4 : 8, Ch = p.up_shift[0], act = p.relu;
  if (p.Cin < 32 || p.Cin % 32 || p.Cin > 1024 || Ch < 1 || Ch > 256 || Ch > p.Cin || p.N <= 0 || p.Hin < 1 || p.Win < 1)
    return fail(UDP_ERR_ARG, "activation + squeeze-excitation: C %d, hidden %d", p.Cin, Ch);
  if (act != UDP_ACT_NONE && act != UDP_ACT_RELU && act != UDP_ACT_HSWISH) return fail(UDP_ERR_ARG, "activation + squeeze-excitation: activation code %d", act);
#define UDP_SEA(T) (act == UDP_ACT_HSWISH ? reinterpret_cast<const void*>(&se_act_kernel<T, UDP_ACT_HSWISH>) \
                    : act == UDP_ACT_RELU ? reinterpret_cast<const void*>(&se_act_kernel<T, UDP_ACT_RELU>)   \
                                          : reinterpret_cast<const void*>(&se_act_kernel<T, UDP_ACT_NONE>))
  out->fn = dtype == UDP_F32 ? UDP_SEA(float) : UDP_SEA(H2);
#undef UDP_SEA
  const int cgs = p.Cin / V, P0 = 256 / cgs > 1 ? 256 / cgs : 1;
  p.relu = 0;
  out->grid = dim3((unsigned)p.N);
  out->block = dim3(256);
  out->lds = (unsigned)(((size_t)P0 * p.Cin + 2 * p.Cin + 256 + Ch) * sizeof(float));
  out->p = p;
  return UDP_OK;
}

int describe_pixshuf(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "pixel shuffle: storage modes f32 and f16x2 only");
  if (!p.in || !p.out) return fail(UDP_ERR_ARG, "pixel shuffle: null pointer");
  const int V = dtype == UDP_F32 ? 4 : 8;
  const long total = (long)p.N * p.Hin * p.Win * 4 * (p.Cout / V);
  if (total <= 0 || total >= (1L << 31) - 256) return fail(UDP_ERR_UNSUPPORTED, "pixel shuffle: %ld threads; split the batch", total);
  p.ntiles = (int)total;
  out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&pixshuf2_kernel<float>) : reinterpret_cast<const void*>(&pixshuf2_kernel<H2>);
  out->grid = dim3((unsigned)((total + 255) / 256));
  out->block = dim3(256);
  out->lds = 0;
  out->p = p;
  return UDP_OK;
}

int dwconv_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
