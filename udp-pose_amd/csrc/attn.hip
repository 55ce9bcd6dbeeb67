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

int attn_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
