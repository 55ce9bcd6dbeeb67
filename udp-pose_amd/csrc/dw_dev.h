// Device-side helpers of the per-pixel VALU kernels on NHWC views (dwconv.hip, attn.hip): 16-byte channel-group loads
// and stores in the fp32 and split-fp16 storage modes.
#pragma once
#include "conv_dev.h"

namespace udp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

template <typename T>
struct DwTr;
template <>
struct DwTr<float> {
  static constexpr int V = 4, PL = 1;
  using E = uint32_t;      // one stored unit of a plane
  using Vec = u32x4;       // 16 bytes of them
};
template <>
struct DwTr<H2> {
  static constexpr int V = 8, PL = 2;
  using E = uint16_t;
  using Vec = u16x8;
};

// V consecutive channels from `c` of pixel `pix` of the input view, decoded to fp32
template <typename T, int V>
__device__ __forceinline__ void dw_load(const ConvParams& p, size_t pix, int c, float (&x)[V]) {
  if constexpr (std::is_same<T, float>::value) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.in) + pix * (size_t)p.in_pitch + p.in_coff + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = v[k];
  } else {
    const _Float16* q = reinterpret_cast<const _Float16*>(p.in) + pix * (2 * (size_t)p.in_pitch) + p.in_coff + c;
    const f16x8 hi = *reinterpret_cast<const f16x8*>(q), lo = *reinterpret_cast<const f16x8*>(q + p.in_pitch);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (float)hi[k] + (float)lo[k] * kLoInv;    // lo * 2^-11 is exact
  }
}

// SILU: the UDP_ACT_SILU instantiations (udp_conv_op.relu == 4) -- silu() where the others apply the ReLU
template <typename T, int V, bool SILU = false>
__device__ __forceinline__ void dw_store(const ConvParams& p, size_t pix, int c, const float (&a)[V]) {
  float v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if constexpr (SILU) v[k] = silu(a[k]);
    else v[k] = p.relu ? __builtin_fmaxf(a[k], 0.f) : a[k];
  }
  if constexpr (std::is_same<T, float>::value) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + pix * (size_t)p.out_pitch + p.out_coff + c) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    f16x8 hi, lo;
    h2_split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, hi, lo);     // raises the range flag
    _Float16* q = reinterpret_cast<_Float16*>(p.out) + pix * (2 * (size_t)p.out_pitch) + p.out_coff + c;
    *reinterpret_cast<f16x8*>(q) = hi;
    *reinterpret_cast<f16x8*>(q + p.out_pitch) = lo;
  }
}

}  // namespace udp
