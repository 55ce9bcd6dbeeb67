// Training kernels of the ShuffleNetV2 pose nets (deep_hrnet/lib/models/backbones/shufflenetv2.py, decoders/DUC.py)
// for gfx950 that the HRNet / pose_resnet steps (train.hip, resnet_train.hip) do not have, next to the depthwise convs of
// dw_train.hip:
//
//   udp_pixshuf2_train_fwd   nn.PixelShuffle(2) in torch's channel order (DUC.py:27) and
//   udp_pixshuf2_train_bwd   its inverse
//   udp_shuffle_pair_fwd     torch.cat + channel_shuffle (:77-92) on a unit output kept as a pair of halves, and
//   udp_shuffle_pair_bwd     the inverse permutation
//   udp_chan_cat2 / _uncat2  the materialised concat where the whole tensor is read, and its inverse
//
// All tensors NHWC fp32 with a stored channel count that is a multiple of 4: a thread owns 4 consecutive channels and
// moves 16 bytes.  Every kernel writes EVERY stored channel of its output (padded channels: zeros), and nothing is
// computed: bit patterns move.
#include "common.h"

namespace udp {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

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

static int move_check(const char* who, const void* a, const void* b, int dtype) {
  if (!a || !b) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  return UDP_OK;
}

}  // namespace udp

using namespace udp;

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
