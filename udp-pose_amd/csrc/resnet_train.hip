// Training kernels of pose_resnet (SimpleBaseline, deep_hrnet/lib/models/pose_resnet.py) for gfx950 that the HRNet
// step (train.hip) does not have:
//
//   udp_deconv4s2_dgrad   input gradient of ConvTranspose2d(4, 2, 1), the deconv head (:155-193).  MFMA fp32 16x16x4,
//                         an LDS-staged halo tile of dY, no atomics, no zero-stuffed or space-to-depth copy.
//   udp_maxpool3s2_fwd    MaxPool2d(3, 2, 1) (:116, :199) on NHWC fp32
//   udp_maxpool3s2_bwd    its backward as a gather (no index tensor, no atomics)
//   udp_stem7_train_fwd   conv1 (3 -> 64, 7x7 s2 p3, :112) on the unfolded weights, no bias, no ReLU
//
// The weight gradients of the deconv and of the stem are udp_conv2d_wgrad with ks 4 / 7 (train.hip).  fp32 only.
#include <cstdlib>

#include "common.h"

namespace udp {

// ---------------------------------------------------------------------------------------------
// dx[n,iy,ix,ci] = sum_{co,ky,kx} dY[n, 2iy-1+ky, 2ix-1+kx, co] * w[ci][co][ky][kx]
//
// A 4x4 stride-2 pad-1 conv over dY.  GEMM view: M = ci (A = weights), N = input-space pixels, K = (co, ky, kx).
// Workgroup = 128 ci x one tile of R x TW <= 64 input-space pixels of one image; wave w owns ci 32w .. 32w+31 (two
// 16-row blocks) for all four 16-pixel blocks.  Per 16-co chunk the (2R+2) x (2TW+2) halo tile of dY is staged once
// (registers -> LDS, the next chunk's global loads fly under the MFMAs) and serves all 16 taps: tap (ky,kx) of tile
// pixel (py,px) is halo pixel (2py+ky, 2px+kx).  Rows outside dY and the co tail of the last chunk are staged as zeros.
// A lane reads 4 consecutive co of its pixel (B) and of its weight row (A, from global / L2: [tap][cin_pad][cout_k])
// and issues 4 MFMAs; a pixel's sum runs over (chunk, tap, co) in that order in ONE accumulator, whatever the tiling.
// ---------------------------------------------------------------------------------------------
struct DeconvDgradParams {
  const float* dy;
  const float* w;
  float* dx;
  int N, H, W, Cin, CinPitch, CinPad, Cout, CoutPitch, CoutK;
  int R, TW, tiles_x, tiles_y, DH, DW;
};

constexpr int kDdPitch = 20;      // floats per staged pixel: 16 co + 4 (16 lanes x 16-byte reads hit 16 different bank quads)
constexpr int kDdItems = 8;       // 16-byte staging items per thread
constexpr int kDdMaxPix = kDdItems * 256 / 4;   // halo pixels a tile may have

__global__ __launch_bounds__(256) void deconv_dgrad_kernel(const DeconvDgradParams p) {
  __shared__ __attribute__((aligned(16))) float sDy[kDdMaxPix * kDdPitch];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 15, kg = lane >> 4;
  int b = blockIdx.x;
  const int tx = b % p.tiles_x;
  b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  const int n = b / p.tiles_y;
  const int y0 = ty * p.R, x0 = tx * p.TW;
  const int RT = p.R * p.TW, HP = p.DH * p.DW;
  const int H2 = 2 * p.H, W2 = 2 * p.W;

  // staging plan of this thread: item -> (halo pixel, 4 co of the chunk); the geometry is the same for every chunk
  long it_off[kDdItems];
#pragma unroll
  for (int k = 0; k < kDdItems; ++k) {
    const int item = t + k * 256, h = item >> 2, c4 = (item & 3) * 4;
    const int hy = h / p.DW, hx = h - hy * p.DW;
    const int gy = 2 * y0 - 1 + hy, gx = 2 * x0 - 1 + hx;
    const bool ok = h < HP && gy >= 0 && gy < H2 && gx >= 0 && gx < W2;
    it_off[k] = ok ? (((long)n * H2 + gy) * W2 + gx) * p.CoutPitch + c4 : -1;
  }
  f32x4 regs[kDdItems];
  auto fetch = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kDdItems; ++k) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (it_off[k] >= 0 && c0 + ((t + k * 256) & 3) * 4 < p.Cout) v = *reinterpret_cast<const f32x4*>(p.dy + it_off[k] + c0);
      regs[k] = v;
    }
  };

  // the lane's pixel of each 16-pixel block: LDS offset of its (0,0) tap
  int brow[4];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int m = min(pb * 16 + li, RT - 1);
    const int py = m / p.TW, px = m - py * p.TW;
    brow[pb] = ((2 * py) * p.DW + 2 * px) * kDdPitch + 4 * kg;
  }
  const int npb = (RT + 15) >> 4;                        // pixel blocks that hold a pixel (wave-uniform)
  const int cw = blockIdx.y * 128 + wave * 32;           // the wave's first ci
  const bool active = cw < p.Cin;                        // wave-uniform; rows cw .. cw+31 < CinPad then
  const long wtap = (long)p.CinPad * p.CoutK;
  const float* wl = p.w + (long)(cw + li) * p.CoutK + 4 * kg;

  f32x4 acc[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) acc[nb][pb] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int c0 = 0; c0 < p.CoutK; c0 += 16) {
    __syncthreads();                                     // the previous chunk's operand reads are done
#pragma unroll
    for (int k = 0; k < kDdItems; ++k) {
      const int item = t + k * 256;
      if ((item >> 2) < HP) *reinterpret_cast<f32x4*>(sDy + (item >> 2) * kDdPitch + (item & 3) * 4) = regs[k];
    }
    __syncthreads();
    if (c0 + 16 < p.CoutK) fetch(c0 + 16);
    if (active) {
      // A fragments one tap ahead (a ring of 4 loaded three steps ahead, as the forward kernel has, measured 12-23 %
      // slower on the three head shapes: the compiler already hoists these loads in the unrolled tap loop)
      f32x4 a[2][2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) a[0][nb] = *reinterpret_cast<const f32x4*>(wl + (long)nb * 16 * p.CoutK + c0);
#pragma unroll
      for (int tap = 0; tap < 16; ++tap) {
        if (tap + 1 < 16) {
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            a[(tap + 1) & 1][nb] = *reinterpret_cast<const f32x4*>(wl + (tap + 1) * wtap + (long)nb * 16 * p.CoutK + c0);
        }
        const int toff = ((tap >> 2) * p.DW + (tap & 3)) * kDdPitch;
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
          if (pb < npb) {
            const f32x4 xb = *reinterpret_cast<const f32x4*>(sDy + brow[pb] + toff);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
              for (int j = 0; j < 4; ++j)
                acc[nb][pb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap & 1][nb][j], xb[j], acc[nb][pb], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!active) return;
  // D[m = 4*kg + r][n = li]: the lane holds 4 consecutive ci of its pixel
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int m = pb * 16 + li;
    const int py = m / p.TW, px = m - py * p.TW;
    const int y = y0 + py, x = x0 + px;
    if (m >= RT || y >= p.H || x >= p.W) continue;
    float* o = p.dx + (((long)n * p.H + y) * p.W + x) * p.CinPitch;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int ci = cw + nb * 16 + 4 * kg;
      if (ci < p.Cin) *reinterpret_cast<f32x4*>(o + ci) = acc[nb][pb];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) on NHWC fp32, 4 channels per thread; padding never wins.  The arg-max of a window is its FIRST
// maximum in row-major window order (ATen's max_pool2d: `val > maxval || isnan(val)`); after a ReLU ties at 0 are the
// common case, and the backward below must pick the same element.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, int Ho,
                                                            int Wo, float* __restrict__ y) {
  const int C4 = C >> 2;
  const long total = (long)N * Ho * Wo * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (idx % C4) * 4;
    const long pix = idx / C4;
    const int ox = pix % Wo;
    const long r = pix / Wo;
    const int oy = r % Ho;
    const long n = r / Ho;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int ky = 0; ky < 3; ++ky) {
      const int gy = 2 * oy - 1 + ky;
      if (gy < 0 || gy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int gx = 2 * ox - 1 + kx;
        if (gx < 0 || gx >= W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + gy) * W + gx) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v[e] > m[e] || v[e] != v[e]) m[e] = v[e];
      }
    }
    *reinterpret_cast<f32x4*>(y + pix * C + c) = m;
  }
}

// One thread = 4 channels of one INPUT pixel.  It visits the at most four windows that contain the pixel (rows
// iy/2 and, for odd iy, (iy+1)/2; columns alike), recomputes each window's arg-max by the rule above and adds the dy of
// the windows its pixel wins, in (oy, ox) order.  Every dx element is written.
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int N,
                                                            int H, int W, int C, int Ho, int Wo, float* __restrict__ dx) {
  const int C4 = C >> 2;
  const long total = (long)N * H * W * C4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int c = (idx % C4) * 4;
    const long pix = idx / C4;
    const int ix = pix % W;
    const long r = pix / W;
    const int iy = r % H;
    const long n = r / H;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    for (int wy = 0; wy <= (iy & 1); ++wy) {
      const int oy = (iy >> 1) + wy;
      if (oy >= Ho) continue;
      for (int wx = 0; wx <= (ix & 1); ++wx) {
        const int ox = (ix >> 1) + wx;
        if (ox >= Wo) continue;
        const int mine = (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1));     // this pixel's position in the window
        f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int best[4] = {-1, -1, -1, -1};
        for (int ky = 0; ky < 3; ++ky) {
          const int gy = 2 * oy - 1 + ky;
          if (gy < 0 || gy >= H) continue;
          for (int kx = 0; kx < 3; ++kx) {
            const int gx = 2 * ox - 1 + kx;
            if (gx < 0 || gx >= W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + gy) * W + gx) * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (best[e] < 0 || v[e] > m[e] || v[e] != v[e]) {
                m[e] = v[e];
                best[e] = ky * 3 + kx;
              }
          }
        }
        const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((n * Ho + oy) * Wo + ox) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (best[e] == mine) g[e] += d[e];
      }
    }
    *reinterpret_cast<f32x4*>(dx + pix * C + c) = g;
  }
}

// ---------------------------------------------------------------------------------------------
// conv1 of pose_resnet.py:112 in train mode: 3 -> 64, 7x7 stride 2 pad 3, no bias (the BatchNorm follows unfolded).
// x: the [n,h,w,cin_k] NHWC image of udp_nchw_to_nhwc (channels 3.. are ignored), weights in the packed forward layout
// [49][cout_pad][cin_k] of udp_pack_conv_weights(ks = 7).  2 % of the net's MACs: a direct conv, the 147 x 64 weights
// in LDS, one thread = one output pixel x 4 output channels, fmaf over (ky, kx, ci) in that order.
// ---------------------------------------------------------------------------------------------
constexpr int kStemCout = 64;

__global__ __launch_bounds__(256) void stem7_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp, int N, int H,
                                                       int W, int CinK, int Ho, int Wo, int CoutPad, float* __restrict__ y) {
  __shared__ f32x4 sW[49 * 3 * (kStemCout / 4)];
  float* sw = reinterpret_cast<float*>(sW);
  for (int i = threadIdx.x; i < 49 * 3 * kStemCout; i += 256) {
    const int co = i % kStemCout, ci = (i / kStemCout) % 3, tap = i / (3 * kStemCout);
    sw[i] = wp[((long)tap * CoutPad + co) * CinK + ci];
  }
  __syncthreads();
  const int q = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const long total = (long)N * Ho * Wo;
  for (long pix = (long)blockIdx.x * 16 + pl; pix < total; pix += (long)gridDim.x * 16) {
    const int ox = pix % Wo;
    const long r = pix / Wo;
    const int oy = r % Ho;
    const long n = r / Ho;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < 7; ++ky) {
      const int gy = 2 * oy - 3 + ky;
      if (gy < 0 || gy >= H) continue;
      for (int kx = 0; kx < 7; ++kx) {
        const int gx = 2 * ox - 3 + kx;
        if (gx < 0 || gx >= W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + ((n * H + gy) * W + gx) * CinK);
        const f32x4* wq = sW + (ky * 7 + kx) * 3 * (kStemCout / 4) + q;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const f32x4 w4 = wq[ci * (kStemCout / 4)];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(v[ci], w4[e], acc[e]);
        }
      }
    }
    *reinterpret_cast<f32x4*>(y + pix * kStemCout + 4 * q) = acc;
  }
}

}  // namespace udp

using namespace udp;

extern "C" int udp_deconv4s2_dgrad(const void* dy, const void* w_dgrad, int n, int hin, int win, int cin, int cin_pitch,
                                   int cout, int cout_pitch, int dtype, void* dx, void* stream) {
  if (!dy || !w_dgrad || !dx) return fail(UDP_ERR_ARG, "udp_deconv4s2_dgrad: null pointer");
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "udp_deconv4s2_dgrad: fp32 only (dtype %d)", dtype);
  if (n <= 0 || hin <= 0 || win <= 0 || cin <= 0 || cin % 16 || cin > 2048 || cout <= 0 || cout % 8 || cin_pitch < cin ||
      (cin_pitch & 3) || cout_pitch < cout || (cout_pitch & 3))
    return fail(UDP_ERR_ARG, "udp_deconv4s2_dgrad: C%d(%d)->%d(%d) %dx%d x%d (cin %% 16, cin <= 2048, cout %% 8, pitches %% 4)", cin,
                cin_pitch, cout, cout_pitch, hin, win, n);
  DeconvDgradParams p;
  memset(&p, 0, sizeof(p));
  p.dy = reinterpret_cast<const float*>(dy);
  p.w = reinterpret_cast<const float*>(w_dgrad);
  p.dx = reinterpret_cast<float*>(dx);
  p.N = n; p.H = hin; p.W = win; p.Cin = cin; p.CinPitch = cin_pitch; p.Cout = cout; p.CoutPitch = cout_pitch;
  p.CinPad = (cin + 31) / 32 * 32;
  p.CoutK = (cout + 15) / 16 * 16;
  // tile: columns in equal segments of <= 16, as many rows as 64 pixel slots hold (<= 32), rows balanced over the tiles
  p.tiles_x = ceil_div(win, 16);
  p.TW = ceil_div(win, p.tiles_x);
  int rmax = 64 / p.TW;
  if (rmax > 32) rmax = 32;
  p.tiles_y = ceil_div(hin, rmax);
  p.R = ceil_div(hin, p.tiles_y);
  p.DH = 2 * p.R + 2;
  p.DW = 2 * p.TW + 2;
  if (p.R * p.TW > 64 || p.DH * p.DW > kDdMaxPix) return fail(UDP_ERR_UNSUPPORTED, "udp_deconv4s2_dgrad: tile %dx%d", p.R, p.TW);
  const long wgs = (long)n * p.tiles_y * p.tiles_x;
  if (wgs >= (1L << 31)) return fail(UDP_ERR_UNSUPPORTED, "udp_deconv4s2_dgrad: %ld tiles", wgs);
  if (getenv("UDP_POSE_DEBUG_TILES"))
    fprintf(stderr, "deconv dgrad %dx%d C%d<-%d: R=%d TW=%d halo=%dx%d wgs=%ldx%d\n", hin, win, cin, cout, p.R, p.TW, p.DH, p.DW, wgs,
            ceil_div(cin, 128));
  deconv_dgrad_kernel<<<dim3((unsigned)wgs, ceil_div(cin, 128)), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(p);
  return launched("udp_deconv4s2_dgrad");
}

static int maxpool_check(const char* who, const void* a, const void* b, int n, int h, int w, int c, int dtype) {
  if (!a || !b) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "%s: fp32 only (dtype %d)", who, dtype);
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || (c & 3)) return fail(UDP_ERR_ARG, "%s: %dx%dx%d x%d (c %% 4)", who, h, w, c, n);
  return UDP_OK;
}

extern "C" int udp_maxpool3s2_fwd(const void* x, int n, int h, int w, int c, int dtype, void* y, void* stream) {
  if (const int rc = maxpool_check("udp_maxpool3s2_fwd", x, y, n, h, w, c, dtype)) return rc;
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const long total = (long)n * ho * wo * (c / 4);
  maxpool3s2_fwd_kernel<<<blocks_for(total, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(x), n, h, w, c, ho, wo, reinterpret_cast<float*>(y));
  return launched("udp_maxpool3s2_fwd");
}

extern "C" int udp_maxpool3s2_bwd(const void* x, const void* dy, int n, int h, int w, int c, int dtype, void* dx, void* stream) {
  if (const int rc = maxpool_check("udp_maxpool3s2_bwd", x, dy, n, h, w, c, dtype)) return rc;
  if (!dx) return fail(UDP_ERR_ARG, "udp_maxpool3s2_bwd: null pointer");
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const long total = (long)n * h * w * (c / 4);
  maxpool3s2_bwd_kernel<<<blocks_for(total, 256, 1 << 20), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(x), reinterpret_cast<const float*>(dy), n, h, w, c, ho, wo, reinterpret_cast<float*>(dx));
  return launched("udp_maxpool3s2_bwd");
}

extern "C" int udp_stem7_train_fwd(const void* x, const void* w_fwd, int n, int h, int w, int cin_k, int cout, int dtype, void* y,
                                   void* stream) {
  if (!x || !w_fwd || !y) return fail(UDP_ERR_ARG, "udp_stem7_train_fwd: null pointer");
  if (dtype != UDP_F32) return fail(UDP_ERR_UNSUPPORTED, "udp_stem7_train_fwd: fp32 only (dtype %d)", dtype);
  if (n <= 0 || h <= 0 || w <= 0 || cin_k != 16 || cout != kStemCout)
    return fail(UDP_ERR_ARG, "udp_stem7_train_fwd: %dx%d x%d, pitch %d, cout %d (3 in a pitch of 16 -> 64 only)", h, w, n, cin_k, cout);
  const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
  const long total = (long)n * ho * wo;
  stem7_fwd_kernel<<<blocks_for(total, 16 * 8, 2048), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<const float*>(x), reinterpret_cast<const float*>(w_fwd), n, h, w, cin_k, ho, wo, (cout + 31) / 32 * 32,
      reinterpret_cast<float*>(y));
  return launched("udp_stem7_train_fwd");
}
