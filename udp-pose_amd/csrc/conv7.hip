// 7x7 stride-1 pad-3 NHWC convolution on the matrix cores of gfx950 (MI355X, CDNA4): UDP_OP_CONV with ks = 7.
//
// The one user is the stem of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py:188-203 (conv 7x7 s1 64 -> 64 at half
// resolution).  conv_mfma_body (conv.hip) stages ALL taps of a K chunk at once; with 49 taps and 64 output channels that
// is 200 KB per plane, more than a CU's 160 KiB of LDS.  This kernel keeps the body's layout -- 64-byte swizzled LDS
// rows filled by LDS-DMA, A = weights (rows = cout), B = pixels, a lane ends up with 4*NB consecutive output channels
// of a pixel -- and streams the weights ONE KERNEL ROW at a time instead:
//
//   stage s = (K chunk c, kernel row ky), s = 7 c + ky.  The input halo tile of chunk c ((R+6) x (TW+6) pixels x 64 B
//   per plane) stays resident for its 7 stages; the weight piece of a stage is 7 taps x BN couts x 64 B per plane
//   (28 KB at BN = 64; 56 KB in split fp16) and is double-buffered: piece s+1 streams in while piece s feeds the MFMAs,
//   one barrier per stage.  fp32 double-buffers the halo tile too (chunk c+1 is requested during the last row of chunk
//   c); split fp16, whose planes double every byte count, keeps ONE halo buffer (ConvParams.sbuf) and refills it
//   between two chunks behind an extra barrier -- once for 64 input channels.
//
//   fp32      : v_mfma_f32_16x16x4_f32 (exact fp32 fma chain), CK = 16 input channels per chunk
//   split fp16: the three v_mfma_f32_16x16x32_f16 of mfma_chunk_h2 (hi*hi -> acc; hi*lo, lo*hi -> accx), fp32
//               accumulation, result acc + 2^-11 accx, CK = 32
//
// A pixel's sum runs over (chunk, ky, kx, k step) in that order inside ONE lane's accumulator, whatever tile or image
// group the pixel falls into: results do not depend on the tiling or the batch.  Halo pixels outside the image and the
// channels of a ragged last chunk are DMA'd from out-of-range buffer offsets, i.e. they are exact zeros.
//
// Contract (describe_conv7): stride 1, wfmt 0 weights [49 taps][cout_pad][cin], cin % 16 == 0, cout % 16 == 0, folded
// bias, ReLU or none, channel-slice views on input and output.  No residual, addends, second outputs, NCHW output,
// stuffed input, hard-swish / SiLU, bf16.
#include "conv_dev.h"

namespace udp {

constexpr int K7 = 7;

// One kernel row (7 taps) of one K chunk for a wave: MBW pixel blocks x NB cout blocks, software-pipelined like
// mfma_chunk (the fragments of step s+1 are read before the MFMAs of step s issue).  `wrow`: the lane's row li of the
// staged piece; `row0` = ky * IW.
template <int NB, int MBW>
__device__ __forceinline__ void mfma_row_f32(f32x4 (&acc)[MBW][NB], const unsigned char* sb, const unsigned char* wrow,
                                             const int (&prow)[MBW], int row0, int kg, int wswz) {
  constexpr int BN = NB * 16;
  constexpr int NSTEP = K7 * 2;
  f32x2 wf[2][NB], pf[2][MBW];
  auto load = [&](int s, f32x2 (&w)[NB], f32x2 (&x)[MBW]) {
    const int kx = s >> 1;
    const int part = 2 * (s & 1) + (kg >> 1);
    const int sub = (kg & 1) * 8;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      w[nb] = *reinterpret_cast<const f32x2*>(wrow + (kx * BN + nb * 16) * ROWB + ((part ^ wswz) << 4) + sub);
#pragma unroll
    for (int i = 0; i < MBW; ++i) {
      const int row = prow[i] + row0 + kx;
      x[i] = *reinterpret_cast<const f32x2*>(sb + row * ROWB + ((part ^ swz<float>(row)) << 4) + sub);
    }
  };
  load(0, wf[0], pf[0]);
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    if (s + 1 < NSTEP) load(s + 1, wf[(s + 1) & 1], pf[(s + 1) & 1]);
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s & 1][nb][0], pf[s & 1][i][0], acc[i][nb], 0, 0, 0);
        acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s & 1][nb][1], pf[s & 1][i][1], acc[i][nb], 0, 0, 0);
      }
  }
}

// The same for split-fp16 operands (mfma_chunk_h2's product): the hi / lo images lie in_lo (input) / w_lo (weights) bytes apart.
template <int NB, int MBW>
__device__ __forceinline__ void mfma_row_h2(f32x4 (&acc)[MBW][NB], f32x4 (&accx)[MBW][NB], const unsigned char* sb,
                                            const unsigned char* wrow, int in_lo, int w_lo, const int (&prow)[MBW], int row0,
                                            int kg, int wswz) {
  constexpr int BN = NB * 16;
  f16x8 wh[2][NB], wl[2][NB], xh[2][MBW], xl[2][MBW];
  auto load = [&](int kx, f16x8 (&a)[NB], f16x8 (&b)[NB], f16x8 (&c)[MBW], f16x8 (&d)[MBW]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const unsigned char* q = wrow + (kx * BN + nb * 16) * ROWB + ((kg ^ wswz) << 4);
      a[nb] = *reinterpret_cast<const f16x8*>(q);
      b[nb] = *reinterpret_cast<const f16x8*>(q + w_lo);
    }
#pragma unroll
    for (int i = 0; i < MBW; ++i) {
      const int row = prow[i] + row0 + kx;
      const unsigned char* q = sb + row * ROWB + ((kg ^ swz<H2>(row)) << 4);
      c[i] = *reinterpret_cast<const f16x8*>(q);
      d[i] = *reinterpret_cast<const f16x8*>(q + in_lo);
    }
  };
  load(0, wh[0], wl[0], xh[0], xl[0]);
#pragma unroll
  for (int s = 0; s < K7; ++s) {
    if (s + 1 < K7) load(s + 1, wh[(s + 1) & 1], wl[(s + 1) & 1], xh[(s + 1) & 1], xl[(s + 1) & 1]);
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s & 1][nb], xh[s & 1][i], acc[i][nb], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) accx[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s & 1][nb], xl[s & 1][i], accx[i][nb], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) accx[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[s & 1][nb], xh[s & 1][i], accx[i][nb], 0, 0, 0);
  }
}

// T = float | H2; NB = 16-cout blocks per workgroup (BN = 16 NB couts: grid.y = CoutPad / BN); MBW = 16-pixel blocks per
// wave (4 waves: tile of M <= 64 MBW pixels).  grid.x = tiles of G images x R rows x TW columns.
template <typename T, int NB, int MBW>
__global__ __launch_bounds__(256) void conv7_mfma_kernel(const ConvParams p) {
  constexpr int NW = 4;
  constexpr int CK = Tr<T>::CK;
  constexpr int ESZ = Tr<T>::ESZ;
  constexpr int PL = Tr<T>::PL;
  constexpr int BN = NB * 16;
  constexpr int PAD = K7 / 2;
  constexpr int WGROUPS = K7 * BN / 16;          // 16-row staging groups of one weight piece (one plane)
  constexpr int WP_BYTES = K7 * BN * ROWB;       // one plane of a weight piece
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15;
  const int kg = lane >> 4;
  const int cb = blockIdx.y;

  int t = blockIdx.x;   // wave-uniform tile decode
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n0 = (t / p.tiles_y) * p.G;
  const int y0 = ty * p.R;
  const int x0 = tx * p.TW;

  const int IH = p.IH, IW = p.IW;
  const int npix_in = p.G * IH * IW;
  const int in_groups = (npix_in + 15) >> 4;
  const int in_bytes = in_groups * 16 * ROWB;            // one plane of the halo tile
  const int nchunks = (p.Cin + CK - 1) / CK;
  const bool ragged = (p.Cin % CK) != 0;   // last chunk is partly past Cin: those 16-byte parts read zeros
  const int RT = p.R * p.TW;
  const int M = p.G * RT;
  const unsigned cinb = (unsigned)p.Cin * ESZ * PL;          // weight row (H2: hi plane, then lo plane)
  const unsigned inpb = (unsigned)p.in_pitch * ESZ * PL;     // input pixel (the conv may read a channel slice)
  const unsigned outpb = (unsigned)p.out_pitch * ESZ * PL;
  const unsigned w_lo = (unsigned)p.Cin * ESZ, in_lo = (unsigned)p.in_pitch * ESZ;   // lo plane offsets (H2)
  const unsigned out_lo = (unsigned)p.out_pitch * ESZ;
  // LDS: [halo tile: 1 (sbuf) or 2 buffers of PL planes][weight pieces: 2 buffers of PL planes]
  unsigned char* const w_lds = smem + (p.sbuf ? 1 : 2) * PL * in_bytes;

  const unsigned out_pix = (unsigned)p.N * p.Hout * p.Wout;
  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.in), 0, (unsigned)p.N * p.Hin * p.Win * inpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.wgt), 0, (unsigned)(K7 * K7) * p.CoutPad * cinb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, out_pix * outpb, 0x00020000);

  // ---- per-lane DMA offsets of the input halo tile (chunk 0); masked rows -> kOobOff -> zeros
  const int srow = lane >> 2;  // row inside a 16-row group
  const int spart = lane & 3;  // stored 16-byte part position
  const int gy0 = y0 - PAD, gx0 = x0 - PAD;
  unsigned src_off[MAXG];
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    unsigned off = kOobOff;
    if ((wave + NW * i) * 16 < npix_in) {   // wave-uniform
      const int row = (wave + NW * i) * 16 + srow;
      const int tmp = fdiv20(row, p.mIW);
      const int ix = row - (int)__umul24(tmp, IW);
      const int g = fdiv20(tmp, p.mIH);
      const int iy = tmp - (int)__umul24(g, IH);
      const int n = n0 + g, gy = gy0 + iy, gx = gx0 + ix;
      const bool ok = row < npix_in && n < p.N && (unsigned)gy < (unsigned)p.Hin && (unsigned)gx < (unsigned)p.Win;
      const unsigned pix = __umul24(__umul24(n, p.Hin) + gy, p.Win) + gx;
      off = ok ? pix * inpb + p.in_coff * ESZ + ((spart ^ swz<T>(row)) << 4) : kOobOff;
    }
    src_off[i] = off;
  }
  auto stage_in = [&](int c, unsigned char* sb) {
    const unsigned coff = (unsigned)c * (CK * ESZ);
    const bool cut = ragged && c == nchunks - 1;           // wave-uniform
    const int parts_left = (p.Cin - c * CK) / (16 / ESZ);  // 16-byte parts of this chunk that exist
#pragma unroll
    for (int i = 0; i < MAXG; ++i) {
      const int gidx = wave + NW * i;
      if (gidx < in_groups) {
        unsigned off = src_off[i] + coff;
        // (a masked row must stay out of range: kOobOff + coff still is)
        if (cut && (spart ^ swz<T>(gidx * 16 + srow)) >= parts_left) off = kOobOff;
        blds16(r_in, off, sb + gidx * (16 * ROWB));
        if constexpr (PL == 2) blds16(r_in, off + in_lo, sb + in_bytes + gidx * (16 * ROWB));
      }
    }
  };
  // weight piece (chunk c, kernel row ky): LDS row (kx, nb*16 + r) holds cout 4*NB*(r>>2) + 4*nb + (r&3) of this block
  auto stage_w = [&](int c, int ky, unsigned char* wb) {
    const unsigned coff = (unsigned)c * (CK * ESZ);
    const bool cut = ragged && c == nchunks - 1;
    const int parts_left = (p.Cin - c * CK) / (16 / ESZ);
    for (int gidx = wave; gidx < WGROUPS; gidx += NW) {
      const int wr = gidx * 16 + srow;
      const int kx = wr / BN;   // BN is a power of two
      const int rho = wr & (BN - 1);
      const int co = (4 * NB) * ((rho & 15) >> 2) + 4 * (rho >> 4) + (rho & 3);
      const int lp = spart ^ swz<T>(wr);
      unsigned e = __umul24(__umul24(ky * K7 + kx, p.CoutPad) + cb * BN + co, cinb) + coff + (lp << 4);
      if (cut && lp >= parts_left) e = kOobOff;
      blds16(r_w, e, wb + gidx * (16 * ROWB));
      if constexpr (PL == 2) blds16(r_w, e + w_lo, wb + WP_BYTES + gidx * (16 * ROWB));
    }
  };

  // ---- the lane's MBW output pixels
  int prow[MBW];        // LDS row of the pixel's (0,0) tap
  int opix[MBW];        // output pixel index, -1 = masked lane
  const int cbase = cb * BN + 4 * NB * kg;
#pragma unroll
  for (int i = 0; i < MBW; ++i) {
    const int m0 = (wave + NW * i) * 16 + li;
    const int m = m0 < M ? m0 : M - 1;
    const int g = fdiv20(m, p.mRT);
    const int rem = m - (int)__umul24(g, RT);
    const int r = fdiv20(rem, p.mTW);
    const int x = rem - (int)__umul24(r, p.TW);
    prow[i] = (int)__umul24(__umul24(g, IH) + r, IW) + x;
    const int n = n0 + g, y = y0 + r, xo = x0 + x;
    const bool ok = m0 < M && n < p.N && y < p.Hout && xo < p.Wout && cbase < p.Cout;
    opix[i] = ok ? (int)(__umul24(__umul24(n, p.Hout) + y, p.Wout) + xo) : -1;
  }
  const int wswz = swz<T>(li);  // weight rows: (kx*BN + nb*16) is a multiple of 16 -> swizzle depends on li only

  f32x4 acc[MBW][NB];
  f32x4 accx[PL == 2 ? MBW : 1][NB];   // H2: the 2^11-scaled cross terms
#pragma unroll
  for (int i = 0; i < (PL == 2 ? MBW : 1); ++i)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) accx[i][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  {
    f32x4 bias[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bias[nb] = *reinterpret_cast<const f32x4*>(p.bias + cbase + 4 * nb);
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = bias[nb];
  }

  stage_in(0, smem);
  stage_w(0, 0, w_lds);
  const int nstages = nchunks * K7;
  int c = 0, ky = 0;
  for (int s = 0; s < nstages; ++s) {
    // one halo buffer: refill it for a new chunk once every wave has left the last row of the previous one
    if (p.sbuf && ky == 0 && c > 0) {
      __syncthreads();
      stage_in(c, smem);
    }
    // stage s has landed (explicit wait: the compiler is not obliged to track LDS-DMA) and every wave is done with
    // stage s-1, whose weight buffer stage s+1 overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (s + 1 < nstages) {
      const bool last_row = ky == K7 - 1;
      stage_w(last_row ? c + 1 : c, last_row ? 0 : ky + 1, w_lds + ((s + 1) & 1) * (PL * WP_BYTES));
      if (!p.sbuf && last_row) stage_in(c + 1, smem + ((c + 1) & 1) * (PL * in_bytes));
    }
    const unsigned char* sb = p.sbuf ? smem : smem + (c & 1) * (PL * in_bytes);
    const unsigned char* wb = w_lds + (s & 1) * (PL * WP_BYTES) + li * ROWB;
    if constexpr (PL == 2)
      mfma_row_h2<NB, MBW>(acc, accx, sb, wb, in_bytes, WP_BYTES, prow, ky * IW, kg, wswz);
    else
      mfma_row_f32<NB, MBW>(acc, sb, wb, prow, ky * IW, kg, wswz);
    if (++ky == K7) {
      ky = 0;
      ++c;
    }
  }
  if constexpr (PL == 2) {
#pragma unroll
    for (int i = 0; i < MBW; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] += accx[i][nb] * kLoInv;
  }

  // ---- epilogue (acc = conv + bias): lane holds couts cbase .. cbase + 4*NB - 1 of pixel i
#pragma unroll
  for (int i = 0; i < MBW; ++i) {
    f32x4 v[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) v[nb] = acc[i][nb];
    if (p.relu) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[nb][q] = v[nb][q] > 0.f ? v[nb][q] : 0.f;
    }
    const unsigned ooff = opix[i] >= 0 ? (unsigned)opix[i] * outpb + (p.out_coff + cbase) * ESZ : kOobOff;
    store_vec_buf<T, NB>(r_out, ooff, out_lo, v);
  }
}

// ---------------------------------------------------------------------------
// Host side: tile choice + dispatch
// ---------------------------------------------------------------------------
constexpr size_t kConv7LdsLimit = 156 * 1024;      // of the CU's 160 KiB, as conv_choose_tile's largest tiles

// Picks NB and the (G, R, TW) tile: the candidate with the fewest workgroups per cout block (every workgroup streams the
// whole weight block of its couts once, so fewer and larger tiles mean less weight traffic), among column splits into
// tiles of about 32 / 16 / 8 columns and every row count, under M = G R TW <= 256 pixels, MAXG * 64 halo rows and the LDS
// limit.  Returns the dynamic LDS bytes, 0 when nothing fits.
size_t conv7_choose_tile(ConvParams& p, int dtype, int* nb_out) {
  const int planes = dtype == UDP_F16X2 ? 2 : 1;
  const int ck = dtype == UDP_F32 ? 16 : 32;
  const int NB = p.CoutPad % 64 == 0 ? 4 : 2;
  const int nchunks = ceil_div(p.Cin, ck);
  // split fp16: one halo buffer (the planes double every byte); fp32: two, when there is a second chunk to prefetch
  p.sbuf = planes == 2 || nchunks == 1;
  const int nin = p.sbuf ? 1 : 2;
  const size_t wbytes = (size_t)2 * planes * K7 * NB * 16 * ROWB;
  auto rows = [&](int g, int r, int tw) { return g * (r + K7 - 1) * (tw + K7 - 1); };
  auto lds = [&](int g, int r, int tw) { return (size_t)nin * planes * ((rows(g, r, tw) + 15) / 16) * 16 * ROWB + wbytes; };
  auto fits = [&](int g, int r, int tw) { return g * r * tw <= 256 && rows(g, r, tw) <= MAXG * 64 && lds(g, r, tw) <= kConv7LdsLimit; };
  long best = -1;
  int bg = 0, br = 0, btw = 0;
  for (int target = 32; target >= 8; target >>= 1) {
    const int tw = ceil_div(p.Wout, ceil_div(p.Wout, target));
    for (int r = p.Hout < 256 / tw ? p.Hout : 256 / tw; r >= 1; --r) {
      if (!fits(1, r, tw)) continue;
      int g = 1;
      if (r == p.Hout && tw == p.Wout)
        while (g < p.N && fits(g + 1, r, tw)) ++g;
      const long wgs = (long)ceil_div(p.N, g) * ceil_div(p.Hout, r) * ceil_div(p.Wout, tw);
      if (best < 0 || wgs < best) {
        best = wgs;
        bg = g;
        br = r;
        btw = tw;
      }
      break;      // smaller r only adds workgroups
    }
  }
  if (best < 0) return 0;
  p.G = bg;
  p.R = br;
  p.TW = btw;
  p.IH = br + K7 - 1;
  p.IW = btw + K7 - 1;
  p.tiles_x = ceil_div(p.Wout, btw);
  p.tiles_y = ceil_div(p.Hout, br);
  auto magic = [](int d) { return (unsigned)(((1u << 20) + (unsigned)d - 1) / (unsigned)d); };   // fdiv20
  p.mIW = magic(p.IW);
  p.mIH = magic(p.IH);
  p.mRT = magic(br * btw);
  p.mTW = magic(btw);
  p.ntiles = ceil_div(p.N, bg) * p.tiles_y * p.tiles_x;
  p.mTX = p.mTY = 0;
  *nb_out = NB;
  return lds(bg, br, btw);
}

template <typename T, int NB, int MBW>
static int describe_conv7_one(const ConvParams& p, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&conv7_mfma_kernel<T, NB, MBW>);
  if (!attr_set) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  out->fn = kern;
  out->grid = dim3(p.ntiles, p.CoutPad / (NB * 16));
  out->block = dim3(256);
  out->lds = (unsigned)lds;
  out->p = p;
  return UDP_OK;
}

template <typename T>
static int describe_conv7_t(const ConvParams& p, int nb, int mbw, size_t lds, Launch* out) {
#define UDP_C7(B, M) \
  if (nb == B && mbw == M) return describe_conv7_one<T, B, M>(p, lds, out);
  UDP_C7(2, 1) UDP_C7(2, 2) UDP_C7(2, 3) UDP_C7(2, 4) UDP_C7(4, 1) UDP_C7(4, 2) UDP_C7(4, 3) UDP_C7(4, 4)
#undef UDP_C7
  return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: no kernel for nb=%d, %d pixel blocks per wave", nb, mbw);
}

// What the 7x7 conv does not do is refused, never ignored (udp_pose_hip.h, UDP_OP_CONV).  `p` carries what describe_conv
// sees; udp_conv_op.group / chain_cout are refused where the op itself is read (hrnet.hip).
int conv7_refuse(const ConvParams& p, int dtype, int stride) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: storage modes f32 and f16x2 only");
  if (stride != 1) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: stride 1 only (got %d)", stride);
  if (p.wfmt != 0) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: wfmt 0 weights ([49][cout_pad][cin]) only (got wfmt %d)", p.wfmt);
  if (p.res || p.nup || p.nout2 || p.out_nchw_f32 || p.in_stuff2 || p.out_skip || p.bn_ws)
    return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: no residual, up-sampled addends, second outputs, NCHW output, stuffed input, out_skip or BatchNorm sums");
  if (p.relu != UDP_ACT_NONE && p.relu != UDP_ACT_RELU) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: activation code %d (0 none, 1 ReLU only)", p.relu);
  if (p.Cin % 16 || p.Cout % 16) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: Cin=%d and Cout=%d must be multiples of 16", p.Cin, p.Cout);
  return UDP_OK;
}

// UDP_OP_CONV with ks = 7 (called by describe_conv after its view / size checks)
int describe_conv7(ConvParams p, int dtype, int stride, Launch* out) {
  if (const int rc = conv7_refuse(p, dtype, stride)) return rc;
  int nb = 2;
  const size_t lds = conv7_choose_tile(p, dtype, &nb);
  if (!lds) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv: no tile fits the LDS");
  if (p.CoutPad % (nb * 16) != 0) return fail(UDP_ERR_UNSUPPORTED, "7x7 conv CoutPad=%d is not a multiple of %d", p.CoutPad, nb * 16);
  const int mbw = ceil_div(ceil_div(p.G * p.R * p.TW, 16), 4);
  if (getenv("UDP_POSE_DEBUG_TILES"))
    fprintf(stderr, "conv k7 s1 %dx%d C%d->%d: G=%d R=%d TW=%d NB=%d mbw=%d halo_bufs=%d lds=%zu wgs=%d\n", p.Hout, p.Wout, p.Cin, p.Cout,
            p.G, p.R, p.TW, nb, mbw, p.sbuf ? 1 : 2, lds, p.ntiles * (p.CoutPad / (nb * 16)));
  return dtype == UDP_F32 ? describe_conv7_t<float>(p, nb, mbw, lds, out) : describe_conv7_t<H2>(p, nb, mbw, lds, out);
}

int conv7_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
