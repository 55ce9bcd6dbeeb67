// Transposed convolution of the pose_resnet head for gfx950 (MI355X, CDNA4): ConvTranspose2d(k=4, s=2, p=1) +
// BatchNorm (eval, folded) + ReLU (deep_hrnet/lib/models/pose_resnet.py:155-193, deconv_layers), one launch per layer.
//
// oy = 2*iy - 1 + ky: output row 2m+a (a in {0,1}) takes input rows m-1+a+t with ky = 3-a-2t (t in {0,1}); columns
// alike.  Each output phase (a,b) is therefore a 2x2 stride-1 conv over the input, and the four phases together read
// exactly the 3x3 input window around pixel (m,n) -- the halo of a 3x3 stride-1 pad-1 conv.  A workgroup stages that
// halo tile of an INPUT-space pixel tile once per K chunk (LDS-DMA, double-buffered, as conv_ws_h2_kernel<3,1,...>)
// and computes all four phases from it: four accumulator sets, 4*Cin*Cout MACs per output pixel (no zero-stuffing,
// no 3x3 conv with 4*Cout outputs, no intermediate tensor).  The epilogue scatters pixel (m,n) of phase (a,b) to
// output pixel (2m+a, 2n+b) of the NHWC output.
//
// Weights: 16 "taps" pt = 4*phase + tap, phase = 2a+b, tap = 2t+u, holding w[ci][co][3-a-2t][3-b-2u] (BN folded):
//   UDP_F32   (wfmt 0): fp32 [pt][cout_pad][cin]; the A fragments are loaded from global memory (L2) per lane.
//   UDP_F16X2 (wfmt 1): the fragment-major split-fp16 blocks of the weight-stationary convs (conv_ws.hip) over those
//             16 taps, scaled by 2^wexp (udp_pose_amd.f16x2.pack_deconv_weights_ws).
// Steps run chunk-major, then tap, then phase (innermost): the A-fragment ring has one slot per phase, so the ring
// slot and the accumulator set of a step are compile-time indices.
#include "conv_dev.h"

namespace udp {

template <bool F32>
struct DeconvA;
template <>
struct DeconvA<true> {
  f32x4 w[2];        // nb = 0, 1: weight row (cout) li of the block, channels 4*kg .. 4*kg+3 of the chunk
};
template <>
struct DeconvA<false> {
  f16x8 h[2], l[2];  // fragment-major hi / lo planes
};

template <typename T, int PB, int CP>
__global__ __launch_bounds__(256, 2) void deconv4s2_kernel(const ConvParams p) {
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int CK = Tr<T>::CK, ESZ = Tr<T>::ESZ, PL = Tr<T>::PL;
  constexpr int NB = 2, NW = 4, TAPS = 16;
  constexpr int LPS = F32 ? NB : 2 * NB;   // A loads per step
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15;
  const int kg = lane >> 4;
  const int cp = wave % CP, pg = wave / CP;          // 4 waves = CP cout pairs x 4/CP pixel groups
  const int cby = blockIdx.y;

  int t = blockIdx.x;   // wave-uniform tile decode (input-space tiles)
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n0 = (t / p.tiles_y) * p.G;
  const int y0 = ty * p.R;
  const int x0 = tx * p.TW;

  const int IH = p.IH, IW = p.IW;
  const int npix_in = p.G * IH * IW;
  const int in_groups = (npix_in + 15) >> 4;
  const int in_bytes = in_groups * 16 * ROWB;
  const int stage_bytes = PL * in_bytes;            // [hi image][lo image] (fp32: one image)
  const int nchunks = p.Cin / CK;
  const int nsteps = nchunks * TAPS;
  const int RT = p.R * p.TW;
  const int M = p.G * RT;
  const unsigned inpb = (unsigned)p.in_pitch * ESZ * PL, in_lo = (unsigned)p.in_pitch * ESZ;
  const unsigned outpb = (unsigned)p.out_pitch * ESZ * PL, out_lo = (unsigned)p.out_pitch * ESZ;
  const unsigned npairs = (unsigned)p.CoutPad >> 5;

  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.in), 0, (unsigned)p.N * p.Hin * p.Win * inpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.wgt), 0, F32 ? (unsigned)TAPS * p.CoutPad * p.Cin * 4u : (unsigned)TAPS * nchunks * npairs * 4096u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(
      p.out, 0, (unsigned)p.N * p.Hout * p.Wout * outpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_bias = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.bias), 0, (unsigned)p.CoutPad * 4u, 0x00020000);

  const int cwave = (cby * CP + cp) * 32;   // first cout of the wave's pair of 16-cout blocks
  const int cbase = cwave + 8 * kg;         // the lane's 8 consecutive output channels
  // A row li of block nb is cout cwave + 8*(li>>2) + 4*nb + (li&3) (fragment-major order; the fp32 rows are loaded
  // in the same order), so that the lane's accumulator rows 4*kg .. 4*kg+3 of blocks 0, 1 are couts cbase .. cbase+7
  const unsigned wvoff = (unsigned)lane * 16u;
  const unsigned wpair = (unsigned)(cby * CP + cp) * 4096u;
  const int frow = cwave + 8 * (li >> 2) + (li & 3);
  auto load_a = [&](int s, DeconvA<F32>& a) __attribute__((always_inline)) {
    const int c = s >> 4, tap = (s >> 2) & 3, ph = s & 3;
    const int pt = 4 * ph + tap;
    if constexpr (F32) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const unsigned off = ((unsigned)(pt * p.CoutPad + frow + 4 * nb) * (unsigned)p.Cin + c * CK + 4 * kg) * 4u;
        a.w[nb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_w, off, 0, 0));
      }
    } else {
      const unsigned soff = (unsigned)(pt * nchunks + c) * (npairs * 4096u) + wpair;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        a.h[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, wvoff + 2048u * nb, soff, 0));
        a.l[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, wvoff + 2048u * nb + 1024u, soff, 0));
      }
    }
  };

  // prologue: A fragments of steps 0..2 and the bias first, then the chunk-0 tile DMA
  DeconvA<F32> ra[4];
  load_a(0, ra[0]);
  load_a(1 < nsteps ? 1 : nsteps - 1, ra[1]);
  load_a(2 < nsteps ? 2 : nsteps - 1, ra[2]);
  f32x4 bias[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    bias[nb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_bias, (unsigned)(cbase + 4 * nb) * 4u, 0, 0));

  // ---- per-lane DMA offsets of the input halo tile (chunk 0); masked rows -> kOobOff -> zeros (the pad of 1)
  const int srow = lane >> 2, spart = lane & 3;
  const int gy0 = y0 - 1, gx0 = x0 - 1;
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
  auto stage = [&](int c, unsigned char* sb) __attribute__((always_inline)) {
    const unsigned coff = (unsigned)c * (CK * ESZ);
#pragma unroll
    for (int i = 0; i < MAXG; ++i) {
      const int gidx = wave + NW * i;
      if (gidx < in_groups) {
        const unsigned off = src_off[i] + coff;
        blds16(r_in, off, sb + gidx * (16 * ROWB));
        if constexpr (PL == 2) blds16(r_in, off + in_lo, sb + in_bytes + gidx * (16 * ROWB));
      }
    }
  };
  stage(0, smem);

  // ---- the lane's PB input-space pixels: LDS row of their window's top-left tap, output pixel of phase (0,0)
  int prow[PB], obase[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int m0 = (pg * PB + i) * 16 + li;
    const int m = m0 < M ? m0 : M - 1;
    const int g = fdiv20(m, p.mRT);
    const int rem = m - (int)__umul24(g, RT);
    const int r = fdiv20(rem, p.mTW);
    const int x = rem - (int)__umul24(r, p.TW);
    prow[i] = (int)__umul24(__umul24(g, IH) + r, IW) + x;
    const int n = n0 + g, y = y0 + r, xo = x0 + x;
    const bool ok = m0 < M && n < p.N && y < p.Hin && xo < p.Win && cbase < p.Cout;
    obase[i] = ok ? (int)(__umul24(__umul24(n, p.Hout) + 2 * y, p.Wout) + 2 * xo) : -1;
  }

  f32x4 acc[4][PB][NB];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int i = 0; i < PB; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[ph][i][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned char* sb = smem;
  // one step = (chunk c, tap (t,u), phase PH): window offset (a+t, b+u)
  auto step = [&](auto PHC, int g) __attribute__((always_inline)) {
    constexpr int PH = decltype(PHC)::value;
    constexpr int A = PH >> 1, B = PH & 1;
    const int c = g >> 2, tap = g & 3;
    const int s = g * 4 + PH;
    // the A fragments of step s + 3 go first (vector-memory operations complete in issue order)
    load_a(s + 3 < nsteps ? s + 3 : nsteps - 1, ra[(PH + 3) & 3]);
    if (PH == 0 && tap == 0) {
      // chunk c's DMA has landed (all but the LPS A loads just issued), for every wave; nobody reads the other
      // stage any more: the next chunk streams into it
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPS) : "memory");
      __syncthreads();
      if (c + 1 < nchunks) stage(c + 1, smem + ((c + 1) & 1) * stage_bytes);
      sb = smem + (c & 1) * stage_bytes;
    }
    const int woff = (A + (tap >> 1)) * IW + B + (tap & 1);
    const DeconvA<F32>& a = ra[PH];
    if constexpr (F32) {
      f32x4 xb[PB];
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int row = prow[i] + woff;
        xb[i] = *reinterpret_cast<const f32x4*>(sb + row * ROWB + ((kg ^ swz<float>(row)) << 4));
      }
#pragma unroll
      for (int i = 0; i < PB; ++i)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[PH][i][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w[nb][j], xb[i][j], acc[PH][i][nb], 0, 0, 0);
    } else {
      f16x8 xh[PB], xl[PB];
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int row = prow[i] + woff;
        const unsigned char* q = sb + row * ROWB + ((kg ^ swz<H2>(row)) << 4);
        xh[i] = *reinterpret_cast<const f16x8*>(q);
        xl[i] = *reinterpret_cast<const f16x8*>(q + in_bytes);
      }
      // the cross term hi * Xlo: activations keep their lo plane scaled by 2^11, the weight side carries 2^-11
      f16x8 a2[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a2[nb] = a.h[nb] * (_Float16)0x1p-11f;
#pragma unroll
      for (int i = 0; i < PB; ++i) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[PH][i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[nb], xh[i], acc[PH][i][nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[PH][i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.l[nb], xh[i], acc[PH][i][nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[PH][i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[nb], xl[i], acc[PH][i][nb], 0, 0, 0);
      }
    }
  };
  for (int g = 0; g < nchunks * 4; ++g) {
    step(std::integral_constant<int, 0>{}, g);
    step(std::integral_constant<int, 1>{}, g);
    step(std::integral_constant<int, 2>{}, g);
    step(std::integral_constant<int, 3>{}, g);
  }

  // ---- epilogue: out = act(acc * 2^-wexp + bias), phase (a,b) of pixel (m,n) -> output pixel (2m+a, 2n+b)
  const float winv = __builtin_ldexpf(1.f, -p.wexp);
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    const int poff = (ph >> 1) * p.Wout + (ph & 1);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      f32x4 v[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float f = __builtin_fmaf(acc[ph][i][nb][q], winv, bias[nb][q]);
          v[nb][q] = p.relu ? (f > 0.f ? f : 0.f) : f;
        }
      const unsigned ooff = obase[i] >= 0 ? (unsigned)(obase[i] + poff) * outpb + (p.out_coff + cbase) * ESZ : kOobOff;
      store_vec_buf<T, NB>(r_out, ooff, out_lo, v);   // (split fp16: h2_split8 raises the range flag)
    }
  }
}

template <typename T, int PB, int CP>
static int describe_deconv_one(const ConvParams& p, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&deconv4s2_kernel<T, PB, CP>);
  if (!attr_set) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  out->fn = kern;
  out->grid = dim3(p.ntiles, p.CoutPad / (CP * 32));
  out->block = dim3(256);
  out->lds = (unsigned)lds;
  out->p = p;
  return UDP_OK;
}
template <typename T>
static int describe_deconv_t(const ConvParams& p, int pb, int cp, size_t lds, Launch* out) {
#define UDP_DC(B, C) \
  if (pb == B && cp == C) return describe_deconv_one<T, B, C>(p, lds, out);
  UDP_DC(1, 4) UDP_DC(2, 4) UDP_DC(3, 4) UDP_DC(1, 2) UDP_DC(2, 2) UDP_DC(3, 2) UDP_DC(1, 1) UDP_DC(2, 1) UDP_DC(3, 1)
#undef UDP_DC
  return fail(UDP_ERR_UNSUPPORTED, "deconv: no kernel for PB=%d CP=%d", pb, cp);
}

// Tile choice + dispatch of one UDP_OP_DECONV launch.  p: Hin x Win -> Hout = 2 Hin x Wout = 2 Win, wgt / bias / in /
// out set.  Candidates (pixel blocks per wave PB, cout pairs per workgroup CP): the input-space tile is the whole
// width (or 2..4 equal column tiles), as many rows as the M = 16*PB*(4/CP) pixel slots hold, whole images side by
// side when an image fits; score = useful pixel slots x the share of a 256-workgroup chip fill reached.
int describe_deconv(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2)
    return fail(UDP_ERR_UNSUPPORTED, "deconv: storage modes f32 and f16x2 only (dtype %d)", dtype);
  const bool h2 = dtype == UDP_F16X2;
  const int ck = h2 ? 32 : 16;
  if (p.wfmt != (h2 ? 1 : 0))
    return fail(UDP_ERR_ARG, "deconv: wfmt %d (f16x2 takes fragment-major weights, wfmt 1; f32 wfmt 0)", p.wfmt);
  if (p.Cin <= 0 || p.Cin % ck || p.Cout <= 0 || p.Cout % 8 || p.CoutPad < p.Cout || p.CoutPad % 32 || p.Hin <= 0 || p.Win <= 0 ||
      p.Hout != 2 * p.Hin || p.Wout != 2 * p.Win)
    return fail(UDP_ERR_UNSUPPORTED, "deconv: C%d->%d %dx%d -> %dx%d (cin %% %d, cout %% 8, output = 2x the input)", p.Cin, p.Cout,
                p.Hin, p.Win, p.Hout, p.Wout, ck);
  if (p.res || p.nup || p.nout2 || p.out_nchw_f32 || p.in_stuff2 || p.bn_ws || !p.in || !p.out || !p.wgt || !p.bias)
    return fail(UDP_ERR_UNSUPPORTED, "deconv: plain NHWC input / output, no addends");
  if ((p.in_coff | p.in_pitch | p.out_coff | p.out_pitch) % 8 || p.in_coff + p.Cin > p.in_pitch || p.out_coff + p.Cout > p.out_pitch)
    return fail(UDP_ERR_ARG, "deconv: channel views");
  if (p.wexp < -40 || p.wexp > 40) return fail(UDP_ERR_ARG, "deconv: wexp %d", p.wexp);
  const int pairs = p.CoutPad / 32;
  struct Cand {
    int pb, cp, G, R, TW, tiles;
    size_t lds;
    double score;
  } best{};
  bool have = false;
  for (int pb : {3, 2, 1}) {
    for (int cp : {4, 2, 1}) {
      if (pairs % cp) continue;
      const int maxM = 16 * pb * (4 / cp);
      for (int split = 1; split <= 4; ++split) {
        const int TW = ceil_div(p.Win, split);
        if (TW > maxM || (split > 1 && TW < 8)) continue;
        int R = maxM / TW < p.Hin ? maxM / TW : p.Hin;
        int G = 1;
        if (R == p.Hin && TW == p.Win) {
          G = maxM / (R * TW);
          if (G > p.N) G = p.N;
          if (G < 1) G = 1;
        }
        auto npix = [&](int g, int r) { return g * (r + 2) * (TW + 2); };
        while (npix(G, R) > MAXG * 64 && G > 1) --G;
        while (npix(G, R) > MAXG * 64 && R > 1) R = (R + 1) / 2;
        if (npix(G, R) > MAXG * 64) continue;
        const int tiles = ceil_div(p.N, G) * ceil_div(p.Hin, R) * ceil_div(p.Win, TW);
        const long wgs = (long)tiles * (pairs / cp);
        const double util = (double)p.N * p.Hin * p.Win / ((double)tiles * maxM);
        const double score = util * (wgs >= 256 ? 1.0 : (double)wgs / 256.0);
        if (!have || score > best.score + 1e-9) {
          have = true;
          best = {pb, cp, G, R, TW, tiles, (size_t)2 * (h2 ? 2 : 1) * ceil_div(npix(G, R), 16) * 16 * ROWB, score};
        }
      }
    }
  }
  if (!have) return fail(UDP_ERR_UNSUPPORTED, "deconv: no tile for %dx%d C%d->%d", p.Hin, p.Win, p.Cin, p.Cout);
  p.G = best.G;
  p.R = best.R;
  p.TW = best.TW;
  p.IH = p.R + 2;
  p.IW = p.TW + 2;
  p.tiles_x = ceil_div(p.Win, p.TW);
  p.tiles_y = ceil_div(p.Hin, p.R);
  auto magic = [](int d) { return (unsigned)(((1u << 20) + (unsigned)d - 1) / (unsigned)d); };
  p.mIW = magic(p.IW);
  p.mIH = magic(p.IH);
  p.mRT = magic(p.R * p.TW);
  p.mTW = magic(p.TW);
  p.ntiles = best.tiles;
  // 32-bit buffer offsets, masked lanes at kOobOff (beyond every buffer): each tensor below that (4 bytes per element)
  if ((double)p.N * p.Hout * p.Wout * p.out_pitch * 4 >= (double)kOobOff || (double)p.N * p.Hin * p.Win * p.in_pitch * 4 >= (double)kOobOff)
    return fail(UDP_ERR_UNSUPPORTED, "deconv: a tensor of 2 GiB or more");
  if (getenv("UDP_POSE_DEBUG_TILES"))
    fprintf(stderr, "deconv %dx%d C%d->%d: G=%d R=%d TW=%d CP=%d PB=%d lds=%zu tiles=%d\n", p.Hin, p.Win, p.Cin, p.Cout, p.G, p.R,
            p.TW, best.cp, best.pb, best.lds, best.tiles);
  return h2 ? describe_deconv_t<H2>(p, best.pb, best.cp, best.lds, out) : describe_deconv_t<float>(p, best.pb, best.cp, best.lds, out);
}

int deconv_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
