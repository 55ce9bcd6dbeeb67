// Weight-stationary split-fp16 convolution kernels of the HRNet / RSN forward for gfx950 (MI355X, CDNA4) and their
// host-side tile choice, dispatch and merged-launch ordering.  Split from conv.hip (same op:
//     out = act( conv(in) + bias [+ res] [+ sum_k nearest_up(up_k)] ),
// deep_hrnet/lib/models/pose_hrnet.py:43-59, :80-100, :189-273, :344-383).
#include "conv_dev.h"

namespace udp {

// ---------------------------------------------------------------------------------------------
// Weight-stationary form for split-fp16 convs ("ws"): the MFMA A operand (weights) never passes through
// LDS.  A wave owns one pair of 16-cout blocks and keeps that pair's fragments of the current tap row
// (KS taps x 2 blocks x hi/lo) in registers -- loaded straight from global memory (L2-resident), one tap
// row ahead -- and sweeps PB pixel blocks under them; LDS holds only the input halo tile (hi + lo image,
// double-buffered over the K chunks).  Against conv_mfma_kernel<H2> (which stages 9*BN weight rows per
// chunk next to the tile) this halves the LDS-DMA instructions, leaves LDS room for two workgroups per CU
// at any K depth, drops the LDS reads per MFMA from 10/18 to 2/6, and a staged input tile serves 4 cout
// pairs (128 channels) instead of one.
//   workgroup = 4 waves = CP cout pairs x PG = 4/CP pixel groups; wave (cp, pg) computes pixel blocks
//   pg*PB .. pg*PB+PB-1 of the tile (M <= 16*PB*PG pixels) x couts (blockIdx.y*CP + cp)*32 .. +31.
// ---------------------------------------------------------------------------------------------
// UDP_WS_LATE_RES (compile time, default 1; 0 = the earlier placement, for A/B builds): the 3x3 stride-1 bodies request the
// residual at the head of the last three steps (the peeled tail of the step loop) instead of in the prologue
#ifndef UDP_WS_LATE_RES
#define UDP_WS_LATE_RES 1
#endif
// UDP_WS_FAST_EPI / UDP_WS_FAST_ADDR (compile time, default 1; 0 = the earlier code, for A/B builds): the
// same values from fewer vector-ALU instructions -- the ALU shares the SIMD with the MFMAs, and the counters show the two
// mostly adding up (NOTES).
//   FAST_EPI   the epilogue: residual decode and hi/lo split through the mixed-precision fma and the packed round-to-nearest
//              fp32 -> fp16 convert (h2_add8_fast / h2_split8_fast, conv_dev.h), the range check as one max3 chain and
//              one compare per pixel block
//   FAST_ADDR  the B-fragment LDS address: byte row offsets kept per block (kg's 16-byte part folded in), stage base + tap
//              offset as one wave-uniform term, the swizzle bit taken from the byte address
#ifndef UDP_WS_FAST_EPI
#define UDP_WS_FAST_EPI 1
#endif
#ifndef UDP_WS_FAST_ADDR
#define UDP_WS_FAST_ADDR 1
#endif
#ifdef UDP_OLD_SWZ      // (the address form below spells out the current swizzle)
#undef UDP_WS_FAST_ADDR
#define UDP_WS_FAST_ADDR 0
#endif
// UDP_WS_INC_STEP (compile time, default 1; 0 = the earlier code, for A/B builds): the step decode of the 3x3 stride-1 bodies
// (LATE below) without divisions.  A trip of their loop is one tap row, so tap % 3 is the compile-time ring slot, and
// tap / 3, the chunk, the row's byte offset and the scalar offset of the next A fragments are running values; the LDS base is
// part of the wave-uniform tap offset, so the B address loses the add of the (zero) base symbol that hipcc does not fold.
// Same MFMAs, same operands, same order (NOTES, r11: of three parts measured, the one that pulled on its own).
#ifndef UDP_WS_INC_STEP
#define UDP_WS_INC_STEP 1
#endif
#if !UDP_WS_FAST_ADDR      // (it builds on the FAST_ADDR address form)
#undef UDP_WS_INC_STEP
#define UDP_WS_INC_STEP 0
#endif
// residual of one pixel block (8 consecutive split-fp16 channels per lane), raw until the epilogue adds it
template <int NB>
struct ResH2 {
  u32x4 hi[NB / 2], lo[NB / 2];
};
template <int NB>
__device__ __forceinline__ void load_res_h2(ResH2<NB>& o, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned lo_off) {
#pragma unroll
  for (int h = 0; h < NB / 2; ++h) {
    o.hi[h] = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16 * h, 0, UDP_H2_RES_AUX);
    o.lo[h] = __builtin_amdgcn_raw_buffer_load_b128(r, voff + lo_off + 16 * h, 0, UDP_H2_RES_AUX);
  }
}
template <int NB>
__device__ __forceinline__ void add_res_h2(f32x4 (&v)[NB], const ResH2<NB>& o) {
#pragma unroll
  for (int h = 0; h < NB / 2; ++h) {
#if UDP_WS_FAST_EPI
    h2_add8_fast(v[2 * h], v[2 * h + 1], o.hi[h], o.lo[h]);
#else
    h2_add8(v[2 * h], v[2 * h + 1], __builtin_bit_cast(f16x8, o.hi[h]), __builtin_bit_cast(f16x8, o.lo[h]));
#endif
  }
}

// HS: the hard-swish / SiLU instantiations (HS = udp_conv_op.relu = UDP_ACT_HSWISH | UDP_ACT_SILU; conv_ws_hs_kernel below)
// NUP = false: a body for convs without up-sampled addends (udp_conv_op.n_up == 0), which then keeps no pixel coordinates
// XP: the wave's cout pair is given (`xpair`) instead of following from the cout block and the wave (conv_ws_s2x_kernel)
template <int KS, int STRIDE, int PB, int CP, bool NCHW, bool OUT2 = false, int HS = 0, bool NUP = true, bool XP = false>
__device__ __forceinline__ void conv_ws_body(const ConvParams& p, const int tile_id, const int cby, const int xpair = 0) {
  using T = H2;
  constexpr int CK = 32, ESZ = 2, NB = 2, NW = 4;
  constexpr int PAD = KS / 2, TAPS = KS * KS;
  // (INC_STEP adds the LDS base to the row offset in front of the swizzle, which looks at bit 8: a base aligned to 512)
  extern __shared__ __attribute__((aligned(UDP_WS_INC_STEP ? 512 : 16))) unsigned char smem[];

  UDP_STAMP(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15;
  const int kg = lane >> 4;
  const int cp = wave % CP, pg = wave / CP;          // 4 waves = CP cout pairs x 4/CP pixel groups

  int t = tile_id;   // wave-uniform tile decode
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
  const int stage_bytes = 2 * in_bytes;             // [hi image][lo image]
  const int nchunks = (p.Cin + CK - 1) / CK;
  const bool ragged = (p.Cin % CK) != 0;
  const int RT = p.R * p.TW;
  const int M = p.G * RT;
  const unsigned inpb = (unsigned)p.in_pitch * ESZ * 2;
  const unsigned outpb = (unsigned)p.out_pitch * ESZ * 2, respb = (unsigned)p.res_pitch * ESZ * 2;
  const unsigned in_lo = (unsigned)p.in_pitch * ESZ;
  const unsigned out_lo = (unsigned)p.out_pitch * ESZ, res_lo = (unsigned)p.res_pitch * ESZ;

  const unsigned out_pix = (unsigned)p.N * p.Hout * p.Wout;
  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.in), 0, (unsigned)p.N * p.Hin * p.Win * inpb, 0x00020000);
  const unsigned npairs = (unsigned)p.CoutPad >> 5;
  const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.wgt), 0, (unsigned)TAPS * nchunks * npairs * 4096u, 0x00020000);
  // (no `out`: second outputs only, udp_conv_op.n_out2 -- a zero-length descriptor drops the stores)
#if UDP_WS_DBG & 32      // (timing-only build: the one-chunk convs store nothing)
  const bool dbg_nost = nchunks == 1;
#else
  constexpr bool dbg_nost = false;
#endif
#if UDP_WS_DBG & 64      // (timing-only build: the one-chunk convs read no residual)
  const bool dbg_nores = nchunks == 1;
#else
  constexpr bool dbg_nores = false;
#endif
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(
      p.out, 0, (!p.out || dbg_nost) ? 0 : NCHW ? (out_pix + (unsigned)p.out_skip * p.Hout * p.Wout) * p.Cout * 4 : out_pix * outpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_bias = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.bias), 0, (unsigned)p.CoutPad * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_res = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void*>(p.res), 0, (p.res && !dbg_nores) ? out_pix * respb : 0, 0x00020000);

  const int pair = XP ? xpair : cby * CP + cp;
  const int cwave = pair * 32;              // first cout of the wave's pair of blocks
  const int cbase = cwave + 8 * kg;                // the lane's 8 consecutive output channels
  // ---- weights (fragment-major, udp_conv_op.wfmt == 1): the 1 KiB block (tap, chunk, cout pair, nb, plane) holds
  // lane l's 8 K values at 16*l -- A-fragment row li of block nb is cout cwave + 8*(li>>2) + 4*nb + (li&3), so
  // that a lane ends up with 8 consecutive couts.  One contiguous load per fragment; cin is zero-padded.
  const unsigned wvoff = (unsigned)lane * 16u;
  const unsigned wpair = (unsigned)pair * 4096u;
  // A fragments of one tap (2 blocks x hi/lo = 16 registers) in a ring of three: the fragments of step s + 2
  // stream in from L2 while step s feeds the MFMAs (step = one tap of one K chunk)
  constexpr int AD = UDP_WS_AD;          // depth of the A ring (fragments of step s + AD - 1 are in flight)
  f16x8 ah[AD][NB], al[AD][NB];
  const int nsteps = nchunks * TAPS;
  auto load_a_at = [&](unsigned soff, f16x8 (&h)[NB], f16x8 (&l)[NB]) __attribute__((always_inline)) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      h[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, wvoff + 2048u * nb, soff, 0));
      l[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, wvoff + 2048u * nb + 1024u, soff, 0));
    }
  };
  auto load_a = [&](int s, f16x8 (&h)[NB], f16x8 (&l)[NB]) __attribute__((always_inline)) {
    const int c = s / TAPS, tap = s - c * TAPS;
    load_a_at((unsigned)(tap * nchunks + c) * (npairs * 4096u) + wpair, h, l);
  };

  // The prologue issues every load it can before it waits for any: A fragments of steps 0 and 1 and the bias first
  // (L2), then the chunk-0 tile DMA, then the residual (consumed in the epilogue) -- ONE memory round trip before
  // the first MFMA.  (The in-kernel timeline had three in a row: the bias, used to initialise the accumulators, made
  // hipcc wait for the DMA issued before it; only then were the A and residual loads issued, and the residual was
  // added -- waited for -- before the loop: 4.2 us of every 15-68 us workgroup lifetime, tools/stamp_multi.py.)
#pragma unroll
  for (int k = 0; k < AD - 1; ++k) load_a(k < nsteps ? k : nsteps - 1, ah[k], al[k]);
  f32x4 bias[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    bias[nb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_bias, (unsigned)(cbase + 4 * nb) * 4u, 0, 0));

  // ---- per-lane DMA offsets of the input halo tile (chunk 0); masked rows -> kOobOff -> zeros
  const int srow = lane >> 2, spart = lane & 3;
  const int gy0 = y0 * STRIDE - PAD, gx0 = x0 * STRIDE - PAD;
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
    const bool cut = ragged && c == nchunks - 1;
    const int parts_left = (p.Cin - c * CK) / 8;
#pragma unroll
    for (int i = 0; i < MAXG; ++i) {
      const int gidx = wave + NW * i;
      if (gidx < in_groups) {
        unsigned off = src_off[i] + coff;
        if (cut && (spart ^ swz<T>(gidx * 16 + srow)) >= parts_left) off = kOobOff;
        blds16(r_in, off, sb + gidx * (16 * ROWB));
        blds16(r_in, off + in_lo, sb + in_bytes + gidx * (16 * ROWB));
      }
    }
  };

  UDP_STAMP(1);
  stage(0, smem);      // chunk 0 is on its way while the rest of the per-lane state is set up

  // ---- the lane's PB output pixels
  int prow[PB], opix[PB], ocrd[NCHW || NUP ? PB : 1];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int m0 = (pg * PB + i) * 16 + li;
    const int m = m0 < M ? m0 : M - 1;
    const int g = fdiv20(m, p.mRT);
    const int rem = m - (int)__umul24(g, RT);
    const int r = fdiv20(rem, p.mTW);
    const int x = rem - (int)__umul24(r, p.TW);
    prow[i] = (int)__umul24(__umul24(g, IH) + r * STRIDE, IW) + x * STRIDE;
#if UDP_WS_FAST_ADDR
    prow[i] = prow[i] * ROWB + (kg << 4);      // byte offset of the row in a plane, the lane's unswizzled part in bits 4..5
#endif
    const int n = n0 + g, y = y0 + r, xo = x0 + x;
    const bool ok = m0 < M && n < p.N && y < p.Hout && xo < p.Wout && (NCHW || cbase < p.Cout);
    const unsigned pix = __umul24(__umul24(n, p.Hout) + y, p.Wout) + xo;
    opix[i] = ok ? (int)pix : -1;
    if constexpr (NCHW || NUP) ocrd[i] = ok ? (y | (xo << 10) | (n << 20)) : -1;
  }

  // ONE accumulator set: the weights are stored scaled by 2^wexp (power of two, exact) so that their largest
  // magnitude sits in [2^13, 2^14): the lo plane then holds the plain fp16 residual w*2^wexp - hi (no second scale
  // needed to keep it normal), and the three MFMAs of a product -- hi*Xhi, lo*Xhi, (hi*2^-11)*Xlo' -- all add into
  // the same fp32 accumulator, which carries conv*2^wexp; the epilogue computes acc*2^-wexp + bias (+ residual).
  // Against the earlier pair of accumulators (cross terms apart, folded in at the end) this frees 8*PB registers,
  // which now hold the residual from the prologue to the epilogue.
  const float winv = __builtin_ldexpf(1.f, -p.wexp);
  f32x4 acc[PB][NB];
#pragma unroll
  for (int i = 0; i < PB; ++i)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[i][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // residual: issued right behind the chunk-0 DMA (no res: a zero-length descriptor, the loads return zeros -- no
  // branch around loads, see the A ring), added in the epilogue.  The barriers keep hipcc from moving these loads in
  // front of the DMA: the first wait below counts them as YOUNGER than it.
  //
  // LATE (3x3 stride 1): the residual is only needed after the last MFMA, and between the DMA and the first MFMA its
  // PB * NB loads -- in MFMA fragment order, a cache line per lane -- stand in front of the loop while their PB * 8
  // registers are held through all of it.  So the last three steps (taps 6, 7, 8 of the last chunk: exactly the last
  // trip of the ring of three) are peeled out of the step loop as straight-line code, and the residual is requested at
  // the head of that tail, right behind the tail's only A loads (the fragments of tap 8; taps 6 and 7 were fetched at
  // taps 4 and 5): no A fragment queues behind it, and nothing in the tail waits for it -- the tail has no tap-0 wait,
  // the last chunk's DMA was waited for at its tap 0 (or, with one stage buffer, by the refill's vmcnt(0)).  Still
  // unconditional loads against the zero-length descriptor when there is no residual.
  constexpr bool LATE = UDP_WS_LATE_RES && KS == 3 && STRIDE == 1 && !NCHW && AD == 3;
  constexpr int NR = NCHW ? 0 : PB * NB;          // buffer loads per lane
  ResH2<NB> rres[NCHW ? 1 : PB];
  // (8 blocks: the second half of the blocks at the head of tap 7, where no A load is issued either and the ring slot of
  // tap 6 is free -- all 16 at tap 6 next to the full A ring exceed the 256 registers)
  constexpr int RSPLIT = LATE && PB > 6 ? PB / 2 : PB;
  auto load_res = [&](auto I0, auto I1) __attribute__((always_inline)) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = decltype(I0)::value; i < (NCHW ? 0 : decltype(I1)::value); ++i)
      load_res_h2(rres[i], r_res, opix[i] >= 0 ? (unsigned)opix[i] * respb + (p.res_coff + cbase) * ESZ : kOobOff, res_lo);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  if constexpr (!LATE) load_res(std::integral_constant<int, 0>{}, std::integral_constant<int, PB>{});

  UDP_STAMP(2);
  int c = 0, tap = 0;                     // chunk / tap of the current step
  const unsigned char* sb = smem;
  // INC_STEP: the same as running values -- the tap row dy = tap / 3 and its byte offset dy * IW * ROWB advance once per trip
  // of the LATE loop, the scalar offset of the A fragments to request next once per step, the stage's LDS address per chunk
  constexpr bool INC = UDP_WS_INC_STEP && LATE;
  using lds_u8 = const __attribute__((address_space(3))) unsigned char*;
  using lds_f16x8 = const __attribute__((address_space(3))) f16x8*;
  [[maybe_unused]] const unsigned lds0 = INC ? (unsigned)(size_t)(lds_u8)smem : 0u;
  [[maybe_unused]] const unsigned a_tap = (unsigned)nchunks * (npairs * 4096u);      // from one tap to the next of a chunk
  [[maybe_unused]] unsigned a_next = (unsigned)(AD - 1) * a_tap + wpair;             // (the prologue fetched steps 0 .. AD - 2)
  [[maybe_unused]] int dy = 0;
  [[maybe_unused]] unsigned row_off = 0, sb_off = lds0;
  // TAIL: -1 inside the step loop; 0, 1, 2 = taps 6, 7, 8 of the last chunk in the peeled tail (LATE only)
  auto step = [&](auto BUFC, auto TAILC, int s) __attribute__((always_inline)) {
    constexpr int BUF = decltype(BUFC)::value, TAIL = decltype(TAILC)::value;
    // the A loads go first: vector-memory operations complete in issue order, fragments queued behind the
    // next chunk's DMA would wait for it
    // (issued unconditionally -- past the end the last step's fragments are fetched again: a prefetch under a
    // branch makes hipcc assume nothing newer is in flight and wait with vmcnt(0) at every use.  LATE: the loop never
    // runs past the end, and the tail knows where it is -- tap 6 fetches the last step's fragments, taps 7 and 8 nothing)
#if !(UDP_WS_DBG & 1)
    if constexpr (!LATE)
      load_a(s + AD - 1 < nsteps ? s + AD - 1 : nsteps - 1, ah[(BUF + AD - 1) % AD], al[(BUF + AD - 1) % AD]);
    else if constexpr (TAIL <= 0) {
      if constexpr (INC) {
        // (tap BUF + 2 of this row; behind tap 2 of the last row comes tap 0 of the next chunk)
        load_a_at(a_next, ah[(BUF + AD - 1) % AD], al[(BUF + AD - 1) % AD]);
        a_next += (BUF == 0 && dy == KS - 1) ? npairs * 4096u - (unsigned)(TAPS - 1) * a_tap : a_tap;
      } else {
        load_a(s + AD - 1, ah[(BUF + AD - 1) % AD], al[(BUF + AD - 1) % AD]);
      }
    }
#endif
    if constexpr (TAIL == 0) load_res(std::integral_constant<int, 0>{}, std::integral_constant<int, RSPLIT>{});
    if constexpr (TAIL == 1 && RSPLIT < PB) load_res(std::integral_constant<int, RSPLIT>{}, std::integral_constant<int, PB>{});
    if (TAIL < 0 && (INC ? BUF == 0 && dy == 0 : tap == 0)) {
      // chunk c's DMA has landed (vector-memory operations complete in issue order: all but the 2*NB A loads
      // just issued, which may stay in flight; letting the previous step's stay in flight too changes nothing)
      if (c == 1) UDP_STAMP(9);                           // (diagnostic builds only: chunk-boundary stamps of chunks 1, 2, 4)
      if (c == 2) UDP_STAMP(11);
      if (c == 4) UDP_STAMP(13);
      // (at s == 0 the residual loads, where the prologue issued them behind the chunk-0 DMA, may stay in flight as well)
      bool refill = false;
      if constexpr (STRIDE == 2 || OUT2) refill = p.sbuf && c > 0;   // (not in the merged kernel: its members keep two stages)
      if (refill) {
        // ONE stage buffer (convs launched on their own whose two stage buffers exceed half the LDS -- stride-2 convs with
        // several K chunks: 4x input tile, 110 KB; 3x3 convs on 48-pixel-wide rows of 64+ channels: 128 KB -- i.e. one
        // workgroup, four waves, per CU; with one buffer two workgroups fit and hide each other's DMA):
        // refill it once every wave has left chunk c - 1, wait for it (the A loads just issued are older), go on
        __syncthreads();
        stage(c, smem);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        sb = smem;
        if constexpr (INC) sb_off = lds0;
      } else {
        if (s == 0)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB + (LATE ? 0 : NR)) : "memory");
        else
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB) : "memory");
        if (s == 0) UDP_STAMP(3);
        __syncthreads();                                    // ... for every wave; nobody reads the other stage any more
        if (s == 0) UDP_STAMP(4);
        if (c == 1) UDP_STAMP(10);
        if (c == 2) UDP_STAMP(12);
        if (c == 4) UDP_STAMP(14);
#if !(UDP_WS_DBG & 4)
        if (c + 1 < nchunks && !((STRIDE == 2 || OUT2) && p.sbuf)) stage(c + 1, smem + ((c + 1) & 1) * stage_bytes);
#endif
        sb = smem + (c & 1) * stage_bytes;
        if constexpr (INC) sb_off = lds0 + (unsigned)((c & 1) * stage_bytes);
      }
    }
    // the cross term hi * Xlo: activations keep their lo plane scaled by 2^11 (storage format), so the weight side
    // carries 2^-11 -- four packed fp16 multiplies per fragment and step (exact unless the product goes subnormal,
    // i.e. for weights below 2^-17 of the layer's largest: an absolute error of 2^-25 there)
    f16x8 a2[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) a2[nb] = ah[BUF][nb] * (_Float16)0x1p-11f;
    const int tap_rows = KS == 1 ? 0 : TAIL >= 0 ? (KS - 1) * IW + TAIL : (tap / KS) * IW + tap % KS;
    // B fragments (hi, lo) in a ring of three: the LDS reads of block i + 2 are issued before the MFMAs of
    // block i (one wave per SIMD has nothing else to cover the ~200-cycle LDS latency with)
    f16x8 xh[3], xl[3];
#if UDP_WS_FAST_ADDR
    // stage base + tap offset: one wave-uniform byte offset per step (a stage is a multiple of 2 KiB, so bits 6.. of the
    // sum are still the row's: swz<H2>(row) = bit 2 of the row = bit 8 of the byte offset, applied to bit 5 = part bit 1)
    // (INC_STEP: the stage's LDS address + the row's running offset + the tap's place in the row; in the tail BUF = TAIL and
    // row_off stands at the last row)
    const unsigned tap_off = INC ? sb_off + row_off + (unsigned)(BUF * ROWB) : (unsigned)(sb - smem) + (unsigned)tap_rows * ROWB;
    auto load_b = [&](int i, f16x8& h, f16x8& l) __attribute__((always_inline)) {
      const unsigned rb = (unsigned)prow[i] + tap_off;
      // rb ^ ((rb >> 3) & 32) as shift + one three-input bit operation (table 0x6c = (a & c) ^ b)
      const unsigned a = __builtin_amdgcn_bitop3_b32(rb >> 3, rb, 32u, 0x6c);
      if constexpr (INC) {      // `a` is the LDS address itself
        h = *reinterpret_cast<lds_f16x8>((size_t)a);
        l = *reinterpret_cast<lds_f16x8>((size_t)(a + (unsigned)in_bytes));
      } else {
        const unsigned char* q = smem + a;
        h = *reinterpret_cast<const f16x8*>(q);
        l = *reinterpret_cast<const f16x8*>(q + in_bytes);
      }
    };
#else
    auto load_b = [&](int i, f16x8& h, f16x8& l) __attribute__((always_inline)) {
      const int row = prow[i] + tap_rows;
      const unsigned char* q = sb + row * ROWB + ((kg ^ swz<T>(row)) << 4);
      h = *reinterpret_cast<const f16x8*>(q);
      l = *reinterpret_cast<const f16x8*>(q + in_bytes);
    };
#endif
    load_b(0, xh[0], xl[0]);
    if (PB > 1) load_b(1, xh[1], xl[1]);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
#if !(UDP_WS_DBG & 2)
      if (i + 2 < PB) load_b(i + 2, xh[(i + 2) % 3], xl[(i + 2) % 3]);
#endif
      __builtin_amdgcn_sched_barrier(0);   // keep those LDS reads ahead of this block's MFMAs (hipcc sinks them otherwise)
#if UDP_WS_DBG & 16      // (timing-only build: one MFMA instead of six per block, everything else in place)
      acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[BUF][0] + al[BUF][1] + a2[0] + a2[1], xh[i % 3] + xl[i % 3], acc[i][0], 0, 0, 0);
#else
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[BUF][nb], xh[i % 3], acc[i][nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[BUF][nb], xh[i % 3], acc[i][nb], 0, 0, 0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[nb], xl[i % 3], acc[i][nb], 0, 0, 0);
#endif
    }
    if constexpr (TAIL < 0) {
      if constexpr (INC) {
        if constexpr (BUF == KS - 1) {      // the row is done
          ++dy;
          row_off += (unsigned)IW * ROWB;
          if (dy == KS) {
            dy = 0;
            row_off = 0;
            ++c;
          }
        }
      } else if (++tap == TAPS) {
        tap = 0;
        ++c;
      }
    }
  };
  constexpr std::integral_constant<int, -1> LOOP{};
  if constexpr (LATE) {
    // nsteps = 9 * nchunks: whole trips of the ring of three, the last of them peeled (sb stays the last chunk's stage)
    for (int s = 0; s < nsteps - AD; s += AD) {
      step(std::integral_constant<int, 0>{}, LOOP, s);
      step(std::integral_constant<int, 1>{}, LOOP, s + 1);
      step(std::integral_constant<int, 2>{}, LOOP, s + 2);
    }
    step(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, nsteps - 3);
    step(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, nsteps - 2);
    step(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, nsteps - 1);
  } else {
    for (int s = 0; s < nsteps; s += AD) {
      step(std::integral_constant<int, 0>{}, LOOP, s);
      if (s + 1 < nsteps) step(std::integral_constant<int, 1>{}, LOOP, s + 1);
      if (s + 2 < nsteps) step(std::integral_constant<int, 2>{}, LOOP, s + 2);
      if constexpr (AD > 3) if (s + 3 < nsteps) step(std::integral_constant<int, 3>{}, LOOP, s + 3);
      if constexpr (AD > 4) if (s + 4 < nsteps) step(std::integral_constant<int, 4>{}, LOOP, s + 4);
      if constexpr (AD > 5) if (s + 5 < nsteps) step(std::integral_constant<int, 5>{}, LOOP, s + 5);
    }
  }
  UDP_STAMP(5);
  // conv = acc * 2^-wexp; + bias; + residual (hi + lo * 2^-11)
#pragma unroll
  for (int i = 0; i < PB; ++i) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][nb][q] = __builtin_fmaf(acc[i][nb][q], winv, bias[nb][q]);
    if constexpr (!NCHW) add_res_h2(acc[i], rres[i]);
  }

  // ---- epilogue: lane holds couts cbase .. cbase + 7 of pixel i
#if UDP_WS_FAST_EPI
  [[maybe_unused]] const float relu_lim = p.relu ? 0.f : __builtin_nanf("");
#endif
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    f32x4 v[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) v[nb] = acc[i][nb];
    if constexpr (NCHW) {
      const int crd = ocrd[i];
      const int y = crd & 1023, xo = (crd >> 10) & 1023, n = crd >> 20;
      const unsigned hw = __umul24(p.Hout, p.Wout);
      const int no = n >= p.flip_from ? n + p.out_skip : n;     // ConvParams::out_skip (0 everywhere but in a sub-batch lane)
      const unsigned base = __umul24(__umul24(__umul24(no, p.Cout), p.Hout) + y, p.Wout) + xo;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cc = cbase + 4 * nb + q;
          float f = v[nb][q];
          if (p.relu) f = f > 0.f ? f : 0.f;
          const unsigned off = (crd >= 0 && cc < p.Cout) ? (base + cc * hw) * 4u : kOobOff;
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, f), r_out, off, 0, 0);
        }
    } else {
      const unsigned ooff = opix[i] >= 0 ? (unsigned)opix[i] * outpb + (p.out_coff + cbase) * ESZ : kOobOff;
      if (NUP && p.nup) {   // wave-uniform, rare (exchange-unit outputs only)
        const int crd = ocrd[NUP ? i : 0];
        const int y = crd & 1023, xo = (crd >> 10) & 1023, n = crd >> 20;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          if (u < p.nup) {
            const int sh = p.up_shift[u];
            const long up_pix = ((long)(n * (p.Hout >> sh) + (y >> sh)) * (p.Wout >> sh) + (xo >> sh));
            if (crd >= 0)
              add_vec<T, NB>(v, reinterpret_cast<const unsigned char*>(p.up[u]) + (up_pix * p.Cout * 2 + cbase) * ESZ, p.Cout * ESZ);
          }
        }
      }
#if UDP_WS_FAST_EPI
      // the range check follows the activation as before (h2_split8): one max3 chain and one compare per block
      unsigned mag;
      if constexpr (HS) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[nb][q] = act_hs<HS>(v[nb][q]);
        mag = h2_mag8<false>(0u, v[0], v[1]);
      } else {
        // ReLU without a branch around it (relu_lim: 0, or a NaN that lets every value through), so that the blocks' code
        // does not have to meet again behind one; only the maximum for the range check still depends on which it was
        relu8_fast(v[0], v[1], relu_lim);
        mag = p.relu ? h2_mag8<true>(0u, v[0], v[1]) : h2_mag8<false>(0u, v[0], v[1]);
      }
      // (one check per block, not one per wave: with the blocks' code free to mix, conv_ws_multi<1> spills two more SGPRs)
      h2_range_check_bits(mag);
      u32x4 shi, slo;
      h2_split8_fast(v[0], v[1], shi, slo);
      __builtin_amdgcn_raw_buffer_store_b128(shi, r_out, ooff, 0, UDP_H2_STORE_AUX);
      __builtin_amdgcn_raw_buffer_store_b128(slo, r_out, ooff + out_lo, 0, UDP_H2_STORE_AUX);
#else
      if constexpr (HS) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[nb][q] = act_hs<HS>(v[nb][q]);
      } else
      if (p.relu) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[nb][q] = v[nb][q] > 0.f ? v[nb][q] : 0.f;
      }
      store_vec_buf<T, NB>(r_out, ooff, out_lo, v);
#endif
      // (only in the kernels of convs launched on their own: with this code the merged kernel spills 4 KB per lane)
      if (OUT2 && p.nout2) {   // wave-uniform, rare (RSN bottleneck): out2_k = out AS STORED + add2_k (udp_conv_op.n_out2)
        f16x8 sh, sl;
        h2_split8(v[0], v[1], sh, sl);
        f32x4 vr[NB];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          vr[0][q] = (float)sh[q] + (float)sl[q] * kLoInv;
          vr[1][q] = (float)sh[4 + q] + (float)sl[4 + q] * kLoInv;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (u < p.nout2 && opix[i] >= 0) {
            const size_t px = (size_t)opix[i];
            const _Float16* a = reinterpret_cast<const _Float16*>(p.add2[u]) + px * (2 * (size_t)p.add2_pitch[u]) + p.add2_coff[u] + cbase;
            const f16x8 ah8 = *reinterpret_cast<const f16x8*>(a), al8 = *reinterpret_cast<const f16x8*>(a + p.add2_pitch[u]);
            f32x4 w[NB];
#pragma unroll
            for (int q = 0; q < 4; ++q) {      // fuse_sum_kernel's order: addend first, then the conv output
              w[0][q] = ((float)ah8[q] + (float)al8[q] * kLoInv) + vr[0][q];
              w[1][q] = ((float)ah8[4 + q] + (float)al8[4 + q] * kLoInv) + vr[1][q];
            }
            f16x8 oh, ol;
            h2_split8(w[0], w[1], oh, ol);
            _Float16* o2 = reinterpret_cast<_Float16*>(p.out2[u]) + px * (2 * (size_t)p.out2_pitch[u]) + p.out2_coff[u] + cbase;
            *reinterpret_cast<f16x8*>(o2) = oh;
            *reinterpret_cast<f16x8*>(o2 + p.out2_pitch[u]) = ol;
          }
        }
      }
    }
  }
  UDP_STAMP(6);
#ifdef UDP_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  UDP_STAMP(7);
#endif
}

// Flat workgroup index of a conv -> (tile, cout block).  The cout blocks of one pixel tile stage the same input
// tile: they are placed 8 workgroups apart -- same XCD (workgroup i runs on XCD i % 8), started together -- so the
// second read of the tile hits that XCD's L2 instead of HBM: groups of 8 tiles x all cout blocks, cout-block-major
// inside the group (the last ntiles % 8 tiles form a smaller group).  Wave-uniform.
__host__ __device__ __forceinline__ void ws_decode(unsigned b, unsigned ntiles, unsigned nc, int& tile, int& cby) {
  if (nc == 1) {
    tile = (int)b;
    cby = 0;
    return;
  }
  const unsigned full = (ntiles >> 3) * 8u * nc;
  unsigned base = 0, width = 8, r = b;
  if (b < full) {
    const unsigned g = b / (8u * nc);
    r = b - g * 8u * nc;
    base = g * 8u;
  } else {
    r = b - full;
    base = (ntiles >> 3) * 8u;
    width = ntiles & 7u;
  }
  const unsigned c = r / width;
  cby = (int)c;
  tile = (int)(base + r - c * width);
}

template <int KS, int STRIDE, int PB, int CP, bool NCHW>
__global__ __launch_bounds__(256, 2) void conv_ws_h2_kernel(const ConvParams p) {
  int tile, cby;
  ws_decode(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x, gridDim.y, tile, cby);   // dispatch order = flat index
  conv_ws_body<KS, STRIDE, PB, CP, NCHW, KS == 3 && STRIDE == 1 && !NCHW>(p, tile, cby);
}

// 1x1 stride-1 NHWC conv + hard-swish / SiLU (udp_conv_op.relu == ACT): the same body with the HS epilogue
template <int PB, int CP, int ACT>
__global__ __launch_bounds__(256, 2) void conv_ws_hs_kernel(const ConvParams p) {
  int tile, cby;
  ws_decode(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x, gridDim.y, tile, cby);
  conv_ws_body<1, 1, PB, CP, false, false, ACT>(p, tile, cby);
}

// Merged launch of up to 4 independent weight-stationary convs (same-depth convs of different HRNet branches):
// every member runs the 6-pixel-blocks-per-wave body with its own cout-pair split (ConvMulti::code = CP), or the
// 8-block one-pair body (code 8, below).
#ifndef UDP_WS_MPB
#define UDP_WS_MPB 6      // pixel blocks per wave of the merged kernel's members
#define UDP_WS_MOCC 2     // workgroups per CU the merged kernel is compiled for (waves per SIMD)
#endif
// A one-pair (32 output channels) 3x3 member may run 8 pixel blocks per wave instead: 512-pixel tiles, a third more
// pixels under the same per-wave fixed cost.  ConvMulti::code = 8, code field 3 of a table entry.  The registers for
// two more blocks of accumulators and residual come from the late residual (conv_ws_body, LATE), so the arm exists
// only in builds that have it.
constexpr int kWsCode8 = 8;
constexpr bool kWsHave8 = UDP_WS_MPB == 6 && UDP_WS_LATE_RES && UDP_WS_AD == 3;
template <int KS>
__global__ __launch_bounds__(256, UDP_WS_MOCC) void conv_ws_multi(const ConvMulti m) {
  const unsigned b = blockIdx.x;
  int j, tile, cby;
  // (readfirstlane: the dynamically indexed kernel-argument reads are uniform, the compiler does not see it and
  // would wrap every weight load of the body in a waterfall loop)
  int code;
  // the table entry is fetched together with tab_n (its address only needs blockIdx; entry 0 when out of range)
  const unsigned e = __builtin_amdgcn_readfirstlane(m.tab[(b >> 3) < (unsigned)kMultiTab ? (b >> 3) : 0u]);
  if (m.tab_n) {
    j = (int)(e & 3u);
    code = 1 << ((e >> 2) & 3u);
    cby = (int)((e >> 4) & 63u);
    tile = (int)((e >> 10) + (b & 7u));
  } else {
    int sg = 0;
#pragma unroll
    for (int k = 1; k < kMultiSegs; ++k) sg += b >= m.seg_start[k];
    j = __builtin_amdgcn_readfirstlane(m.seg_mem[sg]);
    const unsigned r = __builtin_amdgcn_readfirstlane(b - m.seg_start[sg] + m.seg_first[sg]);
    ws_decode(r, m.tiles[j], m.ncby[j], tile, cby);
    tile = __builtin_amdgcn_readfirstlane(tile);
    cby = __builtin_amdgcn_readfirstlane(cby);
    code = m.code[j];
  }
  if constexpr (KS == 3 && kWsHave8) {
    // one cout pair, 8 pixel blocks per wave (code field 3 of the table entry); 3x3 only, see describe_conv_ws
    if (code == kWsCode8) {
      conv_ws_body<KS, 1, 8, 1, false, false, 0, false>(m.p[j], tile, (int)cby);
      return;
    }
  }
  switch (code) {
    case 1: conv_ws_body<KS, 1, UDP_WS_MPB, 1, false>(m.p[j], tile, (int)cby); break;
    case 2: conv_ws_body<KS, 1, UDP_WS_MPB, 2, false>(m.p[j], tile, (int)cby); break;
    default: conv_ws_body<KS, 1, UDP_WS_MPB, 4, false>(m.p[j], tile, (int)cby); break;
  }
}

// The 8-block body on a launch of its own: only for a conv that was described as a member of a merged launch and then
// found no sibling to share it with (hrnet.hip, make_nodes).
__global__ __launch_bounds__(256, 2) void conv_ws_pb8_kernel(const ConvParams p) {
  conv_ws_body<3, 1, 8, 1, false, false, 0, false>(p, (int)blockIdx.x, (int)blockIdx.y);
}

// ---------------------------------------------------------------------------------------------------------------
// Shared-input launch of an exchange unit (hrnet.hip, mark_x0_share): the branch-0 map x0 (32 channels, the largest map
// of its stage) is read by up to three 3x3 stride-2 convs (fuse_layers.i.0.0: 32 -> 64 | 32 | 32) and by the unit's
// element-wise output 0 (fuse0: relu(x0 + up-sampled addends)).  The convs have one geometry and one K chunk, so ONE
// staged halo tile serves all their cout pairs: a workgroup = CP cout-pair slots, slot s runs the unchanged body with
// the weights / bias / residual / addends / output view of its route (ConvShare::route, ::lpair; wave-uniform).  A slot
// without a route (three pairs under CP = 4) runs the body with a pair index far past its route's last pair: every
// load of it is out of its descriptor's range (zeros) or masked and every store dropped; it takes the barriers and
// stages its share of the tile like any other wave.
//
// Side output: with its halo cut off, the stride-2 tile is exactly the 2R x 2TW patch of x0 under the tile's output
// pixels -- input rows 1..2R, columns 1..2TW of the staged tile -- and these patches partition the map.  After the
// convs' epilogue (one K chunk: the tile is still resident and nothing writes LDS again, so no barrier is needed) the
// workgroup reads the patch back from LDS and writes fuse0's output for it, in fuse_sum_kernel's operation order.
__device__ __forceinline__ void s2x_side(const ConvParams& p, const ConvParams& f, const int tile_id) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int t = tile_id;   // the body's tile decode
  const int tx = t % p.tiles_x;
  t /= p.tiles_x;
  const int ty = t % p.tiles_y;
  const int n0 = (t / p.tiles_y) * p.G;
  const int IH = p.IH, IW = p.IW;
  const int in_bytes = ((p.G * IH * IW + 15) >> 4) * 16 * ROWB;
  const int PW = 2 * p.TW, PHW = 2 * p.R * PW;       // the patch of one image
  const int gy0 = 2 * ty * p.R, gx0 = 2 * tx * p.TW;
  const int items = p.G * PHW * 4;                   // 16-byte parts: four consecutive lanes write one pixel's 64 bytes per plane
  const unsigned outpb = (unsigned)f.out_pitch * 4u, out_lo = (unsigned)f.out_pitch * 2u;
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(f.out, 0, (unsigned)f.N * f.Hout * f.Wout * outpb, 0x00020000);
  for (int it = threadIdx.x; it < items; it += 256) {
    const int part = it & 3, pp = it >> 2;
    const int g = fdiv20(pp, f.mRT);
    const int rem = pp - g * PHW;
    const int r = fdiv20(rem, f.mTW);
    const int x = rem - r * PW;
    const int n = n0 + g, gy = gy0 + r, gx = gx0 + x;
    if (n >= p.N || gy >= p.Hin || gx >= p.Win) continue;
    const int row = (g * IH + r + 1) * IW + x + 1;
    const unsigned char* q = smem + row * ROWB + ((part ^ swz<H2>(row)) << 4);
    const f16x8 hi = *reinterpret_cast<const f16x8*>(q), lo = *reinterpret_cast<const f16x8*>(q + in_bytes);
    f32x4 v[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[0][k] = (float)hi[k] + (float)lo[k] * kLoInv;
      v[1][k] = (float)hi[4 + k] + (float)lo[4 + k] * kLoInv;
    }
    const int c = 8 * part;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      if (u < f.nup) {
        const int sh = f.up_shift[u];
        const size_t up_pix = ((size_t)(n * (f.Hout >> sh) + (gy >> sh)) * (f.Wout >> sh) + (gx >> sh));
        add_vec<H2, 2>(v, reinterpret_cast<const unsigned char*>(f.up[u]) + (up_pix * f.Cout * 2 + c) * 2, f.Cout * 2);
      }
    }
    if (f.relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[0][k] = v[0][k] > 0.f ? v[0][k] : 0.f;
        v[1][k] = v[1][k] > 0.f ? v[1][k] : 0.f;
      }
    }
    const unsigned pix = __umul24(__umul24(n, p.Hin) + gy, p.Win) + gx;
    store_vec_buf<H2, 2>(r_out, pix * outpb + (unsigned)(f.out_coff + c) * 2u, out_lo, v);
  }
}

template <int PB, int CP>
__global__ __launch_bounds__(256, 2) void conv_ws_s2x_kernel(const ConvShare m) {
  // (readfirstlane: see conv_ws_multi -- the route's fields are wave-uniform)
  const int slot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) % CP;
  const int r = __builtin_amdgcn_readfirstlane((int)((m.route >> (8 * slot)) & 255u));
  const int lp = __builtin_amdgcn_readfirstlane((int)((m.lpair >> (8 * slot)) & 255u));
  conv_ws_body<3, 2, PB, CP, false, false, 0, true, true>(m.p[r], (int)blockIdx.x, 0, lp);
  if (m.side.out) s2x_side(m.p[0], m.side, (int)blockIdx.x);
}

// Weight-stationary split-fp16 conv (conv_ws_h2_kernel): tile choice + dispatch.  Returns 1 when the
// shape does not qualify (the caller falls back to conv_mfma_kernel<H2>).
template <int KS, int STRIDE, int PB, int CP, bool NCHW>
static int describe_ws_one(const ConvParams& p, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&conv_ws_h2_kernel<KS, STRIDE, PB, CP, NCHW>);
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
template <int KS, int STRIDE, bool NCHW>
static int describe_ws_pb(const ConvParams& p, int pb, int cp, size_t lds, Launch* out) {
#define UDP_WS(B, C) \
  if (pb == B && cp == C) return describe_ws_one<KS, STRIDE, B, C, NCHW>(p, lds, out);
  UDP_WS(2, 1) UDP_WS(3, 1) UDP_WS(4, 1) UDP_WS(6, 1) UDP_WS(2, 2) UDP_WS(3, 2) UDP_WS(4, 2) UDP_WS(6, 2)
  UDP_WS(2, 4) UDP_WS(3, 4) UDP_WS(4, 4) UDP_WS(6, 4)
#undef UDP_WS
  return 1;
}
static int describe_ws_pb8(const ConvParams& p, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&conv_ws_pb8_kernel);
  if (!attr_set) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  out->fn = kern;
  out->grid = dim3(p.ntiles, p.CoutPad / 32);
  out->block = dim3(256);
  out->lds = (unsigned)lds;
  out->p = p;
  return UDP_OK;
}
template <int PB, int CP, int ACT>
static int describe_ws_hs_one(const ConvParams& p, size_t lds, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&conv_ws_hs_kernel<PB, CP, ACT>);
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
static int describe_ws_hs(const ConvParams& p, int pb, int cp, size_t lds, Launch* out) {
#define UDP_WS(B, C) \
  if (pb == B && cp == C) return p.relu == UDP_ACT_SILU ? describe_ws_hs_one<B, C, UDP_ACT_SILU>(p, lds, out) : describe_ws_hs_one<B, C, UDP_ACT_HSWISH>(p, lds, out);
  UDP_WS(2, 1) UDP_WS(3, 1) UDP_WS(4, 1) UDP_WS(6, 1) UDP_WS(2, 2) UDP_WS(3, 2) UDP_WS(4, 2) UDP_WS(6, 2)
  UDP_WS(2, 4) UDP_WS(3, 4) UDP_WS(4, 4) UDP_WS(6, 4)
#undef UDP_WS
  return 1;
}
// Tile of a (cout pairs per workgroup, pixel blocks per wave) candidate; false if it cannot be built.
static bool ws_tile(const ConvParams& p, int ks, int stride, int cp, int pb, WsTile* t, bool own_launch) {
  const int pg = 4 / cp;
  const int maxM = 16 * pb * pg;
  // column split: the full width, or 2..4 equal column tiles -- whichever fills the wave's pixel blocks best
  // (a 72-column map tiles exactly as 3 x 24 columns x 4 rows = 6 blocks, but only as 9 of 12 block slots at 36)
  bool have = false;
  double best_util = 0.0;
  for (int split = 1; split <= 4 || !have; ++split) {
    if (split > 8) break;
    const int TW = ceil_div(p.Wout, split);
    if (TW > 64 || TW > maxM || (have && TW < 8)) continue;
    int maxR = maxM / TW;
    if (maxR > p.Hout) maxR = p.Hout;
    int R = largest_divisor_leq(p.Hout, maxR);
    if (R * 2 <= maxR) R = maxR;
    int G = 1;
    if (R == p.Hout && TW == p.Wout) {
      G = maxM / (R * TW);
      if (G > p.N) G = p.N;
      if (G < 1) G = 1;
    }
    auto npix = [&](int g, int r) { return g * ((r - 1) * stride + ks) * ((TW - 1) * stride + ks); };
    while (npix(G, R) > MAXG * 64 && G > 1) --G;
    while (npix(G, R) > MAXG * 64 && R > 1) R = (R + 1) / 2;
    if (npix(G, R) > MAXG * 64) continue;
    int nstage = ceil_div(p.Cin, 32) > 1 ? 2 : 1;                               // stage buffers x (hi, lo) images
    size_t lds = (size_t)((npix(G, R) + 15) / 16) * 16 * ROWB * 2 * nstage;
    // a second workgroup per CU is worth more than the second stage buffer (conv_ws_body, `refill`; the kernels of convs
    // launched on their own have it: stride 2, and 3x3 stride 1 outside a launch group).  UDP_POSE_WS_SBUF: 0 off, 2 stride 2 only
    static const int sbuf_mode = getenv("UDP_POSE_WS_SBUF") == nullptr ? 1 : atoi(getenv("UDP_POSE_WS_SBUF"));
    const bool sbuf_kernel = stride == 2 || (ks == 3 && own_launch && sbuf_mode != 2);
    const bool sbuf = sbuf_kernel && nstage == 2 && lds > 80 * 1024 && lds / 2 <= 80 * 1024 && sbuf_mode != 0;
    if (sbuf) {
      nstage = 1;
      lds /= 2;
    }
    if (lds > 160 * 1024) continue;
    // the 8-block arm of the merged launch (describe_conv_ws offers it to one-pair members): only a tile that fills all 8
    // blocks of every wave, tiles the map exactly, and leaves LDS for a second workgroup on the CU.  64x48: 3 column
    // tiles of 16 x 32 rows -- halo 18 x 34 = 612 rows (39 of the 40 staging groups), 79,872 bytes
    if (pb == 8 && (G * R * TW != maxM || p.Hout % R || TW * split != p.Wout || lds > 80 * 1024)) continue;
    // pixel blocks per wave the tile really needs (the halo limit may have shrunk it): the smallest instantiated
    // count that covers them, so no wave idles under masked blocks
    const int need = ceil_div(ceil_div(G * R * TW, 16), pg);
    if (need > pb) continue;
    const int pbe = need <= 2 ? 2 : need <= 3 ? 3 : need <= 4 ? 4 : need <= 6 ? 6 : 8;
    const int tiles = ceil_div(p.N, G) * ceil_div(p.Hout, R) * ceil_div(p.Wout, TW);
    // score = useful pixels / pixel slots over the whole layer (ragged last tiles and masked blocks are waste)
    //         x the share of the staged halo tile that is not halo (narrow tiles stage more of it)
    const double util = (double)p.N * p.Hout * p.Wout / ((double)tiles * 16 * pbe * pg) *
                        ((double)G * R * TW * stride * stride / (double)npix(G, R));
    if (!have || util > best_util + 0.05) {
      have = true;
      best_util = util;
      t->cp = cp;
      t->pb = pbe;
      t->G = G;
      t->R = R;
      t->TW = TW;
      t->lds = lds;
      t->sbuf = sbuf ? 1 : 0;
      t->wgs = tiles * (p.CoutPad / (cp * 32));
    }
  }
  return have;
}

static long g_ws_fill_wgs = 512;
void ws_set_fill_wgs(long wgs) { g_ws_fill_wgs = wgs; }

// Tile choice of describe_conv_ws: fills the tile fields of `p` and `best` (cout pairs per workgroup, pixel blocks per
// wave, LDS bytes, workgroups).  Host arithmetic only -- no HIP call -- so that udp_debug_conv_tile (conv.hip) can
// report the decision without a GPU.
int choose_conv_ws(ConvParams& p, int ks, int stride, bool grouped, WsTile* best_out) {
  if (p.relu >= UDP_ACT_HSWISH && (ks != 1 || stride != 1 || p.out_nchw_f32 || p.res || p.nup || p.nout2 || grouped))
    return fail(UDP_ERR_UNSUPPORTED, "hard-swish / SiLU (activation codes 2, 4): plain 1x1 stride-1 NHWC convs on their own launch only");
  if ((stride != 1 && stride != 2) || (ks != 3 && ks != 1) || (p.out_nchw_f32 && stride != 1))
    return fail(UDP_ERR_UNSUPPORTED, "fragment-major weights (wfmt 1): conv ks=%d stride=%d nchw_out=%d has no weight-stationary kernel",
                ks, stride, p.out_nchw_f32);
  auto knob = [](const char* name, long dflt) {
    const char* v = getenv(name);
    return v ? atol(v) : dflt;
  };
  const int pairs = p.CoutPad / 32;
  const int force_cp = (int)knob("UDP_POSE_WS_CP", 0), force_pb = (int)knob("UDP_POSE_WS_PB", 0);
  // two workgroups on each of the 256 CUs; a member of a merged launch fills the chip with its siblings, and a conv of
  // a sub-batch lane (hrnet.hip: the other lane's kernels run beside it) is better off with the fatter tile from a
  // quarter of that on: W32 7.81 -> 7.98 k images/s at 128 (64: 7.88, 192: 7.83, same box)
  const long min_wgs = grouped ? 0 : knob("UDP_POSE_WS_MINWGS", g_ws_fill_wgs);
  // candidates from the fattest wave tile down: the first one that fills the chip wins, else the one with
  // the most workgroups
  // 8 blocks: one-pair 3x3 members of a merged launch only (ws_tile has the tile's conditions; two- and four-pair
  // members would need 2 x 44 KB of stage buffers and keep 6).  UDP_POSE_WS_PB8=0: the chooser without this candidate
  const bool offer8 = kWsHave8 && grouped && ks == 3 && stride == 1 && pairs % 2 == 1 && !p.out_nchw_f32 && !p.nout2 && !p.nup &&
                      knob("UDP_POSE_WS_PB8", 1) != 0;
  WsTile best{}, t{};
  bool have = false;
  for (int pb : {8, 6, 4, 3, 2}) {
    for (int cp : {4, 2, 1}) {
      if (pb == 8 && (!offer8 || cp != 1)) continue;
      if (pairs % cp || (force_cp && cp != force_cp) || (force_pb && pb != force_pb)) continue;
      if (grouped && stride == 1 && UDP_WS_MPB != 6 && pb != UDP_WS_MPB) continue;   // (diagnostic builds of the merged kernel)
      if (!ws_tile(p, ks, stride, cp, pb, &t, !grouped && !p.out_nchw_f32)) continue;   // (the NCHW-output kernels keep two stage buffers)
      const bool fills = t.wgs >= min_wgs, best_fills = have && best.wgs >= min_wgs;
      if (!have || (!best_fills && (fills || t.wgs > best.wgs))) {
        best = t;
        have = true;
      }
    }
  }
  if (!have) return fail(UDP_ERR_UNSUPPORTED, "weight-stationary conv: no tile for %dx%d C%d->%d", p.Hout, p.Wout, p.Cin, p.Cout);
  p.G = best.G;
  p.R = best.R;
  p.TW = best.TW;
  p.sbuf = best.sbuf;
  p.IH = (p.R - 1) * stride + ks;
  p.IW = (p.TW - 1) * stride + ks;
  p.tiles_x = ceil_div(p.Wout, p.TW);
  p.tiles_y = ceil_div(p.Hout, p.R);
  auto magic = [](int d) { return (unsigned)(((1u << 20) + (unsigned)d - 1) / (unsigned)d); };
  p.mIW = magic(p.IW);
  p.mIH = magic(p.IH);
  p.mRT = magic(p.R * p.TW);
  p.mTW = magic(p.TW);
  p.ntiles = ceil_div(p.N, p.G) * p.tiles_y * p.tiles_x;
  if (getenv("UDP_POSE_DEBUG_TILES"))
    fprintf(stderr, "ws conv k%d s%d %dx%d C%d->%d: G=%d R=%d TW=%d CP=%d PB=%d lds=%zu%s wgs=%d\n", ks, stride, p.Hout, p.Wout, p.Cin,
            p.Cout, p.G, p.R, p.TW, best.cp, best.pb, best.lds, best.sbuf ? " (one stage buffer)" : "", best.wgs);
  *best_out = best;
  return UDP_OK;
}

int describe_conv_ws(ConvParams p, int ks, int stride, Launch* out, bool grouped) {
  WsTile best{};
  if (const int crc = choose_conv_ws(p, ks, stride, grouped, &best)) return crc;
  int rc = 1;
  if (best.pb == 8) {
    rc = describe_ws_pb8(p, best.lds, out);
  } else
  if (ks == 3 && stride == 1 && !p.out_nchw_f32) rc = describe_ws_pb<3, 1, false>(p, best.pb, best.cp, best.lds, out);
  if (ks == 3 && stride == 1 && p.out_nchw_f32) rc = describe_ws_pb<3, 1, true>(p, best.pb, best.cp, best.lds, out);   // the net's NCHW fp32 output (RSN head)
  if (ks == 3 && stride == 2) rc = describe_ws_pb<3, 2, false>(p, best.pb, best.cp, best.lds, out);
  if (ks == 1 && stride == 1 && !p.out_nchw_f32)
    rc = p.relu >= UDP_ACT_HSWISH ? describe_ws_hs(p, best.pb, best.cp, best.lds, out) : describe_ws_pb<1, 1, false>(p, best.pb, best.cp, best.lds, out);
  if (ks == 1 && stride == 1 && p.out_nchw_f32) rc = describe_ws_pb<1, 1, true>(p, best.pb, best.cp, best.lds, out);   // (HRNet final_layer)
  if (ks == 1 && stride == 2) rc = describe_ws_pb<1, 2, false>(p, best.pb, best.cp, best.lds, out);
  if (rc == 1) return fail(UDP_ERR_UNSUPPORTED, "weight-stationary conv: no kernel for PB=%d CP=%d", best.pb, best.cp);
  if (rc == UDP_OK && p.nout2 && !(ks == 3 && stride == 1))
    return fail(UDP_ERR_UNSUPPORTED, "second outputs: 3x3 stride-1 convs only");
  if (rc == UDP_OK && grouped && (best.pb == UDP_WS_MPB || best.pb == 8) && stride == 1 && !p.nout2) {
    // storage/kernel family 3 = split fp16 weight-stationary; last digit: the member's pixel blocks per wave (6 and 8 share a launch)
    out->groupable = 300 + ks * 10 + (best.pb == 8 ? 8 : 6);
    out->ws_cp = best.cp;
  }
  return rc;
}

template <int PB, int CP>
static int describe_s2x_one(size_t lds, int ntiles, Launch* out) {
  static bool attr_set = false;
  const void* kern = reinterpret_cast<const void*>(&conv_ws_s2x_kernel<PB, CP>);
  if (!attr_set) {
    UDP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  out->fn = kern;
  out->grid = dim3(ntiles);
  out->block = dim3(256);
  out->lds = (unsigned)lds;
  return UDP_OK;
}

// Tile of the shared-input launch: every cout pair of every route under one workgroup (cp slots), the fattest wave tile
// that still fills the chip (choose_conv_ws's rule), within the 80 KB that leave room for a second workgroup on the CU.
// Host arithmetic only.  false: no such tile.
static bool choose_share_tile(const ConvParams& c0, int cp, WsTile* best) {
  ConvParams q = c0;
  q.Cout = q.CoutPad = cp * 32;
  const char* v = getenv("UDP_POSE_WS_MINWGS");
  const long min_wgs = v ? atol(v) : g_ws_fill_wgs;
  WsTile t{};
  bool have = false;
  for (int pb : {6, 4, 3, 2}) {
    if (!ws_tile(q, 3, 2, cp, pb, &t, false) || t.lds > 80 * 1024 || t.sbuf) continue;
    const bool fills = t.wgs >= min_wgs, best_fills = have && best->wgs >= min_wgs;
    if (!have || (!best_fills && (fills || t.wgs > best->wgs))) {
      *best = t;
      have = true;
    }
  }
  return have;
}

// convs[0..n): UDP_OP_CONVs as describe_all resolved them (3x3 stride 2, Cin = 32, the same input view); `fuse`: the
// UDP_OP_FUSE over that view, or null.  Returns 1 when there is no kernel for the set (the caller keeps its launches).
int describe_x0_share(const ConvParams* convs, int n, const ConvParams* fuse, const char* tag, Launch* out) {
  if (n < 1 || n > kShareRoutes) return 1;
  const ConvParams& c0 = convs[0];
  int pairs = 0;
  for (int j = 0; j < n; ++j) {
    const ConvParams& c = convs[j];
    if (c.Cin != 32 || c.wfmt != 1 || c.out_nchw_f32 || c.nout2 || c.in_stuff2 || c.bn_ws || c.relu > UDP_ACT_RELU || !c.out || c.in != c0.in ||
        c.in_pitch != c0.in_pitch || c.in_coff != c0.in_coff || c.N != c0.N || c.Hin != c0.Hin || c.Win != c0.Win || c.Hout != c0.Hout ||
        c.Wout != c0.Wout || c.CoutPad % 32 || c.CoutPad / 32 > 4)
      return 1;
    pairs += c.CoutPad / 32;
  }
  if (pairs > 4 || n + (fuse ? 1 : 0) < 2) return 1;
  if (fuse && (fuse->in != c0.in || fuse->in_pitch != c0.in_pitch || fuse->in_coff != c0.in_coff || fuse->Cout != 32 || fuse->N != c0.N ||
               fuse->Hout != c0.Hin || fuse->Wout != c0.Win || fuse->res || !fuse->out || fuse->relu > UDP_ACT_RELU || fuse->out_pitch % 8 ||
               fuse->out_coff % 8 || (size_t)fuse->N * fuse->Hout * fuse->Wout * fuse->out_pitch * 4 >= 0x7FFF0000u))
    return 1;
  const int cp = pairs <= 2 ? 2 : 4;
  WsTile best{};
  if (!choose_share_tile(c0, cp, &best)) return 1;
  auto m = std::make_shared<ConvShare>();
  memset(m.get(), 0, sizeof(ConvShare));
  auto magic = [](int d) { return (unsigned)(((1u << 20) + (unsigned)d - 1) / (unsigned)d); };
  int ntiles = 0;
  for (int j = 0; j < n; ++j) {
    ConvParams& p = m->p[j];
    p = convs[j];
    p.G = best.G;
    p.R = best.R;
    p.TW = best.TW;
    p.sbuf = 0;
    p.IH = (p.R - 1) * 2 + 3;
    p.IW = (p.TW - 1) * 2 + 3;
    p.tiles_x = ceil_div(p.Wout, p.TW);
    p.tiles_y = ceil_div(p.Hout, p.R);
    p.mIW = magic(p.IW);
    p.mIH = magic(p.IH);
    p.mRT = magic(p.R * p.TW);
    p.mTW = magic(p.TW);
    p.ntiles = ntiles = ceil_div(p.N, p.G) * p.tiles_y * p.tiles_x;
  }
  for (int j = n; j < kShareRoutes; ++j) m->p[j] = m->p[0];
  // slot -> (route, pair in the route); a slot without a route: route 0, pair 255 -- past the weight and bias descriptors at
  // every tap (<= 4 pairs x 9 taps x 4 KiB), so the wave multiplies zeros and its range check sees zeros
  int slot = 0;
  for (int j = 0; j < n; ++j)
    for (int lp = 0; lp < convs[j].CoutPad / 32; ++lp, ++slot) {
      m->route |= (unsigned)j << (8 * slot);
      m->lpair |= (unsigned)lp << (8 * slot);
    }
  for (; slot < cp; ++slot) m->lpair |= 255u << (8 * slot);
  if (fuse) {
    m->side = *fuse;
    m->side.mRT = magic(4 * best.R * best.TW);
    m->side.mTW = magic(2 * best.TW);
  }
  int rc = 1;
#define UDP_S2X(B, C) \
  if (best.pb == B && cp == C) rc = describe_s2x_one<B, C>(best.lds, ntiles, out);
  UDP_S2X(2, 2) UDP_S2X(3, 2) UDP_S2X(4, 2) UDP_S2X(6, 2) UDP_S2X(2, 4) UDP_S2X(3, 4) UDP_S2X(4, 4) UDP_S2X(6, 4)
#undef UDP_S2X
  if (rc) return rc;
  out->groupable = 0;
  out->ws_cp = 0;
  out->pair = 0;
  out->p = m->p[0];
  out->share = m;
  if (getenv("UDP_POSE_DEBUG_TILES")) {
    char routes[64] = "";
    for (int j = 0; j < n; ++j) snprintf(routes + strlen(routes), sizeof(routes) - strlen(routes), "%s%d", j ? "," : "", convs[j].Cout);
    fprintf(stderr, "x0 share %dx%d C32: %s pairs=%d routes=[%s] fuse0=%d G=%d R=%d TW=%d CP=%d PB=%d lds=%zu wgs=%d\n", c0.Hin, c0.Win, tag ? tag : "",
            pairs, routes, fuse ? 1 : 0, best.G, best.R, best.TW, cp, best.pb, best.lds, ntiles);
  }
  return UDP_OK;
}

// Dispatch order of a merged weight-stationary launch.  Members arrive deepest-K first: long, matrix-bound
// workgroups (a 256-channel workgroup lives ~65 us, 72 K steps) down to the short HBM-bound 32-channel ones
// (~15 us).  Workgroups are dispatched in flat-index order, breadth first over the CUs.  Member after member
// (longest first) leaves the second half of the launch to the shallow member alone -- HBM-bound at ~4.9 TB/s while
// the matrix pipe idles, after a first half in which HBM idles (in-kernel timeline, tools/stamp_multi.py).  So the
// grid alternates chunks of the deep members (list A, longest first) with chunks of the shallowest member (list
// B), in about the proportion that exhausts both lists together: every CU holds both kinds for the whole launch, the
// deepest workgroups still all start in the first round, and the last workgroups to start are short ones.
// Chunks are multiples of 8 workgroups (one per XCD -- workgroup i runs on XCD i % 8, an uneven pattern would
// leave some XCDs with all the long workgroups).  UDP_POSE_WS_ORDER=lpt keeps the plain member-after-member order.
static void ws_order(ConvMulti* m, int n) {
  struct Seg {
    unsigned start, first, cnt;
    int mem;
  };
  unsigned cnt_of[4];
  unsigned total = 0;
  for (int j = 0; j < n; ++j) {
    cnt_of[j] = (j + 1 < n ? m->start[j + 1] : m->start[4]) - m->start[j];
    total += cnt_of[j];
  }
  const char* mode = getenv("UDP_POSE_WS_ORDER");
  const bool lpt = mode && strcmp(mode, "lpt") == 0;
  // list A runs 25 % ahead of its share, so the deep members are exhausted first and the launch ends on the short
  // workgroups of B alone (tail = one 15 us workgroup instead of a 20-25 us one): +2 % (UDP_POSE_WS_BIAS, percent)
  const unsigned bias = getenv("UDP_POSE_WS_BIAS") ? (unsigned)atoi(getenv("UDP_POSE_WS_BIAS")) : 125u;
  auto build = [&](unsigned g) {
    std::vector<Seg> segs;
    unsigned lo[4] = {0, 0, 0, 0};
    unsigned at = 0;
    auto take = [&](int j, unsigned cnt) {
      if (cnt > cnt_of[j] - lo[j]) cnt = cnt_of[j] - lo[j];
      if (!cnt) return;
      if (!segs.empty() && segs.back().mem == j && segs.back().first + segs.back().cnt == lo[j])
        segs.back().cnt += cnt;
      else
        segs.push_back({at, lo[j], cnt, j});
      lo[j] += cnt;
      at += cnt;
    };
    if (!lpt) {
      const unsigned nb = cnt_of[n - 1];
      const unsigned na = total - nb;
      unsigned ta = 0, tb = 0;                 // taken from A / B so far
      while (ta < na && tb < nb) {
        // the list that is behind its share goes next (ties: A, so that the deepest workgroups lead the grid)
        if ((unsigned long long)ta * nb * 100ull <= (unsigned long long)tb * na * bias) {
          int j = 0;
          while (lo[j] == cnt_of[j]) ++j;
          const unsigned c = cnt_of[j] - lo[j] < g ? cnt_of[j] - lo[j] : g;
          take(j, c);
          ta += c;
        } else {
          const unsigned c = nb - tb < g ? nb - tb : g;
          take(n - 1, c);
          tb += c;
        }
      }
    }
    for (int j = 0; j < n; ++j) take(j, cnt_of[j] - lo[j]);
    return segs;
  };
  // chunk size: 32 workgroups (UDP_POSE_WS_G); the per-8 lookup table (ConvMulti::tab) takes any number of chunks,
  // the segment table searched without it holds kMultiSegs
  unsigned g = getenv("UDP_POSE_WS_G") ? (unsigned)atoi(getenv("UDP_POSE_WS_G")) : 32u;
  if (g < 8 || g % 8) g = 32;
  std::vector<Seg> segs = build(g);
  m->tab_n = 0;
  bool ok = total % 8 == 0 && total / 8 <= (unsigned)kMultiTab && getenv("UDP_POSE_WS_NOTAB") == nullptr;
  for (int j = 0; j < n && ok; ++j)
    ok = m->tiles[j] % 8 == 0 && m->ncby[j] <= 64 && m->tiles[j] < (1u << 22) && (m->code[j] == 1 || m->code[j] == 2 || m->code[j] == 4 || m->code[j] == kWsCode8);
  for (size_t k = 0; k < segs.size() && ok; ++k) ok = segs[k].start % 8 == 0 && segs[k].first % 8 == 0;
  if (ok) {
    for (const Seg& sg : segs) {
      const int j = sg.mem;
      for (unsigned b = sg.start; b < sg.start + sg.cnt; b += 8) {
        int tile, cby;
        ws_decode(b - sg.start + sg.first, m->tiles[j], m->ncby[j], tile, cby);
        const unsigned cl = m->code[j] == 1 ? 0u : m->code[j] == 2 ? 1u : m->code[j] == 4 ? 2u : 3u;      // log2 of the member's code (CP; 3: the 8-block arm)
        m->tab[b >> 3] = (unsigned)j | (cl << 2) | ((unsigned)cby << 4) | ((unsigned)tile << 10);
      }
    }
    m->tab_n = total / 8;
  }
  // the searched table (read by the kernel only when there is no lookup table): coarser chunks until it fits
  while (segs.size() > (size_t)kMultiSegs) {
    g += 8;
    segs = build(g);
  }
  for (int k = 0; k < kMultiSegs; ++k) {
    const bool have = (size_t)k < segs.size();
    m->seg_start[k] = have ? segs[k].start : 0xFFFFFFFFu;
    m->seg_first[k] = have ? segs[k].first : 0;
    m->seg_mem[k] = have ? segs[k].mem : 0;
  }
}

// Diagnostic (tests/test_host_cpu.py, no GPU needed): the dispatch tables ws_order builds for members of
// tiles[j] x ncby[j] workgroups, resolved for every flat block exactly as conv_ws_multi resolves them (table entry
// when there is one, segment search otherwise).  out_*[b] for b < total; returns total, or -1.
extern "C" int udp_debug_multi_order(const unsigned* tiles, const unsigned* ncby, const int* code, int n, unsigned cap,
                                     unsigned* out_member, unsigned* out_tile, unsigned* out_cby, int* used_table) {
  if (!tiles || !ncby || !code || n < 1 || n > 4 || !out_member || !out_tile || !out_cby) return -1;
  static ConvMulti m;
  memset(&m, 0, sizeof(m));
  unsigned total = 0;
  for (int j = 0; j < n; ++j) {
    m.start[j] = total;
    m.tiles[j] = tiles[j];
    m.ncby[j] = ncby[j];
    m.code[j] = code[j];
    total += tiles[j] * ncby[j];
  }
  for (int j = n; j < 5; ++j) m.start[j] = j < 4 ? 0xFFFFFFFFu : total;
  m.start[4] = total;
  for (int j = n; j < 4; ++j) m.tiles[j] = m.ncby[j] = 1;
  if (total > cap) return -1;
  ws_order(&m, n);
  if (used_table) *used_table = m.tab_n != 0;
  for (unsigned b = 0; b < total; ++b) {
    int j, tile, cby;
    if (m.tab_n) {
      const unsigned e = m.tab[b >> 3];
      j = (int)(e & 3u);
      if ((1 << ((e >> 2) & 3u)) != m.code[j]) return -1;
      cby = (int)((e >> 4) & 63u);
      tile = (int)((e >> 10) + (b & 7u));
    } else {
      int sg = 0;
      for (int k = 1; k < kMultiSegs; ++k) sg += b >= m.seg_start[k];
      j = m.seg_mem[sg];
      ws_decode(b - m.seg_start[sg] + m.seg_first[sg], m.tiles[j], m.ncby[j], tile, cby);
    }
    out_member[b] = (unsigned)j;
    out_tile[b] = (unsigned)tile;
    out_cby[b] = (unsigned)cby;
  }
  return (int)total;
}

// Kernel + attribute for a merged launch of `n` weight-stationary members; fills the kernel argument.
int describe_ws_multi(const Launch* members, int n, ConvMulti* m, Launch* out) {
  static bool ws_attr_set = false;
  const void* wk[2] = {reinterpret_cast<const void*>(&conv_ws_multi<3>), reinterpret_cast<const void*>(&conv_ws_multi<1>)};
  if (!ws_attr_set) {
    for (const void* k : wk) UDP_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ws_attr_set = true;
  }
  memset(m, 0, sizeof(*m));
  unsigned total = 0, lds = 0;
  for (int j = 0; j < n; ++j) {
    if (members[j].groupable / 10 != members[0].groupable / 10) return fail(UDP_ERR_ARG, "describe_multi: mixed weight-stationary members");
    m->p[j] = members[j].p;
    m->start[j] = total;
    m->tiles[j] = members[j].grid.x;
    m->ncby[j] = members[j].grid.y;
    m->code[j] = members[j].groupable % 10 == 8 ? kWsCode8 : members[j].ws_cp;
    total += members[j].grid.x * members[j].grid.y;
    if (members[j].lds > lds) lds = members[j].lds;
  }
  for (int j = n; j < 5; ++j) m->start[j] = j < 4 ? 0xFFFFFFFFu : total;
  for (int j = n; j < 4; ++j) m->tiles[j] = m->ncby[j] = 1;
  ws_order(m, n);
  if (getenv("UDP_POSE_DEBUG_TILES")) {
    char codes[64] = "";
    for (int j = 0; j < n; ++j) snprintf(codes + strlen(codes), sizeof(codes) - strlen(codes), "%s%d", j ? "," : "", m->code[j]);
    fprintf(stderr, "ws multi k%d: members=%d wgs=%u codes=[%s] dispatch=%s\n", members[0].groupable / 10 % 10, n, total, codes,
            m->tab_n ? "table" : "search");
  }
  out->fn = wk[members[0].groupable / 10 % 10 == 3 ? 0 : 1];
  out->grid = dim3(total);
  out->block = dim3(256);
  out->lds = lds;
  out->groupable = 0;
  return UDP_OK;
}

#ifdef UDP_STAMPS
int ws_set_stamps(unsigned long long* dev_buf) {
  UDP_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &dev_buf, sizeof(dev_buf)));
  return UDP_OK;
}
// the weight-stationary kernels' stamps alone (libudp_pose_hip_stamps_ws.so links the product conv.o)
extern "C" int udp_debug_set_stamps_ws(unsigned long long* dev_buf) { return ws_set_stamps(dev_buf); }
#endif

// ---------------------------------------------------------------------------------------------------------------
// Two 1x1 convs chained through registers (udp_conv_op.chain_cout; the layer1 Bottlenecks, pose_hrnet.py:80-100: conv3
// + bn3 + shortcut + ReLU of one block, conv1 + bn1 + ReLU of the next):
//     Y = act(W . X + b [+ R])            Cin = 32 * NCH  ->  Cout = 32 * NP      (written to `out`)
//     Z = act2(W2 . Y_as_stored + b2)     Cout            ->  Cout2 = 64          (written to `chain`)
// Both run at the memory roofline on their own; chained, the 4 * planes-channel map Y is written once and not read back
// (1.41 -> 1.01 GB per pair at 128 images).  PIXEL-stationary: a wave owns 16 * PB pixels, keeps their X fragments in
// registers and walks the cout pairs of the first conv; the accumulators of pair p -- lane (kg, li) holds couts
// 32p + 8kg .. + 7 of pixel li, the fragment-major row order (udp_conv_op.wfmt) -- are, after the epilogue and the
// split into (hi, lo), exactly the B fragment of K chunk p of the second conv: no LDS, no barrier, the waves of a
// workgroup only share the weight fragments in L1 / L2.  Every accumulator sees the MFMAs of the separate convs in
// the same order (chunk by chunk: hi * Xhi, lo * Xhi, hi * 2^-11 * Xlo), so Y and Z are theirs bit for bit.
// Chain fields ride in ConvParams members the 1x1 conv does not use (no up-sampled addends here): wgt2 / bias2 = W2 /
// b2, up[0] = Z, up_shift[0..2] = Cout2, wexp2, act2.
// LDSW: the weights of both convs (and the biases) live in LDS -- 128 KiB + 1.25 KiB for Cin = 64, staged once by a
// persistent 8-wave workgroup per CU whose waves then walk the pixel groups: the vector-memory queue carries only what
// comes from / goes to HBM (with the fragments streamed from L2 they are 128 of the 224 vector-memory instructions of a
// wave, each 16 cycles of the CU's address unit, and every one of them queues behind the residual loads).
template <int NCH, int PB, int RD, bool LDSW>
__global__ __launch_bounds__(LDSW ? 512 : 256) __attribute__((amdgpu_waves_per_eu(2))) void conv_chain_kernel(const ConvParams p) {
  using T = H2;
  constexpr int ESZ = 2, NB = 2, Q = 2;          // Q: cout pairs of the second conv (Cout2 = 64)
  constexpr int NWAVES = LDSW ? 8 : 4;
  constexpr int AD = LDSW ? 2 : 3;               // fragment ring: from L2 the step after next is in flight, from LDS the next one
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kg = lane >> 4;
  const unsigned npix = (unsigned)p.N * p.Hout * p.Wout;
  constexpr int NP = 8;                          // cout pairs of the first conv (Cout = 256) = K chunks of the second.  A constant:
  // the pairs are straight-line code -- a pair under `if (k < NP)` makes hipcc drain every load at the join (vmcnt(0)), and
  // with it every prefetch across pairs
  const int cout2 = p.up_shift[0];
  const unsigned inpb = (unsigned)p.in_pitch * ESZ * 2, outpb = (unsigned)p.out_pitch * ESZ * 2, respb = (unsigned)p.res_pitch * ESZ * 2;
  const unsigned zpb = (unsigned)cout2 * ESZ * 2;
  const unsigned in_lo = (unsigned)p.in_pitch * ESZ, out_lo = (unsigned)p.out_pitch * ESZ, res_lo = (unsigned)p.res_pitch * ESZ;
  const unsigned z_lo = (unsigned)cout2 * ESZ;
  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, (p.sbuf & 8) ? 0 : npix * inpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt), 0, (p.sbuf & 1) ? 0 : (unsigned)NCH * NP * 4096u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt2), 0, (p.sbuf & 1) ? 0 : (unsigned)NP * Q * 4096u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_bias = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, (unsigned)p.CoutPad * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_bias2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias2), 0, (unsigned)cout2 * 4u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_res = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.res), 0, (p.res && !(p.sbuf & 4)) ? npix * respb : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (p.sbuf & 2) ? 0 : npix * outpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_z = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.up[0]), 0, (p.sbuf & 2) ? 0 : npix * zpb, 0x00020000);
  const float winv = __builtin_ldexpf(1.f, -p.wexp), winv2 = __builtin_ldexpf(1.f, -p.up_shift[1]);
  const unsigned wvoff = (unsigned)lane * 16u;

  constexpr unsigned kW1 = (unsigned)NCH * 8 * 4096u, kBias = kW1 + 8u * Q * 4096u;     // LDS offsets: second conv's weights, biases
  if constexpr (LDSW) {
    for (unsigned blk = wave; blk < kBias / 1024u; blk += NWAVES) {
      const bool first = blk * 1024u < kW1;
      blds16(first ? r_w : r_w2, (first ? blk * 1024u : blk * 1024u - kW1) + wvoff, smem + blk * 1024u);
    }
    float* sbias = reinterpret_cast<float*>(smem + kBias);
    if (threadIdx.x < 256 + 64) sbias[threadIdx.x] = threadIdx.x < 256 ? p.bias[threadIdx.x] : p.bias2[threadIdx.x - 256];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  const unsigned ngroups = (npix + PB * 16 - 1) / (PB * 16);
  for (unsigned grp = (unsigned)blockIdx.x * NWAVES + wave; grp < ngroups; grp += LDSW ? gridDim.x * NWAVES : ngroups) {
  // (per-lane constants re-derived inside the loop: hoisted out, the offsets of all eight pairs live across it -- spills)
  unsigned wv = wvoff;
  int kgl = kg;
  if constexpr (LDSW) {
    asm volatile("" : "+v"(wv));
    asm volatile("" : "+v"(kgl));
  }
  unsigned pix[PB];
  bool ok[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    pix[i] = grp * (PB * 16) + i * 16 + li;
    ok[i] = pix[i] < npix;
  }
  // X fragments of the wave's pixels: lane (kg, li) holds channels 32c + 8kg .. + 7 of pixel li (hi and lo planes)
  f16x8 xh[PB][NCH], xl[PB][NCH];
#pragma unroll
  for (int i = 0; i < PB; ++i)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const unsigned off = ok[i] ? pix[i] * inpb + (unsigned)(p.in_coff + 32 * c + 8 * kgl) * ESZ : kOobOff;
      xh[i][c] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_in, off, 0, 0));
      xl[i][c] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_in, off + in_lo, 0, 0));
    }
  // weight fragments: steps of one cout pair pr = NCH chunks of the first conv, then Q pairs of the second; the
  // fragments of the step after next stream in from L2 (ring of three, as in conv_ws_body)
  constexpr int S = NCH + Q;
  f16x8 ah[AD][NB], al[AD][NB];
  auto load_a = [&](int pr, int st, f16x8 (&h)[NB], f16x8 (&l)[NB]) __attribute__((always_inline)) {
    const bool first = st < NCH;
    const unsigned soff = first ? (unsigned)(st * NP + pr) * 4096u : (unsigned)(pr * Q + (st - NCH)) * 4096u;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (LDSW) {
        const unsigned char* q = smem + (first ? 0u : kW1) + soff + wv + 2048u * nb;
        h[nb] = *reinterpret_cast<const f16x8*>(q);
        l[nb] = *reinterpret_cast<const f16x8*>(q + 1024);
      } else {
        h[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(first ? r_w : r_w2, wv + 2048u * nb, soff, 0));
        l[nb] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(first ? r_w : r_w2, wv + 2048u * nb + 1024u, soff, 0));
      }
    }
  };
  // residual of the pair RD - 1 ahead in flight (vector-memory operations complete in issue order: the weight fragments
  // requested behind a residual load arrive with it, so the distance also bounds how long a fragment can be held up)
  ResH2<NB> rres[RD][PB];
  auto load_res = [&](int pr, ResH2<NB> (&r)[PB]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < PB; ++i)
      load_res_h2(r[i], r_res, ok[i] ? pix[i] * respb + (unsigned)(p.res_coff + 32 * pr + 8 * kgl) * ESZ : kOobOff, res_lo);
  };
#pragma unroll
  for (int k = 0; k < RD - 1; ++k) load_res(k, rres[k]);
  load_a(0, 0, ah[0], al[0]);
  if constexpr (AD > 2) load_a(0, 1, ah[1], al[1]);

  f32x4 acc2[PB][Q][NB];
#pragma unroll
  for (int i = 0; i < PB; ++i)
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc2[i][q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto mfma3 = [&](f32x4 (&acc)[NB], const f16x8 (&h)[NB], const f16x8 (&l)[NB], const f16x8 (&a2)[NB], const f16x8 bh, const f16x8 bl)
      __attribute__((always_inline)) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h[nb], bh, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l[nb], bh, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[nb], bl, acc[nb], 0, 0, 0);
      };

  // one cout pair of the first conv = one K chunk of the second; BUF0 = ring slot of its first step (S steps per pair)
  auto pair_body = [&](auto KC) __attribute__((always_inline)) {
    constexpr int pr = decltype(KC)::value, BUF0 = (pr * S) % AD, SIDE = pr % RD;
    if constexpr (pr + RD - 1 < NP) load_res(pr + RD - 1, rres[(SIDE + RD - 1) % RD]);
    f32x4 bias[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (LDSW)
        bias[nb] = *reinterpret_cast<const f32x4*>(smem + kBias + (unsigned)(32 * pr + 8 * kgl + 4 * nb) * 4u);
      else
        bias[nb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_bias, (unsigned)(32 * pr + 8 * kgl + 4 * nb) * 4u, 0, 0));
    }
    f32x4 acc[PB][NB];
#pragma unroll
    for (int i = 0; i < PB; ++i)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[i][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 yh[PB], yl[PB];
#pragma unroll
    for (int st = 0; st < S; ++st) {
      constexpr int dummy = 0;
      (void)dummy;
      const int buf = (BUF0 + st) % AD;
      {   // fragments of the step AD - 1 ahead (unconditional: past the end the last step's again)
        int npr = pr, nst = st + AD - 1;
        if (nst >= S) {
          nst -= S;
          npr = pr + 1 < NP ? pr + 1 : pr;
          if (pr + 1 >= NP) nst = S - 1;
        }
        load_a(npr, nst, ah[(buf + AD - 1) % AD], al[(buf + AD - 1) % AD]);
      }
      f16x8 a2[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a2[nb] = ah[buf][nb] * (_Float16)0x1p-11f;
      if (st < NCH) {
#pragma unroll
        for (int i = 0; i < PB; ++i) mfma3(acc[i], ah[buf], al[buf], a2, xh[i][st], xl[i][st]);
        if (st == NCH - 1) {
          // epilogue of the first conv for this pair: conv_ws_body's, value by value
          const int cbase = 32 * pr + 8 * kgl;
#pragma unroll
          for (int i = 0; i < PB; ++i) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[i][nb][q] = __builtin_fmaf(acc[i][nb][q], winv, bias[nb][q]);
            add_res_h2(acc[i], rres[SIDE][i]);
            if (p.relu) {
#pragma unroll
              for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][nb][q] = acc[i][nb][q] > 0.f ? acc[i][nb][q] : 0.f;
            }
            h2_split8(acc[i][0], acc[i][1], yh[i], yl[i]);
            const unsigned ooff = ok[i] ? pix[i] * outpb + (unsigned)(p.out_coff + cbase) * ESZ : kOobOff;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, yh[i]), r_out, ooff, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, yl[i]), r_out, ooff + out_lo, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < PB; ++i) mfma3(acc2[i][st - NCH], ah[buf], al[buf], a2, yh[i], yl[i]);
      }
    }
  };
  // S steps per pair over a ring of three: the ring slot of a pair's first step cycles with period 3 / gcd(S, 3)
  pair_body(std::integral_constant<int, 0>{});
  pair_body(std::integral_constant<int, 1>{});
  pair_body(std::integral_constant<int, 2>{});
  pair_body(std::integral_constant<int, 3>{});
  pair_body(std::integral_constant<int, 4>{});
  pair_body(std::integral_constant<int, 5>{});
  pair_body(std::integral_constant<int, 6>{});
  pair_body(std::integral_constant<int, 7>{});
  // epilogue of the second conv
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int cbase = 32 * q + 8 * kgl;
    f32x4 b2[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (LDSW)
        b2[nb] = *reinterpret_cast<const f32x4*>(smem + kBias + 1024u + (unsigned)(cbase + 4 * nb) * 4u);
      else
        b2[nb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_bias2, (unsigned)(cbase + 4 * nb) * 4u, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      f32x4 v[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[nb][k] = __builtin_fmaf(acc2[i][q][nb][k], winv2, b2[nb][k]);
          if (p.up_shift[2]) v[nb][k] = v[nb][k] > 0.f ? v[nb][k] : 0.f;
        }
      store_vec_buf<T, NB>(r_z, ok[i] ? pix[i] * zpb + (unsigned)cbase * ESZ : kOobOff, z_lo, v);
    }
  }
  }   // pixel groups
}

int describe_conv_chain(ConvParams p, Launch* out) {
  const int cout2 = p.up_shift[0];
  if (p.Cin % 32 || (p.Cin != 64 && p.Cin != 128) || p.CoutPad != p.Cout || p.Cout != 256 || cout2 != 64 || p.nup ||
      p.nout2 || p.out_nchw_f32 || !p.out || !p.up[0] || !p.wgt2 || !p.bias2 || p.Hin != p.Hout || p.Win != p.Wout)
    return fail(UDP_ERR_UNSUPPORTED, "chained 1x1 convs: C%d -> %d -> %d (64 | 128 -> 256 -> 64, dense NHWC outputs)", p.Cin, p.Cout, cout2);
  // A/B (UDP_POSE_CHAIN_VAR): 0 = weights in LDS where they fit (Cin = 64), 1 = streamed from L2 everywhere
  static const int var = getenv("UDP_POSE_CHAIN_VAR") ? atoi(getenv("UDP_POSE_CHAIN_VAR")) : 0;
  constexpr int PB = 2;
  const long npix = (long)p.N * p.Hout * p.Wout;
  if (npix * (long)std::max(std::max(p.in_pitch, p.out_pitch), p.res_pitch) * 4 >= (1L << 31))
    return fail(UDP_ERR_UNSUPPORTED, "chained 1x1 convs: tensor beyond the 2 GiB buffer-descriptor range");
  const long groups = (npix + PB * 16 - 1) / (PB * 16);
  out->lds = 0;
  if (p.Cin == 64 && var == 0) {
    out->fn = reinterpret_cast<const void*>(&conv_chain_kernel<2, PB, 3, true>);
    out->lds = (2 * 8 + 8 * 2) * 4096 + 1280;
    out->grid = dim3((unsigned)std::min<long>(256, (groups + 7) / 8));
    out->block = dim3(512);
    UDP_HIP_CHECK(hipFuncSetAttribute(out->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)out->lds));
  } else {
    out->fn = p.Cin == 64 ? reinterpret_cast<const void*>(&conv_chain_kernel<2, PB, 3, false>) : reinterpret_cast<const void*>(&conv_chain_kernel<4, PB, 2, false>);
    out->grid = dim3((unsigned)((groups + 3) / 4));
    out->block = dim3(256);
  }
  out->groupable = 0;
  out->p = p;
  out->p.sbuf = getenv("UDP_POSE_CHAIN_DBG") ? atoi(getenv("UDP_POSE_CHAIN_DBG")) : 0;   // timing-only ablations (results WRONG): 1 no weights, 2 no stores, 4 no residual, 8 no X
  return UDP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Chained head (hrnet.hip marks the pair; the last two ops of an HRNet-W32 program: stage4's last fuse conv and
// final_layer, pose_hrnet.py:456-470):
//     Y = ReLU(W . X + b + sum_u nearest_up(up_u))    Cin = 32  ->  Cout = 128        (NOT written: nothing else reads it)
//     Z = W2 . Y_as_stored + b2                        128      ->  Cout2 <= 32 * Q    (NCHW fp32, the net's output)
// On their own the two launches write the 128-channel map to HBM and read it straight back: 546 MB for 128 images
// at 64x48, of which X, the addends and Z are 143 MB.  The technique is conv_chain_kernel's: a pixel-stationary wave
// owns 16 * PB flat pixels, keeps their X fragments (one K chunk) and walks the NP = 4 cout pairs of the first conv;
// the accumulators of pair p, after conv_ws_body's epilogue (fma(acc, 2^-wexp, bias), the addends u = 0, 1, 2, ReLU)
// and the split into (hi, lo) -- with the range check of the store that no longer happens -- are the B fragment of K
// chunk p of the second conv.  Every accumulator sees the MFMAs of the separate launches in their order (hi * Bhi,
// lo * Bhi, hi * 2^-11 * Blo, chunk by chunk), so Z is theirs bit for bit.  (The separate launch also adds the empty
// residual, + 0.0f, in front of the addends: that can only turn a -0 into a +0, which the ReLU does anyway.)
// Both weight sets (16 KiB + Q * 16 KiB) and the biases live in LDS, staged once by a persistent 8-wave workgroup
// (conv_chain_kernel's notes: streamed from L2 the fragments made it issue-bound).
// Fields of the second conv ride in ConvParams members the first one does not use: wgt2 / bias2 = W2 / b2, out2[0] = Z,
// out2_pitch[0] = Cout2, out2_coff[0] = wexp2; flip_from / out_skip place Z's image rows (a sub-batch lane's).
template <int Q>
__global__ __launch_bounds__(512) void conv_head_chain_kernel(const ConvParams p) {
  constexpr int ESZ = 2, NB = 2, PB = 2, NP = 4, NWAVES = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kg = lane >> 4;
  const unsigned hw = (unsigned)p.Hout * p.Wout;
  const unsigned npix = (unsigned)p.N * hw;
  const int cout2 = p.out2_pitch[0];
  const unsigned inpb = (unsigned)p.in_pitch * ESZ * 2, in_lo = (unsigned)p.in_pitch * ESZ;
  const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.in), 0, npix * inpb, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt), 0, (unsigned)NP * 4096u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_w2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wgt2), 0, (unsigned)NP * Q * 4096u, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_z = __builtin_amdgcn_make_buffer_rsrc(p.out2[0], 0, (unsigned)(p.N + p.out_skip) * hw * (unsigned)cout2 * 4u, 0x00020000);
  const float winv = __builtin_ldexpf(1.f, -p.wexp), winv2 = __builtin_ldexpf(1.f, -p.out2_coff[0]);
  // addends: dense [N][Hout >> s][Wout >> s][Cout] split-fp16 maps (zero-length descriptor: no such addend)
  const unsigned uppb = (unsigned)p.Cout * ESZ * 2, up_lo = (unsigned)p.Cout * ESZ;
  __amdgpu_buffer_rsrc_t r_up[3];
#pragma unroll
  for (int u = 0; u < 3; ++u)
    r_up[u] = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.up[u]), 0,
                                                u < p.nup ? (unsigned)p.N * (p.Hout >> p.up_shift[u]) * (p.Wout >> p.up_shift[u]) * uppb : 0u, 0x00020000);

  // ---- LDS: [W1: NP blocks of 4 KiB][W2: NP * Q blocks, (chunk, pair) order][b1: 128 floats][b2: 32 * Q floats]
  constexpr unsigned kW2 = (unsigned)NP * 4096u, kBias = kW2 + (unsigned)NP * Q * 4096u;
  for (unsigned off = threadIdx.x * 16u; off < kBias; off += 512u * 16u) {
    const u32x4 v = off < kW2 ? __builtin_amdgcn_raw_buffer_load_b128(r_w, off, 0, 0) : __builtin_amdgcn_raw_buffer_load_b128(r_w2, off - kW2, 0, 0);
    *reinterpret_cast<u32x4*>(smem + off) = v;
  }
  float* sbias = reinterpret_cast<float*>(smem + kBias);
  if (threadIdx.x < 128 + 32 * Q) sbias[threadIdx.x] = threadIdx.x < 128 ? p.bias[threadIdx.x] : p.bias2[threadIdx.x - 128];
  __syncthreads();
  // A fragments of the 4 KiB block at `blk`: (nb, plane) at 2048 * nb + 1024 * plane, lane l's 8 K values at 16 * l
  auto load_a = [&](unsigned blk, f16x8 (&h)[NB], f16x8 (&l)[NB]) __attribute__((always_inline)) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const unsigned char* q = smem + blk + (unsigned)lane * 16u + 2048u * nb;
      h[nb] = *reinterpret_cast<const f16x8*>(q);
      l[nb] = *reinterpret_cast<const f16x8*>(q + 1024);
    }
  };
  auto mfma3 = [&](f32x4 (&acc)[NB], const f16x8 (&h)[NB], const f16x8 (&l)[NB], const f16x8 (&a2)[NB], const f16x8 bh, const f16x8 bl)
      __attribute__((always_inline)) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h[nb], bh, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(l[nb], bh, acc[nb], 0, 0, 0);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[nb], bl, acc[nb], 0, 0, 0);
      };

  const unsigned ngroups = (npix + PB * 16 - 1) / (PB * 16);
  for (unsigned grp = (unsigned)blockIdx.x * NWAVES + wave; grp < ngroups; grp += gridDim.x * NWAVES) {
    unsigned pix[PB], upoff[PB][3];
    int pn[PB], py[PB], px[PB];
    bool ok[PB];
    f16x8 xh[PB], xl[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      pix[i] = grp * (PB * 16) + i * 16 + li;
      ok[i] = pix[i] < npix;
      const unsigned pc = ok[i] ? pix[i] : 0u;
      pn[i] = (int)(pc / hw);
      const unsigned rem = pc - (unsigned)pn[i] * hw;
      py[i] = (int)(rem / (unsigned)p.Wout);
      px[i] = (int)(rem - (unsigned)py[i] * p.Wout);
      // X fragment: lane (kg, li) holds channels 8kg .. + 7 of pixel li (hi and lo planes); masked pixels read zeros
      const unsigned off = ok[i] ? pix[i] * inpb + (unsigned)(p.in_coff + 8 * kg) * ESZ : kOobOff;
      xh[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_in, off, 0, 0));
      xl[i] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_in, off + in_lo, 0, 0));
#pragma unroll
      for (int u = 0; u < 3; ++u) {     // nearest up-sampling: pixel (n, y >> s, x >> s) of addend u
        const int sh = u < p.nup ? p.up_shift[u] : 0;
        const unsigned up_pix = (unsigned)(pn[i] * (p.Hout >> sh) + (py[i] >> sh)) * (unsigned)(p.Wout >> sh) + (unsigned)(px[i] >> sh);
        upoff[i][u] = ok[i] ? up_pix * uppb : kOobOff;
      }
    }
    f32x4 acc2[PB][Q][NB];
#pragma unroll
    for (int i = 0; i < PB; ++i)
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc2[i][q][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one cout pair of the first conv = one K chunk of the second (straight-line code, see conv_chain_kernel)
#pragma unroll
    for (int pr = 0; pr < NP; ++pr) {
      // (the pairs are kept apart: left alone hipcc hoists the addend and fragment loads of all four -- 126 spilled registers)
      __builtin_amdgcn_sched_barrier(0);
      const int cbase = 32 * pr + 8 * kg;
      // the pair's addends (8 consecutive channels of the up-sampled pixel, hi and lo), requested before its MFMAs;
      // an absent addend reads zeros through its zero-length descriptor: no branch around loads
      u32x4 uh[PB][3], ul[PB][3];
#pragma unroll
      for (int i = 0; i < PB; ++i)
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          uh[i][u] = __builtin_amdgcn_raw_buffer_load_b128(r_up[u], upoff[i][u] + (unsigned)cbase * ESZ, 0, 0);
          ul[i][u] = __builtin_amdgcn_raw_buffer_load_b128(r_up[u], upoff[i][u] + (unsigned)cbase * ESZ + up_lo, 0, 0);
        }
      f16x8 ah[NB], al[NB], a2[NB];
      load_a((unsigned)pr * 4096u, ah, al);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a2[nb] = ah[nb] * (_Float16)0x1p-11f;
      f32x4 bias[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bias[nb] = *reinterpret_cast<const f32x4*>(smem + kBias + (unsigned)(cbase + 4 * nb) * 4u);
      f16x8 yh[PB], yl[PB];
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        f32x4 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        mfma3(acc, ah, al, a2, xh[i], xl[i]);
        // epilogue of the first conv for this pair: conv_ws_body's, value by value
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[nb][q] = __builtin_fmaf(acc[nb][q], winv, bias[nb][q]);
#pragma unroll
        for (int u = 0; u < 3; ++u) h2_add8(acc[0], acc[1], __builtin_bit_cast(f16x8, uh[i][u]), __builtin_bit_cast(f16x8, ul[i][u]));
        if (p.relu) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[nb][q] = acc[nb][q] > 0.f ? acc[nb][q] : 0.f;
        }
        h2_split8(acc[0], acc[1], yh[i], yl[i]);
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        f16x8 bh[NB], bl[NB], b2[NB];
        load_a(kW2 + (unsigned)(pr * Q + q) * 4096u, bh, bl);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b2[nb] = bh[nb] * (_Float16)0x1p-11f;
#pragma unroll
        for (int i = 0; i < PB; ++i) mfma3(acc2[i][q], bh, bl, b2, yh[i], yl[i]);
      }
    }
    // epilogue of the second conv: conv_ws_body's NCHW fp32 one (channels >= Cout2 are padding)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      f32x4 b2[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) b2[nb] = *reinterpret_cast<const f32x4*>(smem + kBias + 512u + (unsigned)(32 * q + 8 * kg + 4 * nb) * 4u);
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int no = pn[i] >= p.flip_from ? pn[i] + p.out_skip : pn[i];
        const unsigned base = ((unsigned)no * (unsigned)cout2 * (unsigned)p.Hout + (unsigned)py[i]) * (unsigned)p.Wout + (unsigned)px[i];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int cc = 32 * q + 8 * kg + 4 * nb + k;
            const float f = __builtin_fmaf(acc2[i][q][nb][k], winv2, b2[nb][k]);
            const unsigned off = (ok[i] && cc < cout2) ? (base + (unsigned)cc * hw) * 4u : kOobOff;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, f), r_z, off, 0, 0);
          }
      }
    }
  }
}

// `p`: the first conv as describe_all resolved it; `p2`: the second one (UDP_BUF_OUTPUT writer).  Returns 1 when there
// is no instantiation for the pair (the caller keeps the two launches).
int describe_head_chain(ConvParams p, const ConvParams& p2, Launch* out) {
  const int q = p2.CoutPad / 32;
  if (p.Cin != 32 || p.Cout != 128 || p.CoutPad != 128 || p2.Cin != 128 || (q != 1 && q != 2) || p2.Cout > p2.CoutPad || p.wfmt != 1 ||
      p2.wfmt != 1 || p.relu != UDP_ACT_RELU || p2.relu || p.res || p2.res || p2.nup || p.nout2 || p2.nout2 || !p2.out_nchw_f32 ||
      p.Hin != p.Hout || p.Win != p.Wout || p2.Hout != p.Hout || p2.Wout != p.Wout || p2.N != p.N || p.in_pitch % 8 || p.in_coff % 8)
    return 1;
  const long npix = (long)p.N * p.Hout * p.Wout;
  // 32-bit buffer offsets: X, the largest addend (shift 1: a quarter of the pixels, 128 channels) and Z
  if (npix * p.in_pitch * 4 >= 0x7FFF0000L || npix * 128 >= 0x7FFF0000L || (long)(p.N + p2.out_skip) * p.Hout * p.Wout * p2.Cout * 4 >= 0x7FFF0000L) return 1;
  for (int u = 0; u < p.nup; ++u)
    if (!p.up[u]) return 1;
  p.wgt2 = p2.wgt;
  p.bias2 = p2.bias;
  p.out2[0] = p2.out;
  p.out2_pitch[0] = p2.Cout;
  p.out2_coff[0] = p2.wexp;
  p.flip_from = p2.flip_from;
  p.out_skip = p2.out_skip;
  p.out = nullptr;                       // Y is not written
  const long groups = (npix + 31) / 32;
  out->fn = q == 1 ? reinterpret_cast<const void*>(&conv_head_chain_kernel<1>) : reinterpret_cast<const void*>(&conv_head_chain_kernel<2>);
  out->lds = (unsigned)(4 * 4096 + 4 * q * 4096 + (128 + 32 * q) * 4);
  out->grid = dim3((unsigned)std::min<long>(256, (groups + 7) / 8));     // persistent: one 8-wave workgroup per CU (192 / 216 registers)
  out->block = dim3(512);
  out->groupable = 0;
  out->ws_cp = 0;
  out->p = p;
  UDP_HIP_CHECK(hipFuncSetAttribute(out->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)out->lds));
  if (getenv("UDP_POSE_DEBUG_TILES"))
    fprintf(stderr, "head chain %dx%d C%d->%d->%d: wgs=%u lds=%u\n", p.Hout, p.Wout, p.Cin, p.Cout, p2.Cout, out->grid.x, out->lds);
  return UDP_OK;
}

int conv_ws_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
