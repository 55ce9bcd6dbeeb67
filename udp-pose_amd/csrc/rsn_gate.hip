// The gates of RSN-18 "se + prm" (RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py) for gfx950 (MI355X):
//   UDP_OP_SE_RES    the SELayer that closes every Bottleneck (:51-66, :137-143), with the shortcut add and the ReLU
//   UDP_OP_PRM_GATE  the channel gate of the Pose Refine Machine (:293-296)
//   UDP_OP_PRM_DW9   its spatial gate -- a depthwise 9x9 conv -- and the combine (:297-300)
// (include/udp_pose_hip.h has the contracts).
//
// gate_kernel<T, PRM> serves the first two: both are "pool, two small mat-vecs, sigmoid".  One workgroup per image,
// phases separated by barriers, in the scheme of se_kernel (dwconv.hip):
//   1. mean[c] over the HW pixels: thread (pixel group g, channel group) adds pixels g, g + P, ... in that order, then
//      the P partial sums of a channel are added in the order g = 0 .. P-1 and multiplied by 1 / HW;
//   2. h[j] = relu(b1[j] + sum_c W1[c][j] mean[c]), j < Ch: the channel range is cut into Q equal parts, thread
//      (part, j) runs its part with fmaf from 0 in channel order, the parts are added in order onto b1[j] (SE: onto 0);
//   3. v[c] = b2[c] (SE: 0), then fmaf(W2[j][c], h[j], v) for j = 0 .. Ch-1;  SE: m = sigmoid(v);  PRM: a = sigmoid(relu(v));
//   4. SE: out = act(fmaf(in, m[c], res)) (no res: in * m[c]), every element read and written by one thread;
//      PRM: the fp32 row a[C] of the image is stored.
// P and Q depend on (C, Ch) only and nothing is atomic: an image's result does not depend on the batch, the lane or
// graph replay.  Dynamic LDS: (256 * V + 2 * C + 256 + Ch) floats (V = 4 fp32 | 8 split fp16; at most 14,336 B).
//
// prm_dw9_kernel: 81 taps per output element.  At one global load per tap (dwconvk_kernel) the 64x48x256 map of the
// net would issue 81 x its own size in L1 requests; here a workgroup stages the input tile with its 4-pixel halo
// in LDS once, decoded to fp32, and every tap is an LDS read that feeds several FMAs from registers.
//   tile     8 rows x 16 columns of output x 32 channels per workgroup of 256 threads (4 waves);
//            staged input (8 + 8) x (16 + 8) pixels x 32 channels = 384 pixels, 3.0 x the output pixels
//            (16 x 16 would stage 2.25 x but needs 77 KiB: two workgroups per CU instead of three)
//   thread   4 consecutive output pixels of one row x 4 consecutive channels: per kernel row it reads 12 staged
//            pixels (12 ds_read_b128) and 9 weight quads (global, 16 bytes each, the same 10 KiB for every workgroup
//            of the channel group: L1 / L2 hits) for 9 x 4 x 4 = 144 fmaf
//   LDS      rows of 25 pixels (24 + 1 pad) x 32 floats: 16 x 25 x 32 x 4 B = 51,200 B static -> 3 workgroups per CU
//            (153.6 of 160 KiB) = 3 waves per SIMD.  A pixel is 128 B = one half of the 64 banks; the odd row pitch
//            makes the half alternate with the row, and lane = (channel quad 0-7, row 0-7), wave = column run 0-3,
//            puts both row parities into each 16-lane group of a b128 read: the four (row, quad half) pieces of a
//            group fall on four different 16-bank quarters -- SQ_LDS_BANK_CONFLICT = 0 in fp32 (NOTES.md).  All lanes of
//            a wave share their columns, so a wave runs EITHER the plain tap loop or the one with the per-tap test
//            (with the runs of a row spread over a wave's lanes two thirds of the waves ran both: 4.0 k VALU
//            instructions per wave for 1,296 fmaf)
//   VGPR     16 accumulators + 48 staged values + 36 weights + addresses: 116 (<= 128: 4 waves per SIMD allowed, one
//            more than the LDS admits)
// Measured (NOTES.md): 0.62 / 0.55 ms (f16x2 / f32) on [128, 64, 48, 256], 2.7 / 2.2 x an element-wise launch on the same
// three maps; 40 % of a wave's cycles are waits (SQ_WAIT_ANY), the LDS is busy 6 % of them.  A second
// form -- 8 pixels per thread, the weights staged in LDS, 128 threads, 61.6 KB: one wave per SIMD -- halves the LDS
// and L1 requests per fmaf and ran at 1.32 ms: the occupancy is worth more than the requests, so this form stayed.
// Arithmetic per output element (the contract of UDP_OP_DWCONV): acc = bias, then one fmaf per tap in the order
// ky, kx; a tap outside the image is skipped -- never multiplied by zero -- so the result does not depend on the
// tiling.  Threads whose 12 columns all lie inside the image run without the per-tap test.
// Epilogue: s = 1 / (1 + expf(-max(acc, 0)));  out = res * fmaf(a[c], s, 1).
#include "dw_dev.h"

namespace udp {

// V consecutive channels from `c` of pixel `pix` of the residual view, decoded to fp32
template <typename T, int V>
__device__ __forceinline__ void res_load(const ConvParams& p, size_t pix, int c, float (&x)[V]) {
#pragma unroll
  for (int q = 0; q < V; q += 4) {
    const f32x4 v = ld4<T>(p.res, pix, p.res_pitch, p.res_coff + c + q);
    x[q] = v[0], x[q + 1] = v[1], x[q + 2] = v[2], x[q + 3] = v[3];
  }
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// Parameter block (fp32): SE  W1 transposed [C][Ch], W2 transposed [Ch][C]
//                         PRM W1 transposed [C][Ch], b1 [Ch], W2 transposed [Ch][C], b2 [C]      (Ch = C)
template <typename T, bool PRM>
__global__ __launch_bounds__(256) void gate_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V;
  extern __shared__ __attribute__((aligned(16))) float gate_s[];
  const int C = p.Cin, Ch = p.up_shift[0], HW = p.Hin * p.Win;
  float* part = gate_s;                // [P][C], P * C <= 256 * V
  float* mean = part + 256 * V;        // [C]
  float* mul = mean + C;               // [C]
  float* hpart = mul + C;              // [Q][Ch], Q * Ch <= 256
  float* hid = hpart + 256;            // [Ch]
  const int tid = threadIdx.x;
  const size_t img = (size_t)blockIdx.x * HW;
  const int cgs = C / V;
  const int P = 256 / cgs < HW ? 256 / cgs : HW;        // cgs <= 128 (C <= 512)
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
  const float* b1 = w1 + (size_t)C * Ch;                 // PRM only
  const float* w2 = PRM ? b1 + Ch : b1;
  const float* b2 = w2 + (size_t)Ch * C;                 // PRM only
  const int Q = 256 / Ch < C ? 256 / Ch : C;             // Ch <= 256
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
    float s = PRM ? b1[tid] : 0.f;
    for (int q = 0; q < Q; ++q) s += hpart[q * Ch + tid];
    hid[tid] = __builtin_fmaxf(s, 0.f);
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = PRM ? b2[c] : 0.f;
    for (int j = 0; j < Ch; ++j) s = __builtin_fmaf(w2[(size_t)j * C + c], hid[j], s);
    if constexpr (PRM) reinterpret_cast<float*>(p.out)[(size_t)blockIdx.x * C + c] = sigmoidf(__builtin_fmaxf(s, 0.f));
    else mul[c] = sigmoidf(s);
  }
  if constexpr (!PRM) {
    __syncthreads();
    for (int e = tid; e < HW * cgs; e += 256) {
      const int cg = e % cgs, px = e / cgs;
      float x[V];
      dw_load<T, V>(p, img + px, cg * V, x);
      if (p.res) {
        float r[V];
        res_load<T, V>(p, img + px, cg * V, r);
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = __builtin_fmaf(x[k], mul[cg * V + k], r[k]);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] *= mul[cg * V + k];
      }
      dw_store<T, V>(p, img + px, cg * V, x);          // (+ ReLU if p.relu)
    }
  }
}

constexpr int D9_TH = 8, D9_TW = 16, D9_CG = 32, D9_P = 4, D9_NT = 256;    // output tile, channels per workgroup, pixels per thread, threads
constexpr int D9_IH = D9_TH + 8, D9_IW = D9_TW + 8, D9_ROWP = D9_IW + 1;   // staged tile and its row pitch in pixels

// workgroup = (image, tile row, tile column, channel group of 32), the channel group fastest; p.tiles_x / p.tiles_y
// tiles per image
template <typename T>
__global__ __launch_bounds__(D9_NT) void prm_dw9_kernel(const ConvParams p) {
  constexpr int V = DwTr<T>::V, LG = D9_CG / V;
  __shared__ __attribute__((aligned(16))) float tile[D9_IH * D9_ROWP * D9_CG];
  const int tid = threadIdx.x;
  int b = (int)blockIdx.x;
  const int ncg = p.Cin / D9_CG;
  const int cg0 = (b % ncg) * D9_CG;
  b /= ncg;
  const int x0 = (b % p.tiles_x) * D9_TW;
  b /= p.tiles_x;
  const int y0 = (b % p.tiles_y) * D9_TH;
  const int n = b / p.tiles_y;
  const size_t img = (size_t)n * p.Hin * p.Win;
  // staging: a thread's NI 16-byte groups are all loaded before the first LDS store, so that their latencies overlap
  // (one load -> store round per group cost 4 % / 15 % more, f16x2 / f32, NOTES.md)
  constexpr int NI = D9_IH * D9_IW * LG / D9_NT;                   // 12 fp32 | 6 split fp16: 48 registers
  static_assert(NI * D9_NT == D9_IH * D9_IW * LG, "the staged tile is a whole number of rounds");
  float st[NI][V];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int e = tid + i * D9_NT, g = e % LG, px = e / LG, sx = px % D9_IW, sy = px / D9_IW;
    const int iy = y0 - 4 + sy, ix = x0 - 4 + sx;
    // a position outside the image loads the nearest pixel inside instead (straight-line code: no branch between the
    // loads); what it stages is never used, the tap is skipped
    const int cy = iy < 0 ? 0 : iy >= p.Hin ? p.Hin - 1 : iy, cx = ix < 0 ? 0 : ix >= p.Win ? p.Win - 1 : ix;
    dw_load<T, V>(p, img + (size_t)cy * p.Win + cx, cg0 + g * V, st[i]);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int e = tid + i * D9_NT, g = e % LG, px = e / LG, sx = px % D9_IW, sy = px / D9_IW;
    float* d = tile + (sy * D9_ROWP + sx) * D9_CG + g * V;
#pragma unroll
    for (int q = 0; q < V; q += 4) *reinterpret_cast<f32x4*>(d + q) = f32x4{st[i][q], st[i][q + 1], st[i][q + 2], st[i][q + 3]};
  }
  __syncthreads();
  const int cq = tid & 7, row = (tid >> 3) & 7, xr = tid >> 6;      // a wave = one column run: `inner` below is wave-uniform
  const int oy = y0 + row, ox0 = x0 + xr * D9_P, c = cg0 + cq * 4;
  if (oy >= p.Hin || ox0 >= p.Win) return;                         // (no barrier below)
  float acc[D9_P][4];
  {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + c);
#pragma unroll
    for (int q = 0; q < D9_P; ++q) acc[q][0] = bv[0], acc[q][1] = bv[1], acc[q][2] = bv[2], acc[q][3] = bv[3];
  }
  const float* wg = reinterpret_cast<const float*>(p.wgt) + c;
  const bool inner = ox0 - 4 >= 0 && ox0 + D9_P + 3 < p.Win;       // all 12 columns of the thread inside the image
#pragma unroll 1
  for (int ky = 0; ky < 9; ++ky) {
    const int iy = oy + ky - 4;
    if (iy < 0 || iy >= p.Hin) continue;
    const float* src = tile + ((row + ky) * D9_ROWP + xr * D9_P) * D9_CG + cq * 4;
    f32x4 x[D9_P + 8], w[9];
#pragma unroll
    for (int j = 0; j < D9_P + 8; ++j) x[j] = *reinterpret_cast<const f32x4*>(src + j * D9_CG);
#pragma unroll
    for (int kx = 0; kx < 9; ++kx) w[kx] = *reinterpret_cast<const f32x4*>(wg + (size_t)(ky * 9 + kx) * p.Cin);
    if (inner) {
#pragma unroll
      for (int kx = 0; kx < 9; ++kx)
#pragma unroll
        for (int q = 0; q < D9_P; ++q)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[q][k] = __builtin_fmaf(x[q + kx][k], w[kx][k], acc[q][k]);
    } else {
#pragma unroll
      for (int kx = 0; kx < 9; ++kx)
#pragma unroll
        for (int q = 0; q < D9_P; ++q) {
          const int ix = ox0 + q + kx - 4;
          const bool in = ix >= 0 && ix < p.Win;
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[q][k] = in ? __builtin_fmaf(x[q + kx][k], w[kx][k], acc[q][k]) : acc[q][k];
        }
    }
  }
  const f32x4 a = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.up[0]) + (size_t)n * p.Cin + c);
#pragma unroll
  for (int q = 0; q < D9_P; ++q) {
    if (ox0 + q >= p.Win) break;
    const size_t pix = img + (size_t)oy * p.Win + ox0 + q;
    const f32x4 r = ld4<T>(p.res, pix, p.res_pitch, p.res_coff + c);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = r[k] * __builtin_fmaf(a[k], sigmoidf(__builtin_fmaxf(acc[q][k], 0.f)), 1.f);
    st4<T>(p.out, pix, p.out_pitch, p.out_coff + c, o);            // (split fp16: raises the range flag)
  }
}

// ---------------------------------------------------------------------------------------------- host side
static int views_ok(const udp_conv_op& o) {
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  return !(o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8);
}
static int res_view_ok(const udp_conv_op& o) {
  const int rpitch = o.res_pitch ? o.res_pitch : o.cout;
  return !(o.res_coff < 0 || o.res_coff + o.cout > rpitch || (o.res_coff | rpitch) % 8);
}

// UDP_OP_SE_RES: cin == cout stored channels (a multiple of 32, at most 512), chain_cout = hidden width (1 .. 256)
int se_res_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "se + residual: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "se + residual: dtype %d", dtype);
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cin > 512 || o.cout_pad != o.cout || o.chain_cout < 1 || o.chain_cout > 256 ||
      o.hin < 1 || o.win < 1 || o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "se + residual: cin == cout == cout_pad, a multiple of 32 up to 512, hidden width (chain_cout) 1 .. 256, "
                "output = input size (C%d->%d, hidden %d)", o.cin, o.cout, o.chain_cout);
  if (!views_ok(o) || !res_view_ok(o)) return fail(UDP_ERR_ARG, "se + residual: channel views");
  if (o.relu != UDP_ACT_NONE && o.relu != UDP_ACT_RELU)
    return o.relu == UDP_ACT_HSWISH || o.relu == UDP_ACT_SILU ? fail(UDP_ERR_UNSUPPORTED, "se + residual: activation none | ReLU only (code %d)", o.relu)
                                                              : fail(UDP_ERR_ARG, "se + residual: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "se + residual: no up-sampled addends, second outputs, groups or NCHW output");
  return UDP_OK;
}

// UDP_OP_PRM_GATE: cin == cout stored channels (a multiple of 32, at most 256: the hidden layer is as wide), out = fp32 rows
int prm_gate_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "prm channel gate: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "prm channel gate: dtype %d", dtype);
  if (o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cin > 256 || o.cout_pad != o.cout || o.chain_cout || o.hin < 1 || o.win < 1 ||
      o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "prm channel gate: cin == cout == cout_pad, a multiple of 32 up to 256, chain_cout 0, hout x wout = the map "
                "(C%d->%d, chain_cout %d)", o.cin, o.cout, o.chain_cout);
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
  if (o.in_coff < 0 || o.in_coff + o.cin > ipitch || (o.in_coff | ipitch) % 8 || o.out_coff || (o.out_pitch && o.out_pitch != o.cout))
    return fail(UDP_ERR_ARG, "prm channel gate: channel views (the output is a dense fp32 row per image)");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "prm channel gate: activation code %d", o.relu);
  if (o.n_up || o.n_out2 || o.group || o.in_stuff2 || o.wfmt || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "prm channel gate: no addends, activation code, second outputs, groups or NCHW output");
  return UDP_OK;
}

// UDP_OP_PRM_DW9: depthwise 9x9 stride 1 on cin == cout stored channels (a multiple of 32), n_up = 1: up_buf[0] = the gate rows
int prm_dw9_validate(const udp_conv_op& o, int dtype) {
  if (dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "prm spatial gate: storage modes f32 and f16x2 only");
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "prm spatial gate: dtype %d", dtype);
  if (o.ks != 9 || o.stride != 1 || o.cin <= 0 || o.cin != o.cout || o.cin % 32 || o.cout_pad != o.cout || o.hin < 1 || o.win < 1 ||
      o.hout != o.hin || o.wout != o.win)
    return fail(UDP_ERR_ARG, "prm spatial gate: 9x9, stride 1, cin == cout == cout_pad, a multiple of 32, output = input size "
                "(k%d s%d C%d->%d %dx%d -> %dx%d)", o.ks, o.stride, o.cin, o.cout, o.hin, o.win, o.hout, o.wout);
  if (!views_ok(o) || !res_view_ok(o)) return fail(UDP_ERR_ARG, "prm spatial gate: channel views");
  if (o.relu < 0 || o.relu > UDP_ACT_SILU || o.relu == 3) return fail(UDP_ERR_ARG, "prm spatial gate: activation code %d", o.relu);
  if (o.n_up != 1 || o.up_shift[0] != 0) return fail(UDP_ERR_ARG, "prm spatial gate: n_up = 1, up_buf[0] = the channel gate's rows, up_shift[0] = 0");
  if (o.n_out2 || o.chain_cout || o.group || o.in_stuff2 || o.wfmt || o.relu || o.out_buf == UDP_BUF_OUTPUT)
    return fail(UDP_ERR_UNSUPPORTED, "prm spatial gate: no activation code, second outputs, chain, groups or NCHW output; weights fp32 [81][C] (wfmt 0)");
  return UDP_OK;
}

// p: geometry, views, in / out (PRM: the fp32 rows), wgt = the parameter block, up_shift[0] = hidden width; SE: res
// (optional) with its view, relu.  One workgroup per image.
int describe_gate(ConvParams p, int dtype, bool prm, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "se / prm gate: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.wgt) return fail(UDP_ERR_ARG, "se / prm gate: null pointer");
  const int V = dtype == UDP_F32 ? 4 : 8, Ch = p.up_shift[0];
  if (p.Cin <= 0 || p.Cin % 32 || p.Cin > 512 || Ch < 1 || Ch > 256 || p.N <= 0) return fail(UDP_ERR_ARG, "se / prm gate: C %d, hidden %d", p.Cin, Ch);
  if (prm) out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&gate_kernel<float, true>) : reinterpret_cast<const void*>(&gate_kernel<H2, true>);
  else out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&gate_kernel<float, false>) : reinterpret_cast<const void*>(&gate_kernel<H2, false>);
  out->grid = dim3((unsigned)p.N);
  out->block = dim3(256);
  out->lds = (unsigned)((256 * V + 2 * p.Cin + 256 + Ch) * sizeof(float));
  out->p = p;
  return UDP_OK;
}

// p: geometry, views, in / res / out, wgt = fp32 [81][C], bias, up[0] = the gate rows
int describe_prm_dw9(ConvParams p, int dtype, Launch* out) {
  if (dtype != UDP_F32 && dtype != UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "prm spatial gate: storage modes f32 and f16x2 only");
  if (!p.in || !p.out || !p.res || !p.wgt || !p.bias || !p.up[0]) return fail(UDP_ERR_ARG, "prm spatial gate: null pointer");
  if (p.Cin <= 0 || p.Cin % D9_CG || p.N <= 0 || p.Hin < 1 || p.Win < 1) return fail(UDP_ERR_ARG, "prm spatial gate: C %d, %dx%d", p.Cin, p.Hin, p.Win);
  p.tiles_x = (p.Win + D9_TW - 1) / D9_TW;
  p.tiles_y = (p.Hin + D9_TH - 1) / D9_TH;
  const long total = (long)p.N * p.tiles_y * p.tiles_x * (p.Cin / D9_CG);
  if (total <= 0 || total >= (1L << 31) - 1) return fail(UDP_ERR_UNSUPPORTED, "prm spatial gate: %ld workgroups; split the batch", total);
  out->fn = dtype == UDP_F32 ? reinterpret_cast<const void*>(&prm_dw9_kernel<float>) : reinterpret_cast<const void*>(&prm_dw9_kernel<H2>);
  out->grid = dim3((unsigned)total);
  out->block = dim3(D9_NT);
  out->lds = 0;
  out->p = p;
  return UDP_OK;
}

int rsn_gate_h2_overflow(hipStream_t s, int reset, int* flag) { return h2_overflow_fetch(s, reset, flag); }

}  // namespace udp
