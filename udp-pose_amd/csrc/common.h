// Shared host-side helpers of libudp_pose_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../include/udp_pose_hip.h"

namespace udp {

inline char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define UDP_HIP_CHECK(expr)                                                                  \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return udp::fail(UDP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                       __FILE__, __LINE__);                                                  \
  } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// workgroups of a grid-stride kernel: ceil(total / per), at least 1, at most cap
inline unsigned blocks_for(long total, int per, long cap) {
  long b = (total + per - 1) / per;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}
// behind a <<<...>>> launch of entry point `who`
inline int launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return UDP_OK;
}

// Split-fp16 ("f16x2") range guard.  fp16 tops out at 65504: a value of magnitude >= 65520 splits into hi = inf, and
// the NaN that grows out of it downstream does not survive a ReLU (max(NaN, 0) = 0), so a finiteness test of the
// final heat-maps can miss it.  Every kernel that WRITES split-fp16 values therefore raises this flag at the source
// (one per translation unit; udp_f16x2_overflow() ORs them).
//   h2_range_check(m): m = the magnitude of ONE value about to be split (NaN compares false, so `!(m < limit)` catches
//   it too).  Never hand it an fmaxf() over several values: fmaxf(NaN, x) = x loses a NaN among finite siblings.
//   h2_range_check_bits(m): m = the largest h2_mag() of SEVERAL values.  The bit pattern of |v| as an unsigned integer
//   orders like the magnitude, with inf and every NaN above all finite values, so an integer max keeps what fmaxf drops.
static __device__ int g_h2_overflow;
__device__ __forceinline__ void h2_range_check(float m) {
  if (!(m < 65520.f)) g_h2_overflow = 1;
}
__device__ __forceinline__ unsigned h2_mag(float v) { return __builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned h2_max(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ void h2_range_check_bits(unsigned m) {
  if (m >= __builtin_bit_cast(unsigned, 65520.f)) g_h2_overflow = 1;
}
// flag of the calling translation unit after `s` has drained; cleared when `reset`
static inline int h2_overflow_fetch(hipStream_t s, int reset, int* flag) {
  int v = 0;
  UDP_HIP_CHECK(hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(g_h2_overflow), sizeof(int), 0, hipMemcpyDeviceToHost, s));
  UDP_HIP_CHECK(hipStreamSynchronize(s));
  if (v && reset) {
    const int z = 0;
    UDP_HIP_CHECK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_h2_overflow), &z, sizeof(int), 0, hipMemcpyHostToDevice, s));
    UDP_HIP_CHECK(hipStreamSynchronize(s));
  }
  *flag |= v != 0;
  return UDP_OK;
}

// Parameters of one fused conv launch (device-visible, passed by value).
struct ConvParams {
  const void* in;
  void* out;
  const void* wgt;
  const float* bias;
  const void* wgt2;      // fused BasicBlock: second conv's weights / bias
  const float* bias2;
  const void* res;
  const void* up[3];
  int up_shift[3];
  int nup;
  int N, Hin, Win, Cin, Hout, Wout, Cout, CoutPad;
  int in_pitch, in_coff, out_pitch, out_coff, res_pitch, res_coff;   // channel-slice views (elements); pitch = channels per pixel of the stored tensor
  int G, R, TW;          // tile = G images x R rows x TW cols of output
  int IH, IW;            // input halo tile per image
  int tiles_x, tiles_y;  // tiles per image group
  unsigned mTX, mTY;     // ceil(2^32/d), 0 for d == 1 (tile index decode, t < 65536)
  int ntiles;            // all tiles of the launch (persistent workgroups stride over them)
  unsigned mIW, mIH, mRT, mTW;  // ceil(2^20/d): x/d == (x*m) >> 20 for x*d < 2^20 (24-bit multiply)
  int relu;              // udp_conv_op.relu: 0 none, 1 ReLU, 2 hard-swish / 4 SiLU (the *_hs / SILU instantiations only)
  int out_nchw_f32;      // epilogue writes NCHW fp32 (network output) instead of NHWC T
  int flip_from;         // stem only: images >= flip_from read image (n - flip_from) mirrored in x
  int sbuf;              // conv_mfma_kernel: one stage buffer instead of two (set by conv_choose_tile)
  int wfmt;              // udp_conv_op.wfmt: 1 = fragment-major split-fp16 weights (conv_ws_h2_kernel)
  int wexp;              // udp_conv_op.wexp: those weights are stored scaled by 2^wexp
  int in_stuff2;         // udp_conv_op.in_stuff2: conv_mfma_kernel reads the [Hin/2][Win/2] input as its zero-stuffed image
  int out_skip;          // NCHW fp32 output of the weight-stationary kernels: images >= flip_from are written out_skip image
                         // rows further on (a sub-batch lane's mirrored half lands behind ALL the plain images, hrnet.hip)
  double* bn_ws;         // training: per-workgroup BatchNorm partial sums of the output, [tile][2*Cout] (or null)
  // udp_conv_op.n_out2: second outputs out2[k] = out (as stored) + add2[k] of the weight-stationary split-fp16 convs
  void* out2[2];
  const void* add2[2];
  int nout2, out2_coff[2], out2_pitch[2], add2_coff[2], add2_pitch[2];
};

// Kernel argument of conv_mfma_multi: up to 4 independent convs in one launch (flat block index ->
// sub-problem j, tile, cout block).
constexpr int kMultiSegs = 64;
constexpr int kMultiTab = 480;
struct ConvMulti {
  ConvParams p[4];
  unsigned start[5];      // first flat block of sub-problem j; unused entries 0xFFFFFFFF, start[4] = total
  unsigned tiles[4];      // tiles (grid.x) of sub-problem j
  unsigned ncby[4];       // conv_ws_multi: cout blocks (grid.y) of sub-problem j
  int code[4];            // conv_ws_multi: cout pairs per workgroup (CP) of sub-problem j
  // conv_ws_multi dispatch order: the grid is a sequence of segments, segment s = workgroups seg_first[s] ..
  // of member seg_mem[s], placed at flat blocks seg_start[s] .. seg_start[s + 1] - 1 (unused: 0xFFFFFFFF)
  unsigned seg_start[kMultiSegs];
  unsigned seg_first[kMultiSegs];
  int seg_mem[kMultiSegs];
  // the same order resolved per run of 8 workgroups, when every boundary is a multiple of 8: tab[b >> 3] =
  // member | log2(CP) << 2 | cout block << 4 | first tile << 10, workgroup b takes tile (tab >> 10) + (b & 7).  ONE scalar load whose
  // address only needs blockIdx, instead of the table search + three dependent loads (1.6 us of every workgroup's
  // 15-60 us, tools/stamp_multi.py).  tab_n == 0: search the segment table.
  unsigned tab_n;
  unsigned tab[kMultiTab];
};

// Kernel argument of conv_ws_s2x_kernel: 1..3 stride-2 3x3 convs over the SAME 32-channel input view ("routes", one
// tile geometry, at most 4 cout pairs in all) and, optionally, the element-wise sum that reads that view too.
constexpr int kShareRoutes = 3;
struct ConvShare {
  ConvParams p[kShareRoutes];   // the routes; their tile fields are equal
  ConvParams side;              // the UDP_OP_FUSE member (side.out == null: none); mRT / mTW: magic numbers of its patch
  unsigned route;               // byte s: route of the workgroup's cout-pair slot s (wave s % CP)
  unsigned lpair;               // byte s: that slot's pair inside its route (a slot without a route: 255)
};

}  // namespace udp

namespace udp {
// One kernel launch, described once and then either enqueued on a stream or added to a hipGraph.
struct Launch {
  const void* fn = nullptr;
  dim3 grid, block;
  unsigned lds = 0;
  int groupable = 0;   // conv described by describe_conv_grouped: may be merged with its group siblings
  int ws_cp = 0;       // weight-stationary member: its cout pairs per workgroup
  int pair = 0;        // this launch also does the NEXT op's work (describe_head_chain): the executor skips that op's own launch
  int carried = 0;     // this op's work is done by an EARLIER launch (mark_x0_share): it has no launch of its own
  int n_carry = 0;     // ops this launch carries (later in the program, not adjacent) ...
  int carry[kShareRoutes] = {0, 0, 0};
  int cross_lane = 0;  // ... some of them from another lane than this op's: the program runs as one chain
  std::shared_ptr<ConvShare> share;   // ... and then its kernel argument (instead of `p`)
  ConvParams p;
};
// conv_ws.hip: one launch for convs[0..n) (3x3 stride 2 over one 32-channel view) and `fuse` (may be null); 1: no kernel
// (`tag`: the members, for the UDP_POSE_DEBUG_TILES line)
int describe_x0_share(const ConvParams* convs, int n, const ConvParams* fuse, const char* tag, Launch* out);
// conv_ws.hip: the weight-stationary split-fp16 convs (tile choice + kernel of one conv; merged launch of 2..4)
int describe_conv_ws(ConvParams p, int ks, int stride, Launch* out, bool grouped = false);
struct WsTile {
  int cp, pb, G, R, TW, wgs, sbuf;
  size_t lds;
};
int choose_conv_ws(ConvParams& p, int ks, int stride, bool grouped, WsTile* best);   // its tile choice alone (host arithmetic, no HIP call)
int describe_ws_multi(const Launch* members, int n, ConvMulti* m, Launch* out);
// conv7.hip: UDP_OP_CONV with ks = 7 (stride 1, f32 / f16x2): weights streamed through LDS one kernel row at a time
int describe_conv7(ConvParams p, int dtype, int stride, Launch* out);
int conv7_refuse(const ConvParams& p, int dtype, int stride);          // the refusals of its contract alone (UDP_OK: none applies)
size_t conv7_choose_tile(ConvParams& p, int dtype, int* nb_out);       // its tile choice alone (host arithmetic, no HIP call); 0: nothing fits
int conv7_h2_overflow(hipStream_t s, int reset, int* flag);
int describe_conv_chain(ConvParams p, Launch* out);   // two 1x1 convs chained through registers (udp_conv_op.chain_cout)
// a 1x1 conv with up-sampled addends + ReLU chained into the 1x1 conv that writes the net's NCHW fp32 output; 1: no such kernel
int describe_head_chain(ConvParams p, const ConvParams& p2, Launch* out);
void ws_set_fill_wgs(long wgs);                      // workgroups a conv launched on its own should reach (tile choice)
int ws_set_stamps(unsigned long long* dev_buf);      // diagnostic builds (-DUDP_STAMPS) only
// deconv.hip: ConvTranspose2d(k=4, s=2, p=1) + folded BatchNorm (+ ReLU), UDP_OP_DECONV (fp32 and split fp16)
int describe_deconv(ConvParams p, int dtype, Launch* out);
int deconv_h2_overflow(hipStream_t s, int reset, int* flag);
// dwconv.hip: depthwise 3x3 conv + folded BatchNorm with the ShuffleV2 passthrough (UDP_OP_DWCONV), PixelShuffle(2)
// (UDP_OP_PIXSHUF); the *_validate functions hold the field rules of udp_pose_hip.h for both entry points
int dwconv_validate(const udp_conv_op& o, int dtype);
int pixshuf_validate(const udp_conv_op& o, int dtype);
int describe_dwconv(ConvParams p, int dtype, int ks, int stride, Launch* out);
int describe_pixshuf(ConvParams p, int dtype, Launch* out);
int se_validate(const udp_conv_op& o, int dtype);                // UDP_OP_SE (squeeze-and-excitation, one workgroup per image)
int describe_se(ConvParams p, int dtype, Launch* out);
int se_act_validate(const udp_conv_op& o, int dtype);            // UDP_OP_SE_ACT (activation + squeeze-and-excitation with both biases, C up to 1024)
int describe_se_act(ConvParams p, int dtype, Launch* out);
int dwconv_h2_overflow(hipStream_t s, int reset, int* flag);
// attn.hip: GroupNorm(1, C) (UDP_OP_GNORM) and the separable self-attention core (UDP_OP_LINATTN), one workgroup per image
int gnorm_validate(const udp_conv_op& o, int dtype);
int linattn_validate(const udp_conv_op& o, int dtype);
int describe_gnorm(ConvParams p, int dtype, Launch* out);
int describe_linattn(ConvParams p, int dtype, Launch* out);
// attn.hip: LayerNorm per pixel (UDP_OP_LNORM), soft-max multi-head self-attention (UDP_OP_MHATTN) and the stand-alone
// activation (UDP_OP_ACT) of MobileViT
int lnorm_validate(const udp_conv_op& o, int dtype);
int mhattn_validate(const udp_conv_op& o, int dtype);
int act_op_validate(const udp_conv_op& o, int dtype);
int describe_lnorm(ConvParams p, int dtype, Launch* out);
int describe_mhattn(ConvParams p, int dtype, Launch* out);
int describe_act(ConvParams p, int dtype, Launch* out);
int attn_h2_overflow(hipStream_t s, int reset, int* flag);
// rsn_gate.hip: the SE layer with residual (UDP_OP_SE_RES), the channel gate (UDP_OP_PRM_GATE) and the depthwise 9x9
// spatial gate + combine (UDP_OP_PRM_DW9) of RSN-18 "se + prm"
int se_res_validate(const udp_conv_op& o, int dtype);
int prm_gate_validate(const udp_conv_op& o, int dtype);
int prm_dw9_validate(const udp_conv_op& o, int dtype);
int describe_gate(ConvParams p, int dtype, bool prm, Launch* out);
int describe_prm_dw9(ConvParams p, int dtype, Launch* out);
int rsn_gate_h2_overflow(hipStream_t s, int reset, int* flag);
int conv_h2_overflow(hipStream_t s, int reset, int* flag);       // conv.hip / conv_ws.hip / psa.hip: their g_h2_overflow
int conv_ws_h2_overflow(hipStream_t s, int reset, int* flag);
int psa_h2_overflow(hipStream_t s, int reset, int* flag);
}  // namespace udp
