// HRNet forward executor: runs the host-built program of fused conv launches
// (include/udp_pose_hip.h, udp_conv_op) on one HIP stream, optionally replaying
// it as a hipGraph.  Replaces PoseHighResolutionNet.forward,
// deep_hrnet/lib/models/pose_hrnet.py:436-471.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"

namespace udp {
int describe_conv(ConvParams p, int dtype, int ks, int stride, Launch* out);
int describe_stem(const ConvParams& p, int dtype, Launch* out);
int describe_fuse(const ConvParams& p, int dtype, Launch* out);
int describe_stem7(const ConvParams& p, int dtype, Launch* out);
int describe_maxpool(const ConvParams& p, int dtype, Launch* out);
int describe_bilinear(const ConvParams& p, int dtype, Launch* out);
int describe_psa(const ConvParams& p, int dtype, int kind, Launch* out);
int describe_block(ConvParams p, int dtype, Launch* out);
int describe_conv_grouped(ConvParams p, int dtype, int ks, int stride, Launch* out);
int describe_multi(const Launch* members, int n, ConvMulti* m, Launch* out);
int run_launch(const Launch& l, hipStream_t s);
}  // namespace udp

using namespace udp;

struct GraphEntry {
  int n, flip, skip;     // skip: ConvParams::out_skip of the output writers (a sub-batch lane writing its rows in place)
  const void* in;
  void* ws;
  void* out;
  hipGraph_t graph;
  hipGraphExec_t exec;
};

struct udp_hrnet {
  std::vector<udp_conv_op> ops;
  std::vector<int64_t> buf_elems;  // per image, rounded up to 64 elements
  std::vector<int64_t> buf_off;    // prefix sums (elements per image)
  int64_t total_elems = 0;
  const char* weights = nullptr;
  size_t weights_bytes = 0;
  int dtype = UDP_F32;
  int in_h = 0, in_w = 0, out_channels = 0;
  double flops = 0.0;
  std::vector<GraphEntry> graphs;
  // branch-parallel execution: lane 0 = caller's stream, lanes 1.. = internal streams
  int n_lanes = 1;
  hipStream_t lane_stream[UDP_MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t> op_done;     // one per op (recorded only where another lane waits on it)
  std::vector<char> op_signals;        // op has a cross-lane consumer
  hipEvent_t ev_fork = nullptr, ev_join[UDP_MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
  // sub-batch lanes (udp_hrnet_forward): the second half of a batch runs on this stream beside the first
  hipStream_t split_stream = nullptr;
  hipEvent_t split_fork = nullptr, split_join = nullptr;
  // every writer of UDP_BUF_OUTPUT honours ConvParams::out_skip (decided once, at create): the lanes of a flip-test
  // batch write their heat-map rows where the caller wants them; otherwise they are staged and copied into place
  bool out_in_place = false;
};

static size_t esize(int dtype) { return dtype == UDP_BF16 ? 2 : 4; }   // bytes per stored element (F16X2: hi + lo)

// udp_conv_op.relu as an activation code (udp_pose_hip.h, UDP_ACT_*).  Hard-swish and SiLU exist as separate
// instantiations of the stem kernels and of the plain 1x1 stride-1 NHWC convs (SiLU: of the depthwise convs too) only;
// everywhere else they are refused, never read as a ReLU.  Code 3 is not assigned.
static int act_validate(const udp_conv_op& o, int dtype, bool has_res) {
  if (o.relu < UDP_ACT_NONE || o.relu > UDP_ACT_SILU || o.relu == 3)
    return fail(UDP_ERR_ARG, "activation code %d (0 none, 1 ReLU, 2 hard-swish, 4 SiLU)", o.relu);
  if (o.relu < UDP_ACT_HSWISH || o.kind == UDP_OP_ACT || o.kind == UDP_OP_SE_ACT) return UDP_OK;      // (act_op_validate / se_act_validate have their rules)
  if (o.relu == UDP_ACT_SILU && o.kind == UDP_OP_DWCONV) return UDP_OK;      // (dwconv_validate refuses bf16)
  const bool plain1x1 = o.kind == UDP_OP_CONV && o.ks == 1 && o.stride == 1 && !o.group && !o.chain_cout && !o.n_up && !o.n_out2 && !has_res &&
                        !o.in_stuff2 && o.out_buf != UDP_BUF_OUTPUT;
  if (dtype == UDP_BF16 || (o.kind != UDP_OP_STEM && !plain1x1))
    return fail(UDP_ERR_UNSUPPORTED, "%s: UDP_OP_STEM and 1x1 stride-1 NHWC UDP_OP_CONV without addends, second outputs, "
                "chain or group, in f32 / f16x2 only (kind %d, ks %d, stride %d)",
                o.relu == UDP_ACT_SILU ? "SiLU (activation code 4; also UDP_OP_DWCONV)" : "hard-swish (activation code 2)", o.kind, o.ks, o.stride);
  return UDP_OK;
}

static int validate_op(const udp_hrnet* h, const udp_conv_op& o, int idx) {
  const int nb = (int)h->buf_elems.size();
  auto buf_ok = [&](int b, int64_t need) { return b >= 0 && b < nb && h->buf_elems[b] >= need; };
  const int64_t out_need = (int64_t)o.hout * o.wout * (o.out_pitch ? o.out_pitch : o.cout);
  if (o.kind < UDP_OP_STEM || o.kind > UDP_OP_SE_ACT) return fail(UDP_ERR_ARG, "op %d: bad kind %d", idx, o.kind);
  if (const int rc = act_validate(o, h->dtype, o.res_buf != UDP_BUF_NONE)) return rc;
  if (o.lane < 0 || o.lane >= UDP_MAX_LANES || o.n_wait < 0 || o.n_wait > UDP_MAX_WAIT) return fail(UDP_ERR_ARG, "op %d: lane/n_wait", idx);
  for (int k = 0; k < o.n_wait; ++k)
    if (o.wait_op[k] < 0 || o.wait_op[k] >= idx) return fail(UDP_ERR_ARG, "op %d: wait_op %d must name an earlier op", idx, o.wait_op[k]);
  if (o.kind == UDP_OP_BLOCK) {
    const int64_t hw = (int64_t)o.hin * o.win;
    if (h->dtype != UDP_BF16 || o.cin != 32 || o.cout != 32 || o.hin != o.hout || o.win != o.wout || o.hin % 8)
      return fail(UDP_ERR_ARG, "op %d: fused BasicBlock needs bf16, 32 channels, height %% 8 == 0", idx);
    if (!buf_ok(o.in_buf, hw * 32) || !buf_ok(o.out_buf, hw * 32) || o.in_buf == o.out_buf)
      return fail(UDP_ERR_ARG, "op %d: fused BasicBlock buffers", idx);
    const size_t wbytes = (size_t)9 * 32 * 32 * 2;
    const int64_t offs[4] = {o.w_off, o.w2_off, o.b_off, o.b2_off};
    for (int k = 0; k < 4; ++k)
      if (offs[k] < 0 || (size_t)offs[k] + (k < 2 ? wbytes : 32 * 4) > h->weights_bytes || (offs[k] & 15))
        return fail(UDP_ERR_ARG, "op %d: fused BasicBlock weight/bias range outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_DECONV) {
    // ConvTranspose2d(4, 2, 1) + folded BatchNorm (+ ReLU): hin x win -> 2hin x 2win, no addends (deconv.hip)
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
    const bool h2 = h->dtype == UDP_F16X2;
    if (h->dtype == UDP_BF16) return fail(UDP_ERR_UNSUPPORTED, "op %d: deconv: storage modes f32 and f16x2 only", idx);
    if (o.ks != 4 || o.stride != 2 || o.hin <= 0 || o.win <= 0 || o.hout != 2 * o.hin || o.wout != 2 * o.win || o.cin <= 0 ||
        o.cin % (h2 ? 32 : 16) || o.cout <= 0 || o.cout % 8 || o.cout_pad < o.cout || o.cout_pad % 32)
      return fail(UDP_ERR_ARG, "op %d: deconv must be k4 s2 p1, %dx%d -> 2x, cin %% %d == 0, cout %% 8 == 0", idx, o.hin, o.win, h2 ? 32 : 16);
    if (o.wfmt != (h2 ? 1 : 0)) return fail(UDP_ERR_ARG, "op %d: deconv weights: wfmt %d (f16x2: 1, f32: 0)", idx, o.wfmt);
    if (o.res_buf != UDP_BUF_NONE || o.n_up || o.n_out2 || o.chain_cout || o.group || o.in_stuff2)
      return fail(UDP_ERR_UNSUPPORTED, "op %d: deconv takes no addends, second outputs, chains or groups", idx);
    if (o.in_coff < 0 || o.out_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch || (o.in_coff | ipitch | o.out_coff | opitch) % 8)
      return fail(UDP_ERR_ARG, "op %d: deconv channel views", idx);
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.in_buf == o.out_buf)
      return fail(UDP_ERR_ARG, "op %d: deconv buffers missing, too small or aliased", idx);
    const size_t wbytes = h2 ? (size_t)16 * (o.cin / 32) * (o.cout_pad / 32) * 4096 : (size_t)16 * o.cout_pad * o.cin * 4;
    if (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15) || o.b_off < 0 ||
        (size_t)o.b_off + (size_t)o.cout_pad * 4 > h->weights_bytes || (o.b_off & 15) || o.wexp < -40 || o.wexp > 40)
      return fail(UDP_ERR_ARG, "op %d: deconv weight / bias range outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_SE) {
    // squeeze-and-excitation (dwconv.hip); `out` may be the very view `in` is
    const int rc = se_validate(o, h->dtype);
    if (rc) return rc;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.res_buf != UDP_BUF_NONE)
      return fail(UDP_ERR_ARG, "op %d: squeeze-excitation buffers missing or too small (or a residual)", idx);
    if (o.in_buf == o.out_buf && (o.in_coff != o.out_coff || ipitch != (o.out_pitch ? o.out_pitch : o.cout)))
      return fail(UDP_ERR_ARG, "op %d: squeeze-excitation in place needs the same view for in and out", idx);
    const size_t wbytes = ((size_t)2 * o.cin * o.chain_cout + o.chain_cout) * 4;
    if (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15))
      return fail(UDP_ERR_ARG, "op %d: squeeze-excitation parameter block outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_SE_ACT) {
    // activation + squeeze-and-excitation with both biases (dwconv.hip); `out` may be the very view `in` is
    const int rc = se_act_validate(o, h->dtype);
    if (rc) return rc;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.res_buf != UDP_BUF_NONE)
      return fail(UDP_ERR_ARG, "op %d: activation + squeeze-excitation buffers missing or too small (or a residual)", idx);
    if (o.in_buf == o.out_buf && (o.in_coff != o.out_coff || ipitch != (o.out_pitch ? o.out_pitch : o.cout)))
      return fail(UDP_ERR_ARG, "op %d: activation + squeeze-excitation in place needs the same view for in and out", idx);
    const size_t wbytes = ((size_t)2 * o.cin * o.chain_cout + o.chain_cout + o.cin) * 4;      // W1, b1, W2, b2
    if (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15))
      return fail(UDP_ERR_ARG, "op %d: activation + squeeze-excitation parameter block outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_SE_RES || o.kind == UDP_OP_PRM_GATE || o.kind == UDP_OP_PRM_DW9) {
    // the gates of RSN-18 "se + prm" (rsn_gate.hip); the SE layer's `out` may be the very view `in` is
    const char* what = o.kind == UDP_OP_SE_RES ? "se + residual" : o.kind == UDP_OP_PRM_GATE ? "prm channel gate" : "prm spatial gate";
    const int rc = o.kind == UDP_OP_SE_RES ? se_res_validate(o, h->dtype) : o.kind == UDP_OP_PRM_GATE ? prm_gate_validate(o, h->dtype) : prm_dw9_validate(o, h->dtype);
    if (rc) return rc;
    const int64_t hw = (int64_t)o.hin * o.win;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin, rpitch = o.res_pitch ? o.res_pitch : o.cout;
    const int64_t rows = (int64_t)o.cin * (4 / (int64_t)esize(h->dtype));        // an fp32 row a[C], counted in `dtype` elements
    if (!buf_ok(o.in_buf, hw * ipitch) || !buf_ok(o.out_buf, o.kind == UDP_OP_PRM_GATE ? rows : out_need))
      return fail(UDP_ERR_ARG, "op %d: %s buffers missing or too small", idx, what);
    if (o.kind == UDP_OP_PRM_GATE ? o.res_buf != UDP_BUF_NONE : (o.res_buf != UDP_BUF_NONE || o.kind == UDP_OP_PRM_DW9) && !buf_ok(o.res_buf, hw * rpitch))
      return fail(UDP_ERR_ARG, "op %d: %s: res_buf", idx, what);
    if (o.kind == UDP_OP_SE_RES) {
      if (o.in_buf == o.out_buf && (o.in_coff != o.out_coff || ipitch != (o.out_pitch ? o.out_pitch : o.cout)))
        return fail(UDP_ERR_ARG, "op %d: se + residual in place needs the same view for in and out", idx);
      if (o.res_buf == o.out_buf || o.res_buf == o.in_buf) return fail(UDP_ERR_ARG, "op %d: se + residual: res must not be in or out", idx);
    } else if (o.in_buf == o.out_buf || o.res_buf == o.out_buf) {
      return fail(UDP_ERR_ARG, "op %d: %s: out must not be in or res", idx, what);
    }
    if (o.kind == UDP_OP_PRM_DW9 && (!buf_ok(o.up_buf[0], rows) || o.up_buf[0] == o.out_buf))
      return fail(UDP_ERR_ARG, "op %d: prm spatial gate: up_buf[0] (the channel gate's rows) missing, too small or the output", idx);
    const size_t C = (size_t)o.cin;
    const size_t wbytes = (o.kind == UDP_OP_SE_RES ? 2 * C * o.chain_cout : o.kind == UDP_OP_PRM_GATE ? 2 * C * C + 2 * C : 81 * C) * 4;
    if (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15) ||
        (o.kind == UDP_OP_PRM_DW9 && (o.b_off < 0 || (size_t)o.b_off + C * 4 > h->weights_bytes || (o.b_off & 15))))
      return fail(UDP_ERR_ARG, "op %d: %s parameter block outside the blob or misaligned", idx, what);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_GNORM || o.kind == UDP_OP_LINATTN) {
    // GroupNorm(1, C) / the separable self-attention core (attn.hip); the norm's `out` may be the very view `in` is
    const bool gn = o.kind == UDP_OP_GNORM;
    const int rc = gn ? gnorm_validate(o, h->dtype) : linattn_validate(o, h->dtype);
    if (rc) return rc;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.res_buf != UDP_BUF_NONE)
      return fail(UDP_ERR_ARG, "op %d: %s buffers missing or too small (or a residual)", idx, gn ? "group norm" : "linear attention");
    if (o.in_buf == o.out_buf && (!gn || o.in_coff != o.out_coff || ipitch != (o.out_pitch ? o.out_pitch : o.cout)))
      return fail(UDP_ERR_ARG, "op %d: %s", idx, gn ? "group norm in place needs the same view for in and out" : "linear attention: out must not be in");
    if (gn && (o.w_off < 0 || (size_t)o.w_off + (size_t)2 * o.cin * 4 > h->weights_bytes || (o.w_off & 15)))
      return fail(UDP_ERR_ARG, "op %d: group norm parameter block outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_LNORM || o.kind == UDP_OP_MHATTN || o.kind == UDP_OP_ACT) {
    // LayerNorm per pixel / soft-max multi-head attention / the stand-alone activation (attn.hip); the norm's and the
    // activation's `out` may be the very view `in` is
    const char* what = o.kind == UDP_OP_LNORM ? "layer norm" : o.kind == UDP_OP_MHATTN ? "multi-head attention" : "activation op";
    const int rc = o.kind == UDP_OP_LNORM ? lnorm_validate(o, h->dtype) : o.kind == UDP_OP_MHATTN ? mhattn_validate(o, h->dtype) : act_op_validate(o, h->dtype);
    if (rc) return rc;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.res_buf != UDP_BUF_NONE)
      return fail(UDP_ERR_ARG, "op %d: %s buffers missing or too small (or a residual)", idx, what);
    if (o.in_buf == o.out_buf && (o.kind == UDP_OP_MHATTN || o.in_coff != o.out_coff || ipitch != (o.out_pitch ? o.out_pitch : o.cout)))
      return fail(UDP_ERR_ARG, "op %d: %s: %s", idx, what, o.kind == UDP_OP_MHATTN ? "out must not be in" : "in place needs the same view for in and out");
    if (o.kind == UDP_OP_LNORM && (o.w_off < 0 || (size_t)o.w_off + (size_t)2 * o.cin * 4 > h->weights_bytes || (o.w_off & 15)))
      return fail(UDP_ERR_ARG, "op %d: layer norm parameter block outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind == UDP_OP_DWCONV || o.kind == UDP_OP_PIXSHUF) {
    // depthwise conv + folded BatchNorm (+ the ShuffleV2 passthrough) / PixelShuffle(2) (dwconv.hip)
    const bool dw = o.kind == UDP_OP_DWCONV;
    const int rc = dw ? dwconv_validate(o, h->dtype) : pixshuf_validate(o, h->dtype);
    if (rc) return rc;
    const int ipitch = o.in_pitch ? o.in_pitch : o.cin;
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch) || !buf_ok(o.out_buf, out_need) || o.in_buf == o.out_buf)
      return fail(UDP_ERR_ARG, "op %d: %s buffers missing, too small or aliased", idx, dw ? "depthwise conv" : "pixel shuffle");
    if (dw && o.n_out2) {
      const int64_t hw = (int64_t)o.hout * o.wout;
      const int d = o.out2_buf[0];
      if (!buf_ok(o.res_buf, hw * o.res_pitch) || !buf_ok(d, hw * o.out2_pitch[0]) || d == o.in_buf || d == o.out_buf || d == o.res_buf)
        return fail(UDP_ERR_ARG, "op %d: depthwise conv: passthrough buffers missing, too small or aliased", idx);
    } else if (o.res_buf != UDP_BUF_NONE) {
      return fail(UDP_ERR_UNSUPPORTED, "op %d: %s takes no residual", idx, dw ? "depthwise conv" : "pixel shuffle");
    }
    if (dw && (o.w_off < 0 || (size_t)o.w_off + (size_t)o.ks * o.ks * o.cin * 4 > h->weights_bytes || (o.w_off & 15) || o.b_off < 0 ||
               (size_t)o.b_off + (size_t)o.cin * 4 > h->weights_bytes || (o.b_off & 15)))
      return fail(UDP_ERR_ARG, "op %d: depthwise conv weight / bias range outside the blob or misaligned", idx);
    return UDP_OK;
  }
  if (o.kind >= UDP_OP_PSA_POOL) {
    // polarized self-attention ops: per-image side buffers hold fp32 rows, counted in `dtype` elements
    const int64_t f = 4 / (int64_t)esize(h->dtype);
    const int64_t hw = (int64_t)o.hin * o.win;
    const int C = o.kind == UDP_OP_PSA_SP ? o.cout : o.cin;
    if (C <= 0 || hw <= 0 || C % 16) return fail(UDP_ERR_ARG, "op %d: PSA shape", idx);
    const size_t wbytes = (size_t)(C + (C / 2) * C + (C / 8) * (C / 2) + 3 * (C / 8) + C * (C / 8) + C + (C / 2) * C) * 4;
    bool ok = true;
    switch (o.kind) {
      case UDP_OP_PSA_POOL: ok = buf_ok(o.in_buf, hw * C) && buf_ok(o.out_buf, 2 * C * f); break;
      case UDP_OP_PSA_MLP: ok = buf_ok(o.in_buf, 2 * C * f) && buf_ok(o.out_buf, (C + C / 2) * f); break;
      case UDP_OP_PSA_SCALE: ok = buf_ok(o.in_buf, hw * C) && buf_ok(o.res_buf, (C + C / 2) * f) && buf_ok(o.out_buf, hw * C); break;
      default: ok = buf_ok(o.in_buf, hw * (C / 2)) && buf_ok(o.res_buf, hw * C) && o.n_up == 1 && buf_ok(o.up_buf[0], (C + C / 2) * f) && buf_ok(o.out_buf, hw * C);
    }
    if (!ok) return fail(UDP_ERR_ARG, "op %d: PSA buffers missing or too small", idx);
    if (o.kind <= UDP_OP_PSA_MLP && (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15)))
      return fail(UDP_ERR_ARG, "op %d: PSA parameter block outside the blob or misaligned", idx);
    return UDP_OK;
  }
  const bool is_stem = o.kind == UDP_OP_STEM || o.kind == UDP_OP_STEM7;
  const bool has_w = is_stem || o.kind == UDP_OP_CONV;
  const int ipitch = o.in_pitch ? o.in_pitch : o.cin, opitch = o.out_pitch ? o.out_pitch : o.cout;
  const int rpitch = o.res_pitch ? o.res_pitch : o.cout;
  if (o.in_coff < 0 || o.out_coff < 0 || o.res_coff < 0 || o.in_coff + o.cin > ipitch || o.out_coff + o.cout > opitch ||
      o.res_coff + o.cout > rpitch)
    return fail(UDP_ERR_ARG, "op %d: channel view outside its tensor", idx);
  if (o.cout <= 0 || o.hout <= 0 || o.wout <= 0 || o.cout_pad < o.cout || o.cout_pad % 32)
    return fail(UDP_ERR_ARG, "op %d: bad output shape / cout_pad", idx);
  if (o.out_buf == UDP_BUF_OUTPUT) {
    if (o.kind != UDP_OP_CONV || o.cout != h->out_channels || o.hout * 4 != h->in_h || o.wout * 4 != h->in_w)
      return fail(UDP_ERR_ARG, "op %d: output op must be a conv producing [C=%d,%d,%d]", idx, h->out_channels,
                  h->in_h / 4, h->in_w / 4);
    if (o.res_buf != UDP_BUF_NONE || o.n_up != 0) return fail(UDP_ERR_ARG, "op %d: output op takes no addends", idx);
  } else if (o.out_buf == UDP_BUF_NONE && o.n_out2 > 0 && o.kind == UDP_OP_CONV) {
    // only the second outputs are wanted (nothing reads the plain conv output): its stores are dropped
  } else if (!buf_ok(o.out_buf, out_need)) {
    return fail(UDP_ERR_ARG, "op %d: out_buf %d missing or too small", idx, o.out_buf);
  }
  if (is_stem) {
    const int want = o.kind == UDP_OP_STEM ? 3 : 7;
    if (o.ks != want || o.stride != 2 || o.cin != 3 || o.hin != h->in_h || o.win != h->in_w)
      return fail(UDP_ERR_ARG, "op %d: stem must be %dx%d s2 on the %dx%d input", idx, want, want, h->in_h, h->in_w);
  } else {
    if (!buf_ok(o.in_buf, (int64_t)o.hin * o.win * ipitch)) return fail(UDP_ERR_ARG, "op %d: in_buf %d missing or too small", idx, o.in_buf);
    if (o.in_buf == o.out_buf && o.kind == UDP_OP_CONV && o.ks != 1) return fail(UDP_ERR_ARG, "op %d: in-place 3x3 conv is not supported", idx);
  }
  if (o.kind == UDP_OP_MAXPOOL) {
    if (o.cin != o.cout || o.hout != (o.hin + 2 - 3) / 2 + 1 || o.wout != (o.win + 2 - 3) / 2 + 1)
      return fail(UDP_ERR_ARG, "op %d: maxpool 3x3 s2 p1 shape", idx);
  } else if (o.kind == UDP_OP_BILINEAR) {
    if (o.cin != o.cout) return fail(UDP_ERR_ARG, "op %d: bilinear resize keeps the channel count", idx);
  } else if (has_w) {
    if ((o.ks != 1 && o.ks != 3 && o.ks != 7) || (o.stride != 1 && o.stride != 2)) return fail(UDP_ERR_ARG, "op %d: ks/stride", idx);
    const int pad = o.ks / 2;
    if (o.hout != (o.hin + 2 * pad - o.ks) / o.stride + 1 || o.wout != (o.win + 2 * pad - o.ks) / o.stride + 1)
      return fail(UDP_ERR_ARG, "op %d: output size does not match input/stride", idx);
    if (o.wfmt != 0 && (o.wfmt != 1 || is_stem || h->dtype != UDP_F16X2))
      return fail(UDP_ERR_ARG, "op %d: wfmt %d (fragment-major weights need a UDP_F16X2 UDP_OP_CONV)", idx, o.wfmt);
    const size_t wbytes = is_stem ? (size_t)o.ks * o.ks * 3 * o.cout * 4
                          : o.wfmt == 1 ? (size_t)o.ks * o.ks * ((o.cin + 31) / 32) * (o.cout_pad / 32) * 4096
                                        : (size_t)o.ks * o.ks * o.cout_pad * o.cin * esize(h->dtype);
    if (o.w_off < 0 || (size_t)o.w_off + wbytes > h->weights_bytes || (o.w_off & 15))
      return fail(UDP_ERR_ARG, "op %d: weight range outside the blob or misaligned", idx);
    if (o.b_off < 0 || (size_t)o.b_off + (size_t)o.cout_pad * 4 > h->weights_bytes || (o.b_off & 15))
      return fail(UDP_ERR_ARG, "op %d: bias range outside the blob or misaligned", idx);
  } else if (o.hin != o.hout || o.win != o.wout || o.cin != o.cout) {
    return fail(UDP_ERR_ARG, "op %d: fuse op must keep the shape", idx);
  }
  if (o.lane < 0 || o.lane >= UDP_MAX_LANES || o.n_wait < 0 || o.n_wait > UDP_MAX_WAIT) return fail(UDP_ERR_ARG, "op %d: lane/n_wait", idx);
  for (int k = 0; k < o.n_wait; ++k)
    if (o.wait_op[k] < 0 || o.wait_op[k] >= idx) return fail(UDP_ERR_ARG, "op %d: wait_op %d must name an earlier op", idx, o.wait_op[k]);
  if (o.res_buf != UDP_BUF_NONE && !buf_ok(o.res_buf, (int64_t)o.hout * o.wout * rpitch)) return fail(UDP_ERR_ARG, "op %d: res_buf", idx);
  if (o.n_up < 0 || o.n_up > 3) return fail(UDP_ERR_ARG, "op %d: n_up", idx);
  for (int u = 0; u < o.n_up; ++u) {
    const int s = o.up_shift[u];
    if (s < 1 || s > 5 || (o.hout & ((1 << s) - 1)) || (o.wout & ((1 << s) - 1)))
      return fail(UDP_ERR_ARG, "op %d: up_shift %d does not divide %dx%d", idx, s, o.hout, o.wout);
    if (!buf_ok(o.up_buf[u], (int64_t)(o.hout >> s) * (o.wout >> s) * o.cout)) return fail(UDP_ERR_ARG, "op %d: up_buf %d", idx, u);
  }
  if (o.kind == UDP_OP_CONV && o.ks == 7) {
    // conv7.hip: a plain conv + bias (+ ReLU) over channel views; what it does not do is refused here, not ignored
    if (h->dtype == UDP_BF16 || o.stride != 1 || o.wfmt != 0 || o.res_buf != UDP_BUF_NONE || o.n_up || o.n_out2 || o.chain_cout || o.group ||
        o.in_stuff2 || o.out_buf == UDP_BUF_OUTPUT || o.relu > UDP_ACT_RELU || o.cin % 16 || o.cout % 16)
      return fail(UDP_ERR_UNSUPPORTED, "op %d: a 7x7 conv is stride 1, f32 / f16x2, wfmt 0, cin and cout multiples of 16, NHWC, bias (+ ReLU) only: "
                  "no residual, addends, second outputs, chain, group or stuffed input", idx);
  }
  if (o.chain_cout) {
    if (o.kind != UDP_OP_CONV || o.wfmt != 1 || h->dtype != UDP_F16X2 || o.ks != 1 || o.stride != 1 || o.group || o.n_up || o.n_out2 ||
        o.out_buf < 0 || (o.cin != 64 && o.cin != 128) || o.cout != 256 || o.cout_pad != o.cout || o.chain_cout != 64)
      return fail(UDP_ERR_UNSUPPORTED, "op %d: a chained conv needs an ungrouped split-fp16 1x1 conv (wfmt 1), 64 | 128 -> 256 channels, and 64 chained outputs", idx);
    if (!buf_ok(o.chain_buf, (int64_t)o.hout * o.wout * o.chain_cout) || o.chain_buf == o.out_buf || o.chain_buf == o.in_buf || o.chain_buf == o.res_buf)
      return fail(UDP_ERR_ARG, "op %d: chain_buf %d missing, too small or aliased", idx, o.chain_buf);
    const size_t w2bytes = (size_t)(o.cout / 32) * (o.chain_cout / 32) * 4096;
    if (o.w2_off < 0 || (size_t)o.w2_off + w2bytes > h->weights_bytes || (o.w2_off & 15) || o.b2_off < 0 ||
        (size_t)o.b2_off + (size_t)o.chain_cout * 4 > h->weights_bytes || (o.b2_off & 15) || o.chain_wexp < -40 || o.chain_wexp > 40)
      return fail(UDP_ERR_ARG, "op %d: chained conv: weight / bias range outside the blob or misaligned", idx);
  }
  if (o.n_out2 < 0 || o.n_out2 > 2) return fail(UDP_ERR_ARG, "op %d: n_out2", idx);
  if (o.n_out2 && (o.kind != UDP_OP_CONV || o.wfmt != 1 || h->dtype != UDP_F16X2 || o.out_buf == UDP_BUF_OUTPUT || o.cout % 8 || o.ks != 3 || o.stride != 1 || o.group))
    return fail(UDP_ERR_UNSUPPORTED, "op %d: second outputs need an ungrouped 3x3 stride-1 split-fp16 conv with fragment-major weights, an NHWC output and cout %% 8 == 0", idx);
  for (int k = 0; k < o.n_out2; ++k) {
    const int op = o.out2_pitch[k] ? o.out2_pitch[k] : o.cout, ap = o.add2_pitch[k] ? o.add2_pitch[k] : o.cout;
    if (o.out2_coff[k] < 0 || o.out2_coff[k] + o.cout > op || o.add2_coff[k] < 0 || o.add2_coff[k] + o.cout > ap ||
        (o.out2_coff[k] | o.add2_coff[k] | op | ap) % 8)
      return fail(UDP_ERR_ARG, "op %d: second output %d: channel views", idx, k);
    if (!buf_ok(o.out2_buf[k], (int64_t)o.hout * o.wout * op) || !buf_ok(o.add2_buf[k], (int64_t)o.hout * o.wout * ap))
      return fail(UDP_ERR_ARG, "op %d: second output %d: buffers", idx, k);
  }
  return UDP_OK;
}

extern "C" int udp_abi_version(void) { return UDP_POSE_ABI_VERSION; }
extern "C" const char* udp_last_error(void) { return err_buf(); }

extern "C" int udp_f16x2_overflow(void* stream, int reset) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int flag = 0;
  int rc = conv_h2_overflow(s, reset, &flag);
  if (!rc) rc = conv7_h2_overflow(s, reset, &flag);
  if (!rc) rc = conv_ws_h2_overflow(s, reset, &flag);
  if (!rc) rc = psa_h2_overflow(s, reset, &flag);
  if (!rc) rc = deconv_h2_overflow(s, reset, &flag);
  if (!rc) rc = dwconv_h2_overflow(s, reset, &flag);
  if (!rc) rc = attn_h2_overflow(s, reset, &flag);
  if (!rc) rc = rsn_gate_h2_overflow(s, reset, &flag);
  return rc ? rc : flag;
}

extern "C" int udp_hrnet_create(const udp_conv_op* ops, int n_ops, const int64_t* buf_elems, int n_bufs,
                                const void* weights_dev, size_t weights_bytes, int dtype, int in_h, int in_w,
                                int out_channels, udp_hrnet** out) {
  if (!ops || n_ops <= 0 || !buf_elems || n_bufs <= 0 || !weights_dev || !out)
    return fail(UDP_ERR_ARG, "udp_hrnet_create: null/empty argument");
  if (dtype != UDP_F32 && dtype != UDP_BF16 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "udp_hrnet_create: dtype %d", dtype);
  if (in_h <= 0 || in_w <= 0 || (in_h % 32) || (in_w % 32))
    return fail(UDP_ERR_UNSUPPORTED, "udp_hrnet_create: input %dx%d must be a multiple of 32", in_h, in_w);
  if (reinterpret_cast<uintptr_t>(weights_dev) & 15) return fail(UDP_ERR_ARG, "udp_hrnet_create: weights not 16-byte aligned");
  udp_hrnet* h = new udp_hrnet();
  h->dtype = dtype;
  h->in_h = in_h;
  h->in_w = in_w;
  h->out_channels = out_channels;
  h->weights = reinterpret_cast<const char*>(weights_dev);
  h->weights_bytes = weights_bytes;
  h->buf_off.resize(n_bufs);
  for (int b = 0; b < n_bufs; ++b) {
    if (buf_elems[b] <= 0) {
      delete h;
      return fail(UDP_ERR_ARG, "udp_hrnet_create: buffer %d has %lld elements", b, (long long)buf_elems[b]);
    }
    const int64_t e = (buf_elems[b] + 63) / 64 * 64;
    h->buf_elems.push_back(e);
    h->buf_off[b] = h->total_elems;
    h->total_elems += e;
  }
  bool has_out = false;
  for (int i = 0; i < n_ops; ++i) {
    const int rc = validate_op(h, ops[i], i);
    if (rc) {
      delete h;
      return rc;
    }
    has_out |= ops[i].out_buf == UDP_BUF_OUTPUT;
    if (ops[i].kind == UDP_OP_STEM || ops[i].kind == UDP_OP_STEM7 || ops[i].kind == UDP_OP_CONV)
      h->flops += 2.0 * ops[i].ks * ops[i].ks * ops[i].cin * ops[i].cout * ops[i].hout * ops[i].wout;
    if (ops[i].kind == UDP_OP_BLOCK) h->flops += 2 * 2.0 * 9 * 32 * 32 * ops[i].hout * ops[i].wout;
    if (ops[i].kind == UDP_OP_DECONV) h->flops += 2.0 * 4 * ops[i].cin * ops[i].cout * ops[i].hout * ops[i].wout;   // 2x2 taps per output pixel
    if (ops[i].kind == UDP_OP_DWCONV) h->flops += 2.0 * ops[i].ks * ops[i].ks * ops[i].cout * ops[i].hout * ops[i].wout;   // ks * ks MACs per output element
    if (ops[i].kind == UDP_OP_SE) h->flops += 2.0 * 2 * ops[i].cin * ops[i].chain_cout;   // the two small products (pool and scale are not counted)
    if (ops[i].kind == UDP_OP_SE_RES) h->flops += 2.0 * 2 * ops[i].cin * ops[i].chain_cout;   // as UDP_OP_SE
    if (ops[i].kind == UDP_OP_SE_ACT) h->flops += 2.0 * 2 * ops[i].cin * ops[i].chain_cout;   // as UDP_OP_SE (activation, biases, pool and scale are not counted)
    if (ops[i].kind == UDP_OP_PRM_GATE) h->flops += 2.0 * 2 * ops[i].cin * ops[i].cin;
    if (ops[i].kind == UDP_OP_PRM_DW9) h->flops += 2.0 * 81 * ops[i].cout * ops[i].hout * ops[i].wout;   // the taps (the gate's epilogue is not counted)
    if (ops[i].kind == UDP_OP_LINATTN) h->flops += 2.0 * ops[i].cout * ops[i].hout * ops[i].wout;   // the weighted sum of the keys (soft-max and gate are not counted)
    if (ops[i].kind == UDP_OP_MHATTN)      // q k^T and the weighted sum of the values: 2 d N MACs per pixel, N = HW / 4 keys
      h->flops += 2.0 * 2 * ops[i].chain_cout * (ops[i].hout * ops[i].wout / 4) * ops[i].hout * ops[i].wout;
    if (ops[i].kind == UDP_OP_CONV && ops[i].chain_cout) h->flops += 2.0 * ops[i].cout * ops[i].chain_cout * ops[i].hout * ops[i].wout;
    h->ops.push_back(ops[i]);
  }
  if (!has_out || (h->ops[0].kind != UDP_OP_STEM && h->ops[0].kind != UDP_OP_STEM7) || h->ops[0].lane != 0 || h->ops.back().lane != 0 ||
      h->ops.back().out_buf != UDP_BUF_OUTPUT) {
    delete h;
    return fail(UDP_ERR_ARG, "udp_hrnet_create: program needs a stem op first and the output op last, both on lane 0");
  }
  // the weight-stationary split-fp16 kernels (fragment-major weights) are the output writers that place rows (out_skip)
  h->out_in_place = dtype == UDP_F16X2;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i].out_buf == UDP_BUF_OUTPUT && (ops[i].kind != UDP_OP_CONV || ops[i].wfmt != 1)) h->out_in_place = false;
  h->op_signals.assign(n_ops, 0);
  for (int i = 0; i < n_ops; ++i) {
    if (ops[i].lane + 1 > h->n_lanes) h->n_lanes = ops[i].lane + 1;
    for (int k = 0; k < ops[i].n_wait; ++k) h->op_signals[ops[i].wait_op[k]] = 1;
  }
  h->op_done.assign(n_ops, nullptr);
  hipError_t e = hipSuccess;
  for (int l = 1; l < h->n_lanes && e == hipSuccess; ++l) e = hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking);
  for (int l = 1; l < h->n_lanes && e == hipSuccess; ++l) e = hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
  for (int i = 0; i < n_ops && e == hipSuccess; ++i)
    if (h->op_signals[i]) e = hipEventCreateWithFlags(&h->op_done[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    udp_hrnet_destroy(h);
    return fail(UDP_ERR_HIP, "udp_hrnet_create: stream/event creation failed: %s", hipGetErrorString(e));
  }
  *out = h;
  return UDP_OK;
}

static size_t ws_bytes_one(const udp_hrnet* h, int n, int flip) {
  const size_t b = (size_t)h->total_elems * (size_t)(n * (flip ? 2 : 1)) * esize(h->dtype);
  return (b + 255) & ~(size_t)255;
}
static size_t out_bytes(const udp_hrnet* h, int images) {
  return (size_t)images * h->out_channels * (size_t)(h->in_h / 4) * (size_t)(h->in_w / 4) * sizeof(float);
}
// Sub-batch lanes: a batch of the split-fp16 mode is run as two halves, each its own hipGraph, the second on an
// internal stream BESIDE the first (fork / join by events on the caller's stream).  Measured with two independent
// graph replays on two streams (tools/dual_stream.py, 64 crops + mirrored copies): W32 256x192 7.39 -> 7.81-7.92 k
// images/s, RSN-18 9.67 -> 10.93 k, W48 384x288 1.55 -> 1.53 k; four lanes: 4.5 k.  The launches of one chain leave
// the chip idle between a kernel's last workgroups and its successor's first HBM round trip (42 % of the workgroup
// slot time of the dominant launch is outside its MFMA loop, NOTES.md); a second, independent chain fills those gaps.
// Images are independent (same result for an image whatever batch it arrives in -- tests/test_gpu_e2e.py), so the
// split changes no number.  Default: split-fp16 and bf16 modes (bf16: 13.2 -> 14.3 k), inputs up to 256x192, 16 crops
// or more; UDP_POSE_LANES=1 / 2 forces it off / on.
static bool split_ok(const udp_hrnet* h, int n) {
  if (n < 16) return false;
  const char* e = getenv("UDP_POSE_LANES");
  if (e) return atoi(e) >= 2;
  return h->dtype != UDP_F32 && (long)h->in_h * h->in_w <= 256L * 192L;   // (fp32 mode: 2.86 -> 2.70 k with two lanes)
}
extern "C" int udp_hrnet_lanes(const udp_hrnet* h, int n) { return h && n > 0 && split_ok(h, n) ? 2 : 1; }
extern "C" size_t udp_hrnet_workspace_bytes(const udp_hrnet* h, int n, int flip_test) {
  if (!h || n <= 0) return 0;
  if (!split_ok(h, n)) return ws_bytes_one(h, n, flip_test);
  const int n0 = (n + 1) / 2;
  // two lanes' workspaces + (flip test) their [normal | mirrored] heat-maps before they are copied into place
  return ws_bytes_one(h, n0, flip_test) + ws_bytes_one(h, n - n0, flip_test) + (flip_test ? out_bytes(h, 2 * n) + 512 : 0);
}

extern "C" int udp_hrnet_num_launches(const udp_hrnet* h) { return h ? (int)h->ops.size() : 0; }
extern "C" double udp_hrnet_flops_per_image(const udp_hrnet* h) { return h ? h->flops : 0.0; }

// Resolves buffers / weights of every op for this call and picks kernels + tiles.
// Chained head (conv_ws.hip, conv_head_chain_kernel): op i = a split-fp16 1x1 conv with ReLU (and up-sampled addends)
// into a dense NHWC buffer that ONLY op i + 1 reads, op i + 1 = the plain 1x1 conv that writes the net's output.  Then
// L[i] becomes the one launch of both and the buffer is never written.  UDP_POSE_NO_HEAD_CHAIN=1 keeps the two launches
// (read per describe, so that handles created after a change see it); every program whose tail does not match --
// W48, 16-channel branches, the LDS-staged head (wfmt 0), bf16 / fp32 -- keeps them too.
static int mark_head_chain(const udp_hrnet* h, std::vector<Launch>& L) {
  const char* off = getenv("UDP_POSE_NO_HEAD_CHAIN");
  if (h->dtype != UDP_F16X2 || (off && atoi(off) != 0)) return UDP_OK;
  for (size_t i = 0; i + 1 < h->ops.size(); ++i) {
    const udp_conv_op& a = h->ops[i];
    const udp_conv_op& b = h->ops[i + 1];
    if (a.kind != UDP_OP_CONV || a.ks != 1 || a.stride != 1 || a.wfmt != 1 || a.relu != UDP_ACT_RELU || a.cin % 32 || a.out_buf < 0 ||
        a.out_coff || (a.out_pitch && a.out_pitch != a.cout) || a.res_buf != UDP_BUF_NONE || a.n_out2 || a.chain_cout || a.group || a.in_stuff2)
      continue;
    if (b.kind != UDP_OP_CONV || b.ks != 1 || b.stride != 1 || b.wfmt != 1 || b.out_buf != UDP_BUF_OUTPUT || b.res_buf != UDP_BUF_NONE ||
        b.n_up || b.relu || b.n_out2 || b.chain_cout || b.group || b.in_stuff2 || b.in_buf != a.out_buf || b.in_coff ||
        (b.in_pitch && b.in_pitch != a.cout) || b.cin != a.cout || b.lane != a.lane)
      continue;
    // nobody else reads the intermediate map (any later mention of the buffer counts, whatever is written in between)
    bool shared = false;
    for (size_t k = i + 2; k < h->ops.size() && !shared; ++k) {
      const udp_conv_op& o = h->ops[k];
      shared = o.in_buf == a.out_buf || o.res_buf == a.out_buf || (o.chain_cout && o.chain_buf == a.out_buf);
      for (int u = 0; u < o.n_up && u < 3; ++u) shared |= o.up_buf[u] == a.out_buf;
      for (int u = 0; u < o.n_out2 && u < 2; ++u) shared |= o.add2_buf[u] == a.out_buf || o.out2_buf[u] == a.out_buf;
    }
    if (shared) continue;
    Launch fused;
    const int rc = describe_head_chain(L[i].p, L[i + 1].p, &fused);
    if (rc == 1) continue;       // no instantiation for these widths
    if (rc) return rc;
    fused.pair = 1;
    L[i] = fused;
    ++i;
  }
  return UDP_OK;
}

// Shared-input sets of an exchange unit (conv_ws.hip, conv_ws_s2x_kernel).  The branch-0 map of a unit is read in full
// by its element-wise output 0 (UDP_OP_FUSE) and by the first stride-2 conv of every chain that leaves branch 0
// (fuse_layers.i.0.0): one launch at the position of the EARLIEST of them stages each tile once and does the work of
// all.  A set = 1..3 UDP_OP_CONVs (3x3, stride 2, 32 input channels, fragment-major weights, NHWC output, no chain /
// second outputs / group; <= 4 cout pairs in all) over one input view, and at most one UDP_OP_FUSE of 32 channels over
// that view; two members at least.
//
// A later member runs earlier than the planner placed it, and the planner gave it buffers by lifetime at its own index
// (program.py, _assign_buffers), so every candidate k is checked on the buffer ids (and channel slices), against the launch position e:
//   * an op strictly between e and k that is not a member touches none of k's outputs and writes none of k's inputs
//     (input, residual, addends),
//   * no buffer k writes is read or written by another member, and no member writes what k reads (they run side by
//     side in one launch),
//   * k waits for nothing that comes after e.
// A candidate that fails is left out; it keeps its own launch.
// Lanes: the planner puts an op on the lane of its output's resolution, so the sum and the convs of a set sit on
// different lanes, and a lane orders its own ops without listing them as waits.  A program with such a set therefore
// runs as ONE chain in program order, as a program with merged launch groups does (make_nodes, `grouped`) -- the
// grouped split-fp16 programs are one chain already; members of one lane keep the lanes, the carrying launch then
// takes the carried ops' waits and records their signals (enqueue_all, build_graph).
struct ShareSet {
  int first = -1;            // the carrying op (earliest member)
  int fuse = -1;             // the UDP_OP_FUSE member, or -1
  int conv[kShareRoutes];    // the conv members, in program order
  int n = 0;
};
// Channel slice [lo, hi) of the buffer's pixels of `pitch` channels; pitch 0: the whole buffer (addends, and every
// operand of the op kinds whose fields are not plain channel views).  Slices of one buffer with one pitch and disjoint
// channel ranges share no byte, whatever the map sizes are (a concat tensor written in slices, hrnet_plan.py `cat`).
struct BufView {
  int buf, lo, hi, pitch;
};
static bool views_meet(const BufView& a, const BufView& b) {
  return a.buf == b.buf && (a.pitch == 0 || a.pitch != b.pitch || (a.lo < b.hi && b.lo < a.hi));
}
static void op_views(const udp_conv_op& o, std::vector<BufView>& reads, std::vector<BufView>& writes) {
  reads.clear();
  writes.clear();
  const bool plain = o.kind == UDP_OP_CONV || o.kind == UDP_OP_FUSE;
  auto put = [&](std::vector<BufView>& v, int b, int coff, int c, int pitch) {
    if (b >= 0) v.push_back(plain ? BufView{b, coff, coff + c, pitch ? pitch : c} : BufView{b, 0, 0, 0});
  };
  put(reads, o.in_buf, o.in_coff, o.cin, o.in_pitch);
  put(reads, o.res_buf, o.res_coff, o.cout, o.res_pitch);
  for (int u = 0; u < o.n_up && u < 3; ++u) reads.push_back(BufView{o.up_buf[u], 0, 0, 0});
  for (int u = 0; u < o.n_out2 && u < 2; ++u) put(reads, o.add2_buf[u], o.add2_coff[u], o.cout, o.add2_pitch[u]);
  put(writes, o.out_buf, o.out_coff, o.cout, o.out_pitch);
  for (int u = 0; u < o.n_out2 && u < 2; ++u) put(writes, o.out2_buf[u], o.out2_coff[u], o.cout, o.out2_pitch[u]);
  if (o.chain_cout && o.chain_buf >= 0) writes.push_back(BufView{o.chain_buf, 0, 0, 0});
}
static bool meet(const std::vector<BufView>& a, const std::vector<BufView>& b) {
  for (const BufView& x : a)
    for (const BufView& y : b)
      if (views_meet(x, y)) return true;
  return false;
}
static bool meet2(const std::vector<BufView>& a, const std::vector<BufView>& b, const std::vector<BufView>& c) { return meet(a, b) || meet(a, c); }
static std::vector<ShareSet> find_share_sets(const std::vector<udp_conv_op>& ops) {
  auto conv_ok = [](const udp_conv_op& o) {
    return o.kind == UDP_OP_CONV && o.ks == 3 && o.stride == 2 && o.cin == 32 && o.wfmt == 1 && !o.chain_cout && !o.n_out2 && !o.in_stuff2 &&
           !o.group && o.in_buf >= 0 && o.out_buf >= 0 && o.cout_pad >= 32 && o.cout_pad % 32 == 0 && o.cout_pad <= 128 && o.relu <= UDP_ACT_RELU;
  };
  auto fuse_ok = [](const udp_conv_op& o) {
    return o.kind == UDP_OP_FUSE && o.cin == 32 && o.cout == 32 && o.res_buf == UDP_BUF_NONE && o.in_buf >= 0 && o.out_buf >= 0 && o.relu <= UDP_ACT_RELU;
  };
  auto same_view = [](const udp_conv_op& a, const udp_conv_op& b) {
    return a.in_buf == b.in_buf && a.in_coff == b.in_coff && (a.in_pitch ? a.in_pitch : a.cin) == (b.in_pitch ? b.in_pitch : b.cin) &&
           a.hin == b.hin && a.win == b.win;
  };
  const int n_ops = (int)ops.size();
  std::vector<char> used(ops.size(), 0);
  std::vector<ShareSet> sets;
  std::vector<BufView> rk, wk, ro, wo;
  for (int e = 0; e < n_ops; ++e) {
    if (used[e] || !(conv_ok(ops[e]) || fuse_ok(ops[e]))) continue;
    ShareSet s;
    s.first = e;
    int pairs = 0;
    std::vector<int> members;
    auto take = [&](int k) {
      if (ops[k].kind == UDP_OP_FUSE) {
        s.fuse = k;
      } else {
        s.conv[s.n++] = k;
        pairs += ops[k].cout_pad / 32;
      }
      members.push_back(k);
    };
    take(e);
    for (int k = e + 1; k < n_ops; ++k) {
      const udp_conv_op& c = ops[k];
      op_views(c, rk, wk);
      op_views(ops[e], ro, wo);
      if (meet(wk, std::vector<BufView>(1, ro[0]))) break;   // the view holds another tensor from here on
      if (used[k] || !same_view(c, ops[e])) continue;
      if (fuse_ok(c) ? s.fuse >= 0 : !conv_ok(c) || s.n == kShareRoutes || pairs + c.cout_pad / 32 > 4) continue;
      bool ok = true;
      for (int w = 0; w < c.n_wait && ok; ++w) ok = c.wait_op[w] < e;
      // (one rule for both kinds of op in [e, k): a member there runs beside k, any other op now runs after k)
      for (int i = e; i < k && ok; ++i) {
        op_views(ops[i], ro, wo);
        ok = !meet2(wk, ro, wo) && !meet(wo, rk);
      }
      if (ok) take(k);
    }
    if (members.size() < 2 || s.n < 1) continue;
    for (int k : members) used[k] = 1;
    sets.push_back(s);
  }
  return sets;
}

// Diagnostic (tests/test_x0_share_cpu.py, no GPU needed): the shared-input sets of an op list.  carrier[i] = the op whose
// launch does op i's work (i itself for the carrying op of a set), -1 for an op outside every set.  Returns the number
// of sets, or -1.
extern "C" int udp_debug_x0_share(const udp_conv_op* ops, int n_ops, int* carrier) {
  if (!ops || n_ops < 1 || !carrier) return -1;
  for (int i = 0; i < n_ops; ++i) carrier[i] = -1;
  const std::vector<ShareSet> sets = find_share_sets(std::vector<udp_conv_op>(ops, ops + n_ops));
  for (const ShareSet& s : sets) {
    if (s.fuse >= 0) carrier[s.fuse] = s.first;
    for (int j = 0; j < s.n; ++j) carrier[s.conv[j]] = s.first;
  }
  return (int)sets.size();
}

// UDP_POSE_NO_X0_SHARE=1 keeps every member's own launch (read per describe, as UDP_POSE_NO_HEAD_CHAIN is).
static int mark_x0_share(const udp_hrnet* h, std::vector<Launch>& L) {
  const char* off = getenv("UDP_POSE_NO_X0_SHARE");
  if (h->dtype != UDP_F16X2 || (off && atoi(off) != 0)) return UDP_OK;
  for (const ShareSet& s : find_share_sets(h->ops)) {
    ConvParams convs[kShareRoutes];
    char tag[96] = "ops ";
    auto name = [&](int k) { snprintf(tag + strlen(tag), sizeof(tag) - strlen(tag), "%s%d", strlen(tag) > 4 ? "+" : "", k); };
    if (s.fuse >= 0 && s.fuse < s.conv[0]) name(s.fuse);
    for (int j = 0; j < s.n; ++j) {
      convs[j] = L[s.conv[j]].p;
      name(s.conv[j]);
    }
    if (s.fuse > s.conv[0]) name(s.fuse);
    Launch fused;
    const int rc = describe_x0_share(convs, s.n, s.fuse >= 0 ? &L[s.fuse].p : nullptr, tag, &fused);
    if (rc == 1) continue;       // no kernel for this set
    if (rc) return rc;
    auto carry = [&](int k) {
      if (k < 0 || k == s.first) return;
      fused.carry[fused.n_carry++] = k;
      fused.cross_lane |= h->ops[k].lane != h->ops[s.first].lane;
      L[k] = Launch();
      L[k].carried = 1;
    };
    carry(s.fuse);
    for (int j = 0; j < s.n; ++j) carry(s.conv[j]);
    L[s.first] = fused;
  }
  return UDP_OK;
}

// out_skip: ConvParams::out_skip of the ops that write UDP_BUF_OUTPUT (0: the plain [images | mirrored] layout at `out`).
static int describe_all(const udp_hrnet* h, const float* in, int n, int flip, int out_skip, char* ws, float* out,
                        std::vector<Launch>& ls) {
  const int B = n * (flip ? 2 : 1);
  const size_t es = esize(h->dtype);
  auto buf = [&](int b) -> char* { return ws + (size_t)h->buf_off[b] * B * es; };
  ls.resize(h->ops.size());
  for (size_t i = 0; i < h->ops.size(); ++i) {
    const udp_conv_op& o = h->ops[i];
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.N = B;
    p.Hin = o.hin;
    p.Win = o.win;
    p.Cin = o.cin;
    p.Hout = o.hout;
    p.Wout = o.wout;
    p.Cout = o.cout;
    p.CoutPad = o.cout_pad;
    p.relu = o.relu;
    p.wfmt = o.wfmt;
    p.wexp = o.wexp;
    p.flip_from = flip ? n : B;
    const bool is_stem = o.kind == UDP_OP_STEM || o.kind == UDP_OP_STEM7;
    p.in_pitch = o.in_pitch ? o.in_pitch : o.cin;
    p.in_coff = o.in_coff;
    p.out_pitch = o.out_pitch ? o.out_pitch : o.cout;
    p.out_coff = o.out_coff;
    p.res_pitch = o.res_pitch ? o.res_pitch : o.cout;
    p.res_coff = o.res_coff;
    p.in = is_stem ? reinterpret_cast<const void*>(in) : buf(o.in_buf);
    p.out_nchw_f32 = o.out_buf == UDP_BUF_OUTPUT;
    p.out_skip = p.out_nchw_f32 ? out_skip : 0;     // (a writer without the field refuses a non-zero value: describe_conv)
    p.out = p.out_nchw_f32 ? reinterpret_cast<void*>(out) : o.out_buf == UDP_BUF_NONE ? nullptr : buf(o.out_buf);
    p.res = o.res_buf == UDP_BUF_NONE ? nullptr : buf(o.res_buf);
    p.nup = o.n_up;
    for (int u = 0; u < o.n_up; ++u) {
      p.up[u] = buf(o.up_buf[u]);
      p.up_shift[u] = o.up_shift[u];
    }
    p.nout2 = o.n_out2;
    for (int k = 0; k < o.n_out2; ++k) {
      p.out2[k] = buf(o.out2_buf[k]);
      p.add2[k] = o.kind == UDP_OP_DWCONV ? nullptr : buf(o.add2_buf[k]);    // (the passthrough reads `res`)
      p.out2_coff[k] = o.out2_coff[k];
      p.out2_pitch[k] = o.out2_pitch[k] ? o.out2_pitch[k] : o.cout;
      p.add2_coff[k] = o.add2_coff[k];
      p.add2_pitch[k] = o.add2_pitch[k] ? o.add2_pitch[k] : o.cout;
    }
    if (is_stem || o.kind == UDP_OP_CONV || o.kind == UDP_OP_DECONV || o.kind == UDP_OP_DWCONV || o.kind == UDP_OP_PRM_DW9) {
      p.wgt = h->weights + o.w_off;
      p.bias = reinterpret_cast<const float*>(h->weights + o.b_off);
    }
    if (o.kind == UDP_OP_CONV && o.chain_cout) {     // conv_chain_kernel's use of the addend fields (validate_op: n_up == 0)
      p.wgt2 = h->weights + o.w2_off;
      p.bias2 = reinterpret_cast<const float*>(h->weights + o.b2_off);
      p.up[0] = buf(o.chain_buf);
      p.up_shift[0] = o.chain_cout;
      p.up_shift[1] = o.chain_wexp;
      p.up_shift[2] = o.chain_relu;
    }
    if (o.kind == UDP_OP_DWCONV) p.up_shift[0] = o.chain_cout;   // passthrough: real channels per half (n_up == 0)
    if (o.kind == UDP_OP_SE || o.kind == UDP_OP_GNORM || o.kind == UDP_OP_LNORM || o.kind == UDP_OP_SE_ACT) {
      p.wgt = h->weights + o.w_off;
      p.up_shift[0] = o.chain_cout;                              // hidden width / real channels
    }
    if (o.kind == UDP_OP_MHATTN) {
      p.up_shift[0] = o.chain_cout;                              // real width d
      p.up_shift[1] = o.up_shift[0];                             // heads (mhattn_validate: n_up == 0)
    }
    if (o.kind == UDP_OP_SE_RES || o.kind == UDP_OP_PRM_GATE) {
      p.wgt = h->weights + o.w_off;
      p.up_shift[0] = o.kind == UDP_OP_SE_RES ? o.chain_cout : o.cin;      // hidden width (n_up == 0)
    }
    if (o.kind == UDP_OP_BLOCK) {
      p.wgt = h->weights + o.w_off;
      p.bias = reinterpret_cast<const float*>(h->weights + o.b_off);
      p.wgt2 = h->weights + o.w2_off;
      p.bias2 = reinterpret_cast<const float*>(h->weights + o.b2_off);
    } else if (o.kind >= UDP_OP_PSA_POOL) {
      p.wgt = h->weights + o.w_off;
      if (o.kind == UDP_OP_PSA_SCALE) p.res_pitch = o.cin + o.cin / 2;   // fp32 rows {m[C], gbar[C/2]}
    }
    int rc;
    switch (o.kind) {
      case UDP_OP_PSA_POOL:
      case UDP_OP_PSA_MLP:
      case UDP_OP_PSA_SCALE:
      case UDP_OP_PSA_SP: rc = describe_psa(p, h->dtype, o.kind, &ls[i]); break;
      case UDP_OP_BLOCK: rc = describe_block(p, h->dtype, &ls[i]); break;
      case UDP_OP_STEM: rc = describe_stem(p, h->dtype, &ls[i]); break;
      case UDP_OP_STEM7: rc = describe_stem7(p, h->dtype, &ls[i]); break;
      case UDP_OP_FUSE: rc = describe_fuse(p, h->dtype, &ls[i]); break;
      case UDP_OP_MAXPOOL: rc = describe_maxpool(p, h->dtype, &ls[i]); break;
      case UDP_OP_BILINEAR: rc = describe_bilinear(p, h->dtype, &ls[i]); break;
      case UDP_OP_DECONV: rc = describe_deconv(p, h->dtype, &ls[i]); break;
      case UDP_OP_DWCONV: rc = describe_dwconv(p, h->dtype, o.ks, o.stride, &ls[i]); break;
      case UDP_OP_SE: rc = describe_se(p, h->dtype, &ls[i]); break;
      case UDP_OP_SE_ACT: rc = describe_se_act(p, h->dtype, &ls[i]); break;
      case UDP_OP_GNORM: rc = describe_gnorm(p, h->dtype, &ls[i]); break;
      case UDP_OP_LINATTN: rc = describe_linattn(p, h->dtype, &ls[i]); break;
      case UDP_OP_LNORM: rc = describe_lnorm(p, h->dtype, &ls[i]); break;
      case UDP_OP_MHATTN: rc = describe_mhattn(p, h->dtype, &ls[i]); break;
      case UDP_OP_ACT: rc = describe_act(p, h->dtype, &ls[i]); break;
      case UDP_OP_SE_RES: rc = describe_gate(p, h->dtype, false, &ls[i]); break;
      case UDP_OP_PRM_GATE: rc = describe_gate(p, h->dtype, true, &ls[i]); break;
      case UDP_OP_PRM_DW9: rc = describe_prm_dw9(p, h->dtype, &ls[i]); break;
      case UDP_OP_PIXSHUF: rc = describe_pixshuf(p, h->dtype, &ls[i]); break;
      default:
        if (o.chain_cout) {
          rc = describe_conv_chain(p, &ls[i]);
          break;
        }
        rc = o.group != 0 && getenv("UDP_POSE_NO_GROUPS") == nullptr ? describe_conv_grouped(p, h->dtype, o.ks, o.stride, &ls[i]) : 1;
        if (rc == 1) rc = describe_conv(p, h->dtype, o.ks, o.stride, &ls[i]);
    }
    if (rc) return rc;
  }
  if (const int rc = mark_head_chain(h, ls)) return rc;
  return mark_x0_share(h, ls);
}

// Launch list: runs of groupable convs with the same group id become one conv_mfma_multi launch; a chained head pair
// (Launch::pair) is one node of two ops.
struct Node {
  size_t first;
  int n;
};
static std::vector<Node> make_nodes(const udp_hrnet* h, const std::vector<Launch>& L, bool* grouped) {
  std::vector<Node> nodes;
  *grouped = false;
  for (size_t i = 0; i < L.size();) {
    int n = 1;
    if (L[i].carried) {           // done by an earlier launch (mark_x0_share): no node
      ++i;
      continue;
    }
    *grouped |= L[i].cross_lane != 0;       // a shared-input launch that carries ops of other lanes: one chain
    if (L[i].pair) {
      n = 2;                      // (both ops on one lane: no reason to give up the lanes, `grouped` stays)
    } else if (L[i].groupable && h->ops[i].group != 0) {
      while (n < 4 && i + n < L.size() && L[i + n].groupable / 10 == L[i].groupable / 10 && h->ops[i + n].group == h->ops[i].group) ++n;
      *grouped |= n > 1;
    }
    nodes.push_back({i, n});
    i += n;
  }
  return nodes;
}
static int run_node(const std::vector<Launch>& L, const Node& nd, hipStream_t s) {
  if (nd.n == 1 || L[nd.first].pair) return run_launch(L[nd.first], s);
  ConvMulti m;
  Launch ml;
  const int rc = describe_multi(&L[nd.first], nd.n, &m, &ml);
  if (rc) return rc;
  void* args[] = {&m};
  UDP_HIP_CHECK(hipLaunchKernel(ml.fn, ml.grid, ml.block, args, ml.lds, s));
  return UDP_OK;
}

// Eager execution.  lanes != 0: ops run on their lane's stream (lane 0 = s) with event edges for
// the cross-lane dependencies the host planner listed, forked from / joined back into s.
// ev != null: serial on s with an event pair around every op (profiling).
static int enqueue_all(udp_hrnet* h, const std::vector<Launch>& L, hipStream_t s, hipEvent_t* ev, int lanes) {
  bool grouped = false;
  const std::vector<Node> nodes = make_nodes(h, L, &grouped);
  if (grouped) {
    // merged launches span lanes: one chain on s, the same launches the graph replays.  Profiling: the
    // event pair of a merged launch sits on its first op; udp_hrnet_profile splits the time over the members
    for (const Node& nd : nodes) {
      if (ev) UDP_HIP_CHECK(hipEventRecord(ev[2 * nd.first], s));
      const int rc = run_node(L, nd, s);
      if (rc) return rc;
      if (ev) UDP_HIP_CHECK(hipEventRecord(ev[2 * nd.first + 1], s));
    }
    return UDP_OK;
  }
  lanes = lanes && h->n_lanes > 1 && !ev && getenv("UDP_POSE_SERIAL") == nullptr;
  hipStream_t ls[UDP_MAX_LANES] = {s, s, s, s};
  if (lanes) {
    UDP_HIP_CHECK(hipEventRecord(h->ev_fork, s));
    for (int l = 1; l < h->n_lanes; ++l) {
      ls[l] = h->lane_stream[l];
      UDP_HIP_CHECK(hipStreamWaitEvent(ls[l], h->ev_fork, 0));
    }
  }
  for (size_t i = 0; i < h->ops.size(); ++i) {
    if (L[i].carried) continue;                       // done by an earlier launch (mark_x0_share)
    const udp_conv_op& o = h->ops[i];
    hipStream_t os = ls[o.lane];
    const size_t last = i + (L[i].pair ? 1 : 0);      // a chained head pair: one launch for ops i and i + 1 (same lane)
    // the ops of this launch: i (.. last) and the ops it carries -- their waits are honoured here, their signals
    // recorded behind it (a carried op is on this lane and waits only for ops before i: find_share_sets)
    size_t mine[2 + kShareRoutes];
    int n_mine = 0;
    for (size_t j = i; j <= last; ++j) mine[n_mine++] = j;
    for (int c = 0; c < L[i].n_carry; ++c) mine[n_mine++] = (size_t)L[i].carry[c];
    if (lanes)
      for (int m = 0; m < n_mine; ++m)
        for (int k = 0; k < h->ops[mine[m]].n_wait; ++k)
          if (h->ops[h->ops[mine[m]].wait_op[k]].lane != o.lane) UDP_HIP_CHECK(hipStreamWaitEvent(os, h->op_done[h->ops[mine[m]].wait_op[k]], 0));
    if (ev) UDP_HIP_CHECK(hipEventRecord(ev[2 * i], os));
    const int rc = run_launch(L[i], os);
    if (rc) return rc;
    if (ev) UDP_HIP_CHECK(hipEventRecord(ev[2 * i + 1], os));
    for (int m = 0; m < n_mine; ++m)
      if (lanes && h->op_signals[mine[m]]) UDP_HIP_CHECK(hipEventRecord(h->op_done[mine[m]], os));
    i = last;
  }
  if (lanes)
    for (int l = 1; l < h->n_lanes; ++l) {
      UDP_HIP_CHECK(hipEventRecord(h->ev_join[l], ls[l]));
      UDP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_join[l], 0));
    }
  return UDP_OK;
}

// hipGraph of the same program: one kernel node per op; edges = previous op of the same lane +
// the planner's cross-lane dependencies, so independent HRNet branches overlap on the GPU.
static int build_graph(udp_hrnet* h, const std::vector<Launch>& L, hipGraph_t* graph, hipGraphExec_t* exec) {
  UDP_HIP_CHECK(hipGraphCreate(graph, 0));
  bool grouped = false;
  const std::vector<Node> nodes = make_nodes(h, L, &grouped);
  std::vector<hipGraphNode_t> node(nodes.size());
  std::vector<int> node_of_op(L.size(), -1);
  int last_on_lane[UDP_MAX_LANES] = {-1, -1, -1, -1};
  // merged launches span lanes: one chain (branch overlap through graph edges bought nothing anyway)
  const bool serial = grouped || getenv("UDP_POSE_SERIAL") != nullptr;
  for (size_t k = 0; k < nodes.size(); ++k) {
    const size_t i = nodes[k].first;
    const udp_conv_op& o = h->ops[i];
    std::vector<hipGraphNode_t> deps;
    if (serial) {
      if (k) deps.push_back(node[k - 1]);
    } else {
      if (last_on_lane[o.lane] >= 0) deps.push_back(node[last_on_lane[o.lane]]);
      for (int j = 0; j < nodes[k].n; ++j)       // (n > 1 here: a chained head pair, whose second op may wait on the first)
        for (int w = 0; w < h->ops[i + j].n_wait; ++w)
          if ((size_t)h->ops[i + j].wait_op[w] < i) deps.push_back(node[node_of_op[h->ops[i + j].wait_op[w]]]);
      for (int c = 0; c < L[i].n_carry; ++c)     // the ops this launch carries wait for ops before i only (find_share_sets)
        for (int w = 0; w < h->ops[L[i].carry[c]].n_wait; ++w) deps.push_back(node[node_of_op[h->ops[L[i].carry[c]].wait_op[w]]]);
    }
    ConvParams p = L[i].p;
    ConvMulti m;
    Launch ml = L[i];
    void* args[1] = {&p};
    if (nodes[k].n > 1 && !L[i].pair) {
      const int rc = describe_multi(&L[i], nodes[k].n, &m, &ml);
      if (rc) {
        (void)hipGraphDestroy(*graph);
        return rc;
      }
      args[0] = &m;
    }
    if (L[i].share) args[0] = L[i].share.get();
    hipKernelNodeParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.func = const_cast<void*>(ml.fn);
    kp.gridDim = ml.grid;
    kp.blockDim = ml.block;
    kp.sharedMemBytes = ml.lds;
    kp.kernelParams = args;
    kp.extra = nullptr;
    hipError_t e = hipGraphAddKernelNode(&node[k], *graph, deps.data(), deps.size(), &kp);
    if (e != hipSuccess) {
      (void)hipGraphDestroy(*graph);
      return fail(UDP_ERR_HIP, "hipGraphAddKernelNode(op %zu): %s", i, hipGetErrorString(e));
    }
    for (int j = 0; j < nodes[k].n; ++j) node_of_op[i + j] = (int)k;
    for (int c = 0; c < L[i].n_carry; ++c) node_of_op[L[i].carry[c]] = (int)k;
    last_on_lane[o.lane] = (int)k;
  }
  hipError_t e = hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(*graph);
    return fail(UDP_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  }
  return UDP_OK;
}

static int check_forward_args(const char* who, const udp_hrnet* h, const float* in, int n, int flip, const void* ws,
                              size_t ws_bytes, const float* out) {
  if (!h || !in || !ws || !out) return fail(UDP_ERR_ARG, "%s: null pointer", who);
  if (n <= 0) return fail(UDP_ERR_ARG, "%s: n=%d (the reference engine also requires n >= 1)", who, n);
  if (ws_bytes < udp_hrnet_workspace_bytes(h, n, flip))
    return fail(UDP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, udp_hrnet_workspace_bytes(h, n, flip));
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(UDP_ERR_ARG, "%s: workspace not 256-byte aligned", who);
  return UDP_OK;
}

extern "C" int udp_hrnet_profile(udp_hrnet* h, const float* in_nchw, int n, int flip_test, void* workspace,
                                 size_t workspace_bytes, float* heatmaps_nchw, float* ms_per_op, void* stream) {
  int rc = check_forward_args("udp_hrnet_profile", h, in_nchw, n, flip_test, workspace, workspace_bytes, heatmaps_nchw);
  if (rc) return rc;
  if (!ms_per_op) return fail(UDP_ERR_ARG, "udp_hrnet_profile: null pointer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  std::vector<Launch> L;
  rc = describe_all(h, in_nchw, n, flip_test ? 1 : 0, 0, reinterpret_cast<char*>(workspace), heatmaps_nchw, L);
  if (rc) return rc;
  const size_t nops = h->ops.size();
  std::vector<hipEvent_t> ev(2 * nops, nullptr);
  for (auto& e : ev) {
    const hipError_t ce = hipEventCreate(&e);
    if (ce != hipSuccess) {
      for (auto& d : ev)
        if (d) (void)hipEventDestroy(d);
      return fail(UDP_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(ce));
    }
  }
  rc = enqueue_all(h, L, s, ev.data(), 0);
  hipError_t se = hipStreamSynchronize(s);
  if (!rc && se == hipSuccess) {
    bool grouped = false;
    // (an op carried by an earlier launch: 0 -- the whole time is with the carrying op)
    for (size_t i = 0; i < nops; ++i)
      if (L[i].carried) ms_per_op[i] = 0.f;
    for (const Node& nd : make_nodes(h, L, &grouped)) {
      float t = -1.f;
      if (hipEventElapsedTime(&t, ev[2 * nd.first], ev[2 * nd.first + 1]) != hipSuccess) t = -1.f;
      // a merged launch: its time is shared by the members in proportion to their FLOPs
      double total = 0.0;
      auto flops = [&](size_t i) { const udp_conv_op& o = h->ops[i]; return (double)o.ks * o.ks * o.cin * o.cout * o.hout * o.wout; };
      for (int j = 0; j < nd.n; ++j) total += flops(nd.first + j);
      for (int j = 0; j < nd.n; ++j) ms_per_op[nd.first + j] = nd.n == 1 || t < 0 ? t : (float)(t * flops(nd.first + j) / total);
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (rc) return rc;
  if (se != hipSuccess) return fail(UDP_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(se));
  return UDP_OK;
}

static int forward_one(udp_hrnet* h, const float* in_nchw, int n, int flip_test, int out_skip, void* workspace,
                       float* heatmaps_nchw, int use_graph, hipStream_t s) {
  int rc;
  if (use_graph)
    for (size_t k = 0; k < h->graphs.size(); ++k) {
      const GraphEntry g = h->graphs[k];
      if (g.n == n && g.flip == flip_test && g.skip == out_skip && g.in == in_nchw && g.ws == workspace && g.out == heatmaps_nchw) {
        if (k + 1 != h->graphs.size()) {   // most recently used last
          h->graphs.erase(h->graphs.begin() + k);
          h->graphs.push_back(g);
        }
        UDP_HIP_CHECK(hipGraphLaunch(g.exec, s));
        return UDP_OK;
      }
    }
  std::vector<Launch> L;
  rc = describe_all(h, in_nchw, n, flip_test, out_skip, reinterpret_cast<char*>(workspace), heatmaps_nchw, L);
  if (rc) return rc;
  if (!use_graph) return enqueue_all(h, L, s, nullptr, 1);
  // First call for this (shape, buffers): build the graph, then launch it.
  GraphEntry e;
  e.n = n;
  e.flip = flip_test;
  e.skip = out_skip;
  e.in = in_nchw;
  e.ws = workspace;
  e.out = heatmaps_nchw;
  rc = build_graph(h, L, &e.graph, &e.exec);
  if (rc) return rc;
  if (h->graphs.size() >= 8) {
    // evict the least recently used graph; its last replay may still be running (on the caller's stream or on the
    // second lane's) -> drain the device before the executable goes away
    UDP_HIP_CHECK(hipDeviceSynchronize());
    (void)hipGraphExecDestroy(h->graphs[0].exec);
    (void)hipGraphDestroy(h->graphs[0].graph);
    h->graphs.erase(h->graphs.begin());
  }
  h->graphs.push_back(e);
  UDP_HIP_CHECK(hipGraphLaunch(e.exec, s));
  return UDP_OK;
}

extern "C" int udp_hrnet_forward(udp_hrnet* h, const float* in_nchw, int n, int flip_test, void* workspace,
                                 size_t workspace_bytes, float* heatmaps_nchw, int use_graph, void* stream) {
  int rc = check_forward_args("udp_hrnet_forward", h, in_nchw, n, flip_test, workspace, workspace_bytes, heatmaps_nchw);
  if (rc) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  flip_test = flip_test ? 1 : 0;
  if (!use_graph || !split_ok(h, n)) return forward_one(h, in_nchw, n, flip_test, 0, workspace, heatmaps_nchw, use_graph, s);
  // ---- two sub-batch lanes
  if (!h->split_stream) {
    UDP_HIP_CHECK(hipStreamCreateWithFlags(&h->split_stream, hipStreamNonBlocking));
    UDP_HIP_CHECK(hipEventCreateWithFlags(&h->split_fork, hipEventDisableTiming));
    UDP_HIP_CHECK(hipEventCreateWithFlags(&h->split_join, hipEventDisableTiming));
  }
  const int n0 = (n + 1) / 2, n1 = n - n0;
  struct FillHint {                        // tile choice of the lanes' graphs (built on their first call only)
    FillHint() { ws_set_fill_wgs(128); }
    ~FillHint() { ws_set_fill_wgs(512); }
  } fill_hint;
  char* ws0 = reinterpret_cast<char*>(workspace);
  char* ws1 = ws0 + ws_bytes_one(h, n0, flip_test);
  const size_t img_in = (size_t)3 * h->in_h * h->in_w;
  const size_t img_out = out_bytes(h, 1) / sizeof(float);
  hipStream_t s2 = h->split_stream;
  // Between the fork and the join no HIP error returns: the first one is kept (with its message) and the join still
  // runs, so that whatever was enqueued on the second stream is ordered before the caller's next work on `s`.
  hipError_t he = hipSuccess;
  const char* he_what = "";
  auto hip_try = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && he == hipSuccess) {
      he = e;
      he_what = what;
    }
    return e == hipSuccess;
  };
  bool forked = hip_try(hipEventRecord(h->split_fork, s), "hipEventRecord(fork)");
  forked = forked && hip_try(hipStreamWaitEvent(s2, h->split_fork, 0), "hipStreamWaitEvent(fork)");
  if (!forked) {
    // nothing runs on the second stream
  } else if (!flip_test) {
    rc = forward_one(h, in_nchw, n0, 0, 0, ws0, heatmaps_nchw, 1, s);
    if (!rc) rc = forward_one(h, in_nchw + n0 * img_in, n1, 0, 0, ws1, heatmaps_nchw + n0 * img_out, 1, s2);
  } else if (h->out_in_place && (size_t)2 * n * img_out * sizeof(float) < 0x7FFF0000u) {
    // a lane's heat-maps are [its images | their mirrored copies]; the caller's layout is [all images | all mirrored]:
    // the output writers put a lane's mirrored rows behind ALL the plain images themselves (ConvParams::out_skip), a
    // writer that cannot makes the lane fail with UDP_ERR_UNSUPPORTED (describe_conv) and writes nothing
    rc = forward_one(h, in_nchw, n0, 1, n - n0, ws0, heatmaps_nchw, 1, s);
    if (!rc) rc = forward_one(h, in_nchw + n0 * img_in, n1, 1, n0, ws1, heatmaps_nchw + n0 * img_out, 1, s2);
  } else {
    // staged: each lane writes [its images | mirrored] behind the workspaces, four copies put the halves into place
    float* t0 = reinterpret_cast<float*>(ws1 + ws_bytes_one(h, n1, 1));
    float* t1 = t0 + 2 * n0 * img_out;
    rc = forward_one(h, in_nchw, n0, 1, 0, ws0, t0, 1, s);
    if (!rc) {
      hip_try(hipMemcpyAsync(heatmaps_nchw, t0, n0 * img_out * sizeof(float), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(lane 0)");
      hip_try(hipMemcpyAsync(heatmaps_nchw + n * img_out, t0 + n0 * img_out, n0 * img_out * sizeof(float), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(lane 0, mirrored)");
      rc = forward_one(h, in_nchw + n0 * img_in, n1, 1, 0, ws1, t1, 1, s2);
    }
    if (!rc) {
      hip_try(hipMemcpyAsync(heatmaps_nchw + n0 * img_out, t1, n1 * img_out * sizeof(float), hipMemcpyDeviceToDevice, s2), "hipMemcpyAsync(lane 1)");
      hip_try(hipMemcpyAsync(heatmaps_nchw + (n + n0) * img_out, t1 + n1 * img_out, n1 * img_out * sizeof(float), hipMemcpyDeviceToDevice, s2), "hipMemcpyAsync(lane 1, mirrored)");
    }
  }
  // join: always, also after an error in a lane or in a copy
  if (forked && hip_try(hipEventRecord(h->split_join, s2), "hipEventRecord(join)")) hip_try(hipStreamWaitEvent(s, h->split_join, 0), "hipStreamWaitEvent(join)");
  if (rc) return rc;
  if (he != hipSuccess) return fail(UDP_ERR_HIP, "udp_hrnet_forward: %s failed: %s", he_what, hipGetErrorString(he));
  return UDP_OK;
}

extern "C" int udp_hrnet_destroy(udp_hrnet* h) {
  if (!h) return UDP_OK;
  if (h->split_stream) {
    (void)hipStreamSynchronize(h->split_stream);
    (void)hipStreamDestroy(h->split_stream);
    (void)hipEventDestroy(h->split_fork);
    (void)hipEventDestroy(h->split_join);
  }
  for (auto& g : h->graphs) {
    (void)hipGraphExecDestroy(g.exec);
    (void)hipGraphDestroy(g.graph);
  }
  for (int l = 1; l < UDP_MAX_LANES; ++l) {
    if (h->lane_stream[l]) (void)hipStreamDestroy(h->lane_stream[l]);
    if (h->ev_join[l]) (void)hipEventDestroy(h->ev_join[l]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  for (auto e : h->op_done)
    if (e) (void)hipEventDestroy(e);
  delete h;
  return UDP_OK;
}

static int conv2d_fused_impl(const udp_conv_op* o, int dtype, int n, const void* in, const void* weights,
                             const float* bias, const void* res, const void* up0, const void* up1,
                             const void* up2, void* out, double* bn_ws, size_t bn_ws_doubles, int* bn_rows, void* stream);

extern "C" int udp_conv2d_fused(const udp_conv_op* o, int dtype, int n, const void* in, const void* weights,
                                const float* bias, const void* res, const void* up0, const void* up1,
                                const void* up2, void* out, void* stream) {
  return conv2d_fused_impl(o, dtype, n, in, weights, bias, res, up0, up1, up2, out, nullptr, 0, nullptr, stream);
}

extern "C" int udp_conv2d_fused_bn(const udp_conv_op* o, int dtype, int n, const void* in, const void* weights,
                                   const float* bias, void* out, double* bn_ws, size_t bn_ws_doubles, int* bn_rows,
                                   void* stream) {
  if (!bn_ws || !bn_rows) return fail(UDP_ERR_ARG, "udp_conv2d_fused_bn: null pointer");
  if (dtype == UDP_F16X2 || !o || o->kind != UDP_OP_CONV || o->out_buf == UDP_BUF_OUTPUT || o->n_up || o->relu ||
      (o->out_pitch && o->out_pitch != o->cout) || o->out_coff)
    return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused_bn: a plain fp32 / bf16 NHWC conv without addends, ReLU or channel views");
  return conv2d_fused_impl(o, dtype, n, in, weights, bias, nullptr, nullptr, nullptr, nullptr, out, bn_ws, bn_ws_doubles, bn_rows, stream);
}

static int conv2d_params(const udp_conv_op* o, int dtype, int n, const void* in, const void* weights,
                         const float* bias, const void* res, const void* up0, const void* up1,
                         const void* up2, void* out, ConvParams* pp) {
  ConvParams& p = *pp;
  if (!o || !in || !out) return fail(UDP_ERR_ARG, "udp_conv2d_fused: null pointer");
  if (dtype != UDP_F32 && dtype != UDP_BF16 && dtype != UDP_F16X2) return fail(UDP_ERR_ARG, "udp_conv2d_fused: dtype %d", dtype);
  if (n <= 0) return fail(UDP_ERR_ARG, "udp_conv2d_fused: n=%d", n);
  if (o->kind != UDP_OP_CONV && o->kind != UDP_OP_FUSE && o->kind != UDP_OP_DECONV && o->kind != UDP_OP_DWCONV && o->kind != UDP_OP_PIXSHUF &&
      o->kind != UDP_OP_SE && o->kind != UDP_OP_GNORM && o->kind != UDP_OP_LINATTN && o->kind != UDP_OP_LNORM && o->kind != UDP_OP_MHATTN &&
      o->kind != UDP_OP_ACT && o->kind != UDP_OP_SE_RES && o->kind != UDP_OP_PRM_GATE && o->kind != UDP_OP_PRM_DW9 && o->kind != UDP_OP_SE_ACT)
    return fail(UDP_ERR_ARG, "udp_conv2d_fused: kind %d", o->kind);
  if (const int rc = act_validate(*o, dtype, res != nullptr)) return rc;
  if (o->kind != UDP_OP_FUSE && o->kind != UDP_OP_PIXSHUF && o->kind != UDP_OP_LINATTN && o->kind != UDP_OP_MHATTN && o->kind != UDP_OP_ACT && (!weights || (!bias && o->kind != UDP_OP_SE && o->kind != UDP_OP_GNORM && o->kind != UDP_OP_LNORM && o->kind != UDP_OP_SE_RES && o->kind != UDP_OP_PRM_GATE && o->kind != UDP_OP_SE_ACT))) return fail(UDP_ERR_ARG, "udp_conv2d_fused: conv needs weights and bias");
  if (o->kind == UDP_OP_SE) {
    const int rc = se_validate(*o, dtype);
    if (rc) return rc;
    if (res) return fail(UDP_ERR_ARG, "udp_conv2d_fused: squeeze-excitation takes no residual");
    if (in == out && (o->in_coff != o->out_coff || (o->in_pitch ? o->in_pitch : o->cin) != (o->out_pitch ? o->out_pitch : o->cout)))
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: squeeze-excitation in place needs the same view for in and out");
  }
  if (o->kind == UDP_OP_SE_ACT) {
    const int rc = se_act_validate(*o, dtype);
    if (rc) return rc;
    if (res) return fail(UDP_ERR_ARG, "udp_conv2d_fused: activation + squeeze-excitation takes no residual");
    if (in == out && (o->in_coff != o->out_coff || (o->in_pitch ? o->in_pitch : o->cin) != (o->out_pitch ? o->out_pitch : o->cout)))
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: activation + squeeze-excitation in place needs the same view for in and out");
  }
  if (o->kind == UDP_OP_SE_RES || o->kind == UDP_OP_PRM_GATE || o->kind == UDP_OP_PRM_DW9) {
    // the gates of RSN-18 "se + prm": `res` = the shortcut (optional) / -- / out_1; UDP_OP_PRM_DW9: `up0` = the channel gate's fp32 rows
    const int rc = o->kind == UDP_OP_SE_RES ? se_res_validate(*o, dtype) : o->kind == UDP_OP_PRM_GATE ? prm_gate_validate(*o, dtype) : prm_dw9_validate(*o, dtype);
    if (rc) return rc;
    if (o->kind == UDP_OP_SE_RES) {
      if (in == out && (o->in_coff != o->out_coff || (o->in_pitch ? o->in_pitch : o->cin) != (o->out_pitch ? o->out_pitch : o->cout)))
        return fail(UDP_ERR_ARG, "udp_conv2d_fused: se + residual in place needs the same view for in and out");
      if (res && (res == in || res == out)) return fail(UDP_ERR_ARG, "udp_conv2d_fused: se + residual: res must not be in or out");
    } else {
      if (o->kind == UDP_OP_PRM_GATE ? res != nullptr : !res || !up0) return fail(UDP_ERR_ARG, "udp_conv2d_fused: prm gates: res / up0 (out_1 / the channel gate's rows) belong to the spatial gate alone");
      if (in == out || res == out) return fail(UDP_ERR_ARG, "udp_conv2d_fused: prm gates: out must not be in or res");
    }
  }
  if (o->kind == UDP_OP_GNORM || o->kind == UDP_OP_LINATTN) {
    const bool gn = o->kind == UDP_OP_GNORM;
    const int rc = gn ? gnorm_validate(*o, dtype) : linattn_validate(*o, dtype);
    if (rc) return rc;
    if (res) return fail(UDP_ERR_ARG, "udp_conv2d_fused: %s takes no residual", gn ? "group norm" : "linear attention");
    if (in == out && (!gn || o->in_coff != o->out_coff || (o->in_pitch ? o->in_pitch : o->cin) != (o->out_pitch ? o->out_pitch : o->cout)))
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: %s", gn ? "group norm in place needs the same view for in and out" : "linear attention: out must not be in");
  }
  if (o->kind == UDP_OP_LNORM || o->kind == UDP_OP_MHATTN || o->kind == UDP_OP_ACT) {
    const char* what = o->kind == UDP_OP_LNORM ? "layer norm" : o->kind == UDP_OP_MHATTN ? "multi-head attention" : "activation op";
    const int rc = o->kind == UDP_OP_LNORM ? lnorm_validate(*o, dtype) : o->kind == UDP_OP_MHATTN ? mhattn_validate(*o, dtype) : act_op_validate(*o, dtype);
    if (rc) return rc;
    if (res) return fail(UDP_ERR_ARG, "udp_conv2d_fused: %s takes no residual", what);
    if (in == out && (o->kind == UDP_OP_MHATTN || o->in_coff != o->out_coff || (o->in_pitch ? o->in_pitch : o->cin) != (o->out_pitch ? o->out_pitch : o->cout)))
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: %s: %s", what, o->kind == UDP_OP_MHATTN ? "out must not be in" : "in place needs the same view for in and out");
  }
  if (o->kind == UDP_OP_DWCONV || o->kind == UDP_OP_PIXSHUF) {
    const bool dw = o->kind == UDP_OP_DWCONV;
    const int rc = dw ? dwconv_validate(*o, dtype) : pixshuf_validate(*o, dtype);
    if (rc) return rc;
    // the passthrough of a depthwise launch: source = `res`, destination = `up0` (written)
    const bool pass = dw && o->n_out2 == 1;
    if (pass ? (!res || !up0) : (res != nullptr)) return fail(UDP_ERR_ARG, "udp_conv2d_fused: %s: res / up0 are the passthrough's source / destination (n_out2 = 1) and NULL otherwise", dw ? "depthwise conv" : "pixel shuffle");
  }
  if (o->kind == UDP_OP_DECONV) {
    if (o->ks != 4 || o->stride != 2 || o->hout != 2 * o->hin || o->wout != 2 * o->win)
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: deconv must be k4 s2 p1 (output = 2x the input)");
    if (res || o->n_up || o->out_buf == UDP_BUF_OUTPUT) return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused: deconv takes no addends and writes NHWC");
  }
  if (o->cout <= 0 || o->cout_pad < o->cout || o->cout_pad % 32 || o->n_up < 0 || o->n_up > 3)
    return fail(UDP_ERR_ARG, "udp_conv2d_fused: bad cout/cout_pad/n_up");
  if (o->kind == UDP_OP_CONV) {
    if ((o->ks != 1 && o->ks != 3 && o->ks != 7) || (o->stride != 1 && o->stride != 2)) return fail(UDP_ERR_ARG, "udp_conv2d_fused: ks/stride");
    if (o->ks == 7 && (o->group || o->chain_cout || o->n_out2))
      return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused: a 7x7 conv takes no group, chained conv or second outputs");
    const int pad = o->ks / 2;
    if (o->hout != (o->hin + 2 * pad - o->ks) / o->stride + 1 || o->wout != (o->win + 2 * pad - o->ks) / o->stride + 1)
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: output size does not match input/stride");
  }
  const void* ups[3] = {up0, up1, up2};
  memset(&p, 0, sizeof(p));
  p.N = n;
  p.Hin = o->hin;
  p.Win = o->win;
  p.Cin = o->cin;
  p.Hout = o->hout;
  p.Wout = o->wout;
  p.Cout = o->cout;
  p.CoutPad = o->cout_pad;
  p.relu = o->relu;
  if (o->kind == UDP_OP_SE || o->kind == UDP_OP_GNORM || o->kind == UDP_OP_LNORM || o->kind == UDP_OP_SE_ACT) {
    p.up_shift[0] = o->chain_cout;      // hidden width / real channels (se_validate, gnorm_validate, lnorm_validate: n_up == 0, n_out2 == 0)
  } else if (o->kind == UDP_OP_SE_RES || o->kind == UDP_OP_PRM_GATE) {
    p.up_shift[0] = o->kind == UDP_OP_SE_RES ? o->chain_cout : o->cin;      // hidden width (n_up == 0, n_out2 == 0)
  } else if (o->kind == UDP_OP_MHATTN) {
    p.up_shift[0] = o->chain_cout;      // real width d
    p.up_shift[1] = o->up_shift[0];     // heads (mhattn_validate: n_up == 0, n_out2 == 0)
  } else if (o->kind == UDP_OP_DWCONV) {
    if (o->n_out2) {
      p.nout2 = 1;
      p.out2[0] = const_cast<void*>(up0);
      p.out2_coff[0] = o->out2_coff[0];
      p.out2_pitch[0] = o->out2_pitch[0];
      p.up_shift[0] = o->chain_cout;
    }
  } else {
    if (o->n_out2) return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused: second outputs (n_out2) exist in udp_hrnet programs only");
    if (o->chain_cout) return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused: chained convs (chain_cout) exist in udp_hrnet programs only");
  }
  p.wfmt = o->wfmt;
  p.wexp = o->wexp;
  p.in_stuff2 = o->in_stuff2 ? 1 : 0;
  p.flip_from = n;
  p.in_pitch = o->in_pitch ? o->in_pitch : o->cin;
  p.in_coff = o->in_coff;
  p.out_pitch = o->out_pitch ? o->out_pitch : o->cout;
  p.out_coff = o->out_coff;
  p.res_pitch = o->res_pitch ? o->res_pitch : o->cout;
  p.res_coff = o->res_coff;
  p.in = in;
  p.out = out;
  p.out_nchw_f32 = o->out_buf == UDP_BUF_OUTPUT;
  p.res = res;
  p.wgt = weights;
  p.bias = bias;
  p.nup = o->n_up;
  if (o->kind == UDP_OP_PRM_DW9) {      // n_up == 1: not an addend but the channel gate's fp32 rows (prm_dw9_validate)
    p.up[0] = up0;
    return UDP_OK;
  }
  for (int u = 0; u < o->n_up; ++u) {
    const int s = o->up_shift[u];
    // (UDP_OP_FUSE also takes same-resolution addends, shift 0: the training step's exchange-unit sums have up to four terms)
    if (!ups[u] || s < (o->kind == UDP_OP_FUSE ? 0 : 1) || s > 5 || (o->hout & ((1 << s) - 1)) || (o->wout & ((1 << s) - 1)))
      return fail(UDP_ERR_ARG, "udp_conv2d_fused: up %d", u);
    p.up[u] = ups[u];
    p.up_shift[u] = s;
  }
  return UDP_OK;
}

static int conv2d_fused_impl(const udp_conv_op* o, int dtype, int n, const void* in, const void* weights,
                             const float* bias, const void* res, const void* up0, const void* up1,
                             const void* up2, void* out, double* bn_ws, size_t bn_ws_doubles, int* bn_rows, void* stream) {
  ConvParams p;
  const int prc = conv2d_params(o, dtype, n, in, weights, bias, res, up0, up1, up2, out, &p);
  if (prc) return prc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Launch l;
  p.bn_ws = bn_ws;
  const int rc = o->kind == UDP_OP_FUSE     ? describe_fuse(p, dtype, &l)
                 : o->kind == UDP_OP_DECONV ? describe_deconv(p, dtype, &l)
                 : o->kind == UDP_OP_DWCONV ? describe_dwconv(p, dtype, o->ks, o->stride, &l)
                 : o->kind == UDP_OP_SE     ? describe_se(p, dtype, &l)
                 : o->kind == UDP_OP_SE_ACT ? describe_se_act(p, dtype, &l)
                 : o->kind == UDP_OP_GNORM  ? describe_gnorm(p, dtype, &l)
                 : o->kind == UDP_OP_LINATTN ? describe_linattn(p, dtype, &l)
                 : o->kind == UDP_OP_LNORM  ? describe_lnorm(p, dtype, &l)
                 : o->kind == UDP_OP_MHATTN ? describe_mhattn(p, dtype, &l)
                 : o->kind == UDP_OP_ACT    ? describe_act(p, dtype, &l)
                 : o->kind == UDP_OP_SE_RES ? describe_gate(p, dtype, false, &l)
                 : o->kind == UDP_OP_PRM_GATE ? describe_gate(p, dtype, true, &l)
                 : o->kind == UDP_OP_PRM_DW9 ? describe_prm_dw9(p, dtype, &l)
                 : o->kind == UDP_OP_PIXSHUF ? describe_pixshuf(p, dtype, &l)
                                            : describe_conv(p, dtype, o->ks, o->stride, &l);
  if (rc) return rc;
  if (bn_ws) {
    // one partial row of 2*Cout doubles per tile (grid.x); the caller's workspace must hold them
    // (and udp_bn_train_fwd_from_sums takes at most udp_bn_rows_max() rows: the caller falls back to the separate
    // statistics pass on UDP_ERR_WORKSPACE either way)
    if ((size_t)l.grid.x * 2 * o->cout > bn_ws_doubles || l.grid.x > (unsigned)udp_bn_rows_max())
      return fail(UDP_ERR_WORKSPACE, "udp_conv2d_fused_bn: %u partial rows x %d doubles exceed the workspace or the %d-row limit",
                  l.grid.x, 2 * o->cout, udp_bn_rows_max());
    *bn_rows = (int)l.grid.x;
  }
  return run_launch(l, s);
}

// Up to 4 independent plain convs (same dtype and batch; the same-depth convs of different HRNet branches in the
// training step) in as few launches as possible: members whose tile fits the merged instantiation go into ONE
// conv_mfma_multi launch, the others run on their own.  Per-member results are those of udp_conv2d_fused /
// udp_conv2d_fused_bn (the K loop order does not depend on the tiling).
extern "C" int udp_conv2d_fused_group(udp_conv_item* items, int n_items, int dtype, int n, void* stream) {
  if (!items || n_items < 1 || n_items > 4) return fail(UDP_ERR_ARG, "udp_conv2d_fused_group: %d members (1..4)", n_items);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  std::vector<Launch> L((size_t)n_items);
  for (int j = 0; j < n_items; ++j) {
    udp_conv_item& it = items[j];
    const udp_conv_op* o = it.op;
    if (!o || o->kind != UDP_OP_CONV || o->n_up || o->out_buf == UDP_BUF_OUTPUT)
      return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused_group: member %d is not a plain NHWC conv", j);
    if (o->relu >= UDP_ACT_HSWISH) return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused_group: member %d: hard-swish / SiLU have no merged-launch form", j);
    if (it.bn_ws && (dtype == UDP_F16X2 || o->relu || it.res || (o->out_pitch && o->out_pitch != o->cout) || o->out_coff))
      return fail(UDP_ERR_UNSUPPORTED, "udp_conv2d_fused_group: member %d: BatchNorm sums need a plain fp32 / bf16 conv", j);
    ConvParams p;
    int rc = conv2d_params(o, dtype, n, it.in, it.weights, it.bias, it.res, nullptr, nullptr, nullptr, it.out, &p);
    if (rc) return rc;
    p.bn_ws = it.bn_ws;
    rc = n_items > 1 && getenv("UDP_POSE_NO_GROUPS") == nullptr ? describe_conv_grouped(p, dtype, o->ks, o->stride, &L[j]) : 1;
    if (rc == 1) rc = describe_conv(p, dtype, o->ks, o->stride, &L[j]);
    if (rc) return rc;
    if (it.bn_ws) {
      if ((size_t)L[j].grid.x * 2 * o->cout > it.bn_ws_doubles || L[j].grid.x > (unsigned)udp_bn_rows_max())
        return fail(UDP_ERR_WORKSPACE, "udp_conv2d_fused_group: member %d: %u partial rows x %d doubles exceed the workspace or the %d-row limit",
                    j, L[j].grid.x, 2 * o->cout, udp_bn_rows_max());
      it.bn_rows = (int)L[j].grid.x;
    }
  }
  // merged members first (order inside a merged launch: as given, the caller lists the deepest-K member first)
  std::vector<Launch> G;
  std::vector<int> rest;
  for (int j = 0; j < n_items; ++j) {
    if (L[j].groupable && (G.empty() || L[j].groupable / 10 == G[0].groupable / 10))
      G.push_back(L[j]);
    else
      rest.push_back(j);
  }
  if (G.size() >= 2) {
    ConvMulti m;
    Launch ml;
    const int rc = describe_multi(G.data(), (int)G.size(), &m, &ml);
    if (rc) return rc;
    void* args[] = {&m};
    UDP_HIP_CHECK(hipLaunchKernel(ml.fn, ml.grid, ml.block, args, ml.lds, s));
  } else {
    for (const Launch& l : G) {
      const int rc = run_launch(l, s);
      if (rc) return rc;
    }
  }
  for (int j : rest) {
    const int rc = run_launch(L[j], s);
    if (rc) return rc;
  }
  return UDP_OK;
}
