// Training of the polarized self-attention block (PSA_s) of pose_hrnet_psa on gfx950: the train-mode forward that
// keeps what the backward needs, and the backward.
//
// Replaces PSA_s.forward (deep_hrnet/lib/models/PSA.py:190-269) under model.train() and its autograd backward.
// Per image, on an NHWC map x [HW][C] (csrc/psa.hip has the inference form of the same arithmetic):
//
//   a = softmax_HW(wq.x_p)          xbar = sum_p a_p x_p      ctx = Wv xbar
//   h = W1 ctx + b1                 r = relu(LN(h))           m = sigmoid(W2 r + b2)      x1 = x * m[c]
//   gbar = Wg mean_p(x1)            theta = Wt x1 (1x1 conv, the caller's conv kernel)    T_j = softmax_HW(theta_j)
//   s_p = sigmoid(sum_j gbar_j T_jp)                          x2 = x1 * s_p
//
// Every map-sized pass spreads an image over S workgroups (a chunk of pixels each): a workgroup leaves its partial
// reduction in a row of the per-image save area, and the consumer adds the S rows in row order -- the same order on
// every run, no atomics.  The tiny per-image chain (Wv, W1, LayerNorm, W2) is one workgroup per image.  Parameter
// gradients are summed over the images in image order by psa_t_params (one thread per gradient element).
// Storage types float and __bf16; every reduction in fp32.
#include <type_traits>

#include "common.h"

namespace udp {

// per-image layout of the fp32 save area
struct PsaLay {
  int q, s, dctx;                                    // [HW] each: logits wq.x_p, spatial gate s_p, d(ctx_p)
  int stat;                                          // gmax, gsum, rstd, sum_c dxbar_c xbar_c
  int xbar, xmean, ctx, hhat, r, m, gbar, x1mean;    // forward chain
  int M, Z;                                          // per-channel max / sum of exp of theta
  int dgbar, dz2, dy, dh, dctxv, dxbar;              // backward chain
  int pp, ps, pg, pm, pw;                            // partial rows [S][..]
  int pp_w;                                          // width of a pp row: cmax, csum, -, -, num[C], xsum[C]
  int img;                                           // floats per image
  __host__ __device__ PsaLay(int HW, int C, int S) {
    const int C2 = C / 2, C8 = C / 8;
    int o = 0;
    auto take = [&](int k) { const int at = o; o += (k + 3) & ~3; return at; };
    q = take(HW); s = take(HW); dctx = take(HW);
    stat = take(4);
    xbar = take(C); xmean = take(C); ctx = take(C2); hhat = take(C8); r = take(C8); m = take(C); gbar = take(C2);
    x1mean = take(C);
    M = take(C2); Z = take(C2);
    dgbar = take(C2); dz2 = take(C); dy = take(C8); dh = take(C8); dctxv = take(C2); dxbar = take(C);
    pp_w = 4 + 2 * C;
    pp = take(S * pp_w); ps = take(S * C); pg = take(S * C2); pm = take(S * C); pw = take(S * C);
    img = o;
  }
};

struct PsaT {
  const float *wq, *wv, *w1, *b1, *lg, *lb, *w2, *b2, *wg;
  float *dwq, *dwv, *dw1, *db1, *dlg, *dlb, *dw2, *db2, *dwg;
  const void *x, *x1, *theta, *dx2, *dx1;
  void *o_x1, *o_x2, *o_dx1, *o_dtheta, *o_dx;
  float* save;
  int N, HW, C, S, chunk;
};

template <typename T>
__device__ __forceinline__ float4 ld4(const void* base, size_t i) {
  if constexpr (std::is_same<T, float>::value) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + i);
  } else {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const __bf16*>(base) + i);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
}
template <typename T>
__device__ __forceinline__ void st4(void* base, size_t i, float4 v) {
  if constexpr (std::is_same<T, float>::value) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + i) = v;
  } else {
    union { __bf16 h[4]; uint2 u; } k;
    k.h[0] = (__bf16)v.x; k.h[1] = (__bf16)v.y; k.h[2] = (__bf16)v.z; k.h[3] = (__bf16)v.w;
    *reinterpret_cast<uint2*>(reinterpret_cast<__bf16*>(base) + i) = k.u;
  }
}
__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }

// sum over the L (power of two, <= 64) consecutive lanes that share a pixel; every lane gets the sum
__device__ __forceinline__ float lanes_sum(float v, int L) {
  for (int off = L >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wg_reduce(float v, bool is_max, float* red) {
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_down(v, off);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < 4; ++k) r = is_max ? fmaxf(r, red[k]) : r + red[k];
  return r;
}
// acc = the four channel sums of a thread (channels 4l.., pixel group pg of G): row[c] = sum over the groups in
// group order.  part: 1024 floats of LDS.
__device__ __forceinline__ void groups_sum(float4 acc, float* part, int Cc, int l, int pg, float* row, bool is_max = false) {
  __syncthreads();
  *reinterpret_cast<float4*>(part + pg * Cc + 4 * l) = acc;
  __syncthreads();
  const int G = 1024 / Cc;
  for (int c = threadIdx.x; c < Cc; c += 256) {
    float v = part[c];
    for (int g = 1; g < G; ++g) v = is_max ? fmaxf(v, part[g * Cc + c]) : v + part[g * Cc + c];
    row[c] = v;
  }
}

// What a workgroup of a map-sized pass derives from its block index: image n, pixel chunk [p0, p0 + np) of it, and
// the thread's place -- channels 4l .. 4l+3 (Cc channels per pixel = L lanes) of the pixels pg, pg + PPB, ...
struct Chunk {
  int C, HW, t, L, PPB, l, pg, n, sp, p0, np;
  PsaLay ly;
  float* sv;       // the image's save area
  size_t px0;      // first pixel of the chunk in the [N * HW] map
  __device__ Chunk(const PsaT& a, int Cc) : ly(a.HW, a.C, a.S) {
    C = a.C; HW = a.HW; t = threadIdx.x;
    L = Cc / 4; PPB = 256 / L; l = t % L; pg = t / L;
    n = blockIdx.y; sp = blockIdx.x;
    p0 = sp * a.chunk; np = min(HW, p0 + a.chunk) - p0;
    sv = a.save + (size_t)n * ly.img;
    px0 = (size_t)n * HW + p0;
  }
};

// forward 1: logits of the chunk -> save; chunk max / sum of exp / sum_p e_p x_p / sum_p x_p -> pp row
template <typename T>
__global__ __launch_bounds__(256) void psa_t_pool_part(const PsaT a) {
  extern __shared__ float sm[];   // e[chunk] | part[1024]
  __shared__ float red[4];
  const Chunk k(a, a.C);
  float* e = sm;
  float* part = sm + a.chunk;
  const float4 wq = *reinterpret_cast<const float4*>(a.wq + 4 * k.l);
  float lmax = -INFINITY;
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float q = lanes_sum(dot4(ld4<T>(a.x, (k.px0 + i) * k.C + 4 * k.l), wq), k.L);
    if (k.l == 0) {
      e[i] = q;
      k.sv[k.ly.q + k.p0 + i] = q;
    }
    lmax = fmaxf(lmax, q);
  }
  const float cmax = wg_reduce(lmax, true, red);
  float lsum = 0.f;
  for (int i = k.t; i < k.np; i += 256) {
    const float v = expf(e[i] - cmax);
    e[i] = v;
    lsum += v;
  }
  const float csum = wg_reduce(lsum, false, red);
  float4 num = make_float4(0.f, 0.f, 0.f, 0.f), xs = num;
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float4 v = ld4<T>(a.x, (k.px0 + i) * k.C + 4 * k.l);
    const float w = e[i];
    num.x = fmaf(w, v.x, num.x); num.y = fmaf(w, v.y, num.y); num.z = fmaf(w, v.z, num.z); num.w = fmaf(w, v.w, num.w);
    xs.x += v.x; xs.y += v.y; xs.z += v.z; xs.w += v.w;
  }
  float* row = k.sv + k.ly.pp + k.sp * k.ly.pp_w;
  if (k.t == 0) {
    row[0] = cmax;
    row[1] = csum;
  }
  groups_sum(num, part, k.C, k.l, k.pg, row + 4);
  groups_sum(xs, part, k.C, k.l, k.pg, row + 4 + k.C);
}

// forward 2 (one workgroup per image): the pp rows -> xbar, xmean; the channel chain -> m, gbar and what its backward reads
__global__ __launch_bounds__(256) void psa_t_mlp_fwd(const PsaT a) {
  __shared__ float xb[256], xm[256], ctx[128], h[32], msk[256], sc[64];
  __shared__ float stat[2];
  const int C = a.C, C2 = C / 2, C8 = C / 8, S = a.S, t = threadIdx.x, n = blockIdx.x;
  const PsaLay ly(a.HW, C, S);
  float* sv = a.save + (size_t)n * ly.img;
  const float* pp = sv + ly.pp;
  if (t == 0) {
    float gmax = pp[0];
    for (int s = 1; s < S; ++s) gmax = fmaxf(gmax, pp[s * ly.pp_w]);
    float gsum = 0.f;
    for (int s = 0; s < S; ++s) {
      sc[s] = expf(pp[s * ly.pp_w] - gmax);
      gsum = fmaf(pp[s * ly.pp_w + 1], sc[s], gsum);
    }
    stat[0] = gsum;
    sv[ly.stat] = gmax;
    sv[ly.stat + 1] = gsum;
  }
  __syncthreads();
  if (t < C) {
    float num = 0.f, xs = 0.f;
    for (int s = 0; s < S; ++s) {
      num = fmaf(pp[s * ly.pp_w + 4 + t], sc[s], num);
      xs += pp[s * ly.pp_w + 4 + C + t];
    }
    xb[t] = num / stat[0];
    xm[t] = xs / (float)a.HW;
    sv[ly.xbar + t] = xb[t];
    sv[ly.xmean + t] = xm[t];
  }
  __syncthreads();
  if (t < C2) {
    float v = 0.f;
    for (int c = 0; c < C; ++c) v = fmaf(a.wv[t * C + c], xb[c], v);
    ctx[t] = v;
    sv[ly.ctx + t] = v;
  }
  __syncthreads();
  if (t < C8) {
    float v = a.b1[t];
    for (int j = 0; j < C2; ++j) v = fmaf(a.w1[t * C2 + j], ctx[j], v);
    h[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    float mu = 0.f;
    for (int k = 0; k < C8; ++k) mu += h[k];
    mu /= (float)C8;
    float var = 0.f;
    for (int k = 0; k < C8; ++k) var += (h[k] - mu) * (h[k] - mu);
    stat[0] = mu;
    stat[1] = rsqrtf(var / (float)C8 + 1e-5f);
    sv[ly.stat + 2] = stat[1];
  }
  __syncthreads();
  if (t < C8) {
    const float hh = (h[t] - stat[0]) * stat[1];
    sv[ly.hhat + t] = hh;
    h[t] = fmaxf(hh * a.lg[t] + a.lb[t], 0.f);
    sv[ly.r + t] = h[t];
  }
  __syncthreads();
  if (t < C) {
    float v = a.b2[t];
    for (int k = 0; k < C8; ++k) v = fmaf(a.w2[t * C8 + k], h[k], v);
    const float m = 1.f / (1.f + expf(-v));
    msk[t] = m * xm[t];
    sv[ly.m + t] = m;
    sv[ly.x1mean + t] = msk[t];
  }
  __syncthreads();
  if (t < C2) {
    float v = 0.f;
    for (int c = 0; c < C; ++c) v = fmaf(a.wg[t * C + c], msk[c], v);
    sv[ly.gbar + t] = v;
  }
}

// forward 3: x1 = x * m[c]
template <typename T>
__global__ __launch_bounds__(256) void psa_t_scale(const PsaT a) {
  const int C4 = a.C / 4;
  const long per = (long)a.HW * C4, total = per * a.N;
  const PsaLay ly(a.HW, a.C, a.S);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long n = i / per;
    const int c4 = (int)(i % C4);
    const float4 m = *reinterpret_cast<const float4*>(a.save + (size_t)n * ly.img + ly.m + 4 * c4);
    float4 v = ld4<T>(a.x, (size_t)i * 4);
    v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
    st4<T>(a.o_x1, (size_t)i * 4, v);
  }
}

// forward 4: per-channel max and sum of exp of theta over the chunk -> ps row {max[C2], sum[C2]}
template <typename T>
__global__ __launch_bounds__(256) void psa_t_sp_part(const PsaT a) {
  __shared__ float part[1024];
  __shared__ float cm[128];
  const Chunk k(a, a.C / 2);
  const int C2 = k.C / 2;
  float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float4 v = ld4<T>(a.theta, (k.px0 + i) * C2 + 4 * k.l);
    mx.x = fmaxf(mx.x, v.x); mx.y = fmaxf(mx.y, v.y); mx.z = fmaxf(mx.z, v.z); mx.w = fmaxf(mx.w, v.w);
  }
  groups_sum(mx, part, C2, k.l, k.pg, cm, true);
  __syncthreads();
  const float4 m4 = *reinterpret_cast<const float4*>(cm + 4 * k.l);
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float4 v = ld4<T>(a.theta, (k.px0 + i) * C2 + 4 * k.l);
    z.x += expf(v.x - m4.x); z.y += expf(v.y - m4.y); z.z += expf(v.z - m4.z); z.w += expf(v.w - m4.w);
  }
  float* row = k.sv + k.ly.ps + k.sp * k.C;
  if (k.t < C2) row[k.t] = cm[k.t];
  groups_sum(z, part, C2, k.l, k.pg, row + C2);
}

// M[j], Z[j] of the image from the ps rows (row order) into LDS; block 0 of the image also saves them
__device__ __forceinline__ void theta_stats(const PsaT& a, const PsaLay& ly, float* sv, float* M, float* Z, bool store) {
  const int C = a.C, C2 = C / 2, t = threadIdx.x;
  if (t < C2) {
    const float* ps = sv + ly.ps;
    float m = ps[t];
    for (int s = 1; s < a.S; ++s) m = fmaxf(m, ps[s * C + t]);
    float z = 0.f;
    for (int s = 0; s < a.S; ++s) z = fmaf(ps[s * C + C2 + t], expf(ps[s * C + t] - m), z);
    M[t] = m;
    Z[t] = z;
    if (store) {
      sv[ly.M + t] = m;
      sv[ly.Z + t] = z;
    }
  }
  __syncthreads();
}

// forward 5: s_p = sigmoid(sum_j gbar_j T_jp) -> save; x2 = x1 * s_p
template <typename T>
__global__ __launch_bounds__(256) void psa_t_sp_apply(const PsaT a) {
  extern __shared__ float sm[];   // sg[chunk]
  __shared__ float M[128], Z[128];
  const Chunk k(a, a.C / 2);
  const int C2 = k.C / 2;
  theta_stats(a, k.ly, k.sv, M, Z, k.sp == 0);
  const float4 m4 = *reinterpret_cast<const float4*>(M + 4 * k.l), z4 = *reinterpret_cast<const float4*>(Z + 4 * k.l);
  const float4 g4 = *reinterpret_cast<const float4*>(k.sv + k.ly.gbar + 4 * k.l);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float4 v = ld4<T>(a.theta, (k.px0 + i) * C2 + 4 * k.l);
    float c = g4.x * (expf(v.x - m4.x) / z4.x);
    c = fmaf(g4.y, expf(v.y - m4.y) / z4.y, c);
    c = fmaf(g4.z, expf(v.z - m4.z) / z4.z, c);
    c = fmaf(g4.w, expf(v.w - m4.w) / z4.w, c);
    c = lanes_sum(c, k.L);
    if (k.l == 0) {
      const float s = 1.f / (1.f + expf(-c));
      sm[i] = s;
      k.sv[k.ly.s + k.p0 + i] = s;
    }
  }
  __syncthreads();
  const int C4 = k.C / 4;
  for (int i = k.t; i < k.np * C4; i += 256) {
    const float s = sm[i / C4];
    float4 v = ld4<T>(a.x1, k.px0 * k.C + (size_t)i * 4);
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    st4<T>(a.o_x2, k.px0 * k.C + (size_t)i * 4, v);
  }
}

// backward 1: dctx_p = (sum_c dx2 x1) s_p (1 - s_p) -> save; partial dgbar_j = sum_p dctx_p T_jp -> pg row
template <typename T>
__global__ __launch_bounds__(256) void psa_t_sp_bwd_part(const PsaT a) {
  extern __shared__ float sm[];   // dc[chunk] | part[1024]
  __shared__ float M[128], Z[128];
  const Chunk k(a, a.C);
  const int C2 = k.C / 2;
  float* dc = sm;
  float* part = sm + a.chunk;
  if (k.t < C2) {
    M[k.t] = k.sv[k.ly.M + k.t];
    Z[k.t] = k.sv[k.ly.Z + k.t];
  }
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const size_t at = (k.px0 + i) * k.C + 4 * k.l;
    const float ds = lanes_sum(dot4(ld4<T>(a.dx2, at), ld4<T>(a.x1, at)), k.L);
    if (k.l == 0) {
      const float s = k.sv[k.ly.s + k.p0 + i];
      const float d = ds * s * (1.f - s);
      dc[i] = d;
      k.sv[k.ly.dctx + k.p0 + i] = d;
    }
  }
  __syncthreads();
  const int L2 = C2 / 4, PPB2 = 256 / L2, l2 = k.t % L2, pg2 = k.t / L2;
  const float4 m4 = *reinterpret_cast<const float4*>(M + 4 * l2), z4 = *reinterpret_cast<const float4*>(Z + 4 * l2);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = pg2; i < k.np; i += PPB2) {
    const float4 v = ld4<T>(a.theta, (k.px0 + i) * C2 + 4 * l2);
    const float d = dc[i];
    acc.x = fmaf(d, expf(v.x - m4.x) / z4.x, acc.x);
    acc.y = fmaf(d, expf(v.y - m4.y) / z4.y, acc.y);
    acc.z = fmaf(d, expf(v.z - m4.z) / z4.z, acc.z);
    acc.w = fmaf(d, expf(v.w - m4.w) / z4.w, acc.w);
  }
  groups_sum(acc, part, C2, l2, pg2, k.sv + k.ly.pg + k.sp * C2);
}

// backward 2: dgbar from the pg rows; dtheta_jp = T_jp gbar_j (dctx_p - dgbar_j); dx1 = dx2 s_p + (Wg^T dgbar)_c / HW
template <typename T>
__global__ __launch_bounds__(256) void psa_t_sp_bwd_apply(const PsaT a) {
  __shared__ float M[128], Z[128], dg[128], gg[128], vc[256];
  const Chunk k(a, a.C / 2);
  const int C2 = k.C / 2;
  if (k.t < C2) {
    M[k.t] = k.sv[k.ly.M + k.t];
    Z[k.t] = k.sv[k.ly.Z + k.t];
    gg[k.t] = k.sv[k.ly.gbar + k.t];
    float v = 0.f;
    for (int s = 0; s < a.S; ++s) v += k.sv[k.ly.pg + s * C2 + k.t];
    dg[k.t] = v;
    if (k.sp == 0) k.sv[k.ly.dgbar + k.t] = v;
  }
  __syncthreads();
  if (k.t < k.C) {
    float v = 0.f;
    for (int j = 0; j < C2; ++j) v = fmaf(a.wg[j * k.C + k.t], dg[j], v);
    vc[k.t] = v / (float)k.HW;
  }
  __syncthreads();
  const float4 m4 = *reinterpret_cast<const float4*>(M + 4 * k.l), z4 = *reinterpret_cast<const float4*>(Z + 4 * k.l);
  const float4 g4 = *reinterpret_cast<const float4*>(gg + 4 * k.l), d4 = *reinterpret_cast<const float4*>(dg + 4 * k.l);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const float4 v = ld4<T>(a.theta, (k.px0 + i) * C2 + 4 * k.l);
    const float d = k.sv[k.ly.dctx + k.p0 + i];
    float4 o;
    o.x = expf(v.x - m4.x) / z4.x * g4.x * (d - d4.x);
    o.y = expf(v.y - m4.y) / z4.y * g4.y * (d - d4.y);
    o.z = expf(v.z - m4.z) / z4.z * g4.z * (d - d4.z);
    o.w = expf(v.w - m4.w) / z4.w * g4.w * (d - d4.w);
    st4<T>(a.o_dtheta, (k.px0 + i) * C2 + 4 * k.l, o);
  }
  const int C4 = k.C / 4;
  for (int i = k.t; i < k.np * C4; i += 256) {
    const float s = k.sv[k.ly.s + k.p0 + i / C4];
    const float4 b = *reinterpret_cast<const float4*>(vc + 4 * (i % C4));
    float4 v = ld4<T>(a.dx2, k.px0 * k.C + (size_t)i * 4);
    v.x = fmaf(v.x, s, b.x); v.y = fmaf(v.y, s, b.y); v.z = fmaf(v.z, s, b.z); v.w = fmaf(v.w, s, b.w);
    st4<T>(a.o_dx1, k.px0 * k.C + (size_t)i * 4, v);
  }
}

// backward 3: partial dm_c = sum_p dx1 x -> pm row
template <typename T>
__global__ __launch_bounds__(256) void psa_t_pool_bwd_part(const PsaT a) {
  __shared__ float part[1024];
  const Chunk k(a, a.C);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const size_t at = (k.px0 + i) * k.C + 4 * k.l;
    const float4 g = ld4<T>(a.dx1, at), v = ld4<T>(a.x, at);
    acc.x = fmaf(g.x, v.x, acc.x); acc.y = fmaf(g.y, v.y, acc.y); acc.z = fmaf(g.z, v.z, acc.z); acc.w = fmaf(g.w, v.w, acc.w);
  }
  groups_sum(acc, part, k.C, k.l, k.pg, k.sv + k.ly.pm + k.sp * k.C);
}

// backward 4 (one workgroup per image): dm -> sigmoid -> W2, b2 -> relu -> LayerNorm -> W1, b1 -> Wv -> dxbar
__global__ __launch_bounds__(256) void psa_t_mlp_bwd(const PsaT a) {
  __shared__ float dz[256], dhh[32], dh[32], dcx[128];
  __shared__ float mm[2];
  __shared__ float red[4];
  const int C = a.C, C2 = C / 2, C8 = C / 8, t = threadIdx.x, n = blockIdx.x;
  const PsaLay ly(a.HW, C, a.S);
  float* sv = a.save + (size_t)n * ly.img;
  if (t < C) {
    float v = 0.f;
    for (int s = 0; s < a.S; ++s) v += sv[ly.pm + s * C + t];
    const float m = sv[ly.m + t];
    dz[t] = v * m * (1.f - m);
    sv[ly.dz2 + t] = dz[t];
  }
  __syncthreads();
  if (t < C8) {
    float v = 0.f;
    for (int c = 0; c < C; ++c) v = fmaf(a.w2[c * C8 + t], dz[c], v);
    const float dy = sv[ly.r + t] > 0.f ? v : 0.f;
    sv[ly.dy + t] = dy;
    dhh[t] = dy * a.lg[t];
  }
  __syncthreads();
  if (t == 0) {
    float m1 = 0.f, m2 = 0.f;
    for (int k = 0; k < C8; ++k) {
      m1 += dhh[k];
      m2 = fmaf(dhh[k], sv[ly.hhat + k], m2);
    }
    mm[0] = m1 / (float)C8;
    mm[1] = m2 / (float)C8;
  }
  __syncthreads();
  if (t < C8) {
    dh[t] = sv[ly.stat + 2] * (dhh[t] - mm[0] - sv[ly.hhat + t] * mm[1]);
    sv[ly.dh + t] = dh[t];
  }
  __syncthreads();
  if (t < C2) {
    float v = 0.f;
    for (int k = 0; k < C8; ++k) v = fmaf(a.w1[k * C2 + t], dh[k], v);
    dcx[t] = v;
    sv[ly.dctxv + t] = v;
  }
  __syncthreads();
  float prod = 0.f;
  if (t < C) {
    float v = 0.f;
    for (int j = 0; j < C2; ++j) v = fmaf(a.wv[j * C + t], dcx[j], v);
    sv[ly.dxbar + t] = v;
    prod = v * sv[ly.xbar + t];
  }
  const float sada = wg_reduce(prod, false, red);
  if (t == 0) sv[ly.stat + 3] = sada;
}

// backward 5: dq_p = a_p (dxbar.x_p - dxbar.xbar); dx = dx1 m + a_p dxbar + dq_p wq; partial dwq = sum_p dq_p x_p -> pw row
template <typename T>
__global__ __launch_bounds__(256) void psa_t_pool_bwd_apply(const PsaT a) {
  __shared__ float part[1024];
  const Chunk k(a, a.C);
  const float gmax = k.sv[k.ly.stat], gsum = k.sv[k.ly.stat + 1], sada = k.sv[k.ly.stat + 3];
  const float4 dxb = *reinterpret_cast<const float4*>(k.sv + k.ly.dxbar + 4 * k.l);
  const float4 m4 = *reinterpret_cast<const float4*>(k.sv + k.ly.m + 4 * k.l);
  const float4 wq = *reinterpret_cast<const float4*>(a.wq + 4 * k.l);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = k.pg; i < k.np; i += k.PPB) {
    const size_t at = (k.px0 + i) * k.C + 4 * k.l;
    const float4 v = ld4<T>(a.x, at), g = ld4<T>(a.dx1, at);
    const float da = lanes_sum(dot4(dxb, v), k.L);
    const float ap = expf(k.sv[k.ly.q + k.p0 + i] - gmax) / gsum;
    const float dq = ap * (da - sada);
    float4 o;
    o.x = fmaf(dq, wq.x, fmaf(ap, dxb.x, g.x * m4.x));
    o.y = fmaf(dq, wq.y, fmaf(ap, dxb.y, g.y * m4.y));
    o.z = fmaf(dq, wq.z, fmaf(ap, dxb.z, g.z * m4.z));
    o.w = fmaf(dq, wq.w, fmaf(ap, dxb.w, g.w * m4.w));
    st4<T>(a.o_dx, at, o);
    acc.x = fmaf(dq, v.x, acc.x); acc.y = fmaf(dq, v.y, acc.y); acc.z = fmaf(dq, v.z, acc.z); acc.w = fmaf(dq, v.w, acc.w);
  }
  groups_sum(acc, part, k.C, k.l, k.pg, k.sv + k.ly.pw + k.sp * k.C);
}

// backward 6: the nine parameter gradients, summed over the images in image order (one thread per element; dwq,
// which adds N * S rows, takes a workgroup of its own)
__global__ __launch_bounds__(256) void psa_t_params(const PsaT a) {
  const int C = a.C, C2 = C / 2, C8 = C / 8, N = a.N;
  const PsaLay ly(a.HW, C, a.S);
  const size_t img = ly.img;
  const float* sv = a.save;
  float v = 0.f;
  if (blockIdx.x == 0) {
    // dwq: the N * S partial rows, 256 / C row groups side by side, the groups added in group order
    __shared__ float part[256];
    const int t = threadIdx.x, c = t % C, G = 256 / C, R = N * a.S;
#pragma unroll 4
    for (int r = t / C; r < R; r += G) v += sv[(size_t)(r / a.S) * img + ly.pw + (r % a.S) * C + c];
    part[t] = v;
    __syncthreads();
    if (t < C) {
      float s = part[t];
      for (int k = 1; k < G; ++k) s += part[k * C + t];
      a.dwq[t] = s;
    }
    return;
  }
  int i = (blockIdx.x - 1) * 256 + threadIdx.x;
  if (i < C2 * C) {
    const int j = i / C, c = i % C;
    for (int n = 0; n < N; ++n) v = fmaf(sv[n * img + ly.dctxv + j], sv[n * img + ly.xbar + c], v);
    a.dwv[i] = v;
    return;
  }
  i -= C2 * C;
  if (i < C8 * C2) {
    const int k = i / C2, j = i % C2;
    for (int n = 0; n < N; ++n) v = fmaf(sv[n * img + ly.dh + k], sv[n * img + ly.ctx + j], v);
    a.dw1[i] = v;
    return;
  }
  i -= C8 * C2;
  if (i < 3 * C8) {
    const int which = i / C8, k = i % C8;
    for (int n = 0; n < N; ++n) {
      if (which == 0) v += sv[n * img + ly.dh + k];
      else if (which == 1) v = fmaf(sv[n * img + ly.dy + k], sv[n * img + ly.hhat + k], v);
      else v += sv[n * img + ly.dy + k];
    }
    (which == 0 ? a.db1 : which == 1 ? a.dlg : a.dlb)[k] = v;
    return;
  }
  i -= 3 * C8;
  if (i < C * C8) {
    const int c = i / C8, k = i % C8;
    for (int n = 0; n < N; ++n) v = fmaf(sv[n * img + ly.dz2 + c], sv[n * img + ly.r + k], v);
    a.dw2[i] = v;
    return;
  }
  i -= C * C8;
  if (i < C) {
    for (int n = 0; n < N; ++n) v += sv[n * img + ly.dz2 + i];
    a.db2[i] = v;
    return;
  }
  i -= C;
  if (i < C2 * C) {
    const int j = i / C, c = i % C;
    for (int n = 0; n < N; ++n) v = fmaf(sv[n * img + ly.dgbar + j], sv[n * img + ly.x1mean + c], v);
    a.dwg[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------ host side
static int psa_t_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(UDP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return UDP_OK;
}

// workgroups per image and pixels per workgroup: about 512 workgroups per launch, at least 32 pixels each
static int psa_t_split(int n, int hw, int* S, int* chunk) {
  int s = 512 / n;
  if (s > hw / 32) s = hw / 32;
  if (s > 32) s = 32;
  if (s < 1) s = 1;
  int ch = ((hw + s - 1) / s + 3) & ~3;       // a multiple of 4: the LDS rows behind the chunk stay 16-byte aligned
  if (ch > 8192) ch = 8192;                   // the chunk's per-pixel values live in LDS
  s = (hw + ch - 1) / ch;
  if (s > 64) return fail(UDP_ERR_UNSUPPORTED, "PSA training: a %d-pixel map is too large (at most %d)", hw, 64 * 8192);
  *S = s;
  *chunk = ch;
  return UDP_OK;
}

static int psa_t_shape(const char* who, int n, int h, int w, int c) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(UDP_ERR_ARG, "%s: shape n=%d h=%d w=%d c=%d", who, n, h, w, c);
  if ((long)n * h * w * c >= (1L << 31)) return fail(UDP_ERR_UNSUPPORTED, "%s: more than 2^31 elements", who);
  if (n > 65535) return fail(UDP_ERR_UNSUPPORTED, "%s: n=%d (at most 65535 images per call)", who, n);
  // check_psa_c of the inference kernels; training needs theta's C/2 channels to be a whole 16-channel NHWC row
  if (c < 32 || c > 256 || (256 % c) != 0 || (c % 16) != 0)
    return fail(UDP_ERR_UNSUPPORTED, "%s: PSA: C=%d must divide 256 and be a multiple of 16 (training: at least 32)", who, c);
  return UDP_OK;
}

static int psa_t_setup(const char* who, const udp_psa_train_args* g, int dtype, bool need_w, PsaT* a) {
  if (!g) return fail(UDP_ERR_ARG, "%s: null pointer (args)", who);
  const int rc = psa_t_shape(who, g->n, g->h, g->w_px, g->c);
  if (rc) return rc;
  if (dtype == UDP_F16X2) return fail(UDP_ERR_UNSUPPORTED, "%s: split-fp16 storage has no training mode (f32 or bf16)", who);
  if (dtype != UDP_F32 && dtype != UDP_BF16) return fail(UDP_ERR_ARG, "%s: dtype %d", who, dtype);
  if (!g->save) return fail(UDP_ERR_ARG, "%s: null pointer (save)", who);
  if (need_w)
    for (int k = 0; k < 9; ++k)
      if (!g->w[k]) return fail(UDP_ERR_ARG, "%s: null pointer (parameter %d)", who, k);
  memset(a, 0, sizeof(*a));
  a->N = g->n;
  a->HW = g->h * g->w_px;
  a->C = g->c;
  const int rs = psa_t_split(a->N, a->HW, &a->S, &a->chunk);
  if (rs) return rs;
  const size_t need = (size_t)PsaLay(a->HW, a->C, a->S).img * a->N;
  if (g->save_floats < need) return fail(UDP_ERR_WORKSPACE, "%s: save area of %zu floats, %zu needed", who, g->save_floats, need);
  a->wq = g->w[0]; a->wv = g->w[1]; a->w1 = g->w[2]; a->b1 = g->w[3]; a->lg = g->w[4]; a->lb = g->w[5];
  a->w2 = g->w[6]; a->b2 = g->w[7]; a->wg = g->w[8];
  a->save = g->save;
  return UDP_OK;
}

static unsigned psa_t_ew_blocks(const PsaT& a) {
  const long b = ((long)a.N * a.HW * (a.C / 4) + 255) / 256;
  return (unsigned)(b > 4096 ? 4096 : b);
}

}  // namespace udp

using namespace udp;

#define PSA_T_LAUNCH(kernel, grid, lds)                               \
  do {                                                                \
    if (dtype == UDP_F32) kernel<float><<<grid, 256, lds, s>>>(a);    \
    else kernel<__bf16><<<grid, 256, lds, s>>>(a);                    \
  } while (0)

extern "C" size_t udp_psa_train_save_floats(int n, int h, int w, int c) {
  int S, chunk;
  if (psa_t_shape("udp_psa_train_save_floats", n, h, w, c) || psa_t_split(n, h * w, &S, &chunk)) return 0;
  return (size_t)PsaLay(h * w, c, S).img * n;
}

extern "C" int udp_psa_train_fwd_pool(const udp_psa_train_args* g, int dtype, void* stream) {
  PsaT a;
  const int rc = psa_t_setup("udp_psa_train_fwd_pool", g, dtype, true, &a);
  if (rc) return rc;
  if (!g->x || !g->x1) return fail(UDP_ERR_ARG, "udp_psa_train_fwd_pool: null pointer (x, x1)");
  a.x = g->x;
  a.o_x1 = g->x1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.S, a.N);
  PSA_T_LAUNCH(psa_t_pool_part, grid, (a.chunk + 1024) * sizeof(float));
  psa_t_mlp_fwd<<<a.N, 256, 0, s>>>(a);
  PSA_T_LAUNCH(psa_t_scale, psa_t_ew_blocks(a), 0);
  return psa_t_launched("udp_psa_train_fwd_pool");
}

extern "C" int udp_psa_train_fwd_sp(const udp_psa_train_args* g, int dtype, void* stream) {
  PsaT a;
  const int rc = psa_t_setup("udp_psa_train_fwd_sp", g, dtype, false, &a);
  if (rc) return rc;
  if (!g->x1 || !g->theta || !g->x2) return fail(UDP_ERR_ARG, "udp_psa_train_fwd_sp: null pointer (x1, theta, x2)");
  a.x1 = g->x1;
  a.theta = g->theta;
  a.o_x2 = g->x2;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.S, a.N);
  PSA_T_LAUNCH(psa_t_sp_part, grid, 0);
  PSA_T_LAUNCH(psa_t_sp_apply, grid, a.chunk * sizeof(float));
  return psa_t_launched("udp_psa_train_fwd_sp");
}

extern "C" int udp_psa_train_bwd_sp(const udp_psa_train_args* g, int dtype, void* stream) {
  PsaT a;
  const int rc = psa_t_setup("udp_psa_train_bwd_sp", g, dtype, true, &a);
  if (rc) return rc;
  if (!g->dx2 || !g->x1 || !g->theta || !g->dtheta || !g->dx1)
    return fail(UDP_ERR_ARG, "udp_psa_train_bwd_sp: null pointer (dx2, x1, theta, dtheta, dx1)");
  a.dx2 = g->dx2;
  a.x1 = g->x1;
  a.theta = g->theta;
  a.o_dtheta = g->dtheta;
  a.o_dx1 = g->dx1;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.S, a.N);
  PSA_T_LAUNCH(psa_t_sp_bwd_part, grid, (a.chunk + 1024) * sizeof(float));
  PSA_T_LAUNCH(psa_t_sp_bwd_apply, grid, 0);
  return psa_t_launched("udp_psa_train_bwd_sp");
}

extern "C" int udp_psa_train_bwd_pool(const udp_psa_train_args* g, int dtype, void* stream) {
  PsaT a;
  const int rc = psa_t_setup("udp_psa_train_bwd_pool", g, dtype, true, &a);
  if (rc) return rc;
  if (!g->dx1 || !g->x || !g->dx) return fail(UDP_ERR_ARG, "udp_psa_train_bwd_pool: null pointer (dx1, x, dx)");
  a.dx1 = g->dx1;
  a.x = g->x;
  a.o_dx = g->dx;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a.S, a.N);
  PSA_T_LAUNCH(psa_t_pool_bwd_part, grid, 0);
  psa_t_mlp_bwd<<<a.N, 256, 0, s>>>(a);
  PSA_T_LAUNCH(psa_t_pool_bwd_apply, grid, 0);
  return psa_t_launched("udp_psa_train_bwd_pool");
}

extern "C" int udp_psa_train_bwd_params(const udp_psa_train_args* g, int dtype, void* stream) {
  PsaT a;
  const int rc = psa_t_setup("udp_psa_train_bwd_params", g, dtype, false, &a);
  if (rc) return rc;
  for (int k = 0; k < 9; ++k)
    if (!g->dw[k]) return fail(UDP_ERR_ARG, "udp_psa_train_bwd_params: null pointer (gradient %d)", k);
  a.dwq = g->dw[0]; a.dwv = g->dw[1]; a.dw1 = g->dw[2]; a.db1 = g->dw[3]; a.dlg = g->dw[4]; a.dlb = g->dw[5];
  a.dw2 = g->dw[6]; a.db2 = g->dw[7]; a.dwg = g->dw[8];
  const int C = a.C;
  const int total = C / 2 * C + C / 8 * (C / 2) + 3 * (C / 8) + C * (C / 8) + C + C / 2 * C;      // block 0: dwq
  psa_t_params<<<1 + (total + 255) / 256, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
  return psa_t_launched("udp_psa_train_bwd_params");
}
