"""Hand-made micro-programs for op-level parity tests of the inference ops that only whole nets reach.

A ``Micro`` is a udp_hrnet program of 3 to 5 ops: a 3x3 or 7x7 stem first (udp_hrnet_create demands one), the op(s)
under test, and a final 1x1 conv 64 -> 17 into UDP_BUF_OUTPUT over a pre-filled ``[in_h/4, in_w/4, 64]`` buffer.
udp_hrnet_forward neither clears nor otherwise touches the caller's workspace outside its ops (csrc/hrnet.hip:
describe_all only resolves pointers, enqueue_all only launches), so a test

  1. fills the whole workspace with a NaN bit pattern (``POISON16`` in every 16-bit unit: a NaN as fp16, bf16 and fp32),
  2. pre-fills the buffers the op under test reads, encoded in the storage dtype after quantising (``quant``), so
     that device and reference see identical operands,
  3. runs ONE eager forward (use_graph = 0, n < 16: one lane),
  4. decodes the op's output buffer, and checks that every 16-bit unit outside the declared outputs still holds
     what it held before the run (``Micro.assert_untouched``).

Workspace layout (csrc/hrnet.hip, describe_all): with B = n * (2 if flip_test else 1) images, buffer b starts at
byte ``buf_off[b] * B * esize`` where buf_off is the prefix sum of buf_elems rounded up to 64; inside a buffer the
images are packed at H * W * pitch elements (fp32 side rows of the PSA ops: at their row length).

The plain references at the bottom are torch on the CPU in whatever dtype the operands have (the tests evaluate
them in fp64, and in fp32 for the error floor of the tolerance rule ``3 * err_cpu_fp32 + 4 ulp``).
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from udp_pose_amd import _lib, f16x2
from udp_pose_amd.program import encode_weights, storage_bytes

POISON16 = 0x7FC1
# one unit of the storage format relative to the tensor's max
ULP = {"f32": 2.0 ** -23, "f16x2": 2.0 ** -21, "bf16": 2.0 ** -8}


def round_up(x, m):
    return (x + m - 1) // m * m


def buffer_offsets(buf_elems, batch, dtype):
    """Byte offset of every buffer in the workspace + the total bytes (rounded up to 256 as the library does)."""
    es = storage_bytes(dtype)
    offs, run = [], 0
    for e in buf_elems:
        offs.append(run * batch * es)
        run += round_up(e, 64)
    return offs, round_up(run * batch * es, 256)


def quant(t, dtype):
    """The value the device holds after storing ``t`` in ``dtype`` (fp32 result)."""
    t = t.to(torch.float32)
    if dtype == "bf16":
        return t.to(torch.bfloat16).to(torch.float32)
    if dtype == "f16x2":
        return f16x2.decode(f16x2.encode(t))
    return t


def to_units(t_nhwc, dtype):
    """fp32 NHWC [B,h,w,pitch] -> the int16 units of its device form (numpy, flat)."""
    t = t_nhwc.to(torch.float32).contiguous()
    if dtype == "bf16":
        return t.to(torch.bfloat16).view(torch.int16).numpy().reshape(-1)
    if dtype == "f16x2":
        return f16x2.encode(t).view(torch.int16).numpy().reshape(-1)
    return t.numpy().view(np.int16).reshape(-1)


def from_units(u, dtype, shape):
    """int16 units -> fp32 NHWC tensor of ``shape`` = (B, h, w, pitch)."""
    b, h, w, p = shape
    u = np.ascontiguousarray(u)
    if dtype == "bf16":
        return torch.from_numpy(u).view(torch.bfloat16).reshape(b, h, w, p).to(torch.float32)
    if dtype == "f16x2":
        return f16x2.decode(torch.from_numpy(u).view(torch.float16).reshape(b, h, w, 2, p))
    return torch.from_numpy(u.view(np.float32).copy()).reshape(b, h, w, p)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def new_op(kind, **fields):
    """A udp_conv_op with every buffer id defaulting to UDP_BUF_NONE."""
    op = _lib.ConvOp()
    op.kind = kind
    op.in_buf = op.out_buf = op.res_buf = op.chain_buf = _lib.UDP_BUF_NONE
    op.ks = op.stride = 1
    for k, v in fields.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(op, k)[i] = x
        else:
            if not hasattr(op, k):
                raise TypeError("udp_conv_op has no field %s" % k)
            setattr(op, k, v)
    if not op.cout_pad:
        op.cout_pad = round_up(max(op.cout, 1), 32)
    return op


class Micro:
    """One micro-program.  ``buf`` declares buffers, ``fill`` pre-fills them, ``put`` / ``put_conv`` add weights,
    ``add`` appends ops between the stem and the final conv, ``run`` executes, ``read`` / ``read_rows`` decode."""

    def __init__(self, dtype, n, in_h=32, in_w=32, flip=False, stem_ks=3, seed=0, positive_bias=False):
        self.dtype, self.n, self.in_h, self.in_w, self.flip = dtype, n, in_h, in_w, bool(flip)
        self.B = n * (2 if flip else 1)
        self.es = storage_bytes(dtype)
        self.g = torch.Generator().manual_seed(seed)
        self.buf_elems, self.shapes, self.fills, self.ops, self.written = [], [], {}, [], []
        self._blob, self._blob_size = [], 0
        ks = stem_ks
        # stem: non-symmetric random weights, bias either mixed-sign or large enough that the ReLU clips nothing
        self.x = self.randn(n, 3, in_h, in_w)
        self.stem_w = self.randn(64, 3, ks, ks) * float(np.sqrt(2.0 / (3 * ks * ks)))
        self.stem_b = self.randn(64) * 0.5
        if positive_bias:
            xx = torch.cat([self.x, torch.flip(self.x, [3])]).double()
            lo = F.conv2d(xx, self.stem_w.double(), None, stride=2, padding=ks // 2).amin(dim=(0, 2, 3))
            self.stem_b = (0.5 + self.stem_b.abs() - lo).to(torch.float32)
        self.stem_ks = ks
        self.stem_buf = self.buf(in_h // 2, in_w // 2, 64)
        w_off = self.put(self.stem_w.permute(2, 3, 1, 0).contiguous().numpy().tobytes())       # [ky][kx][ci][64]
        b_off = self.put(self.stem_b.numpy().tobytes())
        self.ops.append(new_op(_lib.UDP_OP_STEM if ks == 3 else _lib.UDP_OP_STEM7, ks=ks, stride=2, relu=1, cin=3, cout=64,
                               hin=in_h, win=in_w, hout=in_h // 2, wout=in_w // 2, out_buf=self.stem_buf, w_off=w_off, b_off=b_off))
        self.wrote(self.stem_buf)
        # final conv 64 -> 17 over a pre-filled buffer
        self.head_buf = self.buf(in_h // 4, in_w // 4, 64)
        self.head_x = self.fill(self.head_buf, self.randn(self.B, 64, in_h // 4, in_w // 4))
        self.head_w = quant(self.randn(17, 64, 1, 1) * float(np.sqrt(2.0 / 64)), dtype)
        self.head_b = self.randn(17) * 0.1
        self.head_off = self.put_conv(self.head_w, self.head_b)

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.g, dtype=torch.float32)

    # ---------------------------------------------------------------- buffers
    def buf(self, h, w, pitch):
        self.buf_elems.append(h * w * pitch)
        self.shapes.append((h, w, pitch))
        return len(self.buf_elems) - 1

    def buf_rows(self, floats):
        """A buffer of one fp32 row of ``floats`` numbers per image (PSA side outputs), counted in dtype elements."""
        self.buf_elems.append(floats * (4 // self.es))
        self.shapes.append(("rows", floats))
        return len(self.buf_elems) - 1

    def fill(self, b, t_nchw, coff=0, outside=float("nan")):
        """Pre-fill buffer ``b`` with the quantised ``t_nchw`` in channels [coff, coff + c) and ``outside`` elsewhere;
        returns the quantised tensor (what the reference must use)."""
        h, w, pitch = self.shapes[b]
        q = quant(t_nchw, self.dtype)
        wide = torch.full((t_nchw.shape[0], h, w, pitch), outside, dtype=torch.float32)
        wide[..., coff:coff + q.shape[1]] = nhwc(q)
        self.fills[b] = wide
        return q

    def wrote(self, b, coff=0, c=None):
        """Declare channels [coff, coff + c) of buffer ``b`` (or its whole fp32 row) as written by the program."""
        self.written.append((b, coff, c))

    # ---------------------------------------------------------------- weights
    def put(self, raw):
        off = round_up(self._blob_size, 256)
        self._blob.append((off, raw))
        self._blob_size = off + len(raw)
        return off

    def put_conv(self, w, b, ws=False):
        """[cout, cin, k, k] weight (already quantised) + bias -> blob; returns dict(w_off, b_off, cout_pad, wfmt, wexp)."""
        cout, cin, kh, kw = w.shape
        cp = round_up(cout, 32)
        wp = torch.zeros(kh * kw, cp, cin, dtype=torch.float32)
        wp[:, :cout] = w.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
        bp = torch.zeros(cp, dtype=torch.float32)
        bp[:cout] = b
        wexp = 0
        if ws:
            packed, wexp = f16x2.pack_weights_ws(wp)
            raw = packed.numpy().tobytes()
        else:
            raw = encode_weights(wp, self.dtype)
        return dict(w_off=self.put(raw), b_off=self.put(bp.numpy().tobytes()), cout_pad=cp, wfmt=int(ws), wexp=wexp)

    def add(self, op):
        self.ops.append(op)
        return op

    # ---------------------------------------------------------------- execution
    def create(self):
        h4, w4 = self.in_h // 4, self.in_w // 4
        ops = list(self.ops) + [new_op(_lib.UDP_OP_CONV, cin=64, cout=17, hin=h4, win=w4, hout=h4, wout=w4, in_buf=self.head_buf,
                                       out_buf=_lib.UDP_BUF_OUTPUT, **self.head_off)]
        arr = (_lib.ConvOp * len(ops))(*ops)
        blob = np.zeros(round_up(self._blob_size, 256), dtype=np.uint8)
        for off, raw in self._blob:
            blob[off:off + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        self.blob = torch.from_numpy(blob).cuda()
        bufs = (C.c_int64 * len(self.buf_elems))(*self.buf_elems)
        h = C.c_void_p()
        _lib.check(_lib.lib().udp_hrnet_create(arr, len(ops), bufs, len(self.buf_elems), _lib.ptr(self.blob), self.blob.numel(),
                                               _lib.DTYPES[self.dtype], self.in_h, self.in_w, 17, C.byref(h)))
        return h

    def host_workspace(self):
        """The workspace as int16 units before the run: poison everywhere, the pre-filled buffers in place."""
        self.offs, total = buffer_offsets(self.buf_elems, self.B, self.dtype)
        ws = np.full(total // 2, POISON16, dtype=np.int16)
        for b, wide in self.fills.items():
            u = to_units(wide, self.dtype)
            ws[self.offs[b] // 2:self.offs[b] // 2 + u.size] = u
        return ws

    def run(self):
        """One eager forward.  Returns the udp status code (0 = ok); keeps the workspace before / after and the heat-maps."""
        L = _lib.lib()
        h = self.create()
        try:
            self.before = self.host_workspace()
            need = L.udp_hrnet_workspace_bytes(h, self.n, int(self.flip))
            if self.n < 16:
                assert need == self.before.size * 2, (need, self.before.size * 2)  # the helper's layout arithmetic = the library's
            elif need > self.before.size * 2:      # 16 images or more: room for the two sub-batch lanes of a graph replay,
                pad = np.full(need // 2 - self.before.size, POISON16, dtype=np.int16)      # which the eager forward leaves alone
                self.before = np.concatenate([self.before, pad])
            ws = torch.from_numpy(self.before).cuda()
            x = self.x.cuda()
            heat = torch.full((self.B, 17, self.in_h // 4, self.in_w // 4), float("nan"), device="cuda")
            rc = L.udp_hrnet_forward(h, _lib.ptr(x), self.n, int(self.flip), _lib.ptr(ws), ws.numel() * 2, _lib.ptr(heat), 0,
                                     _lib.stream_ptr())
            self.error = L.udp_last_error().decode() if rc else ""
            torch.cuda.synchronize()
            self.after = ws.cpu().numpy()
            self.heat = heat.cpu()
        finally:
            L.udp_hrnet_destroy(h)
        return rc

    # ---------------------------------------------------------------- read-back
    def _units(self, arr, b):
        h, w, pitch = self.shapes[b]
        per = {"f32": 2, "bf16": 1, "f16x2": 2}[self.dtype]
        cnt = self.B * h * w * pitch * per
        u = arr[self.offs[b] // 2:self.offs[b] // 2 + cnt]
        if self.dtype == "f32":
            return u.reshape(self.B, h, w, pitch, 2)
        if self.dtype == "f16x2":
            return u.reshape(self.B, h, w, 2, pitch).transpose(0, 1, 2, 4, 3)       # channel axis 3, plane last
        return u.reshape(self.B, h, w, pitch, 1)

    def read(self, b, coff=0, c=None):
        """Channels [coff, coff + c) of buffer ``b`` after the run, decoded to fp32 NCHW."""
        h, w, pitch = self.shapes[b]
        per = {"f32": 2, "bf16": 1, "f16x2": 2}[self.dtype]
        u = self.after[self.offs[b] // 2:self.offs[b] // 2 + self.B * h * w * pitch * per]
        t = from_units(u, self.dtype, (self.B, h, w, pitch))
        return nchw(t[..., coff:coff + (c if c is not None else pitch - coff)])

    def read_raw(self, b, coff=0, c=None):
        """The stored 16-bit units of channels [coff, coff + c): int16 [B, h, w, c, units per element]."""
        pitch = self.shapes[b][2]
        return self._units(self.after, b)[:, :, :, coff:coff + (c if c is not None else pitch - coff)]

    def raw_of(self, t_nchw):
        """The units ``read_raw`` returns for a tensor stored as ``t_nchw`` (fp32 values, encoded as the kernels do)."""
        b, c, h, w = t_nchw.shape
        u = to_units(nhwc(t_nchw), self.dtype)
        if self.dtype == "f16x2":
            return u.reshape(b, h, w, 2, c).transpose(0, 1, 2, 4, 3)
        return u.reshape(b, h, w, c, -1)

    def read_rows(self, b, arr=None):
        floats = self.shapes[b][1]
        u = (self.after if arr is None else arr)[self.offs[b] // 2:self.offs[b] // 2 + self.B * floats * 2]
        return torch.from_numpy(np.ascontiguousarray(u).view(np.float32).copy()).reshape(self.B, floats)

    def assert_untouched(self):
        """Every 16-bit unit outside the declared outputs holds what it held before the run, bit for bit: poison in the
        untouched buffers, in the padding, and in the channels outside an output slice; the operands unchanged."""
        mask = np.zeros(self.after.shape, dtype=bool)
        for b, coff, c in self.written:
            if self.shapes[b][0] == "rows":
                mask[self.offs[b] // 2:self.offs[b] // 2 + self.B * self.shapes[b][1] * 2] = True
            else:
                pitch = self.shapes[b][2]
                self._units(mask, b)[:, :, :, coff:coff + (c if c is not None else pitch - coff)] = True
        bad = np.flatnonzero((self.after != self.before) & ~mask)
        assert bad.size == 0, "%d units outside the outputs changed, first at byte %d" % (bad.size, 2 * int(bad[0]))
        return int(mask.sum())

    def check_head(self):
        """The final conv's heat-maps against the fp64 conv, with the shipped conv gate (tests/test_gpu_ops.py)."""
        ref = F.conv2d(self.head_x.double(), self.head_w.double(), self.head_b.double())
        assert not torch.isnan(self.heat).any(), "heat-maps not fully written"
        err = float((self.heat.double() - ref).abs().max())
        assert err <= conv_tol(self.dtype, ref), err
        return err


def conv_tol(dtype, ref):
    """The gate of test_fused_conv_matches_torch_fp32: 1e-4 (f32) / 2e-5 (split fp16) / 6e-3 (bf16) x scale."""
    scale = max(1.0, float(ref.abs().max()))
    return {"f32": 1e-4, "f16x2": 2e-5, "bf16": 6e-3}[dtype] * scale


def parity(name, got, ref64, ref32, ulp):
    """``|got - ref64| <= 3 * err_cpu_fp32 + 4 ulp`` (errors relative to the tensor's max); prints and returns the errors."""
    ex = ref64.double()
    mx = float(ex.abs().max())
    assert mx > 0, "%s: the reference is zero, the gate would be vacuous" % name
    assert not torch.isnan(got).any(), "%s: output not fully written" % name
    e_hip = float((got.double() - ex).abs().max()) / mx
    e_cpu = float((ref32.double() - ex).abs().max()) / mx
    print("%-40s err hip %.3g  cpu fp32 %.3g  (gate %.3g)" % (name, e_hip, e_cpu, 3 * e_cpu + 4 * ulp))
    return e_hip, e_cpu, 3 * e_cpu + 4 * ulp


# -------------------------------------------------------------------- references (dtype-generic torch, CPU)
def ref_maxpool(x):
    return F.max_pool2d(x, 3, 2, 1)


def ref_bilinear(x, hout, wout):
    return F.interpolate(x, size=(hout, wout), mode="bilinear", align_corners=True)


def ref_conv(x, w, b, stride=1, res=None, relu=False):
    y = F.conv2d(x, w.to(x.dtype), b.to(x.dtype), stride=stride, padding=w.shape[2] // 2)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def ref_fuse(x, res, ups, relu):
    """out = act(in + res + sum_k nearest_up(up_k, 2^shift_k)), added in that order."""
    y = x + res
    for t, s in ups:
        y = y + F.interpolate(t, scale_factor=2 ** s, mode="nearest")
    return F.relu(y) if relu else y


PSA_KEYS = ("wq", "wv", "w1", "b1", "ln_g", "ln_b", "w2", "b2", "wg")     # the fp32 parameter block of csrc/psa.hip, in order


def psa_block_bytes(P):
    return torch.cat([P[k].to(torch.float32).reshape(-1) for k in PSA_KEYS]).numpy().tobytes()


def psa_pool(x, P):
    """{sum_p softmax_HW(wq.x)_p x_p, mean_p x_p}: [N, 2C]."""
    n, c, h, w = x.shape
    xf = x.reshape(n, c, h * w)
    q = torch.softmax(torch.einsum("c,ncp->np", P["wq"].to(x.dtype), xf), dim=1)
    return torch.cat([torch.einsum("np,ncp->nc", q, xf), xf.mean(dim=2)], dim=1)


def psa_mlp(pooled, P):
    """{m = sigmoid(W2 relu(LN(W1 Wv xbar + b1)) + b2), gbar = Wg (m * xmean)}: [N, C + C/2]."""
    d = pooled.dtype
    c = pooled.shape[1] // 2
    xbar, xmean = pooled[:, :c], pooled[:, c:]
    hid = (xbar @ P["wv"].to(d).t()) @ P["w1"].to(d).t() + P["b1"].to(d)
    hid = F.layer_norm(hid, [c // 8], P["ln_g"].to(d), P["ln_b"].to(d), 1e-5)
    m = torch.sigmoid(F.relu(hid) @ P["w2"].to(d).t() + P["b2"].to(d))
    return torch.cat([m, (m * xmean) @ P["wg"].to(d).t()], dim=1)


def psa_scale(x, mask):
    return x * mask[:, :x.shape[1], None, None]


def psa_sp(theta, x1, mask):
    """x1 * sigmoid(sum_j gbar_j softmax_HW(theta_j))."""
    n, c2, h, w = theta.shape
    sm = torch.softmax(theta.reshape(n, c2, h * w), dim=2)
    ctx = torch.einsum("nj,njp->np", mask[:, 2 * c2:], sm)
    return x1 * torch.sigmoid(ctx).reshape(n, 1, h, w)


def psa_block(x, P, wt):
    """The whole PSA_s block (include/udp_pose_hip.h, UDP_OP_PSA_*): POOL -> MLP -> SCALE -> theta = Wt x1 -> SP."""
    mask = psa_mlp(psa_pool(x, P), P)
    x1 = psa_scale(x, mask)
    return psa_sp(F.conv2d(x1, wt.to(x.dtype)), x1, mask)


def psa_inputs(c, h, w, n, spread=4.0, seed=0):
    """x ~ N(0,1), theta and the parameter block of one PSA case.  ``spread``: the approximate max - min of the two
    soft-maxes' logits (wq.x over the pixels, theta_j over the pixels): logits ~ N(0, s^2) span about 5 s.  Wg is scaled
    so that the spatial gate's argument sum_j gbar_j softmax(theta_j)_p is O(1) and not the O(HW^-1.5) that unit weights
    give (gbar ~ |Wg| sqrt(C) / (2 sqrt(HW)), soft-max weights ~ 1 / HW): a flat gate of 0.5 would hide the op
    (tests/test_microprog_cpu.py checks the resulting range)."""
    g = torch.Generator().manual_seed(1000 * c + 10 * h + w + seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    s = spread / 5.0
    wq = r(c)
    P = dict(wq=wq * (s / float(wq.norm())), wv=r(c // 2, c) / np.sqrt(c), w1=r(c // 8, c // 2) / np.sqrt(c // 2), b1=0.1 * r(c // 8),
             ln_g=1.0 + 0.1 * r(c // 8), ln_b=0.1 * r(c // 8), w2=r(c, c // 8) / np.sqrt(c // 8), b2=0.1 * r(c),
             wg=r(c // 2, c) * (1.2 * (h * w) ** 1.5 / c))
    return r(n, c, h, w), r(n, c // 2, h, w) * s, P
