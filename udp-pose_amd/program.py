"""The net-agnostic half of the host compiler: a ``Program`` is a list of op records (one ``udp_conv_op`` of
include/udp_pose_hip.h per fused launch), a packed weight blob and an activation-buffer assignment.

    out = act( conv(in) + bias [+ res] [+ sum_k nearest_up(up_k)] )

The planners (hrnet_plan.HRNetProgram, rsn_plan.RSNProgram, resnet_plan.PoseResNetProgram) derive from it and
supply ``_build()``: they walk their reference graph and call the one fold (``_fold``), the one packer (``_pack``)
and the one op emitter (``_emit``) here; the polarized self-attention block (``_psa``) is here too, for the two nets
that carry one (pose_hrnet_psa, pose_resnet_psa).

* BatchNorm(eval) is folded into the conv: w' = w * gamma/sqrt(var+eps),
  b' = beta - mean*gamma/sqrt(var+eps), computed in fp64, stored fp32 / bf16.
* Activation buffers are assigned by a linear scan over tensor lifetimes.
"""
import os

import numpy as np
import torch

from . import _lib

BN_EPS = 1e-5


class _T:
    """An activation tensor (NHWC, per image) in SSA form."""
    __slots__ = ("id", "c", "h", "w")

    def __init__(self, i, c, h, w):
        self.id, self.c, self.h, self.w = i, c, h, w

    @property
    def elems(self):
        return self.c * self.h * self.w


class _V:
    """Channels [coff, coff + c) of tensor ``t`` (a channel-slice view: udp_conv_op.in_coff / res_coff + pitch)."""
    __slots__ = ("t", "coff", "c")

    def __init__(self, t, coff, c):
        self.t, self.coff, self.c = t, coff, c

    @property
    def h(self):
        return self.t.h

    @property
    def w(self):
        return self.t.w


def _round_up(x, m):
    return (x + m - 1) // m * m


DTYPES = ("f32", "bf16", "f16x2")
F16X2_LO_SCALE = 2048.0          # csrc/conv.hip kLoScale


def encode_weights(wp, dtype):
    """[taps][cout_pad][cin] fp32 -> bytes in the storage dtype.  f16x2: rows of [cin hi][cin lo] fp16 with
    w ~= hi + lo * 2^-11 (include/udp_pose_hip.h, UDP_F16X2); a folded weight beyond fp16's range is refused."""
    if dtype == "bf16":
        return wp.to(torch.bfloat16).contiguous().view(torch.uint8).numpy().tobytes()
    if dtype == "f16x2":
        if not bool(torch.isfinite(wp).all()):                  # (a NaN compares False with every bound below)
            raise ValueError("f16x2 storage: non-finite weight")
        if wp.numel() and float(wp.abs().max()) >= 32768.0:
            raise ValueError("f16x2 storage: a BatchNorm-folded weight of magnitude %g exceeds the fp16 range"
                             % float(wp.abs().max()))
        hi = wp.to(torch.float16)
        lo = ((wp - hi.to(torch.float32)) * F16X2_LO_SCALE).to(torch.float16)
        return torch.stack([hi, lo], dim=2).contiguous().view(torch.uint8).numpy().tobytes()
    return wp.contiguous().numpy().tobytes()


def storage_bytes(dtype):
    """Bytes per stored activation / weight element."""
    return 2 if dtype == "bf16" else 4


class Program:
    """The compiled program: ops (ctypes array), buffer sizes, packed weights.  Subclasses emit the ops in ``_build()``
    and set ``out_channels``."""

    def __init__(self, state_dict, in_h, in_w, dtype="f32"):
        if dtype not in DTYPES:
            raise ValueError("dtype must be one of %s" % (DTYPES,))
        if in_h % 32 or in_w % 32:
            raise ValueError("input %dx%d must be a multiple of 32" % (in_h, in_w))
        self.sd = {k[7:] if k.startswith("module.") else k: v for k, v in state_dict.items()}
        self.dtype = dtype
        self.in_h, self.in_w = in_h, in_w
        # split-fp16 convs on the weight-stationary kernel (fragment-major weights, udp_conv_op.wfmt = 1)
        # (UDP_POSE_WS=0: the LDS-staged conv_mfma_kernel<H2> instead -- A/B knob)
        self.use_ws = dtype == "f16x2" and os.environ.get("UDP_POSE_WS", "1") != "0"
        self._tensors = []
        self._ops = []          # dicts with _T references
        self._blob = []         # list of (offset, np.ndarray uint8)
        self._blob_size = 0
        self._build()
        self._assign_buffers()

    # ------------------------------------------------------------------ weights
    def _put(self, arr_bytes):
        off = _round_up(self._blob_size, 256)
        self._blob.append((off, arr_bytes))
        self._blob_size = off + len(arr_bytes)
        return off

    def _fold(self, conv, bn=None, axis=0, eps=BN_EPS):
        """``conv`` (+ its bias, if the state_dict has one) + BatchNorm(eval) ``bn`` folded in fp64 -> fp32 (weight, bias).
        ``axis``: the weight's output-channel dimension (1 for a ConvTranspose2d's [cin, cout, k, k]); ``eps``: the
        BatchNorm's (torchvision's MobileNetV3 backbone builds its norms with 1e-3)."""
        f64 = lambda k: self.sd[k].detach().to(torch.float64).cpu()
        w = f64(conv + ".weight")
        b = f64(conv + ".bias") if self.sd.get(conv + ".bias") is not None else torch.zeros(w.shape[axis], dtype=torch.float64)
        if bn is not None:
            s = f64(bn + ".weight") / torch.sqrt(f64(bn + ".running_var") + eps)
            w = w * s.reshape([-1 if d == axis else 1 for d in range(4)])
            b = (b - f64(bn + ".running_mean")) * s + f64(bn + ".bias")
        return w.to(torch.float32), b.to(torch.float32)

    def _pack(self, w, b, ws=False, out_map=None, in_map=None, cout_t=None, cin_t=None):
        """Folded [cout, cin, k, k] weight + bias -> blob, as [k*k][cout_pad][cin_t] and [cout_pad].  ``out_map`` /
        ``in_map`` scatter the real channels to positions of a wider (``cout_t`` / ``cin_t``) zero-filled layout.  ``ws``:
        the fragment-major split-fp16 layout of the weight-stationary kernels (udp_conv_op.wfmt = 1), scaled by 2^wexp
        so that any finite magnitude fits.  Returns (w_off, b_off, cout_t, cin_t, k, cout_pad, wexp)."""
        cout, cin, kh, kw = w.shape
        cout_t, cin_t = cout_t or cout, cin_t or cin
        oi = torch.arange(cout) if out_map is None else torch.tensor(out_map)
        ii = torch.arange(cin) if in_map is None else torch.tensor(in_map)
        cout_pad = _round_up(cout_t, 32)
        wp = torch.zeros(kh * kw, cout_pad, cin_t, dtype=torch.float32)
        wp[:, oi[:, None], ii[None, :]] = w.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin)
        bp = torch.zeros(cout_pad, dtype=torch.float32)
        bp[oi] = b
        wexp = 0
        if ws:
            from .f16x2 import pack_weights_ws
            packed, wexp = pack_weights_ws(wp)
            wbytes = packed.numpy().tobytes()
        else:
            wbytes = encode_weights(wp, self.dtype)
        return self._put(wbytes), self._put(bp.numpy().tobytes()), cout_t, cin_t, kh, cout_pad, wexp

    # ------------------------------------------------------------------ emission
    def _new(self, c, h, w):
        t = _T(len(self._tensors), c, h, w)
        self._tensors.append(t)
        return t

    def _emit(self, kind, name, x, out, **fields):
        """Append one op record -- the only place one is made, so every field ops_array() reads is here with its
        default.  ``x`` / ``out``: the input / output tensors (None: the network input / the heat-map output, or no
        plain output at all with ``no_out``); geometry and channel counts default to theirs."""
        op = dict(kind=kind, name=name, inp=x, out=out, res=None, ups=[], ks=1, stride=1, relu=0,
                  cin=x.c if x is not None else 3, cout=out.c if out is not None else 0, cout_pad=None,
                  hin=x.h if x is not None else self.in_h, win=x.w if x is not None else self.in_w,
                  hout=out.h if out is not None else 0, wout=out.w if out is not None else 0,
                  w_off=0, b_off=0, w2_off=0, b2_off=0, group=0, wfmt=0, wexp=0,
                  in_coff=0, in_pitch=0, out_coff=0, out_pitch=0, res_coff=0, res_pitch=0, res_c=None,
                  chain_out=None, chain_cout=0, chain_relu=0, chain_wexp=0, chain_name=None,
                  out2=[], add2=[], no_out=False, heads=0)
        unknown = set(fields) - set(op)
        if unknown:
            raise TypeError("%s: unknown op fields %s" % (name, sorted(unknown)))
        op.update(fields)
        op["relu"] = int(op["relu"])
        if op["cout_pad"] is None:
            op["cout_pad"] = _round_up(op["cout"], 32)
        self._ops.append(op)
        return op

    def _stem(self, kind, conv, bn, ks, name=None):
        """The stem: stride-2 conv + BatchNorm + ReLU on the NCHW fp32 input (VALU kernels), weights fp32
        [ky][kx][ci][cout]."""
        w, b = self._fold(conv, bn)
        if tuple(w.shape) != (64, 3, ks, ks):
            raise ValueError("%s.weight must be [64,3,%d,%d]" % (conv, ks, ks))
        w_off = self._put(w.permute(2, 3, 1, 0).contiguous().numpy().tobytes())
        b_off = self._put(b.numpy().tobytes())
        out = self._new(64, self.in_h // 2, self.in_w // 2)
        self._emit(kind, name or conv, None, out, ks=ks, stride=2, relu=1, w_off=w_off, b_off=b_off)
        return out

    def _conv(self, x, conv, bn, stride=1, relu=True, res=None, ups=(), to_output=False, group=0, in_coff=None,
              into=None, plus=None, chain=None):
        """One conv + folded BatchNorm (+ residual / upsampled addends, + ReLU), named by its state_dict keys
        (``bn`` None: no BatchNorm).  ``in_coff``: read the ``cin`` channels
        of ``x`` that start there (a channel-slice view); ``into = (tensor, coff)``: write the output into that slice of
        an existing wider tensor; ``plus = (conv', bn')``: a second conv + BatchNorm of the same geometry whose input
        channels FOLLOW this conv's in ``x`` and whose result is summed in -- one conv over the concatenated channels
        with the weights side by side and the biases added; ``chain = (conv'', bn'')``: a 1x1 conv + BatchNorm + ReLU
        applied to this conv's result in the same launch (udp_conv_op.chain_cout) -- returns ``(out, chained out)``."""
        # (the output conv writes NCHW fp32 from the weight-stationary kernel too; UDP_POSE_HEAD_WS=0: the LDS-staged kernel)
        head_ws = to_output and stride == 1 and os.environ.get("UDP_POSE_HEAD_WS", "1") != "0"
        ws = self.use_ws and (not to_output or head_ws) and int(self.sd[conv + ".weight"].shape[2]) in (1, 3) and stride in (1, 2)
        w, b = self._fold(conv, bn)
        for other in ([plus] if isinstance(plus, tuple) else (plus or [])):      # conv(x_a) + conv'(x_b) = one conv over [x_a | x_b]
            w2, b2 = self._fold(*other)
            if w2.shape[0] != w.shape[0] or w2.shape[2:] != w.shape[2:]:
                raise ValueError("%s + %s: different geometry" % (conv, other[0]))
            w, b = torch.cat([w, w2], dim=1), b + b2
        w_off, b_off, cout, cin, ks, cout_pad, wexp = self._pack(w, b, ws)
        if isinstance(x, _V):                    # ``x`` / ``res`` may be channel-slice views (_V) of wider tensors
            if cin != x.c:
                raise ValueError("%s: weight expects %d input channels, view has %d" % (conv, cin, x.c))
            x, in_coff = x.t, x.coff
        res_view = res if isinstance(res, _V) else None
        if res_view is not None:
            res = res_view.t
        if cin != x.c and in_coff is None:
            raise ValueError("%s: weight expects %d input channels, tensor has %d" % (conv, cin, x.c))
        pad = ks // 2
        ho = (x.h + 2 * pad - ks) // stride + 1
        wo = (x.w + 2 * pad - ks) // stride + 1
        out = None if to_output else (into[0] if into else self._new(cout, ho, wo))
        views = {}
        if in_coff is not None:
            if in_coff + cin > x.c:
                raise ValueError("%s: channels %d..%d of a %d-channel tensor" % (conv, in_coff, in_coff + cin, x.c))
            views.update(in_coff=in_coff, in_pitch=x.c)
        if res_view is not None:
            if res_view.c != cout or (res.h, res.w) != (ho, wo):
                raise ValueError("%s: residual view does not match the output" % conv)
            views.update(res_coff=res_view.coff, res_pitch=res.c, res_c=cout)
        if into:
            if (out.h, out.w) != (ho, wo) or into[1] + cout > out.c:
                raise ValueError("%s: output slice does not fit its tensor" % conv)
            views.update(out_coff=into[1], out_pitch=out.c)
        z = None
        if chain is not None:
            from .f16x2 import pack_weights_ws
            w2, b2 = self._fold(*chain)
            c2 = int(w2.shape[0])
            if not ws or ks != 1 or tuple(w2.shape[1:]) != (cout, 1, 1) or cout_pad != cout or c2 % 32:
                raise ValueError("%s -> %s: not a chain of split-fp16 1x1 convs" % (conv, chain[0]))
            packed, wexp2 = pack_weights_ws(w2.reshape(1, c2, cout))
            z = self._new(c2, ho, wo)
            views.update(chain_out=z, chain_cout=c2, chain_relu=1, chain_wexp=wexp2, w2_off=self._put(packed.numpy().tobytes()),
                         b2_off=self._put(b2.numpy().tobytes()), chain_name=chain[0])
        self._emit(_lib.UDP_OP_CONV, conv, x, out, ks=ks, stride=stride, relu=relu, cin=cin, cout=cout, cout_pad=cout_pad,
                   hout=ho, wout=wo, res=res, ups=list(ups), w_off=w_off, b_off=b_off, group=group, wfmt=int(ws), wexp=wexp,
                   **views)
        return (out, z) if chain is not None else out

    def _deconv(self, x, d):
        """deconv_layers[3d] (ConvTranspose2d, [cin, cout, 4, 4], bias if DECONV_WITH_BIAS) + [3d+1] (BatchNorm) + ReLU:
        the BatchNorm scale folds along dim 1 (the output channels), the deconv bias into the BatchNorm bias."""
        q = "deconv_layers.%d" % (3 * d)
        w, b = self._fold(q, "deconv_layers.%d" % (3 * d + 1), axis=1)
        cin, cout = int(w.shape[0]), int(w.shape[1])
        if cin != x.c:
            raise ValueError("%s expects %d input channels, got %d" % (q, cin, x.c))
        cout_pad = _round_up(cout, 32)
        from .f16x2 import deconv_phase_taps, pack_deconv_weights_ws
        wexp = 0
        if self.dtype == "f16x2":
            packed, wexp = pack_deconv_weights_ws(w, cout_pad)
            w_off = self._put(packed.numpy().tobytes())
        else:
            w_off = self._put(encode_weights(deconv_phase_taps(w, cout_pad), self.dtype))
        bp = torch.zeros(cout_pad, dtype=torch.float32)
        bp[:cout] = b
        out = self._new(cout, 2 * x.h, 2 * x.w)
        self._emit(_lib.UDP_OP_DECONV, q, x, out, ks=4, stride=2, relu=1, w_off=w_off,
                   b_off=self._put(bp.numpy().tobytes()), wfmt=int(self.dtype == "f16x2"), wexp=wexp)
        return out

    def _deconv_head(self, x, name, n_deconv):
        """The SimpleBaseline head every deconv-head net of the reference shares (pose_resnet.py:155-193, :128-136;
        pose_shufflenetv2_10x.py, pose_shufflenetv2_plus.py and pose_mobilenetv3_small.py repeat it): ``n_deconv`` x
        [ConvTranspose2d(4, 2, 1) + BatchNorm + ReLU] = one UDP_OP_DECONV each, then the biased 1x1 / 3x3
        ``final_layer`` writing the NCHW fp32 heat-maps.  Sets ``out_channels``."""
        for d in range(n_deconv):
            x = self._deconv(x, d)
        if (x.h, x.w) != (self.in_h // 4, self.in_w // 4):
            raise ValueError("%s: heat-maps at %dx%d, expected %dx%d" % (name, x.h, x.w, self.in_h // 4, self.in_w // 4))
        self._conv(x, "final_layer", None, relu=False, to_output=True)
        self.out_channels = self._ops[-1]["cout"]

    def _psa(self, x, p):
        """PSA_s (PSA.py:190-269) as POOL -> MLP -> SCALE -> 1x1 conv (theta) -> SP; see csrc/psa.hip."""
        sd, C = self.sd, x.c
        if (256 % C or C % 16) and C != 512:
            raise ValueError("%s: PSA needs a channel count that divides 256, or 512 (got %d)" % (p, C))
        f32 = lambda k: sd[p + k].detach().to(torch.float32).cpu().reshape(-1)
        block = torch.cat([f32(".conv_q_right.weight"), f32(".conv_v_right.weight"), f32(".conv_up.0.weight"),
                           f32(".conv_up.0.bias"), f32(".conv_up.1.weight"), f32(".conv_up.1.bias"),
                           f32(".conv_up.3.weight"), f32(".conv_up.3.bias"), f32(".conv_q_left.weight")])
        want = C + C // 2 * C + C // 8 * (C // 2) + 3 * (C // 8) + C * (C // 8) + C + C // 2 * C
        if block.numel() != want:
            raise ValueError("%s: PSA parameter shapes do not match planes=%d" % (p, C))
        w_off = self._put(block.numpy().tobytes())
        f = 4 // storage_bytes(self.dtype)                               # fp32 side rows, counted in dtype elements
        geom = dict(cin=C, cout=C, hin=x.h, win=x.w, hout=x.h, wout=x.w, w_off=w_off)       # of the attended map, whatever the operand
        pooled = self._new(2 * C * f, 1, 1)
        self._emit(_lib.UDP_OP_PSA_POOL, p + ".pool", x, pooled, **geom)
        mask = self._new((C + C // 2) * f, 1, 1)
        self._emit(_lib.UDP_OP_PSA_MLP, p + ".mlp", pooled, mask, **geom)
        x1 = self._new(C, x.h, x.w)
        self._emit(_lib.UDP_OP_PSA_SCALE, p + ".scale", x, x1, res=mask, **geom)
        theta = self._conv(x1, p + ".conv_v_left", None, relu=False)
        x2 = self._new(C, x.h, x.w)
        self._emit(_lib.UDP_OP_PSA_SP, p + ".sp", theta, x2, res=x1, ups=[(mask, 0)], **dict(geom, cin=C // 2))
        return x2

    # ------------------------------------------------------------------ lanes + buffers
    @staticmethod
    def _reads(op):
        """Every tensor the op reads (add2: the addends of its second outputs, udp_conv_op.n_out2)."""
        return [t for t in [op["inp"], op["res"]] + [u for u, _ in op["ups"]] + [a for a, _ in op["add2"]] if t is not None]

    @staticmethod
    def _own_writes(op):
        """The tensors that only this op writes besides ``out``: its second outputs and its chained output."""
        return [t for t, _ in op["out2"]] + ([op["chain_out"]] if op["chain_out"] is not None else [])

    def _assign_buffers(self):
        """Linear-scan buffer assignment plus the cross-lane dependency lists.

        Lane = resolution level of the op's output (HRNet branch): ops of different lanes may run
        concurrently, ordered only by (a) producer -> consumer edges and (b) buffer reuse: the new
        writer of a physical buffer waits for the previous tenant's writer and readers.  Same-lane
        predecessors are ordered by the stream itself and are not listed."""
        h4 = self.in_h // 4
        for op in self._ops:
            lvl = 0
            while (h4 >> lvl) > op["hout"] and lvl < _lib.MAX_LANES - 1:
                lvl += 1
            op["lane"] = lvl
        self._ops[0]["lane"] = 0
        producer = {}
        readers = {}
        for idx, op in enumerate(self._ops):
            if op["out"] is not None:
                prev = producer.get(op["out"].id)
                if prev is not None:
                    # ``producer`` keeps only the LAST writer of a tensor written in slices (the earlier ones count as
                    # its readers): whoever waits for that one is ordered after the others by their common lane alone
                    if self._ops[prev]["lane"] != op["lane"]:
                        raise RuntimeError("%s (lane %d) and %s (lane %d) write slices of one tensor from different lanes"
                                           % (self._ops[prev]["name"], self._ops[prev]["lane"], op["name"], op["lane"]))
                    readers.setdefault(op["out"].id, []).append(prev)
                producer[op["out"].id] = idx
            for t in self._own_writes(op):
                producer[t.id] = idx
            for t in self._reads(op):
                readers.setdefault(t.id, []).append(idx)
        last_use = {tid: max(r) for tid, r in readers.items()}
        free = {}             # elems -> [(buffer id, previous tenant tensor id)]
        self.buf_elems = []
        phys = {}
        pending = []
        for idx, op in enumerate(self._ops):
            deps = set()
            for t in self._reads(op):
                if t.id in producer:
                    deps.add(producer[t.id])
            out = op["out"]
            if out is not None and out.id in phys:
                deps.add(producer[out.id])      # later slice of a concat buffer: ordered after its other writers
                out = None
            for out in ([out] if out is not None else []) + self._own_writes(op):
                pool = free.get(out.elems, [])
                pick = None
                for k in range(len(pool) - 1, -1, -1):
                    b, old = pool[k]
                    hazard = {producer[old]} | set(readers.get(old, []))
                    cross = {d for d in (deps | hazard) if self._ops[d]["lane"] != op["lane"]}
                    if len(cross) <= _lib.MAX_WAIT:
                        pick = k
                        deps |= hazard
                        break
                if pick is not None:
                    phys[out.id] = pool.pop(pick)[0]
                else:
                    phys[out.id] = len(self.buf_elems)
                    self.buf_elems.append(out.elems)
            cross = sorted(d for d in deps if self._ops[d]["lane"] != op["lane"])
            if len(cross) > _lib.MAX_WAIT:
                raise RuntimeError("op %s has %d cross-lane dependencies (max %d)" % (op["name"], len(cross), _lib.MAX_WAIT))
            op["wait"] = cross
            # members of a launch group run concurrently: a buffer one of them reads for the last time
            # must not be handed to a later member of the same group
            g = op["group"]
            nxt = self._ops[idx + 1]["group"] if idx + 1 < len(self._ops) else 0
            for t in self._reads(op):
                if last_use.get(t.id) == idx and t.id in phys:
                    pending.append((t.elems, phys[t.id], t.id))
                    last_use[t.id] = -1
            if g == 0 or nxt != g:
                for elems, b, tid in pending:
                    free.setdefault(elems, []).append((b, tid))
                pending = []
        self._phys = phys

    # ------------------------------------------------------------------ output
    def ops_array(self):
        arr = (_lib.ConvOp * len(self._ops))()
        buf = lambda t, none=_lib.UDP_BUF_NONE: none if t is None else self._phys[t.id]
        for o, op in zip(arr, self._ops):
            for f in ("kind", "ks", "stride", "relu", "cin", "cout", "cout_pad", "hin", "win", "hout", "wout", "w_off", "b_off",
                      "in_coff", "in_pitch", "out_coff", "out_pitch", "res_coff", "res_pitch", "w2_off", "b2_off", "group",
                      "wfmt", "wexp", "chain_cout", "chain_relu", "chain_wexp", "lane"):
                setattr(o, f, op[f])
            o.in_buf, o.res_buf = buf(op["inp"]), buf(op["res"])
            o.out_buf = buf(op["out"], _lib.UDP_BUF_NONE if op["no_out"] else _lib.UDP_BUF_OUTPUT)
            o.chain_buf = buf(op["chain_out"], 0)
            o.n_out2 = len(op["out2"])
            for k, ((t2, c2), (ta, ca)) in enumerate(zip(op["out2"], op["add2"])):
                o.out2_buf[k], o.out2_coff[k], o.out2_pitch[k] = self._phys[t2.id], c2, t2.c
                o.add2_buf[k], o.add2_coff[k], o.add2_pitch[k] = self._phys[ta.id], ca, ta.c
            o.n_wait = len(op["wait"])
            for k, d in enumerate(op["wait"]):
                o.wait_op[k] = d
            o.n_up = len(op["ups"])
            for u, (t, s) in enumerate(op["ups"]):
                o.up_buf[u], o.up_shift[u] = self._phys[t.id], s
            if op["heads"]:
                o.up_shift[0] = op["heads"]      # UDP_OP_MHATTN: the head count (n_up == 0 leaves the field free)
        return arr

    def weight_blob(self):
        blob = np.zeros(_round_up(self._blob_size, 256), dtype=np.uint8)
        for off, b in self._blob:
            blob[off:off + len(b)] = np.frombuffer(b, dtype=np.uint8)
        return blob

    def describe(self):
        return [(op["name"], op["kind"], op["ks"], op["stride"], op["cin"], op["cout"], op["hout"], op["wout"])
                for op in self._ops]

    def macs_per_image(self):
        def taps(op):                # multiply-accumulates per (input channel, output element)
            if op["kind"] == _lib.UDP_OP_DECONV:
                return 4             # ConvTranspose2d(k=4, s=2): an output pixel sees 2x2 of the 16 taps
            return op["ks"] ** 2 * (2 if op["kind"] == _lib.UDP_OP_BLOCK else 1)
        return sum((taps(op) * op["cin"] + op["chain_cout"]) * op["cout"] * op["hout"] * op["wout"] for op in self._ops
                   if op["kind"] in (_lib.UDP_OP_STEM, _lib.UDP_OP_CONV, _lib.UDP_OP_STEM7, _lib.UDP_OP_BLOCK, _lib.UDP_OP_DECONV))

    def activation_elems_per_image(self):
        """Layer-wise algorithmic traffic: every op reads its inputs once and writes its output once."""
        n = 0
        for op in self._ops:
            n += op["hin"] * op["win"] * op["cin"] + op["hout"] * op["wout"] * op["cout"]
            if op["res"] is not None:
                n += op["res"].elems // op["res"].c * (op["res_c"] or op["res"].c)
            n += sum(t.elems for t, _ in op["ups"])
            if op["chain_out"] is not None:
                n += op["chain_out"].elems
        return n
