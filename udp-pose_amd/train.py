"""Training step on MI355X: the host side of deep_hrnet/lib/core/function.py:38-77.

``Trainer`` owns the parameters (one flat fp32 buffer in ``named_parameters()`` order, so
the gradient of the whole model is ONE contiguous bucket for the RCCL all-reduce), keeps the tape
of the train-mode forward its subclass runs op by op through the C ABI, walks it backwards
(``loss.backward()``), then ``udp_adam_step`` (``optimizer.step()``).  ``HRNetTrainer`` is the graph of
lib/models/pose_hrnet.py:436-471 (and pose_hrnet_psa), ``PoseResNetTrainer`` that of lib/models/pose_resnet.py:195-209,
``ShuffleNetV2Trainer`` / ``ShuffleNetV2DeconvTrainer`` those of the two ShuffleNetV2 pose nets, ``MobileNetV3Trainer`` /
``MobileNetV3DeconvTrainer`` those of the two MobileNetV3-small pose nets, ``MobileViTv2Trainer`` that of
pose_mobilevitv2_pixel_shuffle.
torch is used for device memory only; every arithmetic step is a kernel of libudp_pose_hip.so.

Reference contract mirrored: ``JointsMSELoss`` / ``JointsMSELoss_offset`` (lib/core/loss.py),
``get_optimizer`` -> Adam(lr) (lib/utils/utils.py:60-76), ``train()`` (function.py:27-77) as
``train_epoch``; multi-GPU replaces nn.DataParallel's implicit gradient reduction by an explicit
mean all-reduce of the flat gradient (dist.allreduce_mean_).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .synth import hrnet_param_shapes

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _rup(x, m):
    return (x + m - 1) // m * m


def _is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


class _Act:
    """An NHWC activation [n,h,w,ck] (ck = channels rounded up to 16) and its gradient."""
    __slots__ = ("buf", "n", "h", "w", "c", "ck", "grad", "needs_grad", "bn_rows", "bn_ws")

    def __init__(self, buf, n, h, w, c, ck, needs_grad=True):
        self.buf, self.n, self.h, self.w, self.c, self.ck = buf, n, h, w, c, ck
        self.grad = None
        self.needs_grad = needs_grad
        self.bn_rows = 0            # > 0: the conv that produced it left that many BatchNorm partial rows in bn_ws
        self.bn_ws = None           # the BatchNorm workspace those rows are in


class _Group:
    """Tape entry of a multi-tensor op: its backward runs once every member's gradient is there (the members are
    outputs of independent branches; in reverse tape order all their consumers precede the op)."""
    __slots__ = ("ys",)

    def __init__(self, ys):
        self.ys = ys

    @property
    def grad(self):
        return None if all(y.grad is None for y in self.ys) else True

    @grad.setter
    def grad(self, v):
        for y in self.ys:
            y.grad = v


class Trainer:
    """Everything of the training step that is not one net's graph: the flat parameter / gradient / Adam buffers, the
    pack table, the primitive ops with their tape entries (``_conv``, ``_bn``, ``_sum_relu``, ``_maxpool``, ``_deconv``), the backward walk with
    its gradient buckets, the criterion, Adam and the captured step.  A subclass supplies ``forward`` (which fills
    ``self._tape`` and sets ``self._out``) and may override ``_conv_entry``."""

    def __init__(self, shapes, state_dict, num_joints, target_type, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, bucket_elems=6 * 1024 * 1024):
        """``shapes``: the net's state_dict contract (key -> shape, registration order).  ``bucket_elems``: gradient
        elements per all-reduce bucket (the default is ~25 MB)."""
        self.num_joints = int(num_joints)
        self.target_type = target_type
        self.device = torch.device(device)
        self.dtype = dtype
        self._dt = _lib.UDP_BF16 if dtype == "bf16" else _lib.UDP_F32
        self._tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_count = 0
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        missing = [k for k in shapes if k not in sd and not k.endswith("num_batches_tracked")]
        if missing:
            raise RuntimeError("state_dict lacks %d tensors, e.g. %s" % (len(missing), missing[:3]))
        self._keys = [k for k in shapes if _is_param(k)]
        self._stat_keys = [k for k in shapes if k.endswith("running_mean") or k.endswith("running_var")]
        self._shapes = shapes
        self._off, n = {}, 0
        for k in self._keys + self._stat_keys:
            self._off[k] = n
            n += self._key_stride(k, int(np.prod(shapes[k])))
        self._n_param = self._off[self._stat_keys[0]] if self._stat_keys else n
        flat = torch.zeros(n, dtype=torch.float32)
        for k in self._keys + self._stat_keys:
            v = sd[k].detach().to(torch.float32).reshape(-1)
            flat[self._off[k]:self._off[k] + v.numel()] = v
        self.flat = flat.to(self.device)                 # parameters, then running statistics
        self.grad = torch.zeros(self._n_param, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        # packed conv operands, refreshed from the fp32 master weights every step
        self._convs, self._transposed = {}, set()
        esz = 2 if dtype == "bf16" else 4
        ws_bytes, widest = 0, 1024
        for k in self._keys:
            s = shapes[k]
            if len(s) != 4:
                continue
            ent = self._conv_entry(k, s)
            if ent is None:
                continue
            cout, cin, ks, transposed, needs_dgrad = ent
            if transposed:
                if dtype != "f32" or ks != 4 or cin % 16 or cout % 16:
                    raise ValueError("%s: transposed convs are fp32, 4x4, with channel counts in multiples of 16" % k)
                self._transposed.add(k[:-len(".weight")])
            # (a transposed conv's operands have the same sizes: [16][ceil32(cout)][cin] and [16][ceil32(cin)][ceil16(cout)])
            fwd = torch.empty(ks * ks * _rup(cout, 32) * _rup(cin, 16) * esz, dtype=torch.uint8, device=self.device)
            dg = None
            if needs_dgrad:
                dg = torch.empty(ks * ks * _rup(cin, 32) * _rup(cout, 16) * esz, dtype=torch.uint8, device=self.device)
            self._convs[k[:-len(".weight")]] = (cout, cin, ks, fwd, dg)
            widest = max(widest, _rup(cout, 32), _rup(cin, 32))
            ws_bytes = max(ws_bytes, _lib.lib().udp_conv2d_wgrad_workspace_bytes(cout, cin, ks))
        self._wgrad_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        # one more per branch slot: the weight gradients of a lock-step level keep their partials until the common reduce
        self._wgrad_wss = [self._wgrad_ws] + [torch.empty(ws_bytes, dtype=torch.uint8, device=self.device) for _ in range(3)]
        descs = (_lib.PackDesc * len(self._convs))()
        for i, (name, (cout, cin, ks, fwd, dg)) in enumerate(self._convs.items()):
            descs[i].w, descs[i].w_fwd = self._p(name + ".weight"), fwd.data_ptr()
            descs[i].w_dgrad = None if dg is None else dg.data_ptr()
            descs[i].cout, descs[i].cin, descs[i].ks = cout, cin, ks
            descs[i].reserved = int(name in self._transposed)
        self._pack_table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(self.device)
        self._zeros = torch.zeros(widest, dtype=torch.float32, device=self.device)    # zero bias rows
        # one BatchNorm workspace per branch slot: the branches of a module run in lock step (_blocks_lockstep), a
        # conv's epilogue leaves its partial rows in its slot until the multi-tensor BatchNorm call has read them
        bn_c = max([shapes[k][0] for k in self._keys if len(shapes[k]) == 1] + [64])     # widest BatchNorm of this net
        self._bn_wss = [torch.zeros(_lib.lib().udp_bn_workspace_doubles(bn_c), dtype=torch.float64, device=self.device)
                        for _ in range(4)]
        self._bn_ws = self._bn_wss[0]
        self._loss = torch.zeros(2, dtype=torch.float64, device=self.device)
        self._graphs, self._warm, self._coef = {}, set(), None            # train_step_graphed
        self.version = 0                      # bumped by every optimizer step (the owning model's staleness check)
        self._tape = []
        # weight gradients on a side stream beside the backward chain (_on_side); A/B knob UDP_POSE_NO_WGRAD_OVERLAP
        self.overlap_wgrad = os.environ.get("UDP_POSE_NO_WGRAD_OVERLAP") is None and torch.device(self.device).type == "cuda"
        self._side = torch.cuda.Stream(device=self.device) if self.overlap_wgrad else None
        self._side_keep, self._side_busy = [], False
        self.fuse_bn_stats = os.environ.get("UDP_POSE_NO_BN_FUSION") is None     # A/B knob
        self.fuse_sums = os.environ.get("UDP_POSE_NO_SUM_FUSION") is None        # exchange-unit sums: one launch (A/B knob)
        # gradient buckets for the all-reduce (~25 MB each): consecutive parameters of the flat
        # gradient; a bucket is reduced as soon as the backward has written its last gradient, so the exchange
        # of the late layers' gradients runs under the backward of the early ones (DDP's overlap, which the
        # reference gets from RSN/exps/RSN18.coco/train.py:46-48 / nn.DataParallel's reducer)
        self.bucket_elems = int(bucket_elems)
        self._buckets, self._bucket_of = [], {}
        lo, cnt = 0, 0
        for i, k in enumerate(self._keys):
            self._bucket_of[k] = len(self._buckets)
            cnt += 1
            end = self._off[self._keys[i + 1]] if i + 1 < len(self._keys) else self._n_param
            if end - lo >= self.bucket_elems or i + 1 == len(self._keys):
                self._buckets.append((lo, end, cnt))
                lo, cnt = end, 0

    bn_over_stored = False       # _bn runs over the stored channels ck of a tensor with c < ck (needs _key_stride % 16 for 1-d keys)

    def _key_stride(self, key, numel):
        """Floats the tensor ``key`` occupies in ``flat`` / ``grad`` (>= numel, a multiple of 4; the slack stays 0)."""
        return _rup(numel, 4)

    def _conv_entry(self, key, shape):
        """(cout, cin, ks, transposed, needs an input gradient) of the 4-d parameter ``key`` for the pack table, or
        None when no conv kernel reads it.  A transposed conv's weight is [cin][cout][4][4]."""
        return shape[0], shape[1], shape[2], False, key != "conv1.weight"

    def forward(self, x):
        raise NotImplementedError

    # ------------------------------------------------------------------ parameter views
    def _p(self, key):
        return self.flat.data_ptr() + 4 * self._off[key]

    def _g(self, key):
        return self.grad.data_ptr() + 4 * self._off[key]

    def param(self, key):
        n = int(np.prod(self._shapes[key]))
        return self.flat[self._off[key]:self._off[key] + n].view(*self._shapes[key])

    def grad_of(self, key):
        n = int(np.prod(self._shapes[key]))
        return self.grad[self._off[key]:self._off[key] + n].view(*self._shapes[key])

    def state_dict(self):
        """Reference-format state_dict (fp32, host) -- loadable by the reference module and by model.MODELS."""
        flat = self.flat.cpu()
        out = {}
        for k, s in self._shapes.items():
            if k.endswith("num_batches_tracked"):
                out[k] = torch.tensor(self.step_count, dtype=torch.int64)
            else:
                n = int(np.prod(s))
                out[k] = flat[self._off[k]:self._off[k] + n].view(*s).clone()
        return out

    # ------------------------------------------------------------------ primitive ops
    def _stream(self):
        return _lib.stream_ptr()

    def _on_side(self, fn, *keep):
        """Run the launches of ``fn`` on the side stream, ordered behind everything queued on the current stream so far
        (fork).  The weight gradients go there: nothing in the backward chain reads them -- only the bucket all-reduce /
        Adam, behind ``_join_side`` -- and at 32 images per GPU the chain's kernels (48-1024 workgroups, BatchNorm
        passes) leave most of the chip idle.  ``keep``: tensors the side launches read; they stay referenced until the
        join, so the allocator cannot hand their memory to the main stream's next kernels."""
        if not self.overlap_wgrad:
            fn()
            return
        self._side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._side):
            fn()
        self._side_keep.extend(keep)
        self._side_busy = True

    def _join_side(self):
        if self._side_busy:
            torch.cuda.current_stream().wait_stream(self._side)
            self._side_keep.clear()
            self._side_busy = False

    def _new(self, n, h, w, c, needs_grad=True):
        ck = _rup(c, 16)
        return _Act(torch.empty(n * h * w * ck, dtype=self._tdt, device=self.device), n, h, w, c, ck, needs_grad)

    def _like(self, a):
        return torch.empty_like(a.buf)

    def _conv_op(self, ks, stride, cin, cout, hin, win, hout, wout, nchw=False):
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, 0
        op.cin, op.cout, op.cout_pad = cin, cout, _rup(cout, 32)
        op.hin, op.win, op.hout, op.wout = hin, win, hout, wout
        op.in_buf = op.res_buf = _lib.UDP_BUF_NONE
        op.out_buf = _lib.UDP_BUF_OUTPUT if nchw else 0
        return op

    def _conv(self, x, name, stride=1, bias_key=None, nchw_out=False, bn_stats=False, slot=0, res=None):
        """``res``: an activation of the output's shape added in the conv's epilogue (y = conv(x) + bias + res, the
        residual pointer of udp_conv2d_fused); the backward hands dy on to ``res.grad``, as ``_bn`` does for its ``res``."""
        L = _lib.lib()
        bn_ws = self._bn_wss[slot]
        cout, cin, ks, wf, wd = self._convs[name]
        if x.c != cin:
            raise ValueError("%s: expects %d input channels, got %d" % (name, cin, x.c))
        pad = ks // 2
        ho, wo = (x.h + 2 * pad - ks) // stride + 1, (x.w + 2 * pad - ks) // stride + 1
        bias = self._p(bias_key) if bias_key else self._zeros.data_ptr()
        if nchw_out:
            y = _Act(torch.empty(x.n, cout, ho, wo, dtype=torch.float32, device=self.device), x.n, ho, wo, cout,
                     _rup(cout, 16))
            op = self._conv_op(ks, stride, x.ck, cout, x.h, x.w, ho, wo, nchw=True)
        else:
            y = self._new(x.n, ho, wo, cout)
            op = self._conv_op(ks, stride, x.ck, y.ck, x.h, x.w, ho, wo)
        if bias_key:                                       # bias row padded to cout_pad
            b = torch.zeros(_rup(cout, 32), dtype=torch.float32, device=self.device)
            b[:cout] = self.param(bias_key)
            bias = b.data_ptr()
            y_keep = b
        else:
            y_keep = None
        if res is not None and (nchw_out or bn_stats or (res.n, res.h, res.w, res.ck) != (y.n, y.h, y.w, y.ck)):
            raise ValueError("%s: a residual needs an NHWC output of its own shape and no fused BatchNorm statistics" % name)
        if bn_stats and self.fuse_bn_stats and not nchw_out and (y.c == y.ck or self.bn_over_stored):
            # the BatchNorm that follows reads its statistics from the conv epilogue's partial sums
            rows = C.c_int(0)
            rc = L.udp_conv2d_fused_bn(C.byref(op), self._dt, x.n, x.buf.data_ptr(), wf.data_ptr(), bias,
                                       y.buf.data_ptr(), bn_ws.data_ptr(), bn_ws.numel(), C.byref(rows),
                                       self._stream())
            if rc == -4:       # UDP_ERR_WORKSPACE: more tiles than partial rows fit -> separate statistics pass
                _lib.check(L.udp_conv2d_fused(C.byref(op), self._dt, x.n, x.buf.data_ptr(), wf.data_ptr(), bias, None,
                                              None, None, None, y.buf.data_ptr(), self._stream()))
            else:
                _lib.check(rc)
                y.bn_rows = rows.value
                y.bn_ws = bn_ws
        else:
            _lib.check(L.udp_conv2d_fused(C.byref(op), self._dt, x.n, x.buf.data_ptr(), wf.data_ptr(), bias,
                                          None if res is None else res.buf.data_ptr(), None, None, None, y.buf.data_ptr(),
                                          self._stream()))

        def backward():
            dy = y.grad                                   # NHWC [n,ho,wo,ck(cout)]
            if res is not None and res.needs_grad:        # a copy: the side stream still reads dy when res.grad is added to
                have = res.grad is not None
                if not have:
                    res.grad = self._like(res)
                _lib.check(L.udp_ew_accumulate(res.grad.data_ptr(), dy.data_ptr(), res.n, res.h, res.w, res.ck, 0,
                                               int(not have), 0, self._dt, self._stream()))

            def wgrad():
                _lib.check(L.udp_conv2d_wgrad(x.buf.data_ptr(), dy.data_ptr(), x.n, x.h, x.w, x.ck, ho, wo, y.ck, ks,
                                              stride, cout, cin, self._dt, self._g(name + ".weight"), 0,
                                              self._wgrad_ws.data_ptr(), self._wgrad_ws.numel(), self._stream()))
                if bias_key:
                    _lib.check(L.udp_bias_grad(dy.data_ptr(), x.n * ho * wo, y.ck, cout, self._g(bias_key), self._dt,
                                               self._stream()))
            self._on_side(wgrad, dy, x.buf)
            if not x.needs_grad:
                return
            src, hh, ww = dy, ho, wo
            stuffed = 0
            if stride == 2:
                # the input gradient of a stride-2 conv = a stride-1 conv over dy on the even grid of a 2x image; the
                # conv kernel reads dy AS that zero-stuffed image (udp_conv_op.in_stuff2) instead of a materialised
                # copy (udp_zero_stuff2: one more launch, 4x the bytes written and read; UDP_POSE_ZERO_STUFF=1 for A/B)
                hh, ww = 2 * ho, 2 * wo
                if os.environ.get("UDP_POSE_ZERO_STUFF"):
                    src = torch.empty(x.n * 4 * ho * wo * y.ck, dtype=self._tdt, device=self.device)
                    _lib.check(L.udp_zero_stuff2(dy.data_ptr(), x.n, ho, wo, y.ck, self._dt, src.data_ptr(), self._stream()))
                else:
                    stuffed = 1
            dop = self._conv_op(ks, 1, y.ck, x.ck, hh, ww, x.h, x.w)
            dop.in_stuff2 = stuffed
            acc = x.grad
            if acc is None:
                x.grad = self._like(x)
            _lib.check(L.udp_conv2d_fused(C.byref(dop), self._dt, x.n, src.data_ptr(), wd.data_ptr(),
                                          self._zeros.data_ptr(), None if acc is None else acc.data_ptr(), None, None,
                                          None, x.grad.data_ptr(), self._stream()))
        self._tape.append((y, backward, y_keep, [name + ".weight"] + ([bias_key] if bias_key else [])))
        return y

    def _bn(self, x, name, relu=True, res=None, eps=BN_EPS, momentum=BN_MOMENTUM):
        L = _lib.lib()
        m, c = x.n * x.h * x.w, x.ck
        if x.c != x.ck and not self.bn_over_stored:
            raise ValueError("%s: BatchNorm over %d channels (not a multiple of 16)" % (name, x.c))
        y = self._new(x.n, x.h, x.w, x.c)
        save = torch.empty(2 * c, dtype=torch.float32, device=self.device)
        args = (x.buf.data_ptr(), m, c, self._p(name + ".weight"), self._p(name + ".bias"), eps, momentum,
                self._p(name + ".running_mean"), self._p(name + ".running_var"), save.data_ptr(), save.data_ptr() + 4 * c,
                None if res is None else res.buf.data_ptr(), int(relu), y.buf.data_ptr(), self._dt,
                (x.bn_ws if x.bn_rows else self._bn_ws).data_ptr())
        if x.bn_rows:
            _lib.check(L.udp_bn_train_fwd_from_sums(*args, x.bn_rows, self._stream()))
        else:
            _lib.check(L.udp_bn_train_fwd(*args, self._stream()))

        def backward():
            x.grad = self._like(x)
            g_out = None
            if res is not None and res.needs_grad:
                g_out = self._like(y)
            _lib.check(L.udp_bn_train_bwd(x.buf.data_ptr(), y.grad.data_ptr(), y.buf.data_ptr() if relu else None, m, c,
                                          self._p(name + ".weight"), save.data_ptr(), save.data_ptr() + 4 * c,
                                          self._g(name + ".weight"), self._g(name + ".bias"), x.grad.data_ptr(),
                                          None if g_out is None else g_out.data_ptr(), self._dt,
                                          self._bn_ws.data_ptr(), self._stream()))
            if g_out is not None:
                if res.grad is None:
                    res.grad = g_out
                else:
                    _lib.check(L.udp_ew_accumulate(res.grad.data_ptr(), g_out.data_ptr(), res.n, res.h, res.w, res.ck,
                                                   0, 0, 0, self._dt, self._stream()))
        self._tape.append((y, backward, save, [name + ".weight", name + ".bias"]))
        return y

    def _sum_relu(self, terms):
        """y = relu(sum_k up(term_k, shift_k)): HighResolutionModule.forward :266-272."""
        L = _lib.lib()
        t0 = terms[0][0]
        y = self._new(t0.n, t0.h << terms[0][1], t0.w << terms[0][1], t0.c)
        # ONE launch: y = relu(((t0 + t1) + t2) + ...), the terms added in the reference's order (udp_conv2d_fused, UDP_OP_FUSE:
        # in + res + up to three addends, each up-sampled by its shift; shift 0 = same resolution); fp32 tensors: the numbers of
        # the term-by-term launches below, bit for bit
        second = len(terms) > 1 and terms[1][1] == 0           # `res` carries no shift
        rest = terms[2:] if second else terms[1:]
        if self.fuse_sums and terms[0][1] == 0 and len(rest) <= 3:
            op = self._conv_op(1, 1, y.ck, y.ck, y.h, y.w, y.h, y.w)
            op.kind, op.relu, op.n_up = _lib.UDP_OP_FUSE, 1, len(rest)
            for k, (t, s) in enumerate(rest):
                op.up_shift[k] = s
            up_ptrs = [t.buf.data_ptr() for t, _ in rest] + [None] * (3 - len(rest))
            _lib.check(L.udp_conv2d_fused(C.byref(op), self._dt, y.n, terms[0][0].buf.data_ptr(), None, None,
                                          terms[1][0].buf.data_ptr() if second else None, up_ptrs[0], up_ptrs[1], up_ptrs[2],
                                          y.buf.data_ptr(), self._stream()))
        else:
            for k, (t, s) in enumerate(terms):
                _lib.check(L.udp_ew_accumulate(y.buf.data_ptr(), t.buf.data_ptr(), y.n, y.h, y.w, y.ck, s, int(k == 0),
                                               int(k == len(terms) - 1), self._dt, self._stream()))

        def backward():
            g = self._like(y)
            _lib.check(L.udp_relu_bwd(y.grad.data_ptr(), y.buf.data_ptr(), g.data_ptr(), g.numel(), self._dt,
                                      self._stream()))
            handed = not self.fuse_sums
            for t, s in terms:
                if not t.needs_grad:
                    continue
                have = t.grad is not None
                if s == 0 and not have and not handed:
                    # the first same-resolution term without a gradient yet takes g itself instead of a copy of it: every
                    # other term of this sum reads g inside this function, later writers of t.grad come later on the tape
                    t.grad = g
                    handed = True
                    continue
                if not have:
                    t.grad = self._like(t)
                if s == 0:
                    _lib.check(L.udp_ew_accumulate(t.grad.data_ptr(), g.data_ptr(), t.n, t.h, t.w, t.ck, 0, int(not have),
                                                   0, self._dt, self._stream()))
                else:
                    _lib.check(L.udp_upsample_bwd(g.data_ptr(), y.n, y.h, y.w, y.ck, s, t.grad.data_ptr(), int(have),
                                                  self._dt, self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    def _maxpool(self, x):
        """MaxPool2d(3, 2, 1) (pose_resnet.py:116, :199; shufflenetv2.py:124)."""
        L = _lib.lib()
        y = self._new(x.n, (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1, x.c)

        _lib.check(L.udp_maxpool3s2_fwd(x.buf.data_ptr(), x.n, x.h, x.w, x.ck, self._dt, y.buf.data_ptr(), self._stream()))

        def backward():
            if x.grad is not None:
                raise RuntimeError("max-pool: its input has one consumer")
            x.grad = self._like(x)
            _lib.check(L.udp_maxpool3s2_bwd(x.buf.data_ptr(), y.grad.data_ptr(), x.n, x.h, x.w, x.ck, self._dt,
                                            x.grad.data_ptr(), self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    def _deconv(self, x, name, bias_key=None):
        """ConvTranspose2d(4, 2, 1) (pose_resnet.py:155-193): forward = the UDP_OP_DECONV kernel on the packed raw weights, weight
        gradient = udp_conv2d_wgrad with ks 4 (dY as its `x`, the input as its `dy`), input gradient =
        udp_deconv4s2_dgrad.  The head is a chain: the input has no other consumer."""
        L = _lib.lib()
        cout, cin, ks, wf, wd = self._convs[name]
        if x.c != cin or x.c != x.ck:
            raise ValueError("%s: expects %d input channels (a multiple of 16), got %d" % (name, cin, x.c))
        y = self._new(x.n, 2 * x.h, 2 * x.w, cout)
        op = self._conv_op(4, 2, x.ck, cout, x.h, x.w, y.h, y.w)
        op.kind = _lib.UDP_OP_DECONV
        bias, keep = self._zeros.data_ptr(), None
        if bias_key:                                       # bias row padded to cout_pad
            keep = torch.zeros(_rup(cout, 32), dtype=torch.float32, device=self.device)
            keep[:cout] = self.param(bias_key)
            bias = keep.data_ptr()
        _lib.check(L.udp_conv2d_fused(C.byref(op), self._dt, x.n, x.buf.data_ptr(), wf.data_ptr(), bias, None, None, None,
                                      None, y.buf.data_ptr(), self._stream()))

        def backward():
            dy = y.grad                                    # NHWC [n,2h,2w,cout]

            def wgrad():
                _lib.check(L.udp_conv2d_wgrad(dy.data_ptr(), x.buf.data_ptr(), x.n, y.h, y.w, y.ck, x.h, x.w, x.ck, 4, 2,
                                              cin, cout, self._dt, self._g(name + ".weight"), 0,
                                              self._wgrad_ws.data_ptr(), self._wgrad_ws.numel(), self._stream()))
                if bias_key:
                    _lib.check(L.udp_bias_grad(dy.data_ptr(), y.n * y.h * y.w, y.ck, cout, self._g(bias_key), self._dt,
                                               self._stream()))
            self._on_side(wgrad, dy, x.buf)
            if not x.needs_grad:
                return
            if x.grad is not None:
                raise RuntimeError("%s: its input has one consumer" % name)
            x.grad = self._like(x)
            _lib.check(L.udp_deconv4s2_dgrad(dy.data_ptr(), wd.data_ptr(), x.n, x.h, x.w, cin, x.ck, cout, y.ck, self._dt,
                                             x.grad.data_ptr(), self._stream()))
        self._tape.append((y, backward, keep, [name + ".weight"] + ([bias_key] if bias_key else [])))
        return y

    def _backward_walk(self, dheat, pre=None):
        """The tape in reverse.  Yields the list of gradient buckets a backward node has just completed (the node wrote
        their last gradient), and finally the buckets no node completed (a bucket with an unused parameter: its gradient
        stays as is).  ``pre()`` is called before anything is launched after a yield (segmented graph capture opens its
        next segment there).  Every parameter gradient is overwritten (implicit zero_grad)."""
        L = _lib.lib()
        if pre:
            pre()
        o = self._out
        g = torch.empty(o.n * o.h * o.w * o.ck, dtype=self._tdt, device=self.device)
        _lib.check(L.udp_nchw_to_nhwc(dheat.data_ptr(), o.n, o.c, o.h, o.w, o.ck, g.data_ptr(), self._dt, self._stream()))
        o.grad = g
        left = [c for _, _, c in self._buckets]
        for y, bwd, _, keys in reversed(self._tape):
            done = []
            if y.grad is not None:
                if pre:
                    pre()
                bwd()
                for k in keys:
                    b = self._bucket_of[k]
                    left[b] -= 1
                    if left[b] == 0:
                        done.append(b)
            y.grad = None
            if done:
                self._join_side()             # the bucket's weight gradients were written on the side stream
                yield done
        self._tape = []
        self._join_side()
        rest = [b for b, n_left in enumerate(left) if n_left > 0]
        if rest:
            yield rest

    def backward(self, dheat, world_size=1):
        """dheat: fp32 [N,C,h,w] = d loss / d heat-maps.  Fills self.grad (zero_grad is implicit: every
        parameter gradient is overwritten).  ``world_size > 1``: every gradient bucket is SUM-all-reduced
        (asynchronously, on the communication stream of torch.distributed) as soon as its last gradient has been
        written, overlapping the rest of the backward; on return all buckets are reduced."""
        works = []
        self.reduce_order = []                # bucket indices in the order their all-reduce was issued
        for done in self._backward_walk(dheat):
            if world_size > 1:
                works += [self._reduce_bucket(b) for b in done]
        for w in works:
            w.wait()

    def _reduce_bucket(self, b):
        from .dist import allreduce_sum_async
        lo, hi, _ = self._buckets[b]
        self.reduce_order.append(b)
        if os.environ.get("UDP_POSE_FAKE_ALLREDUCE"):        # timing diagnosis only (tools/bench_train.py): no exchange
            class _Done:
                def wait(self):
                    return True
            return _Done()
        return allreduce_sum_async(self.grad[lo:hi])

    def loss_and_grad(self, heat, target, target_weight):
        """criterion(output, target, target_weight) (loss.py:15-76) and its gradient w.r.t. output."""
        b, c = heat.shape[:2]
        off = self.target_type == "offset"
        j = c // 3 if off else c
        d = torch.empty_like(heat)
        _lib.check(_lib.lib().udp_mse_loss(heat.data_ptr(), target.data_ptr(), target_weight.data_ptr(), b, j,
                                           heat.shape[2] * heat.shape[3], int(off), self._loss.data_ptr(), d.data_ptr(),
                                           self._stream()))
        self._loss_grad = d
        return self._loss, d

    def adam_step(self, grad_scale=1.0):
        """optimizer.step(): torch.optim.Adam(lr) on the flat parameter buffer (utils.py:70-74).
        ``grad_scale``: 1/world_size after the SUM all-reduce of the gradient."""
        self.step_count += 1
        self.version += 1                                   # owners compare it with the version they last read
        _lib.check(_lib.lib().udp_adam_step(self.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                                            self.exp_avg_sq.data_ptr(), self._n_param, self.lr, self.betas[0],
                                            self.betas[1], self.eps, self.step_count, float(grad_scale),
                                            self._stream()))

    def _adam_step_dev(self, grad_scale=1.0):
        _lib.check(_lib.lib().udp_adam_step_dev(self.flat.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                                                self.exp_avg_sq.data_ptr(), self._n_param, self.betas[0], self.betas[1],
                                                self.eps, self._coef.data_ptr(), float(grad_scale), self._stream()))

    def train_step_graphed(self, x, target, target_weight, world_size=1):
        """train_step with the whole step (weight packing, forward, criterion, backward, Adam: ~1900
        launches issued from the Python tape) captured ONCE per input shape as a hipGraph (torch.cuda.graph: stream
        capture of our launches on torch's capture stream, activations from the graph's private pool) and replayed:
        the host then costs one graph launch per step instead of one ctypes call per kernel.  The first step of a
        shape runs eagerly (lazy one-time initialisation must not be captured), the second captures and replays.
        Arithmetic and results are those of train_step, bit for bit; the learning rate may change between steps
        (it only enters through Adam's two scalars, uploaded before every replay), betas / eps are part of the key.
        At most two shapes stay captured (a full and a ragged last batch).

        ``world_size > 1`` (one process per GPU, config 3): the step is captured in SEGMENTS that end where a gradient
        bucket receives its last gradient -- forward + criterion + the backward of the last layers; the backward
        between two bucket boundaries; ...; and Adam on its own.  A replayed step is: replay segment 0, issue the
        asynchronous SUM all-reduce of its bucket(s) from the host (torch.distributed orders it behind the segment on
        its communication stream: RCCL over xGMI, or gloo), replay segment 1 at once -- the exchange runs under it, as
        DistributedDataParallel's reducer overlaps the reference's backward -- and so on; the work handles are waited
        for (stream order, no host block under RCCL) before the Adam graph with grad_scale 1 / world_size.  All
        segments share one memory pool and are always replayed in capture order.  Same arithmetic, same bucket order
        and the same results as train_step(world_size), bit for bit."""
        key = (tuple(x.shape), tuple(target.shape), tuple(target_weight.shape), self.betas, self.eps, int(world_size))
        ent = self._graphs.get(key)
        if ent is None:
            if key not in self._warm:                                # first step of this shape: eager
                self._warm.add(key)
                return self.train_step(x, target, target_weight, world_size=world_size)
            if self._coef is None:
                self._coef = torch.zeros(2, dtype=torch.float32, device=self.device)
                # pinned staging slots for the asynchronous upload of Adam's two scalars: the host runs steps ahead
                # of the GPU, a slot is rewritten only after the copy that read it has completed (its event)
                self._coef_host = [torch.zeros(2, dtype=torch.float32).pin_memory() for _ in range(4)]
                self._coef_done = [None] * 4
            gx, gt, gw = x.clone(), target.contiguous().clone(), target_weight.contiguous().clone()
            torch.cuda.synchronize()             # the last replay of an evicted graph may still be running
            while len(self._graphs) >= 2:
                self._graphs.pop(next(iter(self._graphs)))
            if world_size == 1:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    heat = self.forward(gx)
                    self.loss_and_grad(heat, gt, gw)
                    self.backward(self._loss_grad)
                    self._adam_step_dev()
                segs = [(graph, [])]
            else:
                segs = self._capture_segments(gx, gt, gw, 1.0 / world_size)
            ent = self._graphs[key] = (segs, gx, gt, gw)
        segs, gx, gt, gw = ent
        gx.copy_(x, non_blocking=True)
        gt.copy_(target, non_blocking=True)
        gw.copy_(target_weight, non_blocking=True)
        self.step_count += 1
        slot = self.step_count % 4
        if self._coef_done[slot] is not None:
            self._coef_done[slot].synchronize()
        _lib.check(_lib.lib().udp_adam_coefficients(self.lr, self.betas[0], self.betas[1], self.step_count,
                                                    self._coef_host[slot].data_ptr()))
        self._coef.copy_(self._coef_host[slot], non_blocking=True)
        self._coef_done[slot] = torch.cuda.Event()
        self._coef_done[slot].record()
        works = []
        self.reduce_order = []
        for graph, buckets in segs:
            if graph is None:                                        # every bucket is reduced: Adam may read the gradient
                for w in works:
                    w.wait()
                continue
            graph.replay()
            works += [self._reduce_bucket(b) for b in buckets]
        self.version += 1
        return self._loss

    def _capture_segments(self, gx, gt, gw, grad_scale):
        """The step as a list of (graph, buckets to all-reduce after it) in replay order, a (None, []) marker where
        the outstanding all-reduces must be waited for, and the Adam graph last."""
        pool = torch.cuda.graph_pool_handle()
        segs = []
        cur = []                                    # [graph, context] of the segment being captured, or empty

        def begin():
            if not cur:
                g = torch.cuda.CUDAGraph()
                ctx = torch.cuda.graph(g, pool=pool)
                ctx.__enter__()
                cur[:] = [g, ctx]

        def end(buckets):
            if cur:
                cur[1].__exit__(None, None, None)
                segs.append((cur[0], list(buckets)))
                cur[:] = []
            elif buckets:                           # buckets nothing was launched for since the last boundary
                segs[-1] = (segs[-1][0], segs[-1][1] + list(buckets))

        try:
            begin()
            heat = self.forward(gx)
            self.loss_and_grad(heat, gt, gw)
            for done in self._backward_walk(self._loss_grad, pre=begin):
                end(done)
            end([])                                 # nodes behind the last bucket boundary (they write no parameter gradient)
        except BaseException:
            if cur:
                cur[1].__exit__(None, None, None)
            raise
        segs.append((None, []))
        adam = torch.cuda.CUDAGraph()
        with torch.cuda.graph(adam, pool=pool):
            self._adam_step_dev(grad_scale)
        segs.append((adam, []))
        return segs

    def train_step(self, x, target, target_weight, world_size=1):
        """function.py:46-76 for one batch.  Returns the loss tensor fp64 [2] = (L_hm, L_offset) on device."""
        heat = self.forward(x)
        loss, d = self.loss_and_grad(heat, target.contiguous(), target_weight.contiguous())
        self.backward(d, world_size)                       # incl. the one exchange step, bucket by bucket
        self.adam_step(1.0 / world_size)                   # mean over ranks = grad_scale
        return loss


class HRNetTrainer(Trainer):
    def __init__(self, cfg, state_dict, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, psa=False,
                 bucket_elems=6 * 1024 * 1024):
        """``psa``: the pose_hrnet_psa variant -- a PSA_s ("<block>.deattn.*") after relu(bn1) of every BasicBlock
        (pose_hrnet_psa.py:37,49), trained through the udp_psa_train_* entry points.  ``bucket_elems``: gradient elements
        per all-reduce bucket (the default is ~25 MB)."""
        from .model import _get
        self.psa = bool(psa)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        num_joints, target_type = int(_get(cfg, "MODEL", "NUM_JOINTS")), _get(cfg, "MODEL", "TARGET_TYPE")
        shapes = hrnet_param_shapes(self.extra, num_joints, target_type, psa=self.psa)
        super().__init__(shapes, state_dict, num_joints, target_type, device=device, dtype=dtype, lr=lr, betas=betas, eps=eps,
                         bucket_elems=bucket_elems)
        self.bn_multi = os.environ.get("UDP_POSE_NO_BN_MULTI") is None           # A/B knob
        self.conv_multi = os.environ.get("UDP_POSE_NO_CONV_MULTI") is None       # A/B knob (merged branch convs)

    def _conv_entry(self, key, shape):
        if ".deattn." in key and not key.endswith(".conv_v_left.weight"):
            return None             # the attention block reads its small fp32 matrices as they are; only theta is a conv
        return super()._conv_entry(key, shape)

    def _bn_multi(self, xs, names, relu=True, res=None):
        """The BatchNorms `names[b]` over `xs[b]` (one per branch, independent) as ONE multi-tensor call per pass
        (udp_bn_train_fwd_multi / _bwd_multi): results are those of `_bn` per branch, bit for bit."""
        L = _lib.lib()
        nb = len(xs)
        res = res or [None] * nb
        relus = list(relu) if isinstance(relu, (list, tuple)) else [relu] * nb
        ys = [self._new(x.n, x.h, x.w, x.c) for x in xs]
        saves = [torch.empty(2 * x.ck, dtype=torch.float32, device=self.device) for x in xs]
        items = (_lib.BnItem * nb)()
        for b, (x, y, sv) in enumerate(zip(xs, ys, saves)):
            if x.c != x.ck:
                raise ValueError("%s: BatchNorm over %d channels (not a multiple of 16)" % (names[b], x.c))
            it = items[b]
            it.x, it.y, it.m, it.c = x.buf.data_ptr(), y.buf.data_ptr(), x.n * x.h * x.w, x.ck
            it.gamma, it.beta = self._p(names[b] + ".weight"), self._p(names[b] + ".bias")
            it.running_mean, it.running_var = self._p(names[b] + ".running_mean"), self._p(names[b] + ".running_var")
            it.save_mean, it.save_invstd = sv.data_ptr(), sv.data_ptr() + 4 * x.ck
            it.res = None if res[b] is None else res[b].buf.data_ptr()
            it.relu, it.rows = int(relus[b]), x.bn_rows
            it.ws = (x.bn_ws if x.bn_rows else self._bn_wss[b]).data_ptr()
        _lib.check(L.udp_bn_train_fwd_multi(items, nb, BN_EPS, BN_MOMENTUM, self._dt, self._stream()))

        def backward():
            bi = (_lib.BnItem * nb)()
            g_outs = []
            for b, (x, y, sv) in enumerate(zip(xs, ys, saves)):
                x.grad = self._like(x)
                if y.grad is None:                     # a branch output nothing consumed: zero gradient
                    y.grad = torch.zeros_like(y.buf)
                g_out = self._like(y) if res[b] is not None and res[b].needs_grad else None
                g_outs.append(g_out)
                it = bi[b]
                it.x, it.dy, it.m, it.c = x.buf.data_ptr(), y.grad.data_ptr(), x.n * x.h * x.w, x.ck
                it.y_relu = y.buf.data_ptr() if relus[b] else None
                it.gamma = self._p(names[b] + ".weight")
                it.save_mean, it.save_invstd = sv.data_ptr(), sv.data_ptr() + 4 * x.ck
                it.dgamma, it.dbeta = self._g(names[b] + ".weight"), self._g(names[b] + ".bias")
                it.dx = x.grad.data_ptr()
                it.g_out = None if g_out is None else g_out.data_ptr()
                it.ws = self._bn_wss[b].data_ptr()
            _lib.check(L.udp_bn_train_bwd_multi(bi, nb, self._dt, self._stream()))
            for b, g_out in enumerate(g_outs):
                if g_out is None:
                    continue
                r = res[b]
                if r.grad is None:
                    r.grad = g_out
                else:
                    _lib.check(L.udp_ew_accumulate(r.grad.data_ptr(), g_out.data_ptr(), r.n, r.h, r.w, r.ck, 0, 0, 0,
                                                   self._dt, self._stream()))
        keys = [n + s for n in names for s in (".weight", ".bias")]
        self._tape.append((_Group(ys), backward, saves, keys))
        return ys

    def _convs_lockstep(self, xs, names):
        """The stride-1 convs `names[b]` on `xs[b]` (one per branch, independent; each followed by a BatchNorm) through
        udp_conv2d_fused_group: the members whose tile fits the merged kernel run as ONE launch, forward and input
        gradient alike (bf16 storage; fp32 members run one launch each).  Per-member results equal `_conv`'s."""
        L = _lib.lib()
        nb = len(xs)
        if not self.conv_multi:
            return [self._conv(xs[b], names[b], bn_stats=True, slot=b) for b in range(nb)]
        metas = [self._convs[nm] for nm in names]                  # (cout, cin, ks, wf, wd)
        ys, ops = [], []
        for x, (cout, cin, ks, wf, wd) in zip(xs, metas):
            if x.c != cin:
                raise ValueError("conv expects %d input channels, got %d" % (cin, x.c))
            y = self._new(x.n, x.h, x.w, cout)
            ys.append(y)
            ops.append(self._conv_op(ks, 1, x.ck, y.ck, x.h, x.w, x.h, x.w))
        order = list(reversed(range(nb)))                          # deepest-K member first in a merged launch
        items = (_lib.ConvItem * nb)()
        for it, b in zip(items, order):
            x, y, (cout, cin, ks, wf, wd) = xs[b], ys[b], metas[b]
            it.op, it.inp, it.weights = C.addressof(ops[b]), x.buf.data_ptr(), wf.data_ptr()
            it.bias, it.res, it.out = self._zeros.data_ptr(), None, y.buf.data_ptr()
            if self.fuse_bn_stats and y.c == y.ck:
                it.bn_ws, it.bn_ws_doubles = self._bn_wss[b].data_ptr(), self._bn_wss[b].numel()
        rc = L.udp_conv2d_fused_group(items, nb, self._dt, xs[0].n, self._stream())
        if rc == -4:           # UDP_ERR_WORKSPACE (more tiles than partial rows fit): the per-conv path sorts it out
            return [self._conv(xs[b], names[b], bn_stats=True, slot=b) for b in range(nb)]
        _lib.check(rc)
        for it, b in zip(items, order):
            if it.bn_ws:
                ys[b].bn_rows, ys[b].bn_ws = it.bn_rows, self._bn_wss[b]

        def backward():
            gi = (_lib.ConvItem * nb)()
            wi = (_lib.WgradItem * nb)()
            dops, k = [], 0
            for slot, b in enumerate(order):
                x, y, (cout, cin, ks, wf, wd) = xs[b], ys[b], metas[b]
                if y.grad is None:
                    y.grad = torch.zeros_like(y.buf)
                w = wi[slot]                           # partial sums one launch per member, their reduces one launch
                w.x, w.dy, w.dw = x.buf.data_ptr(), y.grad.data_ptr(), self._g(names[b] + ".weight")
                w.workspace, w.workspace_bytes = self._wgrad_wss[slot].data_ptr(), self._wgrad_wss[slot].numel()
                w.n, w.hin, w.win, w.cin_k, w.hout, w.wout, w.cout_k = x.n, x.h, x.w, x.ck, x.h, x.w, y.ck
                w.ks, w.stride, w.cout, w.cin, w.accumulate = ks, 1, cout, cin, 0
            self._on_side(lambda: _lib.check(L.udp_conv2d_wgrad_group(wi, nb, self._dt, self._stream())),
                          *[xs[b].buf for b in order], *[ys[b].grad for b in order])
            for b in order:
                x, y, (cout, cin, ks, wf, wd) = xs[b], ys[b], metas[b]
                if not x.needs_grad:
                    continue
                res = x.grad
                if res is None:
                    x.grad = self._like(x)
                dops.append(self._conv_op(ks, 1, y.ck, x.ck, x.h, x.w, x.h, x.w))
                it = gi[k]
                k += 1
                it.op, it.inp, it.weights = C.addressof(dops[-1]), y.grad.data_ptr(), wd.data_ptr()
                it.bias, it.out = self._zeros.data_ptr(), x.grad.data_ptr()
                it.res = None if res is None else res.data_ptr()
            if k:
                _lib.check(L.udp_conv2d_fused_group(gi, k, self._dt, xs[0].n, self._stream()))
        self._tape.append((_Group(ys), backward, ops, [nm + ".weight" for nm in names]))
        return ys

    def _psa(self, x, p):
        """PSA_s `p` on x (PSA.py:190-269), train mode: pool + channel chain + scale (x -> x1), theta = the 1x1 conv
        conv_v_left through `_conv` (its weight and input gradients come with it), spatial gate (x1, theta -> x2).
        Three tape entries; the nine small parameter gradients are written by ONE launch behind the last backward
        piece (side stream), so they are listed on that entry."""
        L = _lib.lib()
        if x.c != x.ck:
            raise ValueError("%s: attention over %d channels (not a multiple of 16)" % (p, x.c))
        nfl = L.udp_psa_train_save_floats(x.n, x.h, x.w, x.c)
        if not nfl:
            _lib.check(-3)
        save = torch.empty(nfl, dtype=torch.float32, device=self.device)
        keys = [p + k for k in _lib.PSA_TRAIN_KEYS]

        def args(**ptrs):
            a = _lib.PsaTrainArgs()
            for i, k in enumerate(keys):
                a.w[i], a.dw[i] = self._p(k), self._g(k)
            a.save, a.save_floats = save.data_ptr(), nfl
            a.n, a.h, a.w_px, a.c = x.n, x.h, x.w, x.c
            for k, t in ptrs.items():
                setattr(a, k, t.data_ptr())
            return a
        x1 = self._new(x.n, x.h, x.w, x.c)
        _lib.check(L.udp_psa_train_fwd_pool(C.byref(args(x=x.buf, x1=x1.buf)), self._dt, self._stream()))

        def bwd_pool():
            had = x.grad
            dx = self._like(x)
            _lib.check(L.udp_psa_train_bwd_pool(C.byref(args(dx1=x1.grad, x=x.buf, dx=dx)), self._dt, self._stream()))
            if had is None:
                x.grad = dx
            else:
                _lib.check(L.udp_ew_accumulate(had.data_ptr(), dx.data_ptr(), x.n, x.h, x.w, x.ck, 0, 0, 0, self._dt,
                                               self._stream()))
            self._on_side(lambda: _lib.check(L.udp_psa_train_bwd_params(C.byref(args()), self._dt, self._stream())), save)
        self._tape.append((x1, bwd_pool, save, keys))
        theta = self._conv(x1, p + ".conv_v_left")
        x2 = self._new(x.n, x.h, x.w, x.c)
        _lib.check(L.udp_psa_train_fwd_sp(C.byref(args(x1=x1.buf, theta=theta.buf, x2=x2.buf)), self._dt, self._stream()))

        def bwd_sp():
            if x1.grad is not None or theta.grad is not None:
                raise RuntimeError("%s: the attention block's inner maps have one consumer each" % p)
            x1.grad, theta.grad = self._like(x1), self._like(theta)
            _lib.check(L.udp_psa_train_bwd_sp(C.byref(args(dx2=x2.grad, x1=x1.buf, theta=theta.buf, dtheta=theta.grad,
                                                           dx1=x1.grad)), self._dt, self._stream()))
        self._tape.append((x2, bwd_sp, save, []))
        return x2

    def _blocks_lockstep(self, xs, ps):
        """BasicBlock `ps[b]` on branch b, all branches at once: the convs stay one launch each, the two BatchNorms
        of the block run as multi-tensor calls over the branches."""
        nb = len(xs)
        c1 = self._convs_lockstep(xs, [q + ".conv1" for q in ps])
        t = self._bn_multi(c1, [q + ".bn1" for q in ps])
        if self.psa:
            t = [self._psa(t[b], ps[b] + ".deattn") for b in range(nb)]
        c2 = self._convs_lockstep(t, [q + ".conv2" for q in ps])
        return self._bn_multi(c2, [q + ".bn2" for q in ps], res=xs)

    def _conv_bn_multi(self, specs):
        """Independent conv + BatchNorm pairs `(x, conv, bn, stride, relu)`: convs one launch each, their
        BatchNorms four at a time as multi-tensor calls."""
        outs = []
        for c0 in range(0, len(specs), 4):
            chunk = specs[c0:c0 + 4]
            if len(chunk) == 1:
                x, cv, bn, st, relu = chunk[0]
                outs.append(self._bn(self._conv(x, cv, stride=st, bn_stats=True), bn, relu=relu))
                continue
            ys = [self._conv(x, cv, stride=st, bn_stats=True, slot=b) for b, (x, cv, _, st, _) in enumerate(chunk)]
            outs += self._bn_multi(ys, [bn for _, _, bn, _, _ in chunk], relu=[r for *_, r in chunk])
        return outs

    def _fuse_lockstep(self, xs, p, last):
        """The fuse layers of a module (pose_hrnet.py:224-272) level by level: every 1x1 (j > i) conv and the k-th
        stride-2 conv of every (i, j < i) chain only depend on the level before."""
        nb = len(xs)
        n_out = 1 if last else nb
        ups, cur = {}, {}
        specs, keys = [], []
        for i in range(n_out):
            for j in range(nb):
                q = "%s.fuse_layers.%d.%d" % (p, i, j)
                if j > i:
                    specs.append((xs[j], q + ".0", q + ".1", 1, False))
                    keys.append(("up", i, j))
                elif j < i:
                    specs.append((xs[j], q + ".0.0", q + ".0.1", 2, i - j != 1))
                    keys.append(("down", i, j))
        for key, t in zip(keys, self._conv_bn_multi(specs)):
            (ups if key[0] == "up" else cur)[key[1:]] = t
        for k in range(1, n_out):
            todo = [(i, j) for (i, j) in cur if i - j > k]
            specs = [(cur[(i, j)], "%s.fuse_layers.%d.%d.%d.0" % (p, i, j, k), "%s.fuse_layers.%d.%d.%d.1" % (p, i, j, k), 2,
                      k != i - j - 1) for i, j in todo]
            for ij, t in zip(todo, self._conv_bn_multi(specs)):
                cur[ij] = t
        outs = []
        for i in range(n_out):
            terms = []
            for j in range(nb):
                if j > i:
                    terms.append((ups[(i, j)], j - i))
                elif j == i:
                    terms.append((self._conv(xs[j], "%s.fuse_layers.%d.%d.0" % (p, i, j)) if last else xs[j], 0))
                else:
                    terms.append((cur[(i, j)], 0))
            outs.append(self._sum_relu(terms))
        return outs

    # ------------------------------------------------------------------ the HRNet graph (pose_hrnet.py)
    def _basic(self, x, p):
        t = self._bn(self._conv(x, p + ".conv1", bn_stats=True), p + ".bn1")
        if self.psa:
            t = self._psa(t, p + ".deattn")
        return self._bn(self._conv(t, p + ".conv2", bn_stats=True), p + ".bn2", res=x)

    def _bottleneck(self, x, p):
        a = self._bn(self._conv(x, p + ".conv1", bn_stats=True), p + ".bn1")
        b = self._bn(self._conv(a, p + ".conv2", bn_stats=True), p + ".bn2")
        r = x
        if (p + ".downsample.0") in self._convs:
            r = self._bn(self._conv(x, p + ".downsample.0", bn_stats=True), p + ".downsample.1", relu=False)
        return self._bn(self._conv(b, p + ".conv3", bn_stats=True), p + ".bn3", res=r)

    def _module(self, xs, p, num_blocks, last):
        nb = len(xs)
        xs = list(xs)
        if self.bn_multi and 1 < nb <= 4 and len(set(num_blocks[:nb])) == 1:
            for k in range(num_blocks[0]):
                xs = self._blocks_lockstep(xs, ["%s.branches.%d.%d" % (p, b, k) for b in range(nb)])
        else:
            for b in range(nb):
                for k in range(num_blocks[b]):
                    xs[b] = self._basic(xs[b], "%s.branches.%d.%d" % (p, b, k))
        if self.bn_multi and nb > 1:
            return self._fuse_lockstep(xs, p, last)
        outs = []
        for i in range(1 if last else nb):
            terms = []
            for j in range(nb):
                q = "%s.fuse_layers.%d.%d" % (p, i, j)
                if j > i:
                    terms.append((self._bn(self._conv(xs[j], q + ".0", bn_stats=True), q + ".1", relu=False), j - i))
                elif j == i:
                    terms.append((self._conv(xs[j], q + ".0") if last else xs[j], 0))
                else:
                    t = xs[j]
                    for k in range(i - j):
                        t = self._bn(self._conv(t, "%s.%d.0" % (q, k), stride=2, bn_stats=True), "%s.%d.1" % (q, k),
                                     relu=(k != i - j - 1))
                    terms.append((t, 0))
            outs.append(self._sum_relu(terms))
        return outs

    def _transition(self, ys, name, n_cur):
        xs = []
        for i in range(n_cur):
            q = "%s.%d" % (name, i)
            if i < len(ys):
                xs.append(self._bn(self._conv(ys[i], q + ".0", bn_stats=True), q + ".1") if (q + ".0") in self._convs else ys[i])
            else:
                y = ys[-1]
                for k in range(i + 1 - len(ys)):
                    y = self._bn(self._conv(y, "%s.%d.0" % (q, k), stride=2, bn_stats=True), "%s.%d.1" % (q, k))
                xs.append(y)
        return xs

    def forward(self, x):
        """Train-mode forward.  x: fp32 [N,3,H,W] on the device.  Returns fp32 [N,C,H/4,W/4]."""
        L = _lib.lib()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [N,3,H,W]")
        n, _, h, w = x.shape
        if h % 32 or w % 32:
            raise ValueError("input %dx%d must be a multiple of 32" % (h, w))
        self._tape = []
        _lib.check(L.udp_pack_conv_weights_batch(self._pack_table.data_ptr(), len(self._convs), self._dt, self._stream()))
        a = self._new(n, h, w, 3, needs_grad=False)
        _lib.check(L.udp_nchw_to_nhwc(x.data_ptr(), n, 3, h, w, a.ck, a.buf.data_ptr(), self._dt, self._stream()))
        a = self._bn(self._conv(a, "conv1", stride=2, bn_stats=True), "bn1")
        a = self._bn(self._conv(a, "conv2", stride=2, bn_stats=True), "bn2")
        for k in range(4):
            a = self._bottleneck(a, "layer1.%d" % k)
        ys = [a]
        for st in (2, 3, 4):
            cfg = self.extra["STAGE%d" % st]
            xs = self._transition(ys, "transition%d" % (st - 1), cfg["NUM_BRANCHES"])
            for mi in range(cfg["NUM_MODULES"]):
                xs = self._module(xs, "stage%d.%d" % (st, mi), cfg["NUM_BLOCKS"],
                                  st == 4 and mi == cfg["NUM_MODULES"] - 1)
            ys = xs
        self._out = self._conv(ys[0], "final_layer", bias_key="final_layer.bias", nchw_out=True)
        return self._out.buf


class PoseResNetTrainer(Trainer):
    """pose_resnet / SimpleBaseline (deep_hrnet/lib/models/pose_resnet.py:105-209; recipe
    experiments/coco/resnet/res50_256x192_d256x3_adam_lr1e-3.yaml) on the base step.  ``spec``: the dict of
    ``resnet_plan.pose_resnet_spec`` (``layers`` may be any 4-tuple of Bottleneck counts).  fp32 only: the reference's
    precision, and the transposed conv has no bf16 form."""

    def __init__(self, spec, num_joints, target_type, state_dict, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, bucket_elems=6 * 1024 * 1024):
        from .synth_resnet import pose_resnet_param_shapes
        if dtype != "f32":
            raise ValueError("pose_resnet trains in fp32 only (dtype %r): the deconv kernels have no bf16 form" % (dtype,))
        self.spec = dict(spec)
        if len(self.spec["layers"]) != 4 or any(f % 16 for f in self.spec["deconv_filters"]):
            raise ValueError("pose_resnet trainer: four stages and deconv filters in multiples of 16 (got %s, %s)"
                             % (self.spec["layers"], self.spec["deconv_filters"]))
        shapes = pose_resnet_param_shapes(layers=tuple(self.spec["layers"]), num_joints=int(num_joints),
                                          deconv_filters=tuple(self.spec["deconv_filters"]), deconv_kernel=4,
                                          final_kernel=self.spec["final_kernel"],
                                          deconv_with_bias=self.spec["deconv_with_bias"])
        super().__init__(shapes, state_dict, num_joints, target_type, device=device, dtype=dtype, lr=lr, betas=betas, eps=eps,
                         bucket_elems=bucket_elems)

    def _conv_entry(self, key, shape):
        if key.startswith("deconv_layers."):
            return shape[1], shape[0], shape[2], True, True       # ConvTranspose2d.weight is [cin][cout][k][k]
        return super()._conv_entry(key, shape)

    # ------------------------------------------------------------------ the ops HRNet does not have
    def _stem(self, x):
        """conv1 (:112, :196): 3 -> 64, 7x7 stride 2 on the unfolded weights.  No input gradient: x is the image."""
        L = _lib.lib()
        cout, cin, ks, wf, _ = self._convs["conv1"]
        ho, wo = (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1
        y = self._new(x.n, ho, wo, cout)
        _lib.check(L.udp_stem7_train_fwd(x.buf.data_ptr(), wf.data_ptr(), x.n, x.h, x.w, x.ck, cout, self._dt,
                                         y.buf.data_ptr(), self._stream()))

        def backward():
            dy = y.grad
            self._on_side(lambda: _lib.check(L.udp_conv2d_wgrad(
                x.buf.data_ptr(), dy.data_ptr(), x.n, x.h, x.w, x.ck, ho, wo, y.ck, ks, 2, cout, cin, self._dt,
                self._g("conv1.weight"), 0, self._wgrad_ws.data_ptr(), self._wgrad_ws.numel(), self._stream())), dy, x.buf)
        self._tape.append((y, backward, None, ["conv1.weight"]))
        return y

    # ------------------------------------------------------------------ the graph (pose_resnet.py:195-209)
    def _bottleneck(self, x, p, stride):
        """Bottleneck.forward (:82-100) as _make_layer builds it (:138-153): the stride sits on conv2 and on the 1x1
        projection shortcut."""
        a = self._bn(self._conv(x, p + ".conv1", bn_stats=True), p + ".bn1")
        b = self._bn(self._conv(a, p + ".conv2", stride=stride, bn_stats=True), p + ".bn2")
        r = x
        if (p + ".downsample.0") in self._convs:
            r = self._bn(self._conv(x, p + ".downsample.0", stride=stride, bn_stats=True), p + ".downsample.1", relu=False)
        return self._bn(self._conv(b, p + ".conv3", bn_stats=True), p + ".bn3", res=r)

    def forward(self, x):
        """Train-mode forward.  x: fp32 [N,3,H,W] on the device.  Returns fp32 [N,J,H/4,W/4]."""
        L = _lib.lib()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [N,3,H,W]")
        n, _, h, w = x.shape
        if h % 32 or w % 32:
            raise ValueError("input %dx%d must be a multiple of 32" % (h, w))
        self._tape = []
        _lib.check(L.udp_pack_conv_weights_batch(self._pack_table.data_ptr(), len(self._convs), self._dt, self._stream()))
        a = self._new(n, h, w, 3, needs_grad=False)
        _lib.check(L.udp_nchw_to_nhwc(x.data_ptr(), n, 3, h, w, a.ck, a.buf.data_ptr(), self._dt, self._stream()))
        a = self._maxpool(self._bn(self._stem(a), "bn1"))
        for li, nblk in enumerate(self.spec["layers"], start=1):
            for k in range(nblk):
                a = self._bottleneck(a, "layer%d.%d" % (li, k), 2 if (li > 1 and k == 0) else 1)
        for d in range(len(self.spec["deconv_filters"])):
            q = "deconv_layers.%d" % (3 * d)
            a = self._bn(self._deconv(a, q, q + ".bias" if self.spec["deconv_with_bias"] else None),
                         "deconv_layers.%d" % (3 * d + 1))
        self._out = self._conv(a, "final_layer", bias_key="final_layer.bias", nchw_out=True)
        return self._out.buf


class ShuffleNetV2Trainer(Trainer):
    """pose_shufflenetv2_10x_pixel_shuffle (deep_hrnet/lib/models/pose_shufflenetv2_10x_pixel_shuffle.py:23-53; recipe
    experiments/coco/shufflenetv2/10x_256x192_adam_lr1e-3_pixel_shuffle.yaml) on the base step.  ``spec``: the dict of
    ``shufflenet_plan.shufflenet_spec``.  fp32 only: the reference's precision, and the depthwise kernels have no bf16 form.

    Channel counts here are not multiples of 16 (24, 58, 88, 116, 232 ...).  A tensor of c channels is stored with
    ck = ceil16(c); every 1-d parameter (and running statistic) occupies ceil16(c) floats of ``flat`` / ``grad`` whose
    slack is 0, and the BatchNorm kernels run over the ck stored channels (``bn_over_stored``).  That is exact as long as
    every stored channel of every activation and gradient is written by its producer and the padded ones are exactly 0:
    a padded channel then has mean 0, variance 0, gamma = beta = 0, output 0, gradient 0, and Adam leaves its slots at 0.

    A unit's output stays a pair of halves (a, b) -- the concat (:92) is materialised only where a whole tensor is read
    (a stride-2 unit, ``conv_last``); a stride-1 unit's channel_shuffle (:86-92) reads the pair directly."""

    NAME = "pose_shufflenetv2_10x_pixel_shuffle"
    bn_over_stored = True

    def __init__(self, spec, num_joints, target_type, state_dict, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, bucket_elems=6 * 1024 * 1024):
        from .synth_shufflenet import shufflenet_units
        if dtype != "f32":
            raise ValueError("%s trains in fp32 only (dtype %r): the depthwise kernels have no bf16 form" % (self.NAME, dtype))
        self.spec = dict(spec)
        shapes = self._head_shapes(num_joints, target_type)
        self._units = shufflenet_units(self.spec["model_size"])
        super().__init__(shapes, state_dict, num_joints, target_type, device=device, dtype=dtype, lr=lr, betas=betas, eps=eps,
                         bucket_elems=bucket_elems)
        self._dw_ws = self._dw_workspace()

    def _head_shapes(self, num_joints, target_type):
        from .synth_shufflenet import shufflenet_param_shapes
        sp = self.spec
        if any(a % 64 for a in sp["architecture"]):
            raise ValueError("%s trainer: ARCHITECTURE=%s -- the pixel shuffle moves 16 input channels per thread, every entry "
                             "must be a multiple of 64" % (self.NAME, tuple(sp["architecture"])))
        return shufflenet_param_shapes(model_size=sp["model_size"], num_joints=int(num_joints), target_type=target_type,
                                       start_channels=sp["start_channels"], architecture=tuple(sp["architecture"]),
                                       final_kernel=sp["final_kernel"])

    @staticmethod
    def _is_dw(key, shape):
        return len(shape) == 4 and shape[1] == 1 and shape[2] == 3 and (".branch_main.3." in key or ".branch_proj.0." in key)

    def _key_stride(self, key, numel):
        return _rup(numel, 16 if len(self._shapes[key]) == 1 else 4)

    def _conv_entry(self, key, shape):
        if self._is_dw(key, shape):
            return None                     # the depthwise kernels read the parameter as it is
        if key.startswith("deconv_layers."):
            return shape[1], shape[0], shape[2], True, True       # ConvTranspose2d.weight is [cin][cout][k][k]
        return shape[0], shape[1], shape[2], False, key != "backbone.first_conv.0.weight"

    # ------------------------------------------------------------------ the ops the other nets do not have
    def _dw_workspace(self):
        """One workspace for every depthwise weight gradient (they run in order on the side stream): the widest split."""
        L = _lib.lib()
        return torch.empty(max(int(L.udp_dwconvk_wgrad_workspace_bytes(256, 1, 1, _rup(s[0], 16), s[2]))
                               for k, s in self._shapes.items() if self._is_dw(k, s)), dtype=torch.uint8, device=self.device)

    def _dw(self, x, name, stride):
        """Depthwise conv (shufflenetv2.py:54, :66; the depthwise member of an InvertedResidual) straight from the
        parameter, whose shape gives the kernel size; its input gradient accumulates when the input already has one (the
        input of a stride-2 ShuffleNetV2 unit feeds both branches)."""
        L = _lib.lib()
        key = name + ".weight"
        c_real, ks = self._shapes[key][0], self._shapes[key][2]
        if x.c != c_real:
            raise ValueError("%s: expects %d channels, got %d" % (name, c_real, x.c))
        y = self._new(x.n, (x.h - 1) // stride + 1, (x.w - 1) // stride + 1, x.c)
        _lib.check(L.udp_dwconvk_train_fwd(x.buf.data_ptr(), self._p(key), x.n, x.h, x.w, x.ck, c_real, ks, stride, self._dt,
                                           y.buf.data_ptr(), self._stream()))

        def backward():
            dy = y.grad
            self._on_side(lambda: _lib.check(L.udp_dwconvk_wgrad(
                x.buf.data_ptr(), dy.data_ptr(), x.n, x.h, x.w, x.ck, c_real, ks, stride, self._dt, self._g(key),
                self._dw_ws.data_ptr(), self._dw_ws.numel(), self._stream())), dy, x.buf)
            if not x.needs_grad:
                return
            have = x.grad is not None
            if not have:
                x.grad = self._like(x)
            _lib.check(L.udp_dwconvk_dgrad(dy.data_ptr(), self._p(key), x.n, x.h, x.w, x.ck, c_real, ks, stride, int(have),
                                           self._dt, x.grad.data_ptr(), self._stream()))
        self._tape.append((y, backward, None, [key]))
        return y

    def _one_consumer(self, what, *xs):
        if any(x.grad is not None for x in xs):
            raise RuntimeError("%s: its inputs have one consumer" % what)

    def _shuffle(self, a, b):
        """channel_shuffle of cat(a, b) (:86-92): (even, odd) logical channels."""
        L = _lib.lib()
        if a.c != b.c or a.ck != b.ck:
            raise ValueError("channel shuffle: halves of %d and %d channels" % (a.c, b.c))
        m = a.n * a.h * a.w
        even, odd = self._new(a.n, a.h, a.w, a.c), self._new(a.n, a.h, a.w, a.c)
        _lib.check(L.udp_shuffle_pair_fwd(a.buf.data_ptr(), b.buf.data_ptr(), m, a.c, a.ck, even.ck, self._dt,
                                          even.buf.data_ptr(), odd.buf.data_ptr(), self._stream()))

        def backward():
            self._one_consumer("channel shuffle", a, b)
            for t in (even, odd):
                if t.grad is None:
                    t.grad = torch.zeros_like(t.buf)
            a.grad, b.grad = self._like(a), self._like(b)
            _lib.check(L.udp_shuffle_pair_bwd(even.grad.data_ptr(), odd.grad.data_ptr(), m, a.c, even.ck, a.ck, self._dt,
                                              a.grad.data_ptr(), b.grad.data_ptr(), self._stream()))
        self._tape.append((_Group([even, odd]), backward, None, []))
        return even, odd

    def _cat(self, a, b):
        """torch.cat((a, b), 1) (:92) materialised."""
        L = _lib.lib()
        m = a.n * a.h * a.w
        y = self._new(a.n, a.h, a.w, a.c + b.c)
        _lib.check(L.udp_chan_cat2(a.buf.data_ptr(), a.ck, a.c, b.buf.data_ptr(), b.ck, b.c, m, y.ck, self._dt,
                                   y.buf.data_ptr(), self._stream()))

        def backward():
            self._one_consumer("concat", a, b)
            a.grad, b.grad = self._like(a), self._like(b)
            _lib.check(L.udp_chan_uncat2(y.grad.data_ptr(), y.ck, m, self._dt, a.grad.data_ptr(), a.ck, a.c,
                                         b.grad.data_ptr(), b.ck, b.c, self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    def _split(self, y, ra, rb):
        """(y[:, :ra], y[:, ra:ra+rb]) as a pair of halves."""
        L = _lib.lib()
        m = y.n * y.h * y.w
        a, b = self._new(y.n, y.h, y.w, ra), self._new(y.n, y.h, y.w, rb)
        _lib.check(L.udp_chan_uncat2(y.buf.data_ptr(), y.ck, m, self._dt, a.buf.data_ptr(), a.ck, ra, b.buf.data_ptr(),
                                     b.ck, rb, self._stream()))

        def backward():
            self._one_consumer("split", y)
            for t in (a, b):
                if t.grad is None:
                    t.grad = torch.zeros_like(t.buf)
            y.grad = self._like(y)
            _lib.check(L.udp_chan_cat2(a.grad.data_ptr(), a.ck, ra, b.grad.data_ptr(), b.ck, rb, m, y.ck, self._dt,
                                       y.grad.data_ptr(), self._stream()))
        self._tape.append((_Group([a, b]), backward, None, []))
        return a, b

    def _pixshuf(self, x):
        """nn.PixelShuffle(2) (DUC.py:27)."""
        L = _lib.lib()
        if x.c != x.ck or x.c % 64:
            raise ValueError("pixel shuffle over %d channels (a multiple of 64)" % x.c)
        y = self._new(x.n, 2 * x.h, 2 * x.w, x.c // 4)
        _lib.check(L.udp_pixshuf2_train_fwd(x.buf.data_ptr(), x.n, x.h, x.w, x.c, self._dt, y.buf.data_ptr(), self._stream()))

        def backward():
            self._one_consumer("pixel shuffle", x)
            x.grad = self._like(x)
            _lib.check(L.udp_pixshuf2_train_bwd(y.grad.data_ptr(), x.n, x.h, x.w, x.c, self._dt, x.grad.data_ptr(),
                                                self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    # ------------------------------------------------------------------ the graph (shufflenetv2.py:77-92, :154-158)
    def _main(self, x, p, stride):
        m = self._bn(self._conv(x, p + ".branch_main.0", bn_stats=True), p + ".branch_main.1")               # pw (:50-52)
        m = self._bn(self._dw(m, p + ".branch_main.3", stride), p + ".branch_main.4", relu=False)            # dw (:54-55)
        return self._bn(self._conv(m, p + ".branch_main.5", bn_stats=True), p + ".branch_main.6")            # pw (:57-59)

    def _unit_s2(self, x, p):
        proj = self._bn(self._dw(x, p + ".branch_proj.0", 2), p + ".branch_proj.1", relu=False)              # dw (:66-67)
        proj = self._bn(self._conv(proj, p + ".branch_proj.2", bn_stats=True), p + ".branch_proj.3")         # pw (:69-71)
        return proj, self._main(x, p, 2)

    def _unit_s1(self, pair, p):
        even, odd = self._shuffle(*pair)
        return even, self._main(odd, p, 1)

    def _head(self, a):
        """PixelShuffleDecoder (decoders/pixelshuffle.py:29-33, DUC.py:23-28)."""
        a = self._conv(a, "decoder.conv_compress")
        for d in range(len(self.spec["architecture"])):
            a = self._pixshuf(self._bn(self._conv(a, "decoder.duc.%d.conv" % d, bn_stats=True), "decoder.duc.%d.bn" % d))
        return a

    def forward(self, x):
        """Train-mode forward.  x: fp32 [N,3,H,W] on the device.  Returns fp32 [N,C,H/4,W/4]."""
        L = _lib.lib()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [N,3,H,W]")
        n, _, h, w = x.shape
        if h % 32 or w % 32:
            raise ValueError("input %dx%d must be a multiple of 32" % (h, w))
        self._tape = []
        _lib.check(L.udp_pack_conv_weights_batch(self._pack_table.data_ptr(), len(self._convs), self._dt, self._stream()))
        a = self._new(n, h, w, 3, needs_grad=False)
        _lib.check(L.udp_nchw_to_nhwc(x.data_ptr(), n, 3, h, w, a.ck, a.buf.data_ptr(), self._dt, self._stream()))
        a = self._bn(self._conv(a, "backbone.first_conv.0", stride=2, bn_stats=True), "backbone.first_conv.1")   # :118-122
        a = self._maxpool(a)                                                                                     # :124
        pair = None
        for idx, inp, oup, mid, stride in self._units:
            p = "backbone.features.%d" % idx
            if stride == 2:
                if pair is not None:
                    a = self._cat(*pair)
                pair = self._unit_s2(a, p)
                if pair[0].c != pair[1].c:         # the first unit: inp and oup - inp channels; the shuffle wants halves
                    half = (pair[0].c + pair[1].c) // 2
                    pair = self._split(self._cat(*pair), half, half)
            else:
                pair = self._unit_s1(pair, p)
        a = self._cat(*pair)
        a = self._bn(self._conv(a, "backbone.conv_last.0", bn_stats=True), "backbone.conv_last.1")               # :143-147
        a = self._head(a)
        self._out = self._conv(a, "final_layer", bias_key="final_layer.bias", nchw_out=True)
        return self._out.buf


class ShuffleNetV2DeconvTrainer(ShuffleNetV2Trainer):
    """pose_shufflenetv2_10x (pose_shufflenetv2_10x.py:22-97; recipe experiments/coco/shufflenetv2/10x_256x192_adam_lr1e-3.yaml):
    the same backbone, the deconv head of pose_resnet behind ``conv_last``.  ``spec``: ``shufflenet_plan.shufflenet_deconv_spec``."""

    NAME = "pose_shufflenetv2_10x"

    def _head_shapes(self, num_joints, target_type):
        from .synth_shufflenet import shufflenet_deconv_param_shapes
        sp = self.spec
        if any(f % 16 for f in sp["deconv_filters"]):
            raise ValueError("%s trainer: deconv filters in multiples of 16 (got %s)" % (self.NAME, tuple(sp["deconv_filters"])))
        return shufflenet_deconv_param_shapes(model_size=sp["model_size"], num_joints=int(num_joints), target_type=target_type,
                                              deconv_filters=tuple(sp["deconv_filters"]), final_kernel=sp["final_kernel"],
                                              deconv_with_bias=sp["deconv_with_bias"])

    def _head(self, a):
        for d in range(len(self.spec["deconv_filters"])):
            q = "deconv_layers.%d" % (3 * d)
            a = self._bn(self._deconv(a, q, q + ".bias" if self.spec["deconv_with_bias"] else None),
                         "deconv_layers.%d" % (3 * d + 1))
        return a


class MobileNetV3Trainer(ShuffleNetV2Trainer):
    """pose_mobilenetv3_small_pixel_shuffle (deep_hrnet/lib/models/pose_mobilenetv3_small_pixel_shuffle.py:23-52; recipe
    experiments/coco/mobilenetv3/small_256x192_adam_lr1e-3_pixel_shuffle.yaml) on the base step.  ``spec``: the dict of
    ``mobilenetv3_plan.mobilenetv3_ps_spec``.  The backbone is torchvision's ``mobilenet_v3_small().features``
    (backbones/mobilenetv3.py:5-16), i.e. the block table ``synth_mobilenetv3.BLOCKS``; its BatchNorms run with
    eps 1e-3 / momentum 0.01 (torchvision's ``partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)``), the heads keep
    1e-5 / 0.1.  fp32 only: the reference's precision, and the depthwise / squeeze-excitation kernels have no bf16 form.

    What it takes from ``ShuffleNetV2Trainer``: the padded layout (``_key_stride``, ``bn_over_stored`` -- 72, 88, 120, 24
    and 40 channels are stored as 80, 96, 128, 32 and 48), ``_pixshuf`` and the head.  The depthwise weights and the
    squeeze-excitation's ``fc1`` / ``fc2`` are read by their kernels as they are (no pack step); their gradients land in
    ``grad`` under their own keys."""

    NAME = "pose_mobilenetv3_small_pixel_shuffle"
    BACKBONE_BN = dict(eps=1e-3, momentum=0.01)

    def __init__(self, spec, num_joints, target_type, state_dict, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, bucket_elems=6 * 1024 * 1024):
        from .synth_mobilenetv3 import BLOCKS
        if dtype != "f32":
            raise ValueError("%s trains in fp32 only (dtype %r): the depthwise and squeeze-excitation kernels have no bf16 "
                             "form" % (self.NAME, dtype))
        self.spec = dict(spec)
        self._blocks = BLOCKS
        shapes = self._head_shapes(num_joints, target_type)
        Trainer.__init__(self, shapes, state_dict, num_joints, target_type, device=device, dtype=dtype, lr=lr, betas=betas,
                         eps=eps, bucket_elems=bucket_elems)
        self._dw_ws = self._dw_workspace()

    def _head_shapes(self, num_joints, target_type):
        from .synth_mobilenetv3 import mobilenetv3_ps_param_shapes
        sp = self.spec
        if any(a % 64 for a in sp["architecture"]):
            raise ValueError("%s trainer: ARCHITECTURE=%s -- the pixel shuffle moves 16 input channels per thread, every entry "
                             "must be a multiple of 64" % (self.NAME, tuple(sp["architecture"])))
        return mobilenetv3_ps_param_shapes(num_joints=int(num_joints), target_type=target_type,
                                           start_channels=sp["start_channels"], architecture=tuple(sp["architecture"]),
                                           final_kernel=sp["final_kernel"])

    @staticmethod
    def _is_dw(key, shape):
        return len(shape) == 4 and shape[1] == 1 and shape[2] > 1 and key.startswith("backbone.0.")

    def _conv_entry(self, key, shape):
        if self._is_dw(key, shape) or ".fc1." in key or ".fc2." in key:
            return None                     # the depthwise and squeeze-excitation kernels read the parameters as they are
        if key.startswith("deconv_layers."):
            return shape[1], shape[0], shape[2], True, True       # ConvTranspose2d.weight is [cin][cout][k][k]
        return shape[0], shape[1], shape[2], False, key != "backbone.0.0.0.weight"

    # ------------------------------------------------------------------ the ops the other nets do not have
    def _hswish(self, x):
        """nn.Hardswish behind a BatchNorm that ran with relu=False; ``x`` stays on the tape for the derivative."""
        L = _lib.lib()
        y = self._new(x.n, x.h, x.w, x.c)
        _lib.check(L.udp_hswish_fwd(x.buf.data_ptr(), y.buf.data_ptr(), x.buf.numel(), self._stream()))

        def backward():
            self._one_consumer("hard-swish", x)
            x.grad = self._like(x)
            _lib.check(L.udp_hswish_bwd(y.grad.data_ptr(), x.buf.data_ptr(), x.grad.data_ptr(), x.buf.numel(), self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    def _bn_act(self, x, name, hs):
        """A backbone BatchNorm + its activation: ReLU inside the BatchNorm kernels, hard-swish as one more launch."""
        if not hs:
            return self._bn(x, name, **self.BACKBONE_BN)
        return self._hswish(self._bn(x, name, relu=False, **self.BACKBONE_BN))

    def _se(self, x, name):
        """torchvision.ops.SqueezeExcitation ``name`` (fc1 / fc2 with biases) in train mode."""
        L = _lib.lib()
        keys = [name + k for k in (".fc1.weight", ".fc1.bias", ".fc2.weight", ".fc2.bias")]
        sq = self._shapes[keys[0]][0]
        if tuple(self._shapes[keys[0]]) != (sq, x.c, 1, 1) or tuple(self._shapes[keys[2]]) != (x.c, sq, 1, 1):
            raise ValueError("%s: squeeze-excitation over %d channels, weights %s / %s" % (name, x.c, self._shapes[keys[0]], self._shapes[keys[2]]))
        pool = torch.empty(x.n * x.ck, dtype=torch.float32, device=self.device)
        hid = torch.empty(x.n * sq, dtype=torch.float32, device=self.device)
        s = torch.empty(x.n * x.ck, dtype=torch.float32, device=self.device)
        y = self._new(x.n, x.h, x.w, x.c)
        _lib.check(L.udp_se_train_fwd(x.buf.data_ptr(), *[self._p(k) for k in keys], x.n, x.h, x.w, x.ck, x.c, sq, self._dt,
                                      pool.data_ptr(), hid.data_ptr(), s.data_ptr(), y.buf.data_ptr(), self._stream()))

        def backward():
            have = x.grad is not None
            if not have:
                x.grad = self._like(x)
            ws = torch.empty(int(L.udp_se_train_workspace_bytes(x.n, x.ck, sq)), dtype=torch.uint8, device=self.device)
            _lib.check(L.udp_se_train_bwd(y.grad.data_ptr(), x.buf.data_ptr(), self._p(keys[0]), self._p(keys[2]), pool.data_ptr(),
                                          hid.data_ptr(), s.data_ptr(), x.n, x.h, x.w, x.ck, x.c, sq, int(have), self._dt,
                                          x.grad.data_ptr(), self._g(keys[0]), self._g(keys[1]), self._g(keys[2]), self._g(keys[3]),
                                          ws.data_ptr(), ws.numel(), self._stream()))
        self._tape.append((y, backward, (pool, hid, s), keys))
        return y

    # ------------------------------------------------------------------ the graph (synth_mobilenetv3.BLOCKS)
    def _block(self, x, i, cin, ks, exp, cout, se, act, stride):
        """InvertedResidual ``backbone.0.<i>``: expand 1x1 (when exp != in), depthwise ks x ks with the stride, the
        squeeze-excitation behind the activation, project 1x1 whose BatchNorm has no activation; ``x + block(x)`` when
        the stride is 1 and in == out (the shortcut is the ``res`` of the project BatchNorm)."""
        p, m, hs = "backbone.0.%d.block" % i, 0, act == "HS"
        y = x
        if exp != cin:
            y = self._bn_act(self._conv(y, "%s.%d.0" % (p, m), bn_stats=True), "%s.%d.1" % (p, m), hs)
            m += 1
        y = self._bn_act(self._dw(y, "%s.%d.0" % (p, m), stride), "%s.%d.1" % (p, m), hs)
        m += 1
        if se:
            y = self._se(y, "%s.%d" % (p, m))
            m += 1
        res = x if stride == 1 and cin == cout else None
        return self._bn(self._conv(y, "%s.%d.0" % (p, m), bn_stats=True), "%s.%d.1" % (p, m), relu=False, res=res,
                        **self.BACKBONE_BN)

    def forward(self, x):
        """Train-mode forward.  x: fp32 [N,3,H,W] on the device.  Returns fp32 [N,C,H/4,W/4]."""
        L = _lib.lib()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [N,3,H,W]")
        n, _, h, w = x.shape
        if h % 32 or w % 32:
            raise ValueError("input %dx%d must be a multiple of 32" % (h, w))
        self._tape = []
        _lib.check(L.udp_pack_conv_weights_batch(self._pack_table.data_ptr(), len(self._convs), self._dt, self._stream()))
        a = self._new(n, h, w, 3, needs_grad=False)
        _lib.check(L.udp_nchw_to_nhwc(x.data_ptr(), n, 3, h, w, a.ck, a.buf.data_ptr(), self._dt, self._stream()))
        a = self._bn_act(self._conv(a, "backbone.0.0.0", stride=2, bn_stats=True), "backbone.0.0.1", True)
        for i, blk in enumerate(self._blocks, start=1):
            a = self._block(a, i, *blk)
        a = self._bn_act(self._conv(a, "backbone.0.12.0", bn_stats=True), "backbone.0.12.1", True)
        a = self._head(a)
        self._out = self._conv(a, "final_layer", bias_key="final_layer.bias", nchw_out=True)
        return self._out.buf


class MobileNetV3DeconvTrainer(MobileNetV3Trainer):
    """pose_mobilenetv3_small (pose_mobilenetv3_small.py; recipe experiments/coco/mobilenetv3/small_256x192_adam_lr1e-3.yaml):
    the same backbone, the deconv head of pose_resnet behind ``backbone.0.12``.  ``spec``: ``mobilenetv3_plan.mobilenetv3_deconv_spec``."""

    NAME = "pose_mobilenetv3_small"

    def _head_shapes(self, num_joints, target_type):
        from .synth_mobilenetv3 import mobilenetv3_deconv_param_shapes
        sp = self.spec
        if any(f % 16 for f in sp["deconv_filters"]):
            raise ValueError("%s trainer: deconv filters in multiples of 16 (got %s)" % (self.NAME, tuple(sp["deconv_filters"])))
        return mobilenetv3_deconv_param_shapes(num_joints=int(num_joints), target_type=target_type,
                                               deconv_filters=tuple(sp["deconv_filters"]), final_kernel=sp["final_kernel"],
                                               deconv_with_bias=sp["deconv_with_bias"])

    _head = ShuffleNetV2DeconvTrainer._head


class MobileViTv2Trainer(ShuffleNetV2Trainer):
    """pose_mobilevitv2_pixel_shuffle (deep_hrnet/lib/models/pose_mobilevitv2_pixel_shuffle.py:23-60; recipes
    experiments/coco/mobilevitv2/mobilevitv2-{0.5,0.75,1.0}_256x192_adam_lr1e-3_pixel_shuffle.yaml) on the base step.
    ``spec``: the dict of ``mobilevitv2_plan.mobilevitv2_spec``.  The graph is tests/mobilevitv2_ref.py's, op for op, in
    train mode; it is deterministic -- the backbone YAMLs set no dropout (backbones/mobilevitv2.py:1340-1357).  The
    backbone's BatchNorms are nn.BatchNorm2d(momentum=0.1) with the default eps 1e-5 (get_normalization_layer :115-120,
    ``model.normalization.momentum`` of backbones/configs/mobilevitv2-*.yaml): ``_bn``'s defaults.  fp32 only: the
    reference's precision, and the depthwise, GroupNorm and attention kernels have no bf16 form.

    What it takes from ``ShuffleNetV2Trainer``: the padded layout (``_key_stride``, ``bn_over_stored`` -- the 0.75 width
    has 24- and 48-channel tensors, and every qkv map has 1 + 2d channels), ``_dw`` for every [C][1][3][3] weight,
    ``_pixshuf`` and the head.  The qkv map keeps the PARAMETER's channel order (query | keys | values), so the weight
    gradient lands in the parameter layout.  ``backbone.classifier.1.*`` are parameters the forward never applies
    (:1440-1444): their gradient stays zero."""

    NAME = "pose_mobilevitv2_pixel_shuffle"
    GN_EPS = 1e-5                        # nn.GroupNorm's default (:139-140 passes none)

    def __init__(self, spec, num_joints, target_type, state_dict, device="cuda", dtype="f32", lr=1e-3, betas=(0.9, 0.999),
                 eps=1e-8, bucket_elems=6 * 1024 * 1024):
        if dtype != "f32":
            raise ValueError("%s trains in fp32 only (dtype %r): the depthwise, GroupNorm and attention kernels have no bf16 "
                             "form" % (self.NAME, dtype))
        self.spec = dict(spec)
        shapes = self._head_shapes(num_joints, target_type)
        Trainer.__init__(self, shapes, state_dict, num_joints, target_type, device=device, dtype=dtype, lr=lr, betas=betas,
                         eps=eps, bucket_elems=bucket_elems)
        self._dw_ws = self._dw_workspace()

    def _head_shapes(self, num_joints, target_type):
        from .synth_mobilevitv2 import mobilevitv2_param_shapes
        sp = self.spec
        if any(a % 64 for a in sp["architecture"]):
            raise ValueError("%s trainer: ARCHITECTURE=%s -- the pixel shuffle moves 16 input channels per thread, every entry "
                             "must be a multiple of 64" % (self.NAME, tuple(sp["architecture"])))
        return mobilevitv2_param_shapes(model_size=sp["model_size"], num_joints=int(num_joints), target_type=target_type,
                                        start_channels=sp["start_channels"], architecture=tuple(sp["architecture"]),
                                        final_kernel=sp["final_kernel"])

    @staticmethod
    def _is_dw(key, shape):
        return len(shape) == 4 and shape[1] == 1 and shape[2] == 3 and key.startswith("backbone.")

    def _conv_entry(self, key, shape):
        if self._is_dw(key, shape):
            return None                     # the depthwise kernels read the parameter as it is
        return shape[0], shape[1], shape[2], False, key != "backbone.conv_1.block.conv.weight"

    # ------------------------------------------------------------------ the ops the other nets do not have
    def _silu(self, x):
        """nn.SiLU behind a BatchNorm that ran with relu=False, or behind a biased conv; ``x`` stays on the tape for the
        derivative."""
        L = _lib.lib()
        y = self._new(x.n, x.h, x.w, x.c)
        _lib.check(L.udp_silu_fwd(x.buf.data_ptr(), y.buf.data_ptr(), x.buf.numel(), self._stream()))

        def backward():
            self._one_consumer("SiLU", x)
            x.grad = self._like(x)
            _lib.check(L.udp_silu_bwd(y.grad.data_ptr(), x.buf.data_ptr(), x.grad.data_ptr(), x.buf.numel(), self._stream()))
        self._tape.append((y, backward, None, []))
        return y

    def _gnorm(self, x, name):
        """GroupNorm(1, C) ``name`` in train mode; its input gradient accumulates when the input already has one (the
        input of every GroupNorm of a LinearAttnFFN also feeds the residual)."""
        L = _lib.lib()
        keys = [name + ".weight", name + ".bias"]
        if tuple(self._shapes[keys[0]]) != (x.c,):
            raise ValueError("%s: GroupNorm over %d channels, weight %s" % (name, x.c, self._shapes[keys[0]]))
        y = self._new(x.n, x.h, x.w, x.c)
        save = torch.empty(2 * x.n, dtype=torch.float32, device=self.device)
        nbytes = int(L.udp_gnorm_train_workspace_bytes(x.n, x.h, x.w, x.ck))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        _lib.check(L.udp_gnorm_train_fwd(x.buf.data_ptr(), self._p(keys[0]), self._p(keys[1]), x.n, x.h, x.w, x.ck, x.c, self._dt,
                                         self.GN_EPS, y.buf.data_ptr(), save.data_ptr(), ws.data_ptr(), nbytes, self._stream()))

        def backward():
            have = x.grad is not None
            if not have:
                x.grad = self._like(x)
            bws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(L.udp_gnorm_train_bwd(y.grad.data_ptr(), x.buf.data_ptr(), self._p(keys[0]), save.data_ptr(), x.n, x.h,
                                             x.w, x.ck, x.c, self._dt, int(have), x.grad.data_ptr(), self._g(keys[0]),
                                             self._g(keys[1]), bws.data_ptr(), nbytes, self._stream()))
        self._tape.append((y, backward, save, keys))
        return y

    def _linattn(self, qkv, d):
        """The separable self-attention core between qkv_proj and out_proj (mobilevitv2.py:671-689) on the qkv map."""
        L = _lib.lib()
        if qkv.c != 1 + 2 * d:
            raise ValueError("linear attention: a qkv map of %d channels for d = %d" % (qkv.c, d))
        y = self._new(qkv.n, qkv.h, qkv.w, d)
        m = qkv.h * qkv.w // 4
        scores = torch.empty(qkv.n * 4 * m, dtype=torch.float32, device=self.device)
        ctx = torch.empty(qkv.n * 4 * d, dtype=torch.float32, device=self.device)
        _lib.check(L.udp_linattn_train_fwd(qkv.buf.data_ptr(), qkv.n, qkv.h, qkv.w, qkv.ck, d, self._dt, y.buf.data_ptr(), y.ck,
                                           scores.data_ptr(), ctx.data_ptr(), self._stream()))

        def backward():
            self._one_consumer("linear attention", qkv)
            qkv.grad = self._like(qkv)
            _lib.check(L.udp_linattn_train_bwd(y.grad.data_ptr(), qkv.buf.data_ptr(), scores.data_ptr(), ctx.data_ptr(), qkv.n,
                                               qkv.h, qkv.w, qkv.ck, d, y.ck, self._dt, qkv.grad.data_ptr(), self._stream()))
        self._tape.append((y, backward, (scores, ctx), []))
        return y

    # ------------------------------------------------------------------ the graph (tests/mobilevitv2_ref.py)
    def _cbn(self, x, name, act, stride=1, dw=False, res=None):
        """ConvLayer with a norm (:321-345): conv or depthwise conv, BatchNorm, SiLU when ``act``."""
        if dw:
            y = self._dw(x, name + ".block.conv", stride)
        else:
            y = self._conv(x, name + ".block.conv", stride=stride, bn_stats=True)
        y = self._bn(y, name + ".block.norm", relu=False, res=res)
        return self._silu(y) if act else y

    def _inverted_residual(self, x, p, stride):
        """InvertedResidual.forward (:226-230); the shortcut is the ``res`` of the red_1x1 BatchNorm."""
        y = self._cbn(x, p + ".block.exp_1x1", True)
        y = self._cbn(y, p + ".block.conv_3x3", True, stride=stride, dw=True)
        cout = self._shapes[p + ".block.red_1x1.block.conv.weight"][0]
        return self._cbn(y, p + ".block.red_1x1", False, res=x if stride == 1 and x.c == cout else None)

    def _biased(self, x, name, res=None):
        return self._conv(x, name + ".block.conv", bias_key=name + ".block.conv.bias", res=res)

    def _mit_block(self, x, q):
        """MobileViTBlockv2.forward_spatial (:1105-1126), map form."""
        t = self._cbn(x, q + ".local_rep.0", True, dw=True)
        t = self._conv(t, q + ".local_rep.1.block.conv")
        d, u = t.c, 0
        while ("%s.global_rep.%d.pre_norm_attn.0.weight" % (q, u)) in self._shapes:            # LinearAttnFFN.forward (:839-855)
            g = "%s.global_rep.%d" % (q, u)
            qkv = self._biased(self._gnorm(t, g + ".pre_norm_attn.0"), g + ".pre_norm_attn.1.qkv_proj")
            t = self._biased(self._linattn(qkv, d), g + ".pre_norm_attn.1.out_proj", res=t)
            f = self._silu(self._biased(self._gnorm(t, g + ".pre_norm_ffn.0"), g + ".pre_norm_ffn.1"))
            t = self._biased(f, g + ".pre_norm_ffn.3", res=t)
            u += 1
        t = self._gnorm(t, "%s.global_rep.%d" % (q, u))
        return self._cbn(t, q + ".conv_proj", False)

    def forward(self, x):
        """Train-mode forward.  x: fp32 [N,3,H,W] on the device.  Returns fp32 [N,C,H/4,W/4]."""
        L = _lib.lib()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
            raise ValueError("expected contiguous fp32 [N,3,H,W]")
        n, _, h, w = x.shape
        if h % 64 or w % 64:
            raise ValueError("input %dx%d must be a multiple of 64 (2x2 patches on the 1/32 map)" % (h, w))
        self._tape = []
        _lib.check(L.udp_pack_conv_weights_batch(self._pack_table.data_ptr(), len(self._convs), self._dt, self._stream()))
        a = self._new(n, h, w, 3, needs_grad=False)
        _lib.check(L.udp_nchw_to_nhwc(x.data_ptr(), n, 3, h, w, a.ck, a.buf.data_ptr(), self._dt, self._stream()))
        a = self._cbn(a, "backbone.conv_1", True, stride=2)                                     # :1198-1206
        a = self._inverted_residual(a, "backbone.layer_1.0", 1)
        a = self._inverted_residual(a, "backbone.layer_2.0", 2)
        a = self._inverted_residual(a, "backbone.layer_2.1", 1)
        for layer in (3, 4, 5):                                                                 # :1313-1366
            a = self._inverted_residual(a, "backbone.layer_%d.0" % layer, 2)
            a = self._mit_block(a, "backbone.layer_%d.1" % layer)
        a = self._head(a)
        self._out = self._conv(a, "final_layer", bias_key="final_layer.bias", nchw_out=True)
        return self._out.buf
