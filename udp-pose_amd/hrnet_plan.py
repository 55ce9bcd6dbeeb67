"""Host-side compiler for HRNet / HRNet-PSA: reference YAML (MODEL.EXTRA) + state_dict -> fused op program
(program.Program: the op records, the weight blob and the buffer assignment are built there).

Walks the same graph as PoseHighResolutionNet.forward
(deep_hrnet/lib/models/pose_hrnet.py:436-471; modules :260-273, fuse layers
:189-255, transitions :344-383, Bottleneck :62-100, BasicBlock :29-59) and
emits one ``udp_conv_op`` (include/udp_pose_hip.h) per fused launch:

    out = act( conv(in) + bias [+ res] [+ sum_k nearest_up(up_k)] )

* An exchange-unit output y_i = ReLU(sum_j f_ij(x_j)) (:267-272) becomes: the
  1x1 convs of the j>i terms write low-resolution temporaries; the last 3x3
  stride-2 conv of each j<i chain adds the running sum (identity term, the
  upsampled temporaries, earlier chains) in its epilogue, the final one applies
  the ReLU; output 0 has no conv term and is one element-wise launch (or, in the
  last stage-4 module, the epilogue of its 1x1 C->4C conv, :213-221).
"""
import os

from . import _lib
from .program import BN_EPS, DTYPES, Program, _T, _V, _round_up, encode_weights, storage_bytes  # noqa: F401 (re-exported)


class HRNetProgram(Program):
    def __init__(self, state_dict, extra, in_h, in_w, dtype="f32"):
        self.extra = extra
        self.fuse_blocks = os.environ.get("UDP_POSE_NO_BLOCK_FUSION") is None
        self.block_major = dtype in ("bf16", "f16x2")       # modules emitted block by block over all branches
        self.group_convs = self.block_major and os.environ.get("UDP_POSE_NO_GROUPS") is None
        self._groups = 0
        super().__init__(state_dict, in_h, in_w, dtype)

    def _next_group(self):
        self._groups += 1
        return self._groups

    def _basic_block(self, x, q):
        """BasicBlock.forward (pose_hrnet.py:43-59; PSA variant pose_hrnet_psa.py:37,49)."""
        if self._can_fuse_block(x, q):
            return self._block(x, q)
        t = self._conv(x, q + ".conv1", q + ".bn1")
        if (q + ".deattn.conv_q_right.weight") in self.sd:
            t = self._psa(t, q + ".deattn")
        return self._conv(t, q + ".conv2", q + ".bn2", res=x)

    def _can_fuse_block(self, x, q):
        """The fused BasicBlock kernel (csrc/conv.hip basic_block_c32_kernel): bf16, 32 channels, rows in
        tiles of 8, the staged (8+4) x (W+2) input tile within 640 LDS rows, no attention inside."""
        return (self.dtype == "bf16" and self.fuse_blocks and x.c == 32 and x.h % 8 == 0 and 12 * (x.w + 2) <= 640
                and x.w in (48, 24, 16, 8) and (q + ".deattn.conv_q_right.weight") not in self.sd
                and tuple(self.sd[q + ".conv1.weight"].shape) == (32, 32, 3, 3)
                and tuple(self.sd[q + ".conv2.weight"].shape) == (32, 32, 3, 3))

    def _block(self, x, q):
        w1, b1 = self._pack(*self._fold(q + ".conv1", q + ".bn1"))[:2]
        w2, b2 = self._pack(*self._fold(q + ".conv2", q + ".bn2"))[:2]
        out = self._new(32, x.h, x.w)
        self._emit(_lib.UDP_OP_BLOCK, q + ".block", x, out, ks=3, relu=1, w_off=w1, b_off=b1, w2_off=w2, b2_off=b2)
        return out

    def _build(self):
        sd = self.sd
        H, W = self.in_h, self.in_w
        x = self._stem(_lib.UDP_OP_STEM, "conv1", "bn1", 3)
        # The first Bottleneck's projection shortcut (pose_hrnet.py:87-98: out = relu(bn3(conv3(t)) + bn_d(conv_d(x))))
        # is a second 1x1 conv of the same shape as conv3: with t and x side by side in one tensor the two are ONE
        # 1x1 conv over the concatenated channels -- the 4*planes-channel shortcut map is never written nor read back.
        # (UDP_POSE_NO_L1_CONCAT=1: the two convs and the residual read, for A/B)
        p0 = "layer1.0"
        concat = (os.environ.get("UDP_POSE_NO_L1_CONCAT") is None and (p0 + ".downsample.0.weight") in sd
                  and tuple(sd[p0 + ".downsample.0.weight"].shape[1:]) == (64, 1, 1)
                  and tuple(sd[p0 + ".conv3.weight"].shape[1:]) == (64, 1, 1)
                  and tuple(sd[p0 + ".conv2.weight"].shape[:2]) == (64, 64))
        # conv3 (+ shortcut + ReLU) of a Bottleneck and conv1 (+ ReLU) of the next one are both 1x1: chained in one launch
        # (udp_conv_op.chain_cout) the 256-channel map between them is written once and not read back.  Split-fp16 storage
        # on the weight-stationary kernels only.  (UDP_POSE_NO_L1_CHAIN=1: separate launches, for A/B)
        def nxt(k):
            q = "layer1.%d" % (k + 1)
            ok = (self.use_ws and os.environ.get("UDP_POSE_NO_L1_CHAIN") is None and k + 1 < 4
                  and (q + ".downsample.0.weight") not in sd and tuple(sd[q + ".conv1.weight"].shape) == (64, 256, 1, 1)
                  and tuple(sd["layer1.%d.conv3.weight" % k].shape) == (256, 64, 1, 1))
            return (q + ".conv1", q + ".bn1") if ok else None
        a = None                                                     # conv1 output of the block, when chained in
        if concat:
            cat = self._new(128, H // 4, W // 4)                     # [conv2 output t | block input x]
            self._conv(x, "conv2", "bn2", stride=2, into=(cat, 64))
            a = self._conv(cat, p0 + ".conv1", p0 + ".bn1", in_coff=64)
            self._conv(a, p0 + ".conv2", p0 + ".bn2", into=(cat, 0))
            x = self._conv(cat, p0 + ".conv3", p0 + ".bn3", plus=(p0 + ".downsample.0", p0 + ".downsample.1"), chain=nxt(0))
            x, a = x if isinstance(x, tuple) else (x, None)
        else:
            x = self._conv(x, "conv2", "bn2", stride=2)
        for k in range(1 if concat else 0, 4):                       # layer1 (:297, Bottleneck :80-100)
            p = "layer1.%d" % k
            if a is None:
                a = self._conv(x, p + ".conv1", p + ".bn1")
            bt = self._conv(a, p + ".conv2", p + ".bn2")
            r = x
            if (p + ".downsample.0.weight") in sd:
                r = self._conv(x, p + ".downsample.0", p + ".downsample.1", relu=False)
            x = self._conv(bt, p + ".conv3", p + ".bn3", res=r, chain=nxt(k))
            x, a = x if isinstance(x, tuple) else (x, None)
        ys = [x]
        for st in (2, 3, 4):
            cfg = self.extra["STAGE%d" % st]
            if cfg["BLOCK"] != "BASIC" or cfg.get("FUSE_METHOD", "SUM") != "SUM":
                raise ValueError("stage %d: only BASIC blocks with SUM fusion are supported" % st)
            nb = cfg["NUM_BRANCHES"]
            if nb != len(cfg["NUM_BLOCKS"]) or nb != len(cfg["NUM_CHANNELS"]):
                raise ValueError("NUM_BRANCHES(%d) <> NUM_BLOCKS/NUM_CHANNELS" % nb)   # pose_hrnet.py:121-139
            xs = self._transition(ys, "transition%d" % (st - 1), nb)
            for m in range(cfg["NUM_MODULES"]):
                last = (st == 4 and m == cfg["NUM_MODULES"] - 1)
                xs = self._module(xs, "stage%d.%d" % (st, m), cfg["NUM_BLOCKS"], last)
            ys = xs
        self._conv(ys[0], "final_layer", None, relu=False, to_output=True)
        self.out_channels = self._ops[-1]["cout"]

    def _transition(self, ys, name, n_cur):
        xs = []
        for i in range(n_cur):
            q = "%s.%d" % (name, i)
            if i < len(ys):
                if (q + ".0.weight") in self.sd:
                    xs.append(self._conv(ys[i], q + ".0", q + ".1"))
                else:
                    xs.append(ys[i])
            else:
                y = ys[-1]
                for k in range(i + 1 - len(ys)):
                    y = self._conv(y, "%s.%d.0" % (q, k), "%s.%d.1" % (q, k), stride=2)
                xs.append(y)
        return xs

    def _module(self, xs, p, num_blocks, last):
        nb = len(xs)
        xs = list(xs)
        n_out = 1 if last else nb
        # Exchange-unit output i >= 2 sums stride-2 convs of tensors that all live at resolution level i - 1: the
        # intermediates of the chains from branches j < i - 1 and the output of branch i - 1 itself (pose_hrnet.py:
        # 236-255).  Side by side in ONE tensor they are one conv over the concatenated channels (weights side by side,
        # biases added, one fp32 accumulation): cat[i] = (tensor, channel offset of branch i - 1's output in it); the
        # branch's last conv2 and the chains' last intermediates write their slices.  (UDP_POSE_NO_FUSE_CONCAT=1: one
        # conv per term, for A/B)
        cat = {}
        if (self.block_major and len(set(num_blocks[:nb])) == 1 and os.environ.get("UDP_POSE_NO_FUSE_CONCAT") is None):
            for i in range(2, n_out):
                lead = sum(xs[j].c for j in range(i - 1))
                if (lead + xs[i - 1].c) % 8 == 0 and lead % 8 == 0:          # 16-byte aligned slices in both planes
                    cat[i] = (self._new(lead + xs[i - 1].c, xs[i - 1].h, xs[i - 1].w), lead)
        if self.block_major and len(set(num_blocks[:nb])) == 1:
            # block-major order: conv1 of block k of every branch, then conv2 of every branch.  The convs of
            # one such row are independent; those the executor can merge carry a common group id
            for k in range(num_blocks[0]):
                qs = ["%s.branches.%d.%d" % (p, b, k) for b in range(nb)]
                plain = [b for b in range(nb) if not self._can_fuse_block(xs[b], qs[b])
                         and (qs[b] + ".deattn.conv_q_right.weight") not in self.sd]
                gid = (self._next_group(), self._next_group()) if self.group_convs and len(plain) > 1 else (0, 0)
                mids = {}
                order = list(reversed(plain)) if os.environ.get("UDP_POSE_GROUP_FWD") is None else plain
                for b in order:            # deepest-K members first: their workgroups run longest
                    mids[b] = self._conv(xs[b], qs[b] + ".conv1", qs[b] + ".bn1", group=gid[0])
                final = k == num_blocks[0] - 1
                for b in order:
                    dst = cat.get(b + 1) if final else None
                    y = self._conv(mids[b], qs[b] + ".conv2", qs[b] + ".bn2", res=xs[b], group=gid[1], into=dst)
                    xs[b] = _V(dst[0], dst[1], xs[b].c) if dst else y
                for b in range(nb):
                    if b not in plain:
                        xs[b] = self._basic_block(xs[b], qs[b])
                        if final:
                            cat.pop(b + 1, None)        # no slice writer for this branch: one conv per term
        else:
            for b in range(nb):
                for k in range(num_blocks[b]):
                    xs[b] = self._basic_block(xs[b], "%s.branches.%d.%d" % (p, b, k))
        outs = []
        # the 1x1 convs of all j > i terms only read the branch outputs: emitted first, in launch groups of <= 4
        pairs = [(i, j) for i in range(n_out) for j in range(i + 1, nb)]
        if os.environ.get("UDP_POSE_GROUP_FWD") is None:
            pairs.sort(key=lambda ij: (-ij[1], ij[0]))          # deepest-K (lowest-resolution source) first
        up_terms = {i: [] for i in range(n_out)}
        for c0 in range(0, len(pairs), 4):
            chunk = pairs[c0:c0 + 4]
            gid = self._next_group() if self.group_convs and len(chunk) > 1 else 0
            for i, j in chunk:
                q = "%s.fuse_layers.%d.%d" % (p, i, j)
                up_terms[i].append((self._conv(xs[j], q + ".0", q + ".1", relu=False, group=gid), j - i))
        for i in range(n_out):
            ups = up_terms[i]
            if i == 0:
                if last:
                    outs.append(self._conv(xs[0], "%s.fuse_layers.0.0.0" % p, None, ups=ups))
                else:
                    out = self._new(xs[0].c, xs[0].h, xs[0].w)
                    self._emit(_lib.UDP_OP_FUSE, p + ".fuse0", xs[0], out, relu=1, ups=ups)
                    outs.append(out)
                continue
            if i in cat:
                ct, _ = cat[i]
                off = 0
                for j in range(i - 1):                  # the chains: their last intermediate lands in its slice of ct
                    t = xs[j]
                    for k in range(i - j - 1):
                        q = "%s.fuse_layers.%d.%d.%d" % (p, i, j, k)
                        t = self._conv(t, q + ".0", q + ".1", stride=2, into=(ct, off) if k == i - j - 2 else None)
                    off += xs[j].c
                names = ["%s.fuse_layers.%d.%d.%d" % (p, i, j, i - j - 1) for j in range(i)]
                outs.append(self._conv(ct, names[0] + ".0", names[0] + ".1", stride=2, relu=True, res=xs[i], ups=ups,
                                       plus=[(n + ".0", n + ".1") for n in names[1:]]))
                continue
            res, t = xs[i], None
            for j in range(i):
                t = xs[j]
                for k in range(i - j):
                    q = "%s.fuse_layers.%d.%d.%d" % (p, i, j, k)
                    if k != i - j - 1:
                        t = self._conv(t, q + ".0", q + ".1", stride=2)
                    else:
                        t = self._conv(t, q + ".0", q + ".1", stride=2, relu=(j == i - 1), res=res, ups=ups)
                        res, ups = t, []
            outs.append(t)
        return outs
