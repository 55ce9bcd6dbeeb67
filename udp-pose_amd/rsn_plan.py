"""Host compiler for RSN-18 (RSN/exps/RSN18.coco/network.py) -> the same fused op program.

Graph restated from the reference: ResNet_top :125-137 (7x7 s2 conv+BN+ReLU, 3x3 s2 max-pool),
four levels of two RSN Bottlenecks :49-122, top-down Upsample_units :202-255 (only what
``outputs[-1][-1]`` needs: u_skip, bilinear align-corners up + up_conv, res_conv1/2 of the finest
level), single stage.

RSN's bottleneck splits a 1x1 conv's output into four groups of ``in_planes*26//64`` channels and
concatenates four branch outputs (:102-114).  Here both are **views**: each group is padded to a
multiple of 16 channels (26 -> 32, 52 -> 64, 104 -> 112, 208), the 1x1 conv's weight rows / the
closing 1x1 conv's weight columns are scattered to the padded positions with zeros in between, the
3x3 convs read / write channel slices in place, and the pad channels stay exactly 0 (zero weights,
zero bias, ReLU).  The ``a + b`` that precedes most 3x3 convs is one element-wise launch.

``se`` / ``prm``: the two additions of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py.  ``se``: conv_bn_relu3 runs without residual and ReLU, and one UDP_OP_SE_RES launch follows in place with
the shortcut as ``res`` and the ReLU on (:51-66, :135-143) -- 16 launches.  ``prm``: behind up4's ReLU the Pose Refine
Machine (:267-301, :357-358) as 3x3 conv, UDP_OP_PRM_GATE, 1x1 conv, UDP_OP_PRM_DW9 -- 4 launches; res_conv1 reads the
result.  Both need f32 / f16x2 storage.

``stem``: ``"pool"`` is the ResNet_top above; ``"conv7"`` is that experiment's own ResNet_top (:188-203) -- UDP_OP_STEM
for ``top.conv.0`` (3x3 s2, 3 -> 64, from the NCHW input, mirrored half included), the 7x7 stride-1 64 -> 64 conv
``top.conv.1`` at half resolution (UDP_OP_CONV with ks = 7, csrc/conv7.hip), the 3x3 s2 conv ``top.conv.2``, no max-pool:
3 launches instead of 2, 2.5 GMAC per 256x192 image more.  It goes with or without se / prm and needs f32 / f16x2
storage as well (the 7x7 conv has no bf16 form); with se + prm the program takes the experiment's own checkpoints.
"""
import os

import torch

from . import _lib
from .program import Program, _round_up, storage_bytes


class RSNProgram(Program):
    def __init__(self, state_dict, in_h, in_w, dtype="f32", chl_num=256, se=False, prm=False, stem="pool"):
        self.chl_num = chl_num
        self.se, self.prm = bool(se), bool(prm)
        if stem not in ("pool", "conv7"):
            raise ValueError("RSN-18 stem must be 'pool' or 'conv7' (got %r)" % (stem,))
        self.stem = stem
        if (self.se or self.prm) and dtype not in ("f32", "f16x2"):
            raise ValueError("RSN-18 with se / prm: storage modes 'f32' and 'f16x2' only (got %r)" % (dtype,))
        if stem == "conv7" and dtype not in ("f32", "f16x2"):
            raise ValueError("RSN-18 with the conv7 stem: storage modes 'f32' and 'f16x2' only (got %r)" % (dtype,))
        super().__init__(state_dict, in_h, in_w, dtype)

    def _fold_cbr(self, name):
        """conv_bn_relu module ``name`` (conv with bias + BatchNorm) -> folded fp32 weight [cout,cin,k,k], bias [cout]."""
        return self._fold(name + ".conv", name + ".bn")

    def _op(self, kind, x, out, name, res=None, **fields):
        """An op over channel-slice views: every operand carries its tensor's channel count as pitch."""
        self._emit(kind, name, x, out, res=res, in_pitch=x.c, out_pitch=out.c if out is not None else 0,
                   res_pitch=res.c if res is not None else 0, **fields)

    def _conv_v(self, x, name, out=None, ks=None, stride=1, relu=True, res=None, in_coff=0, cin_view=None,
                out_coff=0, out_map=None, in_map=None, cout_t=None, cin_t=None, to_output=False, sums=(), keep=True):
        """``sums``: [(tensor, channel offset)] addends -- for each one the conv also writes (its stored output + that
        slice) into a new tensor (udp_conv_op.n_out2) and returns ``(out, [sum tensors])``; ``keep=False``: nothing reads
        the plain output, only the sums are stored."""
        w, b = self._fold_cbr(name)
        # split-fp16 3x3 / 1x1 convs on the weight-stationary kernels (UDP_POSE_RSN_WS=0: the LDS-staged kernel, A/B)
        # (the 3x3 head conv writes the NCHW fp32 output from the weight-stationary kernel too; UDP_POSE_HEAD_WS=0: LDS-staged)
        head_ws = to_output and stride == 1 and os.environ.get("UDP_POSE_HEAD_WS", "1") != "0"
        ws = (self.use_ws and (not to_output or head_ws) and int(w.shape[2]) in (1, 3) and stride in (1, 2)
              and os.environ.get("UDP_POSE_RSN_WS", "1") != "0")
        w_off, b_off, cout, cin, k, cout_pad, wexp = self._pack(w, b, ws, out_map, in_map, cout_t, cin_t)
        if cin_view is not None and cin_view != cin:
            raise ValueError("%s: view has %d channels, weights expect %d" % (name, cin_view, cin))
        pad = k // 2
        ho = (x.h + 2 * pad - k) // stride + 1
        wo = (x.w + 2 * pad - k) // stride + 1
        if sums and not ws:
            raise ValueError("%s: second outputs need the weight-stationary split-fp16 conv" % name)
        if out is None and not to_output and keep:
            out = self._new(cout, ho, wo)
        s2 = [self._new(cout, ho, wo) for _ in sums]
        self._op(_lib.UDP_OP_CONV, x, out, name, ks=k, stride=stride, relu=relu, cin=cin, cout=cout, cout_pad=cout_pad,
                 res=res, w_off=w_off, b_off=b_off, in_coff=in_coff, out_coff=out_coff, hout=ho, wout=wo,
                 wfmt=int(ws), wexp=wexp, out2=[(t, 0) for t in s2], add2=list(sums), no_out=not keep)
        return (out, s2) if sums else out

    def _add(self, a, a_coff, b, b_coff, c, name):
        """out[c channels] = a[a_coff:a_coff+c] + b[b_coff:b_coff+c] (no activation)."""
        out = self._new(c, a.h, a.w)
        self._op(_lib.UDP_OP_FUSE, a, out, name, cin=c, cout=c, res=b, in_coff=a_coff, res_coff=b_coff)
        return out

    def _bottleneck(self, x, p, planes, stride):
        sd = self.sd
        in_planes = sd[p + ".conv_bn_relu1.conv.weight"].shape[1]
        bch = sd[p + ".conv_bn_relu1.conv.weight"].shape[0] // 4
        bp = _round_up(bch, 16)
        scatter = [k * bp + j for k in range(4) for j in range(bch)]       # real channel -> padded position
        if in_planes != x.c:
            raise ValueError("%s expects %d input channels, got %d" % (p, in_planes, x.c))
        s = self._conv_v(x, p + ".conv_bn_relu1", stride=stride, out_map=scatter, cout_t=4 * bp)
        cat = self._new(4 * bp, s.h, s.w)
        pad_in = list(range(bch))

        def c3(src, src_coff, name, out=None, out_coff=0, sums=(), keep=True):
            return self._conv_v(src, p + ".conv_bn_relu" + name, out=out, in_coff=src_coff, out_coff=out_coff,
                                out_map=pad_in, in_map=pad_in, cout_t=bp, cin_t=bp, sums=sums, keep=keep)

        if self.use_ws and os.environ.get("UDP_POSE_RSN_WS", "1") != "0" and os.environ.get("UDP_POSE_RSN_FUSE_ADDS", "1") != "0":
            # split-fp16: the six element-wise sums between the 3x3 convs (network.py:102-114) ride in the epilogue of the
            # conv that produces their second operand (second outputs, udp_conv_op.n_out2) instead of being launches of
            # their own -- 48 launches and a third of their traffic per forward; same numbers as the separate sums
            _, (t21,) = c3(s, 0, "2_1_1", out=cat, out_coff=0, sums=[(s, bp)])           # cat[0]; + spx[1]
            o21, (t31,) = c3(t21, 0, "2_2_1", sums=[(s, 2 * bp)])                        # out_2_1; + spx[2]
            c3(o21, 0, "2_2_2", out=cat, out_coff=bp)                                    # out_2_2 -> cat[1]
            _, (t32, t41) = c3(t31, 0, "2_3_1", sums=[(cat, bp), (s, 3 * bp)], keep=False)   # out_3_1 (+ cat[1]; + spx[3])
            o32 = c3(t32, 0, "2_3_2")                                                    # out_3_2
            c3(o32, 0, "2_3_3", out=cat, out_coff=2 * bp)                                # out_3_3 -> cat[2]
            _, (t42,) = c3(t41, 0, "2_4_1", sums=[(o32, 0)], keep=False)                 # out_4_1 + out_3_2
            _, (t43,) = c3(t42, 0, "2_4_2", sums=[(cat, 2 * bp)], keep=False)            # out_4_2 + cat[2]
            o43 = c3(t43, 0, "2_4_3")
            c3(o43, 0, "2_4_4", out=cat, out_coff=3 * bp)                                # out_4_4 -> cat[3]
        else:
            c3(s, 0, "2_1_1", out=cat, out_coff=0)                                   # out_1_1 -> cat[0]
            o21 = c3(self._add(s, bp, cat, 0, bp, p + ".add21"), 0, "2_2_1")
            c3(o21, 0, "2_2_2", out=cat, out_coff=bp)                                # out_2_2 -> cat[1]
            o31 = c3(self._add(s, 2 * bp, o21, 0, bp, p + ".add31"), 0, "2_3_1")
            o32 = c3(self._add(o31, 0, cat, bp, bp, p + ".add32"), 0, "2_3_2")
            c3(o32, 0, "2_3_3", out=cat, out_coff=2 * bp)                            # out_3_3 -> cat[2]
            o41 = c3(self._add(s, 3 * bp, o31, 0, bp, p + ".add41"), 0, "2_4_1")
            o42 = c3(self._add(o41, 0, o32, 0, bp, p + ".add42"), 0, "2_4_2")
            o43 = c3(self._add(o42, 0, cat, 2 * bp, bp, p + ".add43"), 0, "2_4_3")
            c3(o43, 0, "2_4_4", out=cat, out_coff=3 * bp)                            # out_4_4 -> cat[3]
        r = x
        if (p + ".downsample.conv.weight") in sd:
            r = self._conv_v(x, p + ".downsample", stride=stride, relu=False)
        if not self.se:
            return self._conv_v(cat, p + ".conv_bn_relu3", res=r, in_map=scatter, cin_t=4 * bp)
        out = self._conv_v(cat, p + ".conv_bn_relu3", relu=False, in_map=scatter, cin_t=4 * bp)
        return self._se_res(out, p + ".se", r)

    def _f32(self, key, shape):
        if key not in self.sd:
            raise ValueError("state_dict has no %s" % key)
        t = self.sd[key].detach().to(torch.float32).cpu()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s must be %s, got %s" % (key, list(shape), list(t.shape)))
        return t

    def _se_res(self, x, p, res):
        """SELayer ``p`` (reduction 8, no biases) on ``x`` in place, then + ``res`` and ReLU: one UDP_OP_SE_RES launch."""
        c, ch = x.c, x.c // 8
        w1, w2 = self._f32(p + ".fc.0.weight", (ch, c)), self._f32(p + ".fc.2.weight", (c, ch))
        w_off = self._put(torch.cat([w1.t().reshape(-1), w2.t().reshape(-1)]).contiguous().numpy().tobytes())
        self._op(_lib.UDP_OP_SE_RES, x, x, p, res=res, relu=1, cin=c, cout=c, cout_pad=c, chain_cout=ch, w_off=w_off)
        return x

    def _prm(self, x, p):
        """PRM.forward (network.py:290-301) on ``x`` -> a new tensor."""
        c = x.c
        out1 = self._conv_v(x, p + ".conv_bn_relu_prm_1")
        blk = []
        for nm in ("2_1", "2_2"):
            w, b = self._fold_cbr(p + ".conv_bn_relu_prm_" + nm)
            if tuple(w.shape) != (c, c, 1, 1):
                raise ValueError("%s.conv_bn_relu_prm_%s.conv.weight must be [%d, %d, 1, 1]" % (p, nm, c, c))
            blk += [w.reshape(c, c).t().reshape(-1), b]
        rows = self._new(c * (4 // storage_bytes(self.dtype)), 1, 1)          # an fp32 row a[C] per image
        self._emit(_lib.UDP_OP_PRM_GATE, p + ".gate", out1, rows, cin=c, cout=c, cout_pad=c, hout=out1.h, wout=out1.w,
                   w_off=self._put(torch.cat(blk).contiguous().numpy().tobytes()))
        t = self._conv_v(out1, p + ".conv_bn_relu_prm_3_1")
        w, b = self._fold_cbr(p + ".conv_bn_relu_prm_3_2")
        if tuple(w.shape) != (c, 1, 9, 9):
            raise ValueError("%s.conv_bn_relu_prm_3_2.conv.weight must be [%d, 1, 9, 9]" % (p, c))
        out = self._new(c, x.h, x.w)
        self._op(_lib.UDP_OP_PRM_DW9, t, out, p + ".conv_bn_relu_prm_3_2", res=out1, ks=9, cin=c, cout=c, cout_pad=c, ups=[(rows, 0)],
                 w_off=self._put(w.reshape(c, 81).t().contiguous().numpy().tobytes()), b_off=self._put(b.numpy().tobytes()))
        return out

    def _build(self):
        H, W = self.in_h, self.in_w
        if self.stem == "conv7":
            x = self._stem(_lib.UDP_OP_STEM, "top.conv.0.conv", "top.conv.0.bn", 3, name="top.conv.0")
            if tuple(self.sd["top.conv.1.conv.weight"].shape) != (64, 64, 7, 7) or tuple(self.sd["top.conv.2.conv.weight"].shape) != (64, 64, 3, 3):
                raise ValueError("top.conv.1 / top.conv.2 conv weights must be [64,64,7,7] / [64,64,3,3]")
            x = self._conv_v(x, "top.conv.1")
            x = self._conv_v(x, "top.conv.2", stride=2)
        else:
            x = self._stem(_lib.UDP_OP_STEM7, "top.conv.conv", "top.conv.bn", 7, name="top.conv")
            pooled = self._new(64, H // 4, W // 4)
            self._op(_lib.UDP_OP_MAXPOOL, x, pooled, "top.maxpool", ks=3, stride=2)
            x = pooled
        feats = []
        for layer, planes in zip(range(1, 5), (64, 128, 256, 512)):
            for blk in range(2):
                x = self._bottleneck(x, "stage0.downsample.layer%d.%d" % (layer, blk), planes,
                                     2 if (layer > 1 and blk == 0) else 1)
            feats.append(x)
        up = None
        out = None
        for ind, xin in enumerate(reversed(feats)):                       # x4, x3, x2, x1
            p = "stage0.upsample.up%d" % (ind + 1)
            if ind == 0:
                out = self._conv_v(xin, p + ".u_skip", relu=True)            # relu(u_skip(x)), no addend
            else:
                big = self._new(up.c, xin.h, xin.w)
                self._op(_lib.UDP_OP_BILINEAR, up, big, p + ".bilinear")
                t = self._conv_v(big, p + ".up_conv", relu=False)
                out = self._conv_v(xin, p + ".u_skip", relu=True, res=t)     # relu(u_skip(x) + up_conv(up))
            up = out
        if self.prm:
            out = self._prm(out, "stage0.upsample.up4.prm")
        r1 = self._conv_v(out, "stage0.upsample.up4.res_conv1", relu=True)
        # the closing bilinear resize to OUTPUT_SHAPE (:255) is the identity at the finest level
        if (out.h, out.w) != (H // 4, W // 4):
            raise ValueError("finest RSN level must be at 1/4 resolution")
        self._conv_v(r1, "stage0.upsample.up4.res_conv2", relu=False, to_output=True)
        self.out_channels = self._ops[-1]["cout"]
