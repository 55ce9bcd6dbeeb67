"""Host compiler for pose_shufflenetv2_10x_pixel_shuffle (deep_hrnet/lib/models/pose_shufflenetv2_10x_pixel_shuffle.py:23-53)
-> the fused op program.

Graph restated from the reference: 3x3 s2 conv + BN + ReLU and a 3x3 s2 max-pool (backbones/shufflenetv2.py:118-124),
16 ShuffleV2 units in three stages (:34-92, :126-139), a 1x1 ``conv_last`` + BN + ReLU (:143-147), the decoder's linear
1x1 ``conv_compress`` and three DUC blocks = 3x3 conv + BN + ReLU + PixelShuffle(2) (decoders/pixelshuffle.py:15-31,
DUC.py:15-28), and the biased ``final_layer`` writing the NCHW fp32 heat-maps.

Channel layout.  A unit's output is cat(first, second) (:80, :84).  It is stored as two halves of r = oup / 2 real
channels, each zero-padded to cp = a multiple of 32: logical channel j sits at j (j < r) or cp + j - r.  Pad channels
are exact zeros from every producer (zero weights, zero bias).  The channel shuffle (:86-92) never moves a tensor:

* stride-1 unit, 3 launches: ``pw1`` reads the whole padded input through an ``in_map`` that picks the odd logical
  channels; the depthwise launch also copies the even ones (x_proj) into the first half of the unit's output
  (UDP_OP_DWCONV passthrough); ``pw2`` writes the second half.
* stride-2 unit, 4 launches: both depthwise convs write halves of one tensor, and ONE 1x1 conv over it with the
  block-diagonal weight [branch_proj.2 0; 0 branch_main.5] produces the whole unit output (the zero blocks add exact
  zeros; ReLU is per channel).  The first stride-2 unit's output is cat(24, 92) channels in the reference: the
  merged conv's ``out_map`` scatters them to the same two-halves layout.
"""
import os

import torch

from . import _lib
from .program import BN_EPS, Program, _round_up
from .resnet_plan import _Tracked, _get, _head_spec
from .synth_shufflenet import DECODER_INPLANES, STAGE_OUT_CHANNELS, shufflenet_units


def shufflenet_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_shufflenetv2_10x_pixel_shuffle YAML -> dict(model_size, architecture, start_channels,
    final_kernel, out_channels).  Raises NotImplementedError for what cannot run."""
    size = str(_get(extra, "MODEL_SIZE", "1.0x"))
    if size == "2.0x":
        raise NotImplementedError("pose_shufflenetv2_10x_pixel_shuffle MODEL_SIZE='2.0x': the reference itself cannot run it -- "
                                  "conv_last has 2048 channels but the decoder is built for %d "
                                  "(pose_shufflenetv2_10x_pixel_shuffle.py:26)" % DECODER_INPLANES)
    if size not in STAGE_OUT_CHANNELS:
        raise NotImplementedError("pose_shufflenetv2_10x_pixel_shuffle MODEL_SIZE=%r (one of '0.5x', '1.0x', '1.5x')" % size)
    arch = tuple(int(a) for a in _get(extra, "ARCHITECTURE", (512, 256, 128)))
    if len(arch) != 3 or any(a <= 0 or a % 128 for a in arch):
        raise NotImplementedError("pose_shufflenetv2_10x_pixel_shuffle ARCHITECTURE=%s: three DUC blocks (heat-maps at 1/4 of "
                                  "the input) with multiples of 128 channels are supported" % (arch,))
    start = int(_get(extra, "START_CHANNELS", 256))
    if start <= 0 or start % 32:
        raise NotImplementedError("pose_shufflenetv2_10x_pixel_shuffle START_CHANNELS=%d (a multiple of 32)" % start)
    final_kernel = int(_get(extra, "FINAL_CONV_KERNEL", 1))
    if final_kernel not in (1, 3):
        raise NotImplementedError("pose_shufflenetv2_10x_pixel_shuffle FINAL_CONV_KERNEL=%d (1 or 3)" % final_kernel)
    return dict(model_size=size, architecture=arch, start_channels=start, final_kernel=final_kernel,
                out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


def shufflenet_deconv_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_shufflenetv2_10x YAML (the deconv-head sibling, pose_shufflenetv2_10x.py:22-97) ->
    dict(model_size, deconv_filters, final_kernel, deconv_with_bias, out_channels).  The MODEL_SIZE refusals of the
    pixel-shuffle net (the head is built for 1024 channels here too, :25) and the head refusals of ``_head_spec``."""
    size = str(_get(extra, "MODEL_SIZE", "1.0x"))
    if size == "2.0x":
        raise NotImplementedError("pose_shufflenetv2_10x MODEL_SIZE='2.0x': the reference itself cannot run it -- conv_last has "
                                  "2048 channels but the deconv head is built for %d (pose_shufflenetv2_10x.py:25)" % DECODER_INPLANES)
    if size not in STAGE_OUT_CHANNELS:
        raise NotImplementedError("pose_shufflenetv2_10x MODEL_SIZE=%r (one of '0.5x', '1.0x', '1.5x')" % size)
    return dict(_head_spec(extra, "pose_shufflenetv2_10x"), model_size=size,
                out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


def _halves(r):
    """Positions of the 2r logical channels of a unit tensor: (positions, cp)."""
    cp = _round_up(r, 32)
    return [j if j < r else cp + j - r for j in range(2 * r)], cp


class ShuffleNetV2Program(Program):
    NAME = "pose_shufflenetv2"
    DW_KERNELS = (3,)

    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        if dtype not in ("f32", "f16x2"):
            raise ValueError("pose_shufflenetv2_10x_pixel_shuffle: dtype %r; supported storage modes are 'f32' and 'f16x2' "
                             "(the depthwise kernel has no bf16 form)" % (dtype,))
        self.spec = spec
        super().__init__(state_dict, in_h, in_w, dtype)

    @property
    def consumed_keys(self):
        return set(self.sd.used)

    # ------------------------------------------------------------------ op helpers
    def _pw(self, name, x, w, b, relu, in_map=None, cin_t=None, out_map=None, cout_t=None, in_view=None, into=None,
            to_output=False, res=None, res_view=None):
        """One dense conv (1x1 / 3x3, stride 1) from an already folded weight, with the channel maps of ``_pack``.
        ``in_view = cin``: read the first ``cin`` channels of a wider ``x``; ``into = (tensor, coff)``; ``res``: a tensor
        of the output's shape added in the epilogue (the MobileViTv2 planner's residuals); ``res_view = (tensor, coff)``:
        the residual is the output's width of channels from ``coff`` of a wider tensor (the MobileViT planner's shortcut
        from the stem)."""
        ks = int(w.shape[2])
        head_ws = to_output and os.environ.get("UDP_POSE_HEAD_WS", "1") != "0"
        ws = self.use_ws and (not to_output or head_ws)
        w_off, b_off, cout, cin, ks, cout_pad, wexp = self._pack(w, b, ws, out_map=out_map, in_map=in_map, cout_t=cout_t, cin_t=cin_t)
        views = {}
        if in_view is not None:
            if cin != in_view or in_view > x.c:
                raise ValueError("%s: a view of %d channels for a weight of %d" % (name, in_view, cin))
            views.update(in_coff=0, in_pitch=x.c)
        elif cin != x.c:
            raise ValueError("%s: weight expects %d input channels, tensor has %d" % (name, cin, x.c))
        out = None if to_output else (into[0] if into else self._new(cout, x.h, x.w))
        if into:
            if (out.h, out.w) != (x.h, x.w) or into[1] + cout > out.c:
                raise ValueError("%s: output slice does not fit its tensor" % name)
            views.update(out_coff=into[1], out_pitch=out.c)
        if res is not None:
            if (res.c, res.h, res.w) != (cout, x.h, x.w):
                raise ValueError("%s: residual does not match the output" % name)
            views.update(res=res)
        if res_view is not None:
            rt, rc = res_view
            if res is not None or (rt.h, rt.w) != (x.h, x.w) or rc + cout > rt.c:
                raise ValueError("%s: residual view does not match the output" % name)
            views.update(res=rt, res_coff=rc, res_pitch=rt.c, res_c=cout)
        self._emit(_lib.UDP_OP_CONV, name, x, out, ks=ks, stride=1, relu=relu, cin=cin, cout=cout, cout_pad=cout_pad,
                   hout=x.h, wout=x.w, w_off=w_off, b_off=b_off, wfmt=int(ws), wexp=wexp, **views)
        return out

    def _dw(self, conv, bn, x, cin, pos, stride, into=None, passthrough=None, act=0, eps=BN_EPS):
        """Depthwise k x k conv (k = 3, or 5 / 7 in the ShuffleNetV2+ planner) + BatchNorm on the first ``cin`` stored
        channels of ``x``; ``pos[j]``: where logical channel j of the [C,1,k,k] weight sits.  ``into = (tensor, coff)``; ``passthrough = (src, dst, r)``: the
        x_proj copy of a stride-1 unit (include/udp_pose_hip.h, UDP_OP_DWCONV); ``act``: the activation code; ``eps``: the BatchNorm's."""
        w, b = self._fold(conv, bn, eps=eps)
        ks = int(w.shape[2])
        if tuple(w.shape[1:]) != (1, ks, ks) or ks not in self.DW_KERNELS or w.shape[0] != len(pos):
            raise ValueError("%s.weight must be [%d,1,k,k], k one of %s" % (conv, len(pos), self.DW_KERNELS))
        idx = torch.tensor(pos)
        wp = torch.zeros(ks * ks, cin, dtype=torch.float32)
        wp[:, idx] = w.reshape(len(pos), ks * ks).t()
        bp = torch.zeros(cin, dtype=torch.float32)
        bp[idx] = b
        ho, wo = (x.h - 1) // stride + 1, (x.w - 1) // stride + 1
        out = into[0] if into else self._new(cin, ho, wo)
        views = {}
        if cin != x.c:
            views.update(in_coff=0, in_pitch=x.c)
        if into:
            views.update(out_coff=into[1], out_pitch=out.c)
        if passthrough:
            src, dst, r = passthrough
            # field reuse of kind 12 (include/udp_pose_hip.h): the source is ``res``; ``add2`` only mirrors it so that
            # ops_array() can zip it with ``out2`` and _reads() sees the dependency -- the kernel never reads add2;
            # ``chain_cout`` carries r, no chained conv
            views.update(res=src, res_coff=0, res_pitch=src.c, res_c=src.c, out2=[(dst, 0)], add2=[(src, 0)], chain_cout=r)
        self._emit(_lib.UDP_OP_DWCONV, conv, x, out, ks=ks, stride=stride, relu=act, cin=cin, cout=cin, cout_pad=cin, hout=ho, wout=wo,
                   w_off=self._put(wp.numpy().tobytes()), b_off=self._put(bp.numpy().tobytes()), **views)
        return out

    def _ps_head(self, x, c=None):
        """The pixel-shuffle head every ``*_pixel_shuffle`` net of the reference shares (decoders/pixelshuffle.py:15-31,
        DUC.py:15-28): the linear 1x1 ``conv_compress`` on the ``c`` real channels of ``x`` (default: all it stores),
        three DUC blocks = 3x3 conv + BN + ReLU + PixelShuffle(2), and the biased ``final_layer`` writing the NCHW fp32
        heat-maps.  Sets ``out_channels``."""
        w, b = self._fold("decoder.conv_compress")                      # linear: no BatchNorm, no activation (pixelshuffle.py:15-16)
        c = x.c if c is None else c
        if int(w.shape[1]) != c:
            raise ValueError("decoder.conv_compress expects %d input channels, the backbone ends with %d" % (int(w.shape[1]), c))
        x = self._pw("decoder.conv_compress", x, w, b, False, cin_t=x.c)
        for d, planes in enumerate(self.spec["architecture"]):          # DUC.py:23-28
            q = "decoder.duc.%d" % d
            w, b = self._fold(q + ".conv", q + ".bn")
            cq = planes // 4
            # PixelShuffle reads channel 4c + g for sub-pixel g = 2i + j: store it at g * cq + c (UDP_OP_PIXSHUF)
            t = self._pw(q + ".conv", x, w, b, True, out_map=[(o % 4) * cq + o // 4 for o in range(planes)])
            x = self._new(cq, 2 * t.h, 2 * t.w)
            self._emit(_lib.UDP_OP_PIXSHUF, q + ".pixel_shuffle", t, x, ks=1, stride=1)
        if (x.h, x.w) != (self.in_h // 4, self.in_w // 4):
            raise ValueError("%s: heat-maps at %dx%d, expected %dx%d" % (self.NAME, x.h, x.w, self.in_h // 4, self.in_w // 4))
        w, b = self._fold("final_layer")
        self._pw("final_layer", x, w, b, False, to_output=True)
        self.out_channels = self._ops[-1]["cout"]

    def _head(self, x):
        """Behind the backbone: the deconv head when the spec carries ``deconv_filters`` (the nets without
        ``_pixel_shuffle`` in their name), the pixel-shuffle head otherwise."""
        if "deconv_filters" in self.spec:
            self._deconv_head(x, self.NAME, len(self.spec["deconv_filters"]))
        else:
            self._ps_head(x)

    # ------------------------------------------------------------------ the net
    def _build(self):
        self.sd = _Tracked(self.sd)
        self._head(self._backbone())
        self._mark_unused()

    def _backbone(self):
        """Stem to ``conv_last``: returns its output tensor."""
        sd, spec = self.sd, self.spec
        H, W = self.in_h, self.in_w
        # stem: the kernel computes 64 output channels; the real ones first, zero weights and bias behind them
        w, b = self._fold("backbone.first_conv.0", "backbone.first_conv.1")
        c0 = int(w.shape[0])
        if tuple(w.shape[1:]) != (3, 3, 3) or c0 > 64:
            raise ValueError("backbone.first_conv.0.weight must be [<=64,3,3,3]")
        wp = torch.zeros(64, 3, 3, 3)
        wp[:c0] = w
        bp = torch.zeros(64)
        bp[:c0] = b
        x = self._new(64, H // 2, W // 2)
        self._emit(_lib.UDP_OP_STEM, "backbone.first_conv.0", None, x, ks=3, stride=2, relu=1,
                   w_off=self._put(wp.permute(2, 3, 1, 0).contiguous().numpy().tobytes()), b_off=self._put(bp.numpy().tobytes()))
        pooled = self._new(64, H // 4, W // 4)
        self._emit(_lib.UDP_OP_MAXPOOL, "backbone.maxpool", x, pooled, ks=3, stride=2)
        x, pos = pooled, list(range(c0))
        for idx, inp, oup, mid, stride in shufflenet_units(spec["model_size"]):
            p = "backbone.features.%d" % idx
            r = oup // 2
            npos, cp = _halves(r)
            if stride == 2:
                xc = _round_up(max(pos) + 1, 32)             # stored channels the unit reads (all of x but for the pooled stem)
                mp = _round_up(mid, 32)
                ho, wo = (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1
                t = self._new(xc + mp, ho, wo)               # [dw_proj | dw]: the input of the merged pw conv
                self._dw(p + ".branch_proj.0", p + ".branch_proj.1", x, xc, pos, 2, into=(t, 0))
                w1, b1 = self._fold(p + ".branch_main.0", p + ".branch_main.1")
                a = self._pw(p + ".branch_main.0", x, w1, b1, True, in_map=pos, cin_t=xc, cout_t=mp, in_view=xc if xc != x.c else None)
                self._dw(p + ".branch_main.3", p + ".branch_main.4", a, mp, list(range(mid)), 2, into=(t, xc))
                wa, ba = self._fold(p + ".branch_proj.2", p + ".branch_proj.3")        # [inp, inp]
                wb, bb = self._fold(p + ".branch_main.5", p + ".branch_main.6")        # [oup - inp, mid]
                wm = torch.zeros(oup, inp + mid, 1, 1)
                wm[:inp, :inp] = wa
                wm[inp:, inp:] = wb
                x = self._pw(p + ".branch_proj.2+branch_main.5", t, wm, torch.cat([ba, bb]), True,
                             in_map=pos + [xc + m for m in range(mid)], cin_t=t.c, out_map=npos, cout_t=2 * cp)
            else:
                if pos != npos or x.c != 2 * cp or inp != r or mid != r:
                    raise ValueError("%s: a stride-1 unit keeps its channel count" % p)
                w1, b1 = self._fold(p + ".branch_main.0", p + ".branch_main.1")
                a = self._pw(p + ".branch_main.0", x, w1, b1, True, in_map=[pos[2 * k + 1] for k in range(r)], cin_t=2 * cp, cout_t=cp)
                y = self._new(2 * cp, x.h, x.w)
                d = self._dw(p + ".branch_main.3", p + ".branch_main.4", a, cp, list(range(r)), 1, passthrough=(x, y, r))
                w2, b2 = self._fold(p + ".branch_main.5", p + ".branch_main.6")
                self._pw(p + ".branch_main.5", d, w2, b2, True, cin_t=cp, cout_t=cp, into=(y, cp))
                x = y
            pos = npos
        w, b = self._fold("backbone.conv_last.0", "backbone.conv_last.1")
        return self._pw("backbone.conv_last.0", x, w, b, True, in_map=pos, cin_t=x.c)

    def _mark_unused(self):
        for k in self.sd:
            if k.endswith("num_batches_tracked") or k == "backbone.classifier.0.weight":
                self.sd.used.add(k)              # BatchNorm bookkeeping / the ImageNet classifier forward() never applies (:160-165)

    def macs_per_image(self):
        return super().macs_per_image() + sum(op["ks"] ** 2 * op["cout"] * op["hout"] * op["wout"] for op in self._ops
                                              if op["kind"] == _lib.UDP_OP_DWCONV)
