"""Host compiler for pose_shufflenetv2_plus_pixel_shuffle
(deep_hrnet/lib/models/pose_shufflenetv2_plus_pixel_shuffle.py:23-55) -> the fused op program.

Graph restated from the reference (backbones/shufflenetv2_plus.py): a 3x3 s2 conv + BN + hard-swish, NO max-pool
(:259-263), 20 units in four stages of [4, 4, 8, 4] (:246, :267-300) picked by the fixed architecture list (:360) --
0 / 1 / 2: ``Shufflenet`` with a 3x3 / 5x5 / 7x7 depthwise conv (:74-141), 3: ``Shuffle_Xception`` (:143-221) --, ReLU in
stage 0 and hard-swish after it (:271), a squeeze-and-excitation layer behind branch_main in stages 2 and 3 (:272,
:34-60), a 1x1 ``conv_last`` + BN + hard-swish (:304-308); then the decoder and head of the ShuffleNetV2 net
(shufflenet_plan.py): ``conv_compress``, three DUC blocks, ``final_layer``.

It shares the two-halves channel layout, the ``in_map`` + passthrough form of the channel shuffle and the block-diagonal
merged 1x1 conv of a stride-2 unit with shufflenet_plan.ShuffleNetV2Program, whose helpers it inherits.  What is new:

* hard-swish is an activation code of the 1x1 convs and the stem (no launch of its own);
* a squeeze-and-excitation layer is ONE launch (UDP_OP_SE), in place on the main half of the unit's output;
* a stride-1 Xception unit is 6 launches: its first depthwise conv runs over the WHOLE stored input with zero weights
  on the even logical channels (``_dw``'s ``pos``), the 1x1 conv behind it picks the odd ones through ``in_map``, and
  the second depthwise conv carries the passthrough.

Launches for the fixed architecture: stem 1 + stage 0 (4 + 3 + 6 + 3 = 16) + stage 1 (4 + 3 + 3 + 3 = 13) + stage 2
(5 + 7 x 4 = 33) + stage 3 (5 + 4 + 7 + 4 = 20) + conv_last 1 + conv_compress 1 + DUC 6 + head 1 = 92.
"""
import torch

from . import _lib
from .program import _round_up
from .resnet_plan import _get, _head_spec
from .shufflenet_plan import ShuffleNetV2Program, _halves
from .synth_shufflenet_plus import DECODER_INPLANES, STAGE_OUT_CHANNELS, shufflenet_plus_units, unused_keys

NAME = "pose_shufflenetv2_plus_pixel_shuffle"


def shufflenet_plus_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_shufflenetv2_plus_pixel_shuffle YAML -> dict(model_size, architecture, start_channels,
    final_kernel, out_channels).  Raises NotImplementedError for what cannot run."""
    size = str(_get(extra, "MODEL_SIZE", "Small"))
    if size not in STAGE_OUT_CHANNELS:
        raise NotImplementedError("%s MODEL_SIZE=%r (one of 'Small', 'Medium', 'Large')" % (NAME, size))
    arch = tuple(int(a) for a in _get(extra, "ARCHITECTURE", (512, 256, 128)))
    if len(arch) != 3 or any(a <= 0 or a % 128 for a in arch):
        raise NotImplementedError("%s ARCHITECTURE=%s: three DUC blocks (heat-maps at 1/4 of the input) with multiples of "
                                  "128 channels are supported" % (NAME, arch))
    start = int(_get(extra, "START_CHANNELS", 256))
    if start <= 0 or start % 32:
        raise NotImplementedError("%s START_CHANNELS=%d (a multiple of 32)" % (NAME, start))
    final_kernel = int(_get(extra, "FINAL_CONV_KERNEL", 1))
    if final_kernel not in (1, 3):
        raise NotImplementedError("%s FINAL_CONV_KERNEL=%d (1 or 3)" % (NAME, final_kernel))
    return dict(model_size=size, architecture=arch, start_channels=start, final_kernel=final_kernel,
                out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


def shufflenet_plus_deconv_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_shufflenetv2_plus YAML (the deconv-head sibling, pose_shufflenetv2_plus.py:22-99) ->
    dict(model_size, deconv_filters, final_kernel, deconv_with_bias, out_channels): the MODEL_SIZE refusal of the
    pixel-shuffle net and the head refusals of ``resnet_plan._head_spec``."""
    size = str(_get(extra, "MODEL_SIZE", "Small"))
    if size not in STAGE_OUT_CHANNELS:
        raise NotImplementedError("pose_shufflenetv2_plus MODEL_SIZE=%r (one of 'Small', 'Medium', 'Large')" % size)
    return dict(_head_spec(extra, "pose_shufflenetv2_plus"), model_size=size,
                out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


class ShuffleNetV2PlusProgram(ShuffleNetV2Program):
    NAME = "pose_shufflenetv2_plus"
    DW_KERNELS = (3, 5, 7)

    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        if dtype not in ("f32", "f16x2"):
            raise ValueError("%s: dtype %r; supported storage modes are 'f32' and 'f16x2' (the depthwise and "
                             "squeeze-excitation kernels have no bf16 form)" % (NAME, dtype))
        super().__init__(state_dict, spec, in_h, in_w, dtype)

    def _se(self, name, t, coff, c, r):
        """SELayer ``name`` on channels [coff, coff + c) of ``t`` (r real ones first), in place: one UDP_OP_SE launch.
        Parameter block (include/udp_pose_hip.h): W1 transposed [c][hidden] with the BatchNorm folded in, b1 [hidden],
        W2 transposed [hidden][c]; zero rows / columns at the pad channels."""
        w1, b1 = self._fold(name + ".SE_opr.1", name + ".SE_opr.2")
        w2, _ = self._fold(name + ".SE_opr.4")
        hid = int(w1.shape[0])
        if tuple(w1.shape) != (hid, r, 1, 1) or tuple(w2.shape) != (r, hid, 1, 1) or hid < 1:
            raise ValueError("%s: squeeze-excitation weights must be [%d,%d,1,1] and [%d,%d,1,1]" % (name, hid, r, r, hid))
        w1t = torch.zeros(c, hid, dtype=torch.float32)
        w1t[:r] = w1.reshape(hid, r).t()
        w2t = torch.zeros(hid, c, dtype=torch.float32)
        w2t[:, :r] = w2.reshape(r, hid).t()
        block = torch.cat([w1t.reshape(-1), b1, w2t.reshape(-1)]).contiguous()
        self._emit(_lib.UDP_OP_SE, name, t, t, cin=c, cout=c, cout_pad=c, in_coff=coff, in_pitch=t.c, out_coff=coff, out_pitch=t.c,
                   chain_cout=hid, w_off=self._put(block.numpy().tobytes()))

    # ------------------------------------------------------------------ the net
    def _backbone(self):
        """Stem to ``conv_last``: returns its output tensor (``_build``, ``_head``: shufflenet_plan.ShuffleNetV2Program)."""
        sd, spec = self.sd, self.spec
        H, W = self.in_h, self.in_w
        HS = _lib.UDP_ACT_HSWISH
        # stem: the kernel computes 64 output channels; the real ones first, zero weights and bias behind them (hswish(0) = 0)
        w, b = self._fold("backbone.first_conv.0", "backbone.first_conv.1")
        c0 = int(w.shape[0])
        if tuple(w.shape[1:]) != (3, 3, 3) or c0 > 64:
            raise ValueError("backbone.first_conv.0.weight must be [<=64,3,3,3]")
        wp = torch.zeros(64, 3, 3, 3)
        wp[:c0] = w
        bp = torch.zeros(64)
        bp[:c0] = b
        x = self._new(64, H // 2, W // 2)
        self._emit(_lib.UDP_OP_STEM, "backbone.first_conv.0", None, x, ks=3, stride=2, relu=HS,
                   w_off=self._put(wp.permute(2, 3, 1, 0).contiguous().numpy().tobytes()), b_off=self._put(bp.numpy().tobytes()))
        pos = list(range(c0))
        for idx, inp, oup, mid, stride, block, act, se in shufflenet_plus_units(spec["model_size"]):
            p = "backbone.features.%d" % idx
            a_code = HS if act == "hs" else _lib.UDP_ACT_RELU
            r = oup // 2
            npos, cp = _halves(r)
            if stride == 2:
                if block == 3:
                    raise NotImplementedError("%s: a stride-2 Shuffle_Xception unit (the reference cannot run one either: all "
                                              "three of its depthwise convs take the stride, shufflenetv2_plus.py:160-174)" % p)
                xc = _round_up(max(pos) + 1, 32)             # stored channels the unit reads (all of x but for the stem's 64)
                mp = _round_up(mid, 32)
                ho, wo = (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1
                t = self._new(xc + mp, ho, wo)               # [dw_proj | dw]: the input of the merged pw conv
                self._dw(p + ".branch_proj.0", p + ".branch_proj.1", x, xc, pos, 2, into=(t, 0))
                w1, b1 = self._fold(p + ".branch_main.0", p + ".branch_main.1")
                a = self._pw(p + ".branch_main.0", x, w1, b1, a_code, in_map=pos, cin_t=xc, cout_t=mp, in_view=xc if xc != x.c else None)
                self._dw(p + ".branch_main.3", p + ".branch_main.4", a, mp, list(range(mid)), 2, into=(t, xc))
                wa, ba = self._fold(p + ".branch_proj.2", p + ".branch_proj.3")        # [inp, inp]
                wb, bb = self._fold(p + ".branch_main.5", p + ".branch_main.6")        # [oup - inp, mid]
                wm = torch.zeros(oup, inp + mid, 1, 1)
                wm[:inp, :inp] = wa
                wm[inp:, inp:] = wb
                y = self._pw(p + ".branch_proj.2+branch_main.5", t, wm, torch.cat([ba, bb]), a_code,
                             in_map=pos + [xc + m for m in range(mid)], cin_t=t.c, out_map=npos, cout_t=2 * cp)
                if se:
                    if oup - inp != r:
                        raise ValueError("%s: squeeze-excitation on a main branch of %d channels beside %d" % (p, oup - inp, inp))
                    self._se(p + ".branch_main.8", y, cp, cp, r)
            else:
                if pos != npos or x.c != 2 * cp or inp != r or mid != r:
                    raise ValueError("%s: a stride-1 unit keeps its channel count" % p)
                odd = [pos[2 * k + 1] for k in range(r)]
                y = self._new(2 * cp, x.h, x.w)
                if block == 3:                               # Shuffle_Xception: 3 x (dw 3x3 + BN, pw + BN + act)
                    d = self._dw(p + ".branch_main.0", p + ".branch_main.1", x, 2 * cp, odd, 1)
                    w1, b1 = self._fold(p + ".branch_main.2", p + ".branch_main.3")
                    a = self._pw(p + ".branch_main.2", d, w1, b1, a_code, in_map=odd, cin_t=2 * cp, cout_t=cp)
                    d = self._dw(p + ".branch_main.5", p + ".branch_main.6", a, cp, list(range(r)), 1, passthrough=(x, y, r))
                    w2, b2 = self._fold(p + ".branch_main.7", p + ".branch_main.8")
                    a = self._pw(p + ".branch_main.7", d, w2, b2, a_code, cin_t=cp, cout_t=cp)
                    d = self._dw(p + ".branch_main.10", p + ".branch_main.11", a, cp, list(range(r)), 1)
                    w3, b3 = self._fold(p + ".branch_main.12", p + ".branch_main.13")
                    self._pw(p + ".branch_main.12", d, w3, b3, a_code, cin_t=cp, cout_t=cp, into=(y, cp))
                    se_name = p + ".branch_main.15"
                else:
                    w1, b1 = self._fold(p + ".branch_main.0", p + ".branch_main.1")
                    a = self._pw(p + ".branch_main.0", x, w1, b1, a_code, in_map=odd, cin_t=2 * cp, cout_t=cp)
                    d = self._dw(p + ".branch_main.3", p + ".branch_main.4", a, cp, list(range(r)), 1, passthrough=(x, y, r))
                    w2, b2 = self._fold(p + ".branch_main.5", p + ".branch_main.6")
                    self._pw(p + ".branch_main.5", d, w2, b2, a_code, cin_t=cp, cout_t=cp, into=(y, cp))
                    se_name = p + ".branch_main.8"
                if se:
                    self._se(se_name, y, cp, cp, r)
            x, pos = y, npos
        w, b = self._fold("backbone.conv_last.0", "backbone.conv_last.1")
        x = self._pw("backbone.conv_last.0", x, w, b, HS, in_map=pos, cin_t=x.c)
        if x.c != DECODER_INPLANES:
            raise ValueError("%s: the head expects %d input channels, conv_last has %d" % (self.NAME, DECODER_INPLANES, x.c))
        return x

    def _mark_unused(self):
        # accepted and unused: BatchNorm bookkeeping and the ImageNet tail forward() never applies (shufflenetv2_plus.py:324-331)
        self.unused_keys = unused_keys(self.sd)
        self.sd.used.update(self.unused_keys)

    def macs_per_image(self):
        # + the two small products of every squeeze-excitation layer (its pool and scale are not counted)
        return super().macs_per_image() + sum(2 * op["cin"] * op["chain_cout"] for op in self._ops if op["kind"] == _lib.UDP_OP_SE)
