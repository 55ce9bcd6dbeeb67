"""Host compiler for pose_mobilevitv2_pixel_shuffle (deep_hrnet/lib/models/pose_mobilevitv2_pixel_shuffle.py:23-60)
-> the fused op program.

Graph restated from the reference (backbones/mobilevitv2.py, widths from backbones/configs/mobilevitv2.py:39-105): a
3x3 s2 conv + BN + SiLU (:1198-1206); layers 1 and 2 of ``InvertedResidual`` blocks (:185-230: 1x1 + BN + SiLU,
depthwise 3x3 + BN + SiLU, linear 1x1 + BN, the shortcut when stride 1 and in == out); layers 3-5 of a stride-2
``InvertedResidual`` and a ``MobileViTBlockv2`` (:858-1126, :1313-1366) with 2 / 4 / 3 attention units; then the decoder
and head of the ShuffleNetV2 nets (shufflenet_plan.py): ``conv_compress``, three DUC blocks, ``final_layer``.

The unfold / fold around the attention units (:1026-1055) never happens.  Between them sit only 1x1 convs,
GroupNorm(1, C) over the whole sample, and the separable attention whose soft-max runs over the patches separately for
each of the 2 x 2 positions inside a patch -- on the NHWC map pixel (y, x) simply belongs to class 2 (y & 1) + (x & 1)
(UDP_OP_GNORM, UDP_OP_LINATTN in include/udp_pose_hip.h).

Channel layout: every tensor holds its real channels first, zero-padded to a multiple of 32 (the 0.75 net has 24 / 48 /
144 / 288 channels).  Pad channels are exact zeros from every producer: zero weights and bias rows, silu(0) = 0, and
GroupNorm takes the real count and writes zeros behind it.  The qkv conv stores key | value | query (the reference's
order is query, key, value :671-673) at 0 / Cp / 2 Cp of a 2 Cp + 32 wide tensor through its output-channel map.

An attention unit (LinearAttnFFN.forward :839-855) is seven launches: GNORM, qkv conv + bias, LINATTN, out_proj + bias +
residual, GNORM, ffn 1x1 + bias + SiLU, ffn 1x1 + bias + residual.

Launches at any width: stem 1 + layer 1 (3) + layer 2 (3 + 3) + layer 3 (3 + [2 + 2 x 7 + 2] = 21) + layer 4
(3 + [2 + 4 x 7 + 2] = 35) + layer 5 (3 + [2 + 3 x 7 + 2] = 28) + conv_compress 1 + DUC 6 + head 1 = 102.
"""
import torch

from . import _lib
from .program import _round_up
from .resnet_plan import _Tracked, _get
from .shufflenet_plan import ShuffleNetV2Program
from .synth_mobilevitv2 import ATTN_BLOCKS, DECODER_INPLANES, MODEL_SIZES, unused_keys

NAME = "pose_mobilevitv2_pixel_shuffle"
N_LAUNCHES = 102


def mobilevitv2_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_mobilevitv2_pixel_shuffle YAML -> dict(model_size, architecture, start_channels,
    final_kernel, out_channels).  The reference reads the width from a second YAML (MODEL.CONFIG,
    mobilevitv2.py:1456-1458); here EXTRA.MODEL_SIZE decides.  Raises NotImplementedError for what cannot run."""
    try:
        size = float(_get(extra, "MODEL_SIZE", 0.5))
    except (TypeError, ValueError):
        size = None
    if size not in MODEL_SIZES:
        raise NotImplementedError("%s MODEL_SIZE=%r (one of 0.5, 0.75, 1.0, as pose_mobilevitv2_pixel_shuffle.py:27-34)"
                                  % (NAME, _get(extra, "MODEL_SIZE", None)))
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


class MobileViTv2Program(ShuffleNetV2Program):
    NAME = NAME
    """On ``program.Program`` through the ShuffleNetV2 planner, whose ``_pw`` / ``_dw`` helpers it uses."""

    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        if dtype not in ("f32", "f16x2"):
            raise NotImplementedError("%s: dtype %r; supported storage modes are 'f32' and 'f16x2' (the depthwise, group-norm "
                                      "and attention kernels have no bf16 form)" % (NAME, dtype))
        if in_h % 64 or in_w % 64:
            raise NotImplementedError("%s: input %dx%d: height and width must be multiples of 64 -- the attention works on "
                                      "2x2 patches down to 1/32 of the input, and the reference resizes maps of odd size "
                                      "bilinearly (mobilevitv2.py:1095-1103), which has no kernel" % (NAME, in_h, in_w))
        super().__init__(state_dict, spec, in_h, in_w, dtype)

    # ------------------------------------------------------------------ op helpers
    def _conv1(self, name, x, cin_real, act, bn=True, res=None, out_map=None, cout_t=None, in_view=None):
        """ConvLayer ``name`` (1x1; + BatchNorm when ``bn``, else + its bias if it has one) over the first ``cin_real``
        channels of ``x``; the output is padded to a multiple of 32.  Returns (tensor, real channels)."""
        w, b = self._fold(name + ".block.conv", name + ".block.norm" if bn else None)
        cout = int(w.shape[0])
        if tuple(w.shape[1:]) != (cin_real, 1, 1):
            raise ValueError("%s.block.conv.weight must be [*,%d,1,1]" % (name, cin_real))
        out = self._pw(name, x, w, b, act, cin_t=in_view or x.c, cout_t=cout_t or _round_up(cout, 32), out_map=out_map,
                       in_view=in_view, res=res)
        return out, cout

    def _dw3(self, name, x, c_real, stride):
        """Depthwise ConvLayer ``name`` (3x3 + BN + SiLU) on ``x`` (``c_real`` real channels first)."""
        return self._dw(name + ".block.conv", name + ".block.norm", x, x.c, list(range(c_real)), stride, act=_lib.UDP_ACT_SILU)

    def _gnorm(self, name, x, r):
        """GroupNorm(1, r) ``name`` on ``x`` (r real channels first) -> a new tensor: one UDP_OP_GNORM launch.
        Parameter block (include/udp_pose_hip.h): gamma [C], beta [C], zeros at the pad channels."""
        g, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        if tuple(g.shape) != (r,) or tuple(b.shape) != (r,):
            raise ValueError("%s: weight and bias must be [%d]" % (name, r))
        block = torch.zeros(2, x.c, dtype=torch.float32)
        block[0, :r], block[1, :r] = g.detach().float().cpu(), b.detach().float().cpu()
        out = self._new(x.c, x.h, x.w)
        self._emit(_lib.UDP_OP_GNORM, name, x, out, cin=x.c, cout=x.c, cout_pad=x.c, chain_cout=r,
                   w_off=self._put(block.contiguous().numpy().tobytes()))
        return out

    def _inverted_residual(self, p, x, cin, in_view=None):
        """InvertedResidual ``p`` (:226-230) on ``x`` (``cin`` real channels); returns (tensor, real channels)."""
        stride = 1 if p in self._stride1 else 2
        S = _lib.UDP_ACT_SILU
        h, hid = self._conv1(p + ".block.exp_1x1", x, cin, S, in_view=in_view)
        h = self._dw3(p + ".block.conv_3x3", h, hid, stride)
        cout = int(self.sd[p + ".block.red_1x1.block.conv.weight"].shape[0])
        res = x if stride == 1 and cin == cout and in_view is None else None
        if stride == 1 and cin == cout and res is None:
            raise ValueError("%s: a shortcut from the stem tensor is not planned for" % p)
        return self._conv1(p + ".block.red_1x1", h, hid, False, res=res)

    def _mit_block(self, q, x, c, n_units):
        """MobileViTBlockv2 ``q`` (forward_spatial :1105-1126) on ``x`` (``c`` real channels)."""
        S = _lib.UDP_ACT_SILU
        if x.h % 2 or x.w % 2:
            raise NotImplementedError("%s: a %dx%d map (the reference resizes it bilinearly, mobilevitv2.py:1095-1103)" % (q, x.h, x.w))
        t = self._dw3(q + ".local_rep.0", x, c, 1)
        t, d = self._conv1(q + ".local_rep.1", t, c, False, bn=False)
        dp = t.c
        for u in range(n_units):
            g = "%s.global_rep.%d" % (q, u)
            a = self._gnorm(g + ".pre_norm_attn.0", t, d)
            # reference channel order: query, key, value (:671-673) -> key at 0, value at dp, query at 2 dp
            qkv, n = self._conv1(g + ".pre_norm_attn.1.qkv_proj", a, d, False, bn=False, cout_t=2 * dp + 32,
                                 out_map=[2 * dp] + list(range(d)) + [dp + j for j in range(d)])
            if n != 1 + 2 * d:
                raise ValueError("%s.pre_norm_attn.1.qkv_proj must have %d outputs" % (g, 1 + 2 * d))
            o = self._new(dp, t.h, t.w)
            self._emit(_lib.UDP_OP_LINATTN, g + ".pre_norm_attn.1", qkv, o, ks=2, cin=qkv.c, cout=dp, cout_pad=dp)
            t, _ = self._conv1(g + ".pre_norm_attn.1.out_proj", o, d, False, bn=False, res=t)
            f = self._gnorm(g + ".pre_norm_ffn.0", t, d)
            f, ffn = self._conv1(g + ".pre_norm_ffn.1", f, d, S, bn=False)
            t, _ = self._conv1(g + ".pre_norm_ffn.3", f, ffn, False, bn=False, res=t)
        t = self._gnorm("%s.global_rep.%d" % (q, n_units), t, d)
        return self._conv1(q + ".conv_proj", t, d, False)

    # ------------------------------------------------------------------ the net
    def _build(self):
        self.sd = _Tracked(self.sd)
        sd, spec = self.sd, self.spec
        H, W = self.in_h, self.in_w
        self._stride1 = {"backbone.layer_1.0", "backbone.layer_2.1"}          # configs/mobilevitv2.py:59, :66 (+ i > 0)
        # stem: the kernel computes 64 output channels; the real ones first, zero weights and bias behind them (silu(0) = 0)
        w, b = self._fold("backbone.conv_1.block.conv", "backbone.conv_1.block.norm")
        c0 = int(w.shape[0])
        if tuple(w.shape[1:]) != (3, 3, 3) or c0 > 32:
            raise ValueError("backbone.conv_1.block.conv.weight must be [<=32,3,3,3]")
        wp = torch.zeros(64, 3, 3, 3)
        wp[:c0] = w
        bp = torch.zeros(64)
        bp[:c0] = b
        x = self._new(64, H // 2, W // 2)
        self._emit(_lib.UDP_OP_STEM, "backbone.conv_1.block.conv", None, x, ks=3, stride=2, relu=_lib.UDP_ACT_SILU,
                   w_off=self._put(wp.permute(2, 3, 1, 0).contiguous().numpy().tobytes()), b_off=self._put(bp.numpy().tobytes()))
        x, c = self._inverted_residual("backbone.layer_1.0", x, c0, in_view=32)       # reads the first 32 of the stem's 64
        x, c = self._inverted_residual("backbone.layer_2.0", x, c)
        x, c = self._inverted_residual("backbone.layer_2.1", x, c)
        for li, n_units in enumerate(ATTN_BLOCKS):
            p = "backbone.layer_%d" % (li + 3)
            x, c = self._inverted_residual(p + ".0", x, c)
            x, c = self._mit_block(p + ".1", x, c, n_units)
        if c != DECODER_INPLANES[spec["model_size"]]:
            raise ValueError("%s: the decoder expects %d input channels, the backbone ends with %d" % (NAME, DECODER_INPLANES[spec["model_size"]], c))
        self._ps_head(x, c)
        # accepted and unused: BatchNorm bookkeeping and the ImageNet classifier forward() never applies (mobilevitv2.py:1440-1444)
        self.unused_keys = unused_keys(sd)
        sd.used.update(self.unused_keys)

    def macs_per_image(self):
        # + the weighted sum of the keys of every attention launch (soft-max, gate and the norms are not counted)
        return super().macs_per_image() + sum(op["cout"] * op["hout"] * op["wout"] for op in self._ops if op["kind"] == _lib.UDP_OP_LINATTN)
