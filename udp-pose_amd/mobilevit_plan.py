"""Host compiler for pose_mobilevit_pixel_shuffle (deep_hrnet/lib/models/pose_mobilevit_pixel_shuffle.py:23-60) -> the
fused op program.

Graph restated from the reference (backbones/mobilevit.py, widths from backbones/configs/mobilevit.py:29-202): a 3x3 s2
conv + BN + SiLU (:711-714); layers 1 and 2 of ``InvertedResidual`` blocks (:155-201: 1x1 + BN + SiLU, depthwise 3x3 +
BN + SiLU, linear 1x1 + BN, the shortcut when stride 1 and in == out); layers 3-5 of a stride-2 ``InvertedResidual`` and
a ``MobileViTBlock`` (:517-677, :875-928) with 2 / 4 / 3 pre-norm transformer encoders (:469-514); ``conv_1x1_exp`` +
BN + SiLU (:750-753, applied by forward :821); then the decoder and head of the ShuffleNetV2 nets (shufflenet_plan.py):
``conv_compress``, three DUC blocks, ``final_layer``.

The unfolding / folding around the encoders (:593-655) never happens.  Between them sit only per-token ops -- LayerNorm
and linear layers, which are per-pixel ops and 1x1 convs on the NHWC map -- and the multi-head attention, which mixes the
N = HW / 4 pixels of one 2x2-position class: on the map pixel (y, x) simply belongs to class 2 (y & 1) + (x & 1)
(UDP_OP_LNORM, UDP_OP_MHATTN in include/udp_pose_hip.h).

Channel layout: every tensor holds its real channels first, zero-padded to a multiple of 32.  Pad channels are exact
zeros from every producer: zero weight and bias rows, silu(0) = 0, LayerNorm takes the real count and writes zeros
behind it, the attention writes zeros behind its d real channels.  The qkv conv stores q | k | v at 0 / dp / 2 dp of a
3 dp wide tensor through its output-channel map, so a head's real channels [h hd, (h + 1) hd) stay where the reference
has them inside each section; the hd^-0.5 scaling of q (:441) is folded into the q rows of its weight and bias in fp64.

A MobileViT block is 7 n + 7 launches: conv3x3 (code 0), ACT, conv1x1; n encoders of seven launches (LNORM, qkv conv,
MHATTN, out_proj + residual, LNORM, ffn + SiLU, ffn + residual); LNORM, conv_proj + SiLU, the fusion conv3x3 (code 0),
ACT.  The 3x3 conv kernels have no SiLU epilogue, hence the UDP_OP_ACT launches.  cat(block input, conv_proj output)
(:674-676) is never copied: the block input is written by its producer into the first half of a 2 Cp wide tensor,
conv_proj writes the second half, the first 3x3 conv reads its half as a view and the fusion conv's weight is laid out
for the two padded halves.

Launches at any width: stem 1 + layer 1 (3) + layer 2 (3 x 3) + layers 3-5 (3 x 3 + 7 x (2 + 4 + 3) + 7 x 3 = 93) +
conv_1x1_exp 1 + conv_compress 1 + DUC 6 + head 1 = 115.
"""
import torch

from . import _lib
from .program import _round_up
from .resnet_plan import _Tracked, _get
from .shufflenet_plan import ShuffleNetV2Program
from .synth_mobilevit import DECODER_INPLANES, ENCODERS, HEADS, MODEL_SIZES, unused_keys

NAME = "pose_mobilevit_pixel_shuffle"
N_LAUNCHES = 115


def mobilevit_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_mobilevit_pixel_shuffle YAML -> dict(model_size, architecture, start_channels,
    final_kernel, out_channels).  The reference reads the backbone's settings from a second YAML (MODEL.CONFIG,
    mobilevit.py:931-933); here EXTRA.MODEL_SIZE decides, with what all three shipped YAMLs say: four heads, 3x3 convs,
    fusion on.  Raises NotImplementedError for what cannot run."""
    size = _get(extra, "MODEL_SIZE", "xxs")
    if size not in MODEL_SIZES:
        raise NotImplementedError("%s MODEL_SIZE=%r (one of 'xxs', 'xs', 's', as pose_mobilevit_pixel_shuffle.py:27-34)" % (NAME, size))
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


class MobileViTProgram(ShuffleNetV2Program):
    NAME = NAME
    """On ``program.Program`` through the ShuffleNetV2 planner, whose ``_pw`` / ``_dw`` helpers it uses."""

    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        if dtype not in ("f32", "f16x2"):
            raise NotImplementedError("%s: dtype %r; supported storage modes are 'f32' and 'f16x2' (the depthwise, layer-norm "
                                      "and attention kernels have no bf16 form)" % (NAME, dtype))
        if in_h % 64 or in_w % 64:
            raise NotImplementedError("%s: input %dx%d: height and width must be multiples of 64 -- the attention works on "
                                      "2x2 patches down to 1/32 of the input, and the reference resizes maps of odd size "
                                      "bilinearly (mobilevit.py:598-605), which has no kernel" % (NAME, in_h, in_w))
        super().__init__(state_dict, spec, in_h, in_w, dtype)

    # ------------------------------------------------------------------ op helpers
    def _convlayer(self, name, x, cin_real, act, bn=True, **kw):
        """ConvLayer ``name`` (1x1 or 3x3, stride 1; + BatchNorm when ``bn``) over the first ``cin_real`` channels of
        ``x``; the output is padded to a multiple of 32.  ``kw``: ``_pw``'s views.  Returns (tensor, real channels)."""
        w, b = self._fold(name + ".block.conv", name + ".block.norm" if bn else None)
        cout = int(w.shape[0])
        if int(w.shape[1]) != cin_real or w.shape[2] != w.shape[3] or int(w.shape[2]) not in (1, 3):
            raise ValueError("%s.block.conv.weight must be [*,%d,k,k], k 1 or 3" % (name, cin_real))
        in_view = kw.pop("in_view", None)
        out = self._pw(name, x, w, b, act, cin_t=in_view or x.c, cout_t=_round_up(cout, 32), in_view=in_view, **kw)
        return out, cout

    def _linear(self, name, x, cin_real, act, res=None, q_rows=0, q_scale=1.0, out_map=None, cout_t=None):
        """LinearLayer ``name`` (mobilevit.py:231-238) on every pixel: a 1x1 conv with its [out, in] matrix and bias.
        ``q_rows`` / ``q_scale``: the first rows (and their bias) are scaled in fp64 before packing."""
        w = self.sd[name + ".weight"].detach().to(torch.float64).cpu()
        b = self.sd[name + ".bias"].detach().to(torch.float64).cpu()
        if w.dim() != 2 or int(w.shape[1]) != cin_real or tuple(b.shape) != (int(w.shape[0]),):
            raise ValueError("%s.weight must be [*,%d] with a bias" % (name, cin_real))
        if q_rows:
            w, b = w.clone(), b.clone()
            w[:q_rows] *= q_scale
            b[:q_rows] *= q_scale
        cout = int(w.shape[0])
        out = self._pw(name, x, w.to(torch.float32)[:, :, None, None], b.to(torch.float32), act, cin_t=x.c,
                       cout_t=cout_t or _round_up(cout, 32), out_map=out_map, res=res)
        return out, cout

    def _dw3(self, name, x, c_real, stride):
        """Depthwise ConvLayer ``name`` (3x3 + BN + SiLU) on ``x`` (``c_real`` real channels first)."""
        return self._dw(name + ".block.conv", name + ".block.norm", x, x.c, list(range(c_real)), stride, act=_lib.UDP_ACT_SILU)

    def _lnorm(self, name, x, r):
        """LayerNorm(r) ``name`` on every pixel of ``x`` (r real channels first) -> a new tensor: one UDP_OP_LNORM launch.
        Parameter block (include/udp_pose_hip.h): gamma [C], beta [C], zeros at the pad channels."""
        g, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        if tuple(g.shape) != (r,) or tuple(b.shape) != (r,):
            raise ValueError("%s: weight and bias must be [%d]" % (name, r))
        block = torch.zeros(2, x.c, dtype=torch.float32)
        block[0, :r], block[1, :r] = g.detach().float().cpu(), b.detach().float().cpu()
        out = self._new(x.c, x.h, x.w)
        self._emit(_lib.UDP_OP_LNORM, name, x, out, cin=x.c, cout=x.c, cout_pad=x.c, chain_cout=r,
                   w_off=self._put(block.contiguous().numpy().tobytes()))
        return out

    def _act(self, name, x):
        """SiLU on ``x`` in place: one UDP_OP_ACT launch (behind a 3x3 conv, whose kernels have no SiLU epilogue)."""
        self._emit(_lib.UDP_OP_ACT, name, x, x, relu=_lib.UDP_ACT_SILU, cin=x.c, cout=x.c, cout_pad=x.c)
        return x

    def _inverted_residual(self, p, x, cin, stride, in_view=None, into=None):
        """InvertedResidual ``p`` (:196-200) on ``x`` (``cin`` real channels; ``in_view``: the first channels of a wider
        tensor); ``into = (tensor, coff)`` for the output.  Returns (tensor, real channels)."""
        S = _lib.UDP_ACT_SILU
        h, hid = self._convlayer(p + ".block.exp_1x1", x, cin, S, in_view=in_view)
        h = self._dw3(p + ".block.conv_3x3", h, hid, stride)
        cout = int(self.sd[p + ".block.red_1x1.block.conv.weight"].shape[0])
        kw = {}
        if stride == 1 and cin == cout:              # use_res_connect (:172)
            if in_view is None:
                kw["res"] = x
            else:                                    # the shortcut from the stem tensor (xxs): a channel view of its buffer
                kw["res_view"] = (x, 0)
        out, _ = self._convlayer(p + ".block.red_1x1", h, hid, False, into=into, **kw)
        return out, cout

    def _mit_block(self, q, cat, c, n_enc):
        """MobileViTBlock ``q`` (forward :657-677); its input is the first half of ``cat`` (``c`` real channels of
        cat.c / 2), conv_proj's output becomes the second half."""
        S = _lib.UDP_ACT_SILU
        cp = cat.c // 2
        if cat.h % 2 or cat.w % 2:
            raise NotImplementedError("%s: a %dx%d map (the reference resizes it bilinearly, mobilevit.py:598-605)" % (q, cat.h, cat.w))
        t, _ = self._convlayer(q + ".local_rep.conv_3x3", cat, c, 0, in_view=cp)
        t = self._act(q + ".local_rep.conv_3x3.block.act", t)
        t, d = self._convlayer(q + ".local_rep.conv_1x1", t, c, False, bn=False)
        dp = t.c
        if d % HEADS:
            raise ValueError("%s: transformer width %d is no multiple of %d heads" % (q, d, HEADS))
        hd = d // HEADS
        for u in range(n_enc):
            g = "%s.global_rep.%d" % (q, u)
            a = self._lnorm(g + ".pre_norm_mha.0", t, d)
            # reference channel order: query, key, value (:433-439), each with its heads' channels in a row
            qkv, n = self._linear(g + ".pre_norm_mha.1.qkv_proj", a, d, False, q_rows=d, q_scale=float(hd) ** -0.5, cout_t=3 * dp,
                                  out_map=[(o // d) * dp + o % d for o in range(3 * d)])
            if n != 3 * d:
                raise ValueError("%s.pre_norm_mha.1.qkv_proj must have %d outputs" % (g, 3 * d))
            o = self._new(dp, t.h, t.w)
            self._emit(_lib.UDP_OP_MHATTN, g + ".pre_norm_mha.1", qkv, o, ks=2, cin=qkv.c, cout=dp, cout_pad=dp, chain_cout=d, heads=HEADS)
            t, _ = self._linear(g + ".pre_norm_mha.1.out_proj", o, d, False, res=t)
            f = self._lnorm(g + ".pre_norm_ffn.0", t, d)
            f, ffn = self._linear(g + ".pre_norm_ffn.1", f, d, S)
            t, _ = self._linear(g + ".pre_norm_ffn.4", f, ffn, False, res=t)
        t = self._lnorm("%s.global_rep.%d" % (q, n_enc), t, d)
        self._convlayer(q + ".conv_proj", t, d, S, into=(cat, cp))
        # fusion over cat(input, conv_proj output): logical channel j sits at j, c + j at cp + j
        w, b = self._fold(q + ".fusion.block.conv", q + ".fusion.block.norm")
        if tuple(w.shape) != (c, 2 * c, 3, 3):
            raise ValueError("%s.fusion.block.conv.weight must be [%d,%d,3,3]" % (q, c, 2 * c))
        y = self._pw(q + ".fusion", cat, w, b, 0, in_map=list(range(c)) + [cp + j for j in range(c)], cin_t=cat.c, cout_t=cp)
        return self._act(q + ".fusion.block.act", y), c

    # ------------------------------------------------------------------ the net
    def _build(self):
        self.sd = _Tracked(self.sd)
        sd, spec = self.sd, self.spec
        H, W = self.in_h, self.in_w
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
        x, c = self._inverted_residual("backbone.layer_1.0", x, c0, 1, in_view=32)    # reads the first 32 of the stem's 64
        x, c = self._inverted_residual("backbone.layer_2.0", x, c, 2)
        x, c = self._inverted_residual("backbone.layer_2.1", x, c, 1)
        x, c = self._inverted_residual("backbone.layer_2.2", x, c, 1)
        for li, n_enc in enumerate(ENCODERS):
            p = "backbone.layer_%d" % (li + 3)
            cout = int(sd[p + ".0.block.red_1x1.block.conv.weight"].shape[0])
            cat = self._new(2 * _round_up(cout, 32), x.h // 2, x.w // 2)   # [block input | conv_proj output]: the fusion conv's input
            _, c = self._inverted_residual(p + ".0", x, c, 2, into=(cat, 0))
            x, c = self._mit_block(p + ".1", cat, c, n_enc)
        x, c = self._convlayer("backbone.conv_1x1_exp", x, c, _lib.UDP_ACT_SILU)
        if c != DECODER_INPLANES[spec["model_size"]]:
            raise ValueError("%s: the decoder expects %d input channels, the backbone ends with %d" % (NAME, DECODER_INPLANES[spec["model_size"]], c))
        self._ps_head(x, c)
        # accepted and unused: BatchNorm bookkeeping and the ImageNet classifier forward() never applies (mobilevit.py:824-828)
        self.unused_keys = unused_keys(sd)
        sd.used.update(self.unused_keys)

    def macs_per_image(self):
        # + q k^T and the weighted sum of the values of every attention launch: 2 d N per pixel, N = HW / 4 keys
        # (soft-max, norms and the activation launches are not counted)
        return super().macs_per_image() + sum(2 * op["chain_cout"] * (op["hout"] * op["wout"] // 4) * op["hout"] * op["wout"]
                                              for op in self._ops if op["kind"] == _lib.UDP_OP_MHATTN)
