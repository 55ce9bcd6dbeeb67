"""Host compiler for pose_mobilenetv3_small_pixel_shuffle and pose_mobilenetv3_small
(deep_hrnet/lib/models/pose_mobilenetv3_small_pixel_shuffle.py:23-52, pose_mobilenetv3_small.py) -> the fused op program.

The backbone is torchvision's ``mobilenet_v3_small().features`` (backbones/mobilenetv3.py:5-16), restated as the table
of synth_mobilenetv3.py: a 3x3 s2 conv + BN + hard-swish, eleven InvertedResidual blocks (expand 1x1 + BN + act,
depthwise 3x3 / 5x5 + BN + act, squeeze-excitation with biased fc1 / fc2, project 1x1 + BN, the shortcut when stride 1
and in == out), a 1x1 conv 96 -> 576 + BN + hard-swish; every backbone BatchNorm has eps 1e-3.  Behind it the
pixel-shuffle head (shufflenet_plan.ShuffleNetV2Program._ps_head) or the deconv head (program.Program._deconv_head).

Channel layout: a tensor of c real channels stores round_up(c, 32), the real ones first, exact zeros behind them from
every producer (zero weights and bias; act(0) = 0).  Launches per block:

* expand: a plain 1x1 UDP_OP_CONV with the block's activation code (1 ReLU / 2 hard-swish) -- absent in block 1;
* depthwise: UDP_OP_DWCONV with code 1 in an RE block; in an HS block code 0, because that kernel has no hard-swish
  epilogue, and the activation moves into the next launch;
* squeeze-excitation: ONE UDP_OP_SE_ACT in place, with code 0 behind an RE depthwise conv and code 2 behind an HS one
  (it applies the activation while it pools and while it scales).  An HS block without squeeze-excitation -- none in
  ``small`` -- gets a UDP_OP_ACT instead;
* project: a 1x1 UDP_OP_CONV without activation, the shortcut as ``res``.

``small`` at any input size: stem 1 + blocks (3 + 3 + 3 + 8 x 4 = 41) + last conv 1 = 43 launches, + conv_compress 1 +
DUC 6 + head 1 = 51 (pixel shuffle) or + deconv 3 + head 1 = 47 (deconv).
"""
import torch

from . import _lib
from .program import _round_up
from .resnet_plan import _get, _head_spec
from .shufflenet_plan import ShuffleNetV2Program
from .synth_mobilenetv3 import BACKBONE_BN_EPS, BLOCKS, LAST_CHANNELS

NAME_PS = "pose_mobilenetv3_small_pixel_shuffle"
NAME_DECONV = "pose_mobilenetv3_small"


def _model_size(name, extra):
    size = str(_get(extra, "MODEL_SIZE", "small"))
    if size == "large":
        raise NotImplementedError("%s MODEL_SIZE='large': the reference itself cannot run it -- the large backbone ends in 960 "
                                  "channels but the head is built for %d (inplanes is hard-coded, :26)" % (name, LAST_CHANNELS))
    if size != "small":
        raise NotImplementedError("%s MODEL_SIZE=%r ('small')" % (name, size))
    return size


def mobilenetv3_ps_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_mobilenetv3_small_pixel_shuffle YAML -> dict(model_size, architecture, start_channels,
    final_kernel, out_channels).  Raises NotImplementedError for what cannot run."""
    size = _model_size(NAME_PS, extra)
    arch = tuple(int(a) for a in _get(extra, "ARCHITECTURE", (512, 256, 128)))
    if len(arch) != 3 or any(a <= 0 or a % 128 for a in arch):
        raise NotImplementedError("%s ARCHITECTURE=%s: three DUC blocks (heat-maps at 1/4 of the input) with multiples of "
                                  "128 channels are supported" % (NAME_PS, arch))
    start = int(_get(extra, "START_CHANNELS", 256))
    if start <= 0 or start % 32:
        raise NotImplementedError("%s START_CHANNELS=%d (a multiple of 32)" % (NAME_PS, start))
    final_kernel = int(_get(extra, "FINAL_CONV_KERNEL", 1))
    if final_kernel not in (1, 3):
        raise NotImplementedError("%s FINAL_CONV_KERNEL=%d (1 or 3)" % (NAME_PS, final_kernel))
    return dict(model_size=size, architecture=arch, start_channels=start, final_kernel=final_kernel,
                out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


def mobilenetv3_deconv_spec(extra, num_joints=17, target_type="gaussian"):
    """MODEL.EXTRA of a pose_mobilenetv3_small YAML -> dict(model_size, deconv_filters, final_kernel, deconv_with_bias,
    out_channels), with the head refusals of ``resnet_plan._head_spec``."""
    size = _model_size(NAME_DECONV, extra)
    return dict(_head_spec(extra, NAME_DECONV), model_size=size, out_channels=int(num_joints) * (3 if target_type == "offset" else 1))


class MobileNetV3Program(ShuffleNetV2Program):
    """Both nets: the head follows the spec (``deconv_filters``: the deconv head, else pixel shuffle)."""
    DW_KERNELS = (3, 5)

    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        self.NAME = NAME_DECONV if "deconv_filters" in spec else NAME_PS
        if dtype == "bf16":
            raise NotImplementedError("%s: dtype 'bf16'; supported storage modes are 'f32' and 'f16x2' (the depthwise and "
                                      "squeeze-excitation kernels have no bf16 form)" % self.NAME)
        super().__init__(state_dict, spec, in_h, in_w, dtype)

    def _fold3(self, conv, bn):
        return self._fold(conv, bn, eps=BACKBONE_BN_EPS)

    def _se_act(self, name, t, r, act):
        """SqueezeExcitation ``name`` (fc1 / fc2 with biases) on ``t`` (r real channels first) with activation ``act``
        applied to the input, in place: one UDP_OP_SE_ACT launch.  Parameter block (include/udp_pose_hip.h): W1
        transposed [C][Ch], b1 [Ch], W2 transposed [Ch][C], b2 [C]; zero rows / columns / biases at the pad channels."""
        w1, b1 = self._fold(name + ".fc1")
        w2, b2 = self._fold(name + ".fc2")
        c, hid = t.c, int(w1.shape[0])
        if tuple(w1.shape) != (hid, r, 1, 1) or tuple(w2.shape) != (r, hid, 1, 1) or hid < 1:
            raise ValueError("%s: squeeze-excitation weights must be [%d,%d,1,1] and [%d,%d,1,1]" % (name, hid, r, r, hid))
        w1t = torch.zeros(c, hid, dtype=torch.float32)
        w1t[:r] = w1.reshape(hid, r).t()
        w2t = torch.zeros(hid, c, dtype=torch.float32)
        w2t[:, :r] = w2.reshape(r, hid).t()
        b2p = torch.zeros(c, dtype=torch.float32)
        b2p[:r] = b2
        block = torch.cat([w1t.reshape(-1), b1, w2t.reshape(-1), b2p]).contiguous()
        self._emit(_lib.UDP_OP_SE_ACT, name, t, t, relu=act, cin=c, cout=c, cout_pad=c, chain_cout=hid,
                   w_off=self._put(block.numpy().tobytes()))

    def _block(self, p, x, cin, k, exp, cout, se, act, stride):
        """InvertedResidual ``p`` on ``x`` (cin real channels first): returns its output tensor."""
        code = _lib.UDP_ACT_HSWISH if act == "HS" else _lib.UDP_ACT_RELU
        cs, es = _round_up(cin, 32), _round_up(exp, 32)
        q, m = p + ".block", 0
        t = x
        if exp != cin:
            w, b = self._fold3("%s.%d.0" % (q, m), "%s.%d.1" % (q, m))
            t = self._pw("%s.%d.0" % (q, m), x, w, b, code, cin_t=cs, cout_t=es, in_view=cs if cs != x.c else None)
            m += 1
        hs = act == "HS"
        # (a block without an expand conv reads the first es stored channels of a wider input: block 1 and the stem's 64)
        d = self._dw("%s.%d.0" % (q, m), "%s.%d.1" % (q, m), t, es, list(range(exp)), stride, act=0 if hs else _lib.UDP_ACT_RELU,
                     eps=BACKBONE_BN_EPS)
        m += 1
        if se:
            self._se_act("%s.%d" % (q, m), d, exp, _lib.UDP_ACT_HSWISH if hs else _lib.UDP_ACT_NONE)
            m += 1
        elif hs:        # hard-swish without a squeeze-excitation to carry it: one UDP_OP_ACT, in place
            self._emit(_lib.UDP_OP_ACT, "%s.%d.2" % (q, m - 1), d, d, relu=_lib.UDP_ACT_HSWISH, cin=d.c, cout=d.c, cout_pad=d.c)
        w, b = self._fold3("%s.%d.0" % (q, m), "%s.%d.1" % (q, m))
        res = x if stride == 1 and cin == cout else None
        if res is not None and res.c != _round_up(cout, 32):
            raise ValueError("%s: the shortcut has %d stored channels, the output %d" % (p, res.c, _round_up(cout, 32)))
        return self._pw("%s.%d.0" % (q, m), d, w, b, False, cin_t=es, cout_t=_round_up(cout, 32), res=res)

    def _backbone(self):
        H, W = self.in_h, self.in_w
        HS = _lib.UDP_ACT_HSWISH
        # stem: the kernel computes 64 output channels; the real ones first, zero weights and bias behind them (hswish(0) = 0)
        w, b = self._fold3("backbone.0.0.0", "backbone.0.0.1")
        c0 = int(w.shape[0])
        if tuple(w.shape[1:]) != (3, 3, 3) or c0 > 64:
            raise ValueError("backbone.0.0.0.weight must be [<=64,3,3,3]")
        wp = torch.zeros(64, 3, 3, 3)
        wp[:c0] = w
        bp = torch.zeros(64)
        bp[:c0] = b
        x = self._new(64, H // 2, W // 2)
        self._emit(_lib.UDP_OP_STEM, "backbone.0.0.0", None, x, ks=3, stride=2, relu=HS,
                   w_off=self._put(wp.permute(2, 3, 1, 0).contiguous().numpy().tobytes()), b_off=self._put(bp.numpy().tobytes()))
        c = c0
        for i, (cin, k, exp, cout, se, act, stride) in enumerate(BLOCKS, start=1):
            if cin != c:
                raise ValueError("backbone.0.%d expects %d input channels, got %d" % (i, cin, c))
            x, c = self._block("backbone.0.%d" % i, x, cin, k, exp, cout, se, act, stride), cout
        w, b = self._fold3("backbone.0.12.0", "backbone.0.12.1")
        x = self._pw("backbone.0.12.0", x, w, b, HS, cin_t=x.c)
        if x.c != LAST_CHANNELS:
            raise ValueError("%s: the head expects %d input channels, the backbone ends with %d" % (self.NAME, LAST_CHANNELS, x.c))
        return x

    def _mark_unused(self):
        for k in self.sd:
            if k.endswith("num_batches_tracked"):
                self.sd.used.add(k)             # BatchNorm bookkeeping, not an operand

    def macs_per_image(self):
        # + the two small products of every squeeze-excitation layer (its activation, pool and scale are not counted)
        return super().macs_per_image() + sum(2 * op["cin"] * op["chain_cout"] for op in self._ops if op["kind"] == _lib.UDP_OP_SE_ACT)
