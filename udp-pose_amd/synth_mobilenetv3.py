"""pose_mobilenetv3_small / pose_mobilenetv3_small_pixel_shuffle weight-file contract + seeded synthetic weights.

Key names / shapes of the two modules' ``state_dict()`` (deep_hrnet/lib/models/pose_mobilenetv3_small.py,
pose_mobilenetv3_small_pixel_shuffle.py), in registration order.  The backbone is torchvision's
``mobilenet_v3_small()`` with its last two children cut off (backbones/mobilenetv3.py:9-12): ``nn.Sequential(features)``,
so every backbone key starts with ``backbone.0.``.  torchvision is not a dependency here; the net is defined by the
table below, which is its ``features``:

* ``backbone.0.0``: Conv 3 -> 16, k3 s2 p1 (``.0.weight``), BatchNorm (``.1.*``), hard-swish;
* ``backbone.0.1`` .. ``backbone.0.11``: InvertedResidual, ``BLOCKS`` below; members of ``.block`` in order: the
  expand 1x1 conv + BN + act (only when exp != in), the depthwise k x k conv (stride s, pad (k - 1) / 2) + BN + act,
  the squeeze-excitation (``fc1`` / ``fc2`` with biases, ReLU between them, Hardsigmoid behind), the project 1x1
  conv + BN without activation; ``x + block(x)`` when the stride is 1 and in == out;
* ``backbone.0.12``: Conv 96 -> 576 1x1 + BN + hard-swish.

Every backbone BatchNorm has eps = 1e-3 (``BACKBONE_BN_EPS``); the heads' keep 1e-5.
"""
from collections import OrderedDict

from .synth_shufflenet import _bn, _final, deconv_head_shapes, seeded_state_dict

# (in, kernel, expanded, out, squeeze-excitation, activation, stride) of backbone.0.1 .. backbone.0.11
BLOCKS = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
          (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
          (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
          (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
STEM_CHANNELS = 16
LAST_CHANNELS = 576              # backbone.0.12 and ``inplanes`` of both pose modules (:26)
BACKBONE_BN_EPS = 1e-3
BACKBONE_PARAMS = 927008         # conv / BatchNorm / squeeze-excitation weights and biases (no buffers): the
                                 # torchvision model's 2 542 856 minus its classifier


def make_divisible(v, divisor=8):
    """torchvision.ops.misc / mobilenetv3's ``_make_divisible``."""
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def squeeze_channels(exp):
    return make_divisible(exp // 4, 8)


def backbone_param_shapes():
    s = OrderedDict()
    s["backbone.0.0.0.weight"] = (STEM_CHANNELS, 3, 3, 3)
    _bn(s, "backbone.0.0.1", STEM_CHANNELS)
    for i, (cin, k, exp, cout, se, act, stride) in enumerate(BLOCKS, start=1):
        p, m = "backbone.0.%d.block" % i, 0
        if exp != cin:
            s["%s.%d.0.weight" % (p, m)] = (exp, cin, 1, 1)
            _bn(s, "%s.%d.1" % (p, m), exp)
            m += 1
        s["%s.%d.0.weight" % (p, m)] = (exp, 1, k, k)
        _bn(s, "%s.%d.1" % (p, m), exp)
        m += 1
        if se:
            sq = squeeze_channels(exp)
            s["%s.%d.fc1.weight" % (p, m)] = (sq, exp, 1, 1)
            s["%s.%d.fc1.bias" % (p, m)] = (sq,)
            s["%s.%d.fc2.weight" % (p, m)] = (exp, sq, 1, 1)
            s["%s.%d.fc2.bias" % (p, m)] = (exp,)
            m += 1
        s["%s.%d.0.weight" % (p, m)] = (cout, exp, 1, 1)
        _bn(s, "%s.%d.1" % (p, m), cout)
    s["backbone.0.12.0.weight"] = (LAST_CHANNELS, BLOCKS[-1][3], 1, 1)
    _bn(s, "backbone.0.12.1", LAST_CHANNELS)
    return s


def mobilenetv3_ps_param_shapes(num_joints=17, target_type="gaussian", start_channels=256, architecture=(512, 256, 128),
                                final_kernel=1):
    """pose_mobilenetv3_small_pixel_shuffle."""
    s = backbone_param_shapes()
    s["decoder.conv_compress.weight"] = (start_channels, LAST_CHANNELS, 1, 1)
    cin = start_channels
    for d, planes in enumerate(architecture):
        s["decoder.duc.%d.conv.weight" % d] = (planes, cin, 3, 3)
        _bn(s, "decoder.duc.%d.bn" % d, planes)
        cin = planes // 4
    return _final(s, cin, num_joints, target_type, final_kernel)


def mobilenetv3_deconv_param_shapes(num_joints=17, target_type="gaussian", deconv_filters=(256, 256, 256), final_kernel=1,
                                    deconv_with_bias=False):
    """pose_mobilenetv3_small."""
    return deconv_head_shapes(backbone_param_shapes(), LAST_CHANNELS, num_joints, target_type, deconv_filters, final_kernel,
                              deconv_with_bias)


def synth_mobilenetv3_state_dict(seed=7, head="pixel_shuffle", calib=None, final_scale=1.0, **kw):
    """``head``: "pixel_shuffle" (pose_mobilenetv3_small_pixel_shuffle) or "deconv" (pose_mobilenetv3_small)."""
    shapes = mobilenetv3_ps_param_shapes(**kw) if head == "pixel_shuffle" else mobilenetv3_deconv_param_shapes(**kw)
    return seeded_state_dict(shapes, seed, calib, final_scale)
