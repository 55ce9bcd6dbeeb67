"""pose_mobilevit_pixel_shuffle weight-file contract + seeded synthetic weights.

Key names / shapes of ``PoseMobileVitPixelShuffle.state_dict()``
(deep_hrnet/lib/models/pose_mobilevit_pixel_shuffle.py:23-60 with backbones/mobilevit.py:155-201, :203-238, :369-395,
:469-496, :517-573, :680-770, widths from backbones/configs/mobilevit.py:29-202, and decoders/pixelshuffle.py:7-26,
DUC.py:15-21), in the module's registration order -- including ``backbone.classifier``, which the backbone registers
and its forward() never applies (:824-828, ``clf`` is False).  The synthetic generator draws in that order exactly like
tools/gen_golden_mobilevit.py did when it produced tests/golden/mobilevit_xxs_ps.npz, so the fixture's heat-maps can be
reproduced without the reference.
"""
from collections import OrderedDict

import numpy as np
import torch

from .synth_mobilevitv2 import make_divisible
from .synth_shufflenet import _bn

MODEL_SIZES = ("xxs", "xs", "s")
DECODER_INPLANES = {"xxs": 320, "xs": 384, "s": 640}         # pose_mobilevit_pixel_shuffle.py:27-32
ENCODERS = (2, 4, 3)                                          # layer3 .. layer5 (configs/mobilevit.py:50, :63, :76)
HEADS = 4                                                     # number_heads of all three shipped backbone YAMLs
N_CLASS = 1000                                                # the unused ImageNet classifier (mobilevit.py:757-764)

# (layer 1 out, layer 2 out, mv2 expand ratio, [(out, transformer dim, ffn dim)] of layers 3-5), configs/mobilevit.py:29-202
_WIDTHS = {
    "xxs": (16, 24, 2, ((48, 64, 128), (64, 80, 160), (80, 96, 192))),
    "xs": (32, 48, 4, ((64, 96, 192), (80, 120, 240), (96, 144, 288))),
    "s": (32, 64, 4, ((96, 144, 288), (128, 192, 384), (160, 240, 480))),
}
STEM = 16                                                     # mobilevit.py:692


def mobilevit_widths(model_size):
    """(stem, layer1, layer2, mv2 expand ratio, [(out, transformer dim, ffn dim, encoders)] of layers 3-5)."""
    c1, c2, exp, mit = _WIDTHS[model_size]
    return STEM, c1, c2, exp, [(o, d, f, n) for (o, d, f), n in zip(mit, ENCODERS)]


def _conv_bn(s, name, cout, cin, k):
    """ConvLayer with a norm (:289-301): block.conv (no bias) + block.norm."""
    s[name + ".block.conv.weight"] = (cout, cin, k, k)
    _bn(s, name + ".block.norm", cout)


def _linear(s, name, cout, cin):
    """LinearLayer (:217-220): a [out, in] matrix and a bias."""
    s[name + ".weight"] = (cout, cin)
    s[name + ".bias"] = (cout,)


def _ln(s, name, c):
    s[name + ".weight"] = (c,)
    s[name + ".bias"] = (c,)


def _inverted_residual(s, name, cin, cout, expand):
    """InvertedResidual (:171-190)."""
    hid = make_divisible(int(round(cin * expand)), 8)
    _conv_bn(s, name + ".block.exp_1x1", hid, cin, 1)
    _conv_bn(s, name + ".block.conv_3x3", hid, 1, 3)
    _conv_bn(s, name + ".block.red_1x1", cout, hid, 1)


def mobilevit_param_shapes(model_size="xxs", num_joints=17, target_type="gaussian", start_channels=256,
                           architecture=(512, 256, 128), final_kernel=1):
    c0, c1, c2, exp, mit = mobilevit_widths(model_size)
    s = OrderedDict()
    _conv_bn(s, "backbone.conv_1", c0, 3, 3)
    _inverted_residual(s, "backbone.layer_1.0", c0, c1, exp)
    _inverted_residual(s, "backbone.layer_2.0", c1, c2, exp)
    _inverted_residual(s, "backbone.layer_2.1", c2, c2, exp)
    _inverted_residual(s, "backbone.layer_2.2", c2, c2, exp)
    cin = c2
    for li, (out, d, ffn, n) in enumerate(mit):
        p = "backbone.layer_%d" % (li + 3)
        _inverted_residual(s, p + ".0", cin, out, exp)
        q = p + ".1"                                              # MobileViTBlock (:551-573)
        _conv_bn(s, q + ".local_rep.conv_3x3", out, out, 3)
        s[q + ".local_rep.conv_1x1.block.conv.weight"] = (d, out, 1, 1)
        for u in range(n):                                        # TransformerEncoder (:480-493)
            g = "%s.global_rep.%d" % (q, u)
            _ln(s, g + ".pre_norm_mha.0", d)
            _linear(s, g + ".pre_norm_mha.1.qkv_proj", 3 * d, d)
            _linear(s, g + ".pre_norm_mha.1.out_proj", d, d)
            _ln(s, g + ".pre_norm_ffn.0", d)
            _linear(s, g + ".pre_norm_ffn.1", ffn, d)
            _linear(s, g + ".pre_norm_ffn.4", d, ffn)
        _ln(s, "%s.global_rep.%d" % (q, n), d)
        _conv_bn(s, q + ".conv_proj", out, d, 1)
        _conv_bn(s, q + ".fusion", out, 2 * out, 3)
        cin = out
    cexp = min(4 * cin, 960)                                      # :749
    _conv_bn(s, "backbone.conv_1x1_exp", cexp, cin, 1)
    s["backbone.classifier.fc.weight"] = (N_CLASS, cexp)
    s["backbone.classifier.fc.bias"] = (N_CLASS,)
    s["decoder.conv_compress.weight"] = (start_channels, DECODER_INPLANES[model_size], 1, 1)
    cin = start_channels
    for k, planes in enumerate(architecture):
        s["decoder.duc.%d.conv.weight" % k] = (planes, cin, 3, 3)
        _bn(s, "decoder.duc.%d.bn" % k, planes)
        cin = planes // 4
    nout = num_joints * (3 if target_type == "offset" else 1)
    s["final_layer.weight"] = (nout, cin, final_kernel, final_kernel)
    s["final_layer.bias"] = (nout,)
    return s


def unused_keys(shapes):
    """Keys the reference's forward() never applies: the ImageNet classifier and the BatchNorm step counters."""
    return {k for k in shapes if k.startswith("backbone.classifier.") or k.endswith("num_batches_tracked")}


def synth_mobilevit_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """Seeded weights: convs and the encoders' matrices ~ N(0, 2 / fan_in) (the classifier's ~ N(0, 0.01^2)), norm
    weights ~ U(0.5, 1), biases ~ N(0, 0.05), running statistics 0 / 1 unless ``calib`` ({key: array}) supplies them;
    the head is multiplied by ``final_scale``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, shape in mobilevit_param_shapes(**kw).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3]
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / fan)).astype(np.float32))
        elif len(shape) == 2:
            std = 0.01 if k.startswith("backbone.classifier.") else np.sqrt(2.0 / shape[1])
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32))
        elif k.endswith(".weight"):
            sd[k] = torch.from_numpy(rng.uniform(0.5, 1.0, shape).astype(np.float32))
        elif k.endswith(".bias"):
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * 0.05).astype(np.float32))
        elif k.endswith("running_var"):
            sd[k] = torch.ones(shape)
        else:
            sd[k] = torch.zeros(shape)
    if calib:
        for k, v in calib.items():
            sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32).copy())
    sd["final_layer.weight"] = sd["final_layer.weight"] * float(final_scale)
    sd["final_layer.bias"] = sd["final_layer.bias"] * float(final_scale)
    return sd
