"""pose_mobilevitv2_pixel_shuffle weight-file contract + seeded synthetic weights.

Key names / shapes of ``PoseMobileVitV2PixelShuffle.state_dict()``
(deep_hrnet/lib/models/pose_mobilevitv2_pixel_shuffle.py:23-60 with backbones/mobilevitv2.py:185-230, :547-602,
:748-817, :858-941, :1170-1255, widths from backbones/configs/mobilevitv2.py:39-105, and decoders/pixelshuffle.py:7-26,
DUC.py:15-21), in the module's registration order -- including ``backbone.classifier``, which the backbone registers
and its forward() never applies (:1440-1444).  The synthetic generator draws in that order exactly like
tools/gen_golden_mobilevitv2.py did when it produced tests/golden/mobilevitv2_05_ps.npz, so the fixture's heat-maps
can be reproduced without the reference.
"""
from collections import OrderedDict

import numpy as np
import torch

from .synth_shufflenet import _bn

MODEL_SIZES = (0.5, 0.75, 1.0)
DECODER_INPLANES = {0.5: 256, 0.75: 384, 1.0: 512}          # pose_mobilevitv2_pixel_shuffle.py:27-32
ATTN_BLOCKS = (2, 4, 3)                                      # layer3 .. layer5 (configs/mobilevitv2.py:73, :84, :95)
N_CLASS = 1000                                               # the unused ImageNet classifier (mobilevitv2.py:1252-1255)


def make_divisible(v, divisor=8, min_value=None):
    """configs/mobilevitv2.py:9-30."""
    min_value = divisor if min_value is None else min_value
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def mobilevitv2_widths(model_size):
    """(stem, layer1, layer2, [(out, attn dim, ffn dim, attn units)] of layers 3-5) for a width multiplier
    (configs/mobilevitv2.py:41-101; the ffn width is 2 x the attention width rounded down to 16, mobilevitv2.py:1004)."""
    m = float(model_size)
    c0 = int(make_divisible(max(16, min(64, 32 * m)), divisor=8, min_value=16))
    c1 = int(make_divisible(64 * m, divisor=16))
    c2 = int(make_divisible(128 * m, divisor=8))
    mit = []
    for out, attn, n in ((256, 128, ATTN_BLOCKS[0]), (384, 192, ATTN_BLOCKS[1]), (512, 256, ATTN_BLOCKS[2])):
        d = int(make_divisible(attn * m, divisor=8))
        mit.append((int(make_divisible(out * m, divisor=8)), d, int(2 * d // 16 * 16), n))
    return c0, c1, c2, mit


def _conv_bn(s, name, cout, cin, k):
    """ConvLayer with a norm (:321-330): block.conv (no bias) + block.norm."""
    s[name + ".block.conv.weight"] = (cout, cin, k, k)
    _bn(s, name + ".block.norm", cout)


def _conv_bias(s, name, cout, cin):
    """ConvLayer(bias=True, use_norm=False): block.conv with bias."""
    s[name + ".block.conv.weight"] = (cout, cin, 1, 1)
    s[name + ".block.conv.bias"] = (cout,)


def _gn(s, name, c):
    s[name + ".weight"] = (c,)
    s[name + ".bias"] = (c,)


def _inverted_residual(s, name, cin, cout, expand=2):
    """InvertedResidual (:201-218)."""
    hid = make_divisible(int(round(cin * expand)), 8)
    _conv_bn(s, name + ".block.exp_1x1", hid, cin, 1)
    _conv_bn(s, name + ".block.conv_3x3", hid, 1, 3)
    _conv_bn(s, name + ".block.red_1x1", cout, hid, 1)


def mobilevitv2_param_shapes(model_size=0.5, num_joints=17, target_type="gaussian", start_channels=256,
                             architecture=(512, 256, 128), final_kernel=1):
    c0, c1, c2, mit = mobilevitv2_widths(model_size)
    s = OrderedDict()
    _conv_bn(s, "backbone.conv_1", c0, 3, 3)
    _inverted_residual(s, "backbone.layer_1.0", c0, c1)
    _inverted_residual(s, "backbone.layer_2.0", c1, c2)
    _inverted_residual(s, "backbone.layer_2.1", c2, c2)
    cin = c2
    for li, (out, d, ffn, n) in enumerate(mit):
        p = "backbone.layer_%d" % (li + 3)
        _inverted_residual(s, p + ".0", cin, out)
        q = p + ".1"                                              # MobileViTBlockv2 (:898-941)
        _conv_bn(s, q + ".local_rep.0", out, 1, 3)
        s[q + ".local_rep.1.block.conv.weight"] = (d, out, 1, 1)
        for u in range(n):                                        # LinearAttnFFN (:779-817)
            g = "%s.global_rep.%d" % (q, u)
            _gn(s, g + ".pre_norm_attn.0", d)
            _conv_bias(s, g + ".pre_norm_attn.1.qkv_proj", 1 + 2 * d, d)
            _conv_bias(s, g + ".pre_norm_attn.1.out_proj", d, d)
            _gn(s, g + ".pre_norm_ffn.0", d)
            _conv_bias(s, g + ".pre_norm_ffn.1", ffn, d)
            _conv_bias(s, g + ".pre_norm_ffn.3", d, ffn)
        _gn(s, "%s.global_rep.%d" % (q, n), d)
        _conv_bn(s, q + ".conv_proj", out, d, 1)
        cin = out
    s["backbone.classifier.1.weight"] = (N_CLASS, cin)
    s["backbone.classifier.1.bias"] = (N_CLASS,)
    s["decoder.conv_compress.weight"] = (start_channels, DECODER_INPLANES[float(model_size)], 1, 1)
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


def synth_mobilevitv2_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """Seeded weights: convs ~ N(0, 2 / fan_in), norm weights ~ U(0.5, 1), biases ~ N(0, 0.05), running statistics
    0 / 1 unless ``calib`` ({key: array}) supplies them; the head is multiplied by ``final_scale``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, shape in mobilevitv2_param_shapes(**kw).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(0, dtype=torch.long)
        elif len(shape) == 4:
            fan = shape[1] * shape[2] * shape[3]
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * np.sqrt(2.0 / fan)).astype(np.float32))
        elif len(shape) == 2:
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * 0.01).astype(np.float32))
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
