"""pose_shufflenetv2_10x_pixel_shuffle weight-file contract + seeded synthetic weights.

Key names / shapes of ``PoseShuffleNetV210xPixelShuffle.state_dict()``
(deep_hrnet/lib/models/pose_shufflenetv2_10x_pixel_shuffle.py:23-53 with backbones/shufflenetv2.py:34-152 and
decoders/pixelshuffle.py:7-26, DUC.py:15-21), in the module's registration order.  The synthetic generator draws in
that order exactly like tools/gen_golden_shufflenet.py did when it produced tests/golden/shufflenetv2_10x_ps.npz, so
the fixture's heat-maps can be reproduced without the reference.
"""
from collections import OrderedDict

import numpy as np
import torch

# ShuffleNetV2.stage_out_channels[1:] (shufflenetv2.py:105-112) and stage_repeats (:103)
STAGE_OUT_CHANNELS = {"0.5x": (24, 48, 96, 192, 1024), "1.0x": (24, 116, 232, 464, 1024), "1.5x": (24, 176, 352, 704, 1024),
                      "2.0x": (24, 244, 488, 976, 2048)}
STAGE_REPEATS = (4, 8, 4)
DECODER_INPLANES = 1024          # pose_shufflenetv2_10x_pixel_shuffle.py:26
N_CLASS = 1000                   # the unused ImageNet classifier the backbone still registers (shufflenetv2.py:151)


def _bn(s, name, c):
    s[name + ".weight"] = (c,)
    s[name + ".bias"] = (c,)
    s[name + ".running_mean"] = (c,)
    s[name + ".running_var"] = (c,)
    s[name + ".num_batches_tracked"] = ()


def shufflenet_units(model_size):
    """[(index, inp, oup, mid, stride)] of ``backbone.features`` (shufflenetv2.py:126-139): ``inp`` is the channel count
    the unit's convs see (all of the input for a stride-2 unit, half of it for a stride-1 unit)."""
    ch = STAGE_OUT_CHANNELS[model_size]
    units, cin, idx = [], ch[0], 0
    for stage, rep in enumerate(STAGE_REPEATS):
        oup = ch[stage + 1]
        for i in range(rep):
            units.append((idx, cin if i == 0 else cin // 2, oup, oup // 2, 2 if i == 0 else 1))
            cin = oup
            idx += 1
    return units


def _backbone_shapes(model_size):
    ch = STAGE_OUT_CHANNELS[model_size]
    s = OrderedDict()
    s["backbone.first_conv.0.weight"] = (ch[0], 3, 3, 3)
    _bn(s, "backbone.first_conv.1", ch[0])
    for idx, inp, oup, mid, stride in shufflenet_units(model_size):
        p = "backbone.features.%d" % idx
        s[p + ".branch_main.0.weight"] = (mid, inp, 1, 1)
        _bn(s, p + ".branch_main.1", mid)
        s[p + ".branch_main.3.weight"] = (mid, 1, 3, 3)
        _bn(s, p + ".branch_main.4", mid)
        s[p + ".branch_main.5.weight"] = (oup - inp, mid, 1, 1)
        _bn(s, p + ".branch_main.6", oup - inp)
        if stride == 2:
            s[p + ".branch_proj.0.weight"] = (inp, 1, 3, 3)
            _bn(s, p + ".branch_proj.1", inp)
            s[p + ".branch_proj.2.weight"] = (inp, inp, 1, 1)
            _bn(s, p + ".branch_proj.3", inp)
    s["backbone.conv_last.0.weight"] = (ch[4], ch[3], 1, 1)
    _bn(s, "backbone.conv_last.1", ch[4])
    s["backbone.classifier.0.weight"] = (N_CLASS, ch[4])
    return s


def shufflenet_param_shapes(model_size="1.0x", num_joints=17, target_type="gaussian", start_channels=256,
                            architecture=(512, 256, 128), final_kernel=1):
    s = _backbone_shapes(model_size)
    s["decoder.conv_compress.weight"] = (start_channels, DECODER_INPLANES, 1, 1)
    cin = start_channels
    for d, planes in enumerate(architecture):
        s["decoder.duc.%d.conv.weight" % d] = (planes, cin, 3, 3)
        _bn(s, "decoder.duc.%d.bn" % d, planes)
        cin = planes // 4
    nout = num_joints * (3 if target_type == "offset" else 1)
    s["final_layer.weight"] = (nout, cin, final_kernel, final_kernel)
    s["final_layer.bias"] = (nout,)
    return s


def _final(s, cin, num_joints, target_type, final_kernel):
    nout = num_joints * (3 if target_type == "offset" else 1)
    s["final_layer.weight"] = (nout, cin, final_kernel, final_kernel)
    s["final_layer.bias"] = (nout,)
    return s


def deconv_head_shapes(s, inplanes, num_joints=17, target_type="gaussian", deconv_filters=(256, 256, 256), final_kernel=1,
                       deconv_with_bias=False):
    """``deconv_layers`` ([ConvTranspose2d(4, 2, 1), BatchNorm, ReLU] x n: indices 3d, 3d + 1) and ``final_layer``
    appended to ``s`` -- the head of pose_resnet that the deconv-head nets repeat."""
    cin = inplanes
    for d, planes in enumerate(deconv_filters):
        s["deconv_layers.%d.weight" % (3 * d)] = (cin, planes, 4, 4)
        if deconv_with_bias:
            s["deconv_layers.%d.bias" % (3 * d)] = (planes,)
        _bn(s, "deconv_layers.%d" % (3 * d + 1), planes)
        cin = planes
    return _final(s, cin, num_joints, target_type, final_kernel)


def shufflenet_deconv_param_shapes(model_size="1.0x", num_joints=17, target_type="gaussian", deconv_filters=(256, 256, 256),
                                   final_kernel=1, deconv_with_bias=False):
    """pose_shufflenetv2_10x (pose_shufflenetv2_10x.py:22-97): the same backbone, the deconv head behind ``conv_last``."""
    return deconv_head_shapes(_backbone_shapes(model_size), DECODER_INPLANES, num_joints, target_type, deconv_filters, final_kernel,
                              deconv_with_bias)


def seeded_state_dict(shapes, seed, calib=None, final_scale=1.0):
    """Seeded weights for a shape table: convs ~ N(0, 2 / fan_in), BatchNorm weight ~ U(0.5, 1), biases ~ N(0, 0.05),
    running statistics 0 / 1 unless ``calib`` ({key: array}) supplies them; the head is multiplied by ``final_scale``.
    (The draws of synth_shufflenet.synth_shufflenet_state_dict, in the table's order.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, shape in shapes.items():
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


def synth_shufflenet_deconv_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """``synth_shufflenet_state_dict`` for pose_shufflenetv2_10x."""
    return seeded_state_dict(shufflenet_deconv_param_shapes(**kw), seed, calib, final_scale)


def synth_shufflenet_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """Seeded weights: convs ~ N(0, 2 / fan_in), BatchNorm weight ~ U(0.5, 1), biases ~ N(0, 0.05), running statistics
    0 / 1 unless ``calib`` ({key: array}) supplies them; the head is multiplied by ``final_scale``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, shape in shufflenet_param_shapes(**kw).items():
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
