"""pose_shufflenetv2_plus_pixel_shuffle weight-file contract + seeded synthetic weights.

Key names / shapes of ``PoseShuffleNetV2PlusPixelShuffle.state_dict()``
(deep_hrnet/lib/models/pose_shufflenetv2_plus_pixel_shuffle.py:23-55 with backbones/shufflenetv2_plus.py:34-316 and
decoders/pixelshuffle.py:7-26, DUC.py:15-21), in the module's registration order -- including ``LastSE``, ``fc`` and
``classifier``, which the backbone registers and its forward() never applies (:324-331).  The synthetic generator draws
in that order exactly like tools/gen_golden_shufflenet_plus.py did when it produced
tests/golden/shufflenetv2_plus_small_ps.npz, so the fixture's heat-maps can be reproduced without the reference.
"""
from collections import OrderedDict

import numpy as np
import torch

from .synth_shufflenet import _bn, deconv_head_shapes, seeded_state_dict

# ShuffleNetV2_Plus.stage_out_channels[1:] (shufflenetv2_plus.py:247-252) and stage_repeats (:246)
STAGE_OUT_CHANNELS = {"Small": (16, 36, 104, 208, 416, 1280), "Medium": (16, 48, 128, 256, 512, 1280),
                      "Large": (16, 68, 168, 336, 672, 1280)}
STAGE_REPEATS = (4, 4, 8, 4)
# get_shufflenetv2_plus (:360): per unit 0 / 1 / 2 = Shufflenet with a 3x3 / 5x5 / 7x7 depthwise conv, 3 = Shuffle_Xception
ARCHITECTURE = (0, 0, 3, 1, 1, 1, 0, 0, 2, 0, 2, 1, 1, 0, 2, 0, 2, 1, 3, 2)
DECODER_INPLANES = 1280          # pose_shufflenetv2_plus_pixel_shuffle.py:26
N_CLASS = 1000                   # the unused ImageNet classifier (:316)


def shufflenet_plus_units(model_size):
    """[(index, inp, oup, mid, stride, block, act, se)] of ``backbone.features`` (shufflenetv2_plus.py:267-300).
    ``inp``: the channels the unit's convs see (all of the input for a stride-2 unit, half of it for a stride-1
    unit); ``block``: the ARCHITECTURE code; ``act``: "relu" in stage 0, "hs" after it (:271); ``se``: stages 2, 3 (:272)."""
    ch = STAGE_OUT_CHANNELS[model_size]
    units, cin, idx = [], ch[0], 0
    for stage, rep in enumerate(STAGE_REPEATS):
        oup = ch[stage + 1]
        for i in range(rep):
            units.append((idx, cin if i == 0 else cin // 2, oup, oup // 2, 2 if i == 0 else 1, ARCHITECTURE[idx],
                          "hs" if stage >= 1 else "relu", stage >= 2))
            cin = oup
            idx += 1
    return units


def _se(s, name, c):
    """SELayer (:34-46): SE_opr = [pool, conv C -> C/4, BatchNorm, ReLU, conv C/4 -> C]."""
    s[name + ".SE_opr.1.weight"] = (c // 4, c, 1, 1)
    _bn(s, name + ".SE_opr.2", c // 4)
    s[name + ".SE_opr.4.weight"] = (c, c // 4, 1, 1)


def _backbone_shapes(model_size):
    ch = STAGE_OUT_CHANNELS[model_size]
    s = OrderedDict()
    s["backbone.first_conv.0.weight"] = (ch[0], 3, 3, 3)
    _bn(s, "backbone.first_conv.1", ch[0])
    for idx, inp, oup, mid, stride, block, act, se in shufflenet_plus_units(model_size):
        p = "backbone.features.%d" % idx
        out = oup - inp
        if block == 3:                   # Shuffle_Xception (:158-196): 3 x (dw 3x3 + BN, pw + BN + act)
            chain = [(inp, inp), (mid, mid), (mid, out)]
            for k, (ci, co) in enumerate(chain):
                s[p + ".branch_main.%d.weight" % (5 * k)] = (ci, 1, 3, 3)
                _bn(s, p + ".branch_main.%d" % (5 * k + 1), ci)
                s[p + ".branch_main.%d.weight" % (5 * k + 2)] = (co, ci, 1, 1)
                _bn(s, p + ".branch_main.%d" % (5 * k + 3), co)
            if se:
                _se(s, p + ".branch_main.15", out)
            ks = 3
        else:                            # Shufflenet (:91-114): pw + BN + act, dw k x k + BN, pw + BN + act
            ks = 3 + 2 * block
            s[p + ".branch_main.0.weight"] = (mid, inp, 1, 1)
            _bn(s, p + ".branch_main.1", mid)
            s[p + ".branch_main.3.weight"] = (mid, 1, ks, ks)
            _bn(s, p + ".branch_main.4", mid)
            s[p + ".branch_main.5.weight"] = (out, mid, 1, 1)
            _bn(s, p + ".branch_main.6", out)
            if se:
                _se(s, p + ".branch_main.8", out)
        if stride == 2:                  # (:117-130, :199-212)
            s[p + ".branch_proj.0.weight"] = (inp, 1, ks, ks)
            _bn(s, p + ".branch_proj.1", inp)
            s[p + ".branch_proj.2.weight"] = (inp, inp, 1, 1)
            _bn(s, p + ".branch_proj.3", inp)
    s["backbone.conv_last.0.weight"] = (ch[5], ch[4], 1, 1)
    _bn(s, "backbone.conv_last.1", ch[5])
    _se(s, "backbone.LastSE", ch[5])
    s["backbone.fc.0.weight"] = (ch[5], ch[5])
    s["backbone.classifier.0.weight"] = (N_CLASS, ch[5])
    return s


def shufflenet_plus_deconv_param_shapes(model_size="Small", num_joints=17, target_type="gaussian", deconv_filters=(256, 256, 256),
                                        final_kernel=1, deconv_with_bias=False):
    """pose_shufflenetv2_plus (pose_shufflenetv2_plus.py:22-99): the same backbone, the deconv head behind ``conv_last``."""
    return deconv_head_shapes(_backbone_shapes(model_size), DECODER_INPLANES, num_joints, target_type, deconv_filters, final_kernel,
                              deconv_with_bias)


def synth_shufflenet_plus_deconv_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """``synth_shufflenet_plus_state_dict`` for pose_shufflenetv2_plus."""
    return seeded_state_dict(shufflenet_plus_deconv_param_shapes(**kw), seed, calib, final_scale)


def shufflenet_plus_param_shapes(model_size="Small", num_joints=17, target_type="gaussian", start_channels=256,
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


def unused_keys(shapes):
    """Keys the reference's forward() never applies: the ImageNet tail and the BatchNorm step counters."""
    return {k for k in shapes if k.startswith(("backbone.LastSE.", "backbone.fc.", "backbone.classifier."))
            or k.endswith("num_batches_tracked")}


def synth_shufflenet_plus_state_dict(seed=7, calib=None, final_scale=1.0, **kw):
    """Seeded weights: convs ~ N(0, 2 / fan_in), BatchNorm weight ~ U(0.5, 1), biases ~ N(0, 0.05), running statistics
    0 / 1 unless ``calib`` ({key: array}) supplies them; the head is multiplied by ``final_scale``."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, shape in shufflenet_plus_param_shapes(**kw).items():
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
