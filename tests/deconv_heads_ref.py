"""pose_shufflenetv2_10x and pose_shufflenetv2_plus (the deconv-head siblings of the ``*_pixel_shuffle`` nets) restated
on stock torch.nn.functional: the backbones of tests/shufflenet_ref.py / tests/shufflenet_plus_ref.py up to ``conv_last``,
then ``deconv_layers`` and ``final_layer`` (pose_shufflenetv2_10x.py:93-97, pose_shufflenetv2_plus.py:95-99).
tests/test_deconv_heads_cpu.py pins both to the heat-maps the reference's own modules produced
(tests/golden/shufflenetv2_10x_deconv.npz, shufflenetv2_plus_small_deconv.npz)."""
import torch
import torch.nn.functional as F

import shufflenet_plus_ref as RP
import shufflenet_ref as R0
from mobilenetv3_ref import deconv_head


def forward_10x(sd, x, calibrate=False, dtype=None):
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = F.relu(R0._bn(sd, "backbone.first_conv.1", R0._conv(sd, "backbone.first_conv.0", x, 2), calibrate))
        x = F.max_pool2d(x, 3, 2, 1)
        i = 0
        while ("backbone.features.%d.branch_main.0.weight" % i) in sd:
            x = R0._unit(sd, "backbone.features.%d" % i, x, calibrate)
            i += 1
        x = F.relu(R0._bn(sd, "backbone.conv_last.1", R0._conv(sd, "backbone.conv_last.0", x), calibrate))
        return deconv_head(sd, x, calibrate)


def forward_plus(sd, x, calibrate=False, dtype=None):
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = RP.hswish(R0._bn(sd, "backbone.first_conv.1", R0._conv(sd, "backbone.first_conv.0", x, 2), calibrate))
        i = 0
        while ("backbone.features.%d.branch_main.0.weight" % i) in sd:
            x = RP._unit(sd, "backbone.features.%d" % i, x, F.relu if i < RP.STAGE_REPEATS[0] else RP.hswish, calibrate)
            i += 1
        x = RP.hswish(R0._bn(sd, "backbone.conv_last.1", R0._conv(sd, "backbone.conv_last.0", x), calibrate))
        return deconv_head(sd, x, calibrate)


FORWARD = {"pose_shufflenetv2_10x": forward_10x, "pose_shufflenetv2_plus": forward_plus}
