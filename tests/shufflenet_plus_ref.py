"""pose_shufflenetv2_plus_pixel_shuffle restated on stock torch.nn.functional, straight from a reference-format
state_dict: the reference module does not exist where the GPU tests run.  Any MODEL_SIZE (read off the weight shapes),
any input size, any floating dtype (the GPU tests use fp64).  tests/test_shufflenet_plus_cpu.py pins it to the
heat-maps the reference's own module produced (tests/golden/shufflenetv2_plus_small_ps.npz).

Line numbers: deep_hrnet/lib/models/backbones/shufflenetv2_plus.py (backbone), decoders/pixelshuffle.py + DUC.py
(decoder), pose_shufflenetv2_plus_pixel_shuffle.py (head).
"""
import torch
import torch.nn.functional as F

from shufflenet_ref import _bn, _conv

STAGE_REPEATS = (4, 4, 8, 4)                                                     # :246


def hswish(x):
    """HS (:63-70)."""
    return x * (torch.clamp(x + 3, 0, 6) / 6)


def se_layer(sd, name, x, calibrate=False):
    """SELayer (:34-60): x * clamp(W2 relu(BN(W1 mean(x))) + 3, 0, 6) / 6."""
    a = x.mean(dim=(2, 3), keepdim=True)
    a = F.relu(_bn(sd, name + ".SE_opr.2", _conv(sd, name + ".SE_opr.1", a), calibrate))
    a = _conv(sd, name + ".SE_opr.4", a)
    return x * (torch.clamp(a + 3, 0, 6) / 6)


def _dwbn(sd, p, conv, bn, x, stride, calibrate):
    return _bn(sd, "%s.%d" % (p, bn), _conv(sd, "%s.%d" % (p, conv), x, stride, x.shape[1]), calibrate)


def _pwbn(sd, p, conv, bn, x, act, calibrate):
    return act(_bn(sd, "%s.%d" % (p, bn), _conv(sd, "%s.%d" % (p, conv), x), calibrate))


def _unit(sd, p, x, act, calibrate):
    """Shufflenet.forward (:134-141) / Shuffle_Xception.forward (:214-221)."""
    stride2 = (p + ".branch_proj.0.weight") in sd
    s = 2 if stride2 else 1
    if stride2:                                     # :117-130
        proj = _pwbn(sd, p + ".branch_proj", 2, 3, _dwbn(sd, p + ".branch_proj", 0, 1, x, 2, calibrate), act, calibrate)
        main = x
    else:                                           # channel_shuffle (:224-230): even channels pass, odd ones go on
        proj, main = x[:, 0::2], x[:, 1::2]
    m, q = main, p + ".branch_main"
    if sd[q + ".0.weight"].shape[1] == 1:           # Shuffle_Xception (:158-180): it opens with a depthwise conv
        for k in range(3):
            m = _pwbn(sd, q, 5 * k + 2, 5 * k + 3, _dwbn(sd, q, 5 * k, 5 * k + 1, m, s, calibrate), act, calibrate)
        se = q + ".15"
    else:                                           # Shufflenet (:91-103)
        m = _pwbn(sd, q, 0, 1, m, act, calibrate)
        m = _pwbn(sd, q, 5, 6, _dwbn(sd, q, 3, 4, m, s, calibrate), act, calibrate)
        se = q + ".8"
    if (se + ".SE_opr.1.weight") in sd:             # :112-113, :192-194
        m = se_layer(sd, se, m, calibrate)
    return torch.cat((proj, m), 1)


def forward(sd, x, calibrate=False, dtype=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W].  ``calibrate``: overwrite every BatchNorm's running statistics in
    ``sd`` with those of this batch (seeded random weights then neither die nor blow up)."""
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = hswish(_bn(sd, "backbone.first_conv.1", _conv(sd, "backbone.first_conv.0", x, 2), calibrate))         # :259-263
        i = 0
        while ("backbone.features.%d.branch_main.0.weight" % i) in sd:                                           # :321
            act = F.relu if i < STAGE_REPEATS[0] else hswish                                                     # :271
            x = _unit(sd, "backbone.features.%d" % i, x, act, calibrate)
            i += 1
        x = hswish(_bn(sd, "backbone.conv_last.1", _conv(sd, "backbone.conv_last.0", x), calibrate))              # :304-308
        x = _conv(sd, "decoder.conv_compress", x)                                                                 # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                                          # DUC.py:23-28
            x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), calibrate)), 2)
            d += 1
        return _conv(sd, "final_layer", x)                                                                        # :54
