"""pose_shufflenetv2_10x_pixel_shuffle restated on stock torch.nn.functional, straight from a reference-format state_dict:
the reference module does not exist where the GPU tests run.  Any MODEL_SIZE (read off the weight shapes), any input
size, any floating dtype (the GPU tests use fp64).  tests/test_shufflenet_cpu.py pins it to the heat-maps the
reference's own module produced (tests/golden/shufflenetv2_10x_ps.npz).

Line numbers: deep_hrnet/lib/models/backbones/shufflenetv2.py (backbone), decoders/pixelshuffle.py + DUC.py (decoder),
pose_shufflenetv2_10x_pixel_shuffle.py (head).
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def _bn(sd, name, x, calibrate):
    if calibrate:                                   # the statistics of this very batch become the running ones
        sd[name + ".running_mean"] = x.mean(dim=(0, 2, 3)).to(torch.float32)
        sd[name + ".running_var"] = x.var(dim=(0, 2, 3), unbiased=False).to(torch.float32)
    t = lambda k: sd[name + k].to(x.dtype)
    return F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), False, 0.0, BN_EPS)


def _conv(sd, name, x, stride=1, groups=1):
    w = sd[name + ".weight"].to(x.dtype)
    b = sd.get(name + ".bias")
    return F.conv2d(x, w, None if b is None else b.to(x.dtype), stride=stride, padding=w.shape[2] // 2, groups=groups)


def _unit(sd, p, x, calibrate):
    """ShuffleV2Block.forward (shufflenetv2.py:77-92)."""
    stride2 = (p + ".branch_proj.0.weight") in sd
    if stride2:                                     # :81-84
        proj = _bn(sd, p + ".branch_proj.1", _conv(sd, p + ".branch_proj.0", x, 2, x.shape[1]), calibrate)          # dw (:66-67)
        proj = F.relu(_bn(sd, p + ".branch_proj.3", _conv(sd, p + ".branch_proj.2", proj), calibrate))             # pw (:69-71)
        main = x
    else:                                           # channel_shuffle (:86-92): even channels pass, odd ones go on
        proj, main = x[:, 0::2], x[:, 1::2]
    m = F.relu(_bn(sd, p + ".branch_main.1", _conv(sd, p + ".branch_main.0", main), calibrate))                    # pw (:50-52)
    m = _bn(sd, p + ".branch_main.4", _conv(sd, p + ".branch_main.3", m, 2 if stride2 else 1, m.shape[1]), calibrate)   # dw (:54-55)
    m = F.relu(_bn(sd, p + ".branch_main.6", _conv(sd, p + ".branch_main.5", m), calibrate))                       # pw-linear (:57-59)
    return torch.cat((proj, m), 1)


def forward(sd, x, calibrate=False, dtype=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W].  ``calibrate``: overwrite every BatchNorm's running statistics in
    ``sd`` with those of this batch (seeded random weights then neither die nor blow up)."""
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = F.relu(_bn(sd, "backbone.first_conv.1", _conv(sd, "backbone.first_conv.0", x, 2), calibrate))          # :118-122
        x = F.max_pool2d(x, 3, 2, 1)                                                                              # :124
        i = 0
        while ("backbone.features.%d.branch_main.0.weight" % i) in sd:                                           # :157
            x = _unit(sd, "backbone.features.%d" % i, x, calibrate)
            i += 1
        x = F.relu(_bn(sd, "backbone.conv_last.1", _conv(sd, "backbone.conv_last.0", x), calibrate))               # :143-147
        x = _conv(sd, "decoder.conv_compress", x)                                                                 # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                                          # DUC.py:23-28
            x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), calibrate)), 2)
            d += 1
        return _conv(sd, "final_layer", x)                                                                        # :52
