"""pose_mobilenetv3_small_pixel_shuffle / pose_mobilenetv3_small restated on stock torch.nn.functional, straight from
a reference-format state_dict.  The backbone is torchvision's ``mobilenet_v3_small().features``; torchvision is not
installed where the tests run, so no fixture of the reference's own module exists: this restatement of the block
table (udp_pose_amd/synth_mobilenetv3.py states it, and its 927 008 backbone parameters) is the arbiter of the GPU
tests, in fp64.  Any input size, any floating dtype.

The structure is read off the KEYS, not off the planner's table: a block's members are walked in order, a member with
``fc1`` is the squeeze-excitation, a [C, 1, k, k] weight is the depthwise conv (its stride is the only thing taken
from ``STRIDES``), the last member is the project conv.  The deconv head also closes the two deconv-head ShuffleNets
(``deconv_head``).
"""
import torch
import torch.nn.functional as F

from shufflenet_ref import _conv
from shufflenet_plus_ref import hswish

BACKBONE_BN_EPS = 1e-3          # torchvision: partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)
HEAD_BN_EPS = 1e-5
STRIDES = (2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1)                 # of backbone.0.1 .. backbone.0.11
HS_FROM = 4                                                  # blocks 1 - 3 use ReLU, 4 - 11 hard-swish


def _bn(sd, name, x, calibrate, eps):
    if calibrate:                                   # the statistics of this very batch become the running ones
        sd[name + ".running_mean"] = x.mean(dim=(0, 2, 3)).to(torch.float32)
        sd[name + ".running_var"] = x.var(dim=(0, 2, 3), unbiased=False).to(torch.float32)
    t = lambda k: sd[name + k].to(x.dtype)
    return F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), False, 0.0, eps)


def squeeze_excitation(sd, name, x):
    """torchvision.ops.SqueezeExcitation: x * hardsigmoid(fc2(relu(fc1(avgpool(x)))))."""
    a = x.mean(dim=(2, 3), keepdim=True)
    a = _conv(sd, name + ".fc2", F.relu(_conv(sd, name + ".fc1", a)))
    return x * (torch.clamp(a + 3, 0, 6) / 6)


def _block(sd, p, x, stride, act, calibrate):
    """InvertedResidual.forward: x + block(x) when stride 1 and in == out."""
    y, m = x, 0
    members = []
    while ("%s.block.%d.0.weight" % (p, m)) in sd or ("%s.block.%d.fc1.weight" % (p, m)) in sd:
        members.append(m)
        m += 1
    for m in members:
        q = "%s.block.%d" % (p, m)
        if (q + ".fc1.weight") in sd:
            y = squeeze_excitation(sd, q, y)
            continue
        w = sd[q + ".0.weight"]
        dw = w.shape[1] == 1 and w.shape[2] > 1
        y = _bn(sd, q + ".1", _conv(sd, q + ".0", y, stride if dw else 1, y.shape[1] if dw else 1), calibrate, BACKBONE_BN_EPS)
        if m != members[-1]:                        # the project conv has no activation
            y = act(y)
    return x + y if stride == 1 and x.shape[1] == y.shape[1] else y


def backbone(sd, x, calibrate=False):
    x = hswish(_bn(sd, "backbone.0.0.1", _conv(sd, "backbone.0.0.0", x, 2), calibrate, BACKBONE_BN_EPS))
    for i, stride in enumerate(STRIDES, start=1):
        x = _block(sd, "backbone.0.%d" % i, x, stride, hswish if i >= HS_FROM else F.relu, calibrate)
    return hswish(_bn(sd, "backbone.0.12.1", _conv(sd, "backbone.0.12.0", x), calibrate, BACKBONE_BN_EPS))


def deconv_head(sd, x, calibrate=False):
    """deconv_layers = [ConvTranspose2d(4, 2, 1), BatchNorm, ReLU] x n (pose_resnet.py:155-193), then final_layer."""
    d = 0
    while ("deconv_layers.%d.weight" % (3 * d)) in sd:
        w = sd["deconv_layers.%d.weight" % (3 * d)].to(x.dtype)
        b = sd.get("deconv_layers.%d.bias" % (3 * d))
        x = F.conv_transpose2d(x, w, None if b is None else b.to(x.dtype), stride=2, padding=1)
        x = F.relu(_bn(sd, "deconv_layers.%d" % (3 * d + 1), x, calibrate, HEAD_BN_EPS))
        d += 1
    return _conv(sd, "final_layer", x)


def ps_head(sd, x, calibrate=False):
    """decoders/pixelshuffle.py:29-31 + DUC.py:23-28, then final_layer."""
    x = _conv(sd, "decoder.conv_compress", x)
    d = 0
    while ("decoder.duc.%d.conv.weight" % d) in sd:
        x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), calibrate, HEAD_BN_EPS)), 2)
        d += 1
    return _conv(sd, "final_layer", x)


def forward(sd, x, calibrate=False, dtype=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W]; the head follows the keys.  ``calibrate``: overwrite every
    BatchNorm's running statistics in ``sd`` with those of this batch."""
    with torch.no_grad():
        x = backbone(sd, x.to(dtype or x.dtype), calibrate)
        return (deconv_head if "deconv_layers.0.weight" in sd else ps_head)(sd, x, calibrate)
