"""The two MobileNetV3-small pose nets (pose_mobilenetv3_small_pixel_shuffle, pose_mobilenetv3_small) in train mode,
restated functionally in torch for the training tests -- the train-mode twin of tests/mobilenetv3_ref.py: the graph of
``nn.Module.train()`` + forward + JointsMSELoss + backward, in whatever dtype the state_dict has (fp64 for the reference,
fp32 for the yardstick of what summation order alone costs).  Runs on the CPU; nothing here needs a GPU.

The backbone is torchvision's ``mobilenet_v3_small().features``; torchvision is not installed where the tests run, so no
fixture of the reference's own module can exist.  tests/test_mobilenetv3_train_cpu.py pins this restatement instead to
``mobilenetv3_ref.forward`` (``training=False``) and to an ``nn.Module`` mirror built from stock layers (nn.Hardswish,
nn.Hardsigmoid, nn.BatchNorm2d(eps=1e-3, momentum=0.01)) under autograd.

Like mobilenetv3_ref.py the structure is read off the KEYS: a block's members are walked in order, a member with ``fc1``
is the squeeze-excitation, a [C, 1, k, k] weight is the depthwise conv (its stride is the only thing taken from
``STRIDES``), the last member is the project conv; the head follows the keys.  Backbone BatchNorms: eps 1e-3, momentum
0.01 (torchvision's ``partial(nn.BatchNorm2d, eps=0.001, momentum=0.01)``); the heads': 1e-5 / 0.1.
"""
import torch
import torch.nn.functional as F

from mobilenetv3_ref import BACKBONE_BN_EPS, HEAD_BN_EPS, HS_FROM, STRIDES
from pose_resnet_train_ref import is_param, joints_mse, make_batch          # noqa: F401  (the same batch and criterion)
from shufflenet_plus_ref import hswish

BACKBONE_BN = (BACKBONE_BN_EPS, 0.01)          # (eps, momentum)
HEAD_BN = (HEAD_BN_EPS, 0.1)


def _bn(sd, name, x, training, eps_momentum):
    eps, momentum = eps_momentum
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        training, momentum if training else 0.0, eps)


def _conv(sd, name, x, stride=1, groups=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd.get(name + ".bias"), stride=stride, padding=w.shape[2] // 2, groups=groups)


def squeeze_excitation(sd, name, x):
    """torchvision.ops.SqueezeExcitation: x * hardsigmoid(fc2(relu(fc1(avgpool(x)))))."""
    a = x.mean(dim=(2, 3), keepdim=True)
    a = _conv(sd, name + ".fc2", F.relu(_conv(sd, name + ".fc1", a)))
    return x * (torch.clamp(a + 3, 0, 6) / 6)


def _block(sd, p, x, stride, act, training):
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
        y = _bn(sd, q + ".1", _conv(sd, q + ".0", y, stride if dw else 1, y.shape[1] if dw else 1), training, BACKBONE_BN)
        if m != members[-1]:                        # the project conv has no activation
            y = act(y)
    return x + y if stride == 1 and x.shape[1] == y.shape[1] else y


def forward(sd, x, training=True):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W] in the dtype of ``sd``.  ``training``: batch statistics, and the
    running ones in ``sd`` move in place; otherwise the eval forward of tests/mobilenetv3_ref.py."""
    x = hswish(_bn(sd, "backbone.0.0.1", _conv(sd, "backbone.0.0.0", x, 2), training, BACKBONE_BN))
    for i, stride in enumerate(STRIDES, start=1):
        x = _block(sd, "backbone.0.%d" % i, x, stride, hswish if i >= HS_FROM else F.relu, training)
    x = hswish(_bn(sd, "backbone.0.12.1", _conv(sd, "backbone.0.12.0", x), training, BACKBONE_BN))
    if "decoder.conv_compress.weight" in sd:
        x = _conv(sd, "decoder.conv_compress", x)                                                      # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                               # DUC.py:23-28
            x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), training, HEAD_BN)), 2)
            d += 1
    else:
        d = 0
        while ("deconv_layers.%d.weight" % (3 * d)) in sd:                                            # pose_resnet.py:155-193
            q = "deconv_layers.%d" % (3 * d)
            x = F.conv_transpose2d(x, sd[q + ".weight"], sd.get(q + ".bias"), stride=2, padding=1)
            x = F.relu(_bn(sd, "deconv_layers.%d" % (3 * d + 1), x, training, HEAD_BN))
            d += 1
    return _conv(sd, "final_layer", x)


def loss_and_grads(sd, x, target, target_weight, dtype, criterion=joints_mse):
    """(loss, heat-maps, {parameter: gradient}, state_dict after the step's running-statistics update), all ``dtype``."""
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = [k for k in sd if is_param(k)]
    for k in keys:
        sd[k].requires_grad_(True)
    y = forward(sd, x.to(dtype), training=True)
    loss = criterion(y, target.to(dtype), target_weight.to(dtype))
    gs = torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)
    gs = [torch.zeros_like(sd[k]) if g is None else g for k, g in zip(keys, gs)]
    return float(loss.detach()), y.detach(), dict(zip(keys, gs)), {k: v.detach() for k, v in sd.items()}
