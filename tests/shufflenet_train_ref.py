"""The two ShuffleNetV2 pose nets (pose_shufflenetv2_10x_pixel_shuffle, pose_shufflenetv2_10x) in train mode, restated
functionally in torch for the training tests -- the train-mode twin of tests/shufflenet_ref.py: the graph of
``nn.Module.train()`` + forward + JointsMSELoss + backward, in whatever dtype the state_dict has (fp64 for the reference,
fp32 for the yardstick of what summation order alone costs).  Runs on the CPU; nothing here needs a GPU.
tests/test_shufflenet_train_cpu.py pins it to one step of the reference's own module
(tests/golden/shufflenet_train_step.npz) and, with ``training=False``, to ``shufflenet_ref.forward``.

Any MODEL_SIZE (read off the weight shapes); the head is read off the keys (``decoder.*`` or ``deconv_layers.*``).
BatchNorm uses batch statistics and moves the running ones (momentum 0.1, unbiased variance), as nn.BatchNorm2d does.
Line numbers: deep_hrnet/lib/models/backbones/shufflenetv2.py.
"""
import torch
import torch.nn.functional as F

from pose_resnet_train_ref import is_param, joints_mse, make_batch          # noqa: F401  (the same batch and criterion)

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _relu(x, probe):
    """ReLU; ``probe`` (a list) collects its inputs -- the fixture tool measures how far each is from the kink."""
    if probe is not None:
        probe.append(x.detach())
    return F.relu(x)


def _bn(sd, name, x, training):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        training, BN_MOMENTUM if training else 0.0, BN_EPS)


def _conv(sd, name, x, stride=1, groups=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd.get(name + ".bias"), stride=stride, padding=w.shape[2] // 2, groups=groups)


def _unit(sd, p, x, training, probe=None):
    """ShuffleV2Block.forward (:77-92)."""
    stride2 = (p + ".branch_proj.0.weight") in sd
    if stride2:                                     # :81-84
        proj = _bn(sd, p + ".branch_proj.1", _conv(sd, p + ".branch_proj.0", x, 2, x.shape[1]), training)            # dw (:66-67)
        proj = _relu(_bn(sd, p + ".branch_proj.3", _conv(sd, p + ".branch_proj.2", proj), training), probe)               # pw (:69-71)
        main = x
    else:                                           # channel_shuffle (:86-92): even channels pass, odd ones go on
        proj, main = x[:, 0::2], x[:, 1::2]
    m = _relu(_bn(sd, p + ".branch_main.1", _conv(sd, p + ".branch_main.0", main), training), probe)                      # pw (:50-52)
    m = _bn(sd, p + ".branch_main.4", _conv(sd, p + ".branch_main.3", m, 2 if stride2 else 1, m.shape[1]), training)  # dw (:54-55)
    m = _relu(_bn(sd, p + ".branch_main.6", _conv(sd, p + ".branch_main.5", m), training), probe)                         # pw-linear (:57-59)
    return torch.cat((proj, m), 1)


def forward(sd, x, training=True, probe=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W] in the dtype of ``sd``.  ``training``: batch statistics, and the
    running ones in ``sd`` move in place; otherwise the eval forward of tests/shufflenet_ref.py."""
    x = _relu(_bn(sd, "backbone.first_conv.1", _conv(sd, "backbone.first_conv.0", x, 2), training), probe)                # :118-122
    x = F.max_pool2d(x, 3, 2, 1)                                                                                   # :124
    i = 0
    while ("backbone.features.%d.branch_main.0.weight" % i) in sd:                                                # :157
        x = _unit(sd, "backbone.features.%d" % i, x, training, probe)
        i += 1
    x = _relu(_bn(sd, "backbone.conv_last.1", _conv(sd, "backbone.conv_last.0", x), training), probe)                     # :143-147
    if "decoder.conv_compress.weight" in sd:
        x = _conv(sd, "decoder.conv_compress", x)                                                                  # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                                           # DUC.py:23-28
            x = F.pixel_shuffle(_relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), training), probe), 2)
            d += 1
    else:
        d = 0
        while ("deconv_layers.%d.weight" % (3 * d)) in sd:                                                        # pose_shufflenetv2_10x.py:53-90
            q = "deconv_layers.%d" % (3 * d)
            x = F.conv_transpose2d(x, sd[q + ".weight"], sd.get(q + ".bias"), stride=2, padding=1)
            x = _relu(_bn(sd, "deconv_layers.%d" % (3 * d + 1), x, training), probe)
            d += 1
    return _conv(sd, "final_layer", x)


def joints_mse_offset(y, target, target_weight):
    """JointsMSELoss_offset with use_target_weight: (L_hm, L_os) summed -- what function.train back-propagates."""
    from oracle.train import joints_mse_loss_offset_t
    l_hm, l_os = joints_mse_loss_offset_t(y, target, target_weight)
    return l_hm + l_os


def loss_and_grads(sd, x, target, target_weight, dtype, criterion=joints_mse):
    """(loss, heat-maps, {parameter: gradient}, state_dict after the step's running-statistics update), all ``dtype``.
    A parameter the graph does not reach (the backbone's unused classifier) has a zero gradient."""
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = [k for k in sd if is_param(k)]
    for k in keys:
        sd[k].requires_grad_(True)
    y = forward(sd, x.to(dtype), training=True)
    loss = criterion(y, target.to(dtype), target_weight.to(dtype))
    gs = torch.autograd.grad(loss, [sd[k] for k in keys], allow_unused=True)
    gs = [torch.zeros_like(sd[k]) if g is None else g for k, g in zip(keys, gs)]
    return float(loss.detach()), y.detach(), dict(zip(keys, gs)), {k: v.detach() for k, v in sd.items()}
