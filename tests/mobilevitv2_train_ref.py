"""pose_mobilevitv2_pixel_shuffle in train mode, restated functionally in torch for the training tests -- the train-mode
twin of tests/mobilevitv2_ref.py: the graph of ``nn.Module.train()`` + forward + JointsMSELoss + backward, in whatever
dtype the state_dict has (fp64 for the reference, fp32 for the yardstick of what summation order alone costs).  Runs on
the CPU; nothing here needs a GPU.  tests/test_mobilevitv2_train_cpu.py pins it to one step of the reference's own module
(tests/golden/mobilevitv2_train_step.npz) and, with ``training=False``, to ``mobilevitv2_ref.forward``.

Any MODEL_SIZE (read off the weight shapes), any input size that is a multiple of 64.  The graph is deterministic: the
backbone YAMLs set no ``mitv2.dropout`` / ``ffn_dropout`` / ``attn_dropout``, so every Dropout has p = 0
(backbones/mobilevitv2.py:1340-1357).  BatchNorm uses batch statistics and moves the running ones -- eps 1e-5 (nn.BatchNorm2d's
default; get_normalization_layer :119-120 passes none), momentum 0.1 (``model.normalization.momentum`` of
backbones/configs/mobilevitv2-*.yaml, and the default of :115); GroupNorm(1, C) has no running state.  The MobileViT block
is in the MAP form of mobilevitv2_ref.py (``silu``, ``group_norm1`` and ``linear_attention_core`` are its functions).
Line numbers: deep_hrnet/lib/models/backbones/mobilevitv2.py.
"""
import torch
import torch.nn.functional as F

from mobilevitv2_ref import group_norm1, linear_attention_core, silu
from pose_resnet_train_ref import is_param, joints_mse, make_batch          # noqa: F401  (the same batch and criterion)

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn(sd, name, x, training):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                        training, BN_MOMENTUM if training else 0.0, BN_EPS)


def _conv(sd, name, x, stride=1, groups=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd.get(name + ".bias"), stride=stride, padding=w.shape[2] // 2, groups=groups)


def _cbn(sd, name, x, act, training, stride=1, groups=1):
    """ConvLayer with a norm (:321-345)."""
    y = _bn(sd, name + ".block.norm", _conv(sd, name + ".block.conv", x, stride, groups), training)
    return silu(y) if act else y


def _inverted_residual(sd, p, x, stride, training):
    """InvertedResidual.forward (:226-230)."""
    y = _cbn(sd, p + ".block.exp_1x1", x, True, training)
    y = _cbn(sd, p + ".block.conv_3x3", y, True, training, stride, y.shape[1])
    y = _cbn(sd, p + ".block.red_1x1", y, False, training)
    return x + y if stride == 1 and x.shape[1] == y.shape[1] else y


def _mit_block(sd, q, x, training, probe=None):
    """MobileViTBlockv2.forward_spatial (:1105-1126), map form."""
    t = _cbn(sd, q + ".local_rep.0", x, True, training, 1, x.shape[1])
    t = _conv(sd, q + ".local_rep.1.block.conv", t)
    d = t.shape[1]
    u = 0
    while ("%s.global_rep.%d.pre_norm_attn.0.weight" % (q, u)) in sd:                               # LinearAttnFFN.forward (:839-855)
        g = "%s.global_rep.%d" % (q, u)
        qkv = _conv(sd, g + ".pre_norm_attn.1.qkv_proj.block.conv", group_norm1(sd, g + ".pre_norm_attn.0", t))
        if probe is not None:
            probe.append(qkv[:, 1 + d:].detach())                                                    # the inputs of relu(v)
        a = linear_attention_core(qkv[:, :1], qkv[:, 1:1 + d], qkv[:, 1 + d:])                       # query, key, value (:671-673)
        t = t + _conv(sd, g + ".pre_norm_attn.1.out_proj.block.conv", a)
        f = silu(_conv(sd, g + ".pre_norm_ffn.1.block.conv", group_norm1(sd, g + ".pre_norm_ffn.0", t)))
        t = t + _conv(sd, g + ".pre_norm_ffn.3.block.conv", f)
        u += 1
    t = group_norm1(sd, "%s.global_rep.%d" % (q, u), t)
    return _cbn(sd, q + ".conv_proj", t, False, training)


def forward(sd, x, training=True, probe=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W] in the dtype of ``sd``.  ``training``: batch statistics, and the
    running ones in ``sd`` move in place; otherwise the eval forward of tests/mobilevitv2_ref.py.  ``probe`` (a list)
    collects the inputs of every ReLU -- the attention's values and the decoder's BatchNorm outputs: the only kinks of
    the graph; ``kink_margin`` measures how far the nearest one is from zero."""
    x = _cbn(sd, "backbone.conv_1", x, True, training, 2)                                            # :1198-1206
    x = _inverted_residual(sd, "backbone.layer_1.0", x, 1, training)
    x = _inverted_residual(sd, "backbone.layer_2.0", x, 2, training)
    x = _inverted_residual(sd, "backbone.layer_2.1", x, 1, training)
    for layer in (3, 4, 5):                                                                          # :1313-1366
        x = _inverted_residual(sd, "backbone.layer_%d.0" % layer, x, 2, training)
        x = _mit_block(sd, "backbone.layer_%d.1" % layer, x, training, probe)
    x = _conv(sd, "decoder.conv_compress", x)                                                        # pixelshuffle.py:29
    d = 0
    while ("decoder.duc.%d.conv.weight" % d) in sd:                                                  # DUC.py:23-28
        x = _bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), training)
        if probe is not None:
            probe.append(x.detach())
        x = F.pixel_shuffle(F.relu(x), 2)
        d += 1
    return _conv(sd, "final_layer", x)                                                               # :59


def kink_margin(sd, x):
    """How far the nearest ReLU input of a train-mode forward lies from zero, in units of what fp32 costs there: per
    ReLU-input tensor the smallest |value| of the fp64 run over the RMS difference between torch's fp32 CPU run and the
    fp64 run of that tensor; the smallest such ratio.  An fp32 evaluation whose rounding puts a ReLU input on the other
    side of zero moves one channel's gradients by percents and everything upstream follows
    (tools/gen_golden_shufflenet_train.py), whichever evaluator it is, so a batch can carry a gradient comparison against
    fp64 only where this ratio is large enough.  Both numbers are the reference's own; nothing here runs the code under test."""
    runs = []
    for dtype in (torch.float64, torch.float32):
        probe = []
        with torch.no_grad():
            forward({k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}, x.to(dtype),
                    training=True, probe=probe)
        runs.append(probe)
    return min(float(a.abs().min()) / float((b.double() - a).pow(2).mean().sqrt()) for a, b in zip(*runs))


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
