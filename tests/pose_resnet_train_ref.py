"""pose_resnet (SimpleBaseline) in train mode, restated functionally in torch for the training tests: the graph of
``nn.Module.train()`` + forward + JointsMSELoss + backward, in whatever dtype the state_dict has (fp64 for the
reference, fp32 for the yardstick of what summation order alone costs).  Runs on the CPU; nothing here needs a GPU.

Graph: conv 7x7 s2 -> BN -> ReLU -> max-pool 3x3 s2 -> four stages of Bottlenecks (1x1, 3x3 carrying the stride, 1x1 x4,
projection shortcut on the first block of a stage) -> 3 x [ConvTranspose2d(4, 2, 1) -> BN -> ReLU] -> final conv with bias.
BatchNorm uses batch statistics and moves the running ones (momentum 0.1, unbiased variance), as nn.BatchNorm2d does.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


def _bn(sd, x, name, relu=True, res=None):
    y = F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"],
                     training=True, momentum=BN_MOMENTUM, eps=BN_EPS)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def forward_train(sd, x, layers, n_deconv=3):
    """Train-mode forward; the running statistics in ``sd`` are updated in place."""
    x = _bn(sd, F.conv2d(x, sd["conv1.weight"], None, stride=2, padding=3), "bn1")
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    for li, nblk in enumerate(layers, start=1):
        for b in range(nblk):
            p = "layer%d.%d" % (li, b)
            s = 2 if (li > 1 and b == 0) else 1
            t = _bn(sd, F.conv2d(x, sd[p + ".conv1.weight"]), p + ".bn1")
            t = _bn(sd, F.conv2d(t, sd[p + ".conv2.weight"], None, stride=s, padding=1), p + ".bn2")
            r = x
            if (p + ".downsample.0.weight") in sd:
                r = _bn(sd, F.conv2d(x, sd[p + ".downsample.0.weight"], None, stride=s), p + ".downsample.1", relu=False)
            x = _bn(sd, F.conv2d(t, sd[p + ".conv3.weight"]), p + ".bn3", res=r)
    for d in range(n_deconv):
        q = "deconv_layers.%d" % (3 * d)
        x = F.conv_transpose2d(x, sd[q + ".weight"], sd.get(q + ".bias"), stride=2, padding=1)
        x = _bn(sd, x, "deconv_layers.%d" % (3 * d + 1))
    w = sd["final_layer.weight"]
    return F.conv2d(x, w, sd["final_layer.bias"], padding=w.shape[2] // 2)


def joints_mse(y, target, target_weight):
    """JointsMSELoss with use_target_weight: the mean over joints of 0.5 * MSE(pred * w, gt * w)."""
    b, j = y.shape[:2]
    w = target_weight.reshape(b, j, 1)
    d = (y.reshape(b, j, -1) - target.reshape(b, j, -1)) * w
    return 0.5 * (d ** 2).mean(dim=(0, 2)).sum() / j


def loss_and_grads(sd, x, target, target_weight, layers, dtype):
    """(loss, heat-maps, {parameter: gradient}, state_dict after the step's running-statistics update), all ``dtype``."""
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = [k for k in sd if is_param(k)]
    for k in keys:
        sd[k].requires_grad_(True)
    y = forward_train(sd, x.to(dtype), layers)
    loss = joints_mse(y, target.to(dtype), target_weight.to(dtype))
    gs = torch.autograd.grad(loss, [sd[k] for k in keys])
    return float(loss.detach()), y.detach(), dict(zip(keys, gs)), {k: v.detach() for k, v in sd.items()}


def make_batch(n, joints, h, w, seed):
    """Images ~ N(0, 1), gaussian heat-map targets (sigma 2) at seeded joint positions, weights in {0, 1, 0.5}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = torch.from_numpy(rng.standard_normal((n, 3, h, w)).astype(np.float32))
    hh, hw = h // 4, w // 4
    cy = rng.uniform(2, hh - 2, (n, joints, 1, 1))
    cx = rng.uniform(2, hw - 2, (n, joints, 1, 1))
    yy, xx = np.mgrid[0:hh, 0:hw]
    tg = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.0 ** 2)).astype(np.float32)
    tw = rng.choice(np.array([0.0, 1.0, 1.0, 0.5], np.float32), (n, joints, 1))
    return x, torch.from_numpy(tg), torch.from_numpy(tw)
