"""pose_resnet_psa (ResNet-18 / 34) restated on stock torch.nn.functional, straight from a reference-format state_dict:
the reference module does not exist where the GPU tests run.  Any BasicBlock depth (read off the keys), any input size
that is a multiple of 32, any floating dtype (the GPU tests use fp64).  tests/test_resnet_psa_cpu.py pins it to the
heat-maps the reference's own module produced (tests/golden/resnet18_psa.npz).

Line numbers: deep_hrnet/lib/models/pose_resnet_psa.py (net), PSA.py (attention).
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
LN_EPS = 1e-5


def _bn(sd, name, x, calibrate=False):
    """nn.BatchNorm2d in eval mode.  ``calibrate``: first set the running statistics in ``sd`` to this batch's (the
    unbiased variance, as one training step with momentum None leaves them)."""
    if calibrate:
        xs = x.detach().double()
        sd[name + ".running_mean"] = xs.mean(dim=(0, 2, 3)).to(torch.float32)
        sd[name + ".running_var"] = xs.transpose(0, 1).reshape(x.shape[1], -1).var(dim=1, unbiased=True).to(torch.float32)
    d = x.dtype
    return F.batch_norm(x, sd[name + ".running_mean"].to(d), sd[name + ".running_var"].to(d), sd[name + ".weight"].to(d),
                        sd[name + ".bias"].to(d), False, 0.0, BN_EPS)


def _conv(sd, name, x, stride=1):
    w = sd[name + ".weight"].to(x.dtype)
    b = sd.get(name + ".bias")
    return F.conv2d(x, w, None if b is None else b.to(x.dtype), stride=stride, padding=w.shape[2] // 2)


def psa_s(sd, p, x):
    """PSA_s.forward (PSA.py:191-269): spatial_pool (the channel mask), then channel_pool (the spatial gate) of its
    result."""
    d = x.dtype
    n, c, h, w = x.shape
    # spatial_pool (:191-223)
    v = _conv(sd, p + ".conv_v_right", x).reshape(n, c // 2, h * w)
    q = torch.softmax(_conv(sd, p + ".conv_q_right", x).reshape(n, 1, h * w), dim=2)
    ctx = torch.matmul(v, q.transpose(1, 2)).unsqueeze(-1)                             # [N, C/2, 1, 1]
    t = _conv(sd, p + ".conv_up.0", ctx)
    t = F.layer_norm(t, [c // 8, 1, 1], sd[p + ".conv_up.1.weight"].to(d), sd[p + ".conv_up.1.bias"].to(d), LN_EPS)
    x = x * torch.sigmoid(_conv(sd, p + ".conv_up.3", F.relu(t)))
    # channel_pool (:225-257)
    g = _conv(sd, p + ".conv_q_left", x).mean(dim=(2, 3)).reshape(n, 1, c // 2)
    theta = torch.softmax(_conv(sd, p + ".conv_v_left", x).reshape(n, c // 2, h * w), dim=2)
    return x * torch.sigmoid(torch.matmul(g, theta).reshape(n, 1, h, w))


def basic_block(sd, p, x, stride, calibrate=False):
    """BasicBlock.forward (pose_resnet_psa.py:45-61)."""
    out = F.relu(_bn(sd, p + ".bn1", _conv(sd, p + ".conv1", x, stride), calibrate))
    out = psa_s(sd, p + ".deattn", out)
    out = _bn(sd, p + ".bn2", _conv(sd, p + ".conv2", out), calibrate)
    if (p + ".downsample.0.weight") in sd:
        x = _bn(sd, p + ".downsample.1", _conv(sd, p + ".downsample.0", x, stride), calibrate)
    return F.relu(out + x)


def forward(sd, x, dtype=torch.float64, calibrate=False):
    """PoseResNet.forward (pose_resnet_psa.py:195-209) -> heat-maps [N, J, H/4, W/4] in ``dtype``."""
    x = x.to(dtype)
    with torch.no_grad():
        x = F.relu(_bn(sd, "bn1", _conv(sd, "conv1", x, 2), calibrate))
        x = F.max_pool2d(x, 3, 2, 1)
        for li in range(1, 5):
            k = 0
            while ("layer%d.%d.conv1.weight" % (li, k)) in sd:
                x = basic_block(sd, "layer%d.%d" % (li, k), x, 2 if (li > 1 and k == 0) else 1, calibrate)
                k += 1
        d = 0
        while ("deconv_layers.%d.weight" % (3 * d)) in sd:                              # :168-193
            b = sd.get("deconv_layers.%d.bias" % (3 * d))
            x = F.conv_transpose2d(x, sd["deconv_layers.%d.weight" % (3 * d)].to(dtype), None if b is None else b.to(dtype),
                                   stride=2, padding=1)
            x = F.relu(_bn(sd, "deconv_layers.%d" % (3 * d + 1), x, calibrate))
            d += 1
        return _conv(sd, "final_layer", x)
