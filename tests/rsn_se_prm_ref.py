"""Functional restatement of RSN-18 with the SELayer and the Pose Refine Machine, for any float dtype: the graph that
``RSN18Hip(se=True, prm=True)`` runs.  Lines cite RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py, except the stem,
which is RSN/exps/RSN18.coco/network.py:125-137 (7x7 s2 conv + max-pool): the planner has no kernel for the 7x7 stride-1
64 -> 64 conv of that experiment's own ResNet_top (:188-203).  Pinned against the reference's own modules composed that
way by tools/gen_golden_rsn_se_prm.py (tests/golden/rsn18_se_prm_17.npz).

``calibrate``: write every BatchNorm's batch statistics into ``sd`` on the way (fixture generation).  ``taps``: a dict that
receives the SE gate vectors ("se:<block>"), the PRM gates ("prm.channel", "prm.spatial") and the PRM output.
``se`` / ``prm`` = False leave the addition out (the sensitivity checks of the generator)."""
import torch
import torch.nn.functional as F

BN_EPS = 1e-5


class _Net:
    def __init__(self, sd, calibrate, taps):
        self.sd, self.calibrate, self.taps = sd, calibrate, taps

    def cbr(self, x, name, stride=1, relu=True, groups=1):
        """conv_bn_relu, :14-46"""
        sd = self.sd
        w = sd[name + ".conv.weight"]
        y = F.conv2d(x, w, sd[name + ".conv.bias"], stride=stride, padding=(w.shape[2] - 1) // 2, groups=groups)
        if self.calibrate:
            sd[name + ".bn.running_mean"] = y.mean(dim=(0, 2, 3)).clone()
            sd[name + ".bn.running_var"] = y.var(dim=(0, 2, 3), unbiased=False).clone()
        y = F.batch_norm(y, sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"], sd[name + ".bn.weight"], sd[name + ".bn.bias"],
                         training=False, eps=BN_EPS)
        return F.relu(y) if relu else y

    def tap(self, k, v):
        if self.taps is not None:
            self.taps[k] = v


def _se(net, x, p):
    """SELayer.forward, :62-66 (reduction 8, no biases)"""
    y = torch.sigmoid(F.relu(x.mean(dim=(2, 3)) @ net.sd[p + ".fc.0.weight"].t()) @ net.sd[p + ".fc.2.weight"].t())
    net.tap("se:" + p, y)
    return x * y[:, :, None, None]


def _bottleneck(net, x, p, stride, se):
    """Bottleneck.forward, :120-145"""
    out = net.cbr(x, p + ".conv_bn_relu1", stride=stride)
    s = torch.split(out, out.shape[1] // 4, 1)
    o11 = net.cbr(s[0], p + ".conv_bn_relu2_1_1")
    o21 = net.cbr(s[1] + o11, p + ".conv_bn_relu2_2_1")
    o22 = net.cbr(o21, p + ".conv_bn_relu2_2_2")
    o31 = net.cbr(s[2] + o21, p + ".conv_bn_relu2_3_1")
    o32 = net.cbr(o31 + o22, p + ".conv_bn_relu2_3_2")
    o33 = net.cbr(o32, p + ".conv_bn_relu2_3_3")
    o41 = net.cbr(s[3] + o31, p + ".conv_bn_relu2_4_1")
    o42 = net.cbr(o41 + o32, p + ".conv_bn_relu2_4_2")
    o43 = net.cbr(o42 + o33, p + ".conv_bn_relu2_4_3")
    o44 = net.cbr(o43, p + ".conv_bn_relu2_4_4")
    out = net.cbr(torch.cat((o11, o22, o33, o44), 1), p + ".conv_bn_relu3", relu=False)
    if se:
        out = _se(net, out, p + ".se")                                       # :137
    if (p + ".downsample.conv.weight") in net.sd:
        x = net.cbr(x, p + ".downsample", stride=stride, relu=False)
    return F.relu(out + x)


def _prm(net, x, p):
    """PRM.forward, :290-301"""
    out1 = net.cbr(x, p + ".conv_bn_relu_prm_1")
    o2 = net.cbr(out1.mean(dim=(2, 3), keepdim=True), p + ".conv_bn_relu_prm_2_1")
    o2 = torch.sigmoid(net.cbr(o2, p + ".conv_bn_relu_prm_2_2"))             # ReLU, then sigmoid (:278-281, :296)
    o3 = net.cbr(out1, p + ".conv_bn_relu_prm_3_1")
    o3 = torch.sigmoid(net.cbr(o3, p + ".conv_bn_relu_prm_3_2", groups=o3.shape[1]))
    net.tap("prm.channel", o2)
    net.tap("prm.spatial", o3)
    return out1 * (1 + o2 * o3)


@torch.no_grad()
def forward(sd, x, output_shape=(64, 48), se=True, prm=True, calibrate=False, taps=None):
    """RSN.forward for STAGE_NUM = 1 (:509-520): x [N,3,H,W] -> [N, C_out, *output_shape], in the dtype of ``sd`` / ``x``."""
    net = _Net(sd, calibrate, taps)
    x = F.max_pool2d(net.cbr(x, "top.conv", stride=2), kernel_size=3, stride=2, padding=1)
    feats = []
    for layer in range(1, 5):
        for b in range(2):
            x = _bottleneck(net, x, "stage0.downsample.layer%d.%d" % (layer, b), 2 if (layer > 1 and b == 0) else 1, se)
        feats.append(x)
    h, w = output_shape
    sizes = [(h // 8, w // 8), (h // 4, w // 4), (h // 2, w // 2), (h, w)]
    up = res = None
    for ind, xin in enumerate(reversed(feats)):                              # Upsample_unit.forward, :347-363
        p = "stage0.upsample.up%d" % (ind + 1)
        out = net.cbr(xin, p + ".u_skip", relu=False)
        if ind > 0:
            out = out + net.cbr(F.interpolate(up, size=sizes[ind], mode="bilinear", align_corners=True), p + ".up_conv", relu=False)
        out = F.relu(out)
        if ind == 3 and prm:
            out = _prm(net, out, p + ".prm")                                 # :357-358
            net.tap("prm.out", out)
        r = net.cbr(net.cbr(out, p + ".res_conv1"), p + ".res_conv2", relu=False)
        res = F.interpolate(r, size=output_shape, mode="bilinear", align_corners=True)
        up = out
    return res


def to_dtype(sd, dt):
    return {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
