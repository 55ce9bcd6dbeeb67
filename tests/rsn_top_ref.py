"""Functional restatement of RSN-18 on the stem of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py, for any float
dtype: the graph that ``RSN18Hip(..., stem="conv7")`` runs.  Everything behind the stem is tests/rsn_se_prm_ref.py's
(its ``_Net``, ``_bottleneck`` and ``_prm`` are reused as they are); the stem is that experiment's own ``ResNet_top``
(:188-203): conv 3x3 s2 3 -> 64, conv 7x7 s1 64 -> 64, conv 3x3 s2 64 -> 64, each with BatchNorm and ReLU, no max-pool.
Pinned against the reference's own module, unmodified, by tools/gen_golden_rsn_se_prm_top.py
(tests/golden/rsn18_se_prm_top_17.npz).

``stem="pool"`` evaluates the plain RSN-18 stem instead (7x7 s2 conv + max-pool), i.e. rsn_se_prm_ref.forward.
``centre_only``: zero the 48 off-centre taps of ``top.conv.1`` on the way (the generator's sensitivity check).
``se`` / ``prm`` = False leave the addition out; ``calibrate`` / ``taps`` as in rsn_se_prm_ref."""
import torch
import torch.nn.functional as F

import rsn_se_prm_ref as base


@torch.no_grad()
def forward(sd, x, output_shape=(64, 48), se=True, prm=True, stem="conv7", calibrate=False, taps=None, centre_only=False):
    if stem == "pool":
        return base.forward(sd, x, output_shape, se=se, prm=prm, calibrate=calibrate, taps=taps)
    if centre_only:
        w = sd["top.conv.1.conv.weight"]
        keep = torch.zeros_like(w)
        keep[:, :, 3, 3] = w[:, :, 3, 3]
        sd = dict(sd)
        sd["top.conv.1.conv.weight"] = keep
    net = base._Net(sd, calibrate, taps)
    x = net.cbr(x, "top.conv.0", stride=2)                                   # ResNet_top.forward, :201-203
    x = net.cbr(x, "top.conv.1")
    x = net.cbr(x, "top.conv.2", stride=2)
    if taps is not None:
        taps["top"] = x
    feats = []
    for layer in range(1, 5):
        for b in range(2):
            x = base._bottleneck(net, x, "stage0.downsample.layer%d.%d" % (layer, b), 2 if (layer > 1 and b == 0) else 1, se)
        feats.append(x)
    h, w = output_shape
    sizes = [(h // 8, w // 8), (h // 4, w // 4), (h // 2, w // 2), (h, w)]
    up = res = None
    for ind, xin in enumerate(reversed(feats)):
        p = "stage0.upsample.up%d" % (ind + 1)
        out = net.cbr(xin, p + ".u_skip", relu=False)
        if ind > 0:
            out = out + net.cbr(F.interpolate(up, size=sizes[ind], mode="bilinear", align_corners=True), p + ".up_conv", relu=False)
        out = F.relu(out)
        if ind == 3 and prm:
            out = base._prm(net, out, p + ".prm")
            net.tap("prm.out", out)
        r = net.cbr(net.cbr(out, p + ".res_conv1"), p + ".res_conv2", relu=False)
        res = F.interpolate(r, size=output_shape, mode="bilinear", align_corners=True)
        up = out
    return res


to_dtype = base.to_dtype
