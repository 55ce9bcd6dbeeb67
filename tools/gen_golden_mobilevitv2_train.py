#!/usr/bin/env python3
"""Golden for one TRAINING step of pose_mobilevitv2_pixel_shuffle (MODEL_SIZE 0.5, 5 joints, gaussian, a batch of
2 x 128x64), produced by the REFERENCE's own module in ``.train()`` mode, its ``JointsMSELoss(use_target_weight=True)``
and one ``backward()``, in fp64 and in fp32.  Build container only (it needs the reference checkout); the fixture holds
data only.

    python tools/gen_golden_mobilevitv2_train.py [seed]     # writes tests/golden/mobilevitv2_train_step.npz

At 128x64 the last map is 4x2: two pixels per parity class of the attention and 16 values per BatchNorm channel.

Contents (those of tests/golden/shufflenet_train_step.npz): the batch, the fp64 loss and heat-maps, the updated running
statistics of three BatchNorms (first, middle, last), per parameter the max-abs and the sum of the fp64 gradient and the
fp32 run's max error against it, the full fp64 gradient of every tensor of at most 4096 elements and 256 seeded sample
positions of the larger ones, and ``zero_keys``.

Before writing, it checks that the fixture can carry the tests: the functional restatement
(tests/mobilevitv2_train_ref.py) agrees with the module in fp64 to 1e-9 of each tensor's max, and the fp32 run is within
1e-3 of each gradient's max-abs (the GPU gate is a multiple of that error).  Otherwise pick another seed.  Seed 9, the
ShuffleNetV2 fixture's, passes both.  Gradients that are zero in exact arithmetic have no max to be relative to; they are
listed in ``zero_keys``: the unused classifier, and the bias of every norm (a red_1x1 / conv_proj BatchNorm, a block's
last GroupNorm) in front of a bias-free 1x1 conv and another train-mode BatchNorm, where the shift cancels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden as gg                                               # noqa: E402  (reference loader helpers)
from gen_golden_mobilevitv2 import EXTRA, load_reference_module       # noqa: E402
from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict  # noqa: E402

JOINTS, BATCH_SEED, FULL_MAX, N_SAMPLES = 5, 23, 4096, 256
SIZE = 0.5
ZERO_REL = 1e-12             # a gradient whose max is below this fraction of the largest gradient is a structural zero
STAT_BNS = ("backbone.conv_1.block.norm", "backbone.layer_4.1.conv_proj.block.norm", "decoder.duc.2.bn")


def _is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


def _module_step(ref, loss_mod, sd, batch, dtype):
    """One train-mode forward + criterion + backward of the reference's module: (loss, heat-maps, grads, state_dict)."""
    cfg = gg.model_cfg(dict(EXTRA, MODEL_SIZE=SIZE), JOINTS, "gaussian")
    dict.__getitem__(cfg, "MODEL")["CONFIG"] = os.path.join(gg.REF, "lib/models/backbones/configs/mobilevitv2-%s.yaml" % SIZE)
    net = ref.get_pose_net(cfg, is_train=False)
    assert list(sd) == list(net.state_dict()), "synth_mobilevitv2 key order != the reference module's"
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).train()
    x, tg, tw = (t.to(dtype) for t in batch)
    y = net(x)
    loss = loss_mod.JointsMSELoss(use_target_weight=True)(y, tg, tw)
    loss.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}
    return float(loss.detach()), y.detach(), grads, {k: v.detach().clone() for k, v in net.state_dict().items()}


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    ref = load_reference_module()
    loss_mod = gg.load_reference()[2]
    import mobilevitv2_train_ref as R                                  # noqa: E402
    sd = synth_mobilevitv2_state_dict(seed=seed, model_size=SIZE, num_joints=JOINTS)
    batch = R.make_batch(2, JOINTS, 128, 64, seed=BATCH_SEED)
    loss64, y64, g64, sd64 = _module_step(ref, loss_mod, sd, batch, torch.float64)
    loss32, _, g32, _ = _module_step(ref, loss_mod, sd, batch, torch.float32)
    keys = [k for k in sd if _is_param(k)]
    assert list(g64) == keys
    # 1. the restatement is the module
    rl, ry, rg, rsd = R.loss_and_grads(sd, *batch, torch.float64)
    assert abs(rl - loss64) <= 1e-9 * abs(loss64), "restatement loss %r vs module %r" % (rl, loss64)
    assert float((ry - y64).abs().max()) <= 1e-9 * float(y64.abs().max())
    gscale = max(float(g.abs().max()) for g in g64.values())
    zeros = []
    for k in keys:
        mx = float(g64[k].abs().max())
        if mx <= ZERO_REL * gscale:
            zeros.append(k)
            continue
        assert float((rg[k] - g64[k]).abs().max()) <= 1e-9 * mx, "restatement gradient of %s differs: pick another seed" % k
    for k in sd64:
        if "running_" in k:
            assert float((rsd[k] - sd64[k]).abs().max()) <= 1e-9 * float(sd64[k].abs().max()), k
    # 2. fp32 is a sane yardstick
    out = {"x": batch[0].numpy(), "target": batch[1].numpy(), "target_weight": batch[2].numpy(), "seed": np.int64(seed),
           "loss": np.float64(loss64), "loss_f32": np.float64(loss32), "heatmaps": y64.numpy(),
           "keys": np.array(keys), "zero_keys": np.array(zeros), "stat_bns": np.array(STAT_BNS)}
    gmax, gsum, e32 = [], [], []
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    worst = 0.0
    for i, k in enumerate(keys):
        g = g64[k].numpy().reshape(-1)
        err = float(np.abs(g32[k].double().numpy().reshape(-1) - g).max())
        mx = float(np.abs(g).max())
        if k not in zeros:
            worst = max(worst, err / mx)
            assert err <= 1e-3 * mx, "fp32 gradient of %s is %.3g of its max off fp64: pick another seed" % (k, err / mx)
        gmax.append(mx), gsum.append(float(g.sum())), e32.append(err)
        if g.size <= FULL_MAX:
            out["g_%d" % i] = g.reshape(g64[k].shape)
        else:
            pos = np.sort(rng.choice(g.size, N_SAMPLES, replace=False)).astype(np.int64)
            out["p_%d" % i] = pos
            out["s_%d" % i] = g[pos]
    out.update(gmax=np.array(gmax), gsum=np.array(gsum), e32=np.array(e32))
    for bn in STAT_BNS:
        for s in (".running_mean", ".running_var"):
            out["stat_" + bn + s] = sd64[bn + s].numpy()
    path = os.path.join(gg.OUT, "mobilevitv2_train_step.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "loss", loss64, "fp32 loss", loss32, "worst fp32 gradient error / max", worst, "zero keys", len(zeros),
          "full tensors", sum(1 for k in out if k.startswith("g_")), "sampled", sum(1 for k in out if k.startswith("s_")),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
