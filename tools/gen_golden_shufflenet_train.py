#!/usr/bin/env python3
"""Golden for one TRAINING step of pose_shufflenetv2_10x_pixel_shuffle (1.0x, 5 joints, gaussian, a batch of 2 x 96x64),
produced by the REFERENCE's own module in ``.train()`` mode, its ``JointsMSELoss(use_target_weight=True)`` and one
``backward()``, in fp64 and in fp32.  Build container only (it needs the reference checkout); the fixture holds data only.

    python tools/gen_golden_shufflenet_train.py [seed]     # writes tests/golden/shufflenet_train_step.npz

Contents: the batch, the fp64 loss and heat-maps, the updated running statistics of three BatchNorms (first, middle,
last), per parameter the max-abs and the sum of the fp64 gradient and the fp32 run's max error against it, the full fp64
gradient of every tensor of at most 4096 elements (every depthwise and BatchNorm parameter, first_conv, final_layer) and
256 seeded sample positions of the larger ones.

Before writing, it checks that the fixture can carry the tests: the functional restatement
(tests/shufflenet_train_ref.py) agrees with the module in fp64 to 1e-9 of each tensor's max, and the fp32 run is within
1e-3 of each gradient's max-abs (the GPU gate is a multiple of that error).  Otherwise pick another seed: of seeds 1-45
only 8, 9, 16, 17, 22, 28, 35, 36, 38 and 44 pass the second check.  The step is ill-conditioned by construction -- the
stage-4 BatchNorms of this batch see 12 values per channel, some ReLU input always lies within 1e-6 of zero, and when
it falls on the other side in an fp32 evaluation that ONE channel's BatchNorm gradients move by percents and everything
upstream follows.  Which element flips depends on the summation order, so a second fp32 evaluator has its own set of
unlucky seeds: the HIP step flips one channel at seeds 8, 16, 17, 28 and 36 (conv_last.1 channel 487 at seed 8) and
none at 9, 22 and 38.  Seed 9 is the first that carries both.  Gradients that are zero in exact arithmetic have no max to
be relative to; they are listed in ``zero_keys`` (see main).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as gg                                               # noqa: E402  (reference loader helpers)
from udp_pose_amd.synth_shufflenet import synth_shufflenet_state_dict  # noqa: E402

EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "1.0x", "FINAL_CONV_KERNEL": 1}
JOINTS, BATCH_SEED, FULL_MAX, N_SAMPLES = 5, 23, 4096, 256
ZERO_REL = 1e-12             # a gradient whose max is below this fraction of the largest gradient is a structural zero
STAT_BNS = ("backbone.first_conv.1", "backbone.features.8.branch_main.4", "decoder.duc.2.bn")


def _is_param(k):
    return not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))


def _module_step(ref, loss_mod, sd, batch, dtype):
    """One train-mode forward + criterion + backward of the reference's module: (loss, heat-maps, grads, state_dict)."""
    net = ref.get_pose_net(gg.model_cfg(EXTRA, JOINTS, "gaussian"), is_train=False)
    assert list(sd) == list(net.state_dict()), "synth_shufflenet key order != the reference module's"
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
    _, _, loss_mod, _, _ = gg.load_reference()
    models = os.path.join(gg.REF, "lib", "models")
    for sub in ("backbones", "decoders"):
        pkg = type(sys)("refmodels." + sub)
        pkg.__path__ = [os.path.join(models, sub)]
        sys.modules["refmodels." + sub] = pkg
    gg._load("refmodels.backbones.shufflenetv2", os.path.join(models, "backbones/shufflenetv2.py"), "refmodels.backbones")
    gg._load("refmodels.decoders.DUC", os.path.join(models, "decoders/DUC.py"), "refmodels.decoders")
    gg._load("refmodels.decoders.pixelshuffle", os.path.join(models, "decoders/pixelshuffle.py"), "refmodels.decoders")
    ref = gg._load("refmodels.pose_shufflenetv2_10x_pixel_shuffle",
                   os.path.join(models, "pose_shufflenetv2_10x_pixel_shuffle.py"), "refmodels")
    import shufflenet_train_ref as R                                   # noqa: E402
    sd = synth_shufflenet_state_dict(seed=seed, num_joints=JOINTS)
    batch = R.make_batch(2, JOINTS, 96, 64, seed=BATCH_SEED)
    loss64, y64, g64, sd64 = _module_step(ref, loss_mod, sd, batch, torch.float64)
    loss32, _, g32, _ = _module_step(ref, loss_mod, sd, batch, torch.float32)
    keys = [k for k in sd if _is_param(k)]
    assert list(g64) == keys
    # 1. the restatement is the module
    rl, ry, rg, rsd = R.loss_and_grads(sd, *batch, torch.float64)
    assert abs(rl - loss64) <= 1e-9 * abs(loss64), "restatement loss %r vs module %r" % (rl, loss64)
    assert float((ry - y64).abs().max()) <= 1e-9 * float(y64.abs().max())
    # A gradient that is zero in exact arithmetic -- the bias of a BatchNorm in front of a bias-free 1x1 conv and another
    # train-mode BatchNorm: the shift cancels -- is rounding noise (1e-17 in fp64, 1e-9 in fp32) with no scale of its
    # own; those tensors are listed as ``zero_keys`` and left out of the two relative checks.
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
    path = os.path.join(gg.OUT, "shufflenet_train_step.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "loss", loss64, "fp32 loss", loss32, "worst fp32 gradient error / max", worst,
          "full tensors", sum(1 for k in out if k.startswith("g_")), "sampled", sum(1 for k in out if k.startswith("s_")),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
