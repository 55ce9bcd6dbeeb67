#!/usr/bin/env python3
"""Write tests/golden/rsn18_se_prm_17.npz and rsn18_se_prm_keys_17.json from the REFERENCE's own modules (build container
only: it needs the reference tree, which is imported from where it lies through the loader helpers of
oracle/gen_golden.py; nothing is copied).

The module is ``RSN(cfg)`` of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py -- its Bottleneck with the SELayer, its
Upsample_unit with the PRM -- with ONE substitution made here at generation time: ``net.top`` is the ``ResNet_top`` of
RSN/exps/RSN18.coco/network.py (7x7 s2 conv + max-pool): this is the fixture of ``RSN18Hip(se=True, prm=True)`` on the
default ``stem="pool"``.  Both stems deliver 64 channels at 1/4 resolution, so everything behind it is the reference's
graph unchanged.  The experiment's own stem (network.py:188-203: 3x3 s2, 7x7 s1 64 -> 64, 3x3 s2; ``stem="conv7"``) has the
fixture of tools/gen_golden_rsn_se_prm_top.py, made from the module without any substitution.

The .npz holds the module's fp32 output for one synthetic crop (seed 8) at 256x192 and the BatchNorm calibration
statistics (24 crops, seed 15; running means rounded to fp16 as in bn_calib_rsn18_17.npz) plus ``final.scale``; it holds
no weights: ``synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=...)`` re-draws them.

Before writing, it asserts that the fixture can see the feature:
  * synth key order and shapes equal the module's;
  * the fp64 restatement (tests/rsn_se_prm_ref.py) equals the module's fp64 evaluation to 1e-9;
  * every SE gate vector and both PRM gates have a standard deviation >= 0.05 over their domain;
  * leaving the SE layers out (m = 1) or skipping the PRM each moves the fp64 output by more than 100 x the 3e-3
    comparison tolerance of tests/test_gpu_rsn_se_prm.py.
Chosen so that they hold (synth.py): fc.0 weights N(0, 400 / fan_in) -- with N(0, 4 / fan_in) the first SE gate had a
standard deviation of 0.02, because the pooled vector is the closing BatchNorm's bias (order 0.05) --, fc.2 weights
N(0, 4 / fan_in), PRM BatchNorm weights in [0.8, 1.6], seed 4.

    python tools/gen_golden_rsn_se_prm.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gen_golden as gg          # noqa: E402  (loader helpers: _load, AttrDict, OUT)
from udp_pose_amd import synth               # noqa: E402
import rsn_se_prm_ref as ref                 # noqa: E402

RSN_DIR = "/root/reference/RSN"
TOL = 3e-3


def main():
    sys.path.insert(0, RSN_DIR)
    plain = gg._load("ref_rsn_network", os.path.join(RSN_DIR, "exps/RSN18.coco/network.py"))
    prm = gg._load("ref_rsn_se_prm_network", os.path.join(RSN_DIR, "exps/RSN18.coco.e1.se.36x8x132000_prm/network.py"))
    cfg = gg.AttrDict({"MODEL": {"STAGE_NUM": 1, "UPSAMPLE_CHANNEL_NUM": 256}, "DATASET": {"KEYPOINT": {"NUM": 17}},
                       "OUTPUT_SHAPE": (64, 48), "LOSS": {"OHKM": True, "TOPK": 8, "COARSE_TO_FINE": True}})
    net = prm.RSN(cfg)
    net.top = plain.ResNet_top()
    net.eval()
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    want = synth.rsn18_se_prm_param_shapes(17)
    assert list(keys) == list(want) and all(tuple(keys[k]) == tuple(want[k]) for k in keys), "key contract"

    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4)
    xc = torch.from_numpy(synth.synth_crops(24, 256, 192, seed=15))
    yc = ref.forward(sd, xc, calibrate=True)
    calib = {k: v.numpy().astype(np.float16).astype(np.float32) if "running_mean" in k else v.numpy() for k, v in sd.items() if "running_" in k}
    calib["final.scale"] = np.float32(0.25 / float(yc.std()))
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=calib)
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    with torch.no_grad():
        y = net(x).numpy()
        y64 = net.double()(x.double()).numpy()
    sd64 = ref.to_dtype(sd, torch.float64)
    taps = {}
    r64 = ref.forward(sd64, x.double(), taps=taps).numpy()
    d = float(np.abs(r64 - y64).max())
    assert d <= 1e-9, "restatement vs the module in fp64: %g" % d
    for k, v in taps.items():
        if k != "prm.out":
            assert float(v.std()) >= 0.05, "gate %s is flat: std %g" % (k, float(v.std()))
    no_se = float(np.abs(ref.forward(sd64, x.double(), se=False).numpy() - r64).max())
    no_prm = float(np.abs(ref.forward(sd64, x.double(), prm=False).numpy() - r64).max())
    assert no_se > 100 * TOL and no_prm > 100 * TOL, "the output does not see the feature: without se %g, without prm %g" % (no_se, no_prm)
    with open(os.path.join(gg.OUT, "rsn18_se_prm_keys_17.json"), "w") as f:
        json.dump(keys, f)
    np.savez_compressed(os.path.join(gg.OUT, "rsn18_se_prm_17.npz"), out=y,
                        **{"calib:" + k: (v.astype(np.float16) if "running_mean" in k else v) for k, v in calib.items()})
    stds = sorted(float(v.std()) for k, v in taps.items() if k != "prm.out")
    print("rsn18 se+prm: absmax %.3g std %.3g |fp32 - fp64| %.3g  gate std min %.3g  without se %.3g  without prm %.3g"
          % (float(np.abs(y).max()), float(y.std()), float(np.abs(y - y64).max()), stds[0], no_se, no_prm))


if __name__ == "__main__":
    main()
