#!/usr/bin/env python3
"""Write tests/golden/rsn18_se_prm_top_17.npz and rsn18_se_prm_top_keys_17.json from the REFERENCE's own module (build
container only: it needs the reference tree, which is imported from where it lies through the loader helpers of
oracle/gen_golden.py; nothing is copied).

The module is ``RSN(cfg)`` of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py exactly as that file builds it: its
Bottleneck with the SELayer, its Upsample_unit with the PRM, and its OWN ``ResNet_top`` (network.py:188-203: conv 3x3 s2
3 -> 64, conv 7x7 s1 64 -> 64, conv 3x3 s2 64 -> 64, no max-pool).  Nothing is substituted, unlike
tools/gen_golden_rsn_se_prm.py, which had to swap the stem in.

The .npz holds the module's fp32 output for one synthetic crop (seed 8) at 256x192 and the BatchNorm calibration
statistics (24 crops, seed 15; running means rounded to fp16 as in bn_calib_rsn18_17.npz) plus ``final.scale``; it holds
no weights: ``synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=..., stem="conv7")`` re-draws them (the stem convs by
the rule of every other conv there: He scale, N(0, 2 / fan_in)).

Before writing, it asserts that the fixture can see the feature:
  * synth key order and shapes equal the module's;
  * the fp64 restatement (tests/rsn_top_ref.py) equals the module's fp64 evaluation to 1e-9;
  * every SE gate vector and both PRM gates have a standard deviation >= 0.05 over their domain;
  * zeroing the 48 off-centre taps of ``top.conv.1`` moves the fp64 output by more than 100 x the 3e-3 comparison
    tolerance of tests/test_gpu_rsn_top.py.
The same weights cannot be evaluated on the plain stem's graph at all: that graph reads ``top.conv.conv.*`` / ``top.conv.bn.*``,
which this key set does not have (and it has ``top.conv.{0,1,2}.*``, which that graph refuses) -- stated, not run.

    python tools/gen_golden_rsn_se_prm_top.py
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
import rsn_top_ref as ref                    # noqa: E402

RSN_DIR = "/root/reference/RSN"
TOL = 3e-3
SEED = 4


def main():
    sys.path.insert(0, RSN_DIR)
    prm = gg._load("ref_rsn_se_prm_network", os.path.join(RSN_DIR, "exps/RSN18.coco.e1.se.36x8x132000_prm/network.py"))
    cfg = gg.AttrDict({"MODEL": {"STAGE_NUM": 1, "UPSAMPLE_CHANNEL_NUM": 256}, "DATASET": {"KEYPOINT": {"NUM": 17}},
                       "OUTPUT_SHAPE": (64, 48), "LOSS": {"OHKM": True, "TOPK": 8, "COARSE_TO_FINE": True}})
    net = prm.RSN(cfg)
    net.eval()
    keys = {k: list(v.shape) for k, v in net.state_dict().items()}
    want = synth.rsn18_se_prm_param_shapes(17, stem="conv7")
    assert list(keys) == list(want) and all(tuple(keys[k]) == tuple(want[k]) for k in keys), "key contract"
    assert "top.conv.conv.weight" not in keys and "top.conv.1.conv.weight" in keys      # the plain stem's graph cannot take these weights

    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=SEED, stem="conv7")
    xc = torch.from_numpy(synth.synth_crops(24, 256, 192, seed=15))
    yc = ref.forward(sd, xc, calibrate=True)
    calib = {k: v.numpy().astype(np.float16).astype(np.float32) if "running_mean" in k else v.numpy() for k, v in sd.items() if "running_" in k}
    calib["final.scale"] = np.float32(0.25 / float(yc.std()))
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=SEED, bn_calib=calib, stem="conv7")
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
    gates = {k: v for k, v in taps.items() if k not in ("prm.out", "top")}
    for k, v in gates.items():
        assert float(v.std()) >= 0.05, "gate %s is flat: std %g" % (k, float(v.std()))
    centre = float(np.abs(ref.forward(sd64, x.double(), centre_only=True).numpy() - r64).max())
    assert centre > 100 * TOL, "the output does not see the 48 off-centre taps of top.conv.1: %g" % centre
    with open(os.path.join(gg.OUT, "rsn18_se_prm_top_keys_17.json"), "w") as f:
        json.dump(keys, f)
    np.savez_compressed(os.path.join(gg.OUT, "rsn18_se_prm_top_17.npz"), out=y,
                        **{"calib:" + k: (v.astype(np.float16) if "running_mean" in k else v) for k, v in calib.items()})
    stds = sorted(float(v.std()) for v in gates.values())
    top = taps["top"]
    print("rsn18 se+prm, own stem: absmax %.3g std %.3g |fp32 - fp64| %.3g  gate std min %.3g  centre tap only %.3g  "
          "stem output absmax %.3g, %.0f %% zeros"
          % (float(np.abs(y).max()), float(y.std()), float(np.abs(y - y64).max()), stds[0], centre, float(top.abs().max()),
             100 * float((top == 0).double().mean())))


if __name__ == "__main__":
    main()
