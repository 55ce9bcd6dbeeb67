"""RSN-18 (256x192) throughput on one MI355X, plain or with the SELayer (``--se``) and the Pose Refine Machine (``--prm``),
on RSN18.coco's stem or (``--stem conv7``) on the one of RSN18.coco.e1.se.36x8x132000_prm with its 7x7 stride-1 conv: batch 64 with the flip test and the offset decode (51-channel head), synthetic weights, hipGraph replay.  Prints ONE JSON
line per storage mode: images/s (median of 5 windows of ``--steps`` steps, with min / max), ms per step, launches per
forward, and the kernel time per op class of udp_hrnet_profile (hipEvents around every launch, eager).

    python tools/bench_rsn.py [--se] [--prm] [--stem conv7] [--dtype f16x2,f32] [--steps 20] [--warmup 5] [--batch 64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from bench import HotPath                             # noqa: E402
from udp_pose_amd import _lib, synth                  # noqa: E402
from udp_pose_amd.model import RSN18Hip               # noqa: E402

CLASSES = {_lib.UDP_OP_SE_RES: "se_res", _lib.UDP_OP_PRM_GATE: "prm_gate", _lib.UDP_OP_PRM_DW9: "prm_dw9", _lib.UDP_OP_STEM7: "stem7", _lib.UDP_OP_STEM: "stem3",
           _lib.UDP_OP_MAXPOOL: "maxpool", _lib.UDP_OP_BILINEAR: "bilinear", _lib.UDP_OP_FUSE: "sum"}


def build(dtype, se, prm, stem="pool"):
    if not (se or prm) and stem == "pool":
        cp = os.path.join(ROOT, "tests", "golden", "bn_calib_rsn18_51.npz")
        sd = synth.synth_rsn18_state_dict(51, seed=4, bn_calib=dict(np.load(cp)))
        return RSN18Hip(51, dtype=dtype).load_state_dict(sd)
    # BatchNorm statistics of the 17-channel fixture (the 51-channel head keeps its own unit statistics)
    g = np.load(os.path.join(ROOT, "tests", "golden", "rsn18_se_prm_17.npz"))
    if stem == "conv7":     # the fixture of the experiment's own stem has the statistics of top.conv.{0,1,2} too
        g = np.load(os.path.join(ROOT, "tests", "golden", "rsn18_se_prm_top_17.npz"))
    want = synth.rsn18_se_prm_param_shapes(51, 256, se, prm, stem)
    calib = {k[6:]: g[k] for k in g.files if k.startswith("calib:") and (k[6:] == "final.scale" or tuple(want.get(k[6:], ())) == g[k].shape)}
    sd = synth.synth_rsn18_se_prm_state_dict(51, seed=4, bn_calib=calib, se=se, prm=prm, stem=stem)
    return RSN18Hip(51, dtype=dtype, se=se, prm=prm, stem=stem).load_state_dict(sd)


def run(dtype, a):
    net = build(dtype, a.se, a.prm, a.stem).to("cuda")
    net.use_graph = True
    hp = HotPath(net, a.batch, torch.device("cuda"), seed=100, h=256, w=192, target_type="offset")
    for _ in range(a.warmup):
        hp.step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            out = hp.step()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / a.steps)
    assert torch.isfinite(out[1]).all()
    handle, _, prog = net._compiled[(256, 192)]
    x = torch.from_numpy(synth.synth_crops(a.batch, 256, 192, seed=3)).cuda()
    net.profile(x, flip_test=True)
    ms_op, desc = net.profile(x, flip_test=True)
    by = {}
    for (name, kind, ks, stride, cin, cout, hout, wout), t in zip(desc, ms_op):
        k = CLASSES.get(kind, "conv%dx%d" % (ks, ks))
        e = by.setdefault(k, {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] = round(e["ms"] + float(t), 4)
    med = float(np.median(ms))
    return {"net": "rsn18" + ("+se" if a.se else "") + ("+prm" if a.prm else "") + ("+conv7stem" if a.stem == "conv7" else ""), "dtype": dtype, "batch": a.batch,
            "images_per_s": round(a.batch / med * 1e3, 1), "images_per_s_min_max": [round(a.batch / max(ms) * 1e3, 1), round(a.batch / min(ms) * 1e3, 1)],
            "ms_per_step": round(med, 3), "windows": "5 windows of %d steps, median" % a.steps, "lanes": int(_lib.lib().udp_hrnet_lanes(handle, a.batch)),
            "launches_per_forward": int(_lib.lib().udp_hrnet_num_launches(handle)), "kernel_ms_profiled": round(float(sum(ms_op)), 3),
            "by_class": by}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--se", action="store_true")
    ap.add_argument("--prm", action="store_true")
    ap.add_argument("--stem", choices=["pool", "conv7"], default="pool")
    ap.add_argument("--dtype", default="f16x2,f32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rsn.py needs a GPU: a timing from anywhere else says nothing")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for dtype in a.dtype.split(","):
        print(json.dumps(run(dtype, a)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
