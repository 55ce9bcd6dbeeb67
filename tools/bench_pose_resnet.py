"""pose_resnet_50 (SimpleBaseline, 256x192) throughput on one MI355X: batch 64 with the flip test and the DARK decode,
split-fp16 ("f16x2") and fp32 storage.  Prints ONE JSON line: images/s, ms per step, launches per forward and the
per-op-class kernel time of udp_hrnet_profile (hipEvents around every launch, eager), with algorithmic TFLOP/s and the
fraction of the matrix peak (833 TFLOP/s dense fp16 for f16x2 -- each product is three fp16 MFMAs, counted once --,
157 TFLOP/s fp32) per class; the deconv layers are their own class.

    python tools/bench_pose_resnet.py [--steps 20] [--warmup 5] [--batch 64] [--dtypes f16x2,f32]

``--model pose_resnet_psa --layers 18|34`` measures the BasicBlock ResNet with polarized self-attention instead; its
result also lists the mean time of the four attention launches per channel width (``psa_ms_by_width``).
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

from udp_pose_amd import _lib, synth                                # noqa: E402
from udp_pose_amd.inference import decode_device                    # noqa: E402
from udp_pose_amd.model import MODELS                               # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_psa_state_dict, synth_pose_resnet_state_dict  # noqa: E402
from udp_pose_amd.transforms import COCO_FLIP_PAIRS, flip_fuse      # noqa: E402

PEAK_TF = {"f16x2": 833.0, "f32": 157.0}
EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
         "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}


PSA_KINDS = {_lib.UDP_OP_PSA_POOL: "pool", _lib.UDP_OP_PSA_MLP: "mlp", _lib.UDP_OP_PSA_SCALE: "scale", _lib.UDP_OP_PSA_SP: "sp"}
PSA_LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def op_class(name, kind, ks, stride):
    if kind == _lib.UDP_OP_DECONV:
        return "deconv"
    if kind == _lib.UDP_OP_STEM7:
        return "stem7"
    if kind == _lib.UDP_OP_MAXPOOL:
        return "maxpool"
    if name == "final_layer":
        return "head"
    if kind in PSA_KINDS:
        return "psa_" + PSA_KINDS[kind]
    return "conv%dx%d_s%d" % (ks, ks, stride)


def run(dtype, n, steps, warmup, model="pose_resnet", layers=50):
    cfg = {"MODEL": {"NAME": model, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": dict(EXTRA, NUM_LAYERS=layers)}}
    if model == "pose_resnet_psa":
        sd = synth_pose_resnet_psa_state_dict(seed=7, layers=PSA_LAYERS[layers])
    else:
        sd = synth_pose_resnet_state_dict(seed=7)
    net = MODELS[model](cfg, is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()
    x = torch.from_numpy(synth.synth_crops(n, 256, 192, seed=3)).cuda()
    c, s = synth.synth_center_scale(n, seed=1)
    c, s = torch.from_numpy(c.astype(np.float64)).cuda(), torch.from_numpy(s.astype(np.float64)).cuda()

    def step():
        raw = net.raw_forward(x, flip_test=True)
        hm = flip_fuse(raw[:n], raw[n:], COCO_FLIP_PAIRS, False)
        return decode_device(hm, c, s, "gaussian", True, 4.0, True)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    handle, _, prog = net._compiled[(256, 192)]
    lib = _lib.lib()
    ms_op, desc = net.profile(x, flip_test=True)
    ms_op, desc = net.profile(x, flip_test=True)           # second run: warm caches, kernels loaded
    images = 2 * n                                          # images per launch sequence (flip test)
    classes = {}
    for (name, kind, ks, stride, cin, cout, hout, wout), t in zip(desc, ms_op):
        k = op_class(name, kind, ks, stride)
        macs = (4 if kind == _lib.UDP_OP_DECONV else ks * ks) * cin * cout * hout * wout
        if kind == _lib.UDP_OP_MAXPOOL or kind in PSA_KINDS:
            macs = 0
        e = classes.setdefault(k, {"launches": 0, "ms": 0.0, "gflop": 0.0})
        e["launches"] += 1
        e["ms"] += float(t)
        e["gflop"] += 2.0 * macs * images / 1e9
    total = sum(e["ms"] for e in classes.values())
    for e in classes.values():
        e["share"] = round(e["ms"] / total, 4)
        e["tflops"] = round(e["gflop"] / e["ms"] if e["ms"] > 0 else 0.0, 1)
        e["peak_frac"] = round(e["tflops"] / PEAK_TF[dtype], 4)
        e["ms"] = round(e["ms"], 4)
        e["gflop"] = round(e["gflop"], 2)
    gflop_dec = classes["deconv"]["gflop"]
    gflop_all = sum(e["gflop"] for e in classes.values())
    res = {"dtype": dtype, "images_per_s": round(n / ms * 1000.0, 1), "ms_per_step": round(ms, 3),
           "launches_per_forward": int(lib.udp_hrnet_num_launches(handle)),
           "gflop_per_image": round(lib.udp_hrnet_flops_per_image(handle) / 1e9, 3),
           "kernel_ms_profiled": round(total, 3), "deconv_flop_share": round(gflop_dec / gflop_all, 4),
           "by_class": classes}
    if model == "pose_resnet_psa":
        # mean ms of each attention launch per width "C<channels>@<h>x<w>" (SP: cout is the map's width), and of the
        # whole block with its theta conv
        by_width = {}
        for (name, kind, ks, stride, cin, cout, hout, wout), t in zip(desc, ms_op):
            if kind in PSA_KINDS or name.endswith(".deattn.conv_v_left"):
                c = cin if kind != _lib.UDP_OP_PSA_SP else cout
                e = by_width.setdefault("C%d@%dx%d" % (c, hout, wout), {})
                e.setdefault(PSA_KINDS.get(kind, "theta"), []).append(float(t))
        res["psa_ms_by_width"] = {k: {op: round(float(np.mean(v)), 4) for op, v in e.items()} for k, e in by_width.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtypes", default="f16x2,f32")
    ap.add_argument("--model", default="pose_resnet", choices=["pose_resnet", "pose_resnet_psa"])
    ap.add_argument("--layers", type=int, default=None, choices=[18, 34], help="pose_resnet_psa only (default 18)")
    a = ap.parse_args()
    if a.model == "pose_resnet" and a.layers is not None:
        ap.error("--layers goes with --model pose_resnet_psa")
    layers = 50 if a.model == "pose_resnet" else (a.layers or 18)
    res = [run(d, a.batch, a.steps, a.warmup, a.model, layers) for d in a.dtypes.split(",")]
    out = {"workload": "%s_%d 256x192 flip-test + DARK decode" % (a.model, layers), "batch": a.batch, "results": res}
    if len(res) == 2:
        out["f16x2_over_f32"] = round(res[0]["images_per_s"] / res[1]["images_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
