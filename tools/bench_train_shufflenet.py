#!/usr/bin/env python3
"""The training step of the two ShuffleNetV2 pose nets (1.0x, 256x192, batch 32, fp32, hipGraph replay).

    python tools/bench_train_shufflenet.py [--head pixel_shuffle|deconv|both] [--batch 32] [--no-profile]

Per head: median and [min, max] ms per step of 5 windows of 20 steps after 5 warm-up steps (one JSON line each).  Then,
unless --no-profile, a `rocprofv3 --kernel-trace --stats` run of a short run of itself (a process of its own) and from its
kernel trace: the share of all kernel time per kernel, and for the three depthwise kernels, the channel shuffle / concat
and the pixel shuffle the achieved bytes/s of every launch shape next to the element-wise yardstick -- a `udp_relu_bwd`
launch over a map of the same byte count (--yardstick, run in the same traced process)."""
import argparse
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PS_EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "1.0x", "FINAL_CONV_KERNEL": 1}
DC_EXTRA = {"MODEL_SIZE": "1.0x", "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
            "NUM_DECONV_KERNELS": [4, 4, 4], "FINAL_CONV_KERNEL": 1}
# kernel-name fragment -> (label, bytes moved per launch as a function of the recorded grid is unknown: we time shapes
# through the yardstick run instead)
OURS = ("dwk_fwd_kernel", "dwk_dgrad_kernel", "dwk_wgrad_partial_kernel", "dwk_wgrad_reduce_kernel", "pixshuf2_train_kernel",
        "shuffle_pair_fwd_kernel", "shuffle_pair_bwd_kernel", "chan_cat2_kernel", "chan_uncat2_kernel")


def make_trainer(head):
    from udp_pose_amd.shufflenet_plan import shufflenet_deconv_spec, shufflenet_spec
    from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict, synth_shufflenet_state_dict
    from udp_pose_amd.train import ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer
    if head == "deconv":
        return ShuffleNetV2DeconvTrainer(shufflenet_deconv_spec(DC_EXTRA), 17, "gaussian", synth_shufflenet_deconv_state_dict(seed=7))
    return ShuffleNetV2Trainer(shufflenet_spec(PS_EXTRA), 17, "gaussian", synth_shufflenet_state_dict(seed=7))


def time_head(head, batch, windows, steps, warmup):
    import torch
    from udp_pose_amd import synth
    tr = make_trainer(head)
    x = torch.from_numpy(synth.synth_crops(batch, 256, 192, seed=1)).cuda()
    tg = torch.from_numpy(synth.synth_heatmaps(batch, 17, 64, 48, seed=2, channels_per_joint=1)).cuda()
    tw = torch.ones(batch, 17, 1, device="cuda")
    for _ in range(max(warmup, 2)):
        loss = tr.train_step_graphed(x, tg, tw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            loss = tr.train_step_graphed(x, tg, tw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    ms.sort()
    med = ms[len(ms) // 2]
    print(json.dumps({"model": "pose_shufflenetv2_10x" + ("" if head == "deconv" else "_pixel_shuffle"),
                      "metric": "ms per training step, ShuffleNetV2 1.0x 256x192 (fwd + JointsMSELoss + bwd + Adam)",
                      "value": round(med, 3), "unit": "ms/step", "min": round(ms[0], 3), "max": round(ms[-1], 3),
                      "windows": windows, "steps_per_window": steps, "images_per_s": round(batch / med * 1e3, 1), "dtype": "f32",
                      "batch_per_gpu": batch, "hipgraph": True, "loss": [float(v) for v in loss.cpu().numpy()]}), flush=True)
    return tr, (x, tg, tw)


def yardstick(batch):
    """udp_relu_bwd over maps of the byte counts the new kernels move (3 tensors of that size pass through it: dy, y, g)."""
    import torch
    from udp_pose_amd import _lib
    L = _lib.lib()
    for label, h, w, c in (("64x48x32", 64, 48, 32), ("32x24x128", 32, 24, 128), ("32x24x64", 32, 24, 64), ("16x12x240", 16, 12, 240),
                           ("16x12x128", 16, 12, 128), ("8x6x464", 8, 6, 464), ("8x6x240", 8, 6, 240), ("64x48x32 head", 64, 48, 128)):
        n = batch * h * w * c
        a, b, g = (torch.randn(n, device="cuda") for _ in range(3))
        for _ in range(5):
            _lib.check(L.udp_relu_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), n, _lib.UDP_F32, _lib.stream_ptr()))
        torch.cuda.synchronize()
        print("yardstick %s floats %d" % (label, n))


def report(trace_dir, batch):
    files = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        raise RuntimeError("no kernel_trace.csv under %s" % trace_dir)
    rows = list(csv.DictReader(open(files[0])))
    total = 0.0
    per_kernel = collections.Counter()
    launches = collections.defaultdict(list)                   # (kernel, grid) -> [us]
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        name = r["Kernel_Name"]
        short = name.split("(")[0].split("<")[0].replace("void ", "").replace("udp::", "")
        total += us
        per_kernel[short] += us
        grid = r.get("Grid_Size_X") or r.get("Grid_Size") or "?"
        if any(o in name for o in OURS) or "relu_bwd" in name:
            launches[(short, grid)].append(us)
    print("share of all kernel time (rocprofv3 --kernel-trace --stats, %d-image steps, %d launches, %.1f ms):" % (batch, len(rows), total / 1e3))
    for k, v in per_kernel.most_common(24):
        print("  %-44s %5.1f %%" % (k, 100 * v / total))
    print("launch shapes of the new kernels and of udp_relu_bwd (grid = work items; median us over the trace):")
    for (k, grid), v in sorted(launches.items()):
        v.sort()
        print("  %-30s grid %-10s launches %-4d median %8.1f us" % (k, grid, len(v), v[len(v) // 2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--head", default="both", choices=("pixel_shuffle", "deconv", "both"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--yardstick", action="store_true", help="also launch udp_relu_bwd over the maps of the new kernels (traced runs)")
    a = ap.parse_args()
    heads = ("pixel_shuffle", "deconv") if a.head == "both" else (a.head,)
    for head in heads:
        time_head(head, a.batch, a.windows, a.steps, a.warmup)
    if a.yardstick:
        yardstick(a.batch)
    if a.no_profile:
        return 0
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    out = tempfile.mkdtemp(prefix="bench_train_shufflenet_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--head", heads[0], "--no-profile", "--yardstick", "--batch", str(a.batch), "--windows", "1", "--steps", "4", "--warmup", "2"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        report(out, a.batch)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
