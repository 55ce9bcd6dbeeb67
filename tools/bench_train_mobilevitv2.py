#!/usr/bin/env python3
"""The training step of pose_mobilevitv2_pixel_shuffle (width 0.5, 256x192, batch 32, fp32, hipGraph replay).

    python tools/bench_train_mobilevitv2.py [--size 0.5] [--batch 32] [--no-profile | --profile-only]

Median and [min, max] ms per step of 5 windows of 20 steps after 5 warm-up steps (one JSON line).  Then, unless
--no-profile, a `rocprofv3 --kernel-trace --stats` run of a short run of itself (a process of its own) and from its kernel
trace: the share of all kernel time per kernel, and for the SiLU, GroupNorm and attention kernels every launch shape next
to the element-wise yardstick -- a `udp_relu_bwd` launch over a map of the same float count (--yardstick, run in the same
traced process).  One trainer per process: --profile-only skips the timing, so that a job script can give the timed run
and the traced run a time limit each."""
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
EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": 0.5, "FINAL_CONV_KERNEL": 1}
OURS = ("silu_fwd_kernel", "silu_bwd_kernel", "gn_stats_kernel", "gn_apply_kernel", "gn_bwd_reduce_kernel", "gn_bwd_apply_kernel",
        "gn_param_grad_kernel", "linattn_fwd_kernel", "linattn_bwd_kernel")


def time_step(size, batch, windows, steps, warmup):
    import torch
    from udp_pose_amd import synth
    from udp_pose_amd.mobilevitv2_plan import mobilevitv2_spec
    from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict
    from udp_pose_amd.train import MobileViTv2Trainer
    tr = MobileViTv2Trainer(mobilevitv2_spec(dict(EXTRA, MODEL_SIZE=size)), 17, "gaussian",
                            synth_mobilevitv2_state_dict(seed=7, model_size=size))
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
    print(json.dumps({"model": "pose_mobilevitv2_pixel_shuffle",
                      "metric": "ms per training step, MobileViTv2-%s 256x192 (fwd + JointsMSELoss + bwd + Adam)" % size,
                      "value": round(med, 3), "unit": "ms/step", "min": round(ms[0], 3), "max": round(ms[-1], 3),
                      "windows": windows, "steps_per_window": steps, "images_per_s": round(batch / med * 1e3, 1), "dtype": "f32",
                      "batch_per_gpu": batch, "hipgraph": True, "loss": [float(v) for v in loss.cpu().numpy()]}), flush=True)


def yardstick(batch):
    """udp_relu_bwd over maps of the float counts the new kernels see (3 tensors of that size pass through it: dy, y, g)."""
    import torch
    from udp_pose_amd import _lib
    L = _lib.lib()
    for label, h, w, c in (("128x96x16 silu stem", 128, 96, 16), ("128x96x32 silu", 128, 96, 32), ("64x48x64 silu", 64, 48, 64),
                           ("32x24x64 gnorm", 32, 24, 64), ("32x24x144 qkv", 32, 24, 144), ("32x24x128 silu ffn", 32, 24, 128),
                           ("16x12x96 gnorm", 16, 12, 96), ("16x12x208 qkv", 16, 12, 208), ("8x6x128 gnorm", 8, 6, 128),
                           ("8x6x272 qkv", 8, 6, 272)):
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
        grid = "%sx%s" % (r.get("Grid_Size_X") or r.get("Grid_Size") or "?", r.get("Grid_Size_Y") or "1")
        if any(o in name for o in OURS) or "relu_bwd" in name:
            launches[(short, grid)].append(us)
    print("share of all kernel time (rocprofv3 --kernel-trace --stats, %d-image steps, %d launches, %.1f ms):" % (batch, len(rows), total / 1e3))
    for k, v in per_kernel.most_common(24):
        print("  %-44s %5.1f %%" % (k, 100 * v / total))
    print("launch shapes of the new kernels and of udp_relu_bwd (grid = work items; median us over the trace):")
    for (k, grid), v in sorted(launches.items()):
        v.sort()
        print("  %-30s grid %-14s launches %-4d median %8.1f us" % (k, grid, len(v), v[len(v) // 2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=float, default=0.5, choices=(0.5, 0.75, 1.0))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-only", action="store_true", help="only the traced child run and its report (this process opens no GPU)")
    ap.add_argument("--yardstick", action="store_true", help="also launch udp_relu_bwd over the maps of the new kernels (traced runs)")
    a = ap.parse_args()
    if not a.profile_only:
        time_step(a.size, a.batch, a.windows, a.steps, a.warmup)
        if a.yardstick:
            yardstick(a.batch)
    if a.no_profile:
        return 0
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    out = tempfile.mkdtemp(prefix="bench_train_mobilevitv2_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--size", str(a.size), "--no-profile", "--yardstick", "--batch", str(a.batch), "--windows", "1", "--steps", "4", "--warmup", "2"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        report(out, a.batch)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
