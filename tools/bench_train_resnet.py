"""`tools/bench_train.py --model pose_resnet`: the training step of res50 at 256x192, batch 32, fp32, graphed.

Prints one JSON line (ms per step, images/s), then starts `rocprofv3 --kernel-trace --stats` on a short run of itself
and reads the kernel trace: the share of all kernel time the deconv head's forward (deconv4s2_kernel), input-gradient
(deconv_dgrad_kernel) and weight-gradient (wgrad_kernel<float, 4>) launches take, and the median duration of each of
those launches per head shape (8x6 2048->256, 16x12 and 32x24 256->256 at the default input) -- the forward and the
input gradient do the same MACs, so the forward kernel is the yardstick of the new one."""
import collections
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES50_EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
               "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}
HEAD = (("deconv forward", "deconv4s2_kernel"), ("deconv dgrad", "deconv_dgrad_kernel"), ("deconv wgrad", "wgrad_kernelIfLi4E"),
        ("deconv wgrad", "wgrad_kernel<float, 4>"))


SHAPES = ("2048->256 @ 8x6", "256->256 @ 16x12", "256->256 @ 32x24")      # the head at 256x192, in forward order


def head_report(trace_dir):
    """(share of all kernel time per head launch kind, [(kind, head shape, launches, median us)]).  Two head shapes can
    have the same grid, so a launch is attributed by its position: the forward runs the three layers in order, the
    backward (input and weight gradients alike) in reverse, step after step."""
    files = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        raise RuntimeError("no kernel_trace.csv under %s" % trace_dir)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    total, per_kind = 0.0, collections.OrderedDict()
    per_launch, seen = collections.OrderedDict(), collections.Counter()
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        total += us
        for kind, sub in HEAD:
            if sub in r["Kernel_Name"]:
                per_kind[kind] = per_kind.get(kind, 0.0) + us
                layer = seen[kind] % 3 if kind == "deconv forward" else 2 - seen[kind] % 3
                seen[kind] += 1
                per_launch.setdefault((kind, layer), []).append(us)
                break
    shares = {k: v / total for k, v in per_kind.items()}
    out = []
    for (kind, layer), v in sorted(per_launch.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        v = sorted(v[len(v) // 4:])                      # drop warm-up launches
        out.append((kind, SHAPES[layer], len(v), v[len(v) // 2]))
    return shares, out


def main(a):
    import torch
    sys.path.insert(0, ROOT)
    from udp_pose_amd import synth
    from udp_pose_amd.resnet_plan import PoseResNetProgram, pose_resnet_spec
    from udp_pose_amd.synth_resnet import synth_pose_resnet_state_dict
    from udp_pose_amd.train import PoseResNetTrainer
    if a.dtype != "f32" or a.target != "gaussian":
        raise SystemExit("pose_resnet trains in fp32 with gaussian targets")
    nj, spec = 17, pose_resnet_spec(RES50_EXTRA)
    sd = synth_pose_resnet_state_dict(seed=7)
    tr = PoseResNetTrainer(spec, nj, "gaussian", sd)
    x = torch.from_numpy(synth.synth_crops(a.batch, 256, 192, seed=1)).cuda()
    tg = torch.from_numpy(synth.synth_heatmaps(a.batch, nj, 64, 48, seed=2, channels_per_joint=1)).cuda()
    tw = torch.ones(a.batch, nj, 1, device="cuda")
    graphed = not a.no_graph

    def step():
        return tr.train_step_graphed(x, tg, tw) if graphed else tr.train_step(x, tg, tw)

    for _ in range(max(a.warmup, 2 if graphed else 0)):
        loss = step()
    torch.cuda.synchronize()
    t0 = time.time()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.time() - t0) / a.steps * 1e3
    dev = e0.elapsed_time(e1) / a.steps
    macs = PoseResNetProgram(sd, spec, 256, 192, "f32").macs_per_image()
    tf = 3 * 2.0 * macs * a.batch / (dev * 1e-3) / 1e12        # forward + input gradient + weight gradient
    print(json.dumps({"model": a.model, "metric": "images/sec pose_resnet-50 256x192 training step (fwd + JointsMSELoss + bwd + Adam)",
                      "value": round(a.batch / wall * 1e3, 1), "unit": "images/s", "n_gpus": 1, "ms_per_step": round(wall, 3),
                      "device_ms_per_step": round(dev, 3), "dtype": "f32", "batch_per_gpu": a.batch, "hipgraph": graphed,
                      "roofline": {"bound": "mfma", "achieved": round(tf, 2), "peak": 157.3, "unit": "TFLOP/s",
                                   "frac": round(tf / 157.3, 4)}}))
    print("train pose_resnet-50 b=%d f32%s: %.1f ms/step (device %.1f ms), %.0f img/s, loss %s after %d steps, peak mem %.1f GiB" % (
        a.batch, " hipGraph replay" if graphed else "", wall, dev, a.batch / wall * 1e3, loss.cpu().numpy(), tr.step_count,
        torch.cuda.max_memory_allocated() / 2**30))
    if a.no_profile:
        return 0
    prof = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    out = tempfile.mkdtemp(prefix="bench_train_resnet_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.join(ROOT, "tools", "bench_train.py"), "--model", "pose_resnet", "--no-profile", "--batch", str(a.batch),
               "--steps", "4", "--warmup", "2"] + (["--no-graph"] if a.no_graph else [])
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        shares, rows = head_report(out)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    print("share of all kernel time (rocprofv3 --kernel-trace --stats, %d-image steps): %s" % (
        a.batch, ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in shares.items())))
    for kind, shape, n, med in rows:
        print("  %-18s %-15s launches %-3d median %8.1f us" % (shape, kind, n, med))
    return 0
