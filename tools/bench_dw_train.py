#!/usr/bin/env python3
"""Op-level timer of the depthwise 3x3 training kernels on the shapes of the two training steps that use them
(ShuffleNetV2 1.0x and MobileNetV3-small, 256x192, batch 32, fp32).

    python tools/bench_dw_train.py [--batch 32] [--reps 7] [--launches 400] [--warmup 20] [--limit 60]

Plain ctypes calls on torch-allocated buffers: no trainer, no graph.  A figure is the time of one launch inside a run of
--launches back-to-back launches on one stream, bracketed by a pair of events, after --warmup launches.  The whole table
(every shape x forward / input gradient with accumulate 0 / weight gradient) is walked --reps times; per walk and pass the
count-weighted sum over the table is one step's worth of that pass.  Reported per pass: the median sum, min, max and the
spread max - min over the walks.

While the library still exports udp_dwconv3_* the 3x3 family is timed next to udp_dwconvk_*(ks=3), the two alternating
inside every cell of the table, and the verdict per pass is printed: the strip arm replaces the 3x3 family when its median
sum is not above the other's by more than the other's own spread.  Without those exports udp_dwconvk_* is timed alone.

One process, sequential.  Every timed run has --limit seconds (SIGALRM with its default action ends the process: nothing
more is started on a device that does not answer).  The smallest maps take a few microseconds a launch, about what the
host needs to enqueue one, so their figures are bounded below by the enqueue rate -- for both families alike."""
import argparse
import collections
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PASSES = ("fwd", "dgrad", "wgrad")


def table(height=256, width=192):
    """[(net, real channels, stored channels, h, w, stride, count)] of every 3x3 depthwise conv of the two steps, from
    the nets' own tables.  Both backbones reach their first unit / block through a stride-2 stem; ShuffleNetV2 has a
    stride-2 max-pool behind it (shufflenetv2.py:124)."""
    from udp_pose_amd.synth_mobilenetv3 import BLOCKS
    from udp_pose_amd.synth_shufflenet import shufflenet_units
    count = collections.OrderedDict()

    def add(net, c, h, w, stride):
        key = (net, c, (c + 15) // 16 * 16, h, w, stride)
        count[key] = count.get(key, 0) + 1

    h, w = height // 4, width // 4
    for _, inp, _, mid, stride in shufflenet_units("1.0x"):
        if stride == 2:
            add("shufflenetv2_10x", inp, h, w, 2)              # branch_proj.0
        add("shufflenetv2_10x", mid, h, w, stride)             # branch_main.3
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
    h, w = height // 2, width // 2
    for _, ks, exp, _, _, _, stride in BLOCKS:
        if ks == 3:
            add("mobilenetv3_small", exp, h, w, stride)
        h, w = (h - 1) // stride + 1, (w - 1) // stride + 1
    return [k + (n,) for k, n in count.items()]


def calls(L, fam, n, cr, cs, h, w, stride, bufs, stream):
    """{pass: a function that enqueues one launch} of family ``fam`` ("dw3" | "dwk")."""
    from udp_pose_amd import _lib
    F32 = _lib.UDP_F32
    x, wt, y, dy, dx, dw, ws = (b.data_ptr() for b in bufs)
    ws_bytes = bufs[6].numel()
    if fam == "dw3":
        return {"fwd": lambda: L.udp_dwconv3_train_fwd(x, wt, n, h, w, cs, cr, stride, F32, y, stream),
                "dgrad": lambda: L.udp_dwconv3_dgrad(dy, wt, n, h, w, cs, cr, stride, 0, F32, dx, stream),
                "wgrad": lambda: L.udp_dwconv3_wgrad(x, dy, n, h, w, cs, cr, stride, F32, dw, ws, ws_bytes, stream)}
    return {"fwd": lambda: L.udp_dwconvk_train_fwd(x, wt, n, h, w, cs, cr, 3, stride, F32, y, stream),
            "dgrad": lambda: L.udp_dwconvk_dgrad(dy, wt, n, h, w, cs, cr, 3, stride, 0, F32, dx, stream),
            "wgrad": lambda: L.udp_dwconvk_wgrad(x, dy, n, h, w, cs, cr, 3, stride, F32, dw, ws, ws_bytes, stream)}


def timed(fn, launches, warmup, limit):
    """us per launch of ``launches`` back-to-back calls of ``fn``."""
    import torch
    from udp_pose_amd import _lib
    signal.alarm(limit)
    for _ in range(warmup):
        _lib.check(fn())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        rc = fn()
    e1.record()
    torch.cuda.synchronize()
    signal.alarm(0)
    _lib.check(rc)
    return e0.elapsed_time(e1) * 1e3 / launches


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2), "spread": round(s[-1] - s[0], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7, help="walks over the whole table (>= 5: the spread is max - min over them)")
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--limit", type=int, default=60, help="seconds a timed run may take")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps %d: the spread needs at least 5 walks" % a.reps)
    import torch
    from udp_pose_amd import _lib
    if not torch.cuda.is_available():
        raise RuntimeError("bench_dw_train.py times kernels on the GPU; none is visible")
    L = _lib.lib()
    fams = (["dw3"] if hasattr(L, "udp_dwconv3_train_fwd") else []) + ["dwk"]
    stream = _lib.stream_ptr()
    n = a.batch
    shapes = table()
    cells = []
    for net, cr, cs, h, w, stride, cnt in shapes:
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        gen = torch.Generator(device="cuda").manual_seed(cr * 1000 + h)
        ws_bytes = int(L.udp_dwconvk_wgrad_workspace_bytes(n, ho, wo, cs, 3))
        bufs = [torch.randn(n * h * w * cs, device="cuda", generator=gen), torch.randn(cr * 9, device="cuda", generator=gen),
                torch.empty(n * ho * wo * cs, device="cuda"), torch.randn(n * ho * wo * cs, device="cuda", generator=gen),
                torch.empty(n * h * w * cs, device="cuda"), torch.empty(cr * 9, device="cuda"),
                torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")]
        cells.append((bufs, {f: calls(L, f, n, cr, cs, h, w, stride, bufs, stream) for f in fams}))
    sums = {f: {p: [] for p in PASSES} for f in fams}
    per_cell = {f: {p: [[] for _ in shapes] for p in PASSES} for f in fams}
    for rep in range(a.reps):
        tot = {f: dict.fromkeys(PASSES, 0.0) for f in fams}
        for i, (shape, (_, by_fam)) in enumerate(zip(shapes, cells)):
            for p in PASSES:
                for f in (fams if rep % 2 == 0 else fams[::-1]):     # alternate, and swap who goes first from walk to walk
                    us = timed(by_fam[f][p], a.launches, a.warmup, a.limit)
                    per_cell[f][p][i].append(us)
                    tot[f][p] += shape[6] * us
        for f in fams:
            for p in PASSES:
                sums[f][p].append(tot[f][p])
        print(json.dumps({"walk": rep, "sum_us": {f: {p: round(tot[f][p], 2) for p in PASSES} for f in fams}}), flush=True)
    print("median us per launch (batch %d, %d launches per run, %d walks)" % (n, a.launches, a.reps))
    print("%-18s %9s %8s %2s %3s  " % ("net", "C (st.)", "map", "s", "x") + "  ".join("%s %s" % (f, p) for p in PASSES for f in fams))
    for i, (net, cr, cs, h, w, stride, cnt) in enumerate(shapes):
        print("%-18s %4d (%3d) %8s %2d %3d  " % (net, cr, cs, "%dx%d" % (h, w), stride, cnt) +
              "  ".join("%9.2f" % stats(per_cell[f][p][i])["median"] for p in PASSES for f in fams))
    result = {"batch": n, "launches": a.launches, "walks": a.reps, "unit": "us per step (count-weighted sum over the table)",
              "sums": {f: {p: stats(sums[f][p]) for p in PASSES} for f in fams}}
    if len(fams) == 2:
        result["verdict"] = {}
        for p in PASSES:
            d3, dk = result["sums"]["dw3"][p], result["sums"]["dwk"][p]
            result["verdict"][p] = "dwk" if dk["median"] <= d3["median"] + d3["spread"] else "dw3"
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
