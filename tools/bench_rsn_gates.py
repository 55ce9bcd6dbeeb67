"""The three gate kernels of RSN-18 "se + prm" (UDP_OP_SE_RES, UDP_OP_PRM_GATE, UDP_OP_PRM_DW9; csrc/rsn_gate.hip) on one
MI355X at the shapes they have in the net for a batch-64 flip step (128 images), split-fp16 ("f16x2") and fp32 storage.
Prints ONE JSON line per storage mode.

    python tools/bench_rsn_gates.py [--images 128] [--dtypes f16x2,f32] [--reps 100]

Each launch is timed against a UDP_OP_FUSE launch (out = relu(in + res): an existing element-wise kernel) that moves the same
three maps, in the same session: 7 alternating windows of ``--reps`` launches, device events around a window, median
[min - max].  For the depthwise 9x9 the line also carries the achieved bytes/s on its algorithmic traffic (t and out_1
read once, the result written once) and its distance from the VALU floor of 81 FMAs per output element at the chip's
peak fp32 vector rate (157.3 TFLOP/s: 78.65e12 FMA/s, MI355X data sheet).

    --once KIND   one warm-up and 20 launches of that kernel alone (se | gate | dw9 | all: the three in turn), for a kernel
                  trace in a process of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_rsn_gates.py --once all)
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from udp_pose_amd import _lib                     # noqa: E402

PEAK_FMA_PER_S = 157.3e12 / 2
H, W = 64, 48                                     # the finest level of a 256x192 crop


def _window(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _samples(fns, reps, samples=7, warm=10):
    """``samples`` timed windows per function, ALTERNATING window by window -> per function (median, min, max) ms."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(samples):
        for k, fn in enumerate(fns):
            ts[k].append(_window(fn, reps))
    return [(float(np.median(t)), min(t), max(t)) for t in ts]


def _op(kind, c, **fields):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride = kind, 1, 1
    op.cin = op.cout = op.cout_pad = c
    op.hin, op.win, op.hout, op.wout = H, W, H, W
    for k, v in fields.items():
        setattr(op, k, v)
    return op


def _map(images, c, dtype):
    """A [images, H, W, c] map of N(0, 1) values in the storage mode (4 bytes per element in both)."""
    t = torch.randn(images, H, W, c, device="cuda")
    if dtype == "f16x2":
        from udp_pose_amd import f16x2
        return f16x2.encode(t)
    return t


def launches(dtype, images):
    """{name: (callable, elements of one map)} for the three kernels and their element-wise yardsticks."""
    lib, dt, s, P = _lib.lib(), _lib.DTYPES[dtype], _lib.stream_ptr(), _lib.ptr
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *sh: torch.randn(*sh, device="cuda", generator=g)
    out = {}
    keep = []                                                                   # the tensors must outlive the closures

    def call(op, x, wgt, bias, res, up0, y):
        keep.extend([x, wgt, bias, res, up0, y])
        return lambda: _lib.check(lib.udp_conv2d_fused(C.byref(op), dt, images, P(x), P(wgt), P(bias), P(res), P(up0), None, None, P(y), s))
    for c, names in ((256, ("dw9", "gate")), (64, ("se",))):
        x, res, y = _map(images, c, dtype), _map(images, c, dtype), _map(images, c, dtype)
        elems = images * H * W * c
        fuse = _op(_lib.UDP_OP_FUSE, c, relu=1)
        out["fuse%d" % c] = (call(fuse, x, None, None, res, None, y), elems)
        if "dw9" in names:
            wt, bias, a = r(81, c) * float(np.sqrt(2.0 / 81)), r(c) * 0.1, torch.rand(images, c, device="cuda", generator=g)
            out["dw9"] = (call(_op(_lib.UDP_OP_PRM_DW9, c, ks=9, n_up=1), x, wt, bias, res, a, y), elems)
            blk = torch.cat([(r(c, c) * (2.0 / np.sqrt(c))).reshape(-1), r(c) * 0.3, (r(c, c) * (3.0 / np.sqrt(c))).reshape(-1), r(c) * 0.3])
            rows = torch.empty(images, c, device="cuda")
            out["gate"] = (call(_op(_lib.UDP_OP_PRM_GATE, c), x, blk, None, None, None, rows), elems)
        else:
            ch = c // 8
            blk = torch.cat([(r(c, ch) * (2.0 / np.sqrt(c))).reshape(-1), (r(ch, c) * (3.0 / np.sqrt(ch))).reshape(-1)])
            out["se"] = (call(_op(_lib.UDP_OP_SE_RES, c, relu=1, chain_cout=ch), x, blk, None, res, None, y), elems)
    return out


def run(dtype, images, reps):
    L = launches(dtype, images)
    order = ["dw9", "gate", "fuse256", "se", "fuse64"]
    t = dict(zip(order, _samples([L[k][0] for k in order], reps)))
    us = lambda k: {"us": round(t[k][0] * 1e3, 1), "us_min_max": [round(t[k][1] * 1e3, 1), round(t[k][2] * 1e3, 1)]}
    e256, e64 = L["dw9"][1], L["se"][1]
    res = {"dtype": dtype, "images": images, "map": [H, W], "windows": "7 alternating windows of %d launches each" % reps,
           "dw9_c256": us("dw9"), "prm_gate_c256": us("gate"), "fuse_c256": us("fuse256"), "se_res_c64": us("se"), "fuse_c64": us("fuse64")}
    res["dw9_c256"].update(over_fuse=round(t["dw9"][0] / t["fuse256"][0], 2), gbytes_per_s=round(3.0 * e256 * 4 / t["dw9"][0] / 1e6, 1),
                           valu_floor_us=round(81.0 * e256 / PEAK_FMA_PER_S * 1e6, 1),
                           over_valu_floor=round(t["dw9"][0] * 1e-3 / (81.0 * e256 / PEAK_FMA_PER_S), 2))
    res["fuse_c256"].update(gbytes_per_s=round(3.0 * e256 * 4 / t["fuse256"][0] / 1e6, 1))
    res["prm_gate_c256"].update(gbytes_per_s=round(1.0 * e256 * 4 / t["gate"][0] / 1e6, 1))            # one read of the map
    res["se_res_c64"].update(over_fuse=round(t["se"][0] / t["fuse64"][0], 2), gbytes_per_s=round(4.0 * e64 * 4 / t["se"][0] / 1e6, 1))  # 2 reads of in, res, out
    res["fuse_c64"].update(gbytes_per_s=round(3.0 * e64 * 4 / t["fuse64"][0] / 1e6, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--dtypes", default="f16x2,f32")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--once", choices=["se", "gate", "dw9", "all"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rsn_gates.py needs a GPU: a timing from anywhere else says nothing")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for dtype in a.dtypes.split(","):
        if a.once:
            L = launches(dtype, a.images)
            for k in (["se", "gate", "dw9"] if a.once == "all" else [a.once]):
                for _ in range(21):
                    L[k][0]()
            torch.cuda.synchronize()
            continue
        print(json.dumps(run(dtype, a.images, a.reps)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
