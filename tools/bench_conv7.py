"""One launch of the 7x7 stride-1 64 -> 64 conv (UDP_OP_CONV ks 7, csrc/conv7.hip) on one MI355X at the shapes of a
batch-64 flip step of RSN-18 on the conv7 stem: 128 images of 128 x 96, f32 and split fp16.  Prints ONE JSON line per
storage mode.

    python tools/bench_conv7.py [--images 128] [--dtypes f16x2,f32] [--reps 20]

The launch is timed against the existing 3x3 stride-1 64 -> 64 conv on the same map in the same session (f32: the
LDS-staged conv_mfma_kernel; f16x2: the weight-stationary kernel, wfmt 1): 7 alternating windows of ``--reps`` launches,
device events around a window, median [min - max], and the time per multiply-accumulate of both.  Two derived floors
ride along: the MFMA time of the launch's FLOPs at the measured fp32 matrix rate of 155 TFLOP/s (f32) and of three times
its FLOPs at 2.5 PFLOP/s fp16 (f16x2: three MFMAs per product).  Weights are random bytes of the right size: timing only.

    --once    one warm-up and 10 launches of the 7x7 conv alone, for a kernel trace in a process of its own
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch         # noqa: E402

from tools.bench_rsn_gates import _samples        # noqa: E402
from udp_pose_amd import _lib                     # noqa: E402

H, W, CH = 128, 96, 64


def launch(dtype, images, ks):
    g = torch.Generator("cuda").manual_seed(ks)
    mk = lambda nbytes, s: (torch.randn(nbytes // 2, device="cuda", generator=g) * s).to(torch.float16)
    x = mk(images * H * W * CH * 4, 0.5) if dtype == "f16x2" else torch.randn(images * H * W * CH, device="cuda", generator=g)
    w = mk(ks * ks * CH * CH * 4, 0.05) if dtype == "f16x2" else torch.randn(ks * ks * CH * CH, device="cuda", generator=g) * 0.05
    b = torch.zeros(CH, device="cuda")
    out = torch.empty(images * H * W * CH * 4, dtype=torch.uint8, device="cuda")
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, 1, 1
    op.cin, op.cout, op.cout_pad = CH, CH, CH
    op.hin, op.win, op.hout, op.wout = H, W, H, W
    op.wfmt = int(ks == 3 and dtype == "f16x2")
    keep = (x, w, b, out, op)
    return lambda: (keep, _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], images, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b),
                                                                 None, None, None, None, _lib.ptr(out), _lib.stream_ptr())))


def run(dtype, images, reps):
    t7, t3 = _samples([launch(dtype, images, 7), launch(dtype, images, 3)], reps)
    macs = lambda ks: float(ks * ks * CH * CH) * H * W * images
    tile = (C.c_int * 9)()
    _lib.check(_lib.lib().udp_debug_conv_tile(_lib.DTYPES[dtype], 0, 7, 1, images, H, W, CH, CH, 0, 0, tile))
    floor_ms = 2 * macs(7) / 155e12 * 1e3 if dtype == "f32" else 3 * 2 * macs(7) / 2.5e15 * 1e3
    ms = lambda t: {"ms": round(t[0], 4), "ms_min_max": [round(t[1], 4), round(t[2], 4)]}
    res = {"dtype": dtype, "images": images, "map": [H, W], "channels": CH, "windows": "7 alternating windows of %d launches each" % reps,
           "conv7x7": ms(t7), "conv3x3": ms(t3)}
    res["conv7x7"].update(tflops=round(2 * macs(7) / t7[0] / 1e9, 1), ps_per_mac=round(t7[0] * 1e9 / macs(7), 4),
                          mfma_floor_ms=round(floor_ms, 3), over_mfma_floor=round(t7[0] / floor_ms, 2),
                          tile={"nb": tile[0], "mbw": tile[1], "g": tile[2], "r": tile[3], "tw": tile[4], "lds": tile[6], "workgroups": tile[7]})
    res["conv3x3"].update(tflops=round(2 * macs(3) / t3[0] / 1e9, 1), ps_per_mac=round(t3[0] * 1e9 / macs(3), 4))
    res["time_per_mac_7x7_over_3x3"] = round((t7[0] / macs(7)) / (t3[0] / macs(3)), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--dtypes", default="f16x2,f32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv7.py needs a GPU: a timing from anywhere else says nothing")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for dtype in a.dtypes.split(","):
        if a.once:
            fn = launch(dtype, a.images, 7)
            for _ in range(11):
                fn()
            torch.cuda.synchronize()
            continue
        print(json.dumps(run(dtype, a.images, a.reps)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
