#!/usr/bin/env python3
"""Writes tests/golden/dw3_train_parent_bits.npz: what the one-pixel-per-thread 3x3 depthwise training kernels
(udp_dwconv3_*) computed, bit for bit, before the library kept udp_dwconvk_* alone.

    python tools/gen_golden_dw3_parent.py [--out tests/golden/dw3_train_parent_bits.npz]

It runs on a GPU against a library that still exports udp_dwconv3_train_fwd (the commit before the one that removed it)
and refuses any other.  tests/test_gpu_mobilenetv3_train_ops.py replays the recorded inputs through udp_dwconvk_*(ks=3) and
asks for the same bits.

Every array is the int32 bit pattern of an fp32 buffer as the kernels see it (NHWC, stored channels, zero pads):
  a_*      stored / real channels 32 / 24, 3 x 7 x 9, for s in (1, 2): forward, input gradient with accumulate 0 and 1
           (onto a_prev) and the weight gradient with the full workspace
  b_*      64 / 58, 3 x 7 x 9, stride 1: the weight gradient with room for 5 partials (21 rows in runs of 5, 5, 5, 5, 1)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dw3_train_parent_bits.npz"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from udp_pose_amd import _lib
    L = _lib.lib()
    if not hasattr(L, "udp_dwconv3_train_fwd"):
        raise SystemExit("this library has no udp_dwconv3_train_fwd: the fixture is a record of the kernels it no longer has")
    F32, st = _lib.UDP_F32, _lib.stream_ptr()
    gen = torch.Generator().manual_seed(20)

    def nhwc(n, h, w, cs, cr):
        t = torch.zeros(n, h, w, cs)
        t[..., :cr] = torch.randn(n, h, w, cr, generator=gen)
        return t.cuda()

    def bits(t):
        torch.cuda.synchronize()
        return t.cpu().contiguous().view(torch.int32).numpy()

    out = {}
    n, h, w = 3, 7, 9
    cs, cr = 32, 24
    x, prev, wt = nhwc(n, h, w, cs, cr), nhwc(n, h, w, cs, cr), torch.randn(cr * 9, generator=gen).cuda()
    out.update(a_x=bits(x), a_prev=bits(prev), a_w=bits(wt))
    for s in (1, 2):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        dy = nhwc(n, ho, wo, cs, cr)
        y, dx0, dx1, dw = torch.empty_like(dy), torch.empty_like(x), prev.clone(), torch.empty(cr * 9, device="cuda")
        ws = torch.empty(int(L.udp_dwconv3_wgrad_workspace_bytes(n, ho, wo, cs)), dtype=torch.uint8, device="cuda")
        _lib.check(L.udp_dwconv3_train_fwd(x.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, s, F32, y.data_ptr(), st))
        _lib.check(L.udp_dwconv3_dgrad(dy.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, s, 0, F32, dx0.data_ptr(), st))
        _lib.check(L.udp_dwconv3_dgrad(dy.data_ptr(), wt.data_ptr(), n, h, w, cs, cr, s, 1, F32, dx1.data_ptr(), st))
        _lib.check(L.udp_dwconv3_wgrad(x.data_ptr(), dy.data_ptr(), n, h, w, cs, cr, s, F32, dw.data_ptr(), ws.data_ptr(), ws.numel(), st))
        out.update({"a_dy_s%d" % s: bits(dy), "a_y_s%d" % s: bits(y), "a_dx_acc0_s%d" % s: bits(dx0),
                    "a_dx_acc1_s%d" % s: bits(dx1), "a_dw_s%d" % s: bits(dw)})
    cs, cr = 64, 58
    x, dy, dw = nhwc(n, h, w, cs, cr), nhwc(n, h, w, cs, cr), torch.empty(cr * 9, device="cuda")
    ws = torch.empty(5 * 9 * cs * 4, dtype=torch.uint8, device="cuda")
    _lib.check(L.udp_dwconv3_wgrad(x.data_ptr(), dy.data_ptr(), n, h, w, cs, cr, 1, F32, dw.data_ptr(), ws.data_ptr(), ws.numel(), st))
    out.update(b_x=bits(x), b_dy=bits(dy), b_dw_ws5=bits(dw))
    np.savez_compressed(a.out, **out)
    print("%s: %d arrays, %d bytes" % (a.out, len(out), os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
