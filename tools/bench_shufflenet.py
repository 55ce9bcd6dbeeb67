"""pose_shufflenetv2_10x_pixel_shuffle (1.0x, 256x192) throughput on one MI355X: batch 64 with the flip test and the DARK
decode, split-fp16 ("f16x2") and fp32 storage.  Prints ONE JSON line: images/s, ms per step, launches per forward, the
per-op-class kernel time of udp_hrnet_profile (hipEvents around every launch, eager) and, for the depthwise kernel,
the achieved bytes/s on its algorithmic traffic (one read and one write of the map) next to the launch time of a
UDP_OP_FUSE (an existing kernel that moves the same bytes) on a tensor of the same size, in the same session.

    python tools/bench_shufflenet.py [--steps 20] [--warmup 5] [--batch 64] [--dtypes f16x2,f32] [--model v2|plus|mobilevitv2|mobilevit|
                                         mobilenetv3|mobilenetv3_deconv|v2_deconv|plus_deconv]

``--model plus``: pose_shufflenetv2_plus_pixel_shuffle (Small) instead, with the same measurements; its depthwise
launches are classed by kernel size, and the squeeze-excitation launches and the 1x1 convs with the hard-swish
epilogue get classes of their own.

``--model mobilevitv2``: pose_mobilevitv2_pixel_shuffle (MODEL_SIZE 0.5) instead; group-norm, attention, the 1x1 convs
with the SiLU epilogue and those with a residual get classes of their own, and a UDP_OP_GNORM and a UDP_OP_LINATTN
launch on the layer-3 map (32 x 24, 64 channels; the attention reads the 160-channel qkv map) are timed against a
UDP_OP_FUSE launch on the map they read.

``--model mobilevit``: pose_mobilevit_pixel_shuffle (MODEL_SIZE xxs) instead; layer norm, multi-head attention, the
stand-alone activation launches, the 1x1 convs by epilogue and the 3x3 convs get classes of their own (no side
measurement).

``--model mobilenetv3 | mobilenetv3_deconv | v2_deconv | plus_deconv``: pose_mobilenetv3_small_pixel_shuffle,
pose_mobilenetv3_small, pose_shufflenetv2_10x (1.0x) and pose_shufflenetv2_plus (Small) instead, with the classes of
``--model plus`` plus ``se_act`` (UDP_OP_SE_ACT), ``deconv`` and ``conv1x1_res`` (the project convs with their shortcut).
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

from udp_pose_amd import _lib, synth                                        # noqa: E402
from udp_pose_amd.inference import decode_device                            # noqa: E402
from udp_pose_amd.model import MODELS                                       # noqa: E402
from udp_pose_amd.synth_shufflenet import synth_shufflenet_state_dict       # noqa: E402
from udp_pose_amd.transforms import COCO_FLIP_PAIRS, flip_fuse              # noqa: E402

NAME = "pose_shufflenetv2_10x_pixel_shuffle"
EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "1.0x", "FINAL_CONV_KERNEL": 1}
PLUS_NAME = "pose_shufflenetv2_plus_pixel_shuffle"
PLUS_EXTRA = dict(EXTRA, MODEL_SIZE="Small")
MVIT_NAME = "pose_mobilevitv2_pixel_shuffle"
MVIT_EXTRA = dict(EXTRA, MODEL_SIZE=0.5)
VIT_NAME = "pose_mobilevit_pixel_shuffle"
VIT_EXTRA = dict(EXTRA, MODEL_SIZE="xxs")
DECONV = {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4],
          "FINAL_CONV_KERNEL": 1}


def _later_nets():
    """--model choice -> (MODEL.NAME, MODEL.EXTRA, seeded state dict, workload text) of the MobileNetV3 nets and the
    deconv-head ShuffleNets."""
    from udp_pose_amd.synth_mobilenetv3 import synth_mobilenetv3_state_dict
    from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict
    from udp_pose_amd.synth_shufflenet_plus import synth_shufflenet_plus_deconv_state_dict
    return {"mobilenetv3": ("pose_mobilenetv3_small_pixel_shuffle", dict(EXTRA, MODEL_SIZE="small"),
                            lambda: synth_mobilenetv3_state_dict(seed=7), "pose_mobilenetv3_small_pixel_shuffle"),
            "mobilenetv3_deconv": ("pose_mobilenetv3_small", dict(DECONV, MODEL_SIZE="small"),
                                   lambda: synth_mobilenetv3_state_dict(seed=7, head="deconv"), "pose_mobilenetv3_small"),
            "v2_deconv": ("pose_shufflenetv2_10x", dict(DECONV, MODEL_SIZE="1.0x"), lambda: synth_shufflenet_deconv_state_dict(seed=7),
                          "pose_shufflenetv2_10x 1.0x"),
            "plus_deconv": ("pose_shufflenetv2_plus", dict(DECONV, MODEL_SIZE="Small"), lambda: synth_shufflenet_plus_deconv_state_dict(seed=7),
                            "pose_shufflenetv2_plus Small")}


LATER = ("mobilenetv3", "mobilenetv3_deconv", "v2_deconv", "plus_deconv")


def op_class(name, kind, ks, stride):
    if kind == _lib.UDP_OP_DWCONV:
        return "dwconv_s%d" % stride
    if kind == _lib.UDP_OP_PIXSHUF:
        return "pixel_shuffle"
    if kind == _lib.UDP_OP_STEM:
        return "stem"
    if kind == _lib.UDP_OP_MAXPOOL:
        return "maxpool"
    if name == "final_layer":
        return "head"
    return "conv%dx%d" % (ks, ks)


def op_class_plus(op):
    """Classes of the ShuffleNetV2+ program: as above, but depthwise launches by kernel size, UDP_OP_SE, and the 1x1
    convs whose epilogue is the hard-swish."""
    if op["kind"] == _lib.UDP_OP_DWCONV:
        return "dwconv%d_s%d" % (op["ks"], op["stride"])
    if op["kind"] == _lib.UDP_OP_SE:
        return "se"
    if op["kind"] == _lib.UDP_OP_SE_ACT:
        return "se_act"
    if op["kind"] == _lib.UDP_OP_DECONV:
        return "deconv"
    if op["kind"] == _lib.UDP_OP_CONV and op["ks"] == 1 and op["res"] is not None:
        return "conv1x1_res"
    if op["kind"] == _lib.UDP_OP_CONV and op["relu"] == _lib.UDP_ACT_HSWISH:
        return "conv1x1_hs"
    return op_class(op["name"], op["kind"], op["ks"], op["stride"])


def op_class_mvit(op):
    """Classes of the MobileViTv2 program: group norm, attention, depthwise by stride, and the 1x1 convs by epilogue."""
    if op["kind"] == _lib.UDP_OP_GNORM:
        return "gnorm"
    if op["kind"] == _lib.UDP_OP_LINATTN:
        return "linattn"
    if op["kind"] == _lib.UDP_OP_CONV and op["ks"] == 1 and op["name"] != "final_layer":
        return "conv1x1_silu" if op["relu"] == _lib.UDP_ACT_SILU else "conv1x1_res" if op["res"] is not None else "conv1x1"
    return op_class(op["name"], op["kind"], op["ks"], op["stride"])


def op_class_vit(op):
    """Classes of the MobileViT program: layer norm, multi-head attention, the activation launches, else as MobileViTv2."""
    cls = {_lib.UDP_OP_LNORM: "lnorm", _lib.UDP_OP_MHATTN: "mhattn", _lib.UDP_OP_ACT: "act"}.get(op["kind"])
    return cls or op_class_mvit(op)


def _window(fn, reps):
    """Milliseconds per call of one timed window of ``reps`` calls (device events around the window)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def _samples(fns, reps, samples=7, warm=20):
    """``samples`` timed windows per function, the functions ALTERNATING window by window (other work shares the host
    and the chip: a drift hits all of them alike) -> per function (median, min, max) ms per call."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(samples):
        for k, fn in enumerate(fns):
            ts[k].append(_window(fn, reps))
    return [(float(np.median(t)), min(t), max(t)) for t in ts]


def dw_vs_fuse(dtype, images, c=128, h=32, w=24):
    """One stride-1 depthwise launch (the stage-2 map of the 1.0x net: 2 x 64 stored channels) against one UDP_OP_FUSE
    launch (out = relu(in)) on a tensor of the same size; both read the map once and write it once."""
    lib, dt = _lib.lib(), _lib.DTYPES[dtype]
    elems = images * h * w * c
    a = torch.randn(elems, device="cuda").to(torch.float32)                 # 4 bytes per element in both modes
    b = torch.empty_like(a)
    wt, bias = torch.randn(9 * c, device="cuda"), torch.randn(c, device="cuda")
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.cin, op.cout, op.cout_pad = _lib.UDP_OP_DWCONV, 3, 1, c, c, c
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    fu = _lib.ConvOp()
    fu.kind, fu.ks, fu.stride, fu.relu, fu.cin, fu.cout, fu.cout_pad = _lib.UDP_OP_FUSE, 1, 1, 1, c, c, c
    fu.hin, fu.win, fu.hout, fu.wout = h, w, h, w
    if dtype == "f16x2":
        a.view(torch.float16).fill_(0.5)
    s = _lib.stream_ptr()
    run = lambda o, wp, bp: _lib.check(lib.udp_conv2d_fused(C.byref(o), dt, images, _lib.ptr(a), wp, bp, None, None, None, None, _lib.ptr(b), s))
    (ms_dw, dw_lo, dw_hi), (ms_fu, fu_lo, fu_hi) = _samples(
        [lambda: run(op, _lib.ptr(wt), _lib.ptr(bias)), lambda: run(fu, None, None)], reps=300)
    nbytes = 2.0 * elems * 4
    return {"shape": [images, h, w, c], "windows": "7 alternating windows of 300 launches each",
            "dw_us": round(ms_dw * 1e3, 2), "dw_us_min_max": [round(dw_lo * 1e3, 2), round(dw_hi * 1e3, 2)],
            "fuse_us": round(ms_fu * 1e3, 2), "fuse_us_min_max": [round(fu_lo * 1e3, 2), round(fu_hi * 1e3, 2)],
            "dw_over_fuse": round(ms_dw / ms_fu, 3), "dw_gbytes_per_s": round(nbytes / ms_dw / 1e6, 1),
            "fuse_gbytes_per_s": round(nbytes / ms_fu / 1e6, 1)}


def attn_vs_fuse(dtype, images, c=64, h=32, w=24):
    """One UDP_OP_GNORM launch and one UDP_OP_LINATTN launch on the layer-3 map of the 0.5 net, each against a UDP_OP_FUSE
    launch (out = relu(in)) on the map it reads: [h, w, c] for the norm, the [h, w, 2c + 32] qkv map for the attention."""
    lib, dt = _lib.lib(), _lib.DTYPES[dtype]
    cq = 2 * c + 32
    a = torch.randn(images * h * w * cq, device="cuda").to(torch.float32)    # 4 bytes per element in both modes
    if dtype == "f16x2":
        a.view(torch.float16).fill_(0.5)
    b = torch.empty_like(a)
    block = torch.ones(2 * c, device="cuda")

    def mk(kind, cin, cout, **kw):
        o = _lib.ConvOp()
        o.kind, o.ks, o.stride, o.cin, o.cout, o.cout_pad = kind, 1, 1, cin, cout, cout
        o.hin, o.win, o.hout, o.wout = h, w, h, w
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    gn, la = mk(_lib.UDP_OP_GNORM, c, c, chain_cout=c), mk(_lib.UDP_OP_LINATTN, cq, c, ks=2)
    fu, fuq = mk(_lib.UDP_OP_FUSE, c, c, relu=1), mk(_lib.UDP_OP_FUSE, cq, cq, relu=1)
    s = _lib.stream_ptr()
    run = lambda o, wp: _lib.check(lib.udp_conv2d_fused(C.byref(o), dt, images, _lib.ptr(a), wp, None, None, None, None, None, _lib.ptr(b), s))
    t = _samples([lambda: run(gn, _lib.ptr(block)), lambda: run(fu, None), lambda: run(la, None), lambda: run(fuq, None)], reps=300)
    us = lambda k: round(t[k][0] * 1e3, 2)
    return {"shape": [images, h, w, c], "qkv_channels": cq, "windows": "7 alternating windows of 300 launches each",
            "gnorm_us": us(0), "fuse_us": us(1), "gnorm_over_fuse": round(t[0][0] / t[1][0], 3),
            "linattn_us": us(2), "fuse_qkv_us": us(3), "linattn_over_fuse_qkv": round(t[2][0] / t[3][0], 3),
            "us_min_max": [[round(lo * 1e3, 2), round(hi * 1e3, 2)] for _, lo, hi in t]}


def run(dtype, n, steps, warmup, plus=False, mvit=False, vit=False, later=None):
    name = VIT_NAME if vit else MVIT_NAME if mvit else PLUS_NAME if plus else NAME
    cfg = {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian",
                     "EXTRA": VIT_EXTRA if vit else MVIT_EXTRA if mvit else PLUS_EXTRA if plus else EXTRA}}
    if later:
        name, extra, make_sd, _ = _later_nets()[later]
        cfg["MODEL"].update(NAME=name, EXTRA=extra)
        sd = make_sd()
        plus = True                  # the classes of op_class_plus (with se_act, deconv and the residual 1x1 convs)
    elif vit:
        from udp_pose_amd.synth_mobilevit import synth_mobilevit_state_dict
        sd = synth_mobilevit_state_dict(seed=7)
    elif mvit:
        from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict
        sd = synth_mobilevitv2_state_dict(seed=7)
    elif plus:
        from udp_pose_amd.synth_shufflenet_plus import synth_shufflenet_plus_state_dict
        sd = synth_shufflenet_plus_state_dict(seed=7)
    else:
        sd = synth_shufflenet_state_dict(seed=7)
    net = MODELS[name](cfg, is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()
    x = torch.from_numpy(synth.synth_crops(n, 256, 192, seed=3)).cuda()
    c, s = synth.synth_center_scale(n, seed=1)
    c, s = torch.from_numpy(c.astype(np.float64)).cuda(), torch.from_numpy(s.astype(np.float64)).cuda()

    def step():
        raw = net.raw_forward(x, flip_test=True)
        hm = flip_fuse(raw[:n], raw[n:], COCO_FLIP_PAIRS, False)
        return decode_device(hm, c, s, "gaussian", True, 4.0, True)

    (ms, ms_lo, ms_hi), = _samples([step], reps=steps, samples=5, warm=warmup)
    handle, _, prog = net._compiled[(256, 192)]
    lib = _lib.lib()
    net.profile(x, flip_test=True)
    ms_op, desc = net.profile(x, flip_test=True)           # second run: warm caches, kernels loaded
    classes = {}
    for k, ((name, kind, ks, stride, cin, cout, hout, wout), t) in enumerate(zip(desc, ms_op)):
        cls = op_class_vit(prog._ops[k]) if vit else op_class_mvit(prog._ops[k]) if mvit else op_class_plus(prog._ops[k]) if plus else op_class(name, kind, ks, stride)
        e = classes.setdefault(cls, {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += float(t)
    total = sum(e["ms"] for e in classes.values())
    for e in classes.values():
        e["share"] = round(e["ms"] / total, 4)
        e["ms"] = round(e["ms"], 4)
    side = {} if vit else {"attn_vs_fuse": attn_vs_fuse(dtype, 2 * n)} if mvit else {"dwconv_vs_fuse": dw_vs_fuse(dtype, 2 * n)}
    return {"dtype": dtype, "images_per_s": round(n / ms * 1000.0, 1), "ms_per_step": round(ms, 3),
            "ms_per_step_min_max": [round(ms_lo, 3), round(ms_hi, 3)], "windows": "5 windows of %d steps, median" % steps,
            "launches_per_forward": int(lib.udp_hrnet_num_launches(handle)),
            "gflop_per_image": round(lib.udp_hrnet_flops_per_image(handle) / 1e9, 3),
            "kernel_ms_profiled": round(total, 3), "by_class": classes, **side}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtypes", default="f16x2,f32")
    ap.add_argument("--model", choices=("v2", "plus", "mobilevitv2", "mobilevit") + LATER, default="v2")
    a = ap.parse_args()
    plus, mvit, vit = a.model == "plus", a.model == "mobilevitv2", a.model == "mobilevit"
    later = a.model if a.model in LATER else None
    res = [run(d, a.batch, a.steps, a.warmup, plus, mvit, vit, later) for d in a.dtypes.split(",")]
    workload = (_later_nets()[later][3] if later else "pose_mobilevit_pixel_shuffle xxs" if vit else "pose_mobilevitv2_pixel_shuffle 0.5" if mvit else "pose_shufflenetv2_plus_pixel_shuffle Small" if plus
                else "pose_shufflenetv2_10x_pixel_shuffle 1.0x")
    out = {"workload": workload + " 256x192 flip-test + DARK decode", "batch": a.batch, "results": res}
    if len(res) == 2:
        out["f16x2_over_f32"] = round(res[0]["images_per_s"] / res[1]["images_per_s"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
