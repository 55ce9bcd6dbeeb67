#!/usr/bin/env python3
"""One line per planner configuration: label, op count, buffer count, blob bytes and the SHA-256 over the op array,
the buffer sizes and the weight blob.  CPU only, seeded synthetic weights; two trees whose outputs ``diff`` empty hand
the library byte-identical programs.  The synthetic running statistics (mean 0, variance 1) are replaced by seeded
non-trivial ones so that every term of the conv + BatchNorm fold reaches the digest.

    python tools/program_digest.py > digest.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from udp_pose_amd import synth  # noqa: E402
from udp_pose_amd.hrnet_plan import HRNetProgram  # noqa: E402
from udp_pose_amd.resnet_plan import PoseResNetProgram, pose_resnet_spec  # noqa: E402
from udp_pose_amd.rsn_plan import RSNProgram  # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_state_dict  # noqa: E402

RES_EXTRA = {"FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
             "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}
RES_LAYERS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
SWITCHES = ["UDP_POSE_NO_BLOCK_FUSION=1", "UDP_POSE_NO_GROUPS=1", "UDP_POSE_WS=0", "UDP_POSE_HEAD_WS=0",
            "UDP_POSE_NO_L1_CHAIN=1", "UDP_POSE_NO_L1_CONCAT=1", "UDP_POSE_NO_FUSE_CONCAT=1", "UDP_POSE_GROUP_FWD=1",
            "UDP_POSE_RSN_WS=0", "UDP_POSE_RSN_FUSE_ADDS=0"]


def stats(sd, seed=11):
    """Seeded running_mean ~ N(0, 0.1), running_var ~ U(0.5, 1.5) in place of the synthetic (0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.from_numpy((rng.standard_normal(tuple(sd[k].shape)) * 0.1).astype(np.float32))
        elif k.endswith("running_var"):
            sd[k] = torch.from_numpy(rng.uniform(0.5, 1.5, tuple(sd[k].shape)).astype(np.float32))
    return sd


def line(label, make, switch=""):
    name, _, value = switch.partition("=")
    if name:
        os.environ[name] = value
    try:
        prog = make()
    finally:
        if name:
            del os.environ[name]
    h = hashlib.sha256()
    blob = prog.weight_blob()
    for part in (bytes(prog.ops_array()), np.asarray(prog.buf_elems, dtype=np.int64).tobytes(), blob.tobytes()):
        h.update(part)
    print("%-52s ops %4d bufs %3d blob %10d out %3d %s" % (label + (" " + switch if switch else ""), len(prog._ops),
          len(prog.buf_elems), blob.size, prog.out_channels, h.hexdigest()), flush=True)


def main():
    hr = {t: stats(synth.synth_state_dict(synth.W32_EXTRA, 17, t, seed=1)) for t in ("gaussian", "offset")}
    for t in ("gaussian", "offset"):
        for d in ("f32", "bf16", "f16x2"):
            line("hrnet_w32 256x192 %s %s" % (t, d), lambda: HRNetProgram(hr[t], synth.W32_EXTRA, 256, 192, d))
    w48 = synth.scaled_extra(48)
    sd48 = stats(synth.synth_state_dict(w48, 17, "gaussian", seed=2))
    line("hrnet_w48 384x288 f16x2", lambda: HRNetProgram(sd48, w48, 384, 288, "f16x2"))
    for width in (16, 32):
        mini = synth.scaled_extra(width, modules=(1, 1, 1), blocks=1)
        sdm = stats(synth.synth_state_dict(mini, 17, "gaussian", seed=3))
        for d in ("f32", "bf16", "f16x2"):
            line("hrnet_mini%d 64x64 %s" % (width, d), lambda: HRNetProgram(sdm, mini, 64, 64, d))
    psa = synth.scaled_extra(32, modules=(1, 1, 1), blocks=2)
    sdp = stats(synth.synth_state_dict(psa, 17, "gaussian", seed=4, psa=True))
    for d in ("f32", "bf16", "f16x2"):
        line("hrnet_psa 128x96 %s" % d, lambda: HRNetProgram(sdp, psa, 128, 96, d))

    rsn = {c: stats(synth.synth_rsn18_state_dict(c, seed=5)) for c in (17, 51)}
    for c in (17, 51):
        for d in ("f32", "bf16", "f16x2"):
            line("rsn18 c%d 256x192 %s" % (c, d), lambda: RSNProgram(rsn[c], 256, 192, d))

    for depth, h, w in ((50, 256, 192), (101, 256, 192), (152, 256, 192), (50, 384, 288)):
        sdr = stats(synth_pose_resnet_state_dict(seed=7, layers=RES_LAYERS[depth]))
        spec = pose_resnet_spec(dict(RES_EXTRA, NUM_LAYERS=depth))
        for d in ("f32", "f16x2"):
            line("pose_resnet%d %dx%d %s" % (depth, h, w, d), lambda: PoseResNetProgram(sdr, spec, h, w, d))
    sdb = stats(synth_pose_resnet_state_dict(seed=8, final_kernel=3, deconv_with_bias=True))
    spec = pose_resnet_spec(dict(RES_EXTRA, FINAL_CONV_KERNEL=3, DECONV_WITH_BIAS=True))
    for d in ("f32", "f16x2"):
        line("pose_resnet50 k3 bias 256x192 %s" % d, lambda: PoseResNetProgram(sdb, spec, 256, 192, d))

    for sw in SWITCHES:
        line("hrnet_w32 256x192 gaussian f16x2", lambda: HRNetProgram(hr["gaussian"], synth.W32_EXTRA, 256, 192, "f16x2"), sw)
        line("rsn18 c17 256x192 f16x2", lambda: RSNProgram(rsn[17], 256, 192, "f16x2"), sw)
        line("pose_resnet50 256x192 f16x2", lambda: PoseResNetProgram(
            stats(synth_pose_resnet_state_dict(seed=7)), pose_resnet_spec(RES_EXTRA), 256, 192, "f16x2"), sw)
    for sw in ("UDP_POSE_NO_BLOCK_FUSION=1", "UDP_POSE_NO_GROUPS=1", "UDP_POSE_NO_FUSE_CONCAT=1", "UDP_POSE_GROUP_FWD=1"):
        line("hrnet_w32 256x192 gaussian bf16", lambda: HRNetProgram(hr["gaussian"], synth.W32_EXTRA, 256, 192, "bf16"), sw)


if __name__ == "__main__":
    main()
