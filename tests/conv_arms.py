"""The case table of the conv tile-arm tests (test_conv_arms_cpu.py, test_gpu_conv_arms.py).

Both conv families of the library are template matrices, and a host-side chooser picks the instantiation ("arm") from
the map size and the batch:

  * weight-stationary split fp16 (csrc/conv_ws.hip): conv_ws_h2_kernel<KS, STRIDE, PB, CP, NCHW> and
    conv_ws_hs_kernel<PB, CP, ACT>, arm = (PB, CP): pixel blocks per wave, cout pairs per workgroup;
  * LDS-staged (csrc/conv.hip): conv_mfma_kernel<T, KS, STRIDE, NB, MBW, NCHW, NW> and conv_mfma_persist1 (bf16), arm =
    (NB, MBW): 16-channel cout blocks per workgroup, pixel blocks per wave.

A row names one udp_conv2d_fused call and the arm it must reach.  The arm is forced with the choosers' own knobs
(read with getenv at every call): UDP_POSE_WS_PB / UDP_POSE_WS_CP cap the weight-stationary candidate (the arm that
runs is the smallest instantiated block count covering the tile, so a forced 6 on a small map reports less),
UDP_POSE_MINWGS / UDP_POSE_MAXM steer the LDS-staged chooser.  ``decide(row)`` asks the library's host-only diagnostic
udp_debug_conv_tile what the choosers do with the row; it needs no GPU.

h and w are the OUTPUT map; the input is stride x as large.  Maps stay at or below 40 x 40 and N at or below 5, with
two exceptions the arms themselves force: the 6-block one-pair arm of the 1x1 stride-2 family needs a tile of more
than 256 pixels whose stride-2 halo stays under the 640-row staging cap (one row of 52 columns x 5 images), and the
persistent bf16 form needs at least 2048 tiles.
"""
import collections
import ctypes as C
import os

from udp_pose_amd import _lib

HS, SILU = _lib.UDP_ACT_HSWISH, _lib.UDP_ACT_SILU

Row = collections.namedtuple("Row", "id fam dtype ks stride nchw env n h w cin cout res act views arm group feats")
# fam: "ws" (wfmt 1) | "hs" (wfmt 1, hard-swish / SiLU) | "lds" (wfmt 0);  dtype: storage mode;  act: udp_conv_op.relu
# views: residual and output are channel slices of wider tensors (NaN / POISON outside);  arm: (PB, CP) | (NB, MBW)
# group: rows of one group run on identical operands and must store bit-equal outputs;  feats: what the tile must show

WS_FAMILIES = [(3, 1, 0), (3, 1, 1), (3, 2, 0), (1, 1, 0), (1, 1, 1), (1, 2, 0)]          # (ks, stride, nchw)
LDS_FORMS = WS_FAMILIES
ARMS_WS = [(pb, cp) for pb in (2, 3, 4, 6) for cp in (1, 2, 4)]
ARMS_LDS = [(nb, mbw) for nb in (2, 4) for mbw in (1, 2, 3, 4)]
SHARED_WS = (2, 26, 40, 48)          # N, Hout, Wout, Cin: a ragged K chunk (48 = 32 + 16); Cout 128 = four cout pairs
SHARED_LDS = (3, 13, 24, 48)

# the arm each forced (PB, CP) reaches on the shared map, where it is not the forced one
_SHARED_WS_REACH = {
    (3, 1, 0): {(4, 1): (3, 1)},
    (3, 1, 1): {(4, 1): (3, 1)},
    (3, 2, 0): {(3, 1): (2, 1), (4, 1): (2, 1), (6, 1): (2, 1), (6, 2): (3, 2)},
    (1, 1, 0): {(4, 1): (3, 1), (4, 4): (3, 4)},
    (1, 1, 1): {(4, 1): (3, 1), (4, 4): (3, 4)},
    (1, 2, 0): {(4, 1): (2, 1), (4, 2): (3, 2), (4, 4): (3, 4), (6, 1): (2, 1)},
}
# (forced, (N, Hout, Wout, Cin), arm, feats): arms the shared map does not reach, then the feature rows
_STD_WS = [((6, 2), (3, 5, 13, 32), (6, 2), ("raggedG",)),
           ((6, 4), (1, 13, 25, 32), (6, 4), ("raggedRW",))]
_R34 = lambda h, w: [((3, 4), (1, h, w, 32), (3, 4), ("raggedRW",))]
_EXTRA_WS = {
    (3, 1, 0): [((4, 1), (1, 5, 39, 32), (4, 1), ()),
                ((4, 1), (5, 4, 13, 32), (4, 1), ("raggedG",)),
                ((6, 4), (1, 26, 28, 32), (6, 4), ("raggedRW",)),
                ((6, 2), (5, 1, 26, 48), (6, 2), ("sbuf",)),
                ((3, 1), (5, 4, 9, 48), (3, 1), ("sbuf",))] + _STD_WS + _R34(13, 26),
    (3, 1, 1): [((4, 1), (1, 5, 39, 32), (4, 1), ())] + _STD_WS + _R34(13, 26),
    (3, 2, 0): [((3, 1), (1, 5, 26, 48), (3, 1), ("sbuf",)),
                ((6, 2), (1, 5, 26, 48), (6, 2), ("sbuf",)),
                ((3, 2), (2, 5, 7, 48), (3, 2), ("sbuf",)),
                ((6, 2), (5, 5, 9, 32), (6, 2), ("halo", "raggedG")),
                ((6, 2), (5, 4, 11, 32), (6, 2), ("halo", "raggedG"))] + _STD_WS + _R34(13, 26),
    (1, 1, 0): [((4, 1), (1, 5, 39, 32), (4, 1), ()),
                ((4, 4), (1, 7, 7, 32), (4, 4), ())] + _STD_WS + _R34(13, 17),
    (1, 1, 1): [((4, 1), (1, 5, 39, 32), (4, 1), ()),
                ((4, 4), (1, 7, 7, 32), (4, 4), ())] + _STD_WS + _R34(13, 17),
    (1, 2, 0): [((4, 1), (5, 1, 39, 32), (4, 1), ()),
                ((4, 2), (1, 7, 14, 32), (4, 2), ()),
                ((4, 4), (1, 7, 7, 32), (4, 4), ()),
                ((6, 1), (5, 1, 52, 16), (6, 1), ()),
                ((6, 4), (1, 10, 9, 48), (6, 4), ("sbuf",)),
                ((6, 2), (5, 4, 12, 32), (6, 2), ("halo", "raggedG"))] + _STD_WS + _R34(19, 17),
}
# NCHW families with 17 and 51 output channels (one and two cout pairs; the shared map runs 100): (forced, shape, arm)
_NCHW_COUT = [(17, (6, 1), (1, 7, 37, 32), (6, 1)), (17, (3, 1), (1, 5, 26, 32), (3, 1)),
              (51, (6, 2), (1, 5, 26, 32), (6, 2)), (51, (3, 2), (3, 5, 13, 48), (3, 2))]

# LDS-staged: (MAXM, (N, Hout, Wout, Cin), Cout, arm) with UDP_POSE_MINWGS=0, the arms the shared map does not reach
_S2_LDS = [(128, (5, 1, 21, 16), 32, (2, 2)), (192, (3, 5, 13, 16), 32, (2, 3)), (64, (1, 5, 1, 16), 64, (4, 1)),
           (128, (5, 1, 21, 16), 64, (4, 2)), (192, (3, 5, 13, 16), 64, (4, 3))]
_NB4_LDS = [(64, (5, 1, 1, 16), 64, (4, 1)), (128, (1, 5, 26, 16), 64, (4, 2)), (192, (1, 5, 39, 16), 64, (4, 3)),
            (256, (1, 7, 37, 16), 64, (4, 4))]
_K1S2_LDS = [(192, (5, 5, 7, 16), 32, (2, 3)), (256, (5, 1, 39, 16), 32, (2, 4)), (192, (5, 5, 7, 16), 64, (4, 3)),
             (256, (5, 1, 39, 16), 64, (4, 4))]
_EXTRA_LDS = {
    "f32": {(3, 1, 0): _NB4_LDS, (3, 1, 1): _NB4_LDS, (3, 2, 0): _S2_LDS, (1, 2, 0): _K1S2_LDS},
    "f16x2": {(3, 1, 0): _NB4_LDS[:1], (3, 1, 1): _NB4_LDS[:1],
              (3, 2, 0): [(128, (1, 5, 22, 16), 32, (2, 2)), (64, (1, 5, 1, 16), 64, (4, 1))], (1, 2, 0): _K1S2_LDS},
    "bf16": {(3, 1, 0): _NB4_LDS, (3, 1, 1): _NB4_LDS, (3, 2, 0): _S2_LDS, (1, 2, 0): _K1S2_LDS},
}
# the arm the shared LDS map reaches under MAXM = 64, 128, 192, 256 (NB: 4 with MINWGS=0 where the family allows it)
_SHARED_LDS_MBW = {(3, 1): (1, 2, 3, 4), (1, 1): (1, 2, 3, 4), (1, 2): (1, 2, 2, 2)}
# 3x3 stride 2 on SHARED_LDS has one tile whatever MAXM (2 rows of 24 columns fill the staging cap); its shared map is
# smaller, with one K chunk.  Arms by (split fp16?, MINWGS=0?) under MAXM = 64, 128, 192, 256
SHARED_LDS_S2 = (3, 5, 13, 16)
_SHARED_LDS_S2_ARMS = {(False, True): ((4, 1), (4, 2), (4, 3), (4, 3)), (False, False): ((2, 1), (2, 2), (2, 2), (2, 2)),
                       (True, True): ((2, 1), (2, 1), (2, 1), (2, 1)), (True, False): ((2, 1), (2, 2), (2, 2), (2, 2))}

# Arms the scan of test_conv_arms_cpu.py must find NO shape for (instantiated, never chosen), with the reason.
UNREACHABLE_WS = {
    (3, 2, 0): {(4, 1): "a one-pair tile of more than 192 output pixels has a stride-2 halo above the 640-row staging cap",
                (6, 1): "a one-pair tile of more than 192 output pixels has a stride-2 halo above the 640-row staging cap"},
}
_H2_NB4 = "split fp16 keeps one stage buffer under 76 KB: 72 KB of 3x3 weight rows for 4 cout blocks leave 16 halo rows"
_S2_M4 = "a tile of more than 192 output pixels has a 3x3 stride-2 halo above the 640-row staging cap"
UNREACHABLE_LDS = {
    ("f32", 3, 2, 0): {(2, 4): _S2_M4, (4, 4): _S2_M4},
    ("bf16", 3, 2, 0): {(2, 4): _S2_M4, (4, 4): _S2_M4},
    ("f16x2", 3, 1, 0): {(4, 2): _H2_NB4, (4, 3): _H2_NB4, (4, 4): _H2_NB4},
    ("f16x2", 3, 1, 1): {(4, 2): _H2_NB4, (4, 3): _H2_NB4, (4, 4): _H2_NB4},
    ("f16x2", 3, 2, 0): {(2, 3): "two planes of a stride-2 halo tile of more than 128 output pixels exceed the 76 KB of one stage buffer",
                         (2, 4): _S2_M4, (4, 2): _H2_NB4, (4, 3): _H2_NB4, (4, 4): _H2_NB4},
}


def _tag(ks, stride, nchw):
    return "k%ds%d%s" % (ks, stride, "o" if nchw else "")


def _ws_rows():
    rows = []
    for fam in WS_FAMILIES:
        ks, stride, nchw = fam
        t = _tag(*fam)
        n, h, w, cin = SHARED_WS
        for pb, cp in ARMS_WS:
            env = {"UDP_POSE_WS_PB": str(pb), "UDP_POSE_WS_CP": str(cp)}
            arm = _SHARED_WS_REACH[fam].get((pb, cp), (pb, cp))
            rows.append(Row("ws-%s-shared-f%d.%d" % (t, pb, cp), "ws", "f16x2", ks, stride, nchw, env, n, h, w, cin,
                            100 if nchw else 128, not nchw, 0 if nchw else 1, False, arm, "ws-" + t, ()))
        for (pb, cp), (n, h, w, cin), arm, feats in _EXTRA_WS[fam]:
            env = {"UDP_POSE_WS_PB": str(pb), "UDP_POSE_WS_CP": str(cp)}
            rows.append(Row("ws-%s-n%d_%dx%d_c%d-f%d.%d" % (t, n, h, w, cin, pb, cp), "ws", "f16x2", ks, stride, nchw, env, n, h, w,
                            cin, 100 if nchw else 128, not nchw, 0 if nchw else 1, False, arm, None, feats))
        if nchw:
            for cout, (pb, cp), (n, h, w, cin), arm in _NCHW_COUT:
                env = {"UDP_POSE_WS_PB": str(pb), "UDP_POSE_WS_CP": str(cp)}
                rows.append(Row("ws-%s-cout%d-f%d.%d" % (t, cout, pb, cp), "ws", "f16x2", ks, stride, nchw, env, n, h, w, cin, cout,
                                False, 0, False, arm, None, ()))
        else:
            # the residual is channels 16..143 of a 160-channel tensor that is NaN elsewhere, the output channels 32..159
            # of a 192-channel tensor; three images in tiles of one, on the 6-block four-pair arm
            env = {"UDP_POSE_WS_PB": "6", "UDP_POSE_WS_CP": "4"}
            rows.append(Row("ws-%s-views-f6.4" % t, "ws", "f16x2", ks, stride, nchw, env, 3, 5, 13, 32, 128, True, 1, True, (6, 4),
                            None, ()))
    return rows


def _hs_rows():
    rows = []
    n, h, w, cin = SHARED_WS
    for act, name in ((HS, "hswish"), (SILU, "silu")):
        for pb, cp in ARMS_WS:
            env = {"UDP_POSE_WS_PB": str(pb), "UDP_POSE_WS_CP": str(cp)}
            arm = _SHARED_WS_REACH[(1, 1, 0)].get((pb, cp), (pb, cp))
            rows.append(Row("hs-%s-shared-f%d.%d" % (name, pb, cp), "hs", "f16x2", 1, 1, 0, env, n, h, w, cin, 128, False, act, False,
                            arm, "hs-" + name, ()))
        for (pb, cp), (n2, h2, w2, cin2), arm, feats in _EXTRA_WS[(1, 1, 0)]:
            env = {"UDP_POSE_WS_PB": str(pb), "UDP_POSE_WS_CP": str(cp)}
            rows.append(Row("hs-%s-n%d_%dx%d_c%d-f%d.%d" % (name, n2, h2, w2, cin2, pb, cp), "hs", "f16x2", 1, 1, 0, env, n2, h2, w2,
                            cin2, 128, False, act, False, arm, None, feats))
    return rows


def _lds_rows():
    rows = []
    for dtype in ("f32", "f16x2", "bf16"):
        for form in LDS_FORMS:
            ks, stride, nchw = form
            t = _tag(*form)
            n, h, w, cin = SHARED_LDS
            nb4 = 4 if ks == 1 else 2         # 3x3: the weight rows of 4 cout blocks do not fit beside two stages of the tile
            if form == (3, 2, 0):
                n, h, w, cin = SHARED_LDS_S2
            for minwgs in ("0", None):
                for i, maxm in enumerate((64, 128, 192, 256)):
                    env = {"UDP_POSE_MAXM": str(maxm)}
                    if minwgs is not None:
                        env["UDP_POSE_MINWGS"] = minwgs
                    if form == (3, 2, 0):
                        arm = _SHARED_LDS_S2_ARMS[dtype == "f16x2", minwgs is not None][i]
                    else:
                        arm = (nb4 if minwgs is not None else 2, _SHARED_LDS_MBW[(ks, stride)][i])
                    rows.append(Row("lds-%s-%s-shared-w%s-m%d" % (dtype, t, minwgs or "dflt", maxm), "lds", dtype, ks, stride, nchw, env,
                                    n, h, w, cin, 100 if nchw else 64, not nchw, 0 if nchw else 1, False, arm,
                                    "lds-%s-%s" % (dtype, t), ()))
            for maxm, (n2, h2, w2, cin2), cout, arm in _EXTRA_LDS[dtype].get(form, []):
                env = {"UDP_POSE_MAXM": str(maxm), "UDP_POSE_MINWGS": "0"}
                cout = 100 if nchw and cout == 64 else 17 if nchw else cout
                rows.append(Row("lds-%s-%s-n%d_%dx%d_c%d-%d-m%d" % (dtype, t, n2, h2, w2, cin2, cout, maxm), "lds", dtype, ks, stride, nchw,
                                env, n2, h2, w2, cin2, cout, not nchw, 0 if nchw else 1, False, arm, None, ()))
            if form == (1, 1, 0) and dtype != "bf16":
                # conv1x1_hs_kernel<T, NB, MBW, ACT>: the 1x1 stride-1 chooser, so the shared map reaches all eight arms
                for act, name in ((HS, "hswish"), (SILU, "silu")):
                    for minwgs in ("0", None):
                        for maxm, mbw in zip((64, 128, 192, 256), (1, 2, 3, 4)):
                            env = {"UDP_POSE_MAXM": str(maxm)}
                            if minwgs is not None:
                                env["UDP_POSE_MINWGS"] = minwgs
                            rows.append(Row("lds-%s-%s-shared-w%s-m%d" % (dtype, name, minwgs or "dflt", maxm), "lds", dtype, 1, 1, 0, env,
                                            n, h, w, cin, 64, False, act, False, (4 if minwgs is not None else 2, mbw),
                                            "lds-%s-%s" % (dtype, name), ()))
            if nchw:
                for cout, nb in ((17, 2), (51, 4 if ks == 1 else 2)):
                    env = {"UDP_POSE_MAXM": "256", "UDP_POSE_MINWGS": "0"}
                    rows.append(Row("lds-%s-%s-cout%d" % (dtype, t, cout), "lds", dtype, ks, stride, nchw, env, n, h, w, cin, cout, False, 0,
                                    False, (nb, 4), None, ()))
            elif stride == 1:
                env = {"UDP_POSE_MAXM": "192", "UDP_POSE_MINWGS": "0"}
                one = ks == 3 and dtype != "bf16"       # (two stages of fp32 / two planes of split fp16: one image per tile)
                rows.append(Row("lds-%s-%s-views" % (dtype, t), "lds", dtype, ks, stride, nchw, env, 3, 5, 13, 32, 64, True, 1, True,
                                (2, 2) if one else (4, 3), None, () if one else ("raggedG",)))
    # the persistent bf16 form with two tiles per workgroup: 128 images of 32 x 32 in tiles of 2 rows -> 2048 tiles on
    # 1024 workgroups (4 per CU on 256 CUs, one cout block)
    rows.append(Row("lds-bf16-k3s1-persist", "lds", "bf16", 3, 1, 0, {"UDP_POSE_MAXM": "64"}, 128, 32, 32, 32, 32, True, 1, False, (2, 1),
                    None, ("persist2",)))
    return rows


ROWS = _ws_rows() + _hs_rows() + _lds_rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS), "duplicate row ids"


class env_knobs:
    """Set the chooser knobs around one call and restore the environment (the _env helper of test_gpu_ws_pb8.py); every knob
    the choosers read per call that the row does not name is removed for the duration."""
    KNOBS = ("UDP_POSE_WS_PB", "UDP_POSE_WS_CP", "UDP_POSE_MINWGS", "UDP_POSE_MAXM", "UDP_POSE_LDS_KB", "UDP_POSE_NO_PERSIST",
             "UDP_POSE_DEBUG_TILES")

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.KNOBS}
        for k in self.KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


Tile = collections.namedtuple("Tile", "arm G R TW sbuf lds wgs persist")


def debug_tile(dtype, wfmt, ks, stride, n, h, w, cin, cout, nchw=0, grouped=0):
    """udp_debug_conv_tile under the current environment: a Tile, or None when the library refuses the conv."""
    out = (C.c_int * 9)()
    rc = _lib.lib().udp_debug_conv_tile(_lib.DTYPES[dtype], wfmt, ks, stride, n, h, w, cin, cout, nchw, grouped, out)
    return None if rc else Tile((out[0], out[1]), out[2], out[3], out[4], out[5], out[6], out[7], out[8])


def decide(row):
    """What the library's choosers do with ``row`` under its knobs."""
    with env_knobs(**row.env):
        return debug_tile(row.dtype, int(row.fam != "lds"), row.ks, row.stride, row.n, row.h, row.w, row.cin, row.cout, row.nchw)


def has_feature(row, t, feat):
    """The tile properties the feature rows exist for."""
    halo = lambda g: g * ((t.R - 1) * row.stride + row.ks) * ((t.TW - 1) * row.stride + row.ks)
    if feat == "raggedG":                # more than one image per tile, and a last tile with fewer
        return t.G > 1 and row.n % t.G != 0
    if feat == "raggedRW":               # a column split and a row split, both with a ragged last tile
        return row.h % t.R != 0 and row.w % t.TW != 0
    if feat == "sbuf":
        return t.sbuf == 1
    if feat == "halo":                   # one more image would fit the wave's pixel blocks, but not the 640 staged halo rows
        max_m = 16 * int(row.env["UDP_POSE_WS_PB"]) * (4 // int(row.env["UDP_POSE_WS_CP"]))
        return t.R == row.h and t.TW == row.w and t.G < row.n and (t.G + 1) * t.R * t.TW <= max_m and halo(t.G + 1) > 640
    if feat == "persist2":               # conv_mfma_persist1 with at least two tiles on every workgroup
        tiles = -(-row.n // t.G) * -(-row.h // t.R) * -(-row.w // t.TW)
        return t.persist > 0 and tiles >= 2 * t.persist
    raise KeyError(feat)
