"""The case table of tests/conv_arms.py against the library's own tile choosers, without a GPU.

udp_debug_conv_tile (include/udp_pose_hip.h) reports what choose_conv_ws (csrc/conv_ws.hip, the tile choice of
describe_conv_ws) and conv_choose_tile (csrc/conv.hip) decide for a conv: host arithmetic, no HIP call.  The tests
check that
  * every row of the table reaches exactly the arm -- and the tile feature -- it names,
  * every INSTANTIATED arm of both kernel families is reached by a row, or is on the table's unreachable list,
  * an arm is on that list only if the diagnostic returns it for no shape of a scan over map sizes, batches, channel
    counts and forced knobs (so a dead instantiation is a finding of the scan, not a convenience of the table).
tests/test_gpu_conv_arms.py runs the same rows on the GPU and ties this report to the launch through the
UDP_POSE_DEBUG_TILES line.
"""
import ctypes as C

import pytest

import conv_arms as ca
from udp_pose_amd import _lib

# The instantiated arms, as the dispatch macros of the library list them:
#   csrc/conv_ws.hip  describe_ws_pb<KS, STRIDE, NCHW>: UDP_WS(B, C) for B in 2, 3, 4, 6 and C in 1, 2, 4, called for
#                     <3,1,false> <3,1,true> <3,2,false> <1,1,false> <1,1,true> <1,2,false>   (conv_ws_h2_kernel)
#                     describe_ws_hs: the same UDP_WS(B, C) list for hard-swish and for SiLU   (conv_ws_hs_kernel)
#   csrc/conv.hip     describe_conv_t<T>: UDP_CASE(K, S, B) for (3,1) (3,2) (1,1) (1,2) x B in 2, 4 and UDP_CASE_OUT(K, S, B)
#                     for (1,1) (3,1) x B in 2, 4, each through describe_mbw's MBW 1..4, T in float, H2, bf16 (conv_mfma_kernel)
#                     describe_hs<T>: UDP_HS(B, M) for B in 2, 4 and M in 1..4, both activations, T in float, H2 (conv1x1_hs_kernel)
# (the merged launches conv_ws_multi / conv_mfma_multi and the 8-block kernel run in programs only: tests/test_gpu_ws_pb8.py)
WS_ARMS = [(pb, cp) for pb in (2, 3, 4, 6) for cp in (1, 2, 4)]
LDS_ARMS = [(nb, mbw) for nb in (2, 4) for mbw in (1, 2, 3, 4)]
FORMS = [(3, 1, 0), (3, 1, 1), (3, 2, 0), (1, 1, 0), (1, 1, 1), (1, 2, 0)]        # (ks, stride, NCHW output)
INSTANTIATED = set()
for _f in FORMS:
    INSTANTIATED |= {("ws", "f16x2", 0) + _f + a for a in WS_ARMS}
    for _t in ("f32", "f16x2", "bf16"):
        INSTANTIATED |= {("lds", _t, 0) + _f + a for a in LDS_ARMS}
for _act in (ca.HS, ca.SILU):
    INSTANTIATED |= {("hs", "f16x2", _act, 1, 1, 0) + a for a in WS_ARMS}
    for _t in ("f32", "f16x2"):
        INSTANTIATED |= {("lds", _t, _act, 1, 1, 0) + a for a in LDS_ARMS}

NS = (1, 2, 3, 5, 8, 64, 128)
CINS = (16, 32, 48, 64, 256)


def _key(row, arm):
    return (row.fam, row.dtype, row.act if row.act >= ca.HS else 0, row.ks, row.stride, row.nchw) + tuple(arm)


def test_every_row_reaches_the_arm_it_names():
    bad = []
    for row in ca.ROWS:
        t = ca.decide(row)
        if t is None:
            bad.append((row.id, "refused: " + _lib.lib().udp_last_error().decode()))
        elif t.arm != row.arm:
            bad.append((row.id, "expected arm %s" % (row.arm,), t))
        else:
            bad += [(row.id, "lacks " + f, t) for f in row.feats if not ca.has_feature(row, t, f)]
        assert row.fam == "lds" or set(row.env) == {"UDP_POSE_WS_PB", "UDP_POSE_WS_CP"}, row.id
    assert not bad, bad


def test_table_limits():
    """Maps at or below 40 x 40 and N at or below 5 (two named exceptions), every feature on an arm with PB >= 3 and CP >= 2,
    every bit-equality group with more than one arm."""
    big = {r.id for r in ca.ROWS if r.h > 40 or r.w > 40 or r.n > 5}
    assert big == {"ws-k1s2-n5_1x52_c16-f6.1", "lds-bf16-k3s1-persist"}, big
    for feat in ("raggedG", "raggedRW", "sbuf", "halo"):
        assert any(feat in r.feats and r.fam == "ws" and r.arm[0] >= 3 and r.arm[1] >= 2 for r in ca.ROWS), feat
    groups = {}
    for r in ca.ROWS:
        if r.group:
            groups.setdefault(r.group, []).append(r)
    for g, rows in groups.items():
        assert len({(r.n, r.h, r.w, r.cin, r.cout, r.res, r.act, r.ks, r.stride, r.nchw, r.dtype) for r in rows}) == 1, g
        assert len({ca.decide(r) for r in rows}) > 1, g
    assert any(r.views and r.fam == "ws" and r.arm[0] >= 3 and r.arm[1] >= 2 for r in ca.ROWS)
    for f in ((3, 1, 1), (1, 1, 1)):
        assert {17, 51, 100} <= {r.cout for r in ca.ROWS if r.fam == "ws" and (r.ks, r.stride, r.nchw) == f}


def _unreachable():
    un = {}
    for (ks, s, nchw), arms in ca.UNREACHABLE_WS.items():
        for arm, why in arms.items():
            un[("ws", "f16x2", 0, ks, s, nchw) + arm] = why
    for (dtype, ks, s, nchw), arms in ca.UNREACHABLE_LDS.items():
        for arm, why in arms.items():
            un[("lds", dtype, 0, ks, s, nchw) + arm] = why
    return un


def test_every_instantiated_arm_is_covered_or_listed_unreachable():
    covered = {_key(r, r.arm) for r in ca.ROWS}
    un = _unreachable()
    assert covered <= INSTANTIATED, sorted(covered - INSTANTIATED)
    assert not (covered & set(un)), "listed unreachable and reached by a row: %s" % sorted(covered & set(un))
    missing = INSTANTIATED - covered - set(un)
    assert not missing, "instantiated arms that no row reaches and the unreachable list does not name: %s" % sorted(missing)
    assert all(why for why in un.values())


def _scan(dtype, wfmt, ks, stride, nchw, couts, sizes, found):
    """Every arm udp_debug_conv_tile returns over the grid, under the knobs of the current environment."""
    f, out, dt = _lib.lib().udp_debug_conv_tile, (C.c_int * 9)(), _lib.DTYPES[dtype]
    for cout in couts:
        for n in NS:
            for cin in CINS:
                for h in sizes:
                    for w in sizes:
                        if f(dt, wfmt, ks, stride, n, h, w, cin, cout, nchw, 0, out) == 0:
                            found.add((out[0], out[1]))


@pytest.mark.parametrize("fam", sorted(ca.UNREACHABLE_WS), ids=lambda f: "k%ds%d%s" % (f[0], f[1], "o" if f[2] else ""))
def test_unreachable_weight_stationary_arms_are_never_chosen(fam):
    """Hout, Wout in 1..64, N in NS, Cin in CINS, Cout 128 (every CP divides four pairs).  Knobs: for a listed arm (PB, CP)
    the forced CP and every forced PB >= that PB, plus PB unforced with and without the fill target -- ws_tile rejects a
    candidate whose tile needs more blocks than the forced PB (`need > pb`), so a smaller forced PB cannot return the arm."""
    ks, stride, nchw = fam
    listed = set(ca.UNREACHABLE_WS[fam])
    knobs = set()
    for pb, cp in listed:
        knobs |= {(str(p), str(cp), None) for p in (2, 3, 4, 6) if p >= pb} | {("0", str(cp), None), ("0", str(cp), "0")}
    found = set()
    for pb, cp, minwgs in sorted(knobs, key=str):
        env = {"UDP_POSE_WS_PB": pb, "UDP_POSE_WS_CP": cp}
        if minwgs is not None:
            env["UDP_POSE_MINWGS"] = minwgs
        with ca.env_knobs(**env):
            _scan("f16x2", 1, ks, stride, nchw, (100 if nchw else 128,), range(1, 65), found)
    assert not (found & listed), "the scan reaches %s" % sorted(found & listed)
    cps = {cp for _, cp in listed}                                   # not blind: the other arms of the scanned CP all turn up
    assert {a for a in WS_ARMS if a[1] in cps} - listed <= found, found


@pytest.mark.parametrize("key", sorted(ca.UNREACHABLE_LDS), ids=lambda k: "%s-k%ds%d%s" % (k[0], k[1], k[2], "o" if k[3] else ""))
def test_unreachable_lds_staged_arms_are_never_chosen(key):
    """(UDP_POSE_MINWGS, UDP_POSE_MAXM) in {0, default} x {64, 128, 192, 256}; Cout 32 and 64 (NCHW: 17 and 100) for both NB;
    N in NS, Cin in CINS; Hout, Wout in 1..16 and every third size from 17 to 62 (the full 1..64 grid finds the same arms --
    NOTES.md -- and takes five times as long).  Every arm the family does reach must turn up, so the scan is not blind."""
    dtype, ks, stride, nchw = key
    listed = set(ca.UNREACHABLE_LDS[key])
    sizes = list(range(1, 17)) + list(range(17, 65, 3))
    found = set()
    for minwgs in ("0", None):
        for maxm in ("64", "128", "192", "256"):
            env = {"UDP_POSE_MAXM": maxm}
            if minwgs is not None:
                env["UDP_POSE_MINWGS"] = minwgs
            with ca.env_knobs(**env):
                _scan(dtype, 0, ks, stride, nchw, (17, 100) if nchw else (32, 64), sizes, found)
    assert not (found & listed), "the scan reaches %s" % sorted(found & listed)
    assert found == set(LDS_ARMS) - listed, "reachable arms the scan missed: %s" % sorted(set(LDS_ARMS) - listed - found)


def test_forced_pb_only_caps_the_tile():
    """UDP_POSE_WS_PB caps the candidate; the arm that runs is the smallest instantiated block count covering the tile."""
    with ca.env_knobs(UDP_POSE_WS_PB="6", UDP_POSE_WS_CP="1"):
        t = ca.debug_tile("f16x2", 1, 3, 1, 1, 8, 8, 32, 32)
    assert t.arm == (2, 1) and (t.G, t.R, t.TW) == (1, 8, 8), t
    with ca.env_knobs():
        assert ca.debug_tile("f16x2", 1, 3, 1, 3, 64, 48, 32, 32).arm == (2, 1)           # CONV_CASES: below 512 workgroups, most workgroups win


def test_diagnostic_follows_the_knobs_at_every_call_and_rejects_bad_input():
    seen = set()
    for maxm in ("64", "256", "64"):
        with ca.env_knobs(UDP_POSE_MAXM=maxm, UDP_POSE_MINWGS="0"):
            seen.add((maxm, ca.debug_tile("bf16", 0, 1, 1, 3, 13, 24, 48, 64).arm))
    assert seen == {("64", (4, 1)), ("256", (4, 4))}, seen
    lib, out = _lib.lib(), (C.c_int * 9)()
    assert lib.udp_debug_conv_tile(_lib.UDP_F16X2, 1, 3, 1, 1, 8, 8, 24, 32, 0, 0, out) == -3 and b"multiple of 16" in lib.udp_last_error()
    assert lib.udp_debug_conv_tile(_lib.UDP_F32, 1, 3, 1, 1, 8, 8, 32, 32, 0, 0, out) == -1          # wfmt 1 needs split fp16
    assert lib.udp_debug_conv_tile(_lib.UDP_F32, 0, 5, 1, 1, 8, 8, 32, 32, 0, 0, out) == -1
    assert lib.udp_debug_conv_tile(_lib.UDP_F32, 0, 3, 1, 1, 8, 8, 32, 32, 0, 0, None) == -1
    assert lib.udp_debug_conv_tile(_lib.UDP_F16X2, 1, 3, 2, 1, 8, 8, 32, 32, 1, 0, out) == -3         # no NCHW stride-2 kernel
