"""The case table of tests/multi_arms.py against the library's host-only diagnostics, without a GPU.

For every row: udp_debug_conv_tile(..., grouped = 1) gives each member the arm the row names (and refuses with 1 the convs
the row says run alone), the members' tiles, cout blocks and codes derived from it form exactly the row's launches under
make_nodes' run rule, and udp_debug_multi_order over each weight-stationary launch reports the dispatch the row names.
The fp64 reference of every ReLU member clips between 20 % and 80 % of its elements (checked here, on the operands the
GPU test uses, so the GPU test need not).  The census holds the table to the coverage list it was built for.
tests/test_gpu_multi_arms.py runs the same rows on the GPU and ties this to the launches through the UDP_POSE_DEBUG_TILES lines.
"""
import ctypes as C

import pytest

import multi_arms as ma
from udp_pose_amd import _lib

ROWS = ma.ROWS


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_row_matches_the_library(row):
    ds, launches = ma.plan(row)
    for i, (m, d) in enumerate(zip(row.members, ds)):
        assert d.arm == m.arm, (row.id, i, m, d)
        if row.mode == "ws":
            assert d.member == (m.arm[0] in (6, 8) and not m.up), (row.id, i, d)
        else:
            assert d.member == (row.mode != "f32" and not m.up), (row.id, i, d)
    assert launches == list(row.launches), (row.id, launches)
    for l in launches:
        assert 2 <= len(l.members) <= 4
        assert [row.members[i] for i in l.members] == sorted((row.members[i] for i in l.members), key=lambda m: -m.cin), "deepest K first"


def test_diagnostic_says_1_for_a_conv_that_runs_alone():
    """The refusals the table relies on: f32 and stride 2.  What udp_debug_conv_tile cannot see -- an upsampled addend,
    which describe_conv_grouped refuses (p.nup) -- the GPU test observes through the report lines."""
    out = (C.c_int * 9)()
    f = _lib.lib().udp_debug_conv_tile
    assert f(_lib.UDP_F32, 0, 3, 1, 3, 16, 12, 32, 32, 0, 1, out) == 1
    assert f(_lib.UDP_BF16, 0, 3, 1, 3, 16, 12, 32, 32, 0, 1, out) == 0 and (out[0], out[1]) == (2, 3)
    assert f(_lib.UDP_F16X2, 1, 3, 2, 3, 16, 12, 32, 32, 0, 1, out) == 1          # stride 2


@pytest.mark.parametrize("spec", sorted({r.spec for r in ROWS}))
def test_relu_members_clip_some_and_not_all(spec):
    row = ma.BY_ID[spec]
    for i, (m, d) in enumerate(zip(row.members, ma.operands(row))):
        assert tuple(d["ref"].shape) == (row.n, m.cout, m.h, m.w)
        if m.relu:
            frac = float((d["ref"] == 0).double().mean())
            assert 0.2 < frac < 0.8, (spec, i, frac)
        if row.mode == "ws":
            assert ma.wexp(d) != 0, (spec, i)
    for a, b in ((a, b) for a in range(len(row.members)) for b in range(a)):
        same = row.members[a].twin and row.members[a].twin == row.members[b].twin
        assert bool(same) == (ma.operands(row)[a] is ma.operands(row)[b])


def test_twin_rows_share_program_and_operands():
    for r in ROWS:
        if r.base:
            b = ma.BY_ID[r.base]
            assert (r.spec, r.mode, r.n, r.members) == (b.spec, b.mode, b.n, b.members) and r.env != b.env, r.id
            assert [l.members for l in r.launches] == [l.members for l in b.launches], r.id
        assert all(m.h <= 32 and m.w <= 16 for m in r.members) and r.n <= 8, r.id


def _cells():
    """Every cell of the coverage list the table reaches, from the library's decisions (not from the table's own claims)."""
    got = set()
    for row in ROWS:
        ds, launches = ma.plan(row)
        mem = row.members
        if row.mode == "ws":
            for l in launches:
                ks = mem[l.members[0]].ks
                got.add(("ws-size", len(l.members)))
                if len({(mem[i].h, mem[i].w) for i in l.members}) > 1 and len({mem[i].cin for i in l.members}) > 1 and \
                        mem[l.members[0]].h * mem[l.members[0]].w == min(mem[i].h * mem[i].w for i in l.members):
                    got.add(("ws-maps", ks))
                for i, code in zip(l.members, l.codes):
                    m, d = mem[i], ds[i]
                    got.add(("ws", ks, code, l.how))
                    if d.ncby >= 2:
                        got.add(("ws-ncby2", code))
                    if code == 8 and d.ncby == 3:
                        got.add(("ws-pb8-ncby3",))
                    feats = {"res": m.res, "views": m.views == "out", "in-slice": m.views == "in", "norelu": not m.relu,
                             "raggedG": d.tile.G > 1 and row.n % d.tile.G != 0, "raggedK": m.cin % 32 != 0, "padcout": m.cout % 32 != 0,
                             "wexp": ma.wexp(ma.operands(row)[i]) != 0}
                    for f, on in feats.items():
                        if on and code >= 2:
                            got.add(("ws-feat", f, "code>=2"))
                        if on and ks == 3:
                            got.add(("ws-feat", f, "k3"))
            in_launch = {i for l in launches for i in l.members}
            for g in {m.group for m in mem}:
                idx = [i for i, m in enumerate(mem) if m.group == g]
                if len(idx) >= 5 and idx == list(range(idx[0], idx[0] + len(idx))) and len({mem[i].ks for i in idx}) == 1 and \
                        any(l.members == tuple(idx[:4]) for l in launches) and idx[4] not in in_launch and ds[idx[4]].member:
                    got.add(("ws-five",))
                    if ds[idx[4]].arm[0] == 8:
                        got.add(("ws-alone-pb8",))
                for a, b, c in zip(idx, idx[1:], idx[2:]):
                    if mem[b].up and ds[a].member and ds[c].member and a not in in_launch and c not in in_launch:
                        got.add(("ws-broken",))
                        if ds[a].arm[0] == 8:
                            got.add(("ws-alone-pb8",))
                if {3, 1} <= {mem[i].ks for i in idx} and sum(1 for l in launches if set(l.members) <= set(idx)) >= 2:
                    got.add(("ws-mixed-ks",))
        elif row.mode == "f32":
            if not launches and all(m.group for m in mem):
                got.add(("f32-nothing-merges",))
        else:
            for l in launches:
                ks = mem[l.members[0]].ks
                got.add(("lds", row.mode, ks, l.how))
                got.add(("lds-size", len(l.members)))
                own = [ds[i].arm for i in l.members]
                if l.how == 4 and 3 in own and 4 in own and not row.env:
                    got.add(("lds-mixed", row.mode, ks))
                    # the masked member has a twin in an all-MBW-3 launch of the same program
                    for i in l.members:
                        if ds[i].arm == 3 and any(mem[j].twin == mem[i].twin and j != i and any(j in q.members and q.how == 3 for q in launches)
                                                  for j in range(len(mem)) if mem[i].twin):
                            got.add(("lds-mixed-twin", row.mode, ks))
            in_launch = {i for l in launches for i in l.members}
            for a, b, c in zip(range(len(mem)), range(1, len(mem)), range(2, len(mem))):
                if mem[a].group == mem[b].group == mem[c].group and not ds[b].member and a in in_launch and c in in_launch:
                    got.add(("lds-rejected-inside",))
    return got


def test_census():
    want = {("ws", ks, code, how) for ks in (3, 1) for code in (1, 2, 4) for how in ("table", "search")}
    want |= {("ws", 3, 8, "table"), ("ws", 3, 8, "search")}
    want |= {("ws-size", k) for k in (2, 3, 4)}
    want |= {("ws-five",), ("ws-broken",), ("ws-alone-pb8",), ("ws-mixed-ks",), ("ws-ncby2", 4), ("ws-ncby2", 1), ("ws-pb8-ncby3",),
             ("ws-maps", 3), ("ws-maps", 1)}
    want |= {("ws-feat", f, where) for f in ("res", "views", "in-slice", "norelu", "raggedG", "raggedK", "padcout", "wexp")
             for where in ("code>=2", "k3")}
    want |= {("lds", mode, ks, mbw) for mode in ("bf16", "lds-f16x2") for ks in (3, 1) for mbw in (3, 4)}
    want |= {("lds-mixed", mode, ks) for mode in ("bf16", "lds-f16x2") for ks in (3, 1)}
    want |= {("lds-mixed-twin", mode, ks) for mode in ("bf16", "lds-f16x2") for ks in (3, 1)}
    want |= {("lds-size", 2), ("lds-size", 4), ("lds-rejected-inside",), ("f32-nothing-merges",)}
    got = _cells()
    assert not (want - got), "cells the table no longer reaches: %s" % sorted(want - got, key=repr)
    # every table row has its segment-search twin, every LDS row its forced-MBW-4 twin
    for r in ROWS:
        if not r.base and any(l.how == "table" for l in r.launches):
            assert any(q.base == r.id and "UDP_POSE_WS_NOTAB" in q.env for q in ROWS), r.id
        if not r.base and r.mode in ("bf16", "lds-f16x2"):
            assert any(q.base == r.id and "UDP_POSE_MULTI_MBW4" in q.env for q in ROWS), r.id
