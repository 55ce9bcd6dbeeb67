"""Every member arm and dispatch path of the merged conv launches on the GPU, each member against the fp64 conv
(table: tests/multi_arms.py; tests/test_multi_arms_cpu.py holds the table against the library's host-only diagnostics).

A row is ONE micro-program (tests/microprog.py): pre-filled operand buffers, the member convs with their launch-group ids,
outputs left at the NaN poison.  Per row the test
  1. runs it with the row's knobs and UDP_POSE_DEBUG_TILES: every member's report line ("ws conv" / "grouped conv" / "conv k")
     names the arm and the tile the diagnostic gave, and the "ws multi" / "lds multi" lines name exactly the row's launches --
     members, workgroups, codes, lookup table or segment search, the MBW of the instantiation;
  2. runs it again in a fresh handle with UDP_POSE_NO_GROUPS=1 -- every conv on a launch of its own under the ungrouped
     chooser, no merged-launch line -- and asserts every member's stored output bit-equal between the two runs: the order of K
     chunks and taps into an accumulator does not depend on the launch form;
  3. compares every member's output with the fp64 conv of the operands as stored, max |got - ref| <= microprog.conv_tol (the
     shipped gates 2e-5 / 6e-3 / 1e-4 x scale): two equally wrong paths do not pass;
  4. asserts that no NaN is left, that nothing outside the declared outputs changed (Micro.assert_untouched: the other
     channels of a wide output tensor included) and that the program's head holds (Micro.check_head).
Members with one twin key run on identical operands in different launches of one program (a member described for MBW 3 in
an all-MBW-3 launch and masked under the MBW 4 instantiation) and must store bit-equal outputs; so must a row and its base
row (the same program through the segment search instead of the lookup table, or with MBW 4 forced).
"""
import re
import zlib

import numpy as np
import pytest
import torch

import microprog as mp
import multi_arms as ma
from microprog import Micro, new_op
from udp_pose_amd import _lib

pytestmark = pytest.mark.gpu

WS_LINE = re.compile(r"^ws conv k(\d+) s1 (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) CP=(\d+) PB=(\d+) lds=(\d+)(?: \(one stage buffer\))? wgs=(\d+)$")
GROUPED_LINE = re.compile(r"^grouped conv (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) NB=2 lds=(\d+) wgs=(\d+)$")
LDS_LINE = re.compile(r"^conv k(\d+) s1 (\d+)x(\d+) C(\d+)->(\d+): G=(\d+) R=(\d+) TW=(\d+) NB=(\d+) mbw=(\d+) lds=(\d+) wgs=(\d+)$")
WS_MULTI = re.compile(r"^ws multi k(\d): members=(\d+) wgs=(\d+) codes=\[([\d,]+)\] dispatch=(table|search)$")
LDS_MULTI = re.compile(r"^lds multi (bf16|f16x2) k(\d): members=(\d+) wgs=(\d+) codes=\[([\d,]+)\] MBW=(\d)$")


def _program(row):
    dtype = ma.DTYPE[row.mode]
    m = Micro(dtype, row.n, seed=zlib.crc32(row.spec.encode()))
    bufs = []
    for mem, d in zip(row.members, ma.operands(row)):
        f = dict(ks=mem.ks, stride=1, relu=mem.relu, cin=mem.cin, cout=mem.cout, hin=mem.h, win=mem.w, hout=mem.h, wout=mem.w, group=mem.group)
        if mem.views == "in":
            f.update(in_coff=16, in_pitch=mem.cin + 32)
        f["in_buf"] = m.buf(mem.h, mem.w, f.get("in_pitch", mem.cin))
        m.fill(f["in_buf"], d["x"], coff=f.get("in_coff", 0))
        if mem.views == "out":
            f.update(res_coff=16, res_pitch=mem.cout + 32, out_coff=32, out_pitch=mem.cout + 64)
        if mem.res:
            f["res_buf"] = m.buf(mem.h, mem.w, f.get("res_pitch", mem.cout))
            m.fill(f["res_buf"], d["res"], coff=f.get("res_coff", 0))
        if mem.up:
            ub = m.buf(mem.h // 2, mem.w // 2, mem.cout)
            m.fill(ub, d["up"])
            f.update(n_up=1, up_buf=[ub], up_shift=[1])
        f["out_buf"] = m.buf(mem.h, mem.w, f.get("out_pitch", mem.cout))
        m.wrote(f["out_buf"], f.get("out_coff", 0), mem.cout)
        m.add(new_op(_lib.UDP_OP_CONV, **f, **m.put_conv(d["w"], d["b"], ws=row.mode == "ws")))
        bufs.append((f["out_buf"], f.get("out_coff", 0)))
    return m, bufs


def _lines(err, row):
    """The members' report lines in program order (the head conv 64 -> 17 dropped) and the merged-launch lines."""
    convs, multis = [], []
    for line in err.splitlines():
        g = WS_LINE.match(line)
        if g:
            v = list(map(int, g.groups()))
            convs.append(dict(kind="ws", ks=v[0], shape=tuple(v[1:5]), G=v[5], R=v[6], TW=v[7], arm=(v[9], v[8]), lds=v[10], wgs=v[11]))
        g = GROUPED_LINE.match(line)
        if g:
            v = list(map(int, g.groups()))
            convs.append(dict(kind="grouped", ks=None, shape=tuple(v[0:4]), G=v[4], R=v[5], TW=v[6], arm=-(-v[4] * v[5] * v[6] // 64), lds=v[7], wgs=v[8]))
        g = LDS_LINE.match(line)
        if g and int(g.group(5)) != 17:
            v = list(map(int, g.groups()))
            convs.append(dict(kind="lds", ks=v[0], shape=tuple(v[1:5]), G=v[5], R=v[6], TW=v[7], arm=(v[8], v[9]), lds=v[10], wgs=v[11]))
        g = WS_MULTI.match(line)
        if g:
            multis.append(("ws", int(g.group(1)), int(g.group(2)), int(g.group(3)), tuple(map(int, g.group(4).split(","))), g.group(5)))
        g = LDS_MULTI.match(line)
        if g:
            multis.append((g.group(1), int(g.group(2)), int(g.group(3)), int(g.group(4)), tuple(map(int, g.group(5).split(","))), int(g.group(6))))
    return convs, multis


def _run(row, capfd, grouped):
    m, bufs = _program(row)
    env = dict(row.env, UDP_POSE_DEBUG_TILES="1")
    if not grouped:
        env["UDP_POSE_NO_GROUPS"] = "1"
    capfd.readouterr()
    with ma.env_knobs(**env):
        rc = m.run()
    assert rc == 0, (row.id, m.error)
    convs, multis = _lines(capfd.readouterr().err, row)
    raw = [np.array(m.read_raw(b, coff, mem.cout)) for (b, coff), mem in zip(bufs, row.members)]
    got = [m.read(b, coff, mem.cout) for (b, coff), mem in zip(bufs, row.members)]
    for i, t in enumerate(got):
        assert not torch.isnan(t).any(), "%s member %d: output not fully written, or an unread NaN channel reached it" % (row.id, i)
    m.assert_untouched()
    m.check_head()
    return convs, multis, raw, got


_DONE = {}


def _check(row, capfd):
    if row.id in _DONE:
        return _DONE[row.id]
    dtype = ma.DTYPE[row.mode]
    ds, launches = ma.plan(row)
    assert launches == list(row.launches), (row.id, launches)
    # ---- 1. the merged run: the report names the row's arms and launches
    convs, multis, raw, got = _run(row, capfd, True)
    assert len(convs) == len(row.members), (row.id, convs)
    for i, (mem, d, c) in enumerate(zip(row.members, ds, convs)):
        assert c["shape"] == (mem.h, mem.w, mem.cin, mem.cout) and c["ks"] in (None, mem.ks), (row.id, i, c)
        assert c["kind"] == ("ws" if row.mode == "ws" else "grouped" if d.member else "lds"), (row.id, i, c)
        assert c["arm"] == mem.arm == d.arm, (row.id, i, c, d)
        assert (c["G"], c["R"], c["TW"], c["lds"], c["wgs"]) == (d.tile.G, d.tile.R, d.tile.TW, d.tile.lds, d.tile.wgs), (row.id, i, c, d)
    fam = {"ws": "ws", "lds-f16x2": "f16x2", "bf16": "bf16", "f32": None}[row.mode]
    want = [(fam, row.members[l.members[0]].ks, len(l.members), sum(ds[i].tile.wgs for i in l.members), l.codes, l.how) for l in row.launches]
    assert multis == want, (row.id, multis, want)
    # ---- 2. every conv on a launch of its own: bit-equal
    convs0, multis0, raw0, _ = _run(row, capfd, False)
    assert multis0 == [] and len(convs0) == len(row.members) and all(c["kind"] != "grouped" for c in convs0), (row.id, multis0, convs0)
    for i, (a, b) in enumerate(zip(raw, raw0)):
        diff = int((a != b).sum())
        assert diff == 0, "%s member %d: merged and own launch differ in %d stored units (%s vs %s)" % (row.id, i, diff, convs[i], convs0[i])
    # ---- twins inside the program
    for a in range(len(row.members)):
        for b in range(a):
            if row.members[a].twin and row.members[a].twin == row.members[b].twin:
                assert np.array_equal(raw[a], raw[b]), "%s: members %d and %d (twin %s) differ" % (row.id, b, a, row.members[a].twin)
    # ---- 3. fp64 parity
    worst = 0.0
    for i, (mem, d, t) in enumerate(zip(row.members, ma.operands(row), got)):
        ref = d["ref"]
        err, tol = float((t.double() - ref).abs().max()), mp.conv_tol(dtype, ref)
        worst = max(worst, err / tol)
        print("%s member %d k%d C%d->%d %dx%d n%d: %s arm %s  err %.3g (gate %.3g)" % (
            row.id, i, mem.ks, mem.cin, mem.cout, mem.h, mem.w, row.n, "member" if ds[i].member else "alone", mem.arm, err, tol))
        assert err <= tol, (row.id, i, err, tol)
    print("%s launches %s  own-launch arms %s  worst err / gate %.3g" % (row.id, multis, [c["arm"] for c in convs0], worst))
    _DONE[row.id] = raw
    return raw


@pytest.mark.parametrize("row", ma.ROWS, ids=lambda r: r.id)
def test_merged_launch_matches_fp64_and_own_launches(row, capfd):
    raw = _check(row, capfd)
    if row.base:
        base = _check(ma.BY_ID[row.base], capfd)
        for i, (a, b) in enumerate(zip(raw, base)):
            assert np.array_equal(a, b), "%s and %s: member %d differs" % (row.id, row.base, i)
        print("%s: bit-equal to %s" % (row.id, row.base))
