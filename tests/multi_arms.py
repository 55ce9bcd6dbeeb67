"""The case table of the merged-launch tests (test_multi_arms_cpu.py, test_gpu_multi_arms.py).

Same-depth convs of different branches carry one launch-group id and run as ONE launch (csrc/hrnet.hip, make_nodes:
a run of up to four consecutive groupable convs of one group id, kernel size and storage type), on one of two families:

  * conv_ws_multi<3> / conv_ws_multi<1> (csrc/conv_ws.hip): split fp16 with fragment-major weights.  A conv is a member when
    the grouped chooser gives it 6 pixel blocks per wave (its code = CP, the cout pairs per workgroup: 1, 2 or 4) or the
    8-block one-pair tile (code 8).  The kernel finds a workgroup's (member, tile, cout block) through a per-8 lookup table
    when every member's tile count is a multiple of 8, through a segment search otherwise (ws_order).
  * conv_mfma_multi<T, KS, 1, 2, MBW, 4> (csrc/conv.hip): bf16 and split fp16 with plain weights, MBW = 3 when every member's
    tile has at most 192 pixels, else 4 (a member described for 3 then runs masked under 4).

A row is ONE micro-program (tests/microprog.py): the members in program order, deepest K first as the planners list them,
the chooser knobs to set around create and run, and what must be observed -- per member the arm, per merged launch the
member list, the codes and the dispatch (ws) or the MBW of the instantiation (lds).  ``plan(row)`` derives all of that from
the library's host-only diagnostics (udp_debug_conv_tile with grouped = 1, udp_debug_multi_order) and a port of make_nodes'
run rule; tests/test_multi_arms_cpu.py holds the table against it without a GPU.

Maps stay at or below 32 x 16 and N at or below 8; N = 8 with one tile per image gives the lookup table, N = 3 the search
and, where two images share a tile, a ragged last tile.
"""
import collections
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import conv_arms as ca
import microprog as mp
from udp_pose_amd import f16x2

Member = collections.namedtuple("Member", "ks cin cout h w arm relu res views up group twin")
# arm: ws -- (PB, CP) of the grouped chooser (a member of a merged launch exactly when PB is 6 or 8); lds -- the MBW the grouped
#      chooser describes the member for; a conv that cannot join (up, or f32): the (PB, CP) / (NB, MBW) of the ungrouped chooser
# res: a residual;  views: "in" -- the input is channels 16.. of a tensor 32 wider (NaN elsewhere); "out" -- the residual is
#      channels 16.. of a tensor 32 wider (NaN elsewhere) and the output channels 32.. of one 64 wider (poison elsewhere)
# up: one nearest-upsampled addend (n_up = 1): no merged launch takes such a conv (describe_conv_grouped), it breaks a run
# twin: members of one spec with the same twin key run on identical operands and must store bit-equal outputs
Launch = collections.namedtuple("Launch", "members codes how")        # how: "table" | "search" (ws), the MBW 3 | 4 (lds)
Row = collections.namedtuple("Row", "id spec mode n env members launches base")
# mode: "ws" (f16x2, wfmt 1) | "lds-f16x2" (f16x2, wfmt 0) | "bf16" | "f32";  base: the row of the same spec whose stored
# outputs this row's must equal bit for bit (the UDP_POSE_WS_NOTAB / UDP_POSE_MULTI_MBW4 twin of a row)

DTYPE = {"ws": "f16x2", "lds-f16x2": "f16x2", "bf16": "bf16", "f32": "f32"}


def M(ks, cin, cout, h, w, arm, relu=1, res=0, views="", up=0, group=1, twin=None):
    return Member(ks, cin, cout, h, w, arm, relu, res, views, up, group, twin)


def _k(ks, members):
    return [m._replace(ks=ks) for m in members]


# ---------------------------------------------------------------------------------------------- weight-stationary rows
# four members, one per code 4 (two cout blocks), 4, 2, 1; every tile count 8 -> lookup table
_TAB4 = [M(3, 256, 256, 12, 8, (6, 4), res=1), M(3, 128, 128, 12, 8, (6, 4), res=1, views="out"),
         M(3, 64, 64, 16, 12, (6, 2), views="in"), M(3, 32, 32, 24, 16, (6, 1), res=1)]
# the 8-block arm with one and with three cout blocks beside a code-2 member with a ragged K chunk and a padded Cout
_TAB8 = [M(3, 48, 48, 16, 12, (6, 2), res=1), M(3, 32, 96, 32, 16, (8, 1)), M(3, 32, 32, 32, 16, (8, 1), res=1, views="out")]
# N = 3: two images per tile on the two deepest members (ragged last tile), no ReLU on one, 1 + 2 + 3 + 3 workgroups
_SEARCH = [M(3, 128, 128, 8, 6, (6, 4), res=1), M(3, 64, 64, 12, 8, (6, 2), relu=0, res=1),
           M(3, 48, 48, 16, 12, (6, 2), res=1, views="out"), M(3, 32, 32, 32, 16, (8, 1))]
_WS_SPECS = [
    ("ws-k3-tab4", 8, {}, _TAB4, [Launch((0, 1, 2, 3), (4, 4, 2, 1), "table")]),
    ("ws-k3-tab8", 8, {}, _TAB8, [Launch((0, 1, 2), (2, 8, 8), "table")]),
    ("ws-k3-search", 3, {}, _SEARCH, [Launch((0, 1, 2, 3), (4, 2, 2, 8), "search")]),
    # a forced one-pair split: 64 -> 64 as two cout blocks of code 1, two images per tile
    ("ws-k3-cp1", 8, {"UDP_POSE_WS_CP": "1"}, [M(3, 64, 64, 16, 12, (6, 1), res=1), M(3, 32, 32, 24, 16, (6, 1), views="in")],
     [Launch((0, 1), (1, 1), "search")]),
    # a forced two-pair split of 128 channels, two images per tile with a ragged last one
    ("ws-k3-cp2", 3, {"UDP_POSE_WS_CP": "2"}, [M(3, 128, 128, 12, 8, (6, 2), res=1), M(3, 64, 64, 16, 12, (6, 2))],
     [Launch((0, 1), (2, 2), "search")]),
    # without the 8-block candidate the 32x16 map gets a 4-block tile and is no member
    ("ws-k3-nopb8", 3, {"UDP_POSE_WS_PB8": "0"}, [M(3, 64, 64, 16, 12, (6, 2), res=1), M(3, 32, 32, 24, 16, (6, 1)), M(3, 32, 32, 32, 16, (4, 1))],
     [Launch((0, 1), (2, 1), "search")]),
    # one group id on five consecutive members: four share a launch, the fifth (8 blocks) runs conv_ws_pb8_kernel alone
    ("ws-k3-five", 8, {}, [M(3, 128, 128, 12, 8, (6, 4)), M(3, 64, 64, 16, 12, (6, 2), res=1), M(3, 64, 64, 16, 12, (6, 2), relu=0),
                           M(3, 32, 32, 24, 16, (6, 1)), M(3, 32, 32, 32, 16, (8, 1), res=1)],
     [Launch((0, 1, 2, 3), (4, 2, 2, 1), "table")]),
    # a group broken by a conv with an upsampled addend: its neighbours run alone on their grouped tiles (8 blocks: conv_ws_pb8_kernel)
    ("ws-k3-broken", 3, {}, [M(3, 32, 32, 32, 16, (8, 1), res=1), M(3, 64, 64, 16, 12, (2, 2), up=1, res=1), M(3, 64, 64, 16, 12, (6, 2))], []),
    # one group id over 3x3 and 1x1 members: one launch per kernel size
    ("ws-mixed-ks", 8, {}, [M(3, 64, 64, 16, 12, (6, 2), res=1), M(3, 32, 32, 24, 16, (6, 1)),
                            M(1, 64, 64, 16, 12, (6, 2), relu=0, res=1), M(1, 32, 32, 24, 16, (6, 1), relu=0)],
     [Launch((0, 1), (2, 1), "table"), Launch((2, 3), (2, 1), "table")]),
    # conv_ws_multi<1> as the fuse layers use it: no ReLU, four members
    ("ws-k1-tab4", 8, {}, [m._replace(relu=0) for m in _k(1, _TAB4)], [Launch((0, 1, 2, 3), (4, 4, 2, 1), "table")]),
    ("ws-k1-search", 3, {}, [M(1, 128, 128, 8, 6, (6, 4), res=1), M(1, 48, 48, 16, 12, (6, 2), res=1, views="out"),
                             M(1, 32, 32, 24, 16, (6, 1), views="in")],
     [Launch((0, 1, 2), (4, 2, 1), "search")]),
    ("ws-k1-cp", 3, {"UDP_POSE_WS_CP": "2"}, [M(1, 128, 128, 12, 8, (6, 2), relu=0, res=1), M(1, 64, 64, 16, 12, (6, 2))],
     [Launch((0, 1), (2, 2), "search")]),
]

# ---------------------------------------------------------------------------------------------- LDS-staged rows
# group 1: two members described for MBW 3.  group 2, five members of one id: two for MBW 3, a conv with an addend that runs
# alone, then the twin of member 1 beside a 240-pixel tile -> the MBW 4 instantiation runs a member described for 3.
# group 3: four members, one of them of MBW 4.
def _lds_members(ks, own):
    """own = None: bf16 / split fp16 (arm = the member's MBW); else f32, where nothing merges: own[(cin, h, w)] = (NB, MBW)."""
    a = lambda cin, h, w, mbw, up=0: own[(cin, h, w)] if own else ((2, mbw) if up else mbw)
    return [M(ks, 64, 64, 12, 8, a(64, 12, 8, 3), res=1, group=1), M(ks, 32, 32, 16, 12, a(32, 16, 12, 3), group=1, twin="b"),
            M(ks, 64, 64, 12, 8, a(64, 12, 8, 3), relu=0, group=2), M(ks, 48, 64, 16, 12, a(48, 16, 12, 3), res=1, views="out", group=2),
            M(ks, 32, 32, 16, 12, a(32, 16, 12, 3, 1), res=1, up=1, group=2),
            M(ks, 32, 32, 16, 12, a(32, 16, 12, 3), group=2, twin="b"), M(ks, 32, 32, 20, 12, a(32, 20, 12, 4), res=1, group=2),
            M(ks, 64, 64, 12, 8, a(64, 12, 8, 3), views="in", group=3), M(ks, 48, 64, 16, 12, a(48, 16, 12, 3), relu=0, res=1, group=3),
            M(ks, 32, 32, 20, 12, a(32, 20, 12, 4), group=3), M(ks, 32, 32, 16, 12, a(32, 16, 12, 3), res=1, group=3)]


_LDS_LAUNCHES = [Launch((0, 1), (3, 3), 3), Launch((2, 3), (3, 3), 3), Launch((5, 6), (3, 4), 4), Launch((7, 8, 9, 10), (3, 3, 4, 3), 4)]
_LDS_LAUNCHES4 = [Launch(l.members, (4,) * len(l.members), 4) for l in _LDS_LAUNCHES]
_F32_OWN = {3: {(64, 12, 8): (2, 2), (32, 16, 12): (2, 3), (48, 16, 12): (2, 3), (32, 20, 12): (2, 4)}}


def _rows():
    rows = []
    for spec, n, env, members, launches in _WS_SPECS:
        rows.append(Row(spec, spec, "ws", n, env, members, launches, None))
        if any(l.how == "table" for l in launches):      # the same program through the segment search
            rows.append(Row(spec + "-notab", spec, "ws", n, dict(env, UDP_POSE_WS_NOTAB="1"), members,
                            [l._replace(how="search") for l in launches], spec))
    for mode in ("bf16", "lds-f16x2"):
        for ks in (3, 1):
            spec = "%s-k%d" % (mode, ks)
            rows.append(Row(spec, spec, mode, 3, {}, _lds_members(ks, None), _LDS_LAUNCHES, None))
            rows.append(Row(spec + "-mbw4", spec, mode, 3, {"UDP_POSE_MULTI_MBW4": "1"}, _lds_members(ks, None), _LDS_LAUNCHES4, spec))
    # f32: the group ids are set and nothing merges
    rows.append(Row("f32-k3", "f32-k3", "f32", 3, {}, _lds_members(3, _F32_OWN[3]), [], None))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS), "duplicate row ids"


class env_knobs(ca.env_knobs):
    """conv_arms.env_knobs with the knobs of the merged launches: every one the row does not name is removed for the duration."""
    KNOBS = ca.env_knobs.KNOBS + ("UDP_POSE_WS_PB8", "UDP_POSE_WS_NOTAB", "UDP_POSE_WS_ORDER", "UDP_POSE_WS_G", "UDP_POSE_WS_BIAS",
                                  "UDP_POSE_MULTI_MBW4", "UDP_POSE_NO_GROUPS", "UDP_POSE_WS_MINWGS")


# ---------------------------------------------------------------------------------------------- what the library decides
Decision = collections.namedtuple("Decision", "member arm tile code tiles ncby")
# member: joins merged launches;  arm: as Member.arm;  tile: conv_arms.Tile;  code / tiles / ncby: ConvMulti's (ws members)


def decide(row, m):
    """The chooser's decision for one member under the current environment (set the row's knobs around the call)."""
    dtype, wfmt = DTYPE[row.mode], int(row.mode == "ws")
    t = None if m.up else ca.debug_tile(dtype, wfmt, m.ks, 1, row.n, m.h, m.w, m.cin, m.cout, 0, 1)
    if row.mode == "ws" and t is not None:
        if t.arm[0] in (6, 8):
            ncby = mp.round_up(m.cout, 32) // (32 * t.arm[1])
            assert t.wgs % ncby == 0
            return Decision(True, t.arm, t, 8 if t.arm[0] == 8 else t.arm[1], t.wgs // ncby, ncby)
        return Decision(False, t.arm, t, 0, 0, 0)          # runs alone on the grouped chooser's tile
    if t is not None:
        return Decision(True, t.arm[1], t, 4 if "UDP_POSE_MULTI_MBW4" in row.env else t.arm[1], 0, 0)
    t = ca.debug_tile(dtype, wfmt, m.ks, 1, row.n, m.h, m.w, m.cin, m.cout, 0, 0)        # the conv of a launch of its own
    assert t is not None, "refused: %s" % (m,)
    return Decision(False, t.arm, t, 0, 0, 0)


def used_table(ds):
    """udp_debug_multi_order for the ws members ``ds`` of one launch: does the kernel take the lookup table?"""
    C = ca.C
    n = len(ds)
    total = sum(d.tiles * d.ncby for d in ds)
    arr = lambda t, v: (t * len(v))(*v)
    used = C.c_int(-1)
    got = ca._lib.lib().udp_debug_multi_order(arr(C.c_uint, [d.tiles for d in ds]), arr(C.c_uint, [d.ncby for d in ds]),
                                              arr(C.c_int, [d.code for d in ds]), n, total, (C.c_uint * total)(), (C.c_uint * total)(),
                                              (C.c_uint * total)(), C.byref(used))
    assert got == total, (got, total)
    return bool(used.value)


def plan(row):
    """(decisions, launches) as the library forms them: make_nodes' rule -- a run of up to four consecutive members of one
    group id and kernel size is one launch, a run of one runs alone."""
    with env_knobs(**row.env):
        ds = [decide(row, m) for m in row.members]
        launches, i = [], 0
        while i < len(ds):
            k = 1
            if ds[i].member and row.members[i].group:
                while (k < 4 and i + k < len(ds) and ds[i + k].member and row.members[i + k].ks == row.members[i].ks and
                       row.members[i + k].group == row.members[i].group):
                    k += 1
            if k > 1:
                run = ds[i:i + k]
                how = ("table" if used_table(run) else "search") if row.mode == "ws" else max(d.code for d in run)
                launches.append(Launch(tuple(range(i, i + k)), tuple(d.code for d in run), how))
            i += k
    return ds, launches


# ---------------------------------------------------------------------------------------------- operands and references
@functools.lru_cache(maxsize=None)
def _operands(spec, key, dtype, n, ks, cin, cout, h, w, relu, res, up):
    g = torch.Generator().manual_seed(zlib.crc32(repr((spec, key)).encode()))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    d = dict(x=mp.quant(r(n, cin, h, w), dtype), w=mp.quant(r(cout, cin, ks, ks) * float(np.sqrt(2.0 / (cin * ks * ks))), dtype),
             b=r(cout) * 0.1, res=mp.quant(r(n, cout, h, w), dtype) if res else None,
             up=mp.quant(r(n, cout, h // 2, w // 2), dtype) if up else None)
    y = F.conv2d(d["x"].double(), d["w"].double(), d["b"].double(), padding=ks // 2)
    if res:
        y = y + d["res"].double()
    if up:
        y = y + F.interpolate(d["up"].double(), scale_factor=2, mode="nearest")
    d["ref"] = F.relu(y) if relu else y
    return d


def operands(row):
    """Per member: the quantised operands (x, w, b, res, up) and the fp64 reference of the conv over them, computed once per spec."""
    return [_operands(row.spec, m.twin if m.twin else i, DTYPE[row.mode], row.n, m.ks, m.cin, m.cout, m.h, m.w, m.relu, m.res, m.up)
            for i, m in enumerate(row.members)]


def wexp(d):
    """The exponent pack_weights_ws stores for a member's weights."""
    return f16x2.weight_exponent(d["w"])
