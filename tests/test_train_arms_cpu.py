"""Census of the weight-gradient case table (tests/train_arms.py), without a GPU.

udp_debug_wgrad_tile (include/udp_pose_hip.h) reports the kernel family, tile, unit and split-K geometry that
udp_conv2d_wgrad launches -- wgrad_plan in csrc/train.hip is the one function both call.  For every cell (kernel family x
ks x stride) these tests assert that each branch property of train_arms.PROPS is reached by at least one row, so that a
later edit of the table or of the chooser cannot silently drop a cell; the cells where a property cannot occur are
named in UNREACHABLE with the reason.
"""
import collections
import ctypes as C

import pytest

import train_arms as ta
from udp_pose_amd import _lib

# (property, predicate over a cell) -> why no row can have it there
UNREACHABLE = {
    "odd_input_s2": (lambda fam, ks, stride: stride == 1, "an odd input size only changes the geometry under stride 2"),
    "ragged_seen": (lambda fam, ks, stride: ks == 1, "a 1x1 conv reads input column wout * stride >= win under the first "
                    "missing output column: staged zeros, whatever dy holds there"),
}


def _census():
    cells = collections.defaultdict(lambda: collections.defaultdict(list))
    for row, fam in ta.cases():
        for q in ta.props(row, fam):
            cells[(fam, row.ks, row.stride)][q].append(row.id)
    return cells


def test_row_ids_are_unique_and_small():
    ids = [r.id for r in ta.ROWS]
    assert len(ids) == len(set(ids))
    for r in ta.ROWS:
        assert r.w <= 133 and r.h <= 48 and r.n <= 4, r.id
        assert set(r.fams) <= set(ta.FAMILIES) and r.fams, r.id
        assert r.cin <= r.cin_k and r.cout <= r.cout_k, r.id
        if "bf16" in r.fams:
            assert r.cin_k % 8 == 0 and r.cout_k % 8 == 0, r.id
        assert r.cin_k % 4 == 0 and r.cout_k % 4 == 0, r.id


def test_every_cell_reaches_every_property():
    cells = _census()
    missing, wrongly_excused = [], []
    for cell in ta.CELLS:
        for q in ta.PROPS:
            excused = q in UNREACHABLE and UNREACHABLE[q][0](*cell)
            if excused and cells[cell][q]:
                wrongly_excused.append((cell, q, cells[cell][q]))
            if not excused and not cells[cell][q]:
                missing.append((cell, q))
    assert not missing, "no row reaches: %s" % missing
    assert not wrongly_excused, "excused as unreachable but reached: %s" % wrongly_excused
    unreachable = [(cell, q, UNREACHABLE[q][1]) for cell in ta.CELLS for q in UNREACHABLE if UNREACHABLE[q][0](*cell)]
    print("unreachable cells: %s" % unreachable)
    assert len(unreachable) == 12         # odd input at stride 1 and an observable ragged column at ks 1: 6 cells each


def test_family_is_what_the_knob_and_dtype_say():
    for row, fam in ta.cases():
        assert ta.plan(row, fam).family == ta.FAMILY_CODE[fam]


def test_geometry_invariants_of_every_row():
    """What the kernels rely on: TH divides hout (`oy < p.Hout` can never run false), the units cover the map, the
    workgroups cover the units with none empty, the partials fit the workspace, the bf16 staging plan holds the tile."""
    for row, fam in ta.cases():
        p = ta.plan(row, fam)
        ho, wo = ta.out_hw(row)
        assert ho % p.th == 0 and p.units_y * p.th == ho, (row.id, fam)
        assert (p.units_x - 1) * p.tw < wo <= p.units_x * p.tw, (row.id, fam)
        assert p.units == row.n * p.units_x * p.units_y
        assert (p.splits - 1) * p.upw < p.units <= p.splits * p.upw, (row.id, fam)
        assert p.splits * ta.per_bytes(row) <= ta.workspace_bytes(row), (row.id, fam)
        if row.partials is not None:
            assert p.splits <= row.partials
        px = p.th * p.tw
        assert px <= ta.max_px(fam, row.stride)
        xrows = ((p.th - 1) * row.stride + row.ks) * ((p.tw - 1) * row.stride + row.ks)
        if fam == "bf16":
            assert p.pxp == (px + 15) // 16 * 16 and p.rows == p.pxp + xrows <= 512
            assert p.lds == max(p.rows * 80, 16384)
        else:
            assert p.pxp == (px + 3) // 4 * 4 and p.rows == p.pxp + xrows
            assert p.lds == p.rows * 36 * 4
        assert p.lds <= 160 * 1024


def _one(fam, rid):
    row = next(r for r in ta.ROWS if r.id == rid)
    return ta.plan(row, fam)


def test_named_geometries():
    """The shapes whose geometry was worked out by hand from the rule."""
    p = _one("f32", "k3s1-16to16-1x5x65")
    assert (p.tw, p.th, p.units_x, p.pxp - p.tw * p.th) == (33, 1, 2, 3)
    p = _one("bf16", "k3s1-16to16-1x5x65")
    assert (p.tw, p.th, p.units_x, p.pxp - p.tw * p.th, p.rows) == (33, 5, 2, 11, 421)
    p = _one("f32", "k3s2-16to16-1x9x65")
    assert (p.tw, p.units_x) == (17, 2)
    p = _one("bf16", "k3s2-16to16-1x9x65")
    assert (p.tw, p.th, p.pxp - p.tw * p.th) == (33, 1, 15)
    p = _one("bf16", "k3s1-20to36-2x3x67-p24.40")
    assert (p.tw, p.th, p.units_x) == (34, 3, 2)
    p = _one("bf16", "k3s2-32to32-1x3x133")
    assert (p.tw, p.units_x) == (34, 2)                      # wout 67
    p = _one("bf16", "k1s1-64to64-3x13x11")
    assert (p.th, p.tw * p.th) == (13, 143)
    for fam in ("f32", "bf16f32", "bf16"):
        p = _one(fam, "k3s1-32to32-2x11x23-ws4-acc")
        assert (p.units, p.upw, p.splits, p.units - (p.splits - 1) * p.upw) == (22, 6, 4, 4)
        assert _one(fam, "k3s1-32to32-2x11x23-ws1").splits == 1
    assert _one("f32", "k3s1-16to16-4x24x16").splits == 24
    assert _one("bf16", "k3s1-16to16-4x7x130").upw == 2      # the register prefetch fetch(u + 1) runs once per workgroup


def test_splits_follow_the_workspace_not_the_environment():
    """The split count is steered through workspace_bytes (UDP_POSE_WGRAD_WGS is read once per process)."""
    row = next(r for r in ta.ROWS if r.id == "k3s1-32to32-2x11x23")
    ho, wo = ta.out_hw(row)
    for fam in ta.FAMILIES:
        seen = []
        for k in (1, 2, 3, 4, 7, 22, 64):
            rc, p = ta.debug_tile(fam, row.n, row.h, row.w, row.cin_k, ho, wo, row.cout_k, row.ks, row.stride, row.cout,
                                  row.cin, k * ta.per_bytes(row))
            assert rc == 0 and p.splits <= min(k, p.units) and p.splits * p.upw >= p.units
            seen.append(p.splits)
        assert seen[0] == 1 and seen == sorted(seen) and seen[-1] == 22


def test_refusals_of_the_diagnostic_are_those_of_the_launch():
    """Host-side returns of wgrad_plan, by code (-1 UDP_ERR_ARG, -3 UDP_ERR_UNSUPPORTED) and message."""
    L = _lib.lib()
    out = (C.c_int * 11)()
    big = 1 << 20

    def call(fam, *a):
        with ta.family_env(fam):
            return L.udp_debug_wgrad_tile(*a, out)
    F32, BF = _lib.UDP_F32, _lib.UDP_BF16
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, big) == 0
    assert L.udp_debug_wgrad_tile(1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, big, None) == -1
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, 7, big) == -1 and b"dtype" in L.udp_last_error()
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, _lib.UDP_F16X2, big) == -1
    for bad in ((0, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16), (1, 8, 8, 16, 8, 8, 16, 5, 1, 16, 16), (1, 8, 8, 16, 8, 8, 16, 3, 3, 16, 16),
                (1, 8, 8, 16, 8, 8, 16, 3, 1, 17, 16), (1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 17), (1, 8, 8, 18, 8, 8, 16, 3, 1, 16, 16),
                (1, 8, 8, 16, 8, 8, 18, 3, 1, 16, 16), (1, 8, 8, 16, 8, 8, 16, 3, 1, 0, 16)):
        assert call("f32", *bad, F32, big) == -1 and b"shape" in L.udp_last_error(), bad
    # output size not matching input and stride
    for bad in ((1, 8, 8, 16, 7, 8, 16, 3, 1, 16, 16), (1, 7, 9, 16, 3, 5, 16, 3, 2, 16, 16), (1, 7, 9, 16, 4, 4, 16, 1, 2, 16, 16)):
        assert call("f32", *bad, F32, big) == -1 and b"output size" in L.udp_last_error(), bad
    assert call("f32", 1, 7, 9, 16, 4, 5, 16, 3, 2, 16, 16, F32, big) == 0          # odd input: 7 -> 4, 9 -> 5
    # a workspace smaller than one partial
    per = 9 * 16 * 16 * 4
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, per - 1) == -1 and b"smaller than one partial" in L.udp_last_error()
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, 0) == -1
    assert call("f32", 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, per) == 0 and out[7] == 1
    # a bf16 pitch that is a multiple of 4 but not of 8: the bf16 MFMA kernel refuses, the fp32 MFMA kernel takes it
    assert call("bf16", 1, 8, 8, 20, 8, 8, 16, 3, 1, 16, 20, BF, big) == -1 and b"multiples of 8" in L.udp_last_error()
    assert call("bf16", 1, 8, 8, 16, 8, 8, 12, 3, 1, 12, 16, BF, big) == -1 and b"multiples of 8" in L.udp_last_error()
    assert call("bf16f32", 1, 8, 8, 20, 8, 8, 12, 3, 1, 12, 20, BF, big) == 0 and out[0] == 2
    assert call("f32", 1, 8, 8, 20, 8, 8, 12, 3, 1, 12, 20, F32, big) == 0 and out[0] == 0
    # the two UDP_ERR_UNSUPPORTED returns (staging plan, LDS) are defensive: TW <= 64, so the largest tile TH = 1 can
    # have is a stride-2 row of 64 output pixels = 64 + 3 * 129 = 451 staged rows <= 512, and TH > 1 is only chosen
    # under the same limit; the fp32 kernel's tile is at most 64 + 66 * 3 rows of 144 bytes
    assert call("bf16", 1, 2, 128, 16, 1, 64, 16, 3, 2, 16, 16, BF, big) == 0 and out[9] == 451 and out[10] == 451 * 80
    assert call("f32", 1, 1, 64, 16, 1, 64, 16, 3, 1, 16, 16, F32, big) == 0 and out[9] == 64 + 3 * 66


def test_refusals_of_the_training_entry_points():
    """The fail(...) returns of the training entry points no other test reaches, by return code.  Each is a host-side
    return in front of the first HIP call, so host memory stands in for the device pointers and no GPU is needed."""
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p = C.addressof(buf)
    F32, BF = _lib.UDP_F32, _lib.UDP_BF16
    per = 9 * 16 * 16 * 4

    def wgrad(n, h, w, cin_k, ho, wo, cout_k, ks, stride, cout, cin, dt, ws_bytes, fam="f32"):
        with ta.family_env(fam):
            return L.udp_conv2d_wgrad(p, p, n, h, w, cin_k, ho, wo, cout_k, ks, stride, cout, cin, dt, p, 0, p, ws_bytes, None)
    assert wgrad(1, 8, 8, 20, 8, 8, 16, 3, 1, 16, 20, BF, 1 << 20, "bf16") == -1 and b"multiples of 8" in L.udp_last_error()
    assert wgrad(1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, per - 4) == -1 and b"smaller than one partial" in L.udp_last_error()
    assert wgrad(1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, BF, per - 4, "bf16f32") == -1 and b"smaller than one partial" in L.udp_last_error()
    assert wgrad(1, 7, 9, 16, 3, 5, 16, 3, 2, 16, 16, F32, 1 << 20) == -1 and b"output size" in L.udp_last_error()
    assert wgrad(1, 7, 9, 16, 4, 4, 16, 1, 2, 16, 16, BF, 1 << 20, "bf16") == -1 and b"output size" in L.udp_last_error()
    assert L.udp_conv2d_wgrad(None, p, 1, 8, 8, 16, 8, 8, 16, 3, 1, 16, 16, F32, p, 0, p, 1 << 20, None) == -1
    # 0 or 5 group members
    items = (_lib.WgradItem * 5)()
    for k in (0, 5, -1):
        assert L.udp_conv2d_wgrad_group(items, k, F32, None) == -1 and b"members (1..4)" in L.udp_last_error()
    assert L.udp_conv2d_wgrad_group(None, 1, F32, None) == -1
    bn = (_lib.BnItem * 5)()
    for k in (0, 5):
        assert L.udp_bn_train_fwd_multi(bn, k, 1e-5, 0.1, F32, None) == -1 and b"tensors (1..4)" in L.udp_last_error()
        assert L.udp_bn_train_bwd_multi(bn, k, BF, None) == -1 and b"tensors (1..4)" in L.udp_last_error()
    # `rows` out of range
    rows_max = L.udp_bn_rows_max()
    for it in bn:
        it.x = it.gamma = it.beta = it.save_mean = it.save_invstd = it.ws = it.y = it.dy = it.dgamma = it.dbeta = it.dx = p
        it.m, it.c = 4, 4
    for rows in (-1, rows_max + 1):
        bn[0].rows = rows
        assert L.udp_bn_train_fwd_multi(bn, 1, 1e-5, 0.1, F32, None) == -1 and b"partial rows" in L.udp_last_error()
        assert L.udp_bn_train_bwd_multi(bn, 1, F32, None) == -1 and b"partial rows" in L.udp_last_error()
    for rows in (0, -1, rows_max + 1):
        assert L.udp_bn_train_fwd_from_sums(p, 4, 4, p, p, 1e-5, 0.1, None, None, p, p, None, 0, p, F32, p, rows, None) == -1
        assert b"partial rows" in L.udp_last_error()
    assert L.udp_bn_train_fwd(p, 4, 6, p, p, 1e-5, 0.1, None, None, p, p, None, 0, p, F32, p, None) == -1       # c % 4
    assert L.udp_bn_train_bwd(p, p, None, 0, 4, p, p, p, p, p, p, None, F32, p, None) == -1                      # m = 0
    # a shift that does not divide the map
    for dt in (F32, BF):
        assert L.udp_ew_accumulate(p, p, 1, 12, 8, 4, 3, 1, 0, dt, None) == -1 and b"does not divide" in L.udp_last_error()
        assert L.udp_ew_accumulate(p, p, 1, 8, 12, 4, 3, 1, 0, dt, None) == -1
        assert L.udp_ew_accumulate(p, p, 1, 64, 64, 4, 6, 1, 0, dt, None) == -1
        assert L.udp_upsample_bwd(p, 1, 12, 8, 4, 3, p, 0, dt, None) == -1 and b"does not divide" in L.udp_last_error()
        assert L.udp_upsample_bwd(p, 1, 8, 8, 4, 0, p, 0, dt, None) == -1                                           # shift 0
    assert L.udp_bias_grad(p, 4, 16, 17, p, F32, None) == -1                                                     # c > pitch
    assert L.udp_nchw_to_nhwc(p, 1, 17, 2, 2, 16, p, F32, None) == -1
    assert L.udp_adam_step(p, p, p, p, 4, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, None) == -1                            # step 0
    assert L.udp_adam_step_dev(p, p, p, p, 4, 0.9, 0.999, 1e-8, None, 1.0, None) == -1
    assert L.udp_adam_coefficients(1e-3, 0.9, 0.999, 0, (C.c_float * 2)()) == -1


@pytest.mark.parametrize("fam", ta.FAMILIES)
def test_no_row_is_refused(fam):
    for row in ta.ROWS:
        if fam in row.fams:
            ta.plan(row, fam)
