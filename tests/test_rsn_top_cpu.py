"""Host side of RSN-18 on the stem of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm (``stem="conv7"``), without a GPU: the tile
choice and the refusals of the 7x7 conv (udp_debug_conv_tile: host arithmetic only), the planner's op sequence and buffer
lifetimes, the key contract, ``RSN18Hip.from_state_dict`` and strict loading."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import rsn_top_ref as ref
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import RSN18Hip
from udp_pose_amd.rsn_plan import RSNProgram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARG, UNSUP = -1, -3
F32, BF16, H2 = _lib.UDP_F32, _lib.UDP_BF16, _lib.UDP_F16X2


def _tile(dtype, wfmt, ks, stride, n, h, w, cin, cout):
    out = (C.c_int * 9)()
    rc = _lib.lib().udp_debug_conv_tile(dtype, wfmt, ks, stride, n, h, w, cin, cout, 0, 0, out)
    return rc, list(out), _lib.lib().udp_last_error().decode()


@pytest.mark.parametrize("dtype", [F32, H2])
@pytest.mark.parametrize("shape", [(128, 128, 96, 64, 64), (3, 9, 7, 64, 64), (2, 13, 37, 48, 48), (1, 1, 1, 16, 16), (1, 24, 40, 64, 64),
                                   (1, 32, 32, 64, 64), (64, 16, 16, 32, 128)])
def test_tile_choice_covers_the_map_within_the_lds(dtype, shape):
    """out[] for ks 7 (include/udp_pose_hip.h): NB, pixel blocks per wave, G, R, TW, one-halo-buffer flag, LDS bytes, workgroups."""
    n, h, w, cin, cout = shape
    rc, o, msg = _tile(dtype, 0, 7, 1, *shape)
    assert rc == _lib.UDP_OK, msg
    nb, mbw, g, r, tw, one, lds, wgs = o[:8]
    cout_pad = (cout + 31) // 32 * 32
    assert nb in (2, 4) and cout_pad % (16 * nb) == 0
    assert 1 <= g <= n and 1 <= r <= h and 1 <= tw <= w and (g == 1 or (r == h and tw == w))
    assert g * r * tw <= 256 and mbw == -(-(-(-g * r * tw // 16)) // 4) and 1 <= mbw <= 4
    rows = g * (r + 6) * (tw + 6)
    assert rows <= 640
    planes = 2 if dtype == H2 else 1
    halo = (rows + 15) // 16 * 16 * 64 * planes * (1 if one else 2)
    assert lds == halo + 2 * planes * 7 * nb * 16 * 64 and lds <= 163840
    assert wgs == -(-n // g) * -(-h // r) * -(-w // tw) * (cout_pad // (16 * nb))        # the tiles cover the map
    assert one == (1 if dtype == H2 or cin <= 16 else 0)


def test_tile_choice_of_the_stem_conv():
    """The shapes of a batch-64 flip step: 128 images of 128 x 96, 64 -> 64."""
    _, f, _ = _tile(F32, 0, 7, 1, 128, 128, 96, 64, 64)
    _, h, _ = _tile(H2, 0, 7, 1, 128, 128, 96, 64, 64)
    assert f[:6] == [4, 4, 1, 8, 32, 0] and h[:6] == [4, 3, 1, 10, 16, 1]


def test_what_the_7x7_conv_does_not_do_is_refused():
    for dtype in (F32, H2):
        rc, _, msg = _tile(dtype, 0, 7, 2, 1, 8, 8, 64, 64)
        assert rc == UNSUP and "stride 1" in msg
        rc, _, msg = _tile(dtype, 1, 7, 1, 1, 8, 8, 64, 64)
        assert rc in (UNSUP, ARG) and "wfmt" in msg
        assert _tile(dtype, 0, 7, 1, 1, 8, 8, 24, 64)[0] == UNSUP and _tile(dtype, 0, 7, 1, 1, 8, 8, 64, 24)[0] == UNSUP
    rc, _, msg = _tile(BF16, 0, 7, 1, 1, 8, 8, 64, 64)
    assert rc == UNSUP and "f32 and f16x2" in msg
    assert _tile(F32, 0, 5, 1, 1, 8, 8, 64, 64)[0] == ARG
    out = (C.c_int * 9)()
    assert _lib.lib().udp_debug_conv_tile(H2, 0, 7, 1, 1, 8, 8, 64, 64, 0, 1, out) == 1        # no merged launch has a 7x7 member


def test_single_op_entry_refuses_before_any_launch():
    """udp_conv2d_fused with ks 7: the argument rules run before the first HIP call (host pointers, never dereferenced)."""
    mem = (C.c_float * 64)()
    base = C.addressof(mem)
    lib = _lib.lib()

    def call(dtype=F32, res=False, **fields):
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride = _lib.UDP_OP_CONV, 7, 1
        op.in_buf = op.out_buf = op.res_buf = op.chain_buf = _lib.UDP_BUF_NONE
        op.cin = op.cout = op.cout_pad = 64
        op.hin = op.win = op.hout = op.wout = 8
        for k, v in fields.items():
            setattr(op, k, v)
        rc = lib.udp_conv2d_fused(C.byref(op), dtype, 1, base, base + 16, base + 32, base + 48 if res else None, None, None, None, base + 64, None)
        return rc, lib.udp_last_error().decode()

    assert call(BF16)[0] == UNSUP and call(res=True)[0] == UNSUP
    for fields in (dict(n_out2=1), dict(chain_cout=64), dict(group=1), dict(wfmt=1), dict(in_stuff2=1), dict(relu=2), dict(relu=4),
                   dict(out_buf=_lib.UDP_BUF_OUTPUT), dict(stride=2, hout=4, wout=4), dict(cin=24), dict(cout=24)):
        for dtype in (F32, H2):
            rc, msg = call(dtype, **fields)
            assert rc == UNSUP, (fields, rc, msg)
    assert call(hout=7)[0] == ARG and call(ks=5)[0] == ARG


# ------------------------------------------------------------------ planner
def _assert_hazards_ordered(prog):
    """tests/test_host_cpu.py's rule: every RAW / WAR / WAW pair on a physical buffer is ordered by lane order + wait lists."""
    ops = prog.ops_array()
    n = len(ops)
    hb, last = [0] * n, {}
    for i, o in enumerate(ops):
        m = 0
        for j in [o.wait_op[k] for k in range(o.n_wait)] + ([last[o.lane]] if o.lane in last else []):
            assert j < i
            m |= hb[j] | (1 << j)
        hb[i] = m
        last[o.lane] = i
    touched = {}
    for i, o in enumerate(ops):
        reads = [b for b in [o.in_buf, o.res_buf] + [o.up_buf[u] for u in range(o.n_up)] + [o.add2_buf[k] for k in range(o.n_out2)] if b >= 0]
        writes = ([o.out_buf] if o.out_buf >= 0 else []) + [o.out2_buf[k] for k in range(o.n_out2)]
        assert o.ks == 1 or o.kind != _lib.UDP_OP_CONV or not (set(writes) & set(reads)), "op %d: a k x k conv writes a buffer it reads" % i
        for b in reads:
            for j, kind in touched.get(b, []):
                assert kind == "r" or (hb[i] >> j) & 1, "unordered RAW on buffer %d: op %d -> %d" % (b, j, i)
        for b in writes:
            for j, kind in touched.get(b, []):
                assert (hb[i] >> j) & 1, "unordered WA%s on buffer %d: op %d -> %d" % (kind.upper(), b, j, i)
        for b in reads:
            touched.setdefault(b, []).append((i, "r"))
        for b in writes:
            touched.setdefault(b, []).append((i, "w"))
    return n


@pytest.mark.parametrize("size", [(256, 192), (64, 64)])
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_program_head_and_lifetimes(dtype, size):
    H, W = size
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, stem="conv7")
    prog = RSNProgram(sd, H, W, dtype, se=True, prm=True, stem="conv7")
    pool = RSNProgram(synth.synth_rsn18_se_prm_state_dict(17, seed=4), H, W, dtype, se=True, prm=True)
    head = prog._ops[:3]
    assert [(o["kind"], o["ks"], o["stride"], o["cin"], o["cout"], o["relu"]) for o in head] == [
        (_lib.UDP_OP_STEM, 3, 2, 3, 64, 1), (_lib.UDP_OP_CONV, 7, 1, 64, 64, 1), (_lib.UDP_OP_CONV, 3, 2, 64, 64, 1)]
    assert [o["name"] for o in head] == ["top.conv.0", "top.conv.1", "top.conv.2"]
    assert (head[1]["hout"], head[1]["wout"]) == (H // 2, W // 2) and (head[2]["hout"], head[2]["wout"]) == (H // 4, W // 4)
    assert head[1]["wfmt"] == 0 and head[2]["wfmt"] == (1 if dtype == "f16x2" else 0)
    assert head[1]["inp"] is head[0]["out"] and head[2]["inp"] is head[1]["out"] and prog._ops[3]["inp"] is head[2]["out"]
    assert head[1]["res"] is None and not head[1]["ups"] and not head[1]["out2"] and head[1]["group"] == 0
    assert not any(o["kind"] in (_lib.UDP_OP_MAXPOOL, _lib.UDP_OP_STEM7) for o in prog._ops)
    assert [o["name"] for o in prog._ops[3:]] == [o["name"] for o in pool._ops[2:]]                 # everything behind the stem is unchanged
    launches = _assert_hazards_ordered(prog)
    assert launches == len(pool._ops) + 1
    print("rsn18 se+prm conv7 stem %s %dx%d: %d launches (pool stem %d)" % (dtype, H, W, launches, len(pool._ops)))
    assert prog.macs_per_image() - pool.macs_per_image() == (
        (H // 2) * (W // 2) * 64 * (27 + 49 * 64) + (H // 4) * (W // 4) * 64 * 9 * 64 - (H // 2) * (W // 2) * 64 * 147)
    arr = prog.ops_array()
    assert arr[1].ks == 7 and arr[1].in_buf == arr[0].out_buf and arr[1].out_buf not in (arr[1].in_buf, _lib.UDP_BUF_OUTPUT)


def test_stem_goes_with_or_without_the_gates_and_needs_f32_or_f16x2():
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=1, se=False, prm=False, stem="conv7")
    plain = RSNProgram(synth.synth_rsn18_state_dict(17, seed=1), 64, 64, "f32")
    prog = RSNProgram(sd, 64, 64, "f32", stem="conv7")
    assert len(prog._ops) == len(plain._ops) + 1 and _assert_hazards_ordered(prog)
    for make in (lambda: RSNProgram(sd, 64, 64, "bf16", stem="conv7"), lambda: RSN18Hip(17, dtype="bf16", stem="conv7")):
        with pytest.raises(ValueError, match="f32.*f16x2"):
            make()
    for make in (lambda: RSNProgram(sd, 64, 64, "f32", stem="conv5"), lambda: RSN18Hip(17, stem="conv5"),
                 lambda: synth.rsn18_se_prm_param_shapes(17, stem="conv5")):
        with pytest.raises(ValueError, match="pool.*conv7"):
            make()
    bad = dict(sd)
    bad["top.conv.1.conv.weight"] = torch.zeros(64, 64, 5, 5)
    with pytest.raises(ValueError, match="top.conv.1"):
        RSNProgram(bad, 64, 64, "f32", stem="conv7")


# ------------------------------------------------------------------ key contract, loader
def _fixture_keys():
    return json.load(open(os.path.join(GOLDEN, "rsn18_se_prm_top_keys_17.json")))


def test_key_contract_is_the_experiments_own_module():
    keys = _fixture_keys()
    want = synth.rsn18_se_prm_param_shapes(17, stem="conv7")
    assert list(keys) == list(want) and all(tuple(keys[k]) == tuple(want[k]) for k in keys)
    assert tuple(want["top.conv.0.conv.weight"]) == (64, 3, 3, 3) and tuple(want["top.conv.1.conv.weight"]) == (64, 64, 7, 7)
    assert tuple(want["top.conv.2.conv.weight"]) == (64, 64, 3, 3) and "top.conv.conv.weight" not in want
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, stem="conv7")
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == tuple(want[k]) for k in want)


def test_default_arguments_are_untouched():
    old = json.load(open(os.path.join(GOLDEN, "rsn18_se_prm_keys_17.json")))
    want = synth.rsn18_se_prm_param_shapes(17)
    assert list(old) == list(want) and all(tuple(old[k]) == tuple(want[k]) for k in old)
    a, b = synth.synth_rsn18_se_prm_state_dict(17, seed=4), synth.synth_rsn18_se_prm_state_dict(17, seed=4, stem="pool")
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    g = np.load(os.path.join(GOLDEN, "rsn18_se_prm_17.npz"))                     # the pool-stem fixture still describes these tensors
    assert float(np.abs(g["calib:top.conv.bn.running_var"]).max()) > 0 and tuple(a["top.conv.conv.weight"].shape) == (64, 3, 7, 7)


def test_from_state_dict_reads_the_flags_off_the_checkpoint():
    cases = [(synth.synth_rsn18_state_dict(17, seed=2), (False, False, "pool", 17)),
             (synth.synth_rsn18_state_dict(51, seed=2), (False, False, "pool", 51)),
             (synth.synth_rsn18_se_prm_state_dict(17, seed=2), (True, True, "pool", 17)),
             (synth.synth_rsn18_se_prm_state_dict(17, seed=2, stem="conv7"), (True, True, "conv7", 17)),
             (synth.synth_rsn18_se_prm_state_dict(51, seed=2, prm=False, stem="conv7"), (True, False, "conv7", 51))]
    for sd, want in cases:
        for wrap in (lambda d: d, lambda d: {"module." + k: v for k, v in d.items()}):
            net = RSN18Hip.from_state_dict(wrap(sd), dtype="f16x2")
            assert (net.se, net.prm, net.stem, net.out_channels) == want and net.chl_num == 256 and net.dtype == "f16x2"
            assert net._sd is not None and list(net.param_shapes()) == list(sd)
    with pytest.raises(ValueError, match="RSN-18"):
        RSN18Hip.from_state_dict({"conv1.weight": torch.zeros(1)})
    bad = synth.synth_rsn18_se_prm_state_dict(17, seed=2, stem="conv7")
    bad["top.conv.1.conv.weight"] = torch.zeros(64, 64, 3, 3)
    with pytest.raises(ValueError, match="top.conv.1"):
        RSN18Hip.from_state_dict(bad)
    mixed = synth.synth_rsn18_se_prm_state_dict(17, seed=2, stem="conv7")
    mixed.update({k: v for k, v in synth.synth_rsn18_state_dict(17, seed=2).items() if k.startswith("top.")})
    with pytest.raises(RuntimeError, match="unexpected"):
        RSN18Hip.from_state_dict(mixed)


def test_strict_loading_of_the_experiments_key_set():
    keys = _fixture_keys()
    sd = {k: torch.zeros(shape, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, shape in keys.items()}
    net = RSN18Hip(17, se=True, prm=True, stem="conv7").load_state_dict(sd, strict=True)
    assert net._sd is not None
    with pytest.raises(RuntimeError, match="missing.*top.conv.conv.*unexpected.*top.conv.0"):
        RSN18Hip(17, se=True, prm=True, stem="pool").load_state_dict(sd, strict=True)
    plain = synth.synth_rsn18_se_prm_state_dict(17, seed=1)
    with pytest.raises(RuntimeError, match="missing.*top.conv.0.*unexpected.*top.conv.conv"):
        RSN18Hip(17, se=True, prm=True, stem="conv7").load_state_dict(plain, strict=True)


# ------------------------------------------------------------------ fixture
def test_restatement_fp64_matches_the_reference_output():
    """|fp64 restatement - the module's fp32 output| within the fp32-vs-fp64 noise of this fixture (x2, + 1e-5: the rule of
    the GPU test), and the fixture sees the 48 off-centre taps of the 7x7 conv."""
    g = np.load(os.path.join(GOLDEN, "rsn18_se_prm_top_17.npz"))
    calib = {k[len("calib:"):]: g[k] for k in g.files if k.startswith("calib:")}
    assert not any(k.startswith("top.conv.bn") for k in calib) and "top.conv.1.bn.running_var" in calib and "final.scale" in calib
    assert not any("weight" in k or k.endswith(".bias") for k in calib), "the fixture holds no weights"
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=calib, stem="conv7")
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    sd64 = ref.to_dtype(sd, torch.float64)
    r64 = ref.forward(sd64, x.double()).numpy()
    r32 = ref.forward(sd, x).numpy()
    noise = float(np.abs(r32 - r64).max())
    err = float(np.abs(g["out"] - r64).max())
    print("se+prm top fixture: |ref fp32 - fp64| %.3g, |restatement fp32 - fp64| %.3g (absmax %.3g)" % (err, noise, float(np.abs(g["out"]).max())))
    assert 0 < err <= 2.0 * noise + 1e-5
    centre = float(np.abs(ref.forward(sd64, x.double(), centre_only=True).numpy() - r64).max())
    assert centre > 100 * 3e-3, centre
