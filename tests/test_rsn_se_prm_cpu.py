"""Host side of the three op kinds of RSN-18 "se + prm" (include/udp_pose_hip.h, kinds 20 - 22), without a GPU: the
binding and the header agree on the kind numbers, and udp_conv2d_fused refuses what the header says it refuses with the
documented code.  Every call here is refused by the argument rules, which run before the first HIP call; the pointers
are host addresses that are never dereferenced."""
import ctypes as C
import os
import re

from udp_pose_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE, GATE, DW9 = _lib.UDP_OP_SE_RES, _lib.UDP_OP_PRM_GATE, _lib.UDP_OP_PRM_DW9
ARG, UNSUP = -1, -3


def test_kind_numbers_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "udp_pose_hip.h")).read()
    kinds = {k: int(v) for k, v in re.findall(r"\b(UDP_OP_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    assert (kinds["UDP_OP_SE_RES"], kinds["UDP_OP_PRM_GATE"], kinds["UDP_OP_PRM_DW9"]) == (SE, GATE, DW9) == (20, 21, 22)
    assert sorted(kinds.values()) == list(range(23)), "the next free kind numbers, no gap"
    assert _lib.ABI_VERSION == 20 and "#define UDP_POSE_ABI_VERSION 20" in hdr


def _op(kind, c=32, h=8, w=6, **fields):
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride = kind, 1, 1
    op.in_buf = op.out_buf = op.res_buf = op.chain_buf = _lib.UDP_BUF_NONE
    op.cin = op.cout = op.cout_pad = c
    op.hin, op.win, op.hout, op.wout = h, w, h, w
    if kind == SE:
        op.chain_cout = 8
    if kind == DW9:
        op.ks, op.n_up = 9, 1
    for k, v in fields.items():
        setattr(op, k, v)
    return op


def _caller():
    mem = (C.c_float * 64)()
    base = C.addressof(mem)
    ptrs = dict(inp=base, wgt=base + 16, bias=base + 32, res=base + 48, up0=base + 64, out=base + 80)
    lib = _lib.lib()

    def call(op, dtype=_lib.UDP_F32, res=False, up0=False, out="out"):
        rc = lib.udp_conv2d_fused(C.byref(op), dtype, 1, ptrs["inp"], ptrs["wgt"], ptrs["bias"], ptrs["res"] if res else None,
                                  ptrs["up0"] if up0 else None, None, None, ptrs[out], None)
        return rc, lib.udp_last_error().decode()
    return call, mem


def test_bf16_is_unsupported_for_all_three():
    call, _mem = _caller()
    for kind, kw, what in ((SE, {}, "se + residual"), (GATE, {}, "prm channel gate"), (DW9, dict(res=True, up0=True), "prm spatial gate")):
        rc, msg = call(_op(kind), _lib.UDP_BF16, **kw)
        assert rc == UNSUP and what in msg and "f32 and f16x2" in msg, (kind, rc, msg)
        assert call(_op(kind), 7, **kw)[0] == ARG                               # no such storage mode


def test_shape_rules():
    call, _mem = _caller()
    both = dict(res=True, up0=True)
    for kind, kw in ((SE, {}), (GATE, {}), (DW9, both)):
        assert call(_op(kind, c=48), **kw)[0] == ARG                            # C not a multiple of 32
        assert call(_op(kind, hout=4), **kw)[0] == ARG                          # output size != input size
        assert call(_op(kind, in_coff=4, in_pitch=64), **kw)[0] == ARG          # views in multiples of 8
    for ch in (0, 257, -1):
        rc, msg = call(_op(SE, c=512, chain_cout=ch))
        assert rc == ARG and "hidden width" in msg
    assert call(_op(SE, c=544))[0] == ARG and call(_op(GATE, c=288))[0] == ARG  # beyond 512 / 256 channels
    assert call(_op(GATE, chain_cout=8))[0] == ARG
    assert call(_op(DW9, stride=2, hout=4, wout=3), **both)[0] == ARG           # stride 2
    for ks in (3, 7, 11):
        assert call(_op(DW9, ks=ks), **both)[0] == ARG
    assert call(_op(DW9, n_up=0), **both)[0] == ARG and call(_op(DW9, n_up=2), **both)[0] == ARG


def test_operand_and_aliasing_rules():
    call, _mem = _caller()
    both = dict(res=True, up0=True)
    assert call(_op(DW9), out="inp", **both)[0] == ARG and call(_op(DW9), out="res", **both)[0] == ARG      # out must not be in / res
    assert call(_op(DW9), res=True)[0] == ARG and call(_op(DW9), up0=True)[0] == ARG                        # both operands are needed
    assert call(_op(GATE), res=True)[0] == ARG and call(_op(GATE), out="inp")[0] == ARG
    rc, msg = call(_op(SE, in_pitch=64, out_pitch=64, out_coff=32), out="inp")                               # in place through another view
    assert rc == ARG and "same view" in msg
    assert call(_op(SE), res=True, out="res")[0] == ARG


def test_activation_codes():
    call, _mem = _caller()
    both = dict(res=True, up0=True)
    assert call(_op(GATE, relu=1))[0] == UNSUP and call(_op(DW9, relu=1), **both)[0] == UNSUP               # their activations are fixed
    assert call(_op(SE, relu=2))[0] == UNSUP and call(_op(SE, relu=4))[0] == UNSUP                          # none | ReLU only
    for kind, kw in ((SE, {}), (GATE, {}), (DW9, both)):
        assert call(_op(kind, relu=3), **kw)[0] == ARG and call(_op(kind, relu=-1), **kw)[0] == ARG
        assert call(_op(kind, n_out2=1), **kw)[0] == UNSUP and call(_op(kind, group=1), **kw)[0] == UNSUP


# ------------------------------------------------------------------ planner, model, key contract, fixture
import json      # noqa: E402

import numpy as np      # noqa: E402
import pytest           # noqa: E402
import torch            # noqa: E402

import rsn_se_prm_ref as ref                       # noqa: E402
from udp_pose_amd import synth                     # noqa: E402
from udp_pose_amd.model import RSN18Hip            # noqa: E402
from udp_pose_amd.rsn_plan import RSNProgram       # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture_state_dict():
    g = np.load(os.path.join(GOLDEN, "rsn18_se_prm_17.npz"))
    calib = {k[len("calib:"):]: g[k] for k in g.files if k.startswith("calib:")}
    return synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=calib), g["out"]


def test_key_contract_is_the_reference_modules():
    """Names, order and shapes of the module that tools/gen_golden_rsn_se_prm.py composes from the reference's classes."""
    keys = json.load(open(os.path.join(GOLDEN, "rsn18_se_prm_keys_17.json")))
    want = synth.rsn18_se_prm_param_shapes(17)
    assert list(keys) == list(want)
    assert all(tuple(keys[k]) == tuple(want[k]) for k in keys)
    assert tuple(want["stage0.downsample.layer3.1.se.fc.0.weight"]) == (32, 256) and tuple(want["stage0.downsample.layer3.1.se.fc.2.weight"]) == (256, 32)
    assert tuple(want["stage0.upsample.up4.prm.conv_bn_relu_prm_3_2.conv.weight"]) == (256, 1, 9, 9)
    assert "stage0.upsample.up4.prm.conv_bn_relu_prm_3_2.conv.bias" in want
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4)
    assert list(sd) == list(want) and all(tuple(sd[k].shape) == tuple(want[k]) for k in want)


def test_restatement_fp64_matches_the_reference_output():
    """|fp64 restatement - reference fp32| within the fp32-vs-fp64 noise of this fixture (x2, + 1e-5: the rule of the GPU test)."""
    sd, out = fixture_state_dict()
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    r64 = ref.forward(ref.to_dtype(sd, torch.float64), x.double()).numpy()
    r32 = ref.forward(sd, x).numpy()
    noise = float(np.abs(r32 - r64).max())
    err = float(np.abs(out - r64).max())
    print("se+prm fixture: |ref fp32 - fp64| %.3g, |restatement fp32 - fp64| %.3g (absmax %.3g)" % (err, noise, float(np.abs(out).max())))
    assert 0 < err <= 2.0 * noise + 1e-5


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_program_census(dtype):
    """One UDP_OP_SE_RES per Bottleneck (layers [2, 2, 2, 2]: 8) and the PRM's four launches on top of plain RSN-18; each
    flag alone adds its own share; the SE runs in place on conv_bn_relu3's output with the shortcut as res and the ReLU on."""
    plain = len(RSNProgram(synth.synth_rsn18_state_dict(17, seed=4), 256, 192, dtype)._ops)
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4)
    prog = RSNProgram(sd, 256, 192, dtype, se=True, prm=True)
    kinds = [op["kind"] for op in prog._ops]
    assert (kinds.count(SE), kinds.count(GATE), kinds.count(DW9)) == (8, 1, 1)
    assert len(kinds) == plain + 8 + 4
    assert len(RSNProgram(sd, 256, 192, dtype, se=True)._ops) == plain + 8
    for i, op in enumerate(prog._ops):
        if op["kind"] == SE:
            c3 = prog._ops[i - 1] if prog._ops[i - 1]["name"].endswith("conv_bn_relu3") else prog._ops[i - 2]
            assert c3["name"].endswith("conv_bn_relu3") and c3["relu"] == 0 and c3["res"] is None
            assert op["inp"] is op["out"] is c3["out"] and op["res"] is not None and op["relu"] == 1 and op["chain_cout"] == op["cin"] // 8
    names = [op["name"].rsplit(".", 1)[-1] for op in prog._ops]
    i = names.index("conv_bn_relu_prm_1")
    assert names[i:i + 5] == ["conv_bn_relu_prm_1", "gate", "conv_bn_relu_prm_3_1", "conv_bn_relu_prm_3_2", "res_conv1"]
    dw = prog._ops[i + 3]
    assert dw["inp"] is prog._ops[i + 2]["out"] and dw["res"] is prog._ops[i]["out"] and dw["ups"][0][0] is prog._ops[i + 1]["out"]
    assert prog._ops[i + 4]["inp"] is dw["out"]
    arr = prog.ops_array()
    d = [o for o in arr if o.kind == DW9][0]
    assert d.n_up == 1 and d.up_shift[0] == 0 and len({d.in_buf, d.res_buf, d.out_buf, d.up_buf[0]}) == 4


def test_model_constructs_and_refuses():
    net = RSN18Hip(17, se=True, prm=True)
    assert list(net.param_shapes()) == list(synth.rsn18_se_prm_param_shapes(17))
    assert list(RSN18Hip(17).param_shapes()) == list(synth.rsn18_param_shapes(17))
    for kw in (dict(se=True), dict(prm=True)):
        with pytest.raises(ValueError, match="f32.*f16x2"):
            RSN18Hip(17, dtype="bf16", **kw)
        with pytest.raises(ValueError, match="f32.*f16x2"):
            RSNProgram(synth.synth_rsn18_se_prm_state_dict(17, seed=1), 256, 192, "bf16", **kw)
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=1)
    for key, shape in (("stage0.downsample.layer1.0.se.fc.0.weight", None), ("stage0.downsample.layer2.1.se.fc.2.weight", (128, 8)),
                       ("stage0.upsample.up4.prm.conv_bn_relu_prm_3_2.conv.weight", (256, 1, 7, 7)),
                       ("stage0.upsample.up4.prm.conv_bn_relu_prm_2_1.conv.weight", None)):
        bad = dict(sd)
        if shape is None:
            del bad[key]
        else:
            bad[key] = torch.zeros(shape)
        with pytest.raises((ValueError, RuntimeError), match="mismatch|must be|shape"):
            RSN18Hip(17, se=True, prm=True).load_state_dict(bad)
        with pytest.raises((ValueError, KeyError)):
            RSNProgram(bad, 256, 192, "f32", se=True, prm=True)
