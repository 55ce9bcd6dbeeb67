"""pose_mobilenetv3_small_pixel_shuffle / pose_mobilenetv3_small on the host side, no GPU: the model factory, the
weight-file contract (the block table of torchvision's mobilenet_v3_small().features), the op program the planner
emits (census derived from the table, MACs, BatchNorm eps of the fold, every key consumed) and the refused
configurations."""
import numpy as np
import pytest
import torch

import mobilenetv3_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilenetv3 import (BLOCKS, mobilenetv3_deconv_param_shapes, mobilenetv3_ps_param_shapes,
                                            synth_mobilenetv3_state_dict)

PS, DECONV = "pose_mobilenetv3_small_pixel_shuffle", "pose_mobilenetv3_small"
EXTRA = {PS: {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1},
         DECONV: {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
                  "NUM_DECONV_KERNELS": [4, 4, 4], "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1}}
HEAD = {PS: "pixel_shuffle", DECONV: "deconv"}
# the issue's table, restated here on purpose: (in, k, exp, out, SE, act, stride) of backbone.0.1 .. backbone.0.11
TABLE = [(16, 3, 16, 16, 1, "RE", 2), (16, 3, 72, 24, 0, "RE", 2), (24, 3, 88, 24, 0, "RE", 1), (24, 5, 96, 40, 1, "HS", 2),
         (40, 5, 240, 40, 1, "HS", 1), (40, 5, 240, 40, 1, "HS", 1), (40, 5, 120, 48, 1, "HS", 1), (48, 5, 144, 48, 1, "HS", 1),
         (48, 5, 288, 96, 1, "HS", 2), (96, 5, 576, 96, 1, "HS", 1), (96, 5, 576, 96, 1, "HS", 1)]
SQUEEZE = [8, 24, 64, 64, 32, 40, 72, 144, 144]


def _cfg(name, **extra):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": dict(EXTRA[name], **extra)}}


def _ru(c):
    return (c + 31) // 32 * 32


def _bn(keys, p, c):
    keys += [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)),
             (p + ".num_batches_tracked", ())]


def _table_keys():
    """Backbone keys and shapes in registration order, written out from the table."""
    keys = [("backbone.0.0.0.weight", (16, 3, 3, 3))]
    _bn(keys, "backbone.0.0.1", 16)
    sq = iter(SQUEEZE)
    for i, (cin, k, exp, cout, se, act, s) in enumerate(TABLE, start=1):
        p, m = "backbone.0.%d.block." % i, 0
        if exp != cin:
            keys.append((p + "%d.0.weight" % m, (exp, cin, 1, 1)))
            _bn(keys, p + "%d.1" % m, exp)
            m += 1
        keys.append((p + "%d.0.weight" % m, (exp, 1, k, k)))
        _bn(keys, p + "%d.1" % m, exp)
        m += 1
        if se:
            q = next(sq)
            keys += [(p + "%d.fc1.weight" % m, (q, exp, 1, 1)), (p + "%d.fc1.bias" % m, (q,)),
                     (p + "%d.fc2.weight" % m, (exp, q, 1, 1)), (p + "%d.fc2.bias" % m, (exp,))]
            m += 1
        keys.append((p + "%d.0.weight" % m, (cout, exp, 1, 1)))
        _bn(keys, p + "%d.1" % m, cout)
    keys.append(("backbone.0.12.0.weight", (576, 96, 1, 1)))
    _bn(keys, "backbone.0.12.1", 576)
    return keys


def test_kind_23_follows_the_header():
    """The header defines the kind as the successor of the last numbered one (UDP_OP_PRM_DW9 = 22): 23, no gap, the
    value the binding uses; csrc/dwconv.hip holds the same as a static_assert.  The ABI version stays."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "udp_pose_hip.h")).read()
    numbered = {k: int(v) for k, v in re.findall(r"\b(UDP_OP_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    assert re.search(r"\bUDP_OP_SE_ACT\s*=\s*UDP_OP_PRM_DW9\s*\+\s*1\b", hdr)
    assert numbered["UDP_OP_PRM_DW9"] == max(numbered.values()) == 22 and _lib.UDP_OP_SE_ACT == numbered["UDP_OP_PRM_DW9"] + 1 == 23
    assert _lib.ABI_VERSION == 20 and "#define UDP_POSE_ABI_VERSION 20" in hdr


def test_models_has_all_four_names():
    for name in (PS, DECONV, "pose_shufflenetv2_10x", "pose_shufflenetv2_plus"):
        assert name in MODELS                                                   # KeyError before these nets existed
    assert len(MODELS) == 12
    from udp_pose_amd.model import PoseMobileNetV3Hip, PoseMobileNetV3PixelShuffleHip
    for name, cls in ((PS, PoseMobileNetV3PixelShuffleHip), (DECONV, PoseMobileNetV3Hip)):
        net = MODELS[name](_cfg(name), is_train=False)
        assert type(net) is cls and net.DTYPES == ("f32", "f16x2") and net.NAME == name
        with pytest.raises(NotImplementedError):
            net.init_weights()
        with pytest.raises(NotImplementedError):
            net.train()


@pytest.mark.parametrize("name", [PS, DECONV])
def test_param_shapes_equal_the_table(name):
    shapes = MODELS[name](_cfg(name), is_train=False).param_shapes()
    bb = [(k, tuple(v)) for k, v in shapes.items() if k.startswith("backbone.")]
    assert bb == _table_keys()                                                  # key for key, in order
    assert all(k.startswith("backbone.0.") for k, _ in bb)
    assert sum(int(np.prod(v)) for k, v in bb if "running_" not in k and "num_batches" not in k) == 927008
    head = [(k, tuple(v)) for k, v in shapes.items() if not k.startswith("backbone.")]
    if name == PS:
        assert head[0] == ("decoder.conv_compress.weight", (256, 576, 1, 1)) and head[1] == ("decoder.duc.0.conv.weight", (512, 256, 3, 3))
        assert shapes == mobilenetv3_ps_param_shapes()
    else:
        assert [k for k, _ in head if k.endswith(".weight") and "deconv" in k] == ["deconv_layers.%d.weight" % i for i in (0, 1, 3, 4, 6, 7)]
        assert head[0] == ("deconv_layers.0.weight", (576, 256, 4, 4)) and "deconv_layers.0.bias" not in shapes
        assert shapes == mobilenetv3_deconv_param_shapes()
    assert head[-2:] == [("final_layer.weight", (17, 32 if name == PS else 256, 1, 1)), ("final_layer.bias", (17,))]


def _hand_macs(name, h, w):
    """MACs of the emitted program from the table: stored channels (round_up(c, 32), the stem's 64) -- what the kernels
    execute and udp_hrnet_flops_per_image counts --, the two products of every squeeze-excitation included.  Beside it
    the real-channel conv count of the backbone, the figure of the net's description."""
    h, w = h // 2, w // 2
    stored, real = 27 * 64 * h * w, 27 * 16 * h * w
    sq = iter(SQUEEZE)
    for cin, k, exp, cout, se, act, s in TABLE:
        if exp != cin:
            stored, real = stored + _ru(cin) * _ru(exp) * h * w, real + cin * exp * h * w
        h, w = (h - 1) // s + 1, (w - 1) // s + 1
        stored, real = stored + k * k * _ru(exp) * h * w, real + k * k * exp * h * w
        if se:
            stored += 2 * _ru(exp) * next(sq)
        stored, real = stored + _ru(exp) * _ru(cout) * h * w, real + exp * cout * h * w
    stored, real = stored + 96 * 576 * h * w, real + 96 * 576 * h * w
    if name == PS:
        stored += 576 * 256 * h * w
        cin = 256
        for planes in (512, 256, 128):
            stored += 9 * cin * planes * h * w
            cin, h, w = planes // 4, 2 * h, 2 * w
        stored += cin * 17 * h * w                                              # final_layer
    else:
        cin = 576
        for planes in (256, 256, 256):
            h, w = 2 * h, 2 * w
            stored += 4 * cin * planes * h * w
            cin = planes
        stored += cin * 17 * h * w
    return stored, real


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("name", [PS, DECONV])
def test_program_census_at_256x192(name, dtype):
    sd = synth_mobilenetv3_state_dict(seed=7, head=HEAD[name])
    net = MODELS[name](_cfg(name), is_train=False, dtype=dtype).load_state_dict(sd)
    prog = net._make_program(256, 192)
    ops = prog._ops
    kinds = [op["kind"] for op in ops]
    assert kinds[0] == _lib.UDP_OP_STEM and ops[0]["relu"] == _lib.UDP_ACT_HSWISH and ops[0]["cout"] == 64
    # depthwise convs: ks / stride from the table, code 1 in RE blocks and 0 in HS blocks (the activation rides in SE_ACT)
    dw = [op for op in ops if op["kind"] == _lib.UDP_OP_DWCONV]
    assert [(op["ks"], op["stride"], op["relu"], op["cin"]) for op in dw] == \
        [(k, s, 1 if act == "RE" else 0, _ru(exp)) for _, k, exp, _, _, act, s in TABLE] and len(dw) == 11
    se = [op for op in ops if op["kind"] == _lib.UDP_OP_SE_ACT]
    with_se = [t for t in TABLE if t[4]]
    assert [(op["cin"], op["chain_cout"], op["relu"]) for op in se] == \
        [(_ru(exp), q, 0 if act == "RE" else 2) for (_, _, exp, _, _, act, _), q in zip(with_se, SQUEEZE)] and len(se) == 9
    assert all(op["inp"] is op["out"] and op["in_coff"] == op["out_coff"] == 0 and op["res"] is None for op in se)       # in place
    assert _lib.UDP_OP_ACT not in kinds and _lib.UDP_OP_SE not in kinds and _lib.UDP_OP_MAXPOOL not in kinds
    convs = [op for op in ops if op["kind"] == _lib.UDP_OP_CONV and op["name"].startswith("backbone.")]
    proj = [op for op in convs if op["res"] is not None]
    assert [int(op["name"].split(".")[2]) for op in proj] == [3, 5, 6, 8, 10, 11]
    assert all(op["relu"] == 0 and op["ks"] == 1 for op in proj)
    expand = [op for op in convs if op["relu"] != 0 and op["name"] != "backbone.0.12.0"]
    assert [op["relu"] for op in expand] == [1 if act == "RE" else 2 for cin, _, exp, _, _, act, _ in TABLE if exp != cin] and len(expand) == 10
    assert len(convs) == 10 + 11 + 1 and convs[-1]["relu"] == _lib.UDP_ACT_HSWISH and convs[-1]["cout"] == 576
    assert (convs[-1]["hout"], convs[-1]["wout"]) == (8, 6)                     # 576 x H/32 x W/32
    assert len(ops) == (51 if name == PS else 47)
    assert kinds.count(_lib.UDP_OP_DECONV) == (0 if name == PS else 3) and kinds.count(_lib.UDP_OP_PIXSHUF) == (3 if name == PS else 0)
    head = ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and (head["hout"], head["wout"]) == (64, 48) and head["cout"] == 17
    assert prog.ops_array()[len(ops) - 1].out_buf == _lib.UDP_BUF_OUTPUT
    stored, real = _hand_macs(name, 256, 192)
    assert real == 53326848                                                     # the backbone's 53.33 MMAC (real channels, convs only)
    assert prog.macs_per_image() == stored
    assert prog.consumed_keys == set(sd)                                        # every key is an operand or BatchNorm bookkeeping


def test_fold_uses_eps_1e_3_in_the_backbone_and_1e_5_in_the_head():
    from udp_pose_amd.mobilenetv3_plan import MobileNetV3Program, mobilenetv3_ps_spec
    sd = synth_mobilenetv3_state_dict(seed=3)
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k] = torch.rand(sd[k].shape) * 0.01 + 1e-4                       # small variances: eps decides the scale
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(sd[k].shape)
    prog = MobileNetV3Program(sd, mobilenetv3_ps_spec(EXTRA[PS]), 64, 64, "f32")
    blob = prog.weight_blob()

    def bias_of(name, n):
        op = next(op for op in prog._ops if op["name"] == name)
        return np.frombuffer(blob[op["b_off"]:op["b_off"] + 4 * n].tobytes(), dtype=np.float32)

    def hand(bn, eps):
        f = lambda s: sd[bn + s].double()
        return (f(".bias") - f(".running_mean") * f(".weight") / torch.sqrt(f(".running_var") + eps)).float().numpy()
    got = bias_of("backbone.0.2.block.0.0", 72)
    np.testing.assert_array_equal(got, hand("backbone.0.2.block.0.1", 1e-3))
    assert np.abs(got - hand("backbone.0.2.block.0.1", 1e-5)).max() > 1e-2
    duc = bias_of("decoder.duc.0.conv", 512)
    want = hand("decoder.duc.0.bn", 1e-5)
    np.testing.assert_array_equal(duc[[(o % 4) * 128 + o // 4 for o in range(512)]], want)      # stored in pixel-shuffle order
    assert np.abs(want - hand("decoder.duc.0.bn", 1e-3)).max() > 1e-2


def test_restatement_reads_the_same_table():
    """The arbiter of the GPU tests walks the keys, not the planner's table: its output is 576 x H/32 x W/32, and its
    strides / activations agree with the table."""
    assert R.STRIDES == tuple(t[6] for t in TABLE) == tuple(b[6] for b in BLOCKS)
    assert [i + 1 for i, t in enumerate(TABLE) if t[5] == "HS"] == list(range(R.HS_FROM, 12))
    assert [tuple(b[:4]) + (int(b[4]),) + tuple(b[5:]) for b in BLOCKS] == TABLE
    sd = synth_mobilenetv3_state_dict(seed=7)
    y = R.backbone(sd, torch.from_numpy(synth.synth_crops(1, 64, 96, seed=1)))
    assert tuple(y.shape) == (1, 576, 2, 3)
    assert tuple(R.forward(sd, torch.from_numpy(synth.synth_crops(1, 64, 96, seed=1))).shape) == (1, 17, 16, 24)


def test_refusals():
    for name in (PS, DECONV):
        with pytest.raises(NotImplementedError, match="MODEL_SIZE='large'.*960"):
            MODELS[name](_cfg(name, MODEL_SIZE="large"), is_train=False)
        with pytest.raises(NotImplementedError, match="bf16"):
            MODELS[name](_cfg(name), is_train=False, dtype="bf16")
        with pytest.raises(NotImplementedError, match="FINAL_CONV_KERNEL"):
            MODELS[name](_cfg(name, FINAL_CONV_KERNEL=5), is_train=False)
    from udp_pose_amd.mobilenetv3_plan import MobileNetV3Program, mobilenetv3_ps_spec
    with pytest.raises(NotImplementedError, match="no bf16 form"):
        MobileNetV3Program(synth_mobilenetv3_state_dict(seed=7), mobilenetv3_ps_spec(EXTRA[PS]), 64, 64, "bf16")
    with pytest.raises(NotImplementedError, match="ARCHITECTURE"):
        MODELS[PS](_cfg(PS, ARCHITECTURE=(512, 256)), is_train=False)
    with pytest.raises(NotImplementedError, match="START_CHANNELS"):
        MODELS[PS](_cfg(PS, START_CHANNELS=100), is_train=False)
    with pytest.raises(NotImplementedError, match="NUM_DECONV_LAYERS"):
        MODELS[DECONV](_cfg(DECONV, NUM_DECONV_LAYERS=2, NUM_DECONV_FILTERS=[256, 256], NUM_DECONV_KERNELS=[4, 4]), is_train=False)
    with pytest.raises(NotImplementedError, match="NUM_DECONV_KERNELS"):
        MODELS[DECONV](_cfg(DECONV, NUM_DECONV_KERNELS=[4, 3, 4]), is_train=False)


@pytest.mark.parametrize("name", [PS, DECONV])
def test_unknown_and_missing_keys(name):
    net = MODELS[name](_cfg(name), is_train=False)
    sd = synth_mobilenetv3_state_dict(seed=7, head=HEAD[name])
    net.load_state_dict({"module." + k: v for k, v in sd.items()})             # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["backbone.0.4.block.2.fc2.bias"]
    with pytest.raises(RuntimeError, match=r"missing \['backbone.0.4.block.2.fc2.bias'\]"):
        net.load_state_dict(bad)
    with pytest.raises(RuntimeError, match=r"unexpected \['backbone.1.weight'\]"):
        net.load_state_dict(dict(sd, **{"backbone.1.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="size mismatch for backbone.0.1.block.1.fc1.weight"):
        net.load_state_dict(dict(sd, **{"backbone.0.1.block.1.fc1.weight": torch.zeros(8, 16)}))
