"""pose_shufflenetv2_plus_pixel_shuffle on the host side, no GPU: the fp restatement against the fixture the reference's
own module produced, the model factory, the op program the planner emits (launch count and kinds, activation codes,
passthroughs, every key consumed, MACs, write hazards) and the refused configurations."""
import collections
import os

import numpy as np
import pytest
import torch

import shufflenet_plus_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_shufflenet_plus import (ARCHITECTURE, shufflenet_plus_param_shapes, shufflenet_plus_units,
                                                synth_shufflenet_plus_state_dict)

NAME = "pose_shufflenetv2_plus_pixel_shuffle"


def _cfg(size="Small", target="gaussian"):
    return {"MODEL": {"NAME": NAME, "NUM_JOINTS": 17, "TARGET_TYPE": target, "IMAGE_SIZE": [192, 256],
                      "EXTRA": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": size, "FINAL_CONV_KERNEL": 1}}}


def _program(size, h, w, dtype, seed=7):
    from udp_pose_amd.shufflenet_plus_plan import ShuffleNetV2PlusProgram, shufflenet_plus_spec
    sd = synth_shufflenet_plus_state_dict(seed=seed, model_size=size)
    return sd, ShuffleNetV2PlusProgram(sd, shufflenet_plus_spec(_cfg(size)["MODEL"]["EXTRA"]), h, w, dtype)


def test_restatement_equals_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "shufflenetv2_plus_small_ps.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_shufflenet_plus_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    assert sorted("%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()) == list(g["keys"])   # the weight-file contract
    # 549 backbone keys (the reference backbone's own count) + conv_compress + 3 x 6 DUC + 2 head
    assert len(sd) == 570 and sum(1 for k in sd if k.startswith("backbone.")) == 549
    assert sum(v.numel() for v in sd.values() if v.dim()) == 7035805
    # what sum(p.numel() for p in backbone.parameters()) gives on the reference's Small backbone
    assert sum(v.numel() for k, v in sd.items() if k.startswith("backbone.") and v.dim() and "running_" not in k) == 5137116
    hm = R.forward(sd, torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))).numpy()
    assert hm.shape == g["heatmaps"].shape == (1, 17, 64, 48)
    assert float(np.abs(hm - g["heatmaps"]).max()) <= 1e-5


def test_models_has_the_net():
    net = MODELS[NAME](_cfg(), is_train=False)                                  # KeyError before this net existed
    from udp_pose_amd.model import PoseShuffleNetV2PlusHip
    assert isinstance(net, PoseShuffleNetV2PlusHip)
    sd = synth_shufflenet_plus_state_dict(seed=7)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})             # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["backbone.features.9.branch_main.8.SE_opr.1.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        net.trainer()
    with pytest.raises(NotImplementedError):
        net.train()
    with pytest.raises(NotImplementedError):
        net.init_weights()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("size,hw", [("Small", (256, 192)), ("Small", (64, 64)), ("Medium", (64, 64)), ("Large", (96, 64))])
def test_program_census_keys_and_launch_count(size, hw, dtype):
    sd, prog = _program(size, hw[0], hw[1], dtype)
    ops = prog._ops
    kinds = [op["kind"] for op in ops]
    assert kinds[0] == _lib.UDP_OP_STEM and kinds.count(_lib.UDP_OP_STEM) == 1 and _lib.UDP_OP_MAXPOOL not in kinds
    # hand count: stem 1 + stage 0 (4 + 3 + 6 + 3 = 16) + stage 1 (4 + 3 + 3 + 3 = 13) + stage 2 (5 + 7 x 4 = 33) +
    # stage 3 (5 + 4 + 7 + 4 = 20) + conv_last 1 + conv_compress 1 + 3 x (DUC conv + shuffle) 6 + head 1
    assert len(ops) == 1 + 16 + 13 + 33 + 20 + 1 + 1 + 6 + 1 == 92
    assert kinds.count(_lib.UDP_OP_SE) == 12 and kinds.count(_lib.UDP_OP_PIXSHUF) == 3
    # depthwise ops by kernel size: a stride-2 unit has two of its size, a Shufflenet stride-1 unit one, Xception three 3x3
    want = collections.Counter()
    for _, _, _, _, stride, block, _, _ in shufflenet_plus_units(size):
        want[3 if block == 3 else 3 + 2 * block] += 3 if block == 3 else stride
    assert want == {3: 14, 5: 7, 7: 7}
    assert collections.Counter(op["ks"] for op in ops if op["kind"] == _lib.UDP_OP_DWCONV) == want
    assert kinds.count(_lib.UDP_OP_CONV) == 92 - 1 - 28 - 12 - 3
    # activation code 2: the stem, every 1x1 conv of the units of stages 1-3 (ReLU in stage 0), conv_last -- and nothing else
    hs = [op["name"] for op in ops if op["relu"] == _lib.UDP_ACT_HSWISH]
    unit_convs = lambda lo, hi: [op for op in ops if op["kind"] == _lib.UDP_OP_CONV and op["name"].startswith("backbone.features.")
                                 and lo <= int(op["name"].split(".")[2]) < hi]
    assert all(op["relu"] == _lib.UDP_ACT_RELU for op in unit_convs(0, 4)) and len(unit_convs(0, 4)) == 2 + 2 + 3 + 2
    assert all(op["relu"] == _lib.UDP_ACT_HSWISH for op in unit_convs(4, 20)) and len(unit_convs(4, 20)) == 16 * 2 + 1
    assert sorted(hs) == sorted(["backbone.first_conv.0", "backbone.conv_last.0"] + [op["name"] for op in unit_convs(4, 20)]) and len(hs) == 35
    assert all(op["relu"] == 0 for op in ops if op["kind"] in (_lib.UDP_OP_DWCONV, _lib.UDP_OP_SE, _lib.UDP_OP_PIXSHUF))
    assert all(op["ks"] == 1 and op["stride"] == 1 and op["res"] is None and not op["ups"] and not op["group"]
               for op in ops if op["relu"] == _lib.UDP_ACT_HSWISH and op["kind"] == _lib.UDP_OP_CONV)
    assert sum(1 for op in ops if op["out2"]) == 16                              # one passthrough per stride-1 unit
    # every key is consumed or explicitly accepted and unused (the ImageNet tail, the BatchNorm step counters)
    assert prog.consumed_keys == set(shufflenet_plus_param_shapes(model_size=size)) == set(sd)
    assert {k for k in prog.unused_keys if not k.endswith("num_batches_tracked")} == {
        "backbone.LastSE.SE_opr.1.weight", "backbone.LastSE.SE_opr.2.weight", "backbone.LastSE.SE_opr.2.bias",
        "backbone.LastSE.SE_opr.2.running_mean", "backbone.LastSE.SE_opr.2.running_var", "backbone.LastSE.SE_opr.4.weight",
        "backbone.fc.0.weight", "backbone.classifier.0.weight"}
    for k in list(sd):
        if k.startswith(("backbone.LastSE.", "backbone.fc.", "backbone.classifier.")):
            del sd[k]
    from udp_pose_amd.shufflenet_plus_plan import ShuffleNetV2PlusProgram
    assert len(ShuffleNetV2PlusProgram(sd, prog.spec, hw[0], hw[1], dtype)._ops) == 92
    head = ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17 == prog.out_channels
    arr = prog.ops_array()
    assert arr[len(arr) - 1].out_buf == _lib.UDP_BUF_OUTPUT
    dw = [o for o in arr if o.kind == _lib.UDP_OP_DWCONV]
    assert all(o.cin == o.cout == o.cout_pad and o.cin % 32 == 0 and o.wfmt == 0 for o in dw)
    assert all((o.chain_cout > 0) == (o.n_out2 == 1) and (o.n_out2 == 0 or o.stride == 1) for o in dw)
    se = [o for o in arr if o.kind == _lib.UDP_OP_SE]
    assert all(o.in_buf == o.out_buf and o.in_coff == o.out_coff == o.cin and o.in_pitch == o.out_pitch == 2 * o.cin
               and o.cin % 32 == 0 and 1 <= o.chain_cout <= o.cin // 4 for o in se)


def test_multi_writer_tensors_stay_on_one_lane():
    """Write hazards: a tensor written by several ops (the two halves of a unit output, of a stride-2 unit's depthwise
    pair, and the squeeze-excitation that rewrites the main half IN PLACE) is ordered by its writers' common lane alone
    -- so they must share it -- and has one physical buffer.  Slices are disjoint, except that an SE op owns exactly
    the slice its predecessor (the 1x1 conv of the main branch) wrote, or the main half of the merged conv's output."""
    _, prog = _program("Small", 256, 192, "f16x2")
    writers = {}
    for op in prog._ops:
        for t in ([op["out"]] if op["out"] is not None else []) + [t for t, _ in op["out2"]]:
            writers.setdefault(t.id, []).append(op)
    multi = {tid: ops for tid, ops in writers.items() if len(ops) > 1}
    # 16 stride-1 unit outputs + 4 depthwise pairs + the 2 stride-2 unit outputs of the SE stages (merged conv, then SE)
    assert len(multi) == 16 + 4 + 2
    n_se = 0
    for tid, ops in multi.items():
        assert len({op["lane"] for op in ops}) == 1, [op["name"] for op in ops]
        se = [op for op in ops if op["kind"] == _lib.UDP_OP_SE]
        rest = [op for op in ops if op["kind"] != _lib.UDP_OP_SE]
        slices = sorted((op["out_coff"], op["cout"]) if op["out"] is not None and op["out"].id == tid else (0, op["cout"]) for op in rest)
        for a, b in zip(slices, slices[1:]):
            assert a[0] + a[1] <= b[0]                                          # disjoint channel ranges
        for op in se:                                                           # in place: reads what it writes, after its producer
            n_se += 1
            assert op is ops[-1] and op["inp"] is op["out"] and (op["in_coff"], op["in_pitch"]) == (op["out_coff"], op["out_pitch"])
            assert op["out_coff"] == op["cout"] and op["out_pitch"] == 2 * op["cout"]
            prev = ops[-2]
            assert prev["kind"] == _lib.UDP_OP_CONV and prev["out_coff"] <= op["out_coff"] and \
                prev["out_coff"] + prev["cout"] >= op["out_coff"] + op["cout"]
    assert n_se == 12
    assert len(set(prog._phys[tid] for tid in multi)) <= len(multi)
    # a reader on another lane than the tensor's last writer waits for it
    last = {tid: prog._ops.index(ops[-1]) for tid, ops in writers.items()}
    for i, op in enumerate(prog._ops):
        for t in prog._reads(op):
            w = last[t.id]
            assert w == i or prog._ops[w]["lane"] == op["lane"] or w in op["wait"], op["name"]


def test_macs_per_image_hand_count():
    """Small at 256x192, counted as launched (padded channel counts, the zero blocks of the merged stride-2 conv, the
    whole stored tensor under the first depthwise conv of an Xception unit)."""
    _, prog = _program("Small", 256, 192, "f32")
    up = lambda c: (c + 31) // 32 * 32
    macs = 27 * 64 * 128 * 96                                                   # stem (64 stored outputs)
    h, w, cin_stored = 128, 96, 32                                              # no max-pool; 16 real channels, 32 read
    for idx, inp, oup, mid, stride, block, act, se in shufflenet_plus_units("Small"):
        cp = up(oup // 2)
        kk = 9 if block == 3 else (3 + 2 * block) ** 2
        if stride == 2:
            mp = up(mid)
            macs += cin_stored * mp * h * w                                     # pw1 at the input resolution
            h, w = h // 2, w // 2
            macs += kk * (cin_stored + mp) * h * w                              # the two depthwise convs
            macs += (cin_stored + mp) * 2 * cp * h * w                          # merged pw
        elif block == 3:
            macs += 9 * 2 * cp * h * w + 2 * cp * cp * h * w                    # dw over both halves, pw1 (reads both halves)
            macs += 2 * (9 * cp * h * w + cp * cp * h * w)                      # 2 x (dw, pw)
        else:
            macs += 2 * cp * cp * h * w + kk * cp * h * w + cp * cp * h * w     # pw1 (reads both halves), dw, pw2
        if se:
            macs += 2 * cp * ((oup // 2) // 4)                                  # W1 mean, W2 h (stored channels x real hidden width)
        cin_stored = 2 * cp
    assert (h, w) == (8, 6)
    macs += cin_stored * 1280 * h * w + 1280 * 256 * h * w                      # conv_last, conv_compress
    c = 256
    for planes in (512, 256, 128):
        macs += 9 * c * planes * h * w
        c, h, w = planes // 4, 2 * h, 2 * w
    macs += c * 17 * h * w
    assert prog.macs_per_image() == macs
    assert len(ARCHITECTURE) == 20


def test_refused_configurations():
    with pytest.raises(NotImplementedError, match="MODEL_SIZE"):
        MODELS[NAME](_cfg("1.0x"), is_train=False)
    with pytest.raises(ValueError, match="f32, f16x2"):
        MODELS[NAME](_cfg(), is_train=False, dtype="bf16")
    from udp_pose_amd.shufflenet_plus_plan import ShuffleNetV2PlusProgram, shufflenet_plus_spec
    with pytest.raises(ValueError, match="no bf16 form"):
        ShuffleNetV2PlusProgram(synth_shufflenet_plus_state_dict(seed=1), shufflenet_plus_spec({}), 256, 192, "bf16")
    for key, val in (("ARCHITECTURE", (512, 256, 100)), ("ARCHITECTURE", (512, 256)), ("START_CHANNELS", 200), ("FINAL_CONV_KERNEL", 5)):
        bad = _cfg()
        bad["MODEL"]["EXTRA"][key] = val
        with pytest.raises(NotImplementedError, match=key):
            MODELS[NAME](bad, is_train=False)


def test_shufflenetv2_planner_is_untouched():
    """The sibling planner shares ``_dw`` / ``_pw`` with this one: it still refuses a 5x5 depthwise weight and still
    emits 62 ops with 3x3 depthwise convs only."""
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    from udp_pose_amd.synth_shufflenet import synth_shufflenet_state_dict
    sd = synth_shufflenet_state_dict(seed=7, model_size="0.5x")
    prog = ShuffleNetV2Program(sd, shufflenet_spec({"MODEL_SIZE": "0.5x"}), 64, 64, "f32")
    assert len(prog._ops) == 62 and {op["ks"] for op in prog._ops if op["kind"] == _lib.UDP_OP_DWCONV} == {3}
    assert all(op["relu"] in (0, 1) for op in prog._ops)
    sd["backbone.features.1.branch_main.3.weight"] = torch.zeros(24, 1, 5, 5)
    with pytest.raises(ValueError):
        ShuffleNetV2Program(sd, shufflenet_spec({"MODEL_SIZE": "0.5x"}), 64, 64, "f32")
