"""pose_shufflenetv2_10x_pixel_shuffle on the host side, no GPU: the fp restatement against the fixture the reference's
own module produced, the model factory, the op program the planner emits (launch count, every key consumed, MACs,
write hazards), the refused configurations, and the digest of every other planner's programs (unchanged)."""
import contextlib
import io
import os
import runpy

import numpy as np
import pytest
import torch

import shufflenet_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_shufflenet import shufflenet_param_shapes, shufflenet_units, synth_shufflenet_state_dict

NAME = "pose_shufflenetv2_10x_pixel_shuffle"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(size="1.0x", target="gaussian"):
    return {"MODEL": {"NAME": NAME, "NUM_JOINTS": 17, "TARGET_TYPE": target, "IMAGE_SIZE": [192, 256],
                      "EXTRA": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": size, "FINAL_CONV_KERNEL": 1}}}


def _program(size, h, w, dtype, seed=7):
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    sd = synth_shufflenet_state_dict(seed=seed, model_size=size)
    return sd, ShuffleNetV2Program(sd, shufflenet_spec(_cfg(size)["MODEL"]["EXTRA"]), h, w, dtype)


def test_restatement_equals_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "shufflenetv2_10x_ps.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_shufflenet_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    assert sorted("%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()) == list(g["keys"])   # the weight-file contract
    assert len(sd) == 358 and sum(v.numel() for v in sd.values() if v.dim()) == 4109517
    hm = R.forward(sd, torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))).numpy()
    assert hm.shape == g["heatmaps"].shape == (1, 17, 64, 48)
    assert float(np.abs(hm - g["heatmaps"]).max()) <= 1e-5


def test_models_has_the_net():
    from udp_pose_amd.model import PoseShuffleNetV2Hip
    net = MODELS[NAME](_cfg(), is_train=False)
    assert isinstance(net, PoseShuffleNetV2Hip)
    sd = synth_shufflenet_state_dict(seed=7)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})             # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["decoder.duc.1.conv.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        net.trainer()
    with pytest.raises(NotImplementedError):
        net.train()
    with pytest.raises(NotImplementedError):
        net.init_weights()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("size,hw", [("1.0x", (256, 192)), ("0.5x", (64, 64)), ("1.5x", (96, 64))])
def test_program_census_keys_and_launch_count(size, hw, dtype):
    sd, prog = _program(size, hw[0], hw[1], dtype)
    kinds = [op["kind"] for op in prog._ops]
    assert kinds[0] == _lib.UDP_OP_STEM and kinds[1] == _lib.UDP_OP_MAXPOOL
    assert kinds.count(_lib.UDP_OP_DWCONV) == 19 and kinds.count(_lib.UDP_OP_PIXSHUF) == 3
    # stem + max-pool + 3 stride-2 units x 4 + 13 stride-1 units x 3 + conv_last + conv_compress + 3 x (DUC conv + shuffle) + head
    assert len(prog._ops) == 62 <= 65
    assert sum(1 for op in prog._ops if op["out2"]) == 13                       # one passthrough per stride-1 unit
    # every key is consumed; the ImageNet classifier and the BatchNorm step counters are accepted and unused
    assert prog.consumed_keys == set(shufflenet_param_shapes(model_size=size)) == set(sd)
    del sd["backbone.classifier.0.weight"]
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program
    assert len(ShuffleNetV2Program(sd, prog.spec, hw[0], hw[1], dtype)._ops) == 62
    head = prog._ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17 == prog.out_channels
    arr = prog.ops_array()
    assert arr[len(arr) - 1].out_buf == _lib.UDP_BUF_OUTPUT
    dw = [o for o in arr if o.kind == _lib.UDP_OP_DWCONV]
    assert all(o.cin == o.cout == o.cout_pad and o.cin % 32 == 0 and o.wfmt == 0 for o in dw)
    assert all((o.n_out2 == 1) == (o.stride == 1) and (o.chain_cout > 0) == (o.stride == 1) for o in dw)


def test_multi_writer_tensors_stay_on_one_lane():
    """Write hazards: a tensor written by several ops (the two halves of a unit output, of a stride-2 unit's depthwise
    pair) is ordered by its writers' common lane alone -- so they must share it -- and has one physical buffer."""
    _, prog = _program("1.0x", 256, 192, "f16x2")
    writers = {}
    for op in prog._ops:
        for t in ([op["out"]] if op["out"] is not None else []) + [t for t, _ in op["out2"]]:
            writers.setdefault(t.id, []).append(op)
    multi = {tid: ops for tid, ops in writers.items() if len(ops) > 1}
    assert len(multi) == 13 + 3
    for tid, ops in multi.items():
        assert len({op["lane"] for op in ops}) == 1, [op["name"] for op in ops]
        slices = sorted((op["out_coff"], op["cout"]) if op["out"] is not None and op["out"].id == tid else (0, op["cout"]) for op in ops)
        assert slices[0][0] + slices[0][1] <= slices[1][0]                      # disjoint channel ranges
    # a reader on another lane than the tensor's last writer waits for it
    last = {tid: prog._ops.index(ops[-1]) for tid, ops in writers.items()}
    for op in prog._ops:
        for t in prog._reads(op):
            w = last[t.id]
            assert prog._ops[w]["lane"] == op["lane"] or w in op["wait"], op["name"]


def test_macs_per_image_hand_count():
    """1.0x at 256x192, counted as launched (padded channel counts, the zero blocks of the merged stride-2 conv)."""
    _, prog = _program("1.0x", 256, 192, "f32")
    up = lambda c: (c + 31) // 32 * 32
    macs = 27 * 64 * 128 * 96                                                   # stem (64 stored outputs)
    h, w, cin_stored = 64, 48, 32                                               # the pooled map: 24 real channels, 32 read
    for _, inp, oup, mid, stride in shufflenet_units("1.0x"):
        cp = up(oup // 2)
        if stride == 2:
            mp = up(mid)
            macs += cin_stored * mp * h * w                                     # pw1 at the input resolution
            h, w = h // 2, w // 2
            macs += 9 * (cin_stored + mp) * h * w                               # the two depthwise convs
            macs += (cin_stored + mp) * 2 * cp * h * w                          # merged pw
        else:
            macs += 2 * cp * cp * h * w + 9 * cp * h * w + cp * cp * h * w      # pw1 (reads both halves), dw, pw2
        cin_stored = 2 * cp
    macs += cin_stored * 1024 * h * w + 1024 * 256 * h * w                      # conv_last, conv_compress
    c = 256
    for planes in (512, 256, 128):
        macs += 9 * c * planes * h * w
        c, h, w = planes // 4, 2 * h, 2 * w
    macs += c * 17 * h * w
    assert prog.macs_per_image() == macs


def test_refused_configurations():
    cfg = _cfg("2.0x")
    with pytest.raises(NotImplementedError, match="reference itself cannot run"):
        MODELS[NAME](cfg, is_train=False)
    with pytest.raises(ValueError, match="f32, f16x2"):
        MODELS[NAME](_cfg(), is_train=False, dtype="bf16")
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    with pytest.raises(ValueError, match="no bf16 form"):
        ShuffleNetV2Program(synth_shufflenet_state_dict(seed=1), shufflenet_spec({}), 256, 192, "bf16")
    bad = _cfg()
    bad["MODEL"]["EXTRA"]["ARCHITECTURE"] = (512, 256, 100)
    with pytest.raises(NotImplementedError, match="ARCHITECTURE"):
        MODELS[NAME](bad, is_train=False)


def test_existing_program_digests_unchanged(golden_dir):
    """tools/program_digest.py over the 66 configurations of the other planners prints what it printed before this
    net existed (tests/golden/program_digest_66.txt): their programs are byte-identical."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "tools", "program_digest.py"), run_name="__main__")
    with open(os.path.join(golden_dir, "program_digest_66.txt")) as f:
        want = f.read()
    assert len(want.splitlines()) == 66
    assert buf.getvalue() == want
