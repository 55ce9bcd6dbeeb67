"""pose_mobilevitv2_pixel_shuffle on the host side, no GPU: the restatement against the fixture the reference's own
module produced, the weight-file contract, the model factory, the op program the planner emits (launch count and kinds,
activation codes, residuals, the attention unit's seven launches, every key consumed, MACs) and the refused
configurations."""
import collections
import os

import numpy as np
import pytest
import torch

import mobilevitv2_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilevitv2 import mobilevitv2_param_shapes, mobilevitv2_widths, synth_mobilevitv2_state_dict

NAME = "pose_mobilevitv2_pixel_shuffle"
S = _lib.UDP_ACT_SILU


def _cfg(size=0.5, target="gaussian", **model):
    return {"MODEL": dict({"NAME": NAME, "NUM_JOINTS": 17, "TARGET_TYPE": target, "IMAGE_SIZE": [192, 256],
                           "EXTRA": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": size, "FINAL_CONV_KERNEL": 1}},
                          **model)}


def _program(size, h, w, dtype, seed=7):
    from udp_pose_amd.mobilevitv2_plan import MobileViTv2Program, mobilevitv2_spec
    sd = synth_mobilevitv2_state_dict(seed=seed, model_size=size)
    return sd, MobileViTv2Program(sd, mobilevitv2_spec(_cfg(size)["MODEL"]["EXTRA"]), h, w, dtype)


def test_restatement_equals_reference_fixture(golden_dir):
    """The fixture holds the reference module's fp64 forward (tools/gen_golden_mobilevitv2.py: its fp32 forward is 2.5e-5
    away from that, more than this bound), so the restatement runs in fp64 too; the fp32 restatement stays within the
    reference's own fp32 error of it."""
    g = np.load(os.path.join(golden_dir, "mobilevitv2_05_ps.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_mobilevitv2_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    assert sorted("%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()) == list(g["keys"])   # the weight-file contract
    # 290 keys, 2,996,366 elements: what the reference's 0.5 module registers
    assert len(sd) == 290 and sum(v.numel() for v in sd.values()) == 2996366
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    hm = R.forward(sd, x, dtype=torch.float64).numpy()
    assert hm.shape == g["heatmaps"].shape == (1, 17, 64, 48)
    assert float(np.abs(hm - g["heatmaps"]).max()) <= 1e-5
    assert float(np.abs(R.forward(sd, x).numpy() - g["heatmaps"]).max()) <= 1e-4


def test_map_form_equals_unfold_form():
    """What the HIP program relies on: GroupNorm + the attention core on the map equal the reference's
    unfold -> [B, C, P, N] -> fold form (mobilevitv2.py:1026-1055, :671-689) to the last bit in fp64."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    b, c, h, w = 2, 24, 8, 6
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64) + 3
    gam, bet = torch.randn(c, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    qkv = torch.randn(b, 1 + 2 * c, h, w, generator=g, dtype=torch.float64)
    unfold = lambda t: F.unfold(t, kernel_size=(2, 2), stride=(2, 2)).reshape(b, t.shape[1], 4, -1)
    fold = lambda p: F.fold(p.reshape(b, p.shape[1] * 4, -1), output_size=(h, w), kernel_size=(2, 2), stride=(2, 2))
    assert torch.equal(fold(unfold(x)), x)
    gn = lambda t: F.group_norm(t, 1, gam, bet, 1e-5)
    assert float((fold(gn(unfold(x))) - gn(x)).abs().max()) <= 1e-13
    q, k, v = torch.split(unfold(qkv), [1, c, c], dim=1)
    ref = F.relu(v) * (k * F.softmax(q, dim=-1)).sum(dim=-1, keepdim=True)
    got = R.linear_attention_core(qkv[:, :1], qkv[:, 1:1 + c], qkv[:, 1 + c:])
    assert float((fold(ref) - got).abs().max()) <= 1e-13


def test_models_has_the_net():
    net = MODELS[NAME](_cfg(CONFIG="experiments/coco/mobilevitv2/mobilevitv2-0.5.yaml"), is_train=False)   # KeyError before this net existed; MODEL.CONFIG is ignored
    from udp_pose_amd.model import PoseMobileViTv2Hip
    assert isinstance(net, PoseMobileViTv2Hip)
    sd = synth_mobilevitv2_state_dict(seed=7)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})             # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["backbone.layer_4.1.global_rep.2.pre_norm_attn.1.qkv_proj.block.conv.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    for refused in (net.trainer, net.train, net.init_weights):                 # training is refused by name
        with pytest.raises(NotImplementedError, match=NAME):
            refused()


def test_widths_follow_the_reference_configuration():
    assert mobilevitv2_widths(0.5) == (16, 32, 64, [(128, 64, 128, 2), (192, 96, 192, 4), (256, 128, 256, 3)])
    assert mobilevitv2_widths(0.75) == (24, 48, 96, [(192, 96, 192, 2), (288, 144, 288, 4), (384, 192, 384, 3)])
    assert mobilevitv2_widths(1.0) == (32, 64, 128, [(256, 128, 256, 2), (384, 192, 384, 4), (512, 256, 512, 3)])
    # element counts of the reference module's state_dict at 0.75 and 1.0
    assert sum(int(np.prod(s)) for s in mobilevitv2_param_shapes(model_size=0.75).values()) == 4528438
    assert sum(int(np.prod(s)) for s in mobilevitv2_param_shapes(model_size=1.0).values()) == 6600926


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(256, 192), (64, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", [0.5, 0.75, 1.0])
def test_program_census_keys_and_launch_count(size, hw, dtype):
    from udp_pose_amd.mobilevitv2_plan import N_LAUNCHES, MobileViTv2Program
    sd, prog = _program(size, hw[0], hw[1], dtype)
    ops = prog._ops
    kinds = [op["kind"] for op in ops]
    c0, c1, c2, mit = mobilevitv2_widths(size)
    # hand count: stem 1 + layer 1 (3) + layer 2 (3 + 3) + layers 3-5 (3 + [dw, 1x1, 7 per attention unit, norm, proj])
    # + conv_compress 1 + 3 x (DUC conv + shuffle) 6 + head 1
    assert len(ops) == 1 + 3 + 6 + sum(3 + 2 + 7 * n + 2 for _, _, _, n in mit) + 1 + 6 + 1 == 102 == N_LAUNCHES
    assert kinds[0] == _lib.UDP_OP_STEM and collections.Counter(kinds) == {
        _lib.UDP_OP_STEM: 1, _lib.UDP_OP_CONV: 59, _lib.UDP_OP_DWCONV: 9, _lib.UDP_OP_GNORM: 21, _lib.UDP_OP_LINATTN: 9,
        _lib.UDP_OP_PIXSHUF: 3}
    # every attention unit: GNORM, qkv conv, LINATTN, out_proj + residual, GNORM, ffn + SiLU, ffn + residual
    at = [i for i, k in enumerate(kinds) if k == _lib.UDP_OP_LINATTN]
    for i in at:
        u = ops[i - 2:i + 5]
        assert [o["kind"] for o in u] == [_lib.UDP_OP_GNORM, _lib.UDP_OP_CONV, _lib.UDP_OP_LINATTN, _lib.UDP_OP_CONV, _lib.UDP_OP_GNORM,
                                          _lib.UDP_OP_CONV, _lib.UDP_OP_CONV]
        assert [o["relu"] for o in u] == [0, 0, 0, 0, 0, S, 0]
        assert u[3]["res"] is u[0]["inp"] and u[6]["res"] is u[3]["out"] and u[4]["inp"] is u[3]["out"]
        dp = u[2]["cout"]
        assert u[2]["ks"] == 2 and u[2]["cin"] == u[1]["cout"] == 2 * dp + 32 and dp % 32 == 0 and u[2]["hout"] % 2 == 0 and u[2]["wout"] % 2 == 0
        assert u[0]["chain_cout"] == u[4]["chain_cout"] and u[0]["out"] is not u[0]["inp"]
    dims = [d for _, d, _, n in mit for _ in range(n)]
    assert [ops[i - 2]["chain_cout"] for i in at] == dims                        # GroupNorm gets the REAL channel count
    assert [ops[i]["cout"] for i in at] == [(d + 31) // 32 * 32 for d in dims]
    # SiLU: the stem, the two first convs of every InvertedResidual, the depthwise conv of every MobileViT block, the first
    # ffn conv of every unit -- and no conv with a residual
    silu = [op for op in ops if op["relu"] == S]
    assert len(silu) == 1 + 6 * 2 + 3 + 9 and all(op["res"] is None and op["kind"] in (_lib.UDP_OP_STEM, _lib.UDP_OP_CONV, _lib.UDP_OP_DWCONV) for op in silu)
    assert all(op["ks"] == 1 and op["stride"] == 1 for op in silu if op["kind"] == _lib.UDP_OP_CONV)
    assert all(op["relu"] == S for op in ops if op["kind"] == _lib.UDP_OP_DWCONV)
    assert {op["relu"] for op in ops} == {0, 1, S}
    assert sum(1 for op in ops if op["res"] is not None) == 1 + 2 * 9             # layer_2.1 + two per attention unit
    assert [op["stride"] for op in ops if op["kind"] == _lib.UDP_OP_DWCONV] == [1, 2, 1, 2, 1, 2, 1, 2, 1]
    # every key is consumed or explicitly accepted and unused (the ImageNet classifier, the BatchNorm step counters)
    assert prog.consumed_keys == set(mobilevitv2_param_shapes(model_size=size)) == set(sd)
    assert {k for k in prog.unused_keys if not k.endswith("num_batches_tracked")} == {"backbone.classifier.1.weight", "backbone.classifier.1.bias"}
    for k in list(sd):
        if k.startswith("backbone.classifier."):
            del sd[k]
    assert len(MobileViTv2Program(sd, prog.spec, hw[0], hw[1], dtype)._ops) == 102
    head = ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17 == prog.out_channels
    arr = prog.ops_array()
    assert arr[len(arr) - 1].out_buf == _lib.UDP_BUF_OUTPUT
    assert all(o.cin == o.cout == o.cout_pad and o.cin % 32 == 0 and 1 <= o.chain_cout <= o.cin and o.in_buf != o.out_buf
               for o in arr if o.kind == _lib.UDP_OP_GNORM)
    assert all(o.cin % 32 == 0 and o.cout_pad % 32 == 0 for o in arr if o.kind == _lib.UDP_OP_CONV)
    # a reader on another lane than its producer waits for it
    producer = {}
    for i, op in enumerate(ops):
        for t in prog._reads(op):
            w = producer[t.id]
            assert ops[w]["lane"] == op["lane"] or w in op["wait"], op["name"]
        if op["out"] is not None:
            producer[op["out"].id] = i


def test_macs_per_image_hand_count():
    """0.5 at 256x192, counted as launched (padded channel counts)."""
    _, prog = _program(0.5, 256, 192, "f32")
    up = lambda c: (c + 31) // 32 * 32
    c0, c1, c2, mit = mobilevitv2_widths(0.5)
    macs = 27 * 64 * 128 * 96                                                   # stem (64 stored outputs)
    h, w = 128, 96

    def inverted_residual(cin_stored, cin, cout, stride, h, w):
        hid = up(2 * cin)
        m = cin_stored * hid * h * w
        h, w = h // stride, w // stride
        return m + 9 * hid * h * w + hid * up(cout) * h * w, h, w
    m, h, w = inverted_residual(32, c0, c1, 1, h, w)
    macs += m
    cin = c1
    for cout, stride in ((c2, 2), (c2, 1)):
        m, h, w = inverted_residual(up(cin), cin, cout, stride, h, w)
        macs += m
        cin = cout
    for out, d, ffn, n in mit:
        m, h, w = inverted_residual(up(cin), cin, out, 2, h, w)
        macs += m
        o, dp, fp = up(out), up(d), up(ffn)
        macs += 9 * o * h * w + o * dp * h * w                                  # local_rep
        macs += n * (dp * (2 * dp + 32) + dp + dp * dp + 2 * dp * fp) * h * w   # qkv, the weighted sum, out_proj, ffn
        macs += dp * o * h * w                                                  # conv_proj
        cin = out
    assert (h, w) == (8, 6)
    macs += up(cin) * 256 * h * w                                               # conv_compress
    c = 256
    for planes in (512, 256, 128):
        macs += 9 * c * planes * h * w
        c, h, w = planes // 4, 2 * h, 2 * w
    macs += c * 17 * h * w
    assert prog.macs_per_image() == macs


def test_refused_configurations():
    """Every refusal is a NotImplementedError that names the net."""
    for size in (2.0, 0.25, "Small"):
        with pytest.raises(NotImplementedError, match=NAME + " MODEL_SIZE"):
            MODELS[NAME](_cfg(size), is_train=False)
    with pytest.raises(NotImplementedError, match=NAME + ".*bf16"):
        MODELS[NAME](_cfg(), is_train=False, dtype="bf16")
    from udp_pose_amd.mobilevitv2_plan import MobileViTv2Program, mobilevitv2_spec
    sd = synth_mobilevitv2_state_dict(seed=1)
    with pytest.raises(NotImplementedError, match=NAME + ".*bf16"):
        MobileViTv2Program(sd, mobilevitv2_spec({}), 256, 192, "bf16")
    for h, w in ((224, 192), (256, 160), (96, 96)):                             # multiples of 32 whose 1/32 map is odd
        with pytest.raises(NotImplementedError, match=NAME + ".*multiples of 64"):
            MobileViTv2Program(sd, mobilevitv2_spec({}), h, w, "f32")
    net = MODELS[NAME](_cfg(), is_train=False)
    for refused in (net.trainer, net.train, net.init_weights):
        with pytest.raises(NotImplementedError, match=NAME):
            refused()
    for key, val in (("ARCHITECTURE", (512, 256, 100)), ("ARCHITECTURE", (512, 256)), ("START_CHANNELS", 200), ("FINAL_CONV_KERNEL", 5)):
        bad = _cfg()
        bad["MODEL"]["EXTRA"][key] = val
        with pytest.raises(NotImplementedError, match=key):
            MODELS[NAME](bad, is_train=False)


def test_sibling_planners_are_untouched():
    """``_pw`` / ``_dw`` gained a residual and an activation argument: the ShuffleNetV2 planners' programs are the same
    (tests/golden/program_digest_66.txt holds the other nets')."""
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    from udp_pose_amd.synth_shufflenet import synth_shufflenet_state_dict
    sd = synth_shufflenet_state_dict(seed=7, model_size="0.5x")
    prog = ShuffleNetV2Program(sd, shufflenet_spec({"MODEL_SIZE": "0.5x"}), 64, 64, "f32")
    assert len(prog._ops) == 62 and all(op["relu"] in (0, 1) for op in prog._ops)
    assert all(op["res"] is None for op in prog._ops if op["kind"] == _lib.UDP_OP_CONV)
