"""pose_resnet_psa (ResNet-18 / 34 with polarized self-attention) on the host side, no GPU: the model factory and its
refusals, the op program the planner emits (launch census, PSA geometry, every state_dict key consumed), the Bottleneck
depths (the programs of pose_resnet, byte for byte) and the plain-torch restatement (tests/resnet_psa_ref.py) against
the heat-maps the reference's own module produced (tests/golden/resnet18_psa.npz, tools/gen_golden_resnet_psa.py)."""
import os

import numpy as np
import pytest
import torch

import resnet_psa_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS, PoseResNetPsaHip
from udp_pose_amd.resnet_plan import PoseResNetProgram, PoseResNetPsaProgram, pose_resnet_psa_spec, pose_resnet_spec
from udp_pose_amd.synth_resnet import (pose_resnet_psa_param_shapes, synth_pose_resnet_psa_state_dict,
                                       synth_pose_resnet_state_dict)

EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
         "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 18}
LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
PSA_KINDS = [_lib.UDP_OP_PSA_POOL, _lib.UDP_OP_PSA_MLP, _lib.UDP_OP_PSA_SCALE, _lib.UDP_OP_CONV, _lib.UDP_OP_PSA_SP]


def _cfg(name="pose_resnet_psa", **extra):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256],
                      "EXTRA": dict(EXTRA, **extra)}}


# ------------------------------------------------------------------ registry and loading
def test_models_has_pose_resnet_psa():
    net = MODELS["pose_resnet_psa"](_cfg(), is_train=False)
    assert isinstance(net, PoseResNetPsaHip) and net.NAME == "pose_resnet_psa" and net.DTYPES == ("f32", "f16x2")
    sd = synth_pose_resnet_psa_state_dict(seed=7)
    assert len(sd) == 220 and sum(v.numel() for v in sd.values()) == 16567480        # the reference module's census
    assert tuple(sd["layer4.0.deattn.conv_v_right.weight"].shape) == (256, 512, 1, 1)
    assert tuple(sd["layer1.0.deattn.conv_up.0.weight"].shape) == (8, 32, 1, 1)
    assert tuple(sd["layer4.1.deattn.conv_up.1.weight"].shape) == (64, 1, 1)
    assert tuple(sd["deconv_layers.0.weight"].shape) == (512, 256, 4, 4)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})            # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["layer3.1.deattn.conv_q_left.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    bad = dict(sd)
    bad["layer4.0.deattn.conv_v_right.weight"] = torch.zeros(256, 256, 1, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        net.trainer()
    with pytest.raises(NotImplementedError):
        net.init_weights()


def test_resnet34_psa_key_census():
    shapes = pose_resnet_psa_param_shapes(layers=LAYERS[34])
    assert len(shapes) == 396 and sum(int(np.prod(s)) for s in shapes.values()) == 27634432
    assert "layer1.0.downsample.0.weight" not in shapes and shapes["layer2.0.downsample.0.weight"] == (128, 64, 1, 1)


def test_refused_configurations():
    with pytest.raises(ValueError, match="f32, f16x2"):
        MODELS["pose_resnet_psa"](_cfg(), is_train=False, dtype="bf16")
    for extra, what in [({"NUM_DECONV_KERNELS": [3, 3, 3]}, "NUM_DECONV_KERNELS"),
                        ({"NUM_DECONV_KERNELS": [2, 2, 2]}, "NUM_DECONV_KERNELS"),
                        ({"NUM_DECONV_LAYERS": 2, "NUM_DECONV_FILTERS": [256, 256], "NUM_DECONV_KERNELS": [4, 4]}, "NUM_DECONV_LAYERS"),
                        ({"FINAL_CONV_KERNEL": 5}, "FINAL_CONV_KERNEL"), ({"NUM_LAYERS": 20}, "NUM_LAYERS=20")]:
        for layers in ({}, {"NUM_LAYERS": 50}):
            with pytest.raises(NotImplementedError, match=what):
                MODELS["pose_resnet_psa"](_cfg(**dict(layers, **extra)), is_train=False)
    for layers in (18, 34):                                                  # pose_resnet itself keeps refusing them
        with pytest.raises(NotImplementedError, match="NUM_LAYERS=%d" % layers):
            MODELS["pose_resnet"](_cfg("pose_resnet", NUM_LAYERS=layers), is_train=False)
        with pytest.raises(NotImplementedError):
            pose_resnet_spec(dict(EXTRA, NUM_LAYERS=layers))


def test_planner_refuses_other_psa_widths():
    """Program._psa: a width that divides 256 (a multiple of 16), or 512."""
    prog = PoseResNetPsaProgram.__new__(PoseResNetPsaProgram)
    from udp_pose_amd.program import _T
    for c in (48, 384, 1024, 8):
        with pytest.raises(ValueError, match="divides 256"):
            prog.sd = {}
            prog._psa(_T(0, c, 4, 4), "blk.deattn")


# ------------------------------------------------------------------ program census
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(256, 192), (384, 288)])
@pytest.mark.parametrize("num_layers", [18, 34])
def test_program_census(num_layers, hw, dtype):
    layers = LAYERS[num_layers]
    sd = synth_pose_resnet_psa_state_dict(seed=3, layers=layers)
    prog = PoseResNetPsaProgram(sd, pose_resnet_psa_spec(dict(EXTRA, NUM_LAYERS=num_layers)), hw[0], hw[1], dtype)
    ops = prog._ops
    H, W = hw
    assert len(ops) == 7 * sum(layers) + 3 + 2 + 3 + 1 == {18: 65, 34: 121}[num_layers]
    kinds = [op["kind"] for op in ops]
    assert kinds[0] == _lib.UDP_OP_STEM7 and kinds[1] == _lib.UDP_OP_MAXPOOL
    assert kinds.count(_lib.UDP_OP_STEM7) == 1 and kinds.count(_lib.UDP_OP_MAXPOOL) == 1 and kinds.count(_lib.UDP_OP_DECONV) == 3
    # every block: conv1 (the stride), the 5 attention ops in order, [downsample], conv2 + shortcut + ReLU
    i = 2
    for li, (planes, nblk) in enumerate(zip((64, 128, 256, 512), layers), start=1):
        h, w = H >> (li + 1), W >> (li + 1)
        for k in range(nblk):
            p = "layer%d.%d" % (li, k)
            stride = 2 if (li > 1 and k == 0) else 1
            c1 = ops[i]
            assert (c1["name"], c1["ks"], c1["stride"], c1["relu"], c1["cout"], c1["hout"], c1["wout"]) == \
                (p + ".conv1", 3, stride, 1, planes, h, w) and c1["res"] is None
            psa = ops[i + 1:i + 6]
            assert [op["kind"] for op in psa] == PSA_KINDS
            assert [op["name"] for op in psa] == [p + ".deattn" + s for s in (".pool", ".mlp", ".scale", ".conv_v_left", ".sp")]
            for op in psa:
                assert (op["hin"], op["win"], op["hout"], op["wout"]) == (h, w, h, w)
            pool, mlp, scale, theta, sp = psa
            assert (pool["cin"], mlp["cin"], scale["cin"], scale["cout"]) == (planes,) * 4
            assert (theta["cin"], theta["cout"], theta["ks"], theta["relu"], theta["inp"]) == (planes, planes // 2, 1, 0, scale["out"])
            assert (sp["cin"], sp["cout"], sp["inp"], sp["res"], sp["ups"]) == (planes // 2, planes, theta["out"], scale["out"], [(mlp["out"], 0)])
            assert pool["inp"] is c1["out"] and mlp["inp"] is pool["out"] and scale["res"] is mlp["out"]
            assert pool["w_off"] == mlp["w_off"] and pool["w_off"] % 256 == 0
            i += 6
            res = c1["inp"]
            if stride == 2:
                ds = ops[i]
                assert (ds["name"], ds["ks"], ds["stride"], ds["relu"], ds["cout"]) == (p + ".downsample.0", 1, 2, 0, planes)
                assert ds["inp"] is c1["inp"]
                res = ds["out"]
                i += 1
            c2 = ops[i]
            assert (c2["name"], c2["ks"], c2["stride"], c2["relu"], c2["cin"], c2["cout"]) == (p + ".conv2", 3, 1, 1, planes, planes)
            assert c2["inp"] is sp["out"] and c2["res"] is res
            i += 1
    dec = ops[i:i + 3]
    assert all(op["kind"] == _lib.UDP_OP_DECONV and op["ks"] == 4 and op["stride"] == 2 and op["relu"]
               and op["wfmt"] == int(dtype == "f16x2") for op in dec)
    assert [op["cin"] for op in dec] == [512, 256, 256]
    assert [(op["hin"], op["hout"]) for op in dec] == [(H // 32, H // 16), (H // 16, H // 8), (H // 8, H // 4)]
    head = ops[-1]
    assert i + 3 == len(ops) - 1 and head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17
    assert (head["hout"], head["wout"]) == (H // 4, W // 4)
    assert prog.consumed_keys == set(pose_resnet_psa_param_shapes(layers=layers)) == set(sd)
    arr = prog.ops_array()
    assert len(arr) == len(ops) and arr[len(arr) - 1].out_buf == _lib.UDP_BUF_OUTPUT
    assert np.isfinite(prog.macs_per_image()) and prog.macs_per_image() > 0


# ------------------------------------------------------------------ Bottleneck depths
def test_bottleneck_depth_is_pose_resnets_program():
    """pose_resnet_psa with NUM_LAYERS 50 is the reference's plain Bottleneck net: the same ops and weight blob."""
    extra = dict(EXTRA, NUM_LAYERS=50)
    spec = pose_resnet_psa_spec(extra)
    assert spec["basic"] is False and {k: v for k, v in spec.items() if k != "basic"} == pose_resnet_spec(extra)
    sd = synth_pose_resnet_state_dict(seed=7)
    net = MODELS["pose_resnet_psa"](_cfg(NUM_LAYERS=50), is_train=False, dtype="f16x2").load_state_dict(sd)
    a = net._make_program(256, 192)
    b = PoseResNetProgram(sd, pose_resnet_spec(extra), 256, 192, "f16x2")
    assert isinstance(a, PoseResNetPsaProgram)
    assert bytes(a.ops_array()) == bytes(b.ops_array())
    assert np.array_equal(a.weight_blob(), b.weight_blob()) and a.buf_elems == b.buf_elems


# ------------------------------------------------------------------ the restatement against the reference's fixture
@pytest.fixture(scope="module")
def fixture18(golden_dir):
    g = np.load(os.path.join(golden_dir, "resnet18_psa.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    return g, synth_pose_resnet_psa_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))


def test_fixture_keys_are_the_synth_contract(fixture18):
    g, sd = fixture18
    assert sorted("%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()) == list(g["keys"])
    assert g["heatmaps"].shape == (1, 17, 64, 48) and 0.2 < float(g["heatmaps"].std()) < 0.4


def test_restatement_fp64_matches_reference_fixture(fixture18):
    """The fixture is the reference module's fp64 forward rounded to fp32 (heat-maps of order 1: half an fp32 ulp is
    1.2e-7): the fp64 restatement within 1e-6 absolute.  Measured 5.9e-8."""
    g, sd = fixture18
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    y = R.forward(sd, x, dtype=torch.float64).numpy()
    err = float(np.abs(y - g["heatmaps"]).max())
    print("fp64 restatement vs fixture", err)
    assert err <= 1e-6


def test_restatement_fp32_matches_reference_fixture(fixture18):
    """The reference module's own fp32 forward is 7.055e-6 from its fp64 forward on this crop (printed by
    tools/gen_golden_resnet_psa.py): the fp32 restatement within 4 x that.  Measured 7.055e-6."""
    g, sd = fixture18
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    y = R.forward(sd, x, dtype=torch.float32).numpy()
    err = float(np.abs(y - g["heatmaps"]).max())
    print("fp32 restatement vs fixture", err)
    assert err <= 4 * 7.055e-6
    np.testing.assert_array_equal(y.reshape(1, 17, -1).argmax(2), g["heatmaps"].reshape(1, 17, -1).argmax(2))
