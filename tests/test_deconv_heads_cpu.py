"""pose_shufflenetv2_10x and pose_shufflenetv2_plus (the deconv-head ShuffleNets) on the host side, no GPU: the
restatements against the fixtures the reference's own modules produced, the weight-file contract, the op programs
(the pixel-shuffle siblings' backbone, op for op, with the deconv head behind ``conv_last``) and the refusals."""
import os

import numpy as np
import pytest
import torch

import deconv_heads_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict, synth_shufflenet_state_dict
from udp_pose_amd.synth_shufflenet_plus import synth_shufflenet_plus_deconv_state_dict, synth_shufflenet_plus_state_dict

HEAD = {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4],
        "FINAL_CONV_KERNEL": 1}
PS_HEAD = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "FINAL_CONV_KERNEL": 1}
# name -> (MODEL_SIZE, generator, fixture, conv_last channels, pixel-shuffle sibling, its generator); FIXTURE_SEED: the tool's
NETS = {"pose_shufflenetv2_10x": ("1.0x", synth_shufflenet_deconv_state_dict, "shufflenetv2_10x_deconv.npz", 1024,
                                  "pose_shufflenetv2_10x_pixel_shuffle", synth_shufflenet_state_dict),
        "pose_shufflenetv2_plus": ("Small", synth_shufflenet_plus_deconv_state_dict, "shufflenetv2_plus_small_deconv.npz", 1280,
                                   "pose_shufflenetv2_plus_pixel_shuffle", synth_shufflenet_plus_state_dict)}
NAMES = sorted(NETS)
FIXTURE_SEED = {"pose_shufflenetv2_10x": 8, "pose_shufflenetv2_plus": 7}


def _cfg(name, head=HEAD, **extra):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256],
                      "EXTRA": dict(head, MODEL_SIZE=NETS[name][0] if name in NETS else extra.pop("size"), **extra)}}


@pytest.mark.parametrize("name", NAMES)
def test_keys_and_restatement_equal_the_reference_fixture(golden_dir, name):
    size, synth_sd, fixture, clast, _, _ = NETS[name]
    g = np.load(os.path.join(golden_dir, fixture))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_sd(seed=FIXTURE_SEED[name], calib=calib, final_scale=float(g["final_scale"]))
    # the weight-file contract: the reference module's keys and shapes, in its registration order
    assert ["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()] == list(g["keys"])
    net = MODELS[name](_cfg(name), is_train=False)
    assert ["%s:%s" % (k, "x".join(map(str, v))) for k, v in net.param_shapes().items()] == list(g["keys"])
    assert [k for k in sd if k.startswith("deconv_layers") and k.endswith(".weight")] == ["deconv_layers.%d.weight" % i for i in (0, 1, 3, 4, 6, 7)]
    assert tuple(sd["deconv_layers.0.weight"].shape) == (clast, 256, 4, 4) and tuple(sd["final_layer.weight"].shape) == (17, 256, 1, 1)
    hm = R.FORWARD[name](sd, torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))).numpy()
    assert hm.shape == g["heatmaps"].shape == (1, 17, 64, 48)
    assert float(np.abs(hm - g["heatmaps"]).max()) <= 1e-5
    assert os.path.getsize(os.path.join(golden_dir, fixture)) <= os.path.getsize(os.path.join(golden_dir, "shufflenetv2_plus_small_ps.npz"))


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("name", NAMES)
def test_program_is_the_siblings_backbone_plus_the_deconv_head(name, dtype):
    size, synth_sd, _, clast, sib, sib_sd = NETS[name]
    sd = synth_sd(seed=7)
    net = MODELS[name](_cfg(name), is_train=False, dtype=dtype).load_state_dict(sd)
    prog = net._make_program(256, 192)
    ops = prog._ops
    # the same seed draws the same backbone (the tables share their backbone rows): the sibling's ops up to conv_last
    sdp = sib_sd(seed=7)
    assert all(torch.equal(sd[k], sdp[k]) for k in sd if k.startswith("backbone."))
    sib_ops = MODELS[sib]({"MODEL": dict(_cfg(name)["MODEL"], NAME=sib, EXTRA=dict(PS_HEAD, MODEL_SIZE=size))}, is_train=False,
                          dtype=dtype).load_state_dict(sdp)._make_program(256, 192)._ops
    nb = len(sib_ops) - 8                                                       # conv_compress 1 + DUC 6 + head 1
    fields = ("kind", "name", "ks", "stride", "relu", "cin", "cout", "cout_pad", "hout", "wout", "in_coff", "in_pitch", "out_coff",
              "out_pitch", "chain_cout", "wfmt")
    assert [[op[f] for f in fields] for op in ops[:nb]] == [[op[f] for f in fields] for op in sib_ops[:nb]]
    assert ops[nb - 1]["name"] == "backbone.conv_last.0" and ops[nb - 1]["cout"] == clast
    head = ops[nb:]
    assert [op["kind"] for op in head] == [_lib.UDP_OP_DECONV] * 3 + [_lib.UDP_OP_CONV] and len(ops) == nb + 4
    assert [(op["name"], op["cin"], op["cout"], op["hout"], op["wout"], op["relu"]) for op in head[:3]] == \
        [("deconv_layers.0", clast, 256, 16, 12, 1), ("deconv_layers.3", 256, 256, 32, 24, 1), ("deconv_layers.6", 256, 256, 64, 48, 1)]
    assert head[3]["name"] == "final_layer" and head[3]["out"] is None and head[3]["cout"] == 17 == prog.out_channels
    assert (head[3]["hout"], head[3]["wout"]) == (64, 48)
    assert prog.consumed_keys == set(sd)
    head_macs = 4 * clast * 256 * 16 * 12 + 4 * 256 * 256 * (32 * 24 + 64 * 48) + 256 * 17 * 64 * 48
    sib_prog = MODELS[sib]({"MODEL": dict(_cfg(name)["MODEL"], NAME=sib, EXTRA=dict(PS_HEAD, MODEL_SIZE=size))}, is_train=False,
                           dtype=dtype).load_state_dict(sdp)._make_program(256, 192)
    sib_head = clast * 256 * 8 * 6 + 9 * (256 * 512 * 8 * 6 + 128 * 256 * 16 * 12 + 64 * 128 * 32 * 24) + 32 * 17 * 64 * 48
    assert prog.macs_per_image() - head_macs == sib_prog.macs_per_image() - sib_head


def test_model_classes_and_keys():
    from udp_pose_amd.model import PoseShuffleNetV2DeconvHip, PoseShuffleNetV2PlusDeconvHip
    for name, cls in (("pose_shufflenetv2_10x", PoseShuffleNetV2DeconvHip), ("pose_shufflenetv2_plus", PoseShuffleNetV2PlusDeconvHip)):
        net = MODELS[name](_cfg(name), is_train=False)                          # KeyError before these nets existed
        assert type(net) is cls and net.NAME == name and net.DTYPES == ("f32", "f16x2")
        sd = NETS[name][1](seed=7)
        net.load_state_dict({"module." + k: v for k, v in sd.items()})
        bad = dict(sd)
        del bad["deconv_layers.3.weight"]
        with pytest.raises(RuntimeError, match=r"missing \['deconv_layers.3.weight'\]"):
            net.load_state_dict(bad)
        with pytest.raises(RuntimeError, match=r"unexpected \['decoder.conv_compress.weight'\]"):
            net.load_state_dict(dict(sd, **{"decoder.conv_compress.weight": torch.zeros(1)}))
        with pytest.raises(NotImplementedError):
            net.init_weights()
        with pytest.raises(NotImplementedError):
            net.train()
        # DECONV_WITH_BIAS adds the three deconv biases to the contract
        nb = MODELS[name](_cfg(name, DECONV_WITH_BIAS=True), is_train=False)
        assert [k for k in nb.param_shapes() if k not in net.param_shapes()] == ["deconv_layers.%d.bias" % i for i in (0, 3, 6)]


def test_refusals():
    def make(name, dtype="f32", **extra):
        cfg = _cfg(name)
        cfg["MODEL"]["EXTRA"].update(extra)
        return MODELS[name](cfg, is_train=False, dtype=dtype)
    with pytest.raises(NotImplementedError, match="MODEL_SIZE='2.0x'.*2048"):
        make("pose_shufflenetv2_10x", MODEL_SIZE="2.0x")
    with pytest.raises(NotImplementedError, match="MODEL_SIZE='3.0x'"):
        make("pose_shufflenetv2_10x", MODEL_SIZE="3.0x")
    with pytest.raises(NotImplementedError, match="MODEL_SIZE='Tiny'"):
        make("pose_shufflenetv2_plus", MODEL_SIZE="Tiny")
    for name in NAMES:
        with pytest.raises(ValueError, match="f32, f16x2"):
            make(name, dtype="bf16")
        with pytest.raises(NotImplementedError, match=name + ": NUM_DECONV_LAYERS=2"):
            make(name, NUM_DECONV_LAYERS=2, NUM_DECONV_FILTERS=[256, 256], NUM_DECONV_KERNELS=[4, 4])
        with pytest.raises(NotImplementedError, match=name + ": NUM_DECONV_KERNELS"):
            make(name, NUM_DECONV_KERNELS=[4, 2, 4])
        with pytest.raises(NotImplementedError, match=name + ": FINAL_CONV_KERNEL=5"):
            make(name, FINAL_CONV_KERNEL=5)


def test_pose_resnet_refusals_keep_their_wording():
    from udp_pose_amd.resnet_plan import pose_resnet_spec
    with pytest.raises(NotImplementedError, match="pose_resnet: NUM_DECONV_KERNELS"):
        pose_resnet_spec({"NUM_LAYERS": 50, "NUM_DECONV_KERNELS": [4, 3, 4]})
