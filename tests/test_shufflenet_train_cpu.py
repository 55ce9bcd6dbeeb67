"""ShuffleNetV2 training on the host side, no GPU: the train-mode restatement against one step of the reference's own
module (tests/golden/shufflenet_train_step.npz) and against the inference restatement, the trainable model
``MODELS[...](cfg, is_train=True)`` returns (init_weights, the pretrained-file rules, the refusals), the new exports, the
depthwise weight-gradient split against a hand computation, the padded parameter layout, and the inference programs
(unchanged)."""
import contextlib
import ctypes as C
import hashlib
import io
import os
import runpy

import numpy as np
import pytest
import torch

import shufflenet_ref as R
import shufflenet_train_ref as T
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_shufflenet import (shufflenet_deconv_param_shapes, shufflenet_param_shapes,
                                           synth_shufflenet_deconv_state_dict, synth_shufflenet_state_dict)

PS, DC = "pose_shufflenetv2_10x_pixel_shuffle", "pose_shufflenetv2_10x"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS_EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "1.0x", "FINAL_CONV_KERNEL": 1}
DC_EXTRA = {"MODEL_SIZE": "1.0x", "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
            "NUM_DECONV_KERNELS": [4, 4, 4], "FINAL_CONV_KERNEL": 1}
UDP_ERR_ARG, UDP_ERR_UNSUPPORTED, UDP_ERR_WORKSPACE = -1, -3, -4


def _cfg(name=PS, **extra):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256], "INIT_WEIGHTS": False,
                      "EXTRA": dict(PS_EXTRA if name == PS else DC_EXTRA, **extra)}}


# ------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def step(golden_dir):
    g = np.load(os.path.join(golden_dir, "shufflenet_train_step.npz"))
    sd = synth_shufflenet_state_dict(seed=int(g["seed"]), num_joints=5)
    batch = tuple(torch.from_numpy(g[k]) for k in ("x", "target", "target_weight"))
    return g, sd, T.loss_and_grads(sd, *batch, torch.float64)


def test_restatement_reproduces_the_reference_modules_step(step):
    g, sd, (loss, y, grads, sd_after) = step
    keys = [str(k) for k in g["keys"]]
    assert keys == [k for k in sd if T.is_param(k)] == list(grads)
    assert abs(loss - float(g["loss"])) <= 1e-9 * float(g["loss"])
    np.testing.assert_allclose(y.numpy(), g["heatmaps"], rtol=0, atol=1e-9 * float(np.abs(g["heatmaps"]).max()))
    zero = set(str(k) for k in g["zero_keys"])
    gscale = float(g["gmax"].max())
    n_full = n_sampled = 0
    for i, k in enumerate(keys):
        ours = grads[k].numpy().reshape(-1)
        mx = float(g["gmax"][i])
        if k in zero:                     # zero in exact arithmetic: rounding noise without a scale of its own
            assert mx <= 1e-12 * gscale and float(np.abs(ours).max()) <= 1e-12 * gscale, k
            continue
        assert abs(float(np.abs(ours).max()) - mx) <= 1e-9 * mx and abs(float(ours.sum()) - float(g["gsum"][i])) <= 1e-9 * mx * ours.size, k
        if ("g_%d" % i) in g.files:
            want, got = g["g_%d" % i].reshape(-1), ours
            n_full += 1
        else:
            want, got = g["s_%d" % i], ours[g["p_%d" % i]]
            n_sampled += 1
        assert float(np.abs(got - want).max()) <= 1e-9 * mx, k
    assert n_full > 100 and n_sampled > 20 and 0 < len(zero) < 30
    # every depthwise and BatchNorm parameter, first_conv and final_layer are there in full
    for i, k in enumerate(keys):
        if ".branch_main.3." in k or ".branch_proj.0." in k or grads[k].dim() == 1 or k.startswith(("backbone.first_conv", "final_layer")):
            assert ("g_%d" % i) in g.files, k
    for bn in g["stat_bns"]:
        for s in (".running_mean", ".running_var"):
            want = g["stat_%s%s" % (bn, s)]
            np.testing.assert_allclose(sd_after[str(bn) + s].numpy(), want, rtol=1e-9, atol=1e-9 * float(np.abs(want).max()))
    assert float((sd_after["decoder.duc.2.bn.running_mean"] - sd["decoder.duc.2.bn.running_mean"]).abs().max()) > 0


def test_fixture_fp32_yardstick_is_sane(step):
    g = step[0]
    zero = set(str(k) for k in g["zero_keys"])
    for i, k in enumerate(g["keys"]):
        if str(k) not in zero:
            assert g["e32"][i] <= 1e-3 * g["gmax"][i], k


@pytest.mark.parametrize("deconv", [False, True])
def test_eval_mode_restatement_is_the_inference_restatement(deconv):
    """With training=False the graph is the one tests/shufflenet_ref.py (and through it the inference fixture) pins."""
    if deconv:
        import deconv_heads_ref as D
        sd = synth_shufflenet_deconv_state_dict(seed=5, model_size="0.5x", num_joints=5, deconv_filters=(32, 32, 32))
        want = D.FORWARD[DC](sd, torch.from_numpy(synth.synth_crops(2, 64, 64, seed=3)))
    else:
        sd = synth_shufflenet_state_dict(seed=5, model_size="1.5x", num_joints=5)
        want = R.forward(sd, torch.from_numpy(synth.synth_crops(2, 64, 64, seed=3)))
    before = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        got = T.forward(sd, torch.from_numpy(synth.synth_crops(2, 64, 64, seed=3)), training=False)
    assert torch.equal(got, want)
    assert all(torch.equal(before[k], sd[k]) for k in sd)                     # eval mode moves no statistic


# ------------------------------------------------------------------ the model surface
@pytest.mark.parametrize("name", [PS, DC])
def test_init_weights_statistics(name):
    torch.manual_seed(3)
    net = MODELS[name](_cfg(name), is_train=True)
    assert net.trainable and net._sd is None                                  # INIT_WEIGHTS False: load_state_dict
    assert net.init_weights() is net
    sd, shapes = net.state_dict(), net.param_shapes()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    first = sd["backbone.first_conv.0.weight"]
    assert abs(float(first.std()) - 0.01) <= 0.2 * 0.01
    for k, cin in (("backbone.features.5.branch_main.0.weight", 116), ("backbone.conv_last.0.weight", 464),
                   ("backbone.features.4.branch_proj.2.weight", 116)):
        assert shapes[k][1] == cin and abs(float(sd[k].std()) - 1.0 / cin) <= 0.1 / cin, k
    assert abs(float(sd["backbone.features.3.branch_main.3.weight"].std()) - 1.0) <= 0.1          # depthwise: 1 / cin_per_group = 1
    for k in shapes:
        if k.startswith("backbone.") and k.endswith(".bias"):
            assert float((sd[k] - 1e-4).abs().max()) == 0.0, k
        if k.startswith("backbone.") and len(shapes[k]) == 1 and k.endswith(".weight"):
            assert float((sd[k] - 1).abs().max()) == 0.0, k
        if k.endswith("running_mean"):
            assert float(sd[k].abs().max()) == 0.0, k
        if k.endswith("running_var"):
            assert float((sd[k] - 1).abs().max()) == 0.0, k
    # the head keeps torch's defaults: U(+-1/sqrt(fan_in)) for a conv, BatchNorm 1 / 0
    hk = "decoder.duc.0.conv.weight" if name == PS else "deconv_layers.3.weight"
    fan = shapes[hk][1] * shapes[hk][2] * shapes[hk][3]
    assert float(sd[hk].abs().max()) <= fan ** -0.5 and abs(float(sd[hk].std()) - (3 * fan) ** -0.5) <= 0.05 * (3 * fan) ** -0.5
    hb = "decoder.duc.0.bn" if name == PS else "deconv_layers.4"
    assert float((sd[hb + ".weight"] - 1).abs().max()) == 0.0 and float(sd[hb + ".bias"].abs().max()) == 0.0
    assert 0 < float(sd["final_layer.bias"].abs().max()) <= shapes["final_layer.weight"][1] ** -0.5


def test_init_weights_with_a_pretrained_file(tmp_path):
    """load_checkpoint (shufflenetv2.py:6-31): checkpoint["state_dict"], ``module.`` stripped, the backbone's own keys,
    a tensor of another size keeps the initialised value."""
    net = MODELS[PS](_cfg(), is_train=True)
    shapes = net.param_shapes()
    ck = {"module.first_conv.0.weight": torch.full(shapes["backbone.first_conv.0.weight"], 0.5),
          "module.features.2.branch_main.4.running_var": torch.full((58,), 0.25),
          "features.0.branch_main.3.weight": torch.full((58, 1, 3, 3), 2.0),
          "module.conv_last.0.weight": torch.zeros(1024, 400, 1, 1),                       # another size: not taken, no error
          "module.fc.weight": torch.zeros(3, 3)}                                            # not a key of the net
    path = str(tmp_path / "shufflenetv2.pth.tar")
    torch.save({"state_dict": ck, "epoch": 3}, path)
    torch.manual_seed(4)
    sd = net.init_weights(path).state_dict()
    assert float((sd["backbone.first_conv.0.weight"] - 0.5).abs().max()) == 0.0
    assert float((sd["backbone.features.2.branch_main.4.running_var"] - 0.25).abs().max()) == 0.0
    assert float((sd["backbone.features.0.branch_main.3.weight"] - 2.0).abs().max()) == 0.0
    assert tuple(sd["backbone.conv_last.0.weight"].shape) == (1024, 464, 1, 1) and float(sd["backbone.conv_last.0.weight"].std()) > 0
    assert "backbone.fc.weight" not in sd and "fc.weight" not in sd and list(sd) == list(shapes)
    assert abs(float(sd["backbone.features.1.branch_main.0.weight"].std()) - 1.0 / 58) <= 0.1 / 58     # untouched: the init


@pytest.mark.parametrize("name", [PS, DC])
def test_init_weights_under_is_train_follows_the_config(name):
    cfg = _cfg(name)
    cfg["MODEL"]["INIT_WEIGHTS"] = True
    cfg["MODEL"]["PRETRAINED"] = ""
    assert MODELS[name](cfg, is_train=True)._sd is not None
    assert MODELS[name](cfg, is_train=False)._sd is None
    assert MODELS[name](_cfg(name), is_train=True)._sd is None


def test_refusals():
    from udp_pose_amd.shufflenet_plan import shufflenet_deconv_spec, shufflenet_spec
    from udp_pose_amd.train import ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer
    with pytest.raises(ValueError, match="bf16"):
        MODELS[PS](_cfg(), is_train=True, dtype="bf16")
    with pytest.raises(ValueError, match="fp32 only.*bf16|bf16.*fp32 only"):
        ShuffleNetV2Trainer(shufflenet_spec(PS_EXTRA), 17, "gaussian", {}, device="cpu", dtype="bf16")
    with pytest.raises(ValueError, match="fp32 only"):
        ShuffleNetV2DeconvTrainer(shufflenet_deconv_spec(DC_EXTRA), 17, "gaussian", {}, device="cpu", dtype="bf16")
    with pytest.raises(ValueError, match="ARCHITECTURE.*multiple of 64"):
        ShuffleNetV2Trainer(dict(shufflenet_spec(PS_EXTRA), architecture=(512, 256, 96)), 17, "gaussian", {}, device="cpu")
    for name in (PS, DC):                                                     # is_train=False still refuses
        net = MODELS[name](_cfg(name), is_train=False)
        for refused in (net.trainer, net.train, net.init_weights):
            with pytest.raises(NotImplementedError):
                refused()
    plus = {"MODEL": {"NAME": "pose_shufflenetv2_plus_pixel_shuffle", "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian",
                      "IMAGE_SIZE": [192, 256], "INIT_WEIGHTS": False,
                      "EXTRA": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "Small", "FINAL_CONV_KERNEL": 1}}}
    for name, extra in (("pose_shufflenetv2_plus_pixel_shuffle", plus["MODEL"]["EXTRA"]), ("pose_shufflenetv2_plus", dict(DC_EXTRA, MODEL_SIZE="Small"))):
        net = MODELS[name](dict(plus, MODEL=dict(plus["MODEL"], NAME=name, EXTRA=extra)), is_train=True)
        for refused in (net.trainer, net.train, net.init_weights):
            with pytest.raises(NotImplementedError):
                refused()


# ------------------------------------------------------------------ the library
EXPORTS = ("udp_dwconvk_train_fwd", "udp_dwconvk_dgrad", "udp_dwconvk_wgrad", "udp_dwconvk_wgrad_workspace_bytes",
           "udp_debug_dw_wgrad_plan", "udp_pixshuf2_train_fwd", "udp_pixshuf2_train_bwd", "udp_shuffle_pair_fwd",
           "udp_shuffle_pair_bwd", "udp_chan_cat2", "udp_chan_uncat2")


def test_exports_and_abi_version():
    L = _lib.lib()
    assert L.udp_abi_version() == 20
    for name in EXPORTS:
        assert getattr(L, name) is not None, name
    with open(os.path.join(ROOT, "include", "udp_pose_hip.h")) as f:
        header = f.read()
    assert all((" %s(" % name) in header for name in EXPORTS) and "#define UDP_POSE_ABI_VERSION 20" in header


def _plan(n, hout, wout, c, ws=None):
    L = _lib.lib()
    out = (C.c_int * 4)()
    if ws is None:
        ws = int(L.udp_dwconvk_wgrad_workspace_bytes(n, hout, wout, c, 3))
    return L.udp_debug_dw_wgrad_plan(n, hout, wout, c, 3, ws, out), list(out), ws


def test_dw_wgrad_plan_against_a_hand_computation():
    """partials = min(n*hout, 256, workspace / (36 c)); rows = ceil(n*hout / partials); partials = ceil(n*hout / rows);
    workgroups = partials x ceil(c/4 / channel lanes), channel lanes = the power of two in 8..64 that covers c/4."""
    lds = 256 * 3 * 16                                                                    # the lanes' 3 taps of one kernel row x 4 channels
    # the largest case of a 256x192 batch-32 step: 116 (128) channels, 32x24 outputs: 1024 rows -> 256 runs of 4, 32 lanes cover 32 groups
    assert _plan(32, 32, 24, 128) == (0, [4, 256, 256, lds], 256 * 9 * 128 * 4)
    # the smallest maps: 2x2 outputs of 2 images at 464 channels: 4 rows -> 4 runs of 1; 116 groups need two blocks of 64 lanes
    assert _plan(2, 2, 2, 464) == (0, [1, 8, 4, lds], 4 * 9 * 464 * 4)
    # 3 images of 7 rows, 96 channels: 21 rows -> 21 runs of 1; 24 groups in one block of 32 lanes
    assert _plan(3, 7, 9, 96) == (0, [1, 21, 21, lds], 21 * 9 * 96 * 4)
    # a workspace of 5 partials limits the split: ceil(21 / 5) = 5 rows -> ceil(21 / 5) = 5 runs, the last of 1 row
    assert _plan(3, 7, 9, 96, ws=5 * 9 * 96 * 4 + 100)[:2] == (0, [5, 5, 5, lds])
    assert _plan(3, 7, 9, 96, ws=4 * 9 * 96 * 4)[:2] == (0, [6, 4, 4, lds])               # 4 fit: 6 rows -> 4 runs (6, 6, 6, 3)
    assert _plan(1, 1, 1, 4)[:2] == (0, [1, 1, 1, lds])
    # the bound over all shapes
    assert int(_lib.lib().udp_dwconvk_wgrad_workspace_bytes(256, 1, 1, 240, 3)) == 256 * 9 * 240 * 4
    assert int(_lib.lib().udp_dwconvk_wgrad_workspace_bytes(999, 64, 48, 240, 3)) == 256 * 9 * 240 * 4


def test_dw_wgrad_plan_refuses_what_the_launch_refuses():
    L = _lib.lib()
    assert _plan(3, 7, 9, 96, ws=9 * 96 * 4 - 1)[0] == UDP_ERR_WORKSPACE and "workspace" in L.udp_last_error().decode()
    assert _plan(3, 7, 9, 98, ws=1 << 20)[0] == UDP_ERR_ARG                               # C % 4
    assert _plan(0, 7, 9, 96, ws=1 << 20)[0] == UDP_ERR_ARG
    assert L.udp_debug_dw_wgrad_plan(3, 7, 9, 96, 3, 1 << 20, None) == UDP_ERR_ARG
    assert int(L.udp_dwconvk_wgrad_workspace_bytes(3, 7, 9, 98, 3)) == 0
    # the launch itself, on the host: every refusal comes before anything touches the device
    one = C.c_void_p(16)
    for args, code in (((one, one, 3, 7, 9, 96, 88, 3, 1, _lib.UDP_F32, one, one, 9 * 96 * 4 - 1, None), UDP_ERR_WORKSPACE),
                       ((one, one, 3, 7, 9, 96, 88, 3, 3, _lib.UDP_F32, one, one, 1 << 20, None), UDP_ERR_UNSUPPORTED),
                       ((one, one, 3, 7, 9, 96, 88, 3, 1, _lib.UDP_BF16, one, one, 1 << 20, None), UDP_ERR_UNSUPPORTED),
                       ((one, one, 3, 7, 9, 98, 88, 3, 1, _lib.UDP_F32, one, one, 1 << 20, None), UDP_ERR_ARG),
                       ((one, one, 3, 7, 9, 96, 97, 3, 1, _lib.UDP_F32, one, one, 1 << 20, None), UDP_ERR_ARG),
                       ((None, one, 3, 7, 9, 96, 88, 3, 1, _lib.UDP_F32, one, one, 1 << 20, None), UDP_ERR_ARG)):
        assert L.udp_dwconvk_wgrad(*args) == code and L.udp_last_error(), args


# ------------------------------------------------------------------ the parameter layout
@pytest.mark.parametrize("deconv", [False, True])
def test_trainer_layout_pads_one_dimensional_keys_to_16(deconv):
    from udp_pose_amd.shufflenet_plan import shufflenet_deconv_spec, shufflenet_spec
    from udp_pose_amd.train import ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer, Trainer
    if deconv:
        shapes = shufflenet_deconv_param_shapes(num_joints=5, deconv_with_bias=True)
        sd = synth_shufflenet_deconv_state_dict(seed=2, num_joints=5, deconv_with_bias=True)
        tr = ShuffleNetV2DeconvTrainer(shufflenet_deconv_spec(dict(DC_EXTRA, DECONV_WITH_BIAS=True)), 5, "gaussian", sd, device="cpu")
        assert "deconv_layers.3" in tr._transposed and "deconv_layers.3.bias" in tr._keys
    else:
        shapes = shufflenet_param_shapes(num_joints=5)
        sd = synth_shufflenet_state_dict(seed=2, num_joints=5)
        tr = ShuffleNetV2Trainer(shufflenet_spec(PS_EXTRA), 5, "gaussian", sd, device="cpu")
    assert issubclass(ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer) and issubclass(ShuffleNetV2Trainer, Trainer)
    assert tr._keys == [k for k in shapes if T.is_param(k)]
    n = 0
    for k in tr._keys + tr._stat_keys:
        numel = int(np.prod(shapes[k]))
        assert tr._off[k] == n, k
        n += (numel + 15) // 16 * 16 if len(shapes[k]) == 1 else (numel + 3) // 4 * 4
        assert tuple(tr.param(k).shape) == tuple(shapes[k]) and torch.equal(tr.param(k), sd[k].float())
        if k in tr._keys:
            assert tuple(tr.grad_of(k).shape) == tuple(shapes[k])
    assert tr.flat.numel() == n
    # the slack of every key is zero (the BatchNorm kernels read gamma / beta / statistics over the stored channels)
    mask = torch.ones(n, dtype=torch.bool)
    for k in tr._keys + tr._stat_keys:
        mask[tr._off[k]:tr._off[k] + int(np.prod(shapes[k]))] = False
    assert int(mask.sum()) > 0 and float(tr.flat[mask].abs().max()) == 0.0
    out = tr.state_dict()
    assert list(out) == list(shapes) and all(tuple(out[k].shape) == tuple(shapes[k]) for k in shapes)
    assert all(torch.equal(out[k], sd[k]) for k in shapes if not k.endswith("num_batches_tracked"))
    assert sum(cnt for _, _, cnt in tr._buckets) == len(tr._keys) and tr._buckets[-1][1] == tr._n_param
    # the depthwise weights are read in place; every other conv is packed
    assert "backbone.features.0.branch_main.3" not in tr._convs and "backbone.features.0.branch_proj.0" not in tr._convs
    assert tr._convs["backbone.first_conv.0"][4] is None and tr._convs["backbone.features.0.branch_main.0"][4] is not None
    assert len(tr._convs) == sum(1 for k in tr._keys if len(shapes[k]) == 4) - 16 - 3       # 16 + 3 depthwise convs


def test_other_trainers_keep_their_layout():
    """HRNet and pose_resnet: consecutive keys, each rounded up to 4 floats, as before the stride hook existed."""
    from udp_pose_amd.synth_resnet import pose_resnet_param_shapes, synth_pose_resnet_state_dict
    from udp_pose_amd.train import HRNetTrainer, PoseResNetTrainer, Trainer
    kw = dict(layers=(1, 1, 1, 1), num_joints=5, deconv_filters=(32, 32, 32))
    spec = dict(layers=(1, 1, 1, 1), deconv_filters=(32, 32, 32), final_kernel=1, deconv_with_bias=False)
    cfg = {"MODEL": {"EXTRA": synth.W32_EXTRA, "NUM_JOINTS": 5, "TARGET_TYPE": "gaussian"}}
    trs = [(PoseResNetTrainer(spec, 5, "gaussian", synth_pose_resnet_state_dict(seed=1, **kw), device="cpu"),
            pose_resnet_param_shapes(**dict(kw, deconv_kernel=4, final_kernel=1, deconv_with_bias=False))),
           (HRNetTrainer(cfg, synth.synth_state_dict(synth.W32_EXTRA, 5, "gaussian", seed=1), device="cpu"),
            synth.hrnet_param_shapes(synth.W32_EXTRA, 5, "gaussian"))]
    for tr, shapes in trs:
        n = 0
        for k in tr._keys + tr._stat_keys:
            assert tr._off[k] == n, k
            n += (int(np.prod(shapes[k])) + 3) // 4 * 4
        assert tr.flat.numel() == n and tr.bn_over_stored is False
    for name in ("_maxpool", "_deconv", "_key_stride"):
        assert name in vars(Trainer) and name not in vars(PoseResNetTrainer) and name not in vars(HRNetTrainer), name


# ------------------------------------------------------------------ the inference side did not move
def test_program_digests_unchanged(golden_dir):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "tools", "program_digest.py"), run_name="__main__")
    with open(os.path.join(golden_dir, "program_digest_66.txt")) as f:
        assert buf.getvalue() == f.read()
    # and the ShuffleNetV2 program itself (0.5x, 64x64, fp32; recorded on the commit before the trainer existed)
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    prog = ShuffleNetV2Program(synth_shufflenet_state_dict(seed=7, model_size="0.5x"), shufflenet_spec({"MODEL_SIZE": "0.5x"}), 64, 64, "f32")
    h = hashlib.sha256()
    h.update(bytes(prog.ops_array()))
    h.update(prog.weight_blob().tobytes())
    assert h.hexdigest() == "a77fa4444c4c66e452b0681675ac5af8b1b11ac3c600bd413be2d3a4bc9930ef"
