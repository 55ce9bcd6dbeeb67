"""pose_mobilevitv2_pixel_shuffle training on the host side, no GPU: the new exports and every refusal they make before
touching the device, the GroupNorm split as a pure function of the shape, the trainable model
``MODELS[...](cfg, is_train=True)`` returns (init_weights, the local-file rules, the refusals), the trainer's layout, and
the pins of the train-mode restatement (tests/mobilevitv2_train_ref.py): in eval mode to tests/mobilevitv2_ref.py, in
train mode to one step of the reference's own module (tests/golden/mobilevitv2_train_step.npz)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import mobilevitv2_ref as R
import mobilevitv2_train_ref as T
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict
from udp_pose_amd.train import MobileViTv2Trainer, ShuffleNetV2Trainer, Trainer

NAME = "pose_mobilevitv2_pixel_shuffle"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": 0.5, "FINAL_CONV_KERNEL": 1}
UDP_ERR_ARG, UDP_ERR_UNSUPPORTED, UDP_ERR_WORKSPACE = -1, -3, -4
F32, BF16 = _lib.UDP_F32, _lib.UDP_BF16


def _cfg(init=False, pretrained="", joints=17, **extra):
    return {"MODEL": {"NAME": NAME, "NUM_JOINTS": joints, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256], "INIT_WEIGHTS": init,
                      "PRETRAINED": pretrained, "EXTRA": dict(EXTRA, **extra)}}


# ------------------------------------------------------------------ the library
EXPORTS = ("udp_silu_fwd", "udp_silu_bwd", "udp_gnorm_train_fwd", "udp_gnorm_train_bwd", "udp_gnorm_train_workspace_bytes",
           "udp_gnorm_train_split", "udp_linattn_train_fwd", "udp_linattn_train_bwd")


def test_exports_and_abi_version():
    L = _lib.lib()
    assert L.udp_abi_version() == 20 and _lib.ABI_VERSION == 20
    for name in EXPORTS:
        assert getattr(L, name) is not None and name in _lib.EXPORTS, name
    with open(os.path.join(ROOT, "include", "udp_pose_hip.h")) as f:
        header = f.read()
    assert all((" %s(" % name) in header for name in EXPORTS) and "#define UDP_POSE_ABI_VERSION 20" in header
    for cited in ("mobilevitv2.py:78-79", "mobilevitv2.py:139-140", "mobilevitv2.py:671-689"):       # the reference lines replaced
        assert cited in header, cited
    assert len(MODELS) == 12


def _refused(fn, args, code, word=None):
    L = _lib.lib()
    assert fn(*args) == code, (fn.__name__, args)
    msg = L.udp_last_error().decode()
    assert msg and fn.__name__ in msg and (word is None or word in msg), (fn.__name__, msg)


def test_silu_refusals_come_before_the_device():
    """Fake non-null pointers: a call that got past its checks would fault."""
    L = _lib.lib()
    one = C.c_void_p(16)
    for count in (0, -4, 6, 1001):
        _refused(L.udp_silu_fwd, (one, one, count, None), UDP_ERR_ARG, "multiple of 4")
        _refused(L.udp_silu_bwd, (one, one, one, count, None), UDP_ERR_ARG, "multiple of 4")
    for args in ((None, one, 8, None), (one, None, 8, None)):
        _refused(L.udp_silu_fwd, args, UDP_ERR_ARG, "null")
    for args in ((None, one, one, 8, None), (one, None, one, 8, None), (one, one, None, 8, None)):
        _refused(L.udp_silu_bwd, args, UDP_ERR_ARG, "null")


def test_gnorm_refusals_workspace_and_split():
    L = _lib.lib()
    one = C.c_void_p(16)
    shape = dict(n=3, h=8, w=6, c=144, cr=144, dt=F32)

    def fwd(null=None, ws_bytes=1 << 20, eps=1e-5, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(6)]           # x, gamma, beta, y, save, workspace
        return (*p[:3], q["n"], q["h"], q["w"], q["c"], q["cr"], q["dt"], eps, *p[3:], ws_bytes, None)

    def bwd(null=None, ws_bytes=1 << 20, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(8)]           # dy, x, gamma, save, dx, dgamma, dbeta, workspace
        return (*p[:4], q["n"], q["h"], q["w"], q["c"], q["cr"], q["dt"], 0, *p[4:], ws_bytes, None)

    need = int(L.udp_gnorm_train_workspace_bytes(3, 8, 6, 144))
    for fn, mk, nptr in ((L.udp_gnorm_train_fwd, fwd, 6), (L.udp_gnorm_train_bwd, bwd, 8)):
        for i in range(nptr):
            _refused(fn, mk(null=i), UDP_ERR_ARG, "null")
        _refused(fn, mk(dt=BF16), UDP_ERR_UNSUPPORTED, "fp32 only")
        _refused(fn, mk(c=142, cr=142), UDP_ERR_ARG)                 # ck % 4
        _refused(fn, mk(cr=145), UDP_ERR_ARG)                        # c_real > ck
        _refused(fn, mk(cr=0), UDP_ERR_ARG)
        _refused(fn, mk(n=0), UDP_ERR_ARG)
        _refused(fn, mk(h=0), UDP_ERR_ARG)
        _refused(fn, mk(ws_bytes=need - 1), UDP_ERR_WORKSPACE, "workspace")
        _refused(fn, mk(ws_bytes=0), UDP_ERR_WORKSPACE, "workspace")
    _refused(L.udp_gnorm_train_fwd, fwd(eps=0.0), UDP_ERR_ARG, "eps")
    # The split is a pure function of (h, w, ck): a run of consecutive pixels holds at least 1024 16-byte channel groups,
    # at most 64 runs per image; the workspace is n * split * (two fp64 sums + two fp32 rows of ck).
    for (h, w, ck), split in (((2, 2, 32), 1), ((6, 4, 64), 1), ((8, 6, 144), 2), ((32, 24, 64), 12), ((16, 12, 96), 5),
                              ((8, 6, 128), 2), ((4, 2, 128), 1), ((64, 48, 64), 48), ((256, 192, 64), 64), ((1, 1, 4), 1)):
        per = -(-1024 // (ck // 4))
        want = -(-h * w // per)
        if want > 64:
            want = -(-h * w // -(-h * w // 64))
        assert want == split and int(L.udp_gnorm_train_split(h, w, ck)) == split, (h, w, ck)
        for n in (1, 2, 32):
            for _ in range(2):                                       # asked twice: the same answer
                assert int(L.udp_gnorm_train_workspace_bytes(n, h, w, ck)) == n * split * (16 + 8 * ck), (n, h, w, ck)
    assert need == 3 * 2 * (16 + 8 * 144)
    for bad in ((0, 8, 6, 144), (3, 0, 6, 144), (3, 8, 6, 142), (3, 8, 6, 0)):
        before = L.udp_last_error()
        assert int(L.udp_gnorm_train_workspace_bytes(*bad)) == 0, bad
        assert bad[0] == 0 or int(L.udp_gnorm_train_split(*bad[1:])) == 0, bad
        assert L.udp_last_error() == before                          # a size query keeps the last real error


def test_linattn_refusals_come_before_the_device():
    L = _lib.lib()
    one = C.c_void_p(16)
    shape = dict(n=2, h=8, w=6, cq=208, d=96, co=96, dt=F32)

    def fwd(null=None, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(4)]           # qkv, out, scores, ctx
        return (p[0], q["n"], q["h"], q["w"], q["cq"], q["d"], q["dt"], p[1], q["co"], p[2], p[3], None)

    def bwd(null=None, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(5)]           # dout, qkv, scores, ctx, dqkv
        return (*p[:4], q["n"], q["h"], q["w"], q["cq"], q["d"], q["co"], q["dt"], p[4], None)

    for fn, mk, nptr in ((L.udp_linattn_train_fwd, fwd, 4), (L.udp_linattn_train_bwd, bwd, 5)):
        for i in range(nptr):
            _refused(fn, mk(null=i), UDP_ERR_ARG, "null")
        _refused(fn, mk(dt=BF16), UDP_ERR_UNSUPPORTED, "fp32 only")
        _refused(fn, mk(h=7), UDP_ERR_UNSUPPORTED, "even")           # odd height / width: no 2x2 patches
        _refused(fn, mk(w=5), UDP_ERR_UNSUPPORTED, "even")
        _refused(fn, mk(d=100, cq=208, co=100), UDP_ERR_UNSUPPORTED, "d % 16")
        _refused(fn, mk(d=8, cq=32, co=8), UDP_ERR_UNSUPPORTED, "d % 16")
        for cq in (193, 192, 224, 196):                              # ck_qkv must be ceil16(1 + 2d) = 208
            _refused(fn, mk(cq=cq), UDP_ERR_ARG, "ck_qkv")
        _refused(fn, mk(co=80), UDP_ERR_ARG, "ck_out")               # < d
        _refused(fn, mk(co=98), UDP_ERR_ARG, "ck_out")               # % 4
        _refused(fn, mk(n=0), UDP_ERR_ARG)
        _refused(fn, mk(d=0, cq=16, co=16), UDP_ERR_ARG)
        _refused(fn, mk(d=1024, cq=2064, co=1024), UDP_ERR_UNSUPPORTED, "too large")
        _refused(fn, mk(h=128, w=128), UDP_ERR_UNSUPPORTED, "too large")     # 4096 pixels per class


# ------------------------------------------------------------------ the restatement
def test_eval_mode_restatement_is_the_inference_restatement():
    """With training=False the graph is the one tests/mobilevitv2_ref.py (the arbiter of the inference tests) states."""
    sd = synth_mobilevitv2_state_dict(seed=5, num_joints=5)
    x = torch.from_numpy(synth.synth_crops(2, 128, 64, seed=3))
    R.forward(sd, x, calibrate=True)                                          # running statistics that are not 0 / 1
    want = R.forward(sd, x)
    before = {k: v.clone() for k, v in sd.items()}
    with torch.no_grad():
        got = T.forward(sd, x, training=False)
    assert torch.equal(got, want)
    assert all(torch.equal(before[k], sd[k]) for k in sd)                     # eval mode moves no statistic
    want64 = R.forward(sd, x, dtype=torch.float64)
    with torch.no_grad():
        got64 = T.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, x.double(), training=False)
    assert torch.equal(got64, want64)


def test_restatement_reproduces_the_reference_modules_training_step(golden_dir):
    """tests/golden/mobilevitv2_train_step.npz is one train-mode step of the reference's own module in fp64: the loss, the
    heat-maps and every stored gradient to 1e-9 of its max (``zero_keys``, zero in exact arithmetic, excluded), the
    running statistics to 1e-9."""
    g = np.load(os.path.join(golden_dir, "mobilevitv2_train_step.npz"))
    sd = synth_mobilevitv2_state_dict(seed=int(g["seed"]), num_joints=5)
    batch = tuple(torch.from_numpy(g[k]) for k in ("x", "target", "target_weight"))
    assert tuple(batch[0].shape) == (2, 3, 128, 64) and tuple(batch[1].shape) == (2, 5, 32, 16)
    loss, y, grads, sd_after = T.loss_and_grads(sd, *batch, torch.float64)
    assert abs(loss - float(g["loss"])) <= 1e-9 * abs(float(g["loss"]))
    assert float(np.abs(y.numpy() - g["heatmaps"]).max()) <= 1e-9 * float(np.abs(g["heatmaps"]).max())
    keys = [str(k) for k in g["keys"]]
    assert keys == list(grads) == [k for k in sd if T.is_param(k)]
    zeros = {str(k) for k in g["zero_keys"]}
    assert {"backbone.classifier.1.weight", "backbone.classifier.1.bias"} <= zeros and len(zeros) == 10
    assert float(grads["backbone.classifier.1.weight"].abs().max()) == 0.0    # the forward never applies it
    n_full = n_sampled = 0
    for i, k in enumerate(keys):
        ours = grads[k].numpy().reshape(-1)
        mx = float(g["gmax"][i])
        if k in zeros:
            assert float(np.abs(ours).max()) <= 1e-9 * float(g["gmax"].max()), k
            continue
        assert abs(float(np.abs(ours).max()) - mx) <= 1e-9 * mx and abs(float(ours.sum()) - float(g["gsum"][i])) <= 1e-9 * mx * ours.size, k
        if ("g_%d" % i) in g.files:
            want, n_full = g["g_%d" % i].reshape(-1), n_full + 1
        else:
            want, ours, n_sampled = g["s_%d" % i], ours[g["p_%d" % i]], n_sampled + 1
        assert float(np.abs(ours - want).max()) <= 1e-9 * mx, k
        assert float(g["e32"][i]) <= 1e-3 * mx, k                             # fp32 is a sane yardstick for the GPU gate
    assert n_full > 100 and n_sampled > 40
    for bn in g["stat_bns"]:
        for s in (".running_mean", ".running_var"):
            want = g["stat_%s%s" % (bn, s)]
            assert float(np.abs(sd_after[str(bn) + s].numpy() - want).max()) <= 1e-9 * float(np.abs(want).max()), bn
    # momentum 0.1, eps 1e-5: the stem's running mean (0 before) is a tenth of the batch mean of its conv
    stem = torch.nn.functional.conv2d(batch[0].double(), sd["backbone.conv_1.block.conv.weight"].double(), stride=2, padding=1).mean(dim=(0, 2, 3))
    assert float((sd_after["backbone.conv_1.block.norm.running_mean"] - 0.1 * stem).abs().max()) <= 1e-12 * float(stem.abs().max())


# ------------------------------------------------------------------ the model surface
def test_factory_surface_follows_is_train_and_the_config():
    from udp_pose_amd.model import PoseMobileViTv2Hip
    assert PoseMobileViTv2Hip.TRAINS is True and PoseMobileViTv2Hip.TRAINER == "MobileViTv2Trainer"
    net = MODELS[NAME](_cfg(), is_train=True)
    assert type(net) is PoseMobileViTv2Hip and net.trainable and net._sd is None          # INIT_WEIGHTS False: load_state_dict
    assert MODELS[NAME](_cfg(init=True), is_train=True)._sd is not None
    assert MODELS[NAME](_cfg(init=True), is_train=False)._sd is None
    off = MODELS[NAME](_cfg(), is_train=False)
    assert type(off) is PoseMobileViTv2Hip and not off.trainable
    for refused in (off.trainer, off.train, off.init_weights):
        with pytest.raises(NotImplementedError, match=NAME):
            refused()
    for is_train in (False, True):                                             # bf16 stays a NotImplementedError
        with pytest.raises(NotImplementedError, match=NAME + ".*bf16"):
            MODELS[NAME](_cfg(), is_train=is_train, dtype="bf16")
    with pytest.raises(RuntimeError, match="load_state_dict"):
        net.trainer()                                                          # trainable, but no weights yet
    for size in (0.75, 1.0):
        assert MODELS[NAME](_cfg(init=True, MODEL_SIZE=size), is_train=True).trainable
    with pytest.raises(NotImplementedError, match=NAME + " MODEL_SIZE"):
        MODELS[NAME](_cfg(MODEL_SIZE=2.0), is_train=True)


@pytest.mark.parametrize("size", [0.5, 1.0])
def test_init_weights_statistics(size):
    """initialize_weights (init_utils.py:218-235) under the backbone YAMLs: kaiming_normal_(mode="fan_out") for every
    conv, zeros / ones elsewhere, N(0, 0.01) for the classifier.  Tolerance: the sample standard deviation of n normal
    draws has relative standard error 1 / sqrt(2 n); six of those is the bound per tensor (one failure in 5e8 per tensor
    under the rule, while a wrong fan -- fan_in for fan_out differs by the factor sqrt(cout / cin) >= sqrt(2) here, or a
    depthwise fan that forgot k*k by 3 -- misses it by hundreds)."""
    torch.manual_seed(3)
    net = MODELS[NAME](_cfg(MODEL_SIZE=size), is_train=True)
    assert net.init_weights() is net
    sd, shapes = net.state_dict(), net.param_shapes()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    checked = 0
    for k, shape in shapes.items():
        if not k.startswith("backbone.") or len(shape) not in (2, 4):
            continue
        n = int(np.prod(shape))
        if n < 1024:
            continue                                                           # too few draws to tell anything (the 3x3 stem: 432)
        std = 0.01 if len(shape) == 2 else math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        tol = 6.0 / math.sqrt(2.0 * n)
        assert abs(float(sd[k].std()) - std) <= tol * std, (k, float(sd[k].std()), std, tol)
        assert abs(float(sd[k].mean())) <= 6.0 * std / math.sqrt(n), k
        checked += 1
    assert checked >= 60                                                       # of the 70 conv / linear weights
    dw = "backbone.layer_4.1.local_rep.0.block.conv.weight"                    # a depthwise weight was among them: torch's fan_out
    assert shapes[dw][1] == 1 and shapes[dw][2] == 3 and int(np.prod(shapes[dw])) >= 1024   # of [C,1,3,3] is C * 9, groups ignored
    for k, shape in shapes.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.startswith("backbone.") and k.endswith(".bias"):                  # BatchNorm, GroupNorm, conv and classifier biases
            assert float(sd[k].abs().max()) == 0.0, k
        if k.startswith("backbone.") and len(shape) == 1 and k.endswith(".weight"):       # BatchNorm and GroupNorm weights
            assert float((sd[k] - 1).abs().max()) == 0.0, k
        if k.endswith("running_mean"):
            assert float(sd[k].abs().max()) == 0.0, k
        if k.endswith("running_var"):
            assert float((sd[k] - 1).abs().max()) == 0.0, k
    # the head keeps torch's defaults: U(+-1/sqrt(fan_in)) for a conv, BatchNorm 1 / 0
    hk = "decoder.duc.0.conv.weight"
    fan = shapes[hk][1] * shapes[hk][2] * shapes[hk][3]
    n = int(np.prod(shapes[hk]))
    assert float(sd[hk].abs().max()) <= fan ** -0.5 * (1 + 2.0 ** -22)
    assert abs(float(sd[hk].std()) - (3 * fan) ** -0.5) <= 6.0 / math.sqrt(2.0 * n) * (3 * fan) ** -0.5       # (uniform: the error is smaller still)
    assert float((sd["decoder.duc.0.bn.weight"] - 1).abs().max()) == 0.0 and float(sd["decoder.duc.0.bn.bias"].abs().max()) == 0.0
    assert 0 < float(sd["final_layer.bias"].abs().max()) <= shapes["final_layer.weight"][1] ** -0.5


def test_init_weights_reads_a_local_backbone_file_strictly(tmp_path):
    """load_pretrained_model (backbones/mobilevitv2.py:55-64): torch.load gives a bare state_dict with the backbone's own
    keys, loaded strictly; anything that is not a file is an error, nothing is downloaded."""
    net = MODELS[NAME](_cfg(), is_train=True)
    shapes = net.param_shapes()
    full = {k[len("backbone."):]: torch.full(tuple(s), 0.25) if not k.endswith("num_batches_tracked") else torch.tensor(7)
            for k, s in shapes.items() if k.startswith("backbone.")}
    path = str(tmp_path / "mobilevitv2-0.5.pt")
    torch.save(full, path)
    torch.manual_seed(4)
    sd = net.init_weights(path).state_dict()
    assert list(sd) == list(shapes)
    for k in shapes:
        if k.startswith("backbone.") and not k.endswith("num_batches_tracked"):
            assert float((sd[k] - 0.25).abs().max()) == 0.0, k
    assert int(sd["backbone.conv_1.block.norm.num_batches_tracked"]) == 7
    assert float(sd["decoder.conv_compress.weight"].std()) > 0 and float((sd["decoder.duc.1.bn.weight"] - 1).abs().max()) == 0.0
    # through the factory
    assert float((MODELS[NAME](_cfg(init=True, pretrained=path), is_train=True).state_dict()["backbone.layer_3.1.global_rep.0.pre_norm_attn.0.bias"]
                  - 0.25).abs().max()) == 0.0
    # strict: a missing key, an unexpected key, another width
    for mutate in (lambda d: d.pop("layer_5.1.global_rep.3.weight"), lambda d: d.update({"conv_1x1_exp.weight": torch.zeros(1)}),
                   lambda d: d.update({"conv_1.block.conv.weight": torch.zeros(32, 3, 3, 3)})):
        bad = dict(full)
        mutate(bad)
        torch.save(bad, path)
        with pytest.raises(RuntimeError, match=NAME):
            net.init_weights(path)
    with pytest.raises(FileNotFoundError, match=NAME):
        net.init_weights(str(tmp_path / "absent.pt"))
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        MODELS[NAME](_cfg(init=True, pretrained="https://example.invalid/mobilevitv2-0.5.pt"), is_train=True)


def test_trainer_refusals_and_layout():
    from udp_pose_amd.mobilevitv2_plan import mobilevitv2_spec
    with pytest.raises(ValueError, match="%s trains in fp32 only.*bf16" % NAME):
        MobileViTv2Trainer(mobilevitv2_spec(EXTRA), 17, "gaussian", {}, device="cpu", dtype="bf16")
    assert issubclass(MobileViTv2Trainer, ShuffleNetV2Trainer)
    for name in ("_key_stride", "_pixshuf", "_dw", "_bn", "_head", "_conv"):   # reused, not copied
        assert name not in vars(MobileViTv2Trainer), name
    assert MobileViTv2Trainer.bn_over_stored is True
    import inspect
    sig = inspect.signature(Trainer._conv).parameters
    assert sig["res"].default is None                                          # every existing call keeps its launches
    sig = inspect.signature(Trainer._bn).parameters
    assert sig["eps"].default == 1e-5 and sig["momentum"].default == 0.1       # the backbone's BatchNorms: the defaults
    for size in (0.5, 0.75):
        sd = synth_mobilevitv2_state_dict(seed=2, num_joints=5, model_size=size)
        tr = MobileViTv2Trainer(mobilevitv2_spec(dict(EXTRA, MODEL_SIZE=size), 5), 5, "gaussian", sd, device="cpu")
        shapes = tr._shapes
        net = MODELS[NAME](_cfg(joints=5, MODEL_SIZE=size), is_train=True)
        assert list(shapes) == list(net.param_shapes())                        # the trainer's key order = param_shapes()
        assert tr._keys == [k for k in net.param_shapes() if T.is_param(k)]
        n = 0
        for k in tr._keys + tr._stat_keys:
            numel = int(np.prod(shapes[k]))
            assert tr._off[k] == n, k
            n += (numel + 15) // 16 * 16 if len(shapes[k]) == 1 else (numel + 3) // 4 * 4
            assert torch.equal(tr.param(k), sd[k].float())
        assert tr.flat.numel() == n
        # depthwise weights are read in place, every other conv is packed; the classifier has no kernel at all
        dws = [k for k in tr._keys if len(shapes[k]) == 4 and shapes[k][1] == 1 and shapes[k][2] == 3]
        assert len(dws) == 6 + 3 and not any(k[:-len(".weight")] in tr._convs for k in dws)     # conv_3x3 and local_rep.0
        assert len(tr._convs) == sum(1 for k in tr._keys if len(shapes[k]) == 4) - 9
        assert tr._convs["backbone.conv_1.block.conv"][4] is None and tr._convs["backbone.layer_1.0.block.exp_1x1.block.conv"][4] is not None
        assert all(k in tr._bucket_of and tuple(tr.grad_of(k).shape) == tuple(shapes[k]) for k in dws)
        assert "backbone.classifier.1.weight" in tr._bucket_of and float(tr.grad_of("backbone.classifier.1.weight").abs().max()) == 0.0
    with pytest.raises(ValueError, match="multiple of 64"):
        tr.forward(torch.zeros(1, 3, 96, 64))
