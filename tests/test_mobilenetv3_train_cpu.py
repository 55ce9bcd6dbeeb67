"""MobileNetV3-small training on the host side, no GPU: the new exports and every refusal they make before touching the
device, the trainable models ``MODELS[...](cfg, is_train=True)`` returns (init_weights, the local-file rules, "yes
please", the refusals), the trainer's layout, and the pins of the train-mode restatement
(tests/mobilenetv3_train_ref.py).

torchvision is not installed where the tests run, so no fixture of the reference's own module (its backbone is
``torchvision.models.mobilenet_v3_small().features``) can exist.  The restatement is pinned instead (a) in eval mode to
tests/mobilenetv3_ref.py, the arbiter of the inference tests, and (b) to an ``nn.Module`` mirror built here from stock
layers -- nn.Hardswish, nn.Hardsigmoid, nn.BatchNorm2d(eps=1e-3, momentum=0.01) -- whose ``state_dict()`` keys equal
``param_shapes()`` in order and whose autograd step it must reproduce in fp64."""
import ctypes as C
import logging
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import mobilenetv3_ref as R
import mobilenetv3_train_ref as T
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilenetv3 import BLOCKS, squeeze_channels, synth_mobilenetv3_state_dict
from udp_pose_amd.train import (MobileNetV3DeconvTrainer, MobileNetV3Trainer, ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer,
                                Trainer)

PS, DC = "pose_mobilenetv3_small_pixel_shuffle", "pose_mobilenetv3_small"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {PS: {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1},
         DC: {"MODEL_SIZE": "small", "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
              "NUM_DECONV_KERNELS": [4, 4, 4], "FINAL_CONV_KERNEL": 1}}
HEAD = {PS: "pixel_shuffle", DC: "deconv"}
UDP_ERR_ARG, UDP_ERR_UNSUPPORTED, UDP_ERR_WORKSPACE = -1, -3, -4
F32, BF16 = _lib.UDP_F32, _lib.UDP_BF16


def _cfg(name=PS, init=False, pretrained="", **extra):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256], "INIT_WEIGHTS": init,
                      "PRETRAINED": pretrained, "EXTRA": dict(EXTRA[name], **extra)}}


# ------------------------------------------------------------------ the library
EXPORTS = ("udp_dwconvk_train_fwd", "udp_dwconvk_dgrad", "udp_dwconvk_wgrad", "udp_dwconvk_wgrad_workspace_bytes",
           "udp_hswish_fwd", "udp_hswish_bwd", "udp_se_train_fwd", "udp_se_train_bwd", "udp_se_train_workspace_bytes")


def test_exports_and_abi_version():
    L = _lib.lib()
    assert L.udp_abi_version() == 20 and _lib.ABI_VERSION == 20
    for name in EXPORTS:
        assert getattr(L, name) is not None and name in _lib.EXPORTS, name
    with open(os.path.join(ROOT, "include", "udp_pose_hip.h")) as f:
        header = f.read()
    assert all((" %s(" % name) in header for name in EXPORTS) and "#define UDP_POSE_ABI_VERSION 20" in header
    assert "backbones/mobilenetv3.py:5-16" in header and "synth_mobilenetv3.py" in header
    assert max(v for k, v in vars(_lib).items() if k.startswith("UDP_OP_")) == 23 and len(MODELS) == 12


def _refused(fn, args, code, word=None):
    L = _lib.lib()
    assert fn(*args) == code, (fn.__name__, args)
    msg = L.udp_last_error().decode()
    assert msg and fn.__name__ in msg and (word is None or word in msg), (fn.__name__, msg)


def test_depthwise_refusals_come_before_the_device():
    """Fake non-null pointers: a call that got past its checks would fault."""
    L = _lib.lib()
    one = C.c_void_p(16)
    # (x | dy, w, n, hin, win, c, c_real, ks, stride, dtype, out, stream)
    good = dict(a=one, b=one, n=3, h=7, w=9, c=96, cr=88, ks=5, s=1, dt=F32, out=one)

    def fwd(**kw):
        q = dict(good, **kw)
        return (q["a"], q["b"], q["n"], q["h"], q["w"], q["c"], q["cr"], q["ks"], q["s"], q["dt"], q["out"], None)

    def dgrad(**kw):
        q = dict(good, **kw)
        return (q["a"], q["b"], q["n"], q["h"], q["w"], q["c"], q["cr"], q["ks"], q["s"], 0, q["dt"], q["out"], None)

    def wgrad(ws=one, ws_bytes=1 << 24, **kw):
        q = dict(good, **kw)
        return (q["a"], q["b"], q["n"], q["h"], q["w"], q["c"], q["cr"], q["ks"], q["s"], q["dt"], q["out"], ws, ws_bytes, None)

    for fn, mk in ((L.udp_dwconvk_train_fwd, fwd), (L.udp_dwconvk_dgrad, dgrad), (L.udp_dwconvk_wgrad, wgrad)):
        for ks in (4, 7, 1):
            _refused(fn, mk(ks=ks), UDP_ERR_UNSUPPORTED, "kernel size")
        _refused(fn, mk(s=3), UDP_ERR_UNSUPPORTED, "stride")
        _refused(fn, mk(s=0), UDP_ERR_UNSUPPORTED, "stride")
        _refused(fn, mk(dt=BF16), UDP_ERR_UNSUPPORTED, "fp32 only")
        _refused(fn, mk(c=98), UDP_ERR_ARG)                              # c % 4
        _refused(fn, mk(cr=97), UDP_ERR_ARG)                             # c_real > c
        _refused(fn, mk(cr=0), UDP_ERR_ARG)
        _refused(fn, mk(n=0), UDP_ERR_ARG)
        for k in ("a", "b", "out"):
            _refused(fn, mk(**{k: None}), UDP_ERR_ARG, "null")
    _refused(L.udp_dwconvk_wgrad, wgrad(ws=None), UDP_ERR_ARG, "null")
    _refused(L.udp_dwconvk_wgrad, wgrad(ws_bytes=25 * 96 * 4 - 1), UDP_ERR_WORKSPACE, "workspace")     # not one [25][96] partial
    _refused(L.udp_dwconvk_wgrad, wgrad(ks=3, ws_bytes=9 * 96 * 4 - 1), UDP_ERR_WORKSPACE, "workspace")
    # the workspace bound: partials = ceil(rows / ceil(rows / min(rows, 256))) of [ks^2][c] floats; 0 for what is refused
    assert int(L.udp_dwconvk_wgrad_workspace_bytes(3, 7, 9, 96, 5)) == 21 * 25 * 96 * 4
    assert int(L.udp_dwconvk_wgrad_workspace_bytes(32, 16, 12, 240, 5)) == 256 * 25 * 240 * 4
    assert int(L.udp_dwconvk_wgrad_workspace_bytes(40, 8, 10, 48, 3)) == 160 * 9 * 48 * 4
    assert int(L.udp_dwconvk_wgrad_workspace_bytes(256, 1, 1, 576, 5)) == 256 * 25 * 576 * 4
    for bad in ((3, 7, 9, 96, 4), (3, 7, 9, 96, 7), (3, 7, 9, 98, 5), (0, 7, 9, 96, 5)):
        before = L.udp_last_error()
        assert int(L.udp_dwconvk_wgrad_workspace_bytes(*bad)) == 0, bad
        assert L.udp_last_error() == before and b"udp_dwconvk_wgrad:" in before      # a size query keeps the last real error


def test_hswish_refusals_come_before_the_device():
    L = _lib.lib()
    one = C.c_void_p(16)
    for count in (0, -4, 6, 1001):
        _refused(L.udp_hswish_fwd, (one, one, count, None), UDP_ERR_ARG, "multiple of 4")
        _refused(L.udp_hswish_bwd, (one, one, one, count, None), UDP_ERR_ARG, "multiple of 4")
    for args in ((None, one, 8, None), (one, None, 8, None)):
        _refused(L.udp_hswish_fwd, args, UDP_ERR_ARG, "null")
    for args in ((None, one, one, 8, None), (one, None, one, 8, None), (one, one, None, 8, None)):
        _refused(L.udp_hswish_bwd, args, UDP_ERR_ARG, "null")


def test_se_refusals_come_before_the_device():
    L = _lib.lib()
    one = C.c_void_p(16)
    shape = dict(n=3, h=7, w=3, c=128, cr=120, sq=32, dt=F32)

    def fwd(null=None, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(9)]
        return (*p[:5], q["n"], q["h"], q["w"], q["c"], q["cr"], q["sq"], q["dt"], *p[5:], None)

    def bwd(null=None, ws_bytes=1 << 20, **kw):
        q = dict(shape, **kw)
        p = [None if i == null else one for i in range(13)]
        return (*p[:7], q["n"], q["h"], q["w"], q["c"], q["cr"], q["sq"], 0, q["dt"], *p[7:], ws_bytes, None)

    for fn, mk, nptr in ((L.udp_se_train_fwd, fwd, 9), (L.udp_se_train_bwd, bwd, 13)):
        for i in range(nptr):
            _refused(fn, mk(null=i), UDP_ERR_ARG, "null")
        _refused(fn, mk(dt=BF16), UDP_ERR_UNSUPPORTED, "fp32 only")
        _refused(fn, mk(c=126), UDP_ERR_ARG)                             # c % 4
        _refused(fn, mk(cr=129), UDP_ERR_ARG)                            # c_real > c
        _refused(fn, mk(sq=0), UDP_ERR_ARG)
        _refused(fn, mk(c=0, cr=0), UDP_ERR_ARG)
        _refused(fn, mk(n=0), UDP_ERR_ARG)
        _refused(fn, mk(h=0), UDP_ERR_ARG)
    need = int(L.udp_se_train_workspace_bytes(3, 128, 32))
    assert need == (2 * 3 * 128 + 3 * 32) * 4
    _refused(L.udp_se_train_bwd, bwd(ws_bytes=need - 1), UDP_ERR_WORKSPACE, "workspace")
    for bad in ((0, 128, 32), (3, 126, 32), (3, 128, 0), (3, 0, 32)):
        assert int(L.udp_se_train_workspace_bytes(*bad)) == 0, bad


# ------------------------------------------------------------------ the model surface
@pytest.mark.parametrize("name", [PS, DC])
def test_factory_surface_follows_is_train_and_the_config(name):
    from udp_pose_amd.model import PoseMobileNetV3Hip, PoseMobileNetV3PixelShuffleHip
    cls = PoseMobileNetV3PixelShuffleHip if name == PS else PoseMobileNetV3Hip
    assert cls.TRAINS is True and cls.TRAINER == ("MobileNetV3Trainer" if name == PS else "MobileNetV3DeconvTrainer")
    net = MODELS[name](_cfg(name), is_train=True)
    assert type(net) is cls and net.trainable and net._sd is None              # INIT_WEIGHTS False: load_state_dict
    assert MODELS[name](_cfg(name, init=True), is_train=True)._sd is not None
    assert MODELS[name](_cfg(name, init=True), is_train=False)._sd is None
    off = MODELS[name](_cfg(name), is_train=False)
    assert type(off) is cls and not off.trainable
    for refused in (off.trainer, off.train, off.init_weights):
        with pytest.raises(NotImplementedError):
            refused()
    for is_train in (False, True):                                             # bf16 stays a NotImplementedError
        with pytest.raises(NotImplementedError, match="bf16"):
            MODELS[name](_cfg(name), is_train=is_train, dtype="bf16")
    with pytest.raises(RuntimeError, match="load_state_dict"):
        net.trainer()                                                          # trainable, but no weights yet


@pytest.mark.parametrize("name", [PS, DC])
def test_init_weights_statistics(name):
    torch.manual_seed(3)
    net = MODELS[name](_cfg(name), is_train=True)
    assert net.init_weights() is net
    sd, shapes = net.state_dict(), net.param_shapes()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    # kaiming_normal_(mode="fan_out"): std = sqrt(2 / (shape[0] k k)) -- a depthwise, an SE and two 1x1 weights
    for k, shape in (("backbone.0.10.block.1.0.weight", (576, 1, 5, 5)), ("backbone.0.10.block.2.fc1.weight", (144, 576, 1, 1)),
                     ("backbone.0.10.block.2.fc2.weight", (576, 144, 1, 1)), ("backbone.0.10.block.0.0.weight", (576, 96, 1, 1)),
                     ("backbone.0.12.0.weight", (576, 96, 1, 1)), ("backbone.0.2.block.1.0.weight", (72, 1, 3, 3))):
        std = math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
        assert tuple(shapes[k]) == shape and abs(float(sd[k].std()) - std) <= 0.05 * std and abs(float(sd[k].mean())) <= 0.05 * std, k
    for k in shapes:
        backbone_bn = k.startswith("backbone.") and (k.rsplit(".", 1)[0] + ".running_mean") in shapes
        if k.startswith("backbone.") and k.endswith(".bias"):                  # BatchNorm and squeeze-excitation biases
            assert float(sd[k].abs().max()) == 0.0, k
        if backbone_bn and k.endswith(".weight"):
            assert float((sd[k] - 1).abs().max()) == 0.0, k
        if k.endswith("running_mean"):
            assert float(sd[k].abs().max()) == 0.0, k
        if k.endswith("running_var"):
            assert float((sd[k] - 1).abs().max()) == 0.0, k
    # the head keeps torch's defaults: U(+-1/sqrt(fan_in)) for a conv, BatchNorm 1 / 0
    hk = "decoder.duc.0.conv.weight" if name == PS else "deconv_layers.3.weight"
    fan = shapes[hk][1] * shapes[hk][2] * shapes[hk][3]
    assert float(sd[hk].abs().max()) <= fan ** -0.5 * (1 + 2.0 ** -22) and abs(float(sd[hk].std()) - (3 * fan) ** -0.5) <= 0.05 * (3 * fan) ** -0.5
    hb = "decoder.duc.0.bn" if name == PS else "deconv_layers.4"
    assert float((sd[hb + ".weight"] - 1).abs().max()) == 0.0 and float(sd[hb + ".bias"].abs().max()) == 0.0
    assert 0 < float(sd["final_layer.bias"].abs().max()) <= shapes["final_layer.weight"][1] ** -0.5


@pytest.mark.parametrize("wrapped", [False, True])
def test_init_weights_reads_a_local_torchvision_checkpoint(tmp_path, wrapped):
    """A bare state_dict or one under "state_dict"; ``module.`` stripped; ``features.N.`` -> ``backbone.0.N.``;
    ``classifier.*`` ignored; non-strict by name and size."""
    net = MODELS[PS](_cfg(), is_train=True)
    shapes = net.param_shapes()
    ck = {"module.features.0.0.weight": torch.full(shapes["backbone.0.0.0.weight"], 0.5),
          "features.4.block.1.1.running_var": torch.full((96,), 0.25),
          "features.5.block.2.fc1.bias": torch.full((64,), 0.125),
          "module.features.9.block.1.0.weight": torch.full((288, 1, 5, 5), 2.0),
          "features.12.0.weight": torch.zeros(960, 160, 1, 1),                             # another size ('large'): not taken, no error
          "features.13.0.weight": torch.zeros(3, 3, 1, 1),                                 # not a key of the net
          "classifier.0.weight": torch.zeros(1024, 576), "classifier.3.bias": torch.zeros(1000)}
    path = str(tmp_path / "mobilenet_v3_small.pth")
    torch.save({"state_dict": ck, "epoch": 3} if wrapped else ck, path)
    torch.manual_seed(4)
    sd = net.init_weights(path).state_dict()
    assert float((sd["backbone.0.0.0.weight"] - 0.5).abs().max()) == 0.0
    assert float((sd["backbone.0.4.block.1.1.running_var"] - 0.25).abs().max()) == 0.0
    assert float((sd["backbone.0.5.block.2.fc1.bias"] - 0.125).abs().max()) == 0.0
    assert float((sd["backbone.0.9.block.1.0.weight"] - 2.0).abs().max()) == 0.0
    assert tuple(sd["backbone.0.12.0.weight"].shape) == (576, 96, 1, 1) and float(sd["backbone.0.12.0.weight"].std()) > 0
    assert list(sd) == list(shapes) and not any("classifier" in k for k in sd)
    std = math.sqrt(2.0 / 240)
    assert abs(float(sd["backbone.0.5.block.0.0.weight"].std()) - std) <= 0.05 * std               # untouched: the init


@pytest.mark.parametrize("name", [PS, DC])
def test_yes_please_keeps_the_initialisation_and_never_downloads(name, caplog):
    """The recipe's ``PRETRAINED: "yes please"`` (the reference hands it to torchvision, which downloads): one warning,
    the constructor initialisation stays."""
    torch.manual_seed(5)
    with caplog.at_level(logging.WARNING):
        net = MODELS[name](_cfg(name, init=True, pretrained="yes please"), is_train=True)
    warned = [r for r in caplog.records if "yes please" in r.getMessage()]
    assert len(warned) == 1 and name in warned[0].getMessage()
    sd = net.state_dict()
    std = math.sqrt(2.0 / (576 * 25))
    assert abs(float(sd["backbone.0.10.block.1.0.weight"].std()) - std) <= 0.05 * std
    assert float((sd["backbone.0.12.1.weight"] - 1).abs().max()) == 0.0


def test_trainer_refusals_and_layout():
    from udp_pose_amd.mobilenetv3_plan import mobilenetv3_deconv_spec, mobilenetv3_ps_spec
    with pytest.raises(ValueError, match="%s trains in fp32 only.*bf16" % PS):
        MobileNetV3Trainer(mobilenetv3_ps_spec(EXTRA[PS]), 17, "gaussian", {}, device="cpu", dtype="bf16")
    with pytest.raises(ValueError, match="%s trains in fp32 only.*bf16" % DC):
        MobileNetV3DeconvTrainer(mobilenetv3_deconv_spec(EXTRA[DC]), 17, "gaussian", {}, device="cpu", dtype="bf16")
    assert issubclass(MobileNetV3DeconvTrainer, MobileNetV3Trainer) and issubclass(MobileNetV3Trainer, ShuffleNetV2Trainer)
    for name in ("_key_stride", "_pixshuf", "_deconv", "_bn"):                 # reused, not copied
        assert name not in vars(MobileNetV3Trainer) and name not in vars(MobileNetV3DeconvTrainer), name
    assert MobileNetV3Trainer._head is ShuffleNetV2Trainer._head and MobileNetV3DeconvTrainer._head is ShuffleNetV2DeconvTrainer._head
    assert MobileNetV3Trainer.bn_over_stored is True and MobileNetV3Trainer.BACKBONE_BN == dict(eps=1e-3, momentum=0.01)
    import inspect
    sig = inspect.signature(Trainer._bn).parameters
    assert sig["eps"].default == 1e-5 and sig["momentum"].default == 0.1       # every existing call keeps its numbers
    sd = synth_mobilenetv3_state_dict(seed=2, num_joints=5)
    tr = MobileNetV3Trainer(mobilenetv3_ps_spec(EXTRA[PS], 5), 5, "gaussian", sd, device="cpu")
    shapes = tr._shapes
    assert tr._keys == [k for k in shapes if T.is_param(k)]
    n = 0
    for k in tr._keys + tr._stat_keys:
        numel = int(np.prod(shapes[k]))
        assert tr._off[k] == n, k
        n += (numel + 15) // 16 * 16 if len(shapes[k]) == 1 else (numel + 3) // 4 * 4
        assert torch.equal(tr.param(k), sd[k].float())
    assert tr.flat.numel() == n
    # depthwise and squeeze-excitation weights are read in place; every other conv is packed; their gradients have keys
    dws = [k for k in tr._keys if len(shapes[k]) == 4 and shapes[k][1] == 1 and shapes[k][2] > 1]
    ses = [k for k in tr._keys if ".fc1.weight" in k or ".fc2.weight" in k]
    assert len(dws) == 11 and len(ses) == 18 and not any(k[:-len(".weight")] in tr._convs for k in dws + ses)
    assert len(tr._convs) == sum(1 for k in tr._keys if len(shapes[k]) == 4) - 29
    assert tr._convs["backbone.0.0.0"][4] is None and tr._convs["backbone.0.2.block.0.0"][4] is not None
    assert all(k in tr._bucket_of and tuple(tr.grad_of(k).shape) == tuple(shapes[k]) for k in dws + ses)
    assert tr._dw_ws.numel() == 256 * 25 * 576 * 4


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", [PS, DC])
def test_eval_mode_restatement_is_the_inference_restatement(name):
    """With training=False the graph is the one tests/mobilenetv3_ref.py (the arbiter of the inference tests) states."""
    sd = synth_mobilenetv3_state_dict(seed=5, head=HEAD[name], num_joints=5)
    x = torch.from_numpy(synth.synth_crops(2, 64, 64, seed=3))
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


class _ConvBNAct(nn.Sequential):
    def __init__(self, cin, cout, k, stride, groups, act):
        layers = [nn.Conv2d(cin, cout, k, stride, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01)]
        super().__init__(*(layers + ([act()] if act else [])))


class _SE(nn.Module):
    """torchvision.ops.SqueezeExcitation(c, sq, scale_activation=nn.Hardsigmoid)."""

    def __init__(self, c, sq):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.fc2 = nn.Conv2d(c, sq, 1), nn.Conv2d(sq, c, 1)
        self.activation, self.scale_activation = nn.ReLU(), nn.Hardsigmoid()

    def forward(self, x):
        return x * self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


class _InvertedResidual(nn.Module):
    def __init__(self, cin, k, exp, cout, se, act, stride):
        super().__init__()
        act = nn.Hardswish if act == "HS" else nn.ReLU
        layers = [_ConvBNAct(cin, exp, 1, 1, 1, act)] if exp != cin else []
        layers.append(_ConvBNAct(exp, exp, k, stride, exp, act))
        if se:
            layers.append(_SE(exp, squeeze_channels(exp)))
        layers.append(_ConvBNAct(exp, cout, 1, 1, 1, None))
        self.block = nn.Sequential(*layers)
        self.use_res = stride == 1 and cin == cout

    def forward(self, x):
        return x + self.block(x) if self.use_res else self.block(x)


class _DUC(nn.Module):
    def __init__(self, cin, planes):
        super().__init__()
        self.conv, self.bn = nn.Conv2d(cin, planes, 3, padding=1, bias=False), nn.BatchNorm2d(planes)
        self.relu, self.pixel_shuffle = nn.ReLU(), nn.PixelShuffle(2)

    def forward(self, x):
        return self.pixel_shuffle(self.relu(self.bn(self.conv(x))))


class _PSDecoder(nn.Module):
    def __init__(self, inplanes, start, arch):
        super().__init__()
        self.conv_compress = nn.Conv2d(inplanes, start, 1, bias=False)
        ducs, cin = [], start
        for planes in arch:
            ducs.append(_DUC(cin, planes))
            cin = planes // 4
        self.duc = nn.Sequential(*ducs)
        self.out_channels = cin

    def forward(self, x):
        return self.duc(self.conv_compress(x))


class _Mirror(nn.Module):
    """The pose module from stock layers: ``backbone = nn.Sequential(features)`` (backbones/mobilenetv3.py:12), then the
    pixel-shuffle decoder or ``deconv_layers``, then ``final_layer``."""

    def __init__(self, head, joints, deconv_filters=(256, 256, 256)):
        super().__init__()
        features = [_ConvBNAct(3, 16, 3, 2, 1, nn.Hardswish)] + [_InvertedResidual(*b) for b in BLOCKS] + \
            [_ConvBNAct(96, 576, 1, 1, 1, nn.Hardswish)]
        self.backbone = nn.Sequential(nn.Sequential(*features))
        if head == "pixel_shuffle":
            self.decoder = _PSDecoder(576, 256, (512, 256, 128))
            cin = self.decoder.out_channels
        else:
            layers, cin = [], 576
            for planes in deconv_filters:
                layers += [nn.ConvTranspose2d(cin, planes, 4, 2, 1, bias=False), nn.BatchNorm2d(planes), nn.ReLU()]
                cin = planes
            self.deconv_layers = nn.Sequential(*layers)
        self.final_layer = nn.Conv2d(cin, joints, 1)
        self.head = head

    def forward(self, x):
        x = self.backbone(x)
        x = self.decoder(x) if self.head == "pixel_shuffle" else self.deconv_layers(x)
        return self.final_layer(x)


@pytest.mark.parametrize("name", [PS, DC])
def test_restatement_reproduces_an_nn_module_mirror_of_stock_layers(name):
    """Keys equal ``param_shapes()`` in order; one train-mode step under autograd in fp64: loss, heat-maps, every
    parameter gradient and every running statistic."""
    kw = dict(deconv_filters=(64, 32, 32)) if name == DC else {}
    extra = dict(NUM_DECONV_FILTERS=[64, 32, 32]) if name == DC else {}
    cfg = _cfg(name, **extra)
    cfg["MODEL"]["NUM_JOINTS"] = 5
    shapes = MODELS[name](cfg, is_train=True).param_shapes()
    mirror = _Mirror(HEAD[name], 5, **kw).double()
    assert list(mirror.state_dict()) == list(shapes)
    assert all(tuple(v.shape) == tuple(shapes[k]) for k, v in mirror.state_dict().items())
    assert sum(p.numel() for p in mirror.backbone.parameters()) == 927008
    sd = synth_mobilenetv3_state_dict(seed=11, head=HEAD[name], num_joints=5, **kw)
    mirror.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    x, tg, tw = T.make_batch(2, 5, 64, 64, seed=12)
    loss, y, grads, sd_after = T.loss_and_grads(sd, x, tg, tw, torch.float64)
    mirror.train()
    ym = mirror(x.double())
    lm = T.joints_mse(ym, tg.double(), tw.double())
    lm.backward()
    assert abs(float(lm.detach()) - loss) <= 1e-12 * abs(loss)
    assert float((ym.detach() - y).abs().max()) <= 1e-12 * float(y.abs().max())
    named = dict(mirror.named_parameters())
    assert list(named) == list(grads)
    # Two fp64 evaluations of one graph that order their roundings differently (nn.Hardswish against x * (clamp / 6), the
    # fused batch-norm backward against autograd through F.batch_norm's pieces): 2^-53 times the conditioning of a step
    # whose BatchNorms average as few as 8 values.  1e-7 of a tensor's max is 20 x the largest difference seen (5e-9, the
    # stem weight) and far below what a wrong formula does -- eps 1e-5 for 1e-3, or the other hard-swish piece at one
    # element, moves gradients by a percent.  The bias of a project BatchNorm has a zero gradient in exact arithmetic
    # (the expand conv + BatchNorm behind it removes a per-channel constant): rounding noise without a scale of its own.
    gscale = max(float(g.abs().max()) for g in grads.values())
    n_zero = 0
    for k, g in grads.items():
        mx, e = float(g.abs().max()), float((named[k].grad - g).abs().max())
        if mx <= 1e-12 * gscale:
            assert k.endswith(".1.bias") and float(named[k].grad.abs().max()) <= 1e-12 * gscale, k
            n_zero += 1
            continue
        assert e <= 1e-7 * mx, (k, e, mx)
    assert n_zero == 11                                                        # one per InvertedResidual
    after = mirror.state_dict()
    n_stats = 0
    for k in shapes:
        if k.endswith("running_mean") or k.endswith("running_var"):
            want = after[k]
            assert float((sd_after[k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
            n_stats += 1
    assert n_stats == 2 * sum(1 for k in shapes if k.endswith("running_mean")) > 60
    # the backbone's momentum is 0.01: the stem's running mean (0 before) is that fraction of the batch mean of its conv
    stem = torch.nn.functional.conv2d(x.double(), sd["backbone.0.0.0.weight"].double(), stride=2, padding=1).mean(dim=(0, 2, 3))
    assert float(sd["backbone.0.0.1.running_mean"].abs().max()) == 0.0
    assert float((sd_after["backbone.0.0.1.running_mean"] - 0.01 * stem).abs().max()) <= 1e-12 * float(stem.abs().max())
