"""pose_resnet (SimpleBaseline) on the host side, no GPU: the model factory, the op program the planner emits for
ResNet-50 (op census, every state_dict key consumed, FLOPs), the deconv weight layouts of UDP_OP_DECONV applied phase by
phase against F.conv_transpose2d, and the configurations that are refused."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from udp_pose_amd import _lib, f16x2
from udp_pose_amd.model import MODELS, PoseResNetHip
from udp_pose_amd.resnet_plan import PoseResNetProgram, pose_resnet_spec
from udp_pose_amd.synth_resnet import pose_resnet_param_shapes, synth_pose_resnet_state_dict

# MODEL.EXTRA of deep_hrnet/experiments/coco/resnet/res50_256x192_d256x3_adam_lr1e-3.yaml
RES50_EXTRA = {"TARGET_TYPE": "gaussian", "HEATMAP_SIZE": [48, 64], "SIGMA": 2, "FINAL_CONV_KERNEL": 1,
               "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256],
               "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}


def _cfg(**extra):
    return {"MODEL": {"NAME": "pose_resnet", "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "IMAGE_SIZE": [192, 256],
                      "EXTRA": dict(RES50_EXTRA, **extra)}}


def test_models_has_pose_resnet():
    net = MODELS["pose_resnet"](_cfg(), is_train=False)
    assert isinstance(net, PoseResNetHip)
    sd = synth_pose_resnet_state_dict(seed=7)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})            # DataParallel prefixes are stripped
    bad = dict(sd)
    bad["deconv_layers.0.weight"] = torch.zeros(2048, 128, 4, 4)
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict(bad)
    bad = dict(sd)
    del bad["deconv_layers.3.weight"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    with pytest.raises(NotImplementedError):
        net.trainer()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(256, 192), (384, 288)])
def test_res50_program_census(hw, dtype):
    sd = synth_pose_resnet_state_dict(seed=7)
    prog = PoseResNetProgram(sd, pose_resnet_spec(RES50_EXTRA), hw[0], hw[1], dtype)
    ops = prog._ops
    kinds = [op["kind"] for op in ops]
    assert kinds.count(_lib.UDP_OP_STEM7) == 1 and kinds[0] == _lib.UDP_OP_STEM7
    assert kinds.count(_lib.UDP_OP_MAXPOOL) == 1 and kinds[1] == _lib.UDP_OP_MAXPOOL
    assert kinds.count(_lib.UDP_OP_DECONV) == 3
    convs = [op for op in ops if op["kind"] == _lib.UDP_OP_CONV]
    blocks = [op for op in convs if op["name"].endswith(".conv3")]
    downs = [op for op in convs if ".downsample" in op["name"]]
    assert len(blocks) == 16 and all(op["res"] is not None and op["relu"] for op in blocks)      # 3 + 4 + 6 + 3 Bottlenecks
    assert len(downs) == 4
    assert len(convs) == 3 * 16 + 4 + 1
    head = ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17
    assert (head["hout"], head["wout"]) == (hw[0] // 4, hw[1] // 4)
    dec = [op for op in ops if op["kind"] == _lib.UDP_OP_DECONV]
    assert [(op["hin"], op["hout"]) for op in dec] == [(hw[0] // 32, hw[0] // 16), (hw[0] // 16, hw[0] // 8), (hw[0] // 8, hw[0] // 4)]
    assert all(op["ks"] == 4 and op["stride"] == 2 and op["relu"] and op["wfmt"] == int(dtype == "f16x2") for op in dec)
    assert [op["cin"] for op in dec] == [2048, 256, 256]
    # every state_dict key is read by the planner
    assert prog.consumed_keys == set(pose_resnet_param_shapes())
    # FLOPs per image: 2 x 5.426 GMAC at 256x192 (deconvs: 4 * Cin * Cout MACs per output pixel)
    gmac = prog.macs_per_image() / 1e9
    want = 5.426 * hw[0] * hw[1] / (256 * 192)
    assert abs(gmac - want) <= 1e-3 * want, gmac
    deconv_gmac = sum(4 * op["cin"] * op["cout"] * op["hout"] * op["wout"] for op in dec) / 1e9
    assert abs(deconv_gmac - 1.41 * hw[0] * hw[1] / (256 * 192)) < 0.01 * want
    arr = prog.ops_array()
    assert len(arr) == len(ops) and arr[len(arr) - 1].out_buf == _lib.UDP_BUF_OUTPUT


def _unpack_ws(packed, wexp, taps, cout_pad, cin):
    """Inverse of f16x2.pack_weights_ws: bytes -> fp64 [taps][cout_pad][cin] (hi + lo, times 2^-wexp)."""
    nch = (cin + 31) // 32
    h = packed.view(torch.float16).reshape(taps, nch, cout_pad // 32, 2, 2, 4, 4, 4, 8)   # tap, c, pair, nb, plane, kg, a, b, j
    pl = h.permute(4, 0, 2, 6, 3, 7, 1, 5, 8).reshape(2, taps, cout_pad, nch * 32)          # plane, tap, (pair a nb b), (c kg j)
    w = pl[0].to(torch.float64) + pl[1].to(torch.float64)
    return torch.ldexp(w, torch.tensor(-wexp, dtype=torch.float64))[:, :, :cin]


@pytest.mark.parametrize("wfmt", [0, 1])
@pytest.mark.parametrize("bias", [False, True])
def test_deconv_weight_layout_phase_by_phase(wfmt, bias):
    """The packed weights, unpacked and applied phase by phase (2x2 taps over the 3x3 window, scattered to (2m+a,
    2n+b)) equal F.conv_transpose2d(k=4, s=2, p=1) + BatchNorm (eval) with the BN scale folded along dim 1."""
    g = torch.Generator().manual_seed(5)
    cin, cout, h, w, n = 64, 40, 5, 4, 2
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64) * 0.1
    bt = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1 if bias else None
    gamma, beta = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(cout, generator=g, dtype=torch.float64)
    mean, var = torch.randn(cout, generator=g, dtype=torch.float64), torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    ref = F.batch_norm(F.conv_transpose2d(x, wt, bt, stride=2, padding=1), mean, var, gamma, beta, False, 0.0, 1e-5)
    sd = {"deconv_layers.0.weight": wt.float(), "deconv_layers.1.weight": gamma.float(), "deconv_layers.1.bias": beta.float(),
          "deconv_layers.1.running_mean": mean.float(), "deconv_layers.1.running_var": var.float()}
    if bias:
        sd["deconv_layers.0.bias"] = bt.float()
    prog = PoseResNetProgram.__new__(PoseResNetProgram)          # only the deconv emitter, on a hand-made input tensor
    prog.sd, prog.dtype, prog._ops, prog._tensors, prog._blob, prog._blob_size = sd, ("f16x2" if wfmt else "f32"), [], [], [], 0
    from udp_pose_amd.hrnet_plan import _T
    prog._deconv(_T(0, cin, h, w), 0)
    op = prog._ops[0]
    assert op["kind"] == _lib.UDP_OP_DECONV and op["wfmt"] == wfmt and (op["hout"], op["wout"]) == (2 * h, 2 * w)
    blob = prog.weight_blob()
    cp = op["cout_pad"]
    if wfmt:
        nbytes = 16 * ((cin + 31) // 32) * (cp // 32) * 4096
        wp = _unpack_ws(torch.from_numpy(blob[op["w_off"]:op["w_off"] + nbytes].copy()), op["wexp"], 16, cp, cin)
    else:
        wp = torch.from_numpy(blob[op["w_off"]:op["w_off"] + 16 * cp * cin * 4].copy()).view(torch.float32).reshape(16, cp, cin).double()
    b = torch.from_numpy(blob[op["b_off"]:op["b_off"] + 4 * cp].copy()).view(torch.float32).double()
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(n, cp, 2 * h, 2 * w, dtype=torch.float64)
    for a in range(2):
        for bb in range(2):
            acc = torch.zeros(n, cp, h, w, dtype=torch.float64)
            for t in range(2):
                for u in range(2):
                    win = xp[:, :, a + t:a + t + h, bb + u:bb + u + w]                      # 3x3-window offset (a+t, b+u)
                    acc += torch.einsum("oc,nchw->nohw", wp[4 * (2 * a + bb) + 2 * t + u], win)
            out[:, :, a::2, bb::2] = acc + b[None, :, None, None]
    scale = float(ref.abs().max())
    tol = 1e-5 * scale                                   # split fp16 keeps 22 bits of a weight, fp32 24
    assert float((out[:, :cout] - ref).abs().max()) <= tol
    assert float(out[:, cout:].abs().max()) == 0.0


def test_refused_configurations():
    for extra, what in [({"NUM_LAYERS": 18}, "NUM_LAYERS=18"), ({"NUM_LAYERS": 34}, "NUM_LAYERS=34"),
                        ({"NUM_DECONV_KERNELS": [3, 3, 3]}, "NUM_DECONV_KERNELS"),
                        ({"NUM_DECONV_KERNELS": [2, 2, 2]}, "NUM_DECONV_KERNELS"),
                        ({"NUM_DECONV_LAYERS": 2, "NUM_DECONV_FILTERS": [256, 256], "NUM_DECONV_KERNELS": [4, 4]}, "NUM_DECONV_LAYERS"),
                        ({"FINAL_CONV_KERNEL": 5}, "FINAL_CONV_KERNEL")]:
        with pytest.raises(NotImplementedError, match=what):
            MODELS["pose_resnet"](_cfg(**extra), is_train=False)
    with pytest.raises(ValueError, match="f32, f16x2"):
        PoseResNetHip(_cfg(), dtype="bf16")
    for layers in (101, 152):
        assert pose_resnet_spec(dict(RES50_EXTRA, NUM_LAYERS=layers))["layers"][2] == (23 if layers == 101 else 36)


@pytest.mark.parametrize("layers", [101, 152])
def test_deeper_programs_build(layers):
    extra = dict(RES50_EXTRA, NUM_LAYERS=layers, FINAL_CONV_KERNEL=3, DECONV_WITH_BIAS=True)
    spec = pose_resnet_spec(extra)
    sd = synth_pose_resnet_state_dict(seed=1, layers=spec["layers"], final_kernel=3, deconv_with_bias=True)
    prog = PoseResNetProgram(sd, spec, 256, 192, "f16x2")
    assert sum(op["name"].endswith(".conv3") for op in prog._ops) == sum(spec["layers"])
    assert prog._ops[-1]["ks"] == 3
    assert prog.consumed_keys == set(sd)
    assert np.isfinite(prog.macs_per_image())
