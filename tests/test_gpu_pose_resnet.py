"""pose_resnet (SimpleBaseline) on the GPU: the UDP_OP_DECONV kernel against F.conv_transpose2d in fp64, the wide
Bottleneck conv shapes ResNet-50 adds to the existing conv kernels, and the whole network against the reference
module's own heat-maps / get_final_preds output (tests/golden/resnet50_cfg0.npz) and the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import decode as odec                                   # noqa: E402
from oracle import resnet as oresnet                                # noqa: E402
from udp_pose_amd import _lib, f16x2, synth                         # noqa: E402
from udp_pose_amd.inference import decode_device                    # noqa: E402
from udp_pose_amd.model import MODELS                               # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_state_dict  # noqa: E402

RES50_EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
               "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}


def _cfg(**extra):
    return {"MODEL": {"NAME": "pose_resnet", "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": dict(RES50_EXTRA, **extra)}}


def _q(dtype):
    """Operands exactly as the device holds them (split fp16: 22-bit hi + lo pairs)."""
    return (lambda t: f16x2.decode(f16x2.encode(t))) if dtype == "f16x2" else (lambda t: t)


def _nhwc(t, dtype):
    t = t.permute(0, 2, 3, 1)
    return (f16x2.encode(t) if dtype == "f16x2" else t.contiguous()).cuda()


def _run(op, dtype, n, x, w, b, out, res=None):
    _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES[dtype], n, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b),
                                           _lib.ptr(res), None, None, None, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()


def _nan_out(dtype, n, h, w, c):
    if dtype == "f16x2":
        return torch.full((n, h, w, 2, c), float("nan"), dtype=torch.float16, device="cuda")
    return torch.full((n, h, w, c), float("nan"), dtype=torch.float32, device="cuda")


def _read(out, dtype):
    return (f16x2.decode(out) if dtype == "f16x2" else out).cpu().permute(0, 3, 1, 2).double().numpy()


def _gate(got, ref, dtype):
    assert not np.isnan(got).any(), "output not fully written"
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= 1e-4 * scale, (err, scale)
    if dtype == "f16x2":
        assert err <= 2e-5 * scale, (err, scale)


# ------------------------------------------------------------------ the deconv op
DECONV_SHAPES = [(2048, 256, 8, 6), (256, 256, 16, 12), (256, 256, 32, 24), (2048, 256, 12, 9)]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("relu,bias", [(True, False), (False, True)])
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("shape", DECONV_SHAPES, ids=lambda s: "%d-%d_%dx%d" % s)
def test_deconv_matches_conv_transpose2d_fp64(shape, n, relu, bias, dtype):
    cin, cout, h, w = shape
    rng = np.random.Generator(np.random.PCG64(cin + h + n))
    q = _q(dtype)
    x = q(torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)))
    wt = q(torch.from_numpy((rng.standard_normal((cin, cout, 4, 4)) * np.sqrt(2.0 / (cin * 4))).astype(np.float32)))
    bt = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32)) if bias else torch.zeros(cout)
    ref = F.conv_transpose2d(x.double(), wt.double(), bt.double(), stride=2, padding=1)
    if relu:
        ref = F.relu(ref)
    cout_pad = (cout + 31) // 32 * 32
    if dtype == "f16x2":
        packed, wexp = f16x2.pack_deconv_weights_ws(wt, cout_pad)
        d_w = packed.cuda()
    else:
        d_w, wexp = f16x2.deconv_phase_taps(wt, cout_pad).contiguous().cuda(), 0
    bp = torch.zeros(cout_pad)
    bp[:cout] = bt
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DECONV, 4, 2, int(relu)
    op.cin, op.cout, op.cout_pad = cin, cout, cout_pad
    op.hin, op.win, op.hout, op.wout = h, w, 2 * h, 2 * w
    op.wfmt, op.wexp = int(dtype == "f16x2"), wexp
    out = _nan_out(dtype, n, 2 * h, 2 * w, cout)
    _run(op, dtype, n, _nhwc(x, dtype), d_w, bp.cuda(), out)
    _gate(_read(out, dtype), ref.numpy(), dtype)


def test_deconv_rejects_bf16_and_bad_shapes():
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_DECONV, 4, 2, 1
    op.cin, op.cout, op.cout_pad, op.hin, op.win, op.hout, op.wout = 256, 256, 256, 8, 6, 16, 12
    buf = torch.zeros(1 << 22, dtype=torch.float32, device="cuda")
    lib = _lib.lib()
    args = (1, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), None, None, None, None, _lib.ptr(buf[1 << 21:]), _lib.stream_ptr())
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_BF16, *args) == -3                # UDP_ERR_UNSUPPORTED
    op.hout = 15
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_F32, *args) == -1                 # UDP_ERR_ARG
    op.hout, op.wfmt = 16, 1
    assert lib.udp_conv2d_fused(C.byref(op), _lib.UDP_F32, *args) == -1                 # fp32 takes wfmt 0


# ------------------------------------------------------------------ wide Bottleneck convs of ResNet-50
WIDE_CASES = [
    # ks, stride, cin, cout, h, w (input), res
    (1, 1, 512, 2048, 8, 6, True),       # layer4 conv3 + shortcut
    (1, 1, 2048, 512, 8, 6, False),      # layer4 conv1
    (1, 1, 2048, 512, 12, 9, False),     # the same at 384x288 (ragged tiles)
    (1, 1, 512, 2048, 12, 9, True),
    (1, 2, 1024, 2048, 16, 12, False),   # layer4.0 downsample
    (1, 2, 1024, 2048, 24, 18, False),
    (3, 2, 256, 256, 32, 24, False),     # layer3.0 conv2
    (3, 2, 512, 512, 16, 12, False),     # layer4.0 conv2
    (3, 1, 512, 512, 8, 6, False),       # layer4 conv2
    (1, 1, 1024, 256, 16, 12, False),    # layer3 conv1
]


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "k%ds%d_%d-%d_%dx%d" % c[:6])
def test_wide_convs(case, dtype):
    ks, stride, cin, cout, h, w, res = case
    n = 3
    rng = np.random.Generator(np.random.PCG64(cin + cout + h))
    q = _q(dtype)
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    x = q(torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32)))
    wt = q(torch.from_numpy((rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2.0 / (cin * ks * ks))).astype(np.float32)))
    bt = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32))
    r = q(torch.from_numpy(rng.standard_normal((n, cout, ho, wo)).astype(np.float32))) if res else None
    ref = F.conv2d(x.double(), wt.double(), bt.double(), stride=stride, padding=pad)
    if r is not None:
        ref = ref + r.double()
    ref = F.relu(ref)
    wp = wt.permute(2, 3, 0, 1).reshape(ks * ks, cout, cin).contiguous()
    if dtype == "f16x2":                                   # the weight-stationary kernels, as the planner packs them
        packed, wexp = f16x2.pack_weights_ws(wp)
        d_w = packed.cuda()
    else:
        d_w, wexp = wp.cuda(), 0
    op = _lib.ConvOp()
    op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, ks, stride, 1
    op.cin, op.cout, op.cout_pad = cin, cout, cout
    op.hin, op.win, op.hout, op.wout = h, w, ho, wo
    op.wfmt, op.wexp = int(dtype == "f16x2"), wexp
    out = _nan_out(dtype, n, ho, wo, cout)
    _run(op, dtype, n, _nhwc(x, dtype), d_w, bt.cuda(), out, res=_nhwc(r, dtype) if res else None)
    _gate(_read(out, dtype), ref.numpy(), dtype)


# ------------------------------------------------------------------ whole network
def _dark_shift(hm):
    coords, _, _ = odec.get_max_preds(hm)
    return np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2)


def _fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "resnet50_cfg0.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    return g, synth_pose_resnet_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_res50_matches_reference_fixture(golden_dir, dtype):
    g, sd = _fixture(golden_dir)
    net = MODELS["pose_resnet"](_cfg(), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval()
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19)).cuda()
    hm = net(x).clone()
    got = hm.cpu().numpy()
    assert got.shape == (1, 17, 64, 48)
    assert float(np.abs(got - g["heatmaps"]).max()) <= 1e-3
    np.testing.assert_array_equal(got.reshape(1, 17, -1).argmax(2), g["heatmaps"].reshape(1, 17, -1).argmax(2))
    c, s = np.asarray(g["center"], np.float64), np.asarray(g["scale"], np.float64)
    preds, maxvals, _, idx = decode_device(hm, torch.from_numpy(c), torch.from_numpy(s), "gaussian", True, 4.0, True)
    torch.cuda.synchronize()
    assert float(np.abs(maxvals.cpu().numpy() - g["maxvals"]).max()) <= 1e-3
    preds = preds.cpu().numpy()
    # decode of the device heat-maps == oracle decode of the same maps (well-conditioned joints)
    hp, _, _, hidx = odec.get_final_preds("gaussian", True, 4.0, got.copy(), c, s)
    np.testing.assert_array_equal(idx.cpu().numpy(), hidx)
    hgood = _dark_shift(got) < 1.5
    assert float(np.abs(preds - hp)[hgood].max()) <= 1e-3
    # keypoints vs the reference's get_final_preds: median 1e-3 px, 2e-2 px on the joints whose Taylor step is a
    # genuine sub-pixel refinement (DARK amplifies 1e-5 heat-map noise where the Hessian is near singular)
    err = np.abs(preds - g["preds"]).max(axis=2)
    good = _dark_shift(g["heatmaps"].astype(np.float32)) < 1.5
    print("res50 %s keypoint error px: median %.2g, max(well-conditioned %d/%d) %.2g, max(all) %.2g"
          % (dtype, np.median(err), good.sum(), good.size, err[good].max(), err.max()))
    assert good.mean() > 0.5 and err[good].max() < 2e-2 and np.median(err) < 1e-3


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_res50_384x288_deconv_bias_matches_oracle(dtype):
    sd = synth_pose_resnet_state_dict(seed=11, deconv_with_bias=True)
    x = torch.from_numpy(synth.synth_crops(2, 384, 288, seed=23))
    oresnet.pose_resnet_forward(sd, x, calibrate=True)                    # BatchNorm statistics of this batch
    ref = oresnet.pose_resnet_forward(sd, x).numpy()
    net = MODELS["pose_resnet"](_cfg(DECONV_WITH_BIAS=True), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    got = net(x.cuda()).clone().cpu().numpy()
    assert got.shape == (2, 17, 96, 72)
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(got - ref).max()) <= 1e-3 * scale
    np.testing.assert_array_equal(got.reshape(2, 17, -1).argmax(2), ref.reshape(2, 17, -1).argmax(2))


@pytest.fixture(scope="module")
def res50(golden_dir):
    return _fixture(golden_dir)[1]


@pytest.mark.parametrize("dtype", ["f16x2", "f32"])
def test_res50_flip_batch64(res50, dtype):
    """N = 64 with the flip test (128 images per launch sequence): the mirrored half equals an explicit forward of the
    W-mirrored batch bit for bit (the K loop order of every kernel is independent of the tile, so batch-size dependent
    tile choices change no number), replay == eager, and sampled images equal the CPU oracle."""
    net = MODELS["pose_resnet"](_cfg(), is_train=False, dtype=dtype).load_state_dict(res50).to("cuda")
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=33)).repeat(8, 1, 1, 1)
    x[40:] += 0.01 * torch.randn(24, 3, 256, 192, generator=torch.Generator().manual_seed(1))
    xd = x.cuda()
    raw = net.raw_forward(xd, flip_test=True).clone()
    assert raw.shape == (128, 17, 64, 48) and torch.isfinite(raw).all()
    assert torch.equal(raw, net.raw_forward(xd, flip_test=True))           # graph replay
    net.use_graph = False
    assert torch.equal(raw, net.raw_forward(xd, flip_test=True))           # eager launches
    net.use_graph = True
    mirrored = net.raw_forward(torch.flip(xd, dims=[3]).contiguous()).clone()
    assert torch.equal(mirrored, raw[64:])
    assert torch.equal(raw[0], raw[8])
    for i in (0, 45):
        ref = oresnet.pose_resnet_forward(res50, torch.cat([x[i:i + 1], torch.flip(x[i:i + 1], dims=[3])])).numpy()
        got = raw[[i, 64 + i]].cpu().numpy()
        assert float(np.abs(got - ref).max()) <= 1e-3


@pytest.mark.parametrize("n", [64, 17])
def test_res50_sub_batch_lanes_change_no_number(res50, n):
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=71)).cuda().repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()
    x += 0.01 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    out = {}
    saved = os.environ.get("UDP_POSE_LANES")
    try:
        for lanes in ("1", "2"):
            os.environ["UDP_POSE_LANES"] = lanes
            net = MODELS["pose_resnet"](_cfg(), is_train=False, dtype="f16x2").load_state_dict(res50).to("cuda")
            a = net.raw_forward(x, flip_test=True).clone()
            assert torch.equal(a, net.raw_forward(x, flip_test=True)) and torch.isfinite(a).all()
            assert _lib.lib().udp_hrnet_lanes(net._compiled[(256, 192)][0], C.c_int(n)) == int(lanes)
            out[lanes] = a
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_LANES", None)
        else:
            os.environ["UDP_POSE_LANES"] = saved
    assert torch.equal(out["1"], out["2"])


def test_res50_flops_and_overflow_flag(res50):
    net = MODELS["pose_resnet"](_cfg(), is_train=False, dtype="f16x2").load_state_dict(res50).to("cuda")
    _lib.f16x2_overflow(reset=True)
    net(torch.from_numpy(synth.synth_crops(2, 256, 192, seed=3)).cuda())
    handle, _, prog = net._compiled[(256, 192)]
    assert abs(_lib.lib().udp_hrnet_flops_per_image(handle) - 2 * prog.macs_per_image()) <= 1e-6 * prog.macs_per_image()
    assert not _lib.f16x2_overflow(reset=True)
