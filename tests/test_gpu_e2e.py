"""GPU end-to-end parity: HRNet forward (+flip-test) + UDP decode vs the oracle and
the reference-generated heat-maps in tests/golden.  Through the C ABI."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import data as odata              # noqa: E402
from oracle import decode as odec             # noqa: E402
from oracle import flip as oflip              # noqa: E402
from oracle import hrnet as ohrnet            # noqa: E402
from udp_pose_amd import synth                # noqa: E402
from udp_pose_amd.inference import decode_device  # noqa: E402
from udp_pose_amd.model import MODELS         # noqa: E402
from udp_pose_amd.transforms import COCO_FLIP_PAIRS, flip_fuse  # noqa: E402


def _cfg(extra, nj, tt):
    return {"MODEL": {"NAME": "pose_hrnet", "EXTRA": extra, "NUM_JOINTS": nj, "TARGET_TYPE": tt}}


def _w32(golden_dir, tt):
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_w32_%s.npz" % tt)))
    return synth.synth_state_dict(synth.W32_EXTRA, 17, tt, seed=0, bn_calib=calib)


@pytest.fixture(scope="module")
def w32_gaussian(golden_dir):
    sd = _w32(golden_dir, "gaussian")
    net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False)
    net.load_state_dict(sd, strict=True)
    return sd, net.to("cuda").eval()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_mini_hrnet_matches_reference_fixture(golden_dir, dtype):
    """Width-16 mini HRNet: final heat-maps of the REFERENCE module (tests/golden/hrnet_mini.npz)."""
    g = np.load(os.path.join(golden_dir, "hrnet_mini.npz"))
    extra = synth.scaled_extra(16, modules=(1, 2, 2), blocks=2)
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth.synth_state_dict(extra, 5, "gaussian", seed=1, bn_calib=calib)
    net = MODELS["pose_hrnet"](_cfg(extra, 5, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(2, 96, 64, seed=3)).cuda()
    got = net(x).clone().cpu().numpy()
    assert got.shape == (2, 5, 24, 16)
    np.testing.assert_allclose(got, g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(got.reshape(2, 5, -1).argmax(2), g["out"].reshape(2, 5, -1).argmax(2))


def test_psa_mini_matches_reference_fixture(golden_dir):
    """pose_hrnet_psa mini net (PSA.py:190-269 after conv1 of every BasicBlock) vs the REFERENCE module."""
    g = np.load(os.path.join(golden_dir, "hrnet_psa_mini.npz"))
    extra = synth.scaled_extra(32, modules=(1, 2, 1), blocks=2)
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=6, bn_calib=calib, psa=True)
    x = torch.from_numpy(synth.synth_crops(2, 128, 96, seed=24)).cuda()
    net = MODELS["pose_hrnet_psa"](_cfg(extra, 17, "gaussian"), is_train=False).load_state_dict(sd).to("cuda")
    got = net(x).clone().cpu().numpy()
    assert got.shape == (2, 17, 32, 24)
    np.testing.assert_allclose(got, g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(got.reshape(2, 17, -1).argmax(2), g["out"].reshape(2, 17, -1).argmax(2))
    # flip-folded batch (images N..2N-1 mirrored) still matches a separate mirrored forward
    both = net.raw_forward(x, flip_test=True).clone()
    mirrored = net(torch.flip(x, dims=[3])).clone()
    torch.testing.assert_close(both[2:], mirrored, rtol=0, atol=1e-5)
    # split-fp16 storage: the same north-star gate as fp32 (the attention ops read / write hi + lo pairs)
    nh = MODELS["pose_hrnet_psa"](_cfg(extra, 17, "gaussian"), is_train=False, dtype="f16x2").load_state_dict(sd).to("cuda")
    gh = nh(x).clone().cpu().numpy()
    print("psa mini f16x2 max abs err %.3g" % np.abs(gh - g["out"]).max())
    np.testing.assert_allclose(gh, g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(gh.reshape(2, 17, -1).argmax(2), g["out"].reshape(2, 17, -1).argmax(2))
    # bf16 storage: sanity only (attention softmax amplifies rounding; gate = fraction of the signal)
    nb = MODELS["pose_hrnet_psa"](_cfg(extra, 17, "gaussian"), is_train=False, dtype="bf16").load_state_dict(sd).to("cuda")
    gb = nb(x).clone().cpu().numpy()
    assert np.sqrt(((gb - g["out"]) ** 2).mean()) < 0.15 * g["out"].std()


@pytest.mark.parametrize("modules,blocks", [((1, 1, 1), 1), ((1, 2, 2), 2)])
def test_small_hrnet_fp32_all_module_kinds(modules, blocks):
    extra = synth.scaled_extra(32, modules=modules, blocks=blocks)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=4)
    x = torch.from_numpy(synth.synth_crops(3, 128, 96, seed=6))
    ohrnet.hrnet_forward(sd, extra, x, calibrate=True)
    ref = ohrnet.hrnet_forward(sd, extra, x).numpy()
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False).load_state_dict(sd).to("cuda")
    got = net(x.cuda()).clone().cpu().numpy()
    assert got.shape == ref.shape == (3, 17, 32, 24)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3 * max(1.0, np.abs(ref).max()))


def test_w32_fp32_matches_reference_heatmaps(golden_dir, w32_gaussian):
    """Config 2 network, fp32 mode, on the two crops whose heat-maps the REFERENCE module produced."""
    _, net = w32_gaussian
    g = np.load(os.path.join(golden_dir, "hrnet_w32_gaussian.npz"))
    x = torch.from_numpy(synth.synth_crops(2, 256, 192, seed=5)).cuda()
    got = net(x).clone().cpu().numpy()
    err = np.abs(got - g["out"]).max()
    print("w32 fp32 max abs heat-map error vs reference: %.3g (absmax %.3g)" % (err, np.abs(g["out"]).max()))
    np.testing.assert_allclose(got, g["out"], rtol=0, atol=1e-3)           # north-star tolerance
    ref_idx = g["out"].reshape(2, 17, -1).argmax(2)
    np.testing.assert_array_equal(got.reshape(2, 17, -1).argmax(2), ref_idx)   # arg-max bit-exact


def test_w32_f16x2_matches_reference_heatmaps(golden_dir, w32_gaussian):
    """Config 2 network in the split-fp16 throughput mode (three fp16 MFMAs per product, 22-bit operands,
    fp32 accumulate): the SAME gate as the fp32 mode -- north-star 1e-3 and arg-max bit-exact -- on the two
    crops whose heat-maps the REFERENCE module produced."""
    sd, _ = w32_gaussian
    g = np.load(os.path.join(golden_dir, "hrnet_w32_gaussian.npz"))
    net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype="f16x2")
    net.load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(2, 256, 192, seed=5)).cuda()
    got = net(x).clone().cpu().numpy()
    err = np.abs(got - g["out"]).max()
    print("w32 f16x2 max abs heat-map error vs reference: %.3g (absmax %.3g)" % (err, np.abs(g["out"]).max()))
    np.testing.assert_allclose(got, g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(got.reshape(2, 17, -1).argmax(2), g["out"].reshape(2, 17, -1).argmax(2))


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_w32_offset_head_matches_reference_heatmaps(golden_dir, dtype):
    sd = _w32(golden_dir, "offset")
    net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "offset"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    g = np.load(os.path.join(golden_dir, "hrnet_w32_offset.npz"))
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=5)).cuda()
    got = net(x).clone().cpu().numpy()
    assert got.shape == (1, 51, 64, 48)
    np.testing.assert_allclose(got, g["out"], rtol=0, atol=1e-3)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_w32_flip_test_and_decode_end_to_end(w32_gaussian, dtype):
    """forward + mirrored forward + flip fuse + DARK decode vs the oracle pipeline (N=3), in the reference's
    precision and in the parity-grade split-fp16 mode (the bench headline's mode) under the same gates."""
    sd, net = w32_gaussian
    if dtype != "f32":
        net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype=dtype)
        net = net.load_state_dict(sd, strict=True).to("cuda").eval()
    x = torch.from_numpy(synth.synth_crops(3, 256, 192, seed=21))
    ref = ohrnet.hrnet_forward(sd, synth.W32_EXTRA, torch.cat([x, torch.flip(x, dims=[3])])).numpy()
    ref_hm = oflip.flip_fuse(ref[:3], ref[3:], oflip.COCO_FLIP_PAIRS, False)
    c, s = synth.synth_center_scale(3, seed=5)
    rp, rm, _, ridx = odec.get_final_preds("gaussian", True, 4.0, ref_hm.copy(), c, s)
    raw = net.raw_forward(x.cuda(), flip_test=True)
    np.testing.assert_allclose(raw.cpu().numpy(), ref, rtol=0, atol=1e-3)
    hm = flip_fuse(raw[:3], raw[3:], COCO_FLIP_PAIRS, False)
    np.testing.assert_allclose(hm.cpu().numpy(), ref_hm, rtol=0, atol=1e-3)
    preds, maxvals, _, idx = decode_device(hm, torch.from_numpy(c.astype(np.float64)),
                                           torch.from_numpy(s.astype(np.float64)), "gaussian", True, 4.0, True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_allclose(maxvals.cpu().numpy(), rm, rtol=0, atol=1e-3)
    # (a) decode kernel on the device heat-maps == oracle decode of the SAME heat-maps
    hp, hmv, _, hidx = odec.get_final_preds("gaussian", True, 4.0, hm.cpu().numpy().copy(), c, s)
    np.testing.assert_array_equal(idx.cpu().numpy(), hidx)
    hgood = _dark_shift(hm.cpu().numpy()) < 1.5
    np.testing.assert_allclose(preds.cpu().numpy()[hgood], hp[hgood], rtol=0, atol=1e-3)   # north-star tolerance
    np.testing.assert_allclose(preds.cpu().numpy(), hp, rtol=5e-3, atol=1e-3)   # ill-conditioned Hessians
    # (b) whole pipeline vs the oracle pipeline.  DARK solves H^-1 D on second differences of a
    # log map, so 1e-5 heat-map noise is amplified by 1/|H|: compare where the oracle's own Taylor
    # step is a genuine sub-pixel refinement (|shift| < 1.5 heat-map px); report the rest.
    err = np.abs(preds.cpu().numpy() - rp).max(axis=2)
    shift = _dark_shift(ref_hm)
    good = shift < 1.5
    print("w32 %s end-to-end keypoint error px: median %.2g, p95 %.2g, max(well-conditioned %d/%d) %.2g, max(all) %.2g"
          % (dtype, np.median(err), np.percentile(err, 95), good.sum(), good.size, err[good].max(), err.max()))
    assert good.mean() > 0.5
    assert err[good].max() < 2e-2
    assert np.median(err) < 1e-3        # north-star tolerance holds for the typical joint


def _dark_shift(hm):
    """|Taylor shift| (heat-map px) the oracle applies per joint."""
    coords, _, _ = odec.get_max_preds(hm)
    res = odec.post(coords, hm.copy())
    return np.abs(res - coords).max(axis=2)


@pytest.mark.parametrize("dtype", ["f16x2", "bf16", "f32"])
def test_w32_batch64_properties(w32_gaussian, dtype):
    """Config 2 at its own size (N = 64, flip test on -> 128 images per launch sequence) in every storage mode
    bench.py times: per-image results do not depend on the batch they ride in, the mirrored half equals an
    explicit forward of mirrored inputs, hipGraph replay equals eager launches (merged branch launches, fused
    blocks, the tile chooser's >= 512-workgroup rule at 128 images) -- all bit for bit."""
    sd, net = w32_gaussian
    if dtype != "f32":
        net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype=dtype)
        net.load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=33)).cuda().repeat(8, 1, 1, 1)   # N = 64
    x[40:] += 0.01 * torch.randn(24, 3, 256, 192, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    raw = net.raw_forward(x, flip_test=True).clone()
    assert raw.shape == (128, 17, 64, 48) and torch.isfinite(raw).all()
    replay = net.raw_forward(x, flip_test=True).clone()          # second call = graph replay
    assert torch.equal(raw, replay)
    net.use_graph = False
    eager = net.raw_forward(x, flip_test=True).clone()
    net.use_graph = True
    assert torch.equal(raw, eager)
    assert torch.equal(raw[0], raw[8])                            # identical crops -> identical maps
    one = net.raw_forward(x[41:42].contiguous()).clone()
    assert torch.equal(one[0], raw[41])                           # batch-independence, bit for bit
    mirrored = net.raw_forward(torch.flip(x[:4], dims=[3]).contiguous()).clone()
    assert torch.equal(mirrored, raw[64:68])                      # in-kernel mirror == explicit flip


@pytest.mark.parametrize("n,flip", [(64, True), (17, True), (33, False), (16, True)])
def test_sub_batch_lanes_change_no_number(w32_gaussian, n, flip):
    """udp_hrnet_forward runs a split-fp16 batch of 16 crops or more as two sub-batch lanes (two hipGraphs, the second
    on an internal stream beside the first, mirrored rows copied into place; udp_hrnet_lanes).  The heat-maps are those
    of one lane, bit for bit -- even and odd splits, with and without the flip test, replayed twice (the second replay
    runs while nothing orders it behind the first but the join)."""
    import ctypes as C
    from udp_pose_amd import _lib
    sd, _ = w32_gaussian
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=71)).cuda().repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()
    x += 0.01 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    out = {}
    saved = os.environ.get("UDP_POSE_LANES")
    try:
        for lanes in ("1", "2"):
            os.environ["UDP_POSE_LANES"] = lanes
            net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype="f16x2")
            net.load_state_dict(sd).to("cuda")
            a = net.raw_forward(x, flip_test=flip).clone()
            b = net.raw_forward(x, flip_test=flip).clone()
            assert torch.equal(a, b) and torch.isfinite(a).all()
            handle = net._compiled[(256, 192)][0]
            assert _lib.lib().udp_hrnet_lanes(handle, C.c_int(n)) == int(lanes)
            out[lanes] = a
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_LANES", None)
        else:
            os.environ["UDP_POSE_LANES"] = saved
    assert out["1"].shape == (n * (2 if flip else 1), 17, 64, 48)
    assert torch.equal(out["1"], out["2"])


@pytest.mark.parametrize("n", [3, 64])
def test_layer1_chained_convs_equal_separate_convs(w32_gaussian, n):
    """conv3 (+ shortcut + ReLU) of a layer1 Bottleneck and conv1 (+ ReLU) of the next one run as ONE launch in the
    split-fp16 mode (udp_conv_op.chain_cout, conv_chain_kernel: the second conv's K chunks are the first conv's
    accumulators, handed over in registers).  Every accumulator sees the MFMAs of the separate convs in the same order:
    the heat-maps are those of the separate launches, bit for bit -- a ragged pixel count (3 crops x 2 = 18432 pixels,
    not a multiple of the 128-pixel workgroup) and the bench batch."""
    sd, _ = w32_gaussian
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=83)).cuda().repeat((n + 7) // 8, 1, 1, 1)[:n].contiguous()
    x += 0.01 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(n + 1))
    out = {}
    saved = os.environ.get("UDP_POSE_NO_L1_CHAIN")
    try:
        for chain in (True, False):
            os.environ.pop("UDP_POSE_NO_L1_CHAIN", None)
            if not chain:
                os.environ["UDP_POSE_NO_L1_CHAIN"] = "1"
            net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype="f16x2")
            net.load_state_dict(sd).to("cuda")
            out[chain] = net.raw_forward(x, flip_test=True).clone()
            assert sum(1 for o in net._compiled[(256, 192)][2].ops_array() if o.chain_cout) == (3 if chain else 0)
            del net
    finally:
        os.environ.pop("UDP_POSE_NO_L1_CHAIN", None)
        if saved is not None:
            os.environ["UDP_POSE_NO_L1_CHAIN"] = saved
    assert torch.isfinite(out[True]).all() and out[True].abs().max() > 0
    assert torch.equal(out[True], out[False])


def test_create_rejects_malformed_chained_convs():
    """udp_hrnet_create checks a chained conv (udp_conv_op.chain_cout) where the program is built, not at the first
    forward: shape outside what conv_chain_kernel computes, a chained op inside a launch group, an aliased or missing
    chain buffer, weights outside the blob -- each refused with its own message; the untouched program is accepted."""
    import ctypes as C
    from udp_pose_amd import _lib, hrnet_plan
    extra = synth.scaled_extra(32, modules=(1, 1, 1), blocks=1)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=3)
    prog = hrnet_plan.HRNetProgram(sd, extra, 64, 64, "f16x2")
    blob = torch.from_numpy(prog.weight_blob()).cuda()
    bufs = (C.c_int64 * len(prog.buf_elems))(*prog.buf_elems)

    def create(mutate=None):
        ops = prog.ops_array()
        k = [i for i, o in enumerate(ops) if o.chain_cout][0]
        if mutate:
            mutate(ops[k])
        h = C.c_void_p()
        rc = _lib.lib().udp_hrnet_create(ops, len(ops), bufs, len(prog.buf_elems), _lib.ptr(blob), blob.numel(),
                                         _lib.DTYPES["f16x2"], 64, 64, prog.out_channels, C.byref(h))
        if rc == 0:
            _lib.lib().udp_hrnet_destroy(h)
        return rc, _lib.lib().udp_last_error().decode()

    assert create()[0] == 0
    for mutate, text in ((lambda o: setattr(o, "chain_cout", 32), "chained conv needs"),
                         (lambda o: setattr(o, "group", 7), "chained conv needs"),
                         (lambda o: setattr(o, "ks", 3), ""),
                         (lambda o: setattr(o, "chain_buf", o.out_buf), "chain_buf"),
                         (lambda o: setattr(o, "chain_buf", 10 ** 6), "chain_buf"),
                         (lambda o: setattr(o, "w2_off", blob.numel() - 64), "chained conv: weight"),
                         (lambda o: setattr(o, "chain_wexp", 99), "chained conv: weight")):
        rc, err = create(mutate)
        assert rc != 0 and text in err, (rc, err)


@pytest.mark.parametrize("knob,dtype", [("UDP_POSE_NO_L1_CONCAT", "f32"), ("UDP_POSE_NO_L1_CONCAT", "f16x2"),
                                        ("UDP_POSE_NO_FUSE_CONCAT", "f16x2")])
def test_convs_over_concatenated_channels_match_one_conv_per_term(w32_gaussian, knob, dtype):
    """Two planner rewrites sum convs by concatenating their inputs (weights side by side, biases added, ONE fp32
    accumulation): layer1.0's conv3 + projection shortcut, and the stride-2 convs that end the terms of an exchange-unit
    output.  Against the program with one conv per term (partial results rounded to storage in between) the heat-maps
    move by rounding noise only: <= 2e-5 of their scale, arg-max unchanged."""
    sd, _ = w32_gaussian
    x = torch.from_numpy(synth.synth_crops(6, 256, 192, seed=29)).cuda()
    out = {}
    saved = os.environ.get(knob)
    try:
        for per_term in (False, True):
            os.environ.pop(knob, None)
            if per_term:
                os.environ[knob] = "1"
            net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype=dtype)
            net.load_state_dict(sd).to("cuda")
            out[per_term] = net.raw_forward(x, flip_test=True).clone()
            n_ops = len(net._compiled[(256, 192)][2].ops_array())
            out[(per_term, "ops")] = n_ops
            del net
    finally:
        os.environ.pop(knob, None)
        if saved is not None:
            os.environ[knob] = saved
    assert out[(True, "ops")] > out[(False, "ops")]
    scale = float(out[True].abs().max())
    assert float((out[False] - out[True]).abs().max()) <= 2e-5 * scale
    assert torch.equal(out[False].flatten(2).argmax(2), out[True].flatten(2).argmax(2))


def test_w32_bf16_mode_accuracy(golden_dir, w32_gaussian):
    """bf16 storage (fp32 accumulate) is REDUCED PRECISION and not a parity mode: this is a sanity bound on what it
    does to the (noise-like) reference heat-maps, far outside the 1e-3 / arg-max contract that the fp32 and
    split-fp16 modes hold (test_w32_f16x2_matches_reference_heatmaps); bounds on trained maps:
    test_trained_peaked_maps_bf16_storage_bound."""
    sd, _ = w32_gaussian
    g = np.load(os.path.join(golden_dir, "hrnet_w32_gaussian.npz"))
    net = MODELS["pose_hrnet"](_cfg(synth.W32_EXTRA, 17, "gaussian"), is_train=False, dtype="bf16")
    net.load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(2, 256, 192, seed=5)).cuda()
    got = net(x).clone().cpu().numpy()
    ref = g["out"]
    err = np.abs(got - ref)
    agree = (got.reshape(2, 17, -1).argmax(2) == ref.reshape(2, 17, -1).argmax(2)).mean()
    print("w32 bf16: max abs err %.3g, rms err %.3g, ref std %.3g, arg-max agreement %.3f" %
          (err.max(), np.sqrt((err ** 2).mean()), ref.std(), agree))
    # bf16 storage through ~60 sequential layers: a few % rms error on these noise-like synthetic
    # heat-maps (no trained peak structure), so arg-max agreement is well below the fp32 mode's 100 %.
    assert np.sqrt((err ** 2).mean()) < 0.08 * ref.std()
    assert agree >= 0.7


def test_engine_infer_pose_matches_oracle_pipeline(golden_dir, w32_gaussian):
    from udp_pose_amd.config import default_config
    from udp_pose_amd.pose_engine import UdpPsaPoseHip
    sd, _ = w32_gaussian
    cfg = default_config()
    cfg.MODEL.EXTRA = synth.W32_EXTRA
    cfg.MODEL.IMAGE_SIZE = [192, 256]
    cfg.MODEL.HEATMAP_SIZE = [48, 64]
    cfg.DATASET.DATASET = "coco"
    cfg.TEST.POST_PROCESS = True
    eng = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg)
    frame = synth.synth_frame_u8(480, 640, seed=12)
    boxes = synth.synth_boxes(4, seed=6)
    boxes_before = boxes.copy()
    kp, mv = eng.infer_pose(frame, boxes)
    np.testing.assert_array_equal(boxes, boxes_before)             # caller's boxes untouched
    assert kp.shape == (4, 17, 2) and mv.shape == (4, 17, 1) and kp.dtype == np.float64
    crops, cs = odata.engine_preprocess(frame, boxes, [192, 256])
    hm = ohrnet.hrnet_forward(sd, synth.W32_EXTRA, torch.from_numpy(crops)).numpy()
    rp, rm, _, _ = odec.get_final_preds("gaussian", True, 4.0, hm.copy(), cs[:, :2], cs[:, 2:])
    np.testing.assert_allclose(mv, rm, rtol=0, atol=1e-3)
    err = np.abs(kp - rp).max(axis=2)
    good = _dark_shift(hm) < 1.5
    print("engine keypoint err px: median %.2g, max(well-conditioned) %.2g, max(all) %.2g"
          % (np.median(err), err[good].max(), err.max()))
    assert err[good].max() < 2e-2 and np.median(err) < 1e-3
    with pytest.raises(RuntimeError):
        eng.infer_pose(frame, np.zeros((0, 4), np.float32))        # N >= 1 like the reference


def test_w48_384x288_matches_reference_heatmaps(golden_dir):
    """Config 4: pose_hrnet_w48 384x288 (Cin = 48/96/192/384: ragged K chunks, 96x72 maps in two
    column tiles) vs the heat-maps the REFERENCE module produced; fp32 gate + bf16 report; decode of
    the 96x72 maps against the oracle."""
    g = np.load(os.path.join(golden_dir, "hrnet_w48_gaussian.npz"))
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_w48_gaussian.npz")))
    extra = synth.scaled_extra(48)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=2, bn_calib=calib)
    x = torch.from_numpy(synth.synth_crops(1, 384, 288, seed=6)).cuda()
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False).load_state_dict(sd).to("cuda")
    got = net(x).clone()
    err = np.abs(got.cpu().numpy() - g["out"]).max()
    print("w48 fp32 max abs heat-map error vs reference: %.3g (absmax %.3g)" % (err, np.abs(g["out"]).max()))
    np.testing.assert_allclose(got.cpu().numpy(), g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(got.cpu().numpy().reshape(17, -1).argmax(1), g["out"].reshape(17, -1).argmax(1))
    c, s = synth.synth_center_scale(1, seed=4)
    rp, rm, _, ridx = odec.get_final_preds("gaussian", True, 4.0, got.cpu().numpy().copy(), c, s)
    preds, maxvals, _, idx = decode_device(got, torch.from_numpy(c.astype(np.float64)),
                                           torch.from_numpy(s.astype(np.float64)), "gaussian", True, 4.0, True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(maxvals.cpu().numpy(), rm)
    np.testing.assert_allclose(preds.cpu().numpy(), rp, rtol=5e-3, atol=1e-3)
    # split-fp16 throughput mode: the same north-star gate as fp32
    hnet = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype="f16x2").load_state_dict(sd).to("cuda")
    hgot = hnet(x).clone().cpu().numpy()
    print("w48 f16x2 max abs heat-map error vs reference: %.3g" % np.abs(hgot - g["out"]).max())
    np.testing.assert_allclose(hgot, g["out"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(hgot.reshape(17, -1).argmax(1), g["out"].reshape(17, -1).argmax(1))
    bnet = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype="bf16").load_state_dict(sd).to("cuda")
    bgot = bnet(x).clone().cpu().numpy()
    rms = np.sqrt(((bgot - g["out"]) ** 2).mean())
    print("w48 bf16 rms err %.3g (ref std %.3g)" % (rms, g["out"].std()))
    assert rms < 0.2 * g["out"].std()      # report only: bf16 storage is NOT a parity mode (measured 12 % on these noise-like maps)


@pytest.mark.parametrize("och,tt", [(17, "gaussian"), (51, "offset")])
def test_rsn18_matches_reference_heatmaps(golden_dir, och, tt):
    """Config 5: RSN-18 forward (7x7 stem, max-pool, split/concat as channel views, bilinear
    align-corners top-down path) vs the REFERENCE module's output; then the UDP decode on it
    (offset head = the config-5 composition, pinned half by half: SURVEY 2 'Config 5 caveat')."""
    from udp_pose_amd.model import RSN18Hip
    g = np.load(os.path.join(golden_dir, "rsn18_%d.npz" % och))
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_rsn18_%d.npz" % och)))
    sd = synth.synth_rsn18_state_dict(och, seed=4, bn_calib=calib)
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8)).cuda()
    net = RSN18Hip(och).load_state_dict(sd).to("cuda")
    got = net(x).clone()
    err = np.abs(got.cpu().numpy() - g["out"]).max()
    # With these synthetic weights RSN-18 is ill-conditioned in fp32: the reference's own fp32 result
    # is ~9e-4 away from an fp64 evaluation of the same graph.  Gate: the HIP fp32 result must be as
    # close to the fp64 truth as the reference is (x2), and within 3e-3 of the reference itself.
    from oracle import rsn as orsn
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    truth = orsn.rsn_forward(sd64, x.cpu().double()).numpy()
    ref_noise = np.abs(g["out"] - truth).max()
    hip_noise = np.abs(got.cpu().numpy() - truth).max()
    print("rsn18 (%d ch) fp32: |hip - ref| %.3g, |ref - fp64| %.3g, |hip - fp64| %.3g (absmax %.3g)"
          % (och, err, ref_noise, hip_noise, np.abs(g["out"]).max()))
    assert hip_noise <= 2.0 * ref_noise + 1e-5
    np.testing.assert_allclose(got.cpu().numpy(), g["out"], rtol=0, atol=3e-3)
    c, s = synth.synth_center_scale(1, seed=4)
    rp, rm, _, ridx = odec.get_final_preds(tt, tt == "gaussian", 4.0, got.cpu().numpy().copy(), c, s)
    preds, maxvals, _, idx = decode_device(got, torch.from_numpy(c.astype(np.float64)),
                                           torch.from_numpy(s.astype(np.float64)), tt, tt == "gaussian", 4.0, True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(maxvals.cpu().numpy(), rm)
    np.testing.assert_allclose(preds.cpu().numpy(), rp, rtol=5e-3, atol=1e-3)
    # flip-test + batch: mirrored half == explicit mirrored forward, batch independence
    xb = torch.from_numpy(synth.synth_crops(5, 256, 192, seed=9)).cuda()
    raw = net.raw_forward(xb, flip_test=True).clone()
    mir = net.raw_forward(torch.flip(xb[:2], dims=[3]).contiguous()).clone()
    assert torch.equal(mir, raw[5:7])
    # split-fp16 throughput mode: as close to the fp64 truth as the reference's own fp32 evaluation (x2), like fp32
    hgot = RSN18Hip(och, dtype="f16x2").load_state_dict(sd).to("cuda")(x).clone().cpu().numpy()
    h2_noise = np.abs(hgot - truth).max()
    print("rsn18 (%d ch) f16x2: |hip - ref| %.3g, |hip - fp64| %.3g" % (och, np.abs(hgot - g["out"]).max(), h2_noise))
    assert h2_noise <= 2.0 * ref_noise + 1e-5
    np.testing.assert_allclose(hgot, g["out"], rtol=0, atol=3e-3)
    bnet = RSN18Hip(och, dtype="bf16").load_state_dict(sd).to("cuda")
    rms = np.sqrt(((bnet(x).clone().cpu().numpy() - g["out"]) ** 2).mean())
    print("rsn18 bf16 rms err %.3g (ref std %.3g)" % (rms, g["out"].std()))
    # Sanity only: this synthetic RSN amplifies rounding ~20x more than the synthetic HRNet (fp32 noise
    # 3e-4 vs 1.4e-5 against fp64), so bf16 storage lands near 50 % rms here; the fp32 mode is the parity mode.
    assert np.isfinite(rms) and rms < 0.8 * g["out"].std()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_batches_past_the_launch_limit_are_split(dtype):
    """A batch whose largest activation would exceed the 32-bit offsets of one launch is run in slices
    (here the limit is lowered to 2 images): same result, flip-test row order kept (all plain rows, then
    all mirrored rows)."""
    extra = synth.scaled_extra(32, modules=(1, 1, 1), blocks=1)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=4)
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(5, 64, 64, seed=8)).cuda()
    whole_flip = net.raw_forward(x, flip_test=True).clone()
    whole = net(x).clone()
    net.max_images_per_launch = 2
    torch.testing.assert_close(net.raw_forward(x, flip_test=True), whole_flip, rtol=0, atol=1e-6)
    torch.testing.assert_close(net(x), whole, rtol=0, atol=1e-6)


@pytest.mark.parametrize("h,w", [(256, 192), (128, 96), (64, 64), (32, 32)])
def test_fused_basic_block_equals_the_two_conv_launches(h, w, monkeypatch):
    """bf16: the fused BasicBlock kernel (32-channel branch: intermediate map and residual stay in LDS) against
    the same network run as separate conv launches.  Both round the intermediate map to bf16; the residual
    is added in a different fp32 order, so outputs agree to bf16 rounding of the activations."""
    extra = synth.scaled_extra(32, modules=(1, 2, 1), blocks=2)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=12)
    x = torch.from_numpy(synth.synth_crops(3, h, w, seed=13))
    ohrnet.hrnet_forward(sd, extra, x, calibrate=True)
    outs = {}
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("UDP_POSE_NO_BLOCK_FUSION", raising=False)
        else:
            monkeypatch.setenv("UDP_POSE_NO_BLOCK_FUSION", "1")
        net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype="bf16").load_state_dict(sd).to("cuda")
        kinds = [d[1] for d in net.program(h, w).describe()]
        assert (kinds.count(10) > 0) == fused
        outs[fused] = net.raw_forward(x.cuda(), flip_test=True).clone().float().cpu().numpy()
    ref = ohrnet.hrnet_forward(sd, extra, torch.cat([x, torch.flip(x, dims=[3])])).numpy()
    d = outs[True] - outs[False]
    assert np.sqrt((d ** 2).mean()) < 1.5e-2 * ref.std(), (np.sqrt((d ** 2).mean()), ref.std())
    # and the fused path is as close to the fp32 oracle as the unfused one
    e_f = np.sqrt(((outs[True] - ref) ** 2).mean())
    e_u = np.sqrt(((outs[False] - ref) ** 2).mean())
    assert e_f < 1.15 * e_u + 1e-4, (e_f, e_u)


@pytest.mark.parametrize("dtype", ["bf16", "f16x2", "f16x2-ws"])
def test_merged_branch_launches_equal_separate_launches(monkeypatch, dtype):
    """bf16 graph mode: the same-depth convs of different branches run as ONE conv_mfma_multi launch
    (hrnet.hip build_graph).  Per output element the accumulation order does not depend on the tile
    choice, so the result equals the ungrouped program bit for bit; eager mode (per-op launches) too."""
    extra = synth.scaled_extra(32, modules=(1, 2, 2), blocks=2)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=14)
    x = torch.from_numpy(synth.synth_crops(5, 128, 96, seed=15))
    ohrnet.hrnet_forward(sd, extra, x, calibrate=True)
    outs = {}
    monkeypatch.setenv("UDP_POSE_WS", "1" if dtype.endswith("-ws") else "0")     # weight-stationary kernel family
    dtype = dtype.split("-")[0]
    for mode in ("grouped", "eager", "plain"):
        if mode == "plain":
            monkeypatch.setenv("UDP_POSE_NO_GROUPS", "1")
        else:
            monkeypatch.delenv("UDP_POSE_NO_GROUPS", raising=False)
        net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
        net.use_graph = mode != "eager"
        groups = [o.group for o in net.program(128, 96).ops_array()]
        assert (max(groups) > 0) == (mode != "plain")
        outs[mode] = net.raw_forward(x.cuda(), flip_test=True).clone()
        outs[mode + "2"] = net.raw_forward(x.cuda(), flip_test=True).clone()        # graph replay
    torch.testing.assert_close(outs["grouped"], outs["plain"], rtol=0, atol=0)
    torch.testing.assert_close(outs["grouped2"], outs["plain"], rtol=0, atol=0)
    torch.testing.assert_close(outs["eager"], outs["plain"], rtol=0, atol=0)


@pytest.mark.parametrize("dtype", ["bf16", "f16x2", "f32"])
def test_each_image_is_independent_of_its_batch(dtype):
    """Size-independent property: an image's heat-maps do not depend on which batch it is in (ragged tiles,
    several-images-per-tile kernels, merged launches, fused blocks, flip-test row order): batch of 5 vs the
    same images alone and in a batch of 2 -- bit-identical."""
    extra = synth.scaled_extra(32, modules=(1, 1, 2), blocks=2)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=21)
    x = torch.from_numpy(synth.synth_crops(5, 128, 96, seed=22))
    ohrnet.hrnet_forward(sd, extra, x, calibrate=True)
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    xd = x.cuda()
    whole = net.raw_forward(xd, flip_test=True).clone()
    for i in range(5):
        one = net.raw_forward(xd[i:i + 1].contiguous(), flip_test=True).clone()
        torch.testing.assert_close(one[0], whole[i], rtol=0, atol=0)
        torch.testing.assert_close(one[1], whole[5 + i], rtol=0, atol=0)
    two = net.raw_forward(xd[3:5].contiguous(), flip_test=False).clone()
    torch.testing.assert_close(two, whole[3:5], rtol=0, atol=0)


def _peaked(golden_dir):
    g = np.load(os.path.join(golden_dir, "hrnet_peaked.npz"))
    extra = synth.scaled_extra(16, modules=(1, 1, 1), blocks=1)
    sd = {k[3:]: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("sd/")}
    return g, extra, sd


def _peaked_pipeline(g, extra, sd, dtype):
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.normalize_u8(g["crops_u8"])).cuda()
    n = x.shape[0]
    raw = net.raw_forward(x, flip_test=True)
    hm = flip_fuse(raw[:n], raw[n:], COCO_FLIP_PAIRS, False)
    preds, maxvals, _, idx = decode_device(hm, torch.from_numpy(g["center"].astype(np.float64)),
                                           torch.from_numpy(g["scale"].astype(np.float64)), "gaussian", True, 4.0,
                                           cs_is_f32=g["center"].dtype == np.float32, want_idx=True)
    return raw.cpu().numpy(), hm.cpu().numpy(), preds.cpu().numpy(), maxvals.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_trained_peaked_maps_end_to_end_keypoints_all_joints(golden_dir, dtype):
    """The whole hot path (forward + mirrored forward + flip fuse + DARK decode) on TRAINED, peaked heat-maps against
    what the REFERENCE module + reference get_final_preds produced (tests/golden/hrnet_peaked.npz): north-star
    tolerances on EVERY joint -- heat-maps 1e-3, arg-max identical, keypoints 1e-3 px in image space -- for the
    fp32 mode and for the split-fp16 throughput mode.  (On the random-weight fixtures DARK's Hessian is
    ill-conditioned for many joints; here it is not, so no joint is excluded.)"""
    g, extra, sd = _peaked(golden_dir)
    raw, hm, preds, maxvals, idx = _peaked_pipeline(g, extra, sd, dtype)
    n = g["out"].shape[0]
    np.testing.assert_allclose(raw[:n], g["out"], rtol=0, atol=1e-3)
    np.testing.assert_allclose(raw[n:], g["out_flip"], rtol=0, atol=1e-3)
    np.testing.assert_allclose(hm, g["fused"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(idx, g["fused"].reshape(n, 17, -1).argmax(2))
    np.testing.assert_allclose(maxvals, g["maxvals"], rtol=0, atol=1e-3)
    err = np.abs(preds - g["preds"]).max()
    print("%s peaked end-to-end: heat-map max err %.3g, keypoint max err %.3g px (all %d joints)"
          % (dtype, np.abs(hm - g["fused"]).max(), err, preds.shape[0] * preds.shape[1]))
    np.testing.assert_allclose(preds, g["preds"], rtol=0, atol=1e-3)


def test_trained_peaked_maps_bf16_storage_bound(golden_dir):
    """What bf16 storage (reduced precision, NOT the parity mode) does to trained, peaked heat-maps: stated bounds,
    far looser than the contract -- heat-maps within 0.02 (peaks are ~0.4..1.3; measured 5.4e-3), arg-max
    identical for >= 90 % of the joints and identical or adjacent for >= 95 % (measured 94 % / 98.5 %), keypoints
    within 0.05 heat-map pixels at the 95th percentile (measured 0.01; a joint whose arg-max flips between two
    near-equal peaks moves by pixels -- the maximum is reported, not gated)."""
    g, extra, sd = _peaked(golden_dir)
    raw, hm, preds, maxvals, idx = _peaked_pipeline(g, extra, sd, "bf16")
    n = hm.shape[0]
    ref_idx = g["fused"].reshape(n, 17, -1).argmax(2)
    w = hm.shape[3]
    d = np.maximum(np.abs(idx % w - ref_idx % w), np.abs(idx // w - ref_idx // w))
    px = np.abs(preds - g["preds"]).max(axis=2) / (g["scale"][:, :1] * 200.0 / (w - 1))      # in heat-map pixels
    print("bf16 peaked: heat-map max err %.3g, arg-max equal %.3f / adjacent %.3f, keypoint err (heat-map px) median %.3g p95 %.3g max %.3g"
          % (np.abs(hm - g["fused"]).max(), (d == 0).mean(), (d <= 1).mean(), np.median(px), np.percentile(px, 95), px.max()))
    assert np.abs(hm - g["fused"]).max() < 0.02
    assert (d == 0).mean() >= 0.9 and (d <= 1).mean() >= 0.95
    assert np.percentile(px, 95) < 0.05


def test_engine_buckets_the_box_count_and_bounds_its_caches(golden_dir, w32_gaussian):
    """a frame's box count changes every call.  The engine runs the network at a bucketed batch size
    (1, 2, 4, 8, multiples of 8; padding rows repeat the last box and are dropped), so three boxes give exactly
    the keypoints of the same three boxes inside a call with five; the model keeps at most MAX_IO_SHAPES buffer
    sets (least recently used evicted) and the library at most 8 graphs, however many distinct counts arrive."""
    from udp_pose_amd.config import default_config
    from udp_pose_amd.pose_engine import UdpPsaPoseHip
    sd, _ = w32_gaussian
    cfg = default_config()
    cfg.MODEL.EXTRA = synth.W32_EXTRA
    cfg.MODEL.IMAGE_SIZE = [192, 256]
    cfg.MODEL.HEATMAP_SIZE = [48, 64]
    cfg.DATASET.DATASET = "coco"
    cfg.TEST.POST_PROCESS = True
    eng = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg)
    assert [eng._bucket(n) for n in (1, 2, 3, 4, 5, 8, 9, 16, 17)] == [1, 2, 4, 4, 8, 8, 16, 16, 24]
    frame = synth.synth_frame_u8(480, 640, seed=12)
    boxes = synth.synth_boxes(5, seed=6)
    kp5, mv5 = eng.infer_pose(frame, boxes)
    kp3, mv3 = eng.infer_pose(frame, boxes[:3])
    np.testing.assert_array_equal(kp3, kp5[:3])
    np.testing.assert_array_equal(mv3, mv5[:3])
    kpf, _ = eng.infer_pose(frame, boxes[:3], flip_test=True)
    assert kpf.shape == (3, 17, 2) and np.isfinite(kpf).all()
    for n in (1, 2, 9, 17, 25, 33, 41, 49, 57, 65):        # ten more buckets than the caches hold
        kp, _ = eng.infer_pose(frame, synth.synth_boxes(n, seed=n))
        assert kp.shape == (n, 17, 2) and np.isfinite(kp).all()
    assert len(eng.model._io) <= eng.model.MAX_IO_SHAPES
    kp3b, _ = eng.infer_pose(frame, boxes[:3])               # evicted and rebuilt: same answer
    np.testing.assert_array_equal(kp3b, kp3)


def test_engine_reruns_a_batch_that_leaves_fp16_range_in_fp32(golden_dir):
    """the engine's default storage is split fp16 (|x| >= 65520 -> NaN).  Finiteness is checked
    on the whole heat-map tensor on the device and such a batch is re-run with the same weights in fp32 (the
    reference engine's precision): the result equals an fp32 engine's, bit for bit, and the retry is counted."""
    from udp_pose_amd.config import default_config
    from udp_pose_amd.pose_engine import UdpPsaPoseHip
    sd = dict(_w32(golden_dir, "gaussian"))
    for k in ("bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias"):      # stem activations ~1e3, then ~1e6
        sd[k] = sd[k] * 1.0e3
    cfg = default_config()
    cfg.MODEL.EXTRA = synth.W32_EXTRA
    cfg.MODEL.IMAGE_SIZE = [192, 256]
    cfg.MODEL.HEATMAP_SIZE = [48, 64]
    cfg.DATASET.DATASET = "coco"
    cfg.TEST.POST_PROCESS = True
    frame = synth.synth_frame_u8(480, 640, seed=12)
    boxes = synth.synth_boxes(3, seed=6)
    eng = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg)
    assert eng.model.dtype == "f16x2"
    kp, mv = eng.infer_pose(frame, boxes)
    assert eng.fp32_retries == 1 and np.isfinite(kp).all() and np.isfinite(mv).all()
    ref = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg, dtype="f32")
    kp32, mv32 = ref.infer_pose(frame, boxes)
    assert ref.fp32_retries == 0
    np.testing.assert_array_equal(kp, kp32)
    np.testing.assert_array_equal(mv, mv32)
    kpf, _ = eng.infer_pose(frame, boxes, flip_test=True)
    kpf32, _ = ref.infer_pose(frame, boxes, flip_test=True)
    np.testing.assert_array_equal(kpf, kpf32)


def test_engine_ignores_a_stale_range_flag(w32_gaussian):
    """ADVICE (medium): the split-fp16 range flag is one per process.  A flag left behind by anything before the
    engine's own forward (here a direct op call that stores 65520) must not cost an ordinary frame the fp32 re-run:
    no retry is counted and the result equals a fresh engine's, bit for bit."""
    import ctypes as C
    from udp_pose_amd import _lib, f16x2
    from udp_pose_amd.config import default_config
    from udp_pose_amd.pose_engine import UdpPsaPoseHip
    sd, _ = w32_gaussian
    cfg = default_config()
    cfg.MODEL.EXTRA = synth.W32_EXTRA
    cfg.MODEL.IMAGE_SIZE = [192, 256]
    cfg.MODEL.HEATMAP_SIZE = [48, 64]
    cfg.DATASET.DATASET = "coco"
    cfg.TEST.POST_PROCESS = True
    frame = synth.synth_frame_u8(480, 640, seed=12)
    boxes = synth.synth_boxes(3, seed=6)
    fresh = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg)
    _lib.f16x2_overflow(reset=True)
    kp0, mv0 = fresh.infer_pose(frame, boxes)
    assert fresh.fp32_retries == 0

    def raise_flag():                                               # 1x1 conv, zero weights, bias 65520 -> every output leaves the range
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 1, 1, 0
        op.cin, op.cout, op.cout_pad = 32, 32, 32
        op.hin, op.win, op.hout, op.wout = 2, 2, 2, 2
        x = f16x2.encode(torch.zeros(1, 2, 2, 32)).cuda()
        w = f16x2.encode(torch.zeros(1, 32, 32)).cuda()
        b = torch.full((32,), 65520.0).cuda()
        out = f16x2.encode(torch.zeros(1, 2, 2, 32)).cuda()
        _lib.check(_lib.lib().udp_conv2d_fused(C.byref(op), _lib.DTYPES["f16x2"], 1, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), None, None, None,
                                               None, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
    eng = UdpPsaPoseHip("synthetic", None, "cuda", state_dict=sd, config=cfg)
    for flip in (False, True):
        raise_flag()
        assert _lib.f16x2_overflow(reset=False), "the direct op call did not raise the flag: the test would be vacuous"
        kp, mv = eng.infer_pose(frame, boxes, flip_test=flip)
        assert eng.fp32_retries == 0, "a stale flag cost an ordinary frame the fp32 re-run"
        assert not _lib.f16x2_overflow(reset=True)
        if not flip:
            np.testing.assert_array_equal(kp, kp0)
            np.testing.assert_array_equal(mv, mv0)
    kpf, mvf = fresh.infer_pose(frame, boxes, flip_test=True)
    np.testing.assert_array_equal(kp, kpf)
    np.testing.assert_array_equal(mv, mvf)


def _batch_properties(net, x, n_img_check):
    """Size-independent properties at a config's own batch: graph replay == eager launches, identical crops ->
    identical maps, an image's maps do not depend on the batch it rides in, the in-kernel mirrored half == an
    explicit forward of mirrored inputs -- all bit for bit."""
    n = x.shape[0]
    raw = net.raw_forward(x, flip_test=True).clone()
    assert raw.shape[0] == 2 * n and torch.isfinite(raw).all()
    assert torch.equal(raw, net.raw_forward(x, flip_test=True).clone())      # second call = graph replay
    net.use_graph = False
    eager = net.raw_forward(x, flip_test=True).clone()
    net.use_graph = True
    assert torch.equal(raw, eager)
    assert torch.equal(raw[0], raw[4])                                        # x[4] is a copy of x[0]
    k = n_img_check
    one = net.raw_forward(x[k:k + 1].contiguous()).clone()
    assert torch.equal(one[0], raw[k])
    mirrored = net.raw_forward(torch.flip(x[:2], dims=[3]).contiguous()).clone()
    assert torch.equal(mirrored, raw[n:n + 2])


@pytest.mark.parametrize("dtype", ["f16x2"])
def test_w48_batch32_properties(golden_dir, dtype):
    """Config 4 at its own size (pose_hrnet_w48 384x288, N = 32, flip test on -> 64 images per launch sequence)
    in the mode bench.py times it in."""
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_w48_gaussian.npz")))
    extra = synth.scaled_extra(48)
    sd = synth.synth_state_dict(extra, 17, "gaussian", seed=2, bn_calib=calib)
    net = MODELS["pose_hrnet"](_cfg(extra, 17, "gaussian"), is_train=False, dtype=dtype).load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(4, 384, 288, seed=6)).cuda().repeat(8, 1, 1, 1)      # N = 32
    x[20:] += 0.01 * torch.randn(12, 3, 384, 288, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    _batch_properties(net, x, 21)


@pytest.mark.parametrize("dtype", ["f16x2"])
def test_rsn18_offset_batch64_properties(golden_dir, dtype):
    """Config 5 at its own size (RSN-18 256x192 with the 51-channel offset head, N = 64, flip test on) in the mode
    bench.py times it in, then the offset decode on the fused maps against the oracle decode of the same maps."""
    from udp_pose_amd.model import RSN18Hip
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_rsn18_51.npz")))
    sd = synth.synth_rsn18_state_dict(51, seed=4, bn_calib=calib)
    net = RSN18Hip(51, dtype=dtype).load_state_dict(sd).to("cuda")
    x = torch.from_numpy(synth.synth_crops(4, 256, 192, seed=8)).cuda().repeat(16, 1, 1, 1)     # N = 64
    x[40:] += 0.01 * torch.randn(24, 3, 256, 192, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    _batch_properties(net, x, 41)
    raw = net.raw_forward(x, flip_test=True)
    hm = flip_fuse(raw[:64], raw[64:], COCO_FLIP_PAIRS, True)
    c, s = synth.synth_center_scale(64, seed=4)
    rp, rm, _, ridx = odec.get_final_preds("offset", False, 4.0, hm.cpu().numpy().copy(), c, s)
    preds, maxvals, _, idx = decode_device(hm, torch.from_numpy(c.astype(np.float64)),
                                           torch.from_numpy(s.astype(np.float64)), "offset", False, 4.0, True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_allclose(preds.cpu().numpy(), rp, rtol=0, atol=1e-3)


def test_rsn18_sums_in_conv_epilogues_equal_separate_sums(golden_dir):
    """RSN-18 in split fp16: the six element-wise sums between the 3x3 convs of every bottleneck
    (RSN/exps/RSN18.coco/network.py:102-114) ride in the epilogue of the conv that produces their second operand
    (udp_conv_op.n_out2: second outputs = the output AS STORED + an addend slice; three convs per bottleneck store only
    the sums).  Heat-maps of the 51-channel head at N = 24 with the flip test equal those of the program with separate
    UDP_OP_FUSE launches (UDP_POSE_RSN_FUSE_ADDS=0), bit for bit; the fused program has 48 launches fewer."""
    from udp_pose_amd.model import RSN18Hip
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_rsn18_51.npz")))
    sd = synth.synth_rsn18_state_dict(51, seed=4, bn_calib=calib)
    x = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=12)).cuda().repeat(3, 1, 1, 1)
    x[8:] += 0.01 * torch.randn(16, 3, 256, 192, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    out, nops = {}, {}
    saved = os.environ.get("UDP_POSE_RSN_FUSE_ADDS")
    try:
        for fuse in ("0", "1"):
            os.environ["UDP_POSE_RSN_FUSE_ADDS"] = fuse
            net = RSN18Hip(51, dtype="f16x2").load_state_dict(sd).to("cuda")
            out[fuse] = net.raw_forward(x, flip_test=True).clone()
            nops[fuse] = len(net.program(256, 192).ops_array())
            del net
    finally:
        if saved is None:
            os.environ.pop("UDP_POSE_RSN_FUSE_ADDS", None)
        else:
            os.environ["UDP_POSE_RSN_FUSE_ADDS"] = saved
    assert torch.isfinite(out["1"]).all() and nops["0"] - nops["1"] == 48
    assert torch.equal(out["0"], out["1"])
