"""GPU tests of pose_hrnet_psa training: the udp_psa_train_* kernels (csrc/psa_train.hip) against torch.autograd over
the CPU oracle's PSA_s (oracle/hrnet.py::_psa_s), and HRNetTrainer(psa=True) against oracle/train.py.

Yardstick everywhere: the fp64 evaluation is the truth, the same evaluation in fp32 on the CPU shows what fp32
arithmetic costs; the HIP path may be 3x that far off (the convention of tests/test_gpu_train.py) plus a floor."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hrnet as ohrnet, train as o_train       # noqa: E402
from udp_pose_amd import _lib, synth                       # noqa: E402
from udp_pose_amd.train import HRNetTrainer                # noqa: E402
from test_train_oracle_cpu import make_batch               # noqa: E402

EXTRA = synth.scaled_extra(32, modules=(1, 2, 1), blocks=2)
ULP = 2.0 ** -23


def _cfg(tt):
    return {"MODEL": {"EXTRA": EXTRA, "NUM_JOINTS": 5, "TARGET_TYPE": tt}}


def _rup(x, m):
    return (x + m - 1) // m * m


def _psa_weights(c, seed):
    """One PSA_s block's tensors at the scale synth.synth_state_dict(psa=True) gives them."""
    shapes = OrderedDict()
    synth._psa_s(shapes, "a", c)
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = OrderedDict()
    for k, s in shapes.items():
        if len(s) == 4:
            a = rng.standard_normal(s) * np.sqrt(2.0 / s[1])
        elif k.endswith("conv_up.1.weight"):
            a = rng.uniform(0.6, 1.2, s)
        else:
            a = rng.standard_normal(s) * 0.05
        sd[k] = torch.from_numpy(a.astype(np.float32))
    return sd


def _autograd(sd, x, dy, dtype):
    sd = OrderedDict((k, v.to(dtype).clone().requires_grad_(True)) for k, v in sd.items())
    xr = x.to(dtype).clone().requires_grad_(True)
    y = ohrnet._psa_s(ohrnet._Net(sd), xr, "a")
    gs = torch.autograd.grad((y * dy.to(dtype)).sum(), [xr] + list(sd.values()))
    out = OrderedDict(y=y.detach(), dx=gs[0])
    for k, g in zip(sd, gs[1:]):
        out[k] = g
    return out


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("c,h,w,n", [(32, 64, 48, 3), (64, 32, 24, 3), (128, 16, 12, 5), (256, 8, 6, 3)])
def test_psa_block_forward_and_backward_match_autograd(c, h, w, n):
    """One PSA_s block through the C ABI on the four W32 branch shapes at 256x192 (odd batches): output, dx and
    all ten parameter gradients against fp64 autograd; per tensor err_hip <= 3 * err_cpu_fp32 + 4 ulp of the
    tensor's max (max-abs error relative to the tensor's max)."""
    L = _lib.lib()
    sd = _psa_weights(c, 100 + c)
    g = torch.Generator().manual_seed(c + h)
    x = torch.relu(torch.randn(n, c, h, w, generator=g) + 0.3)          # the block sits behind relu(bn1(.))
    dy = torch.randn(n, c, h, w, generator=g)
    r64, r32 = _autograd(sd, x, dy, torch.float64), _autograd(sd, x, dy, torch.float32)

    dev = {k: v.reshape(-1).cuda() for k, v in sd.items()}
    grads = {k: torch.full_like(v, 7.0) for k, v in dev.items()}
    nfl = L.udp_psa_train_save_floats(n, h, w, c)
    assert nfl > 0
    save = torch.full((nfl,), float("nan"), device="cuda")
    xd, dyd = _nhwc(x), _nhwc(dy)
    x1, x2, dx, dx1 = (torch.full_like(xd, float("nan")) for _ in range(4))
    c2 = c // 2
    theta = torch.full((n, h, w, c2), float("nan"), device="cuda")
    dtheta = torch.full_like(theta, float("nan"))
    a = _lib.PsaTrainArgs()
    for i, k in enumerate(_lib.PSA_TRAIN_KEYS):
        a.w[i], a.dw[i] = dev["a" + k].data_ptr(), grads["a" + k].data_ptr()
    a.save, a.save_floats = save.data_ptr(), nfl
    a.n, a.h, a.w_px, a.c = n, h, w, c
    a.x, a.x1, a.theta, a.x2 = xd.data_ptr(), x1.data_ptr(), theta.data_ptr(), x2.data_ptr()
    a.dx2, a.dtheta, a.dx1, a.dx = dyd.data_ptr(), dtheta.data_ptr(), dx1.data_ptr(), dx.data_ptr()
    st = _lib.stream_ptr()
    # theta = conv_v_left(x1): the project's conv kernels, forward / weight gradient / input gradient
    wt = sd["a.conv_v_left.weight"].cuda().contiguous()
    wf = torch.empty(_rup(c2, 32) * c, device="cuda")
    wd = torch.empty(_rup(c, 32) * c2, device="cuda")
    _lib.check(L.udp_pack_conv_weights(wt.data_ptr(), c2, c, 1, _lib.UDP_F32, wf.data_ptr(), wd.data_ptr(), st))

    def conv_op(cin, cout):
        op = _lib.ConvOp()
        op.kind, op.ks, op.stride, op.relu = _lib.UDP_OP_CONV, 1, 1, 0
        op.cin, op.cout, op.cout_pad = cin, cout, _rup(cout, 32)
        op.hin, op.win, op.hout, op.wout = h, w, h, w
        op.in_buf = op.res_buf = _lib.UDP_BUF_NONE
        return op
    zeros = torch.zeros(_rup(c, 32), device="cuda")
    _lib.check(L.udp_psa_train_fwd_pool(C.byref(a), _lib.UDP_F32, st))
    _lib.check(L.udp_conv2d_fused(C.byref(conv_op(c, c2)), _lib.UDP_F32, n, x1.data_ptr(), wf.data_ptr(), zeros.data_ptr(),
                                  None, None, None, None, theta.data_ptr(), st))
    _lib.check(L.udp_psa_train_fwd_sp(C.byref(a), _lib.UDP_F32, st))
    _lib.check(L.udp_psa_train_bwd_sp(C.byref(a), _lib.UDP_F32, st))
    dwt = torch.full((c2, c, 1, 1), 7.0, device="cuda")
    ws = torch.empty(L.udp_conv2d_wgrad_workspace_bytes(c2, c, 1), dtype=torch.uint8, device="cuda")
    _lib.check(L.udp_conv2d_wgrad(x1.data_ptr(), dtheta.data_ptr(), n, h, w, c, h, w, c2, 1, 1, c2, c, _lib.UDP_F32,
                                  dwt.data_ptr(), 0, ws.data_ptr(), ws.numel(), st))
    _lib.check(L.udp_conv2d_fused(C.byref(conv_op(c2, c)), _lib.UDP_F32, n, dtheta.data_ptr(), wd.data_ptr(),
                                  zeros.data_ptr(), dx1.data_ptr(), None, None, None, dx1.data_ptr(), st))
    _lib.check(L.udp_psa_train_bwd_pool(C.byref(a), _lib.UDP_F32, st))
    _lib.check(L.udp_psa_train_bwd_params(C.byref(a), _lib.UDP_F32, st))
    torch.cuda.synchronize()

    got = OrderedDict(y=_nchw(x2), dx=_nchw(dx))
    for k in sd:
        got[k] = (dwt if k.endswith("conv_v_left.weight") else grads[k]).cpu().reshape(sd[k].shape)
    assert len(got) == 12
    fails = []
    for k, v in got.items():
        ex = r64[k].numpy()
        mx = np.abs(ex).max()
        assert mx > 0, "%s: the fp64 gradient is zero, the gate would be vacuous" % k
        e_hip = np.abs(v.numpy().astype(np.float64) - ex).max() / mx
        e_cpu = np.abs(r32[k].numpy().astype(np.float64) - ex).max() / mx
        print("C=%d %-28s err hip %.3g  cpu fp32 %.3g" % (c, k, e_hip, e_cpu))
        if not e_hip <= 3 * e_cpu + 4 * ULP:
            fails.append((k, e_hip, e_cpu))
    assert not fails, fails


def _oracle(sd0, x, tg, tw, tt, dtype):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in sd0.items()}
    parts, y, grads = o_train.loss_and_grads(sd, EXTRA, x.to(dtype), tg.to(dtype), tw.to(dtype), tt)
    return parts, y, grads, sd


@pytest.mark.parametrize("tt", ["gaussian", "offset"])
def test_psa_net_train_step_matches_oracle(tt):
    """HRNetTrainer(psa=True), one train_step on the width-32 PSA mini net: loss, heat-maps, every gradient (fp64
    oracle as truth, the fp32 oracle as yardstick), running statistics, then the trained weights through the
    inference model."""
    sd0 = synth.synth_state_dict(EXTRA, 5, tt, seed=1, psa=True)
    x, tg, tw = make_batch(tt, seed=11)
    parts64, _, g64, _ = _oracle(sd0, x, tg, tw, tt, torch.float64)
    parts32, y32, g32, sd32 = _oracle(sd0, x, tg, tw, tt, torch.float32)
    tr = HRNetTrainer(_cfg(tt), sd0, device="cuda", lr=1e-3, psa=True)
    loss = tr.train_step(x.cuda(), tg.cuda(), tw.cuda()).cpu().numpy()
    np.testing.assert_allclose(loss[:len(parts32)], np.array(parts32), rtol=1e-5)
    np.testing.assert_allclose(tr._out.buf.cpu().numpy(), y32.numpy(), atol=1e-3)
    assert tr._keys == list(g64.keys())
    e_hip, e_o32 = [], []
    for k in tr._keys:
        ex = g64[k].numpy()
        mx = np.abs(ex).max()
        assert mx > 0, k
        e_hip.append(np.abs(tr.grad_of(k).cpu().numpy() - ex).max() / mx)
        e_o32.append(np.abs(g32[k].numpy() - ex).max() / mx)
    e_hip, e_o32 = np.array(e_hip), np.array(e_o32)
    att = np.array([".deattn." in k for k in tr._keys])
    print("%s: all tensors median hip %.3g / o32 %.3g, q90 %.3g / %.3g, max %.3g / %.3g; deattn max %.3g / %.3g" % (
        tt, np.median(e_hip), np.median(e_o32), np.quantile(e_hip, 0.9), np.quantile(e_o32, 0.9), e_hip.max(), e_o32.max(),
        e_hip[att].max(), e_o32[att].max()))
    assert att.sum() == 240
    assert np.median(e_hip) <= 3 * np.median(e_o32) + 1e-5, (np.median(e_hip), np.median(e_o32))
    assert np.quantile(e_hip, 0.9) <= 3 * np.quantile(e_o32, 0.9) + 1e-3, (np.quantile(e_hip, 0.9), np.quantile(e_o32, 0.9))
    assert e_hip[att].max() <= 3 * e_o32[att].max() + 1e-3, (e_hip[att].max(), e_o32[att].max())
    sd1 = tr.state_dict()
    for k in sd32:
        if k.endswith("running_mean") or k.endswith("running_var"):
            np.testing.assert_allclose(sd1[k].numpy(), sd32[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    assert torch.isfinite(tr.flat).all() and tr.step_count == 1
    # round trip: the trained weights load into the inference model; eval heat-maps equal the oracle's
    from udp_pose_amd.model import MODELS
    net = MODELS["pose_hrnet_psa"](_cfg(tt), is_train=False).load_state_dict(sd1).to("cuda")
    got = net(x.cuda()).clone().cpu().numpy()
    ref = ohrnet.hrnet_forward(dict(sd1), EXTRA, x).numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3 * max(1.0, np.abs(ref).max()))


def test_psa_train_step_is_deterministic_and_graph_replay_equals_eager():
    """Two eager steps from the same start: bit-identical gradients.  train_step_graphed (eager, capture, replays)
    against train_step over eight steps on changing batches: parameters bit for bit."""
    sd0 = synth.synth_state_dict(EXTRA, 5, "gaussian", seed=3, psa=True)
    batches = [make_batch("gaussian", n=6, seed=50 + k) for k in range(4)]
    dev = [(x.cuda(), tg.cuda(), tw.cuda()) for x, tg, tw in batches]
    grads = []
    for _ in range(2):
        tr = HRNetTrainer(_cfg("gaussian"), {k: v.clone() for k, v in sd0.items()}, device="cuda", lr=1e-3, psa=True)
        tr.train_step(*dev[0])
        grads.append(tr.grad.clone())
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0], grads[1])
    outs = []
    for graphed in (False, True):
        tr = HRNetTrainer(_cfg("gaussian"), {k: v.clone() for k, v in sd0.items()}, device="cuda", lr=1e-3, psa=True)
        losses = []
        for x, tg, tw in dev + dev:
            loss = tr.train_step_graphed(x, tg, tw) if graphed else tr.train_step(x, tg, tw)
            losses.append(loss.clone())
        outs.append((np.array([l.cpu().numpy() for l in losses]), tr.flat.cpu().numpy().copy(), tr.step_count))
    assert outs[0][2] == outs[1][2] == 8
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-12)       # the loss VALUE is summed with fp64 atomics
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def _switch_gap(psa):
    """Largest per-tensor gradient difference (relative to the tensor's max) between the per-branch path (_basic)
    and the lock-step path (_blocks_lockstep) of one backward."""
    sd0 = synth.synth_state_dict(EXTRA, 5, "gaussian", seed=4, psa=psa)
    x, tg, tw = make_batch("gaussian", seed=21)
    g = {}
    for multi in (False, True):
        tr = HRNetTrainer(_cfg("gaussian"), sd0, device="cuda", psa=psa)
        tr.bn_multi = multi
        heat = tr.forward(x.cuda())
        _, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
        tr.backward(d)
        g[multi] = {k: tr.grad_of(k).cpu().double() for k in tr._keys}
    return max(float((g[True][k] - g[False][k]).abs().max() / (g[True][k].abs().max() + 1e-300)) for k in g[True])


def test_psa_lockstep_blocks_equal_per_branch_blocks():
    """bn_multi off (_basic) and on (_blocks_lockstep) run the same attention launches: the gradients differ by no
    more than the plain net's do under the same switch (factor 3, the project's convention; 0 stays 0)."""
    plain, psa = _switch_gap(False), _switch_gap(True)
    print("lock-step vs per-branch gradient gap: plain %.3g, psa %.3g" % (plain, psa))
    assert psa <= 3 * plain, (psa, plain)


def test_psa_training_learns_one_batch():
    """Twelve steps on one fixed batch: the loss falls.  The CPU oracle with oracle.train.Adam (fp32) on the same
    net and batch goes from 2.4797 to 0.08446 over the twelve steps (x 0.0341, measured once on the CPU); the gate
    is that factor with the project's margin of three, 0.1 -- far inside the 0.7 the plain net's test uses."""
    sd0 = synth.synth_state_dict(EXTRA, 5, "gaussian", seed=1, psa=True)
    x, tg, tw = make_batch("gaussian", seed=11)
    tr = HRNetTrainer(_cfg("gaussian"), sd0, device="cuda", lr=1e-3, psa=True)
    losses = [float(tr.train_step(x.cuda(), tg.cuda(), tw.cuda()).cpu()[0]) for _ in range(12)]
    print("psa learns:", losses)
    assert np.isfinite(losses).all() and losses[-1] < 0.1 * losses[0], losses


def test_psa_bf16_storage_trains():
    """dtype="bf16" (bf16 activations and activation gradients, fp32 reductions / parameters) is supported for the
    attention block too: step-0 loss within 2 % of the fp32 path and the loss falls (the sanity gates of
    test_bf16_storage_training_tracks_fp32_and_learns)."""
    sd0 = synth.synth_state_dict(EXTRA, 5, "gaussian", seed=1, psa=True)
    x, tg, tw = make_batch("gaussian", seed=11)
    first = {}
    for dt in ("f32", "bf16"):
        tr = HRNetTrainer(_cfg("gaussian"), sd0, device="cuda", dtype=dt, lr=1e-3, psa=True)
        losses = [float(tr.train_step(x.cuda(), tg.cuda(), tw.cuda()).cpu()[0]) for _ in range(12)]
        first[dt] = losses[0]
        assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0], (dt, losses)
    assert abs(first["bf16"] / first["f32"] - 1) < 2e-2, first


def test_psa_public_training_route():
    """MODELS["pose_hrnet_psa"](cfg, is_train=True) -> get_optimizer -> function.train: runs, finite loss; init_weights
    leaves the LayerNorm at weight 1 / bias 0; a torch.optim.Adam over model.parameters() is accepted."""
    from udp_pose_amd.config import default_config
    from udp_pose_amd.function import JointsMSELoss, get_optimizer, train
    from udp_pose_amd.model import MODELS
    extra = synth.scaled_extra(32, modules=(1, 1, 1), blocks=1)
    cfg = default_config()
    cfg.MODEL.NAME = "pose_hrnet_psa"
    cfg.MODEL.EXTRA = extra
    cfg.MODEL.NUM_JOINTS = 17
    cfg.MODEL.TARGET_TYPE = "gaussian"
    cfg.MODEL.INIT_WEIGHTS = True
    cfg.MODEL.PRETRAINED = ""
    cfg.TRAIN.LR = 1e-3
    cfg.TRAIN.OPTIMIZER = "adam"
    torch.manual_seed(5)
    xb = torch.from_numpy(synth.synth_crops(4, 128, 96, seed=70))
    tg = torch.from_numpy(synth.synth_heatmaps(4, 17, 32, 24, seed=120))
    tw = torch.ones(4, 17, 1)
    loader = [(xb, tg, tw, {})] * 2
    model = MODELS[cfg.MODEL.NAME](cfg, is_train=True).cuda()
    sd = model.state_dict()
    ln = [k for k in sd if k.endswith(".deattn.conv_up.1.weight")]
    assert ln
    for k in ln:
        assert float(sd[k].min()) == 1.0 == float(sd[k].max()) and float(sd[k[:-6] + "bias"].abs().max()) == 0.0
    criterion = JointsMSELoss(use_target_weight=True)
    optimizer = get_optimizer(cfg, model)
    loss = train(cfg, loader, model, criterion, optimizer, 0, None, None, None)
    assert np.isfinite(loss) and model.trainer().step_count == 2 and model.trainer().psa
    train(cfg, loader[:1], model, criterion, torch.optim.Adam(model.parameters(), lr=1e-4), 1, None, None, None)
    sd1 = model.state_dict()
    assert set(sd1) == set(synth.hrnet_param_shapes(extra, 17, "gaussian", psa=True))
    k = ln[0][:-len("conv_up.1.weight")] + "conv_q_left.weight"
    assert not torch.equal(sd1[k], sd[k])                               # the attention weights moved
    assert all(torch.isfinite(v).all() for v in sd1.values() if v.is_floating_point())


def test_psa_w32_train_step_at_config3_size(golden_dir):
    """The reference PSA YAML's own shape (w32_256x192_adam_lr1e-3_offset_ofm_psa.yaml): pose_hrnet_psa W32 256x192,
    offset targets, 32 images -- the production grid split of the attention kernels (16 chunks of 192 pixels at
    64x48, one chunk at 8x6, 32 images summed by psa_t_params), several gradient buckets.  One train_step (fp32)
    against the CPU oracle in aggregate, in the form of test_w32_train_step_at_config3_size: both loss parts,
    heat-maps, per-tensor gradient L2 norms, finite parameters.

    The two norm thresholds (median 1e-3, 0.95-quantile 2e-2) are the plain net's.  They are kept because the fp32
    oracle against the fp64 oracle on this net and these inputs at 8 images stays inside them with room (measured
    once on the CPU): median 2.5e-4, 0.95-quantile 2.9e-3, max 2.1e-2 over all 1919 parameter tensors (.deattn. tensors alone:
    4.9e-4 / 3.7e-3 / 2.1e-2); loss parts to 3.5e-8 / 1.3e-7, heat-maps to 1.9e-5 of a 2.15 max.  Two fp32
    evaluations that far from the truth each differ by at most 5e-4 / 5.8e-3 from one another."""
    calib = dict(np.load(os.path.join(golden_dir, "bn_calib_w32_offset.npz")))
    sd0 = synth.synth_state_dict(synth.W32_EXTRA, 17, "offset", seed=0, bn_calib=calib, psa=True)
    cfg = {"MODEL": {"EXTRA": synth.W32_EXTRA, "NUM_JOINTS": 17, "TARGET_TYPE": "offset"}}
    n = 32
    x = torch.from_numpy(np.tile(synth.synth_crops(8, 256, 192, seed=41), (4, 1, 1, 1)))
    x = x + 0.02 * torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    tg = torch.from_numpy(synth.synth_heatmaps(n, 17, 64, 48, seed=42, channels_per_joint=3))
    tw = torch.from_numpy((np.random.default_rng(43).random((n, 17, 1)) > 0.15).astype(np.float32))
    tr = HRNetTrainer(cfg, sd0, device="cuda", lr=1e-3, psa=True)
    assert len(tr._buckets) >= 4
    loss = tr.train_step(x.cuda(), tg.cuda(), tw.cuda()).cpu().numpy()
    heat = tr._out.buf.cpu().numpy()
    gnorm = {k: float(tr.grad_of(k).double().norm()) for k in tr._keys}
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    parts, y, grads = o_train.loss_and_grads({k: v.clone() for k, v in sd0.items()}, synth.W32_EXTRA, x, tg, tw, "offset")
    rel = np.array([abs(gnorm[k] - float(grads[k].double().norm())) / (float(grads[k].double().norm()) + 1e-12) for k in tr._keys])
    att = np.array([".deattn." in k for k in tr._keys])
    print("config-3 PSA step: loss %s (oracle %s), heat-map max err %.3g of max %.3g; gradient norms rel median %.3g "
          "q95 %.3g max %.3g (.deattn.: %.3g / %.3g / %.3g)" % (
              loss, parts, np.abs(heat - y.numpy()).max(), float(y.abs().max()), np.median(rel), np.quantile(rel, 0.95),
              rel.max(), np.median(rel[att]), np.quantile(rel[att], 0.95), rel[att].max()))
    np.testing.assert_allclose(loss, np.array(parts), rtol=1e-4)
    np.testing.assert_allclose(heat, y.numpy(), rtol=0, atol=1e-3 * max(1.0, float(y.abs().max())))
    assert att.sum() == 1040 and min(float(g.double().norm()) for g in grads.values()) > 0
    assert np.median(rel) < 1e-3 and np.quantile(rel, 0.95) < 2e-2, (np.median(rel), np.quantile(rel, 0.95), rel.max())
    assert np.median(rel[att]) < 1e-3 and np.quantile(rel[att], 0.95) < 2e-2, (np.median(rel[att]), np.quantile(rel[att], 0.95))
    assert torch.isfinite(tr.flat).all() and tr.step_count == 1
