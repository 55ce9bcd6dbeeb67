"""MobileViTv2Trainer on the GPU: every parameter gradient, the loss, the heat-maps and the running statistics of one step
against the fp64 step of the reference's own module (tests/golden/mobilevitv2_train_step.npz) and against fp64 autograd of
the same graph (tests/mobilevitv2_train_ref.py) at a second seed and at the other widths, the padded-channel invariant the
padded BatchNorm rests on, graphed steps against eager ones, a loss that goes down, the round trip of the trained weights
into the inference model, and function.train.  128x64 input, 2 images, 5 joints, width 0.5: the last map is 4x2 -- two
pixels per parity class of the attention, 16 values per BatchNorm channel.

The gate is measured, not chosen (the rule of tests/test_gpu_shufflenet_train.py): ours may be at most 4 x as far from
fp64 as torch's fp32 CPU run of the same step is, or 1e-4 * max|ref| (1e-5 * max|ref| for running statistics) where that
is more.

Seeds.  The graph's only kinks are ReLUs (the attention's values, the decoder), some 60 000 inputs per step here, and the
nearest one always lies within a few fp32 rounding errors of zero.  An fp32 evaluation that rounds it to the other side
moves one channel's gradients by percents and everything upstream follows, whichever evaluator it is: torch's own fp32
CPU run does that at width 0.75 / seed 13 (two inputs flip; 3e-2 of a gradient's max off fp64).  A batch can carry a
gradient comparison only if the REFERENCE's own numbers say so, which ``_conditioned`` asserts before anything runs on
the GPU: the fp64 run's nearest ReLU input is at least 2 RMS errors of torch's fp32 CPU forward from zero
(``mobilevitv2_train_ref.kink_margin``; an error beyond 2 sigma has a chance of 5 %, and only the nearest input is that
close), and the fp32 CPU run is within 1e-3 of every gradient's max (the fixture tool's rule).  torch's fp32 rounding
moves with the number of CPU threads (seed 25 at width 0.5: 1.9 with one thread, 2.1 with four), so each case takes the
first seed from its starting number that passes both with 1, 4 and 16 threads: 0.5 from 21 -> 27 (2.9), 0.75 from
13 -> 14 (2.5), 1.0 from 14 -> 17 (6.3)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mobilevitv2_train_ref as T                                        # noqa: E402
from udp_pose_amd.mobilevitv2_plan import mobilevitv2_spec               # noqa: E402
from udp_pose_amd.model import MODELS                                    # noqa: E402
from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict  # noqa: E402
from udp_pose_amd.train import MobileViTv2Trainer, ShuffleNetV2Trainer   # noqa: E402

NAME = "pose_mobilevitv2_pixel_shuffle"
JOINTS, H, W = 5, 128, 64
EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": 0.5, "FINAL_CONV_KERNEL": 1}


def _trainer(sd, size=0.5, joints=JOINTS, **kw):
    return MobileViTv2Trainer(mobilevitv2_spec(dict(EXTRA, MODEL_SIZE=size), joints, "gaussian"), joints, "gaussian",
                              {k: v.clone() for k, v in sd.items()}, device="cuda", **kw)


def _cfg(joints=JOINTS, size=0.5):
    return {"MODEL": {"NAME": NAME, "NUM_JOINTS": joints, "TARGET_TYPE": "gaussian", "INIT_WEIGHTS": False,
                      "EXTRA": dict(EXTRA, MODEL_SIZE=size)}, "TRAIN": {"OPTIMIZER": "adam", "LR": 1e-3}}


def _step(tr, x, tg, tw):
    heat = tr.forward(x.cuda())
    loss, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    return heat, loss


def _gate(tr, g64, g32, tag=""):
    bad = []
    for k in tr._keys:
        exact = g64[k].numpy()
        mx = float(np.abs(exact).max())
        e_ours = float(np.abs(tr.grad_of(k).cpu().double().numpy() - exact).max())
        e_f32 = float(np.abs(g32[k].double().numpy() - exact).max())
        gate = max(4 * e_f32, 1e-4 * mx)
        print("%s%-62s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (tag, k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad


def _gate_stats(tr, sd64, sd32):
    got = tr.state_dict()
    bad = []
    for k in tr._stat_keys:
        want = sd64[k].numpy()
        mx = float(np.abs(want).max())
        e_ours = float(np.abs(got[k].double().numpy() - want).max())
        e_f32 = float(np.abs(sd32[k].double().numpy() - want).max())
        gate = max(4 * e_f32, 1e-5 * mx)
        print("%-62s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, e_f32, gate))
    assert not bad, bad
    return got


def _conditioned(sd, batch, r64, r32):
    """The two rules of the module docstring, from the CPU references alone."""
    margin = T.kink_margin(sd, batch[0])
    gscale = max(float(g.abs().max()) for g in r64[2].values())
    worst = max(float((r32[2][k].double() - g).abs().max()) / float(g.abs().max()) for k, g in r64[2].items()
                if float(g.abs().max()) > 1e-12 * gscale)
    print("conditioning: nearest ReLU input %.2f RMS fp32 errors from zero, worst fp32-CPU gradient error %.2e of its max" % (margin, worst))
    assert margin >= 2.0 and worst <= 1e-3, (margin, worst)


@pytest.fixture(scope="module")
def step0(golden_dir):
    """The fixture's step: its batch and the weights of its seed."""
    g = np.load(os.path.join(golden_dir, "mobilevitv2_train_step.npz"))
    sd = synth_mobilevitv2_state_dict(seed=int(g["seed"]), num_joints=JOINTS)
    batch = tuple(torch.from_numpy(g[k]) for k in ("x", "target", "target_weight"))
    return g, sd, batch


def test_gradients_loss_and_running_statistics_match_the_reference_step(step0):
    """Against the reference module's own fp64 step: the gate is 4 x the fixture's recorded fp32 error of that module."""
    g, sd, (x, tg, tw) = step0
    tr = _trainer(sd)
    assert isinstance(tr, ShuffleNetV2Trainer)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), float(g["loss"]), rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), g["heatmaps"], atol=1e-3)
    keys = [str(k) for k in g["keys"]]
    assert keys == tr._keys
    bad = []
    for i, k in enumerate(keys):
        ours = tr.grad_of(k).cpu().double().numpy().reshape(-1)
        if ("g_%d" % i) in g.files:
            want = g["g_%d" % i].reshape(-1)
        else:
            want, ours = g["s_%d" % i], ours[g["p_%d" % i]]
        e_ours, mx = float(np.abs(ours - want).max()), float(g["gmax"][i])
        gate = max(4 * float(g["e32"][i]), 1e-4 * mx)
        print("fixture %-62s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, float(g["e32"][i]), e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad
    # the classifier is a parameter the forward never applies: its gradient is exactly zero
    assert float(tr.grad_of("backbone.classifier.1.weight").abs().max()) == 0.0
    assert float(tr.grad_of("backbone.classifier.1.bias").abs().max()) == 0.0
    # a wrong BatchNorm eps or momentum shows here: the running ones move by momentum * (batch - running)
    got = tr.state_dict()
    for bn in g["stat_bns"]:
        for s in (".running_mean", ".running_var"):
            want = g["stat_%s%s" % (bn, s)]
            np.testing.assert_allclose(got[str(bn) + s].numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()), err_msg=str(bn) + s)
    assert int(got["backbone.conv_1.block.norm.num_batches_tracked"]) == 0   # no optimizer step yet


@pytest.fixture(scope="module")
def step1():
    """A second seed and the restatement's references of it, computed once: fp64 and fp32 on the CPU."""
    sd = synth_mobilevitv2_state_dict(seed=27, num_joints=JOINTS)
    batch = T.make_batch(2, JOINTS, H, W, seed=31)
    r64, r32 = T.loss_and_grads(sd, *batch, torch.float64), T.loss_and_grads(sd, *batch, torch.float32)
    _conditioned(sd, batch, r64, r32)
    return sd, batch, r64, r32


def test_every_key_matches_the_restatement_at_a_second_seed(step1):
    sd, (x, tg, tw), (loss64, y64, g64, sd64), (_, _, g32, sd32) = step1
    tr = _trainer(sd)
    assert tr._keys == list(g64)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    _gate(tr, g64, g32, tag="restatement ")
    _gate_stats(tr, sd64, sd32)


@pytest.fixture(scope="module")
def wide():
    """Width 0.75 (24-, 48- and 96-channel tensors: pads everywhere) and its references."""
    sd = synth_mobilevitv2_state_dict(seed=14, model_size=0.75, num_joints=JOINTS)
    batch = T.make_batch(2, JOINTS, H, W, seed=32)
    r64, r32 = T.loss_and_grads(sd, *batch, torch.float64), T.loss_and_grads(sd, *batch, torch.float32)
    _conditioned(sd, batch, r64, r32)
    return sd, batch, r64, r32


def test_width_075_matches_the_restatement(wide):
    sd, (x, tg, tw), (loss64, y64, g64, sd64), (_, _, g32, sd32) = wide
    tr = _trainer(sd, size=0.75)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    _gate(tr, g64, g32, tag="0.75 ")
    _gate_stats(tr, sd64, sd32)


def test_width_10_runs_a_step():
    """The 1.0 width through the same code (d = 128 / 192 / 256): one forward + backward against the restatement."""
    sd = synth_mobilevitv2_state_dict(seed=17, model_size=1.0, num_joints=JOINTS)
    x, tg, tw = T.make_batch(2, JOINTS, 64, 64, seed=33)
    r64, r32 = T.loss_and_grads(sd, x, tg, tw, torch.float64), T.loss_and_grads(sd, x, tg, tw, torch.float32)
    _conditioned(sd, (x, tg, tw), r64, r32)
    (loss64, y64, g64, _), g32 = r64, r32[2]
    tr = _trainer(sd, size=1.0)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    _gate(tr, g64, g32, tag="1.0 ")


def _pads(buf, a):
    return buf.view(-1, a.ck)[:, a.c:]


@pytest.mark.parametrize("size", [0.75, 0.5])
def test_padded_channels_stay_exactly_zero(step0, wide, size):
    """What the padded BatchNorm rests on: every stored channel of every activation and gradient is written, pads are 0;
    the slack of ``flat`` / ``grad`` is 0 and stays 0 through optimizer steps.  Width 0.75 has pads everywhere; at 0.5
    the padded tensors are the qkv maps (1 + 2d channels) and their gradients."""
    sd, (x, tg, tw) = (wide[0], wide[1]) if size == 0.75 else (step0[1], step0[2])
    tr = _trainer(sd, size=size, lr=1e-3)
    heat = tr.forward(x.cuda())
    acts = []
    for y, _, _, _ in tr._tape:
        acts += list(y.ys) if hasattr(y, "ys") else [y]
    padded = [a for a in acts if a.c < a.ck and a.buf.dim() == 1]
    if size == 0.75:                                # the three 24-channel stem tensors (stored 32) and the qkv maps
        assert len(padded) == 12 and {a.c for a in padded} == {24, 193, 289, 385}
    else:
        assert len(padded) == 9 and {a.c for a in padded} == {129, 193, 257}       # the 2 + 4 + 3 qkv maps
    for a in padded:
        p = _pads(a.buf, a)
        assert not torch.isnan(p).any() and float(p.abs().max()) == 0.0, (a.c, a.ck)
    # gradients: checked when their consumer runs (they are complete then and freed right after)
    seen = []
    for i, (y, bwd, keep, keys) in enumerate(list(tr._tape)):
        def checked(y=y, bwd=bwd):
            for a in (y.ys if hasattr(y, "ys") else [y]):
                if a.grad is not None and a.c < a.ck and a.buf.dim() == 1:
                    p = _pads(a.grad, a)
                    seen.append((a.c, bool(torch.isnan(p).any()), float(p.abs().max())))
            bwd()
        tr._tape[i] = (y, checked, keep, keys)
    _, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    assert len(seen) == len(padded) and all(not nan and mx == 0.0 for _, nan, mx in seen), [s for s in seen if s[1] or s[2] != 0.0][:5]
    mask = torch.ones(tr.flat.numel(), dtype=torch.bool)
    for k in tr._keys + tr._stat_keys:
        mask[tr._off[k]:tr._off[k] + int(np.prod(tr._shapes[k]))] = False
    mask = mask.cuda()
    assert int(mask.sum()) > 100

    def slack_is_zero():
        return float(tr.flat[mask].abs().max()) == 0.0 and float(tr.grad[mask[:tr._n_param]].abs().max()) == 0.0 and \
            not torch.isnan(tr.flat).any() and not torch.isnan(tr.grad).any()
    assert slack_is_zero()
    tr.adam_step()
    for _ in range(2):
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    torch.cuda.synchronize()
    assert tr.step_count == 3 and slack_is_zero()


def test_graphed_steps_equal_eager_steps(step0):
    sd = step0[1]
    batches = [T.make_batch(2, JOINTS, H, W, seed=40 + k) for k in range(3)]
    outs = []
    for graphed in (False, True):
        tr = _trainer(sd, lr=1e-3)
        losses = []
        for x, tg, tw in batches:
            x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
            losses.append((tr.train_step_graphed(x, tg, tw) if graphed else tr.train_step(x, tg, tw)).clone())
        torch.cuda.synchronize()
        outs.append((np.array([l.cpu().numpy() for l in losses]), tr.flat.cpu().numpy().copy(), tr.step_count))
    assert outs[0][2] == outs[1][2] == 3
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-12)       # the loss VALUE is summed with fp64 atomics
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_loss_goes_down_on_one_batch(step0):
    _, sd, (x, tg, tw) = step0
    tr = _trainer(sd, lr=1e-3)
    x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
    losses = [float(tr.train_step_graphed(x, tg, tw).cpu()[0]) for _ in range(20)]
    print("loss: first %.5g, last %.5g" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_trained_net_round_trips_into_the_inference_model():
    """Two steps, then ``state_dict()`` into ``MODELS[...](cfg, is_train=False)``: its eval forward against the same
    weights through the CPU restatement in eval mode, to what the inference test allows."""
    cfg = _cfg(17)
    sd0 = synth_mobilevitv2_state_dict(seed=7, num_joints=17)
    model = MODELS[NAME](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    tr = model.trainer()
    assert type(tr) is MobileViTv2Trainer
    assert model.parameters()[0].data_ptr() == tr.flat.data_ptr()
    for k in range(2):
        x, tg, tw = T.make_batch(2, 17, H, W, seed=60 + k)
        assert tuple(model(x.cuda()).shape) == (2, 17, H // 4, W // 4)           # train-mode __call__
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    sd2 = model.state_dict()                                                     # read back from the trainer
    assert int(sd2["backbone.conv_1.block.norm.num_batches_tracked"]) == 2
    for k in ("backbone.layer_4.1.global_rep.2.pre_norm_attn.0.weight", "backbone.layer_4.1.global_rep.2.pre_norm_attn.1.qkv_proj.block.conv.bias",
              "backbone.layer_3.1.local_rep.0.block.conv.weight"):
        assert float((sd2[k] - sd0[k]).abs().max()) > 0, k                      # a GroupNorm weight, a qkv bias, a depthwise weight
    assert list(sd2) == list(sd0) and all(tuple(sd2[k].shape) == tuple(sd0[k].shape) for k in sd0)
    net = MODELS[NAME](cfg, is_train=False).load_state_dict(sd2).to("cuda").eval()
    x1 = T.make_batch(1, 17, H, W, seed=70)[0]
    got = net(x1.cuda()).cpu().numpy()
    with torch.no_grad():
        want = T.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd2.items()}, x1.double(), training=False).numpy()
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("round trip: max err %.3g, max|heat-map| %.3g" % (err, scale))
    assert got.shape == (1, 17, H // 4, W // 4) and err <= 1e-3
    same = model.eval()(x1.cuda()).cpu().numpy()
    np.testing.assert_array_equal(same, got)


def test_function_train_drives_the_model():
    from udp_pose_amd.function import JointsMSELoss, get_optimizer, train
    cfg = _cfg()
    sd0 = synth_mobilevitv2_state_dict(seed=9, num_joints=JOINTS)
    model = MODELS[NAME](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    loader = []
    for k in range(2):
        x, tg, tw = T.make_batch(2, JOINTS, H, W, seed=80 + k)
        loader.append((x, tg, tw, {}))
    before = model.trainer().flat.clone()
    loss = train(cfg, loader, model, JointsMSELoss(use_target_weight=True), get_optimizer(cfg, model), 0, None, None, None)
    torch.cuda.synchronize()
    tr = model.trainer()
    assert np.isfinite(loss) and loss > 0 and tr.step_count == 2 and not torch.isnan(tr.flat).any()
    assert float((tr.flat - before).abs().max()) > 0
    assert float((model.state_dict()["final_layer.weight"] - sd0["final_layer.weight"]).abs().max()) > 0
