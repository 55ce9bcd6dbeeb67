"""ShuffleNetV2Trainer / ShuffleNetV2DeconvTrainer on the GPU: every parameter gradient of one step against the fp64
step of the reference's own module (tests/golden/shufflenet_train_step.npz) and against fp64 autograd of the same graph
(tests/shufflenet_train_ref.py), the running statistics, the padded-channel invariant the padded BatchNorm rests on, the
other model sizes and the deconv head, graphed steps against eager ones, a loss that goes down, the round trip of the
trained weights into the inference model, and function.train.

The gradient gate is measured, not chosen: ours may be at most 4 x as far from fp64 as torch's fp32 CPU run of the same
step is (or 1e-4 * max|ref|, whichever is larger)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import shufflenet_ref as R                                              # noqa: E402
import shufflenet_train_ref as T                                        # noqa: E402
from udp_pose_amd.model import MODELS                                   # noqa: E402
from udp_pose_amd.shufflenet_plan import shufflenet_deconv_spec, shufflenet_spec   # noqa: E402
from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict, synth_shufflenet_state_dict   # noqa: E402
from udp_pose_amd.train import ShuffleNetV2DeconvTrainer, ShuffleNetV2Trainer   # noqa: E402

PS, DC = "pose_shufflenetv2_10x_pixel_shuffle", "pose_shufflenetv2_10x"
JOINTS = 5
PS_EXTRA = {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "1.0x", "FINAL_CONV_KERNEL": 1}
DC_EXTRA = {"MODEL_SIZE": "1.0x", "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [64, 32, 32],
            "NUM_DECONV_KERNELS": [4, 4, 4], "FINAL_CONV_KERNEL": 1}


def _trainer(sd, extra=PS_EXTRA, target="gaussian", joints=JOINTS, **kw):
    if "NUM_DECONV_LAYERS" in extra:
        return ShuffleNetV2DeconvTrainer(shufflenet_deconv_spec(extra, joints, target), joints, target,
                                         {k: v.clone() for k, v in sd.items()}, device="cuda", **kw)
    return ShuffleNetV2Trainer(shufflenet_spec(extra, joints, target), joints, target, {k: v.clone() for k, v in sd.items()},
                               device="cuda", **kw)


def _step(tr, x, tg, tw):
    heat = tr.forward(x.cuda())
    loss, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    return heat, loss


def _gate(tr, g64, g32, keys=None, tag=""):
    bad = []
    for k in (keys or tr._keys):
        exact = g64[k].numpy()
        mx = float(np.abs(exact).max())
        e_ours = float(np.abs(tr.grad_of(k).cpu().double().numpy() - exact).max())
        e_f32 = float(np.abs(g32[k].double().numpy() - exact).max())
        gate = max(4 * e_f32, 1e-4 * mx)
        print("%s%-44s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (tag, k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad


@pytest.fixture(scope="module")
def step0(golden_dir):
    """The fixture's step and the restatement's references of it, computed once: fp64 and fp32 on the CPU."""
    g = np.load(os.path.join(golden_dir, "shufflenet_train_step.npz"))
    sd = synth_shufflenet_state_dict(seed=int(g["seed"]), num_joints=JOINTS)
    batch = tuple(torch.from_numpy(g[k]) for k in ("x", "target", "target_weight"))
    return g, sd, batch, T.loss_and_grads(sd, *batch, torch.float64), T.loss_and_grads(sd, *batch, torch.float32)


def test_gradients_loss_and_running_statistics_match_the_reference_step(step0):
    g, sd, (x, tg, tw), (loss64, y64, g64, sd64), (_, _, g32, sd32) = step0
    tr = _trainer(sd)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), float(g["loss"]), rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), g["heatmaps"], atol=1e-3)
    keys = [str(k) for k in g["keys"]]
    assert keys == tr._keys
    bad = []
    for i, k in enumerate(keys):                                        # the reference module's own gradients
        ours = tr.grad_of(k).cpu().double().numpy().reshape(-1)
        if ("g_%d" % i) in g.files:
            want = g["g_%d" % i].reshape(-1)
        else:
            want, ours = g["s_%d" % i], ours[g["p_%d" % i]]
        e_ours, mx = float(np.abs(ours - want).max()), float(g["gmax"][i])
        gate = max(4 * float(g["e32"][i]), 1e-4 * mx)
        print("fixture %-44s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, float(g["e32"][i]), e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad
    got = tr.state_dict()
    for bn in g["stat_bns"]:
        for s in (".running_mean", ".running_var"):
            want = g["stat_%s%s" % (bn, s)]
            np.testing.assert_allclose(got[str(bn) + s].numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()), err_msg=str(bn) + s)
    # the same against the restatement run here: every element of every gradient, every running statistic
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    _gate(tr, g64, g32, tag="restatement ")
    # every running statistic: the fixture rule (1e-5 of the tensor's max), or 4 x what torch's fp32 CPU run of this step is
    # off by where that is more -- a stage-4 BatchNorm averages 12 values per channel, and a mean that nearly cancels
    # carries the absolute error of its terms
    bad = []
    for k in tr._stat_keys:
        want = sd64[k].numpy()
        e_ours = float(np.abs(got[k].double().numpy() - want).max())
        e_f32 = float(np.abs(sd32[k].double().numpy() - want).max())
        gate = max(4 * e_f32, 1e-5 * float(np.abs(want).max()))
        if not e_ours <= gate:
            bad.append((k, e_ours, e_f32, gate))
    assert not bad, bad
    assert int(got["backbone.first_conv.1.num_batches_tracked"]) == 0   # no optimizer step yet


def _pads(buf, a):
    return buf.view(-1, a.ck)[:, a.c:]


def test_padded_channels_stay_exactly_zero(step0):
    """What the padded BatchNorm rests on: every stored channel of every activation and gradient is written, pads are 0;
    the slack of ``flat`` / ``grad`` is 0 and stays 0 through optimizer steps."""
    _, sd, (x, tg, tw), _, _ = step0
    tr = _trainer(sd, lr=1e-3)
    heat = tr.forward(x.cuda())
    acts = []
    for y, _, _, _ in tr._tape:
        acts += list(y.ys) if hasattr(y, "ys") else [y]
    padded = [a for a in acts if a.c < a.ck and a.buf.dim() == 1]
    assert len(padded) > 60 and {a.c for a in padded} >= {24, 58, 116, 232}
    for a in padded:
        p = _pads(a.buf, a)
        assert not torch.isnan(p).any() and float(p.abs().max()) == 0.0, (a.c, a.ck)
    # gradients: checked when their consumer runs (they are complete then and freed right after)
    seen = []
    tape = list(tr._tape)
    for i, (y, bwd, keep, keys) in enumerate(tape):
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
    assert len(seen) > 60 and all(not nan and mx == 0.0 for _, nan, mx in seen), [s for s in seen if s[1] or s[2] != 0.0][:5]
    mask = torch.ones(tr.flat.numel(), dtype=torch.bool)
    for k in tr._keys + tr._stat_keys:
        mask[tr._off[k]:tr._off[k] + int(np.prod(tr._shapes[k]))] = False
    mask = mask.cuda()
    assert int(mask.sum()) > 1000

    def slack_is_zero():
        return float(tr.flat[mask].abs().max()) == 0.0 and float(tr.grad[mask[:tr._n_param]].abs().max()) == 0.0 and \
            not torch.isnan(tr.flat).any() and not torch.isnan(tr.grad).any()
    assert slack_is_zero()
    tr.adam_step()
    for _ in range(2):
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    torch.cuda.synchronize()
    assert tr.step_count == 3 and slack_is_zero()


@pytest.mark.parametrize("size", ["0.5x", "1.5x"])
def test_other_model_sizes(size):
    """r = 24 and 88 (and equal / unequal halves behind the first unit) at 64x64, batch 2."""
    sd = synth_shufflenet_state_dict(seed=13, model_size=size, num_joints=JOINTS)
    x, tg, tw = T.make_batch(2, JOINTS, 64, 64, seed=31)
    _, _, g64, _ = T.loss_and_grads(sd, x, tg, tw, torch.float64)
    _, _, g32, _ = T.loss_and_grads(sd, x, tg, tw, torch.float32)
    tr = _trainer(sd, extra=dict(PS_EXTRA, MODEL_SIZE=size))
    _step(tr, x, tg, tw)
    _gate(tr, g64, g32)


@pytest.mark.parametrize("bias", [False, True])
def test_deconv_sibling(bias):
    extra = dict(DC_EXTRA, DECONV_WITH_BIAS=bias)
    sd = synth_shufflenet_deconv_state_dict(seed=14, num_joints=JOINTS, deconv_filters=(64, 32, 32), deconv_with_bias=bias)
    x, tg, tw = T.make_batch(2, JOINTS, 64, 64, seed=33)
    loss64, y64, g64, _ = T.loss_and_grads(sd, x, tg, tw, torch.float64)
    _, _, g32, _ = T.loss_and_grads(sd, x, tg, tw, torch.float32)
    tr = _trainer(sd, extra=extra)
    heat, loss = _step(tr, x, tg, tw)
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    keys = [k for k in tr._keys if k.startswith("deconv_layers.")]
    assert len(keys) == (12 if bias else 9)
    _gate(tr, g64, g32, keys + ["backbone.conv_last.0.weight", "backbone.features.9.branch_main.3.weight",
                                "backbone.features.4.branch_proj.0.weight", "backbone.first_conv.0.weight", "final_layer.weight"])


def test_3x3_final_layer_and_offset_targets():
    extra = dict(PS_EXTRA, FINAL_CONV_KERNEL=3)
    sd = synth_shufflenet_state_dict(seed=15, num_joints=JOINTS, target_type="offset", final_kernel=3)
    x, tg, tw = T.make_batch(2, 3 * JOINTS, 64, 64, seed=35)
    tw = tw[:, :JOINTS].contiguous()
    _, y64, g64, _ = T.loss_and_grads(sd, x, tg, tw, torch.float64, criterion=T.joints_mse_offset)
    _, _, g32, _ = T.loss_and_grads(sd, x, tg, tw, torch.float32, criterion=T.joints_mse_offset)
    tr = _trainer(sd, extra=extra, target="offset")
    heat, loss = _step(tr, x, tg, tw)
    assert tuple(heat.shape) == (2, 3 * JOINTS, 16, 16) and tuple(sd["final_layer.weight"].shape) == (15, 32, 3, 3)
    assert np.isfinite(loss.cpu().numpy()).all() and float(loss.cpu().sum()) > 0
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    _gate(tr, g64, g32, ["final_layer.weight", "final_layer.bias"])


def test_graphed_steps_equal_eager_steps(step0):
    sd = step0[1]
    batches = [T.make_batch(2, JOINTS, 96, 64, seed=40 + k) for k in range(3)]
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
    sd, (x, tg, tw) = step0[1], step0[2]
    tr = _trainer(sd, lr=1e-3)
    x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
    losses = [float(tr.train_step_graphed(x, tg, tw).cpu()[0]) for _ in range(20)]
    print("loss: first %.5g, last %.5g" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_trained_net_round_trips_into_the_inference_model():
    """Two steps, then ``state_dict()`` into ``MODELS[...](cfg, is_train=False)``: its eval forward against the same
    weights through the CPU restatement, to what the inference test allows."""
    cfg = {"MODEL": {"NAME": PS, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "INIT_WEIGHTS": False, "EXTRA": PS_EXTRA}}
    sd0 = synth_shufflenet_state_dict(seed=7)
    model = MODELS[PS](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    tr = model.trainer()
    assert isinstance(tr, ShuffleNetV2Trainer) and not isinstance(tr, ShuffleNetV2DeconvTrainer)
    assert model.parameters()[0].data_ptr() == tr.flat.data_ptr()
    for k in range(2):
        x, tg, tw = T.make_batch(2, 17, 64, 64, seed=60 + k)
        assert tuple(model(x.cuda()).shape) == (2, 17, 16, 16)                   # train-mode __call__
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    sd2 = model.state_dict()                                                     # read back from the trainer
    assert int(sd2["backbone.first_conv.1.num_batches_tracked"]) == 2
    assert float((sd2["backbone.features.15.branch_main.3.weight"] - sd0["backbone.features.15.branch_main.3.weight"]).abs().max()) > 0
    assert list(sd2) == list(sd0) and all(tuple(sd2[k].shape) == tuple(sd0[k].shape) for k in sd0)
    net = MODELS[PS](cfg, is_train=False).load_state_dict(sd2).to("cuda").eval()
    x1 = T.make_batch(1, 17, 64, 64, seed=70)[0]
    got = net(x1.cuda()).cpu().numpy()
    want = R.forward({k: v.clone() for k, v in sd2.items()}, x1).numpy()
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("round trip: max err %.3g, max|heat-map| %.3g" % (err, scale))
    assert got.shape == (1, 17, 16, 16) and err <= 1e-3
    same = model.eval()(x1.cuda()).cpu().numpy()
    np.testing.assert_array_equal(same, got)


@pytest.mark.parametrize("name", [PS, DC])
def test_function_train_drives_the_model(name):
    from udp_pose_amd.function import JointsMSELoss, get_optimizer, train
    extra = PS_EXTRA if name == PS else DC_EXTRA
    cfg = {"MODEL": {"NAME": name, "NUM_JOINTS": JOINTS, "TARGET_TYPE": "gaussian", "INIT_WEIGHTS": False, "EXTRA": extra},
           "TRAIN": {"OPTIMIZER": "adam", "LR": 1e-3}}
    sd0 = (synth_shufflenet_state_dict(seed=9, num_joints=JOINTS) if name == PS else
           synth_shufflenet_deconv_state_dict(seed=9, num_joints=JOINTS, deconv_filters=(64, 32, 32)))
    model = MODELS[name](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    loader = []
    for k in range(2):
        x, tg, tw = T.make_batch(2, JOINTS, 64, 64, seed=80 + k)
        loader.append((x, tg, tw, {}))
    before = model.trainer().flat.clone()
    loss = train(cfg, loader, model, JointsMSELoss(use_target_weight=True), get_optimizer(cfg, model), 0, None, None, None)
    torch.cuda.synchronize()
    tr = model.trainer()
    assert np.isfinite(loss) and loss > 0 and tr.step_count == 2 and not torch.isnan(tr.flat).any()
    assert float((tr.flat - before).abs().max()) > 0
    assert float((model.state_dict()["final_layer.weight"] - sd0["final_layer.weight"]).abs().max()) > 0
