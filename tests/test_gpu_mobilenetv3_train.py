"""MobileNetV3Trainer / MobileNetV3DeconvTrainer on the GPU: every parameter gradient, the loss, the heat-maps and every
running statistic of one step against fp64 autograd of the same graph (tests/mobilenetv3_train_ref.py), the padded-channel
invariant the padded BatchNorm rests on, graphed steps against eager ones, a loss that goes down, the round trip of the
trained weights into the inference model, and function.train.  Both heads at 64x64 input, 2 images, 5 joints: the last
maps are 2x2 and every BatchNorm still averages 8 values.

torchvision is not installed, so no fixture of the reference's own module can exist: the arbiter is the restatement,
which tests/test_mobilenetv3_train_cpu.py pins to tests/mobilenetv3_ref.py and to an nn.Module mirror of stock layers.

The gate is measured, not chosen (the rule of tests/test_gpu_shufflenet_train.py): ours may be at most 4 x as far from
fp64 as torch's fp32 CPU run of the same step is, or 1e-4 * max|ref| (1e-5 * max|ref| for running statistics) where that
is more."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mobilenetv3_train_ref as T                                        # noqa: E402
from udp_pose_amd.mobilenetv3_plan import mobilenetv3_deconv_spec, mobilenetv3_ps_spec   # noqa: E402
from udp_pose_amd.model import MODELS                                    # noqa: E402
from udp_pose_amd.synth_mobilenetv3 import synth_mobilenetv3_state_dict  # noqa: E402
from udp_pose_amd.train import MobileNetV3DeconvTrainer, MobileNetV3Trainer, ShuffleNetV2Trainer   # noqa: E402

PS, DC = "pose_mobilenetv3_small_pixel_shuffle", "pose_mobilenetv3_small"
JOINTS = 5
EXTRA = {PS: {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": "small", "FINAL_CONV_KERNEL": 1},
         DC: {"MODEL_SIZE": "small", "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [64, 32, 32],
              "NUM_DECONV_KERNELS": [4, 4, 4], "FINAL_CONV_KERNEL": 1}}


def _sd(name, seed, joints=JOINTS):
    if name == PS:
        return synth_mobilenetv3_state_dict(seed=seed, head="pixel_shuffle", num_joints=joints)
    return synth_mobilenetv3_state_dict(seed=seed, head="deconv", num_joints=joints, deconv_filters=(64, 32, 32))


def _trainer(name, sd, joints=JOINTS, **kw):
    sd = {k: v.clone() for k, v in sd.items()}
    if name == PS:
        return MobileNetV3Trainer(mobilenetv3_ps_spec(EXTRA[PS], joints, "gaussian"), joints, "gaussian", sd, device="cuda", **kw)
    return MobileNetV3DeconvTrainer(mobilenetv3_deconv_spec(EXTRA[DC], joints, "gaussian"), joints, "gaussian", sd, device="cuda", **kw)


def _cfg(name, joints=JOINTS):
    return {"MODEL": {"NAME": name, "NUM_JOINTS": joints, "TARGET_TYPE": "gaussian", "INIT_WEIGHTS": False, "EXTRA": EXTRA[name]},
            "TRAIN": {"OPTIMIZER": "adam", "LR": 1e-3}}


@pytest.fixture(scope="module")
def step0():
    """One step of each head and the restatement's references of it, computed once: fp64 and fp32 on the CPU."""
    out = {}
    for name, seed in ((PS, 21), (DC, 22)):
        sd = _sd(name, seed)
        batch = T.make_batch(2, JOINTS, 64, 64, seed=31)
        out[name] = (sd, batch, T.loss_and_grads(sd, *batch, torch.float64), T.loss_and_grads(sd, *batch, torch.float32))
    return out


@pytest.mark.parametrize("name", [PS, DC])
def test_gradients_loss_heatmaps_and_running_statistics_match_fp64(step0, name):
    sd, (x, tg, tw), (loss64, y64, g64, sd64), (_, _, g32, sd32) = step0[name]
    tr = _trainer(name, sd)
    assert isinstance(tr, ShuffleNetV2Trainer) and tr._keys == list(g64)
    heat = tr.forward(x.cuda())
    loss, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    bad = []
    for k in tr._keys:
        exact = g64[k].numpy()
        mx = float(np.abs(exact).max())
        e_ours = float(np.abs(tr.grad_of(k).cpu().double().numpy() - exact).max())
        e_f32 = float(np.abs(g32[k].double().numpy() - exact).max())
        gate = max(4 * e_f32, 1e-4 * mx)
        print("%-44s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad
    # every running statistic: this fails if the backbone used momentum 0.1 or eps 1e-5 (the variance of a channel goes
    # into the next layers through 1 / sqrt(var + eps), and the running ones move by momentum * (batch - running))
    got = tr.state_dict()
    bad = []
    for k in tr._stat_keys:
        want = sd64[k].numpy()
        mx = float(np.abs(want).max())
        e_ours = float(np.abs(got[k].double().numpy() - want).max())
        e_f32 = float(np.abs(sd32[k].double().numpy() - want).max())
        gate = max(4 * e_f32, 1e-5 * mx)
        print("%-44s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, e_f32, gate))
    assert not bad, bad
    moved = float((sd64["backbone.0.5.block.1.1.running_mean"] - sd["backbone.0.5.block.1.1.running_mean"].double()).abs().max())
    assert moved > 0 and int(got["backbone.0.0.1.num_batches_tracked"]) == 0     # no optimizer step yet


def _pads(buf, a):
    return buf.view(-1, a.ck)[:, a.c:]


@pytest.mark.parametrize("name", [PS, DC])
def test_padded_channels_stay_exactly_zero(step0, name):
    """What the padded BatchNorm rests on: every stored channel of every activation and gradient is written, pads are 0;
    the slack of ``flat`` / ``grad`` is 0 and stays 0 through optimizer steps."""
    sd, (x, tg, tw) = step0[name][:2]
    tr = _trainer(name, sd, lr=1e-3)
    heat = tr.forward(x.cuda())
    acts = []
    for y, _, _, _ in tr._tape:
        acts += list(y.ys) if hasattr(y, "ys") else [y]
    padded = [a for a in acts if a.c < a.ck and a.buf.dim() == 1]
    assert len(padded) > 20 and {a.c for a in padded} >= {24, 40, 72, 88, 120}
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
    assert len(seen) > 20 and all(not nan and mx == 0.0 for _, nan, mx in seen), [s for s in seen if s[1] or s[2] != 0.0][:5]
    mask = torch.ones(tr.flat.numel(), dtype=torch.bool)
    for k in tr._keys + tr._stat_keys:
        mask[tr._off[k]:tr._off[k] + int(np.prod(tr._shapes[k]))] = False
    mask = mask.cuda()
    assert int(mask.sum()) > 300

    def slack_is_zero():
        return float(tr.flat[mask].abs().max()) == 0.0 and float(tr.grad[mask[:tr._n_param]].abs().max()) == 0.0 and \
            not torch.isnan(tr.flat).any() and not torch.isnan(tr.grad).any()
    assert slack_is_zero()
    tr.adam_step()
    for _ in range(2):
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    torch.cuda.synchronize()
    assert tr.step_count == 3 and slack_is_zero()


@pytest.mark.parametrize("name", [PS, DC])
def test_graphed_steps_equal_eager_steps(step0, name):
    sd = step0[name][0]
    batches = [T.make_batch(2, JOINTS, 64, 64, seed=40 + k) for k in range(3)]
    outs = []
    for graphed in (False, True):
        tr = _trainer(name, sd, lr=1e-3)
        losses = []
        for x, tg, tw in batches:
            x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
            losses.append((tr.train_step_graphed(x, tg, tw) if graphed else tr.train_step(x, tg, tw)).clone())
        torch.cuda.synchronize()
        outs.append((np.array([l.cpu().numpy() for l in losses]), tr.flat.cpu().numpy().copy(), tr.step_count))
    assert outs[0][2] == outs[1][2] == 3
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=1e-12)       # the loss VALUE is summed with fp64 atomics
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", [PS, DC])
def test_loss_goes_down_on_one_batch(step0, name):
    sd, (x, tg, tw) = step0[name][:2]
    tr = _trainer(name, sd, lr=1e-3)
    x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
    losses = [float(tr.train_step_graphed(x, tg, tw).cpu()[0]) for _ in range(20)]
    print("loss: first %.5g, last %.5g" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


@pytest.mark.parametrize("name", [PS, DC])
def test_trained_net_round_trips_into_the_inference_model(name):
    """Two steps, then ``state_dict()`` into ``MODELS[...](cfg, is_train=False)``: its eval forward against the same
    weights through the CPU restatement in eval mode, to what the inference test allows."""
    cfg = _cfg(name, 17)
    sd0 = _sd(name, 7, joints=17)
    model = MODELS[name](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    tr = model.trainer()
    assert type(tr) is (MobileNetV3Trainer if name == PS else MobileNetV3DeconvTrainer)
    assert model.parameters()[0].data_ptr() == tr.flat.data_ptr()
    for k in range(2):
        x, tg, tw = T.make_batch(2, 17, 64, 64, seed=60 + k)
        assert tuple(model(x.cuda()).shape) == (2, 17, 16, 16)                   # train-mode __call__
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    sd2 = model.state_dict()                                                     # read back from the trainer
    assert int(sd2["backbone.0.0.1.num_batches_tracked"]) == 2
    for k in ("backbone.0.9.block.1.0.weight", "backbone.0.9.block.2.fc1.weight", "backbone.0.9.block.2.fc2.bias"):
        assert float((sd2[k] - sd0[k]).abs().max()) > 0, k                      # a 5x5 depthwise weight, the SE's matrices
    assert list(sd2) == list(sd0) and all(tuple(sd2[k].shape) == tuple(sd0[k].shape) for k in sd0)
    net = MODELS[name](cfg, is_train=False).load_state_dict(sd2).to("cuda").eval()
    x1 = T.make_batch(1, 17, 64, 64, seed=70)[0]
    got = net(x1.cuda()).cpu().numpy()
    with torch.no_grad():
        want = T.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd2.items()}, x1.double(), training=False).numpy()
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("round trip: max err %.3g, max|heat-map| %.3g" % (err, scale))
    assert got.shape == (1, 17, 16, 16) and err <= 1e-3
    same = model.eval()(x1.cuda()).cpu().numpy()
    np.testing.assert_array_equal(same, got)


@pytest.mark.parametrize("name", [PS, DC])
def test_function_train_drives_the_model(name):
    from udp_pose_amd.function import JointsMSELoss, get_optimizer, train
    cfg = _cfg(name)
    sd0 = _sd(name, 9)
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
