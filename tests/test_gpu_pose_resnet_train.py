"""PoseResNetTrainer on the GPU against torch: every parameter gradient of one step against fp64 autograd of the same
graph (tests/pose_resnet_train_ref.py), the running statistics, graphed steps against eager ones, the round trip of
the trained weights into the inference model, and a loss that goes down.

The gradient gate is measured, not chosen: the same helper runs in fp32 on the CPU, and ours may be at most 4 x as
far from fp64 as that is (or 1e-4 * max|ref|, whichever is larger) -- ours and torch's fp32 differ in summation order
only; an indexing or tie-rule bug shows at the size of max|ref|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pose_resnet_train_ref as ref                                    # noqa: E402
from oracle import resnet as oresnet                                   # noqa: E402
from udp_pose_amd.model import MODELS                                  # noqa: E402
from udp_pose_amd.resnet_plan import pose_resnet_spec                  # noqa: E402
from udp_pose_amd.synth_resnet import synth_pose_resnet_state_dict     # noqa: E402
from udp_pose_amd.train import PoseResNetTrainer                       # noqa: E402

LAYERS, FILTERS, JOINTS = (1, 1, 1, 1), (32, 32, 32), 5
KW = dict(layers=LAYERS, num_joints=JOINTS, deconv_filters=FILTERS)
SPEC = dict(layers=LAYERS, deconv_filters=FILTERS, final_kernel=1, deconv_with_bias=False)
RES50_EXTRA = {"TARGET_TYPE": "gaussian", "FINAL_CONV_KERNEL": 1, "DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3,
               "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4], "NUM_LAYERS": 50}


def _trainer(sd, spec=SPEC, joints=JOINTS, **kw):
    return PoseResNetTrainer(spec, joints, "gaussian", {k: v.clone() for k, v in sd.items()}, device="cuda", **kw)


@pytest.fixture(scope="module")
def step0():
    """One step's references, computed once: fp64 and fp32 on the CPU."""
    sd = synth_pose_resnet_state_dict(seed=11, **KW)
    batch = ref.make_batch(2, JOINTS, 96, 64, seed=23)
    r64 = ref.loss_and_grads(sd, *batch, LAYERS, torch.float64)
    r32 = ref.loss_and_grads(sd, *batch, LAYERS, torch.float32)
    return sd, batch, r64, r32


def test_gradients_loss_and_running_statistics_match_fp64_autograd(step0):
    sd, (x, tg, tw), (loss64, y64, g64, sd64), (_, _, g32, _) = step0
    tr = _trainer(sd)
    heat = tr.forward(x.cuda())
    loss, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss.cpu()[0]), loss64, rtol=1e-5)
    np.testing.assert_allclose(heat.cpu().numpy(), y64.numpy(), atol=1e-3)
    assert list(g64) == tr._keys
    bad = []
    for k in tr._keys:
        exact = g64[k].numpy()
        mx = float(np.abs(exact).max())
        e_ours = float(np.abs(tr.grad_of(k).cpu().double().numpy() - exact).max())
        e_f32 = float(np.abs(g32[k].double().numpy() - exact).max())
        gate = max(4 * e_f32, 1e-4 * mx)
        print("%-32s max|ref| %.3e  fp32-CPU err %.3e  ours %.3e  gate %.3e" % (k, mx, e_f32, e_ours, gate))
        if not e_ours <= gate:
            bad.append((k, e_ours, gate))
    assert not bad, bad
    # running statistics: rtol 1e-5, taken against the tensor's scale as well as the element's own value.  A running mean
    # is the mean of an O(1) map and may nearly cancel: torch's own fp32 CPU run of this step is 3.6e-4 RELATIVE (1.6e-7
    # absolute) off fp64 at layer4.0.bn2.running_mean, where max|ref| is 0.116 -- 39 of its 512 elements miss an
    # element-wise rtol of 1e-5, which no fp32 evaluation can hold there.
    got = tr.state_dict()
    for k in ("bn1", "layer4.0.bn2", "deconv_layers.4"):
        for s in (".running_mean", ".running_var"):
            want = sd64[k + s].numpy()
            np.testing.assert_allclose(got[k + s].numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()), err_msg=k + s)
    assert int(got["bn1.num_batches_tracked"]) == 0             # no optimizer step yet


def test_deconv_bias_and_3x3_final_layer_gradients():
    """DECONV_WITH_BIAS and FINAL_CONV_KERNEL 3: the two head options the default spec leaves out, same gate."""
    kw = dict(KW, deconv_with_bias=True, final_kernel=3)
    spec = dict(SPEC, deconv_with_bias=True, final_kernel=3)
    sd = synth_pose_resnet_state_dict(seed=12, **kw)
    x, tg, tw = ref.make_batch(2, JOINTS, 64, 64, seed=29)
    _, _, g64, _ = ref.loss_and_grads(sd, x, tg, tw, LAYERS, torch.float64)
    _, _, g32, _ = ref.loss_and_grads(sd, x, tg, tw, LAYERS, torch.float32)
    tr = _trainer(sd, spec=spec)
    heat = tr.forward(x.cuda())
    _, d = tr.loss_and_grad(heat, tg.cuda(), tw.cuda())
    tr.backward(d)
    torch.cuda.synchronize()
    for k in ("deconv_layers.0.bias", "deconv_layers.6.bias", "deconv_layers.3.weight", "final_layer.weight", "final_layer.bias",
              "layer1.0.conv1.weight", "conv1.weight"):
        exact = g64[k].numpy()
        e_ours = float(np.abs(tr.grad_of(k).cpu().double().numpy() - exact).max())
        e_f32 = float(np.abs(g32[k].double().numpy() - exact).max())
        assert e_ours <= max(4 * e_f32, 1e-4 * float(np.abs(exact).max())), (k, e_ours, e_f32)


def test_graphed_steps_equal_eager_steps(step0):
    sd = step0[0]
    batches = [ref.make_batch(2, JOINTS, 96, 64, seed=40 + k) for k in range(3)]
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
    sd, (x, tg, tw) = step0[0], step0[1]
    tr = _trainer(sd, lr=1e-3)
    x, tg, tw = x.cuda(), tg.cuda(), tw.cuda()
    losses = [float(tr.train_step_graphed(x, tg, tw).cpu()[0]) for _ in range(20)]
    print("loss: first %.5g, last %.5g" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_trained_res50_round_trips_into_the_inference_model(golden_dir):
    """Two steps of the real depth, then ``state_dict()`` into ``MODELS["pose_resnet"](cfg, is_train=False)``: its eval
    forward against the same weights through the CPU oracle, to what test_res50_matches_reference_fixture allows."""
    import os
    g = np.load(os.path.join(golden_dir, "resnet50_cfg0.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd0 = synth_pose_resnet_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    cfg = {"MODEL": {"NAME": "pose_resnet", "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": RES50_EXTRA}}
    model = MODELS["pose_resnet"](cfg, is_train=True).load_state_dict(sd0).to("cuda")
    model.train()
    tr = model.trainer()
    assert isinstance(tr, PoseResNetTrainer) and tr.spec["layers"] == pose_resnet_spec(RES50_EXTRA)["layers"]
    assert model.parameters()[0].data_ptr() == tr.flat.data_ptr()
    for k in range(2):
        x, tg, tw = ref.make_batch(2, 17, 64, 64, seed=60 + k)
        assert tuple(model(x.cuda()).shape) == (2, 17, 16, 16)                   # train-mode __call__
        tr.train_step(x.cuda(), tg.cuda(), tw.cuda())
    sd2 = model.state_dict()                                                     # read back from the trainer
    assert int(sd2["bn1.num_batches_tracked"]) == 2
    assert float((sd2["layer4.2.conv3.weight"] - sd0["layer4.2.conv3.weight"]).abs().max()) > 0
    net = MODELS["pose_resnet"](cfg, is_train=False).load_state_dict(sd2).to("cuda").eval()
    x1 = ref.make_batch(1, 17, 64, 64, seed=70)[0]
    got = net(x1.cuda()).cpu().numpy()
    want = oresnet.pose_resnet_forward({k: v.clone() for k, v in sd2.items()}, x1).numpy()
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("round trip: max err %.3g, max|heat-map| %.3g" % (err, scale))
    assert got.shape == (1, 17, 16, 16) and err <= 1e-3
    # the trained model itself, back in eval mode, runs the moved weights too
    same = model.eval()(x1.cuda()).cpu().numpy()
    np.testing.assert_array_equal(same, got)
