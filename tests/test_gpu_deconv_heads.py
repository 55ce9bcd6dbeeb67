"""pose_shufflenetv2_10x and pose_shufflenetv2_plus (the deconv-head ShuffleNets) on the GPU against the heat-maps /
get_final_preds output of the reference's own modules (tests/golden/shufflenetv2_10x_deconv.npz,
shufflenetv2_plus_small_deconv.npz), with the gates of the pixel-shuffle siblings, plus replay == eager."""
import os

import numpy as np
import pytest
import torch

from oracle import decode as odec
from udp_pose_amd import _lib, synth
from udp_pose_amd.inference import decode_device
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_shufflenet import synth_shufflenet_deconv_state_dict
from udp_pose_amd.synth_shufflenet_plus import synth_shufflenet_plus_deconv_state_dict

pytestmark = pytest.mark.gpu

HEAD = {"DECONV_WITH_BIAS": False, "NUM_DECONV_LAYERS": 3, "NUM_DECONV_FILTERS": [256, 256, 256], "NUM_DECONV_KERNELS": [4, 4, 4],
        "FINAL_CONV_KERNEL": 1}
# name -> (MODEL_SIZE, generator, fixture, the seed tools/gen_golden_shufflenet_deconv.py settled on)
NETS = {"pose_shufflenetv2_10x": ("1.0x", synth_shufflenet_deconv_state_dict, "shufflenetv2_10x_deconv.npz", 8),
        "pose_shufflenetv2_plus": ("Small", synth_shufflenet_plus_deconv_state_dict, "shufflenetv2_plus_small_deconv.npz", 7)}


def _net(name, golden_dir, dtype):
    size, synth_sd, fixture, seed = NETS[name]
    g = np.load(os.path.join(golden_dir, fixture))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_sd(seed=seed, calib=calib, final_scale=float(g["final_scale"]))
    cfg = {"MODEL": {"NAME": name, "NUM_JOINTS": 17, "TARGET_TYPE": "gaussian", "EXTRA": dict(HEAD, MODEL_SIZE=size)}}
    return MODELS[name](cfg, is_train=False, dtype=dtype).load_state_dict(sd).to("cuda").eval(), g


def _dark_shift(hm):
    coords, _, _ = odec.get_max_preds(hm)
    return np.abs(odec.post(coords, hm.copy()) - coords).max(axis=2)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_matches_reference_fixture(golden_dir, name, dtype):
    """Measured max |heat-map - fixture|: see NOTES.md (the contract is 1e-3)."""
    net, g = _net(name, golden_dir, dtype)
    hm = net(torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19)).cuda()).clone()
    got = hm.cpu().numpy()
    assert got.shape == (1, 17, 64, 48)
    err = float(np.abs(got - g["heatmaps"]).max())
    print("%s %s: max |heat-map - fixture| %.3g, %d launches" % (name, dtype, err, len(net.program(256, 192)._ops)))
    assert err <= 1e-3
    np.testing.assert_array_equal(got.reshape(1, 17, -1).argmax(2), g["heatmaps"].reshape(1, 17, -1).argmax(2))
    c, s = np.asarray(g["center"], np.float64), np.asarray(g["scale"], np.float64)
    preds, maxvals, _, _ = decode_device(hm, torch.from_numpy(c), torch.from_numpy(s), "gaussian", True, 4.0, True)
    torch.cuda.synchronize()
    assert float(np.abs(maxvals.cpu().numpy() - g["maxvals"]).max()) <= 1e-3
    # keypoints vs the reference's get_final_preds: median 1e-3 px, 2e-2 px on the joints whose Taylor step is a genuine
    # sub-pixel refinement (the siblings' tolerance, tests/test_gpu_shufflenet_plus.py)
    kerr = np.abs(preds.cpu().numpy() - g["preds"]).max(axis=2)
    good = _dark_shift(g["heatmaps"].astype(np.float32)) < 1.5
    print("keypoint error px: median %.2g, max(well-conditioned %d/%d) %.2g, max(all) %.2g"
          % (np.median(kerr), good.sum(), good.size, kerr[good].max(), kerr.max()))
    assert good.mean() > 0.5 and kerr[good].max() < 2e-2 and np.median(kerr) < 1e-3
    macs = net.program(256, 192).macs_per_image()
    assert abs(_lib.lib().udp_hrnet_flops_per_image(net._compiled[(256, 192)][0]) - 2 * macs) <= 1e-6 * macs


@pytest.mark.parametrize("name", sorted(NETS))
def test_graph_replay_equals_eager(golden_dir, name):
    net, _ = _net(name, golden_dir, "f16x2")
    xd = torch.from_numpy(synth.synth_crops(3, 64, 64, seed=9)).cuda()
    a = net.raw_forward(xd, flip_test=True).clone()
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # replay
    net.use_graph = False
    assert torch.equal(a, net.raw_forward(xd, flip_test=True))               # eager launches
    assert torch.isfinite(a).all()
