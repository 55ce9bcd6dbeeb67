"""RSN-18 on the stem of RSN/exps/RSN18.coco.e1.se.36x8x132000_prm end to end (``RSN18Hip(..., stem="conv7")``) against the
output of the reference's own module, unmodified (tests/golden/rsn18_se_prm_top_17.npz,
tools/gen_golden_rsn_se_prm_top.py), and the fp64 restatement (tests/rsn_top_ref.py), under the rule of
tests/test_gpu_rsn_se_prm.py::test_matches_reference_heatmaps; then the flip half and the two sub-batch lanes.  The conv7
stem without the gates has no reference fixture (no experiment of the reference combines them): it is held against the
fp64 restatement alone."""
import os

import numpy as np
import pytest
import torch

import rsn_top_ref as ref
from oracle import decode as odec
from udp_pose_amd import synth
from udp_pose_amd.inference import decode_device
from udp_pose_amd.model import RSN18Hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(golden_dir):
    g = np.load(os.path.join(golden_dir, "rsn18_se_prm_top_17.npz"))
    calib = {k[len("calib:"):]: g[k] for k in g.files if k.startswith("calib:")}
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=calib, stem="conv7")
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    truth = ref.forward(ref.to_dtype(sd, torch.float64), x.double()).numpy()
    return sd, x, g["out"], truth


@pytest.fixture(scope="module")
def nets(case):
    return {dt: RSN18Hip.from_state_dict(case[0], dtype=dt).to("cuda") for dt in ("f32", "f16x2")}


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_matches_reference_heatmaps(case, nets, dtype):
    sd, x, out, truth = case
    net = nets[dtype]
    assert (net.se, net.prm, net.stem, net.out_channels) == (True, True, "conv7", 17)
    got = net(x.cuda()).clone()
    g = got.cpu().numpy()
    ref_noise = float(np.abs(out - truth).max())
    hip_noise = float(np.abs(g - truth).max())
    print("rsn18 se+prm own stem %s: |hip - ref| %.3g, |ref - fp64| %.3g, |hip - fp64| %.3g (absmax %.3g)"
          % (dtype, float(np.abs(g - out).max()), ref_noise, hip_noise, float(np.abs(out).max())))
    assert hip_noise <= 2.0 * ref_noise + 1e-5
    np.testing.assert_allclose(g, out, rtol=0, atol=3e-3)
    c, s = synth.synth_center_scale(1, seed=4)
    rp, rm, _, ridx = odec.get_final_preds("gaussian", True, 4.0, g.copy(), c, s)
    preds, maxvals, _, idx = decode_device(got, torch.from_numpy(c.astype(np.float64)), torch.from_numpy(s.astype(np.float64)),
                                           "gaussian", True, 4.0, True)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(maxvals.cpu().numpy(), rm)
    np.testing.assert_allclose(preds.cpu().numpy(), rp, rtol=5e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_mirrored_half_is_an_explicit_mirrored_forward(nets, dtype):
    net = nets[dtype]
    xb = torch.from_numpy(synth.synth_crops(5, 256, 192, seed=9)).cuda()
    raw = net.raw_forward(xb, flip_test=True).clone()
    mir = net.raw_forward(torch.flip(xb[:2], dims=[3]).contiguous()).clone()
    assert torch.equal(mir, raw[5:7])
    assert torch.equal(net.raw_forward(xb[3:4].contiguous()).clone(), raw[3:4])        # batch independence


def test_two_lanes_equal_one_lane_at_a_time(nets):
    """20 crops run as two sub-batch lanes of 10 (f16x2, graph replay); the same crops lane by lane give the same bits."""
    net = nets["f16x2"]
    xb = torch.from_numpy(synth.synth_crops(20, 256, 192, seed=11)).cuda()
    both = net.raw_forward(xb, flip_test=True).clone()
    assert both.shape[0] == 40
    for lo in (0, 10):
        one = net.raw_forward(xb[lo:lo + 10].contiguous(), flip_test=True).clone()
        assert torch.equal(one[:10], both[lo:lo + 10]) and torch.equal(one[10:], both[20 + lo:30 + lo])


@pytest.fixture(scope="module")
def plain_case():
    """Synthetic weights of the conv7 stem without se / prm, BatchNorm statistics calibrated on 8 crops, fp64 and fp32 restatements."""
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, se=False, prm=False, stem="conv7")
    xc = torch.from_numpy(synth.synth_crops(8, 256, 192, seed=15))
    yc = ref.forward(sd, xc, se=False, prm=False, calibrate=True)
    f = 0.25 / float(yc.std())
    for k in ("stage0.upsample.up4.res_conv2.bn.weight", "stage0.upsample.up4.res_conv2.bn.bias"):
        sd[k] = sd[k] * f
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    truth = ref.forward(ref.to_dtype(sd, torch.float64), x.double(), se=False, prm=False).numpy()
    r32 = ref.forward(sd, x, se=False, prm=False).numpy()
    return sd, x, truth, r32


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_conv7_stem_without_the_gates(plain_case, dtype):
    """stem="conv7", se = prm = False.  No module of the reference has this combination, so there is no reference output:
    the bound is the first inequality of the rule with the fp32 restatement in the reference's place,
    |hip - fp64| <= 2 |restatement fp32 - fp64| + 1e-5."""
    sd, x, truth, r32 = plain_case
    net = RSN18Hip.from_state_dict(sd, dtype=dtype).to("cuda")
    assert (net.se, net.prm, net.stem) == (False, False, "conv7")
    g = net(x.cuda()).clone().cpu().numpy()
    ref_noise = float(np.abs(r32 - truth).max())
    hip_noise = float(np.abs(g - truth).max())
    print("rsn18 plain, own stem %s: |restatement fp32 - fp64| %.3g, |hip - fp64| %.3g (absmax %.3g)"
          % (dtype, ref_noise, hip_noise, float(np.abs(truth).max())))
    assert float(np.abs(truth).max()) > 0.5 and hip_noise <= 2.0 * ref_noise + 1e-5
