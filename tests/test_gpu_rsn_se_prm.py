"""RSN-18 with the SELayer and the Pose Refine Machine end to end (``RSN18Hip(se=True, prm=True)``) against the output of
the reference's own modules (tests/golden/rsn18_se_prm_17.npz, tools/gen_golden_rsn_se_prm.py) and the fp64 restatement
(tests/rsn_se_prm_ref.py), under the rule of test_rsn18_matches_reference_heatmaps; then the decode, the flip half and the
two sub-batch lanes."""
import os

import numpy as np
import pytest
import torch

import rsn_se_prm_ref as ref
from oracle import decode as odec
from udp_pose_amd import synth
from udp_pose_amd.inference import decode_device
from udp_pose_amd.model import RSN18Hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(golden_dir):
    g = np.load(os.path.join(golden_dir, "rsn18_se_prm_17.npz"))
    calib = {k[len("calib:"):]: g[k] for k in g.files if k.startswith("calib:")}
    sd = synth.synth_rsn18_se_prm_state_dict(17, seed=4, bn_calib=calib)
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=8))
    truth = ref.forward(ref.to_dtype(sd, torch.float64), x.double()).numpy()
    return sd, x, g["out"], truth


@pytest.fixture(scope="module")
def nets(case):
    return {dt: RSN18Hip(17, dtype=dt, se=True, prm=True).load_state_dict(case[0]).to("cuda") for dt in ("f32", "f16x2")}


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_matches_reference_heatmaps(case, nets, dtype):
    sd, x, out, truth = case
    got = nets[dtype](x.cuda()).clone()
    g = got.cpu().numpy()
    ref_noise = float(np.abs(out - truth).max())
    hip_noise = float(np.abs(g - truth).max())
    print("rsn18 se+prm %s: |hip - ref| %.3g, |ref - fp64| %.3g, |hip - fp64| %.3g (absmax %.3g)"
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
    assert torch.equal(net.raw_forward(xb[3:4].contiguous()).clone(), raw[3:4])        # batch independence (the gates are per image)


def test_two_lanes_equal_one_lane_at_a_time(nets):
    """20 crops run as two sub-batch lanes of 10 (f16x2, graph replay); the same crops lane by lane give the same bits."""
    net = nets["f16x2"]
    xb = torch.from_numpy(synth.synth_crops(20, 256, 192, seed=11)).cuda()
    both = net.raw_forward(xb, flip_test=True).clone()
    assert both.shape[0] == 40
    for lo in (0, 10):
        one = net.raw_forward(xb[lo:lo + 10].contiguous(), flip_test=True).clone()
        assert torch.equal(one[:10], both[lo:lo + 10]) and torch.equal(one[10:], both[20 + lo:30 + lo])
