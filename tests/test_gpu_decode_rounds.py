"""decode_gaussian_kernel with two LDS planes (csrc/decode.hip: the blurred map takes the raw map's place): the batch of
the headline step -- 64 crops x 17 joints = 1088 maps of 64x48, more workgroups than the chip held in one round with
three planes -- and small maps whose blur window is wider than the map (7x5, 2x2), against oracle.decode on the same
maps.  Tolerance: that of the DARK tests in tests/test_gpu_ops.py (1e-3 px); maxvals and the arg-max indices are exact."""
import numpy as np
import pytest
import torch

from oracle import decode as odec
from udp_pose_amd import inference as uinf, synth

pytestmark = pytest.mark.gpu


def _maps(n, j, h, w, seed):
    """Heat-maps + (center, scale).  The small maps: Gaussian blobs at sub-pixel means where a blob fits (7x5), positive
    noise where it does not (2x2), and a crop box that maps one heat-map pixel to 4 image pixels, the pipeline's own ratio
    (256x192 crops, 64x48 maps).  synth_center_scale's boxes are made for 48-pixel-wide maps: on a 5-pixel-wide one they
    magnify a heat-map pixel 50 to 100 times, and the 1e-3 px gate of the image-space keypoints with it (measured with
    such boxes and noise maps: 5.3e-3 px, 1e-5 relative)."""
    if h >= 8 and w >= 8:
        return (synth.synth_heatmaps(n, j, h, w, seed=seed),) + tuple(synth.synth_center_scale(n, seed=3))
    rng = np.random.Generator(np.random.PCG64(seed))
    if h >= 5 and w >= 5:
        ys, xs = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
        mx, my = rng.uniform(1.5, w - 2.5, (n, j, 1, 1)), rng.uniform(1.5, h - 2.5, (n, j, 1, 1))
        hm = (rng.uniform(0.3, 1.0, (n, j, 1, 1)) * np.exp(-((xs - mx) ** 2 + (ys - my) ** 2) / 2.0)).astype(np.float32)
    else:
        hm = rng.uniform(0.05, 1.0, (n, j, h, w)).astype(np.float32)
    hm[0, 0] = -1.0                      # a map without a positive peak (the keypoint stays at the origin)
    hm[0, 1] = 0.5                       # a flat map: 0 / 0 in the rescale, NaN in the oracle and on the device
    c = np.tile(np.array([[2.0 * w, 2.0 * h]], dtype=np.float32), (n, 1))
    s = np.tile(np.array([[4.0 * (w - 1) / 200.0, 4.0 * (h - 1) / 200.0]], dtype=np.float32), (n, 1))
    return hm, c, s


@pytest.mark.parametrize("n,h,w", [(64, 64, 48), (3, 7, 5), (3, 2, 2)], ids=["1088x64x48", "7x5", "2x2"])
def test_decode_gaussian_matches_oracle(n, h, w):
    hm, c, s = _maps(n, 17, h, w, seed=100 + h)
    with np.errstate(all="ignore"):
        rp, rm, rpin, ridx = odec.get_final_preds("gaussian", True, 4.0, hm.copy(), c, s)
    cfg = {"MODEL": {"TARGET_TYPE": "gaussian"}, "TEST": {"POST_PROCESS": True}, "LOSS": {"KPD": 4.0}}
    before = hm.copy()
    preds, maxvals, pin, idx = uinf.get_final_preds(cfg, hm, c, s, return_idx=True)
    np.testing.assert_array_equal(hm, before)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(maxvals, rm)
    np.testing.assert_allclose(preds, rp, rtol=0, atol=1e-3, equal_nan=True)
    np.testing.assert_allclose(pin, rpin, rtol=0, atol=1e-3, equal_nan=True)
