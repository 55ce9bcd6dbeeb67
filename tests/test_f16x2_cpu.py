"""The split-fp16 ("f16x2") format on the host side: the edge of fp16's range, the round-trip error away from unit
scale, and the weight encoders' refusal of anything they cannot represent.

The format: x ~= hi + lo * 2^-11 with hi = fp16(x), lo = fp16((x - hi) * 2^11).  fp16 rounds to nearest even, so every
|x| < 65520 (the midpoint of 65504 and the 2^16 fp16 cannot hold) has a finite hi, and 65520 itself is the first
magnitude whose hi is inf."""
import math

import numpy as np
import pytest
import torch

from udp_pose_amd import f16x2
from udp_pose_amd.program import encode_weights

BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))      # the largest fp32 that still splits finite


def _rt(x):
    return f16x2.decode(f16x2.encode(x))


@pytest.mark.parametrize("v", [65504.0, -65504.0, BELOW, -BELOW])
def test_round_trip_at_the_edge_of_the_range_is_finite(v):
    x = torch.tensor([[v, 1.0, -0.5, 0.0]], dtype=torch.float32)
    e = f16x2.encode(x)
    assert torch.isfinite(e.float()).all()
    got = _rt(x)
    assert torch.equal(got[0, 1:], x[0, 1:])                            # the siblings are exact
    # hi = +-65504 and lo holds the remaining 16 - 2^-8 ... rounded to fp16's 11 bits: within 2^-22 of the value
    assert abs(float(got[0, 0]) - v) <= 2.0 ** -22 * abs(v), float(got[0, 0])
    if abs(v) == 65504.0:
        assert float(got[0, 0]) == v


@pytest.mark.parametrize("v", [65520.0, -65520.0, 7e4, float("inf"), float("-inf"), float("nan")])
def test_planes_are_non_finite_from_65520_on(v):
    e = f16x2.encode(torch.tensor([[v, 1.0]], dtype=torch.float32))
    assert not torch.isfinite(e[0, 0, 0].float()), "hi plane"
    assert not torch.isfinite(e[0, 1, 0].float()), "lo plane"
    assert torch.isfinite(e[0, :, 1].float()).all()                     # the sibling is untouched
    assert not torch.isfinite(f16x2.decode(e)[0, 0])


@pytest.mark.parametrize("k", [-10, 0, 12])
def test_round_trip_error_relative_to_the_tensor_max(k):
    g = torch.Generator().manual_seed(k + 100)
    x = torch.randn(64, 257, generator=g, dtype=torch.float32) * 2.0 ** k
    assert float(x.abs().max()) < 65520.0
    got = _rt(x)
    err = float((got.double() - x.double()).abs().max()) / float(x.abs().max())
    print("k=%d: round-trip error %.3g of the tensor max" % (k, err))
    assert err <= 2.0 ** -21, err
    assert torch.equal(_rt(got), got), "decode(encode(.)) is not idempotent"


def test_round_trip_is_idempotent_up_to_the_largest_exact_value():
    """+-65504 is the largest magnitude the format holds exactly.  Above it the decoded value is not a fixed point:
    nextafter(65520, 0) is stored as 65504 + 16 and decodes to 65520.0, which itself no longer splits."""
    x = torch.tensor([[65504.0, -65504.0, 65503.99, 2.0 ** -14, 2.0 ** -24, 0.0, -0.0]], dtype=torch.float32)
    once = _rt(x)
    assert torch.equal(_rt(once), once)
    assert float(_rt(torch.tensor([[BELOW]]))[0, 0]) == 65520.0
    assert not torch.isfinite(_rt(_rt(torch.tensor([[BELOW]])))).any()


# ------------------------------------------------------------------ weights
def _weights(taps=9, cout=32, cin=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(taps, cout, cin, generator=g, dtype=torch.float32) * math.sqrt(2.0 / (taps * cin))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 32768.0, -4e4], ids=str)
@pytest.mark.parametrize("where", [(0, 0, 0), (8, 31, 31), (4, 17, 5)], ids=str)
def test_encode_weights_refuses_what_f16x2_cannot_hold(bad, where):
    wp = _weights()
    encode_weights(wp, "f16x2")                                         # the clean tensor encodes
    wp[where] = bad
    with pytest.raises(ValueError):
        encode_weights(wp, "f16x2")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=str)
@pytest.mark.parametrize("where", [(0, 0, 0), (8, 31, 31), (4, 17, 5)], ids=str)
def test_pack_weights_ws_refuses_non_finite_weights(bad, where):
    wp = _weights()
    f16x2.pack_weights_ws(wp)
    wp[where] = bad
    with pytest.raises(ValueError):
        f16x2.pack_weights_ws(wp)
    with pytest.raises(ValueError):
        f16x2.weight_exponent(wp)


def test_encode_weights_keeps_the_largest_finite_weight():
    """32768 is refused; the fp32 below it is stored exactly as the format allows."""
    wp = _weights()
    top = float(np.nextafter(np.float32(32768.0), np.float32(0.0)))
    wp[3, 3, 3] = top
    raw = np.frombuffer(encode_weights(wp, "f16x2"), dtype=np.float16).reshape(9, 32, 2, 32)
    got = raw[3, 3, 0, 3].astype(np.float64) + raw[3, 3, 1, 3].astype(np.float64) / 2048.0
    assert np.isfinite(raw.astype(np.float32)).all()
    assert abs(got - top) <= 2.0 ** -22 * top


@pytest.mark.parametrize("e", list(range(-45, 30, 3)))
def test_weight_exponent_puts_the_largest_magnitude_in_2p13_2p14(e):
    for f in (1.0, 1.5, float(np.nextafter(np.float32(2.0), np.float32(0.0)))):
        m = f * 2.0 ** e
        wp = torch.tensor([[[m * 0.25, -m, m * 0.5]]], dtype=torch.float32)
        k = f16x2.weight_exponent(wp)
        assert -40 <= k <= 40
        if -40 < k < 40:
            assert 2.0 ** 13 <= m * 2.0 ** k < 2.0 ** 14, (m, k)


def test_weight_exponent_of_zero_and_its_clamps():
    assert f16x2.weight_exponent(torch.zeros(1, 32, 32)) == 0
    assert f16x2.weight_exponent(torch.zeros(0, 32, 32)) == 0
    assert f16x2.weight_exponent(torch.full((1, 1, 1), 2.0 ** -60)) == 40
    assert f16x2.weight_exponent(torch.full((1, 1, 1), -(2.0 ** 60))) == -40
