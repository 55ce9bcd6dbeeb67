"""CPU self-checks of tests/microprog.py: its PSA reference against the project's oracle, its workspace arithmetic
against the layout rule of csrc/hrnet.hip, and the conditioning of the PSA cases tests/test_gpu_program_ops.py runs."""
import numpy as np
import pytest
import torch

import microprog as mp
from oracle import hrnet as ohrnet


def test_psa_reference_equals_oracle():
    """microprog.psa_block in fp32 == oracle.hrnet._psa_s (the path behind tests/golden/hrnet_psa_mini.npz) to 1e-6."""
    c, h, w, n = 32, 9, 7, 3
    x, _, P = mp.psa_inputs(c, h, w, n, seed=5)
    wt = torch.randn(c // 2, c, 1, 1, generator=torch.Generator().manual_seed(1)) / np.sqrt(c)
    p = "a"
    sd = {p + ".conv_q_right.weight": P["wq"].reshape(1, c, 1, 1), p + ".conv_v_right.weight": P["wv"].reshape(c // 2, c, 1, 1),
          p + ".conv_up.0.weight": P["w1"].reshape(c // 8, c // 2, 1, 1), p + ".conv_up.0.bias": P["b1"],
          p + ".conv_up.1.weight": P["ln_g"].reshape(c // 8, 1, 1), p + ".conv_up.1.bias": P["ln_b"].reshape(c // 8, 1, 1),
          p + ".conv_up.3.weight": P["w2"].reshape(c, c // 8, 1, 1), p + ".conv_up.3.bias": P["b2"],
          p + ".conv_q_left.weight": P["wg"].reshape(c // 2, c, 1, 1), p + ".conv_v_left.weight": wt}
    want = ohrnet._psa_s(ohrnet._Net(sd), x, p)
    got = mp.psa_block(x, P, wt)
    assert float(want.abs().max()) > 0.1
    assert float((got - want).abs().max()) <= 1e-6
    # the parameter block has the order and size csrc/psa.hip (PsaW) reads
    assert len(mp.psa_block_bytes(P)) == 4 * (c + c // 2 * c + c // 8 * (c // 2) + 3 * (c // 8) + c * (c // 8) + c + c // 2 * c)


@pytest.mark.parametrize("dtype,es", [("f32", 4), ("bf16", 2), ("f16x2", 4)])
def test_workspace_offsets_follow_the_layout_rule(dtype, es):
    """Buffer b starts at buf_off[b] * B * esize, buf_off = prefix sum of buf_elems rounded up to 64."""
    elems, batch = [8 * 6 * 16, 100, 64], 3
    offs, total = mp.buffer_offsets(elems, batch, dtype)
    assert offs == [0, 768 * batch * es, (768 + 128) * batch * es]
    assert total == ((768 + 128 + 64) * batch * es + 255) // 256 * 256


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16x2"])
def test_units_round_trip(dtype):
    t = torch.randn(2, 3, 5, 8, generator=torch.Generator().manual_seed(2))
    q = mp.quant(t, dtype)
    back = mp.from_units(mp.to_units(q, dtype), dtype, t.shape)
    assert torch.equal(back, q)
    if dtype == "f32":
        assert torch.equal(q, t)
    poison = mp.from_units(np.full(mp.to_units(q, dtype).size, mp.POISON16, np.int16), dtype, t.shape)
    assert torch.isnan(poison).all()


# the PSA cases of tests/test_gpu_program_ops.py (C, h, w); n = 3 each
PSA_CASES = [(16, 8, 6), (32, 16, 12), (64, 9, 7), (128, 8, 6), (256, 8, 6), (32, 64, 48)]


@pytest.mark.parametrize("c,h,w", PSA_CASES)
def test_psa_cases_are_neither_flat_nor_one_hot(c, h, w):
    """Spread-4 parameters: the largest weight of both soft-maxes lies between 2/HW and 0.9; the channel mask and the
    spatial gate are not saturated either."""
    x, theta, P = mp.psa_inputs(c, h, w, 3)
    x, theta = x.double(), theta.double()
    hw = h * w
    q = torch.softmax(torch.einsum("c,ncp->np", P["wq"].double(), x.reshape(3, c, hw)), dim=1)
    sm = torch.softmax(theta.reshape(3, c // 2, hw), dim=2)
    for top in (float(q.max()), float(sm.max())):
        assert 2.0 / hw < top < 0.9, top
    mask = mp.psa_mlp(mp.psa_pool(x, P), P)
    m = mask[:, :c]
    assert 0.02 < float(m.min()) and float(m.max()) < 0.98 and float(m.max() - m.min()) > 0.2
    s = mp.psa_sp(theta, torch.ones(3, c, h, w, dtype=torch.float64), mask)
    assert float(s.max() - s.min()) > 0.1 and 0.001 < float(s.min()) and float(s.max()) < 0.999, (float(s.min()), float(s.max()))


def test_psa_peaked_case_is_peaked():
    x, theta, P = mp.psa_inputs(32, 16, 12, 3, spread=40.0)
    q = torch.einsum("c,ncp->np", P["wq"].double(), x.double().reshape(3, 32, 192))
    assert float((q.max(dim=1).values - q.min(dim=1).values).min()) > 25
    assert float(torch.softmax(q, dim=1).max()) > 0.9
