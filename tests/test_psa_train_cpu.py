"""Host-side checks of pose_hrnet_psa training that need no GPU: argument validation of the udp_psa_train_* entry
points, and the trainer's parameter bookkeeping (key list, offsets, gradient buckets) with and without ``psa``."""
import ctypes as C

import pytest
import torch

from udp_pose_amd import _lib, synth
from udp_pose_amd.train import HRNetTrainer, _is_param

EXTRA = synth.scaled_extra(32, modules=(1, 2, 1), blocks=2)
CFG = {"MODEL": {"EXTRA": EXTRA, "NUM_JOINTS": 5, "TARGET_TYPE": "offset"}}
FNS = ("udp_psa_train_fwd_pool", "udp_psa_train_fwd_sp", "udp_psa_train_bwd_sp", "udp_psa_train_bwd_pool",
       "udp_psa_train_bwd_params")


def _args(c=32, n=2, h=8, w=6, fill=0x1000):
    """Every pointer a non-null dummy (nothing is launched when validation fails)."""
    a = _lib.PsaTrainArgs()
    for i in range(9):
        a.w[i], a.dw[i] = fill, fill
    for k in ("x", "x1", "theta", "x2", "dx2", "dtheta", "dx1", "dx", "save"):
        setattr(a, k, fill)
    a.save_floats = 1 << 30
    a.n, a.h, a.w_px, a.c = n, h, w, c
    return a


def _err():
    return _lib.lib().udp_last_error().decode()


@pytest.mark.parametrize("fn", FNS)
def test_psa_train_entry_points_validate_arguments(fn):
    f = getattr(_lib.lib(), fn)
    assert f(None, _lib.UDP_F32, None) == -1 and "null pointer" in _err()
    for c in (16, 48, 512, 0):                                  # outside the supported channel counts
        rc = f(C.byref(_args(c=c)), _lib.UDP_F32, None)
        assert rc == (-1 if c == 0 else -3), (fn, c, rc)
    assert "must divide 256" in _err() or "shape" in _err()
    assert f(C.byref(_args(n=0)), _lib.UDP_F32, None) == -1
    assert f(C.byref(_args()), _lib.UDP_F16X2, None) == -3 and "f32 or bf16" in _err()
    assert f(C.byref(_args()), 7, None) == -1 and "dtype" in _err()
    a = _args()
    a.save = None
    assert f(C.byref(a), _lib.UDP_F32, None) == -1 and "save" in _err()
    a = _args()
    a.save_floats = 16
    assert f(C.byref(a), _lib.UDP_F32, None) == -4 and "needed" in _err()


@pytest.mark.parametrize("fn,field", [("udp_psa_train_fwd_pool", "x"), ("udp_psa_train_fwd_pool", "x1"),
                                      ("udp_psa_train_fwd_sp", "theta"), ("udp_psa_train_fwd_sp", "x2"),
                                      ("udp_psa_train_bwd_sp", "dx2"), ("udp_psa_train_bwd_sp", "dtheta"),
                                      ("udp_psa_train_bwd_sp", "dx1"), ("udp_psa_train_bwd_pool", "dx1"),
                                      ("udp_psa_train_bwd_pool", "dx")])
def test_psa_train_entry_points_refuse_null_maps(fn, field):
    a = _args()
    setattr(a, field, None)
    assert getattr(_lib.lib(), fn)(C.byref(a), _lib.UDP_F32, None) == -1
    assert "null pointer" in _err()


def test_psa_train_null_parameters_and_gradients():
    L = _lib.lib()
    a = _args()
    a.w[4] = None
    assert L.udp_psa_train_fwd_pool(C.byref(a), _lib.UDP_F32, None) == -1 and "parameter 4" in _err()
    a = _args()
    a.dw[8] = None
    assert L.udp_psa_train_bwd_params(C.byref(a), _lib.UDP_F32, None) == -1 and "gradient 8" in _err()


def test_psa_train_save_area_size():
    L = _lib.lib()
    assert L.udp_psa_train_save_floats(2, 8, 6, 16) == 0 and "must divide 256" in _err()
    assert L.udp_psa_train_save_floats(0, 8, 6, 32) == 0
    small, big = L.udp_psa_train_save_floats(2, 8, 6, 32), L.udp_psa_train_save_floats(32, 64, 48, 32)
    assert 0 < small < big and small % 2 == 0 and big % 32 == 0
    assert big >= 32 * 3 * 64 * 48                                # three per-pixel rows per image


def _trainer(psa):
    sd = synth.synth_state_dict(EXTRA, 5, "offset", seed=1, psa=psa)
    return HRNetTrainer(CFG, sd, device="cpu", psa=psa)


def test_trainer_key_list_covers_the_attention_parameters():
    tr = _trainer(True)
    shapes = synth.hrnet_param_shapes(EXTRA, 5, "offset", psa=True)
    assert tr._keys == [k for k in shapes if _is_param(k)]
    att = [k for k in tr._keys if ".deattn." in k]
    n_blocks = sum(1 for k in shapes if k.endswith(".deattn.conv_q_right.weight"))
    assert n_blocks > 0 and len(att) == 10 * n_blocks
    for k in att:                                                # every attention tensor is in a gradient bucket
        lo, hi, _ = tr._buckets[tr._bucket_of[k]]
        assert lo <= tr._off[k] and tr._off[k] + int(torch.tensor(shapes[k]).prod()) <= hi
        assert tr._off[k] % 4 == 0
    assert sum(cnt for _, _, cnt in tr._buckets) == len(tr._keys)
    # the LayerNorm tensors keep their 3-D shape through param() / state_dict()
    k = att[4]
    assert k.endswith("conv_up.1.weight") and tuple(tr.param(k).shape) == shapes[k] and len(shapes[k]) == 3
    sd = tr.state_dict()
    assert set(sd) == set(shapes) and tuple(sd[k].shape) == shapes[k]
    # only theta's 1x1 conv goes through the packed conv operands
    packed = [k for k in tr._convs if ".deattn." in k]
    assert len(packed) == n_blocks and all(k.endswith(".conv_v_left") for k in packed)


def test_trainer_without_psa_is_unchanged():
    tr = _trainer(False)
    shapes = synth.hrnet_param_shapes(EXTRA, 5, "offset")
    assert tr._keys == [k for k in shapes if _is_param(k)] and not any(".deattn." in k for k in tr._keys)
    n = 0
    for k in tr._keys:                                           # offsets: consecutive, each rounded up to 4 floats
        assert tr._off[k] == n
        numel = 1
        for d in shapes[k]:
            numel *= d
        n += (numel + 3) // 4 * 4
    assert tr._n_param == n and tr.psa is False
    # the plain trainer's offsets are a prefix-compatible subset: the PSA trainer only inserts tensors
    tp = _trainer(True)
    assert [k for k in tp._keys if ".deattn." not in k] == tr._keys


def test_model_init_weights_leaves_layernorm_at_its_default():
    from udp_pose_amd.model import MODELS
    cfg = {"MODEL": {"EXTRA": EXTRA, "NUM_JOINTS": 5, "TARGET_TYPE": "offset", "INIT_WEIGHTS": True, "PRETRAINED": ""}}
    sd = MODELS["pose_hrnet_psa"](cfg, is_train=True)._sd
    ln_w = [k for k in sd if k.endswith(".deattn.conv_up.1.weight")]
    assert ln_w
    for k in ln_w:
        assert float(sd[k].min()) == 1.0 == float(sd[k].max())
        assert float(sd[k[:-6] + "bias"].abs().max()) == 0.0
