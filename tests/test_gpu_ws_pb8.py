"""The 8-pixel-block arm of the merged weight-stationary 3x3 launch (csrc/conv_ws.hip: conv_ws_multi<3>, code 8) and the
late residual of the 3x3 stride-1 bodies, in split fp16.

Every case is a micro-program (tests/microprog.py) of 3x3 convs 32 -> 32 on the branch-0 map and 64 -> 64 on a sibling
map, sharing a launch group, listed deepest-K first as the planner lists them.  It runs twice, each time in a fresh
handle: with the chooser's default and with UDP_POSE_WS_PB8=0 (the chooser without the 8-block candidate, i.e. the
6-block / own-launch kernels), and asserts
  * the stored outputs of the two runs bit-equal (every accumulator sees the same MFMAs in the same order whatever the
    block count),
  * through the UDP_POSE_DEBUG_TILES report which arm each conv took: a conv joins a merged launch exactly when its
    report says PB=6 or PB=8 (describe_conv_ws -> groupable, hrnet.hip make_nodes),
  * each output against the fp64 conv of torch on the CPU within the conv gate of tests/test_gpu_program_ops.py
    (microprog.conv_tol: 2e-5 x scale) -- two equally wrong paths do not pass,
  * and that nothing outside the declared outputs was written.
"""
import os
import re

import numpy as np
import pytest
import torch

import microprog as mp
from microprog import Micro, new_op
from udp_pose_amd import _lib

pytestmark = pytest.mark.gpu

TILE = re.compile(r"ws conv k3 s1 (\d+)x(\d+) C(\d+)->\d+: G=(\d+) R=(\d+) TW=(\d+) CP=(\d+) PB=(\d+) lds=(\d+)")


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _program(n, maps, block, seed):
    """maps = [(c, h, w)] deepest-K first.  block = False: one grouped conv + residual + ReLU per map.  block = True: a
    BasicBlock per map -- conv1 + ReLU of every map in one group, conv2 + residual + ReLU of every map in the next."""
    m = Micro("f16x2", n, seed=seed)
    t = []
    for c, h, w in maps:
        d = dict(c=c, h=h, wid=w, bx=m.buf(h, w, c), bmid=m.buf(h, w, c) if block else None, bout=m.buf(h, w, c))
        d["x"] = m.fill(d["bx"], m.randn(n, c, h, w))
        d["wt"] = [mp.quant(m.randn(c, c, 3, 3) * float(np.sqrt(2.0 / (9 * c))), "f16x2") for _ in range(2 if block else 1)]
        d["b"] = [m.randn(c) * 0.1 for _ in d["wt"]]
        t.append(d)
    geom = lambda d: dict(ks=3, stride=1, relu=1, cin=d["c"], cout=d["c"], hin=d["h"], win=d["wid"], hout=d["h"], wout=d["wid"])
    if block:
        for d in t:
            m.add(new_op(_lib.UDP_OP_CONV, in_buf=d["bx"], out_buf=d["bmid"], group=1, **geom(d), **m.put_conv(d["wt"][0], d["b"][0], ws=True)))
            m.wrote(d["bmid"])
    for d in t:
        m.add(new_op(_lib.UDP_OP_CONV, in_buf=d["bmid"] if block else d["bx"], res_buf=d["bx"], out_buf=d["bout"], group=2,
                     **geom(d), **m.put_conv(d["wt"][-1], d["b"][-1], ws=True)))
        m.wrote(d["bout"])
    return m, t


def _run(capfd, n, maps, block, seed, pb8):
    m, t = _program(n, maps, block, seed)
    capfd.readouterr()
    with _env(UDP_POSE_DEBUG_TILES="1", UDP_POSE_WS_PB8="1" if pb8 else "0"):
        assert m.run() == 0, m.error
    err = capfd.readouterr().err
    arms = {}                                                   # (h, w, cin) -> set of (PB, R, TW, lds)
    for g in TILE.finditer(err):
        h, w, c, _, r, tw, _, pb, lds = map(int, g.groups())
        arms.setdefault((h, w, c), set()).add((pb, r, tw, lds))
    return m, t, arms


def _case(capfd, n, maps, want, block=False, seed=0):
    """want = {(h, w, c): PB} with the 8-block candidate on; without it no conv may report PB=8."""
    m1, t1, arms1 = _run(capfd, n, maps, block, seed, True)
    m0, t0, arms0 = _run(capfd, n, maps, block, seed, False)
    print("arms with the candidate:", arms1, " without:", arms0)
    for key, pb in want.items():
        assert {a[0] for a in arms1[key]} == {pb}, (key, arms1)
    assert all(a[0] != 8 for v in arms0.values() for a in v), arms0
    for d1, d0 in zip(t1, t0):
        for b in ("bmid", "bout"):
            if d1[b] is not None:
                assert np.array_equal(m1.read_raw(d1[b]), m0.read_raw(d0[b])), (d1["c"], b)
    for m, t in ((m1, t1), (m0, t0)):
        for d in t:
            x = d["x"].double()
            if block:
                mid = m.read(d["bmid"])
                ref1 = mp.ref_conv(x, d["wt"][0], d["b"][0], relu=True)
                assert not torch.isnan(mid).any(), "conv1 output not fully written"
                e1 = float((mid.double() - ref1).abs().max())
                print("C%d %dx%d conv1 err %.3g (gate %.3g)" % (d["c"], d["h"], d["wid"], e1, mp.conv_tol("f16x2", ref1)))
                assert e1 <= mp.conv_tol("f16x2", ref1), e1
                src = mid.double()                              # conv2 against the fp64 conv of conv1's output AS STORED
            else:
                src = x
            out = m.read(d["bout"])
            ref = mp.ref_conv(src, d["wt"][-1], d["b"][-1], res=x, relu=True)
            assert not torch.isnan(out).any(), "output not fully written"
            assert 0.2 < float((ref == 0).double().mean()) < 0.8          # the ReLU clips some and not all
            e = float((out.double() - ref).abs().max())
            print("C%d %dx%d n%d err %.3g (gate %.3g)" % (d["c"], d["h"], d["wid"], n, e, mp.conv_tol("f16x2", ref)))
            assert e <= mp.conv_tol("f16x2", ref), e
        m.assert_untouched()
        m.check_head()
    return arms1


def test_one_full_tile_per_image_odd_batch(capfd):
    """(a) 32x16, N = 3: one 16 x 32 tile of 512 pixels per image, beside a 6-block 64-channel sibling (24x8)."""
    arms = _case(capfd, 3, [(64, 24, 8), (32, 32, 16)], {(32, 16, 32): 8, (24, 8, 64): 6})
    assert arms[(32, 16, 32)] == {(8, 32, 16, 79872)}           # R = 32, TW = 16, halo 34 x 18 = 612 rows -> 39 groups x 2 planes


def test_workload_tile_geometry(capfd):
    """(b) 64x48, N = 2 -- the map of the W32 256x192 workload: 3 x 2 tiles of 16 columns x 32 rows per image, so
    every tile touches the border on one to three sides, and the two images give first / last tiles of the grid."""
    arms = _case(capfd, 2, [(64, 32, 24), (32, 64, 48)], {(64, 48, 32): 8, (32, 24, 64): 6}, seed=1)
    assert arms[(64, 48, 32)] == {(8, 32, 16, 79872)}


def test_falls_back_to_six_blocks(capfd):
    """(c) 48x16, N = 2: rows tile as 2 x 24, 384 pixels -- no 512-pixel tile, the 6-block arm beside the same sibling."""
    _case(capfd, 2, [(64, 24, 8), (32, 48, 16)], {(48, 16, 32): 6, (24, 8, 64): 6}, seed=2)


def test_basic_block_pair(capfd):
    """(d) a BasicBlock on each map of (a): one merged launch without a residual, one with."""
    _case(capfd, 3, [(64, 24, 8), (32, 32, 16)], {(32, 16, 32): 8, (24, 8, 64): 6}, block=True, seed=3)


def test_eight_blocks_on_a_launch_of_its_own(capfd):
    """The half-resolution sibling of a 32x16 map (16x8: 128 pixels per image) gets a 4-block tile and is not a
    member of a merged launch, so the 8-block conv runs alone -- on conv_ws_pb8_kernel, the same body."""
    _case(capfd, 3, [(64, 16, 8), (32, 32, 16)], {(32, 16, 32): 8, (16, 8, 64): 4}, seed=4)
