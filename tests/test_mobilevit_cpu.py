"""pose_mobilevit_pixel_shuffle on the host side, no GPU: the restatement against the fixture the reference's own module
produced, the weight-file contract, the model factory, the op program the planner emits (launch count and kinds,
activation codes, residuals, the encoder's seven launches, the never-copied concat, every key consumed, MACs) and the
refused configurations."""
import collections
import os

import numpy as np
import pytest
import torch

import mobilevit_ref as R
from udp_pose_amd import _lib, synth
from udp_pose_amd.model import MODELS
from udp_pose_amd.synth_mobilevit import mobilevit_param_shapes, mobilevit_widths, synth_mobilevit_state_dict

NAME = "pose_mobilevit_pixel_shuffle"
S = _lib.UDP_ACT_SILU
K = _lib


def _cfg(size="xxs", target="gaussian", **model):
    return {"MODEL": dict({"NAME": NAME, "NUM_JOINTS": 17, "TARGET_TYPE": target, "IMAGE_SIZE": [192, 256],
                           "EXTRA": {"START_CHANNELS": 256, "ARCHITECTURE": (512, 256, 128), "MODEL_SIZE": size, "FINAL_CONV_KERNEL": 1}},
                          **model)}


def _program(size, h, w, dtype, seed=7):
    from udp_pose_amd.mobilevit_plan import MobileViTProgram, mobilevit_spec
    sd = synth_mobilevit_state_dict(seed=seed, model_size=size)
    return sd, MobileViTProgram(sd, mobilevit_spec(_cfg(size)["MODEL"]["EXTRA"]), h, w, dtype)


def test_restatement_equals_reference_fixture(golden_dir):
    """The fixture holds the reference module's fp64 forward (tools/gen_golden_mobilevit.py); the restatement in fp64 is
    within 1e-5 of it (measured 6e-8) and in fp32 within 1e-4 (measured 8.4e-6).  The reference module's own
    |fp32 - fp64| is 7.3e-6 for this net, below 1e-4, so the fp32 bound stays at 1e-4."""
    g = np.load(os.path.join(golden_dir, "mobilevit_xxs_ps.npz"))
    calib = {k[len("calib_"):]: g[k] for k in g.files if k.startswith("calib_")}
    sd = synth_mobilevit_state_dict(seed=7, calib=calib, final_scale=float(g["final_scale"]))
    assert sorted("%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in sd.items()) == list(g["keys"])   # the weight-file contract
    # 332 keys, 2,910,524 elements: what the reference's xxs module registers
    assert len(sd) == 332 and sum(v.numel() for v in sd.values()) == 2910524
    x = torch.from_numpy(synth.synth_crops(1, 256, 192, seed=19))
    hm = R.forward(sd, x, dtype=torch.float64).numpy()
    assert hm.shape == g["heatmaps"].shape == (1, 17, 64, 48)
    assert float(np.abs(hm - g["heatmaps"]).max()) <= 1e-5
    assert float(np.abs(R.forward(sd, x).numpy() - g["heatmaps"]).max()) <= 1e-4


def _unfold(t):
    """MobileViTBlock.unfolding (mobilevit.py:593-621) for 2x2 patches: [B, C, H, W] -> [B P, N, C]."""
    b, c, h, w = t.shape
    nh, nw = h // 2, w // 2
    t = t.reshape(b * c * nh, 2, nw, 2).transpose(1, 2).reshape(b, c, nh * nw, 4).transpose(1, 3)
    return t.reshape(b * 4, nh * nw, c)


def _fold(p, b, h, w):
    """MobileViTBlock.folding (:634-652): [B P, N, C] -> [B, C, H, W]."""
    nh, nw = h // 2, w // 2
    c = p.shape[-1]
    p = p.contiguous().view(b, 4, nh * nw, c).transpose(1, 3)
    return p.reshape(b * c * nh, nw, 2, 2).transpose(1, 2).reshape(b, c, h, w)


def test_map_form_equals_unfold_form():
    """What the HIP program relies on: per-pixel LayerNorm and the attention core on the map equal the reference's
    unfold -> [B P, N, C] -> fold form (mobilevit.py:593-655, :426-457) in fp64 to 1e-13, and folding hd^-0.5 into the q
    rows of qkv_proj equals scaling q afterwards.  8x6 map, d = 24, 4 heads (head width 6)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    b, d, h, w, heads = 2, 24, 8, 6, 4
    hd = d // heads
    x = torch.randn(b, d, h, w, generator=g, dtype=torch.float64) + 3
    gam, bet = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
    assert torch.equal(_fold(_unfold(x), b, h, w), x)
    ln = _fold(F.layer_norm(_unfold(x), (d,), gam, bet, 1e-5), b, h, w)
    assert float((ln - R.layer_norm_map(x, gam, bet)).abs().max()) <= 1e-13
    wq, bq = torch.randn(3 * d, d, generator=g, dtype=torch.float64) * 0.3, torch.randn(3 * d, generator=g, dtype=torch.float64) * 0.1
    # the reference's forward_other on the unfolded tokens (:426-457), out_proj left out
    tok = _unfold(ln)
    bp, n, _ = tok.shape
    qkv = (tok @ wq.t() + bq).reshape(bp, n, 3, heads, -1).transpose(1, 3)
    q, k, v = qkv[:, :, 0] * hd ** -0.5, qkv[:, :, 1], qkv[:, :, 2]
    ref = (torch.softmax(q @ k.transpose(2, 3), dim=-1) @ v).transpose(1, 2).reshape(bp, n, -1)
    ref = _fold(ref, b, h, w)
    m = F.conv2d(ln, wq[:, :, None, None], bq)
    got = R.mha_core(m[:, :d] * hd ** -0.5, m[:, d:2 * d], m[:, 2 * d:], heads)
    assert float((got - ref).abs().max()) <= 1e-13
    ws, bs = wq.clone(), bq.clone()
    ws[:d] *= hd ** -0.5
    bs[:d] *= hd ** -0.5
    m = F.conv2d(ln, ws[:, :, None, None], bs)
    assert float((R.mha_core(m[:, :d], m[:, d:2 * d], m[:, 2 * d:], heads) - ref).abs().max()) <= 1e-13


def test_models_has_the_net():
    net = MODELS[NAME](_cfg(CONFIG="lib/models/backbones/configs/mobilevit_xxs.yaml"), is_train=False)   # KeyError before this net existed; MODEL.CONFIG is ignored
    from udp_pose_amd.model import PoseMobileViTHip
    assert isinstance(net, PoseMobileViTHip)
    sd = synth_mobilevit_state_dict(seed=7)
    net.load_state_dict({"module." + k: v for k, v in sd.items()})             # DataParallel prefixes are stripped
    bad = dict(sd)
    del bad["backbone.layer_4.1.global_rep.2.pre_norm_mha.1.qkv_proj.bias"]
    with pytest.raises(RuntimeError, match="missing"):
        net.load_state_dict(bad)
    for refused in (net.trainer, net.train, net.init_weights):                 # training is refused by name
        with pytest.raises(NotImplementedError, match=NAME):
            refused()


def test_widths_follow_the_reference_configuration():
    assert mobilevit_widths("xxs") == (16, 16, 24, 2, [(48, 64, 128, 2), (64, 80, 160, 4), (80, 96, 192, 3)])
    assert mobilevit_widths("xs") == (16, 32, 48, 4, [(64, 96, 192, 2), (80, 120, 240, 4), (96, 144, 288, 3)])
    assert mobilevit_widths("s") == (16, 32, 64, 4, [(96, 144, 288, 2), (128, 192, 384, 4), (160, 240, 480, 3)])
    # key and element counts of the reference module's state_dict at the three widths (tools/gen_golden_mobilevit.py)
    for size, elems in (("xxs", 2910524), ("xs", 3977068), ("s", 7307196)):
        shapes = mobilevit_param_shapes(model_size=size)
        assert len(shapes) == 332 and sum(int(np.prod(s)) for s in shapes.values()) == elems


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(256, 192), (64, 64)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", ["xxs", "xs", "s"])
def test_program_census_keys_and_launch_count(size, hw, dtype):
    from udp_pose_amd.mobilevit_plan import N_LAUNCHES, MobileViTProgram
    sd, prog = _program(size, hw[0], hw[1], dtype)
    ops = prog._ops
    kinds = [op["kind"] for op in ops]
    c0, c1, c2, exp, mit = mobilevit_widths(size)
    up = lambda c: (c + 31) // 32 * 32
    # hand count: stem 1 + layer 1 (3) + layer 2 (3 x 3) + layers 3-5 (3 for the InvertedResidual + [conv3x3, ACT, conv1x1,
    # 7 per encoder, LNORM, conv_proj, fusion, ACT]) + conv_1x1_exp 1 + conv_compress 1 + 3 x (DUC conv + shuffle) 6 + head 1
    assert len(ops) == 1 + 3 + 9 + sum(3 + 3 + 7 * n + 4 for _, _, _, n in mit) + 1 + 1 + 6 + 1 == 115 == N_LAUNCHES
    assert kinds[0] == K.UDP_OP_STEM and collections.Counter(kinds) == {
        K.UDP_OP_STEM: 1, K.UDP_OP_CONV: 68, K.UDP_OP_DWCONV: 7, K.UDP_OP_LNORM: 21, K.UDP_OP_MHATTN: 9, K.UDP_OP_ACT: 6,
        K.UDP_OP_PIXSHUF: 3}
    # every encoder: LNORM, qkv conv, MHATTN, out_proj + residual, LNORM, ffn + SiLU, ffn + residual
    at = [i for i, k in enumerate(kinds) if k == K.UDP_OP_MHATTN]
    for i in at:
        u = ops[i - 2:i + 5]
        assert [o["kind"] for o in u] == [K.UDP_OP_LNORM, K.UDP_OP_CONV, K.UDP_OP_MHATTN, K.UDP_OP_CONV, K.UDP_OP_LNORM, K.UDP_OP_CONV, K.UDP_OP_CONV]
        assert [o["relu"] for o in u] == [0, 0, 0, 0, 0, S, 0]
        assert u[3]["res"] is u[0]["inp"] and u[6]["res"] is u[3]["out"] and u[4]["inp"] is u[3]["out"]
        assert u[1]["inp"] is u[0]["out"] and u[2]["inp"] is u[1]["out"] and u[3]["inp"] is u[2]["out"] and u[2]["out"] is not u[2]["inp"]
        dp = u[2]["cout"]
        assert u[2]["ks"] == 2 and u[2]["cin"] == u[1]["cout"] == 3 * dp and dp % 32 == 0 and u[2]["hout"] % 2 == 0 and u[2]["wout"] % 2 == 0
        assert u[2]["heads"] == 4 and u[2]["chain_cout"] == u[0]["chain_cout"] == u[4]["chain_cout"] and u[0]["out"] is not u[0]["inp"]
    dims = [d for _, d, _, n in mit for _ in range(n)]
    assert [ops[i - 2]["chain_cout"] for i in at] == dims                        # LayerNorm and the attention get the REAL width
    assert [ops[i]["cout"] for i in at] == [up(d) for d in dims]
    ln = [op for op in ops if op["kind"] == K.UDP_OP_LNORM]
    assert [op["chain_cout"] for op in ln] == [d for _, d, _, n in mit for _ in range(2 * n + 1)]
    # every 3x3 conv has activation code 0 (or the DUC's ReLU) -- the MobileViT blocks' six are followed by an in-place ACT
    c3 = [i for i, op in enumerate(ops) if op["kind"] == K.UDP_OP_CONV and op["ks"] == 3]
    assert len(c3) == 6 + 3 and all(ops[i]["relu"] in (0, 1) for i in c3)
    blk3 = [i for i in c3 if not ops[i]["name"].startswith("decoder.")]
    assert len(blk3) == 6 and all(ops[i]["relu"] == 0 for i in blk3)
    for i in blk3:
        a = ops[i + 1]
        assert a["kind"] == K.UDP_OP_ACT and a["relu"] == S and a["inp"] is ops[i]["out"] and a["out"] is a["inp"]
    assert [i - 1 for i, k in enumerate(kinds) if k == K.UDP_OP_ACT] == blk3
    # the concat of the fusion conv is never copied: its one input tensor was written in two halves, by the
    # InvertedResidual before the block (first half) and by conv_proj (second half); the block's first conv reads a view
    for n, i in enumerate(blk3[1::2]):
        fus, first = ops[i], ops[blk3[2 * n]]
        cat, cp = fus["inp"], up(mit[n][0])
        assert cat.c == 2 * cp == fus["cin"] and fus["in_pitch"] == 0 and fus["cout"] == cp
        writers = [(o["name"], o["out_coff"], o["out_pitch"], o["cout"]) for o in ops if o["out"] is cat]
        assert writers == [("backbone.layer_%d.0.block.red_1x1" % (n + 3), 0, 2 * cp, cp), ("backbone.layer_%d.1.conv_proj" % (n + 3), cp, 2 * cp, cp)]
        assert first["inp"] is cat and (first["in_coff"], first["in_pitch"], first["cin"]) == (0, 2 * cp, cp)
        assert ops[i - 1]["name"].endswith("conv_proj") and ops[i - 1]["relu"] == S and ops[i - 2]["kind"] == K.UDP_OP_LNORM
    # SiLU: the stem, the two first convs of the 7 InvertedResiduals, the first ffn conv of the 9 encoders, the 3 conv_proj,
    # conv_1x1_exp, the 6 ACT launches -- and no conv with a residual
    silu = [op for op in ops if op["relu"] == S]
    assert len(silu) == 1 + 7 * 2 + 9 + 3 + 1 + 6 and all(op["res"] is None for op in silu)
    assert all(op["ks"] == 1 and op["stride"] == 1 for op in silu if op["kind"] == K.UDP_OP_CONV)
    assert all(op["relu"] == S for op in ops if op["kind"] == K.UDP_OP_DWCONV)
    assert {op["relu"] for op in ops} == {0, 1, S}
    assert [op["stride"] for op in ops if op["kind"] == K.UDP_OP_DWCONV] == [1, 2, 1, 1, 2, 2, 2]
    # residuals: layer_2.1, layer_2.2, two per encoder -- and at xxs (16 -> 16) layer_1.0, whose shortcut is a channel
    # view of the 64-channel stem tensor
    res = [op for op in ops if op["res"] is not None]
    assert len(res) == 2 + 2 * 9 + (1 if size == "xxs" else 0)
    l1 = next(op for op in ops if op["name"] == "backbone.layer_1.0.block.red_1x1")
    if size == "xxs":
        assert l1["res"] is ops[0]["out"] and (l1["res_coff"], l1["res_pitch"], l1["res_c"], l1["cout"]) == (0, 64, 32, 32)
    else:
        assert l1["res"] is None
    assert all(op["res_pitch"] == 0 for op in res if op is not l1)
    # every key is consumed or explicitly accepted and unused (the ImageNet classifier, the BatchNorm step counters)
    assert prog.consumed_keys == set(mobilevit_param_shapes(model_size=size)) == set(sd)
    assert {k for k in prog.unused_keys if not k.endswith("num_batches_tracked")} == {"backbone.classifier.fc.weight", "backbone.classifier.fc.bias"}
    for k in list(sd):
        if k.startswith("backbone.classifier."):
            del sd[k]
    assert len(MobileViTProgram(sd, prog.spec, hw[0], hw[1], dtype)._ops) == 115
    head = ops[-1]
    assert head["name"] == "final_layer" and head["out"] is None and head["cout"] == 17 == prog.out_channels
    arr = prog.ops_array()
    assert arr[len(arr) - 1].out_buf == K.UDP_BUF_OUTPUT
    assert all(o.cin == o.cout == o.cout_pad and o.cin % 32 == 0 and 1 <= o.chain_cout <= o.cin and o.in_buf != o.out_buf
               for o in arr if o.kind == K.UDP_OP_LNORM)
    assert all(o.cin == 3 * o.cout and o.up_shift[0] == 4 and o.n_up == 0 and o.in_buf != o.out_buf and o.chain_cout % 4 == 0
               for o in arr if o.kind == K.UDP_OP_MHATTN)
    assert all(o.in_buf == o.out_buf and o.cin == o.cout == o.cout_pad for o in arr if o.kind == K.UDP_OP_ACT)
    assert all(o.cin % 32 == 0 and o.cout_pad % 32 == 0 for o in arr if o.kind == K.UDP_OP_CONV)
    # a reader on another lane than its producer waits for it
    producer = {}
    for i, op in enumerate(ops):
        for t in prog._reads(op):
            w = producer[t.id]
            assert ops[w]["lane"] == op["lane"] or w in op["wait"], op["name"]
        if op["out"] is not None:
            producer[op["out"].id] = i


def test_macs_per_image_hand_count():
    """xxs at 256x192, counted as launched (padded channel counts; the attention with its real width)."""
    _, prog = _program("xxs", 256, 192, "f32")
    up = lambda c: (c + 31) // 32 * 32
    c0, c1, c2, exp, mit = mobilevit_widths("xxs")
    macs = 27 * 64 * 128 * 96                                                   # stem (64 stored outputs)
    h, w = 128, 96

    def inverted_residual(cin_stored, cin, cout, stride, h, w):
        hid = up(exp * cin)
        m = cin_stored * hid * h * w
        h, w = h // stride, w // stride
        return m + 9 * hid * h * w + hid * up(cout) * h * w, h, w
    m, h, w = inverted_residual(32, c0, c1, 1, h, w)
    macs += m
    cin = c1
    for cout, stride in ((c2, 2), (c2, 1), (c2, 1)):
        m, h, w = inverted_residual(up(cin), cin, cout, stride, h, w)
        macs += m
        cin = cout
    for out, d, ffn, n in mit:
        m, h, w = inverted_residual(up(cin), cin, out, 2, h, w)
        macs += m
        o, dp, fp = up(out), up(d), up(ffn)
        macs += 9 * o * o * h * w + o * dp * h * w                              # local_rep
        macs += n * (dp * 3 * dp + dp * dp + 2 * dp * fp) * h * w               # qkv, out_proj, ffn
        macs += n * 2 * d * (h * w // 4) * h * w                                # q k^T and the weighted sum
        macs += dp * o * h * w + 9 * 2 * o * o * h * w                          # conv_proj, fusion
        cin = out
    assert (h, w) == (8, 6)
    macs += up(cin) * 320 * h * w + 320 * 256 * h * w                           # conv_1x1_exp, conv_compress
    c = 256
    for planes in (512, 256, 128):
        macs += 9 * c * planes * h * w
        c, h, w = planes // 4, 2 * h, 2 * w
    macs += c * 17 * h * w
    assert prog.macs_per_image() == macs


def test_refused_configurations():
    """Every refusal is a NotImplementedError that names the net."""
    for size in ("xl", 0.5, "XXS"):
        with pytest.raises(NotImplementedError, match=NAME + " MODEL_SIZE"):
            MODELS[NAME](_cfg(size), is_train=False)
    with pytest.raises(NotImplementedError, match=NAME + ".*bf16"):
        MODELS[NAME](_cfg(), is_train=False, dtype="bf16")
    from udp_pose_amd.mobilevit_plan import MobileViTProgram, mobilevit_spec
    sd = synth_mobilevit_state_dict(seed=1)
    with pytest.raises(NotImplementedError, match=NAME + ".*bf16"):
        MobileViTProgram(sd, mobilevit_spec({}), 256, 192, "bf16")
    for h, w in ((224, 192), (256, 160), (96, 96)):                             # multiples of 32 whose 1/32 map is odd
        with pytest.raises(NotImplementedError, match=NAME + ".*multiples of 64"):
            MobileViTProgram(sd, mobilevit_spec({}), h, w, "f32")
    net = MODELS[NAME](_cfg(), is_train=False)
    for refused in (net.trainer, net.train, net.init_weights):
        with pytest.raises(NotImplementedError, match=NAME):
            refused()
    for key, val in (("ARCHITECTURE", (512, 256, 100)), ("ARCHITECTURE", (512, 256)), ("START_CHANNELS", 200), ("FINAL_CONV_KERNEL", 5)):
        bad = _cfg()
        bad["MODEL"]["EXTRA"][key] = val
        with pytest.raises(NotImplementedError, match=key):
            MODELS[NAME](bad, is_train=False)


def test_sibling_planners_are_untouched():
    """``_pw`` gained a residual-view argument and the op record a head count: a ShuffleNetV2 and a MobileViTv2 program are
    the same (tests/golden/program_digest_66.txt holds the other nets')."""
    from udp_pose_amd.mobilevitv2_plan import MobileViTv2Program, mobilevitv2_spec
    from udp_pose_amd.shufflenet_plan import ShuffleNetV2Program, shufflenet_spec
    from udp_pose_amd.synth_mobilevitv2 import synth_mobilevitv2_state_dict
    from udp_pose_amd.synth_shufflenet import synth_shufflenet_state_dict
    sd = synth_shufflenet_state_dict(seed=7, model_size="0.5x")
    prog = ShuffleNetV2Program(sd, shufflenet_spec({"MODEL_SIZE": "0.5x"}), 64, 64, "f32")
    assert len(prog._ops) == 62 and all(op["relu"] in (0, 1) and op["heads"] == 0 for op in prog._ops)
    assert all(op["res"] is None for op in prog._ops if op["kind"] == K.UDP_OP_CONV)
    sd = synth_mobilevitv2_state_dict(seed=7)
    prog = MobileViTv2Program(sd, mobilevitv2_spec({}), 64, 64, "f16x2")
    assert len(prog._ops) == 102 and all(op["heads"] == 0 and op["res_pitch"] == 0 for op in prog._ops)
    assert all(o.up_shift[0] == 0 for o in prog.ops_array())
