"""pose_mobilevitv2_pixel_shuffle restated on stock torch.nn.functional, straight from a reference-format state_dict:
the reference module does not exist where the GPU tests run.  Any MODEL_SIZE (read off the weight shapes), any input
size that is a multiple of 64, any floating dtype (the GPU tests use fp64).  tests/test_mobilevitv2_cpu.py pins it to
the heat-maps the reference's own module produced (tests/golden/mobilevitv2_05_ps.npz).

The MobileViT block is restated in MAP form, the form the HIP program runs: the reference unfolds the map into
[B, C, 4, N] patches, applies the attention units and folds it back (mobilevitv2.py:1026-1055, :1105-1126); here the
map stays [B, C, H, W], GroupNorm(1, C) runs over it as it is, and the attention's soft-max over the patches is taken
per position class (y & 1, x & 1) by viewing the map as [B, C, H/2, 2, W/2, 2].

Line numbers: deep_hrnet/lib/models/backbones/mobilevitv2.py (backbone), decoders/pixelshuffle.py + DUC.py (decoder),
pose_mobilevitv2_pixel_shuffle.py (head).
"""
import torch
import torch.nn.functional as F

from shufflenet_ref import _bn, _conv

GN_EPS = 1e-5


def silu(x):
    """nn.SiLU (:78-79), the arithmetic of UDP_ACT_SILU."""
    return x * (1 / (1 + torch.exp(-x)))


def group_norm1(sd, name, x):
    """GroupNorm(1, C) -- "layer_norm_2d" (:139-140)."""
    return F.group_norm(x, 1, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype), GN_EPS)


def linear_attention_core(q, k, v):
    """LinearSelfAttention._forward_self_attn between qkv_proj and out_proj (:671-689) on maps: q [B,1,H,W], k and v
    [B,C,H,W].  Soft-max over the pixels of each of the four parity classes; context = sum of the keys weighted by it;
    output = relu(v) * the context of the pixel's class."""
    b, c, h, w = k.shape
    cls = lambda t: t.reshape(b, t.shape[1], h // 2, 2, w // 2, 2)
    s = torch.softmax(cls(q).permute(0, 1, 3, 5, 2, 4).reshape(b, 1, 2, 2, -1), dim=-1)          # [B,1,2,2,N]
    kk = cls(k).permute(0, 1, 3, 5, 2, 4).reshape(b, c, 2, 2, -1)
    ctx = (kk * s).sum(dim=-1)                                                                       # [B,C,2,2]
    out = F.relu(cls(v)) * ctx[:, :, None, :, None, :]
    return out.reshape(b, c, h, w)


def _cbn(sd, name, x, act, calibrate, stride=1, groups=1):
    """ConvLayer with a norm (:321-345)."""
    y = _bn(sd, name + ".block.norm", _conv(sd, name + ".block.conv", x, stride, groups), calibrate)
    return silu(y) if act else y


def _inverted_residual(sd, p, x, stride, calibrate):
    """InvertedResidual.forward (:226-230)."""
    y = _cbn(sd, p + ".block.exp_1x1", x, True, calibrate)
    y = _cbn(sd, p + ".block.conv_3x3", y, True, calibrate, stride, y.shape[1])
    y = _cbn(sd, p + ".block.red_1x1", y, False, calibrate)
    return x + y if stride == 1 and x.shape[1] == y.shape[1] else y


def _mit_block(sd, q, x, calibrate):
    """MobileViTBlockv2.forward_spatial (:1105-1126), map form."""
    t = _cbn(sd, q + ".local_rep.0", x, True, calibrate, 1, x.shape[1])
    t = _conv(sd, q + ".local_rep.1.block.conv", t)
    d = t.shape[1]
    u = 0
    while ("%s.global_rep.%d.pre_norm_attn.0.weight" % (q, u)) in sd:                               # LinearAttnFFN.forward (:839-855)
        g = "%s.global_rep.%d" % (q, u)
        qkv = _conv(sd, g + ".pre_norm_attn.1.qkv_proj.block.conv", group_norm1(sd, g + ".pre_norm_attn.0", t))
        a = linear_attention_core(qkv[:, :1], qkv[:, 1:1 + d], qkv[:, 1 + d:])                       # query, key, value (:671-673)
        t = t + _conv(sd, g + ".pre_norm_attn.1.out_proj.block.conv", a)
        f = silu(_conv(sd, g + ".pre_norm_ffn.1.block.conv", group_norm1(sd, g + ".pre_norm_ffn.0", t)))
        t = t + _conv(sd, g + ".pre_norm_ffn.3.block.conv", f)
        u += 1
    t = group_norm1(sd, "%s.global_rep.%d" % (q, u), t)
    return _cbn(sd, q + ".conv_proj", t, False, calibrate)


def forward(sd, x, calibrate=False, dtype=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W].  ``calibrate``: overwrite every BatchNorm's running statistics in
    ``sd`` with those of this batch (seeded random weights then neither die nor blow up)."""
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = _cbn(sd, "backbone.conv_1", x, True, calibrate, 2)                                       # :1198-1206
        x = _inverted_residual(sd, "backbone.layer_1.0", x, 1, calibrate)
        x = _inverted_residual(sd, "backbone.layer_2.0", x, 2, calibrate)
        x = _inverted_residual(sd, "backbone.layer_2.1", x, 1, calibrate)
        for layer in (3, 4, 5):                                                                      # :1313-1366
            x = _inverted_residual(sd, "backbone.layer_%d.0" % layer, x, 2, calibrate)
            x = _mit_block(sd, "backbone.layer_%d.1" % layer, x, calibrate)
        x = _conv(sd, "decoder.conv_compress", x)                                                    # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                              # DUC.py:23-28
            x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), calibrate)), 2)
            d += 1
        return _conv(sd, "final_layer", x)                                                           # :59
