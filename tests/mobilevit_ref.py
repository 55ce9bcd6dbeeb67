"""pose_mobilevit_pixel_shuffle restated on stock torch.nn.functional, straight from a reference-format state_dict: the
reference module does not exist where the GPU tests run.  Any MODEL_SIZE (read off the weight shapes), any input size
that is a multiple of 64, any floating dtype (the GPU tests use fp64).  tests/test_mobilevit_cpu.py pins it to the
heat-maps the reference's own module produced (tests/golden/mobilevit_xxs_ps.npz).

The MobileViT block is restated in MAP form, the form the HIP program runs: the reference unfolds the map into
[B P, N, d] tokens (P = 4 positions of a 2x2 patch, N patches), applies the encoders and folds it back
(mobilevit.py:593-677); here the map stays [B, d, H, W], LayerNorm runs over each pixel's channels, the linear layers
are 1x1 convs and the attention mixes the pixels of one position class (y & 1, x & 1), taken by viewing the map as
[B, d, H/2, 2, W/2, 2].

Line numbers: deep_hrnet/lib/models/backbones/mobilevit.py (backbone), decoders/pixelshuffle.py + DUC.py (decoder),
pose_mobilevit_pixel_shuffle.py (head).
"""
import torch
import torch.nn.functional as F

from shufflenet_ref import _bn, _conv

LN_EPS = 1e-5
HEADS = 4               # number_heads of the three backbone YAMLs the reference ships


def silu(x):
    """nn.SiLU (:76-77), the arithmetic of UDP_ACT_SILU."""
    return x * (1 / (1 + torch.exp(-x)))


def layer_norm_map(x, gamma, beta):
    """nn.LayerNorm(d) (:112-113) of every pixel of a [B, d, H, W] map."""
    y = F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), gamma.to(x.dtype), beta.to(x.dtype), LN_EPS)
    return y.permute(0, 3, 1, 2)


def mha_core(q, k, v, heads):
    """MultiHeadAttention.forward_other between qkv_proj and out_proj (:436-457) on [B, d, H, W] maps, WITHOUT the
    hd^-0.5 scaling of q (the caller has applied it): head h owns channels [h hd, (h + 1) hd); soft-max attention among
    the N = HW / 4 pixels of each of the four parity classes, in patch raster order."""
    b, d, h, w = q.shape
    hd = d // heads

    def tok(t):                      # [B, d, H, W] -> [B, 2, 2, heads, N, hd]
        t = t.reshape(b, heads, hd, h // 2, 2, w // 2, 2).permute(0, 4, 6, 1, 3, 5, 2)
        return t.reshape(b, 2, 2, heads, (h // 2) * (w // 2), hd)
    a = torch.softmax(tok(q) @ tok(k).transpose(-1, -2), dim=-1) @ tok(v)                            # [B,2,2,heads,N,hd]
    a = a.reshape(b, 2, 2, heads, h // 2, w // 2, hd).permute(0, 3, 6, 4, 1, 5, 2)                   # [B,heads,hd,H/2,2,W/2,2]
    return a.reshape(b, d, h, w)


def _lin(sd, name, x):
    """LinearLayer (:231-238) applied to every pixel: a 1x1 conv with the [out, in] matrix."""
    w = sd[name + ".weight"].to(x.dtype)
    return F.conv2d(x, w[:, :, None, None], sd[name + ".bias"].to(x.dtype))


def _ln(sd, name, x):
    return layer_norm_map(x, sd[name + ".weight"], sd[name + ".bias"])


def _cbn(sd, name, x, act, calibrate, stride=1, groups=1):
    """ConvLayer with a norm (:289-327)."""
    y = _bn(sd, name + ".block.norm", _conv(sd, name + ".block.conv", x, stride, groups), calibrate)
    return silu(y) if act else y


def _inverted_residual(sd, p, x, stride, calibrate):
    """InvertedResidual.forward (:196-200)."""
    y = _cbn(sd, p + ".block.exp_1x1", x, True, calibrate)
    y = _cbn(sd, p + ".block.conv_3x3", y, True, calibrate, stride, y.shape[1])
    y = _cbn(sd, p + ".block.red_1x1", y, False, calibrate)
    return x + y if stride == 1 and x.shape[1] == y.shape[1] else y


def _mit_block(sd, q, x, calibrate):
    """MobileViTBlock.forward (:657-677), map form."""
    t = _cbn(sd, q + ".local_rep.conv_3x3", x, True, calibrate)
    t = _conv(sd, q + ".local_rep.conv_1x1.block.conv", t)
    d = t.shape[1]
    u = 0
    while ("%s.global_rep.%d.pre_norm_mha.0.weight" % (q, u)) in sd:                                 # TransformerEncoder.forward (:507-514)
        g = "%s.global_rep.%d" % (q, u)
        qkv = _lin(sd, g + ".pre_norm_mha.1.qkv_proj", _ln(sd, g + ".pre_norm_mha.0", t))
        a = mha_core(qkv[:, :d] * (d // HEADS) ** -0.5, qkv[:, d:2 * d], qkv[:, 2 * d:], HEADS)       # query, key, value (:433-441)
        t = t + _lin(sd, g + ".pre_norm_mha.1.out_proj", a)
        f = silu(_lin(sd, g + ".pre_norm_ffn.1", _ln(sd, g + ".pre_norm_ffn.0", t)))
        t = t + _lin(sd, g + ".pre_norm_ffn.4", f)
        u += 1
    t = _ln(sd, "%s.global_rep.%d" % (q, u), t)
    t = _cbn(sd, q + ".conv_proj", t, True, calibrate)
    return _cbn(sd, q + ".fusion", torch.cat([x, t], dim=1), True, calibrate)


def forward(sd, x, calibrate=False, dtype=None):
    """Heat-maps [N, C, H/4, W/4] of ``x`` [N,3,H,W].  ``calibrate``: overwrite every BatchNorm's running statistics in
    ``sd`` with those of this batch (seeded random weights then neither die nor blow up)."""
    with torch.no_grad():
        x = x.to(dtype or x.dtype)
        x = _cbn(sd, "backbone.conv_1", x, True, calibrate, 2)                                       # :711-714
        x = _inverted_residual(sd, "backbone.layer_1.0", x, 1, calibrate)
        x = _inverted_residual(sd, "backbone.layer_2.0", x, 2, calibrate)
        x = _inverted_residual(sd, "backbone.layer_2.1", x, 1, calibrate)
        x = _inverted_residual(sd, "backbone.layer_2.2", x, 1, calibrate)
        for layer in (3, 4, 5):                                                                      # :875-928
            x = _inverted_residual(sd, "backbone.layer_%d.0" % layer, x, 2, calibrate)
            x = _mit_block(sd, "backbone.layer_%d.1" % layer, x, calibrate)
        x = _cbn(sd, "backbone.conv_1x1_exp", x, True, calibrate)                                    # :821
        x = _conv(sd, "decoder.conv_compress", x)                                                    # pixelshuffle.py:29
        d = 0
        while ("decoder.duc.%d.conv.weight" % d) in sd:                                              # DUC.py:23-28
            x = F.pixel_shuffle(F.relu(_bn(sd, "decoder.duc.%d.bn" % d, _conv(sd, "decoder.duc.%d.conv" % d, x), calibrate)), 2)
            d += 1
        return _conv(sd, "final_layer", x)                                                           # :59
