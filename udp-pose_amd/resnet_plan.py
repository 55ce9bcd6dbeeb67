"""Host compiler for pose_resnet / SimpleBaseline (deep_hrnet/lib/models/pose_resnet.py:105-273) -> the fused op program.

Graph restated from the reference: 7x7 s2 conv + BN + ReLU and a 3x3 s2 max-pool (:112-116, :195-199), four stages
of Bottlenecks (:64-100, :138-153: the stride sits on the 3x3 conv, the projection shortcut is a 1x1 conv + BN), then
NUM_DECONV_LAYERS x [ConvTranspose2d(k=4, s=2, p=1) + BN + ReLU] (:155-193) and the 1x1 / 3x3 ``final_layer`` with
bias (:128-136) writing the NCHW fp32 heat-maps.  ``conv3 + bn3 + shortcut + ReLU`` of a Bottleneck is one conv with
the residual in its epilogue; every deconv layer is one UDP_OP_DECONV launch (csrc/deconv.hip).

``PoseResNetPsaProgram`` is the pose_resnet_psa variant (pose_resnet_psa.py): at NUM_LAYERS 18 / 34 the stages are
BasicBlocks with a polarized self-attention block after bn1.
"""
import torch

from . import _lib
from .program import Program

# resnet_spec of pose_resnet.py:254-260 (Bottleneck depths only; BasicBlock 18 / 34 ship in no YAML)
RESNET_LAYERS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
# the BasicBlock depths of pose_resnet_psa.py:254-260: the only blocks of that file that carry a PSA_s (:39)
RESNET_PSA_LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def pose_resnet_spec(extra):
    """MODEL.EXTRA of a pose_resnet YAML -> dict(layers, deconv_filters, final_kernel, deconv_with_bias).  Raises
    NotImplementedError for what the kernels do not cover: BasicBlock depths (18 / 34), deconv kernels other than 4,
    a deconv count other than 3 (the heat-maps must come out at 1/4 of the input), a final kernel other than 1 / 3."""
    num_layers = int(_get(extra, "NUM_LAYERS"))
    if num_layers not in RESNET_LAYERS:
        raise NotImplementedError("pose_resnet NUM_LAYERS=%d: only the Bottleneck depths %s are supported (BasicBlock "
                                  "ResNet-18 / 34 ships in no reference YAML)" % (num_layers, sorted(RESNET_LAYERS)))
    return dict(_head_spec(extra), layers=RESNET_LAYERS[num_layers])


def _head_spec(extra, name="pose_resnet"):
    """The deconv head / final layer part of the spec, with its refusals (``name``: how the messages call the net)."""
    nd = int(_get(extra, "NUM_DECONV_LAYERS", 3))
    filters = [int(f) for f in _get(extra, "NUM_DECONV_FILTERS", [256] * nd)]
    kernels = [int(k) for k in _get(extra, "NUM_DECONV_KERNELS", [4] * nd)]
    if nd != 3 or len(filters) != nd or len(kernels) != nd:
        raise NotImplementedError("%s: NUM_DECONV_LAYERS=%d (filters %s, kernels %s): only 3 deconv layers "
                                  "(heat-maps at 1/4 of the input) are supported" % (name, nd, filters, kernels))
    if any(k != 4 for k in kernels):
        raise NotImplementedError("%s: NUM_DECONV_KERNELS=%s: only ConvTranspose2d(k=4, s=2, p=1) has a kernel "
                                  "(kernels 2 / 3 ship in no reference YAML)" % (name, kernels))
    final_kernel = int(_get(extra, "FINAL_CONV_KERNEL", 1))
    if final_kernel not in (1, 3):
        raise NotImplementedError("%s: FINAL_CONV_KERNEL=%d (1 or 3)" % (name, final_kernel))
    return dict(deconv_filters=tuple(filters), final_kernel=final_kernel,
                deconv_with_bias=bool(_get(extra, "DECONV_WITH_BIAS", False)))


def pose_resnet_psa_spec(extra):
    """MODEL.EXTRA of a pose_resnet_psa YAML -> the dict of ``pose_resnet_spec`` plus ``basic``: True for NUM_LAYERS
    18 / 34 (BasicBlocks with a PSA_s after bn1), False for 50 / 101 / 152, where the reference builds its plain
    Bottleneck net (pose_resnet_psa.py:64-102 has no attention).  The same refusals as ``pose_resnet_spec``."""
    num_layers = int(_get(extra, "NUM_LAYERS"))
    if num_layers not in RESNET_PSA_LAYERS:
        return dict(pose_resnet_spec(extra), basic=False)
    return dict(_head_spec(extra), layers=RESNET_PSA_LAYERS[num_layers], basic=True)


class _Tracked(dict):
    """The state_dict, remembering which keys the planner read (tests check that every one is consumed)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.used = set()

    def __getitem__(self, k):
        self.used.add(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        if k in self:
            self.used.add(k)
        return super().get(k, default)


class PoseResNetProgram(Program):
    def __init__(self, state_dict, spec, in_h, in_w, dtype="f32"):
        if dtype not in ("f32", "f16x2"):
            raise ValueError("pose_resnet: dtype %r; supported storage modes are 'f32' and 'f16x2' (the deconv kernel "
                             "has no bf16 form)" % (dtype,))
        self.spec = spec
        super().__init__(state_dict, in_h, in_w, dtype)

    @property
    def consumed_keys(self):
        return set(self.sd.used)

    def _block(self, x, p, stride):
        """Bottleneck.forward (:82-100)."""
        a = self._conv(x, p + ".conv1", p + ".bn1")
        t = self._conv(a, p + ".conv2", p + ".bn2", stride=stride)
        r = x
        if (p + ".downsample.0.weight") in self.sd:
            r = self._conv(x, p + ".downsample.0", p + ".downsample.1", stride=stride, relu=False)
        return self._conv(t, p + ".conv3", p + ".bn3", res=r)           # relu(bn3(conv3(t)) + shortcut)

    def _build(self):
        self.sd = _Tracked(self.sd)
        sd = self.sd
        H, W = self.in_h, self.in_w
        x = self._stem(_lib.UDP_OP_STEM7, "conv1", "bn1", 7)
        pooled = self._new(64, H // 4, W // 4)
        self._emit(_lib.UDP_OP_MAXPOOL, "maxpool", x, pooled, ks=3, stride=2)
        x = pooled
        for li, nblk in enumerate(self.spec["layers"], start=1):          # _make_layer (:138-153)
            for k in range(nblk):
                x = self._block(x, "layer%d.%d" % (li, k), 2 if (li > 1 and k == 0) else 1)
        self._deconv_head(x, "pose_resnet", len(self.spec["deconv_filters"]))
        for k in sd:
            if k.endswith("num_batches_tracked"):
                sd.used.add(k)                                              # BatchNorm bookkeeping, not an operand


class PoseResNetPsaProgram(PoseResNetProgram):
    """pose_resnet_psa (deep_hrnet/lib/models/pose_resnet_psa.py:105-209): the same stem, deconv head and
    ``final_layer``; with ``spec["basic"]`` the four stages are BasicBlocks (:31-61) -- conv1 (3x3, carries the stage's
    stride) + bn1 + ReLU, the polarized self-attention ``deattn`` on the planes-channel map at the reduced resolution
    (POOL, MLP, SCALE, the theta conv, SP: csrc/psa.hip; 512 channels in layer 4), conv2 + bn2 with the shortcut (the
    identity, or ``downsample`` = 1x1 stride-2 conv + BN) in its epilogue, ReLU: 7 launches (8 with a projection).
    Without ``basic`` it is PoseResNetProgram's Bottleneck net, op for op."""

    def _block(self, x, p, stride):
        if not self.spec.get("basic"):
            return super()._block(x, p, stride)
        t = self._conv(x, p + ".conv1", p + ".bn1", stride=stride)
        t = self._psa(t, p + ".deattn")
        r = x
        if (p + ".downsample.0.weight") in self.sd:
            r = self._conv(x, p + ".downsample.0", p + ".downsample.1", stride=stride, relu=False)
        return self._conv(t, p + ".conv2", p + ".bn2", res=r)           # relu(bn2(conv2(t)) + shortcut)
