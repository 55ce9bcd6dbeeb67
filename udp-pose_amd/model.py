"""Model factory with the reference's contract: ``MODELS[cfg.MODEL.NAME](cfg, is_train)``.

Mirrors deep_hrnet/lib/models/__init__.py:28-41 and pose_hrnet.py:508-514
(``get_pose_net``): the returned object takes the reference's state_dict
(``load_state_dict``, ``module.`` prefixes stripped as pose_engine.py:107-117
does), ``.to(device)``, ``.eval()`` and is called on an NCHW fp32 batch,
returning the heat-map tensor ``[N, J*(3 if offset else 1), H/4, W/4]`` fp32
on the same device.  The forward runs entirely in libudp_pose_hip.so.
"""
import ctypes as C

import torch

from . import _lib
from .hrnet_plan import HRNetProgram, storage_bytes
from .synth import hrnet_param_shapes


def _get(cfg, *path):
    cur = cfg
    for p in path:
        cur = cur[p] if isinstance(cur, dict) else getattr(cur, p)
    return cur


class PoseNetHip:
    """The runtime every net shares: a reference-format state_dict compiled per input shape into one op program
    (``_make_program``) that libudp_pose_hip.so executes.  Subclasses supply ``param_shapes()`` and ``_make_program()``;
    inference only unless they override ``trainer()``."""

    NAME = None            # how error messages call the net
    MAX_IO_SHAPES = 8      # persistent (input, output) buffer pairs kept, least recently used evicted (= the
                           # library's hipGraph cache size: one graph per buffer set)
    _LACKS = None          # message of a non-strict load_state_dict that misses tensors (None: the strict one)

    def __init__(self, cfg=None, dtype="f32"):
        self.cfg = cfg
        self.dtype = dtype
        self.psa = False
        self.training = False
        self.device = None
        self.use_graph = True
        self.max_images_per_launch = None     # None: only the 2 GiB-per-tensor limit of one launch applies
        self._sd = None
        self._compiled = {}      # (h, w) -> (handle, blob tensor, program)
        self._ws = None
        self._io = {}

    # ---- nn.Module-like surface used by the reference's callers
    def load_state_dict(self, state_dict, strict=True):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        want = self.param_shapes()
        missing = [k for k in want if k not in sd and not k.endswith("num_batches_tracked")]
        unexpected = [k for k in sd if k not in want]
        if missing and not strict and self._LACKS:
            raise RuntimeError(self._LACKS % (len(missing), missing[:3]))
        if missing or (strict and unexpected):
            raise RuntimeError("state_dict mismatch: missing %s unexpected %s" % (missing[:5], unexpected[:5]))
        for k, shape in want.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(sd[k].shape), tuple(shape)))
        self._sd = sd
        self._release()
        return self

    def state_dict(self):
        """Reference-format state_dict; after training steps it is read back from the trainer's flat buffer."""
        self._refresh()
        return dict(self._sd or {})

    def trainer(self):
        raise NotImplementedError("%s: the training step covers pose_hrnet, pose_hrnet_psa, pose_resnet, the two "
                                  "ShuffleNetV2 nets, the two MobileNetV3-small nets and pose_mobilevitv2_pixel_shuffle only"
                                  % self.NAME)

    def to(self, device):
        self.device = torch.device(device)
        return self

    def cuda(self):
        return self.to("cuda")

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        """nn.Module.train(): in training mode ``model(x)`` is the train-mode forward of the trainer (batch
        statistics, tape kept for the backward); in eval mode the compiled inference program."""
        if mode:
            self.trainer()
        self.training = bool(mode)
        return self

    def _refresh(self):
        """Runs before the weights are used (forward, state_dict): a net whose weights can move under its compiled
        programs re-reads them here."""

    # ---- compile / run
    def _release(self):
        for h, _, _ in self._compiled.values():
            _lib.lib().udp_hrnet_destroy(h)
        self._compiled = {}
        self._io = {}

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _compile(self, h, w):
        if self._sd is None:
            raise RuntimeError("load_state_dict() first")
        prog = self._make_program(h, w)
        blob = torch.from_numpy(prog.weight_blob()).to(self.device)
        ops = prog.ops_array()
        bufs = (C.c_int64 * len(prog.buf_elems))(*prog.buf_elems)
        handle = C.c_void_p()
        _lib.check(_lib.lib().udp_hrnet_create(ops, len(ops), bufs, len(prog.buf_elems), _lib.ptr(blob),
                                               blob.numel(), _lib.DTYPES[self.dtype],
                                               h, w, prog.out_channels, C.byref(handle)))
        self._compiled[(h, w)] = (handle, blob, prog)
        return self._compiled[(h, w)]

    def program(self, h, w):
        if self.device is None:
            self.to("cuda")
        return (self._compiled.get((h, w)) or self._compile(h, w))[2]

    def io_buffers(self, n, h, w, flip_test=False):
        """Persistent (input [n,3,h,w], heat-maps [n*(1|2),C,h/4,w/4]) device buffers for this
        shape.  Launch sequences are replayed as hipGraphs keyed on these addresses, so the
        forward reads the network input from / writes heat-maps to the same memory every call."""
        if self.device is None:
            self.to("cuda")
        key = (n, h, w, bool(flip_test))
        io = self._io.pop(key, None)
        if io is None:
            prog = self.program(h, w)
            b = n * (2 if flip_test else 1)
            io = (torch.empty(n, 3, h, w, dtype=torch.float32, device=self.device),
                  torch.empty(b, prog.out_channels, h // 4, w // 4, dtype=torch.float32, device=self.device))
            while len(self._io) >= self.MAX_IO_SHAPES:     # least recently used first (dicts keep insertion order)
                self._io.pop(next(iter(self._io)))
        self._io[key] = io                                  # (re-)inserted last = most recently used
        return io

    def _stage(self, handle, x, flip_test):
        """Before a launch of ``handle``: ``x`` in the persistent input buffer of its shape, a workspace that is large
        enough -> (input buffer, output buffer)."""
        n, _, h, w = x.shape
        xin, out = self.io_buffers(n, h, w, flip_test)
        if x.data_ptr() != xin.data_ptr():
            xin.copy_(x)
        need = _lib.lib().udp_hrnet_workspace_bytes(handle, n, int(flip_test))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        return xin, out

    def raw_forward(self, x, flip_test=False):
        """x: cuda fp32 [N,3,H,W] -> heat-maps [N*(2 if flip_test else 1), C, H/4, W/4]
        (rows N.. are the raw outputs for the W-mirrored inputs).  The returned tensor is the
        model's persistent output buffer: it is overwritten by the next call of the same shape
        (the reference's callers ``.clone()`` it, pose_engine.py:125)."""
        if self.device is None:
            self.to(x.device)
        if not x.is_cuda:
            raise RuntimeError("udp-pose_amd has no CPU path: the input must live on the GPU")
        self._refresh()
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected fp32 [N,3,H,W], got %s %s" % (x.dtype, tuple(x.shape)))
        n, _, h, w = x.shape
        if n < 1:
            raise ValueError("empty batch (the reference's torch.stack of no crops raises too)")
        handle, _, prog = self._compiled.get((h, w)) or self._compile(h, w)
        # one launch addresses a tensor with 32-bit byte offsets: split batches whose largest activation
        # ([2N, H/2, W/2, 64]) would pass 2 GiB
        cap = max(1, (2 ** 31 - 1) // (max(t.elems for t in prog._tensors) * storage_bytes(self.dtype)
                                      * (2 if flip_test else 1)))
        cap = min(cap, self.max_images_per_launch or cap)
        if n > cap:
            parts = [self.raw_forward(x[i:i + cap].contiguous(), flip_test).clone() for i in range(0, n, cap)]
            if not flip_test:
                return torch.cat(parts)
            sizes = [min(cap, n - i) for i in range(0, n, cap)]
            return torch.cat([p[:k] for p, k in zip(parts, sizes)] + [p[k:] for p, k in zip(parts, sizes)])
        xin, out = self._stage(handle, x, flip_test)
        _lib.check(_lib.lib().udp_hrnet_forward(handle, _lib.ptr(xin), n, int(flip_test), _lib.ptr(self._ws),
                                                self._ws.numel(), _lib.ptr(out), int(self.use_graph), _lib.stream_ptr()))
        return out

    def profile(self, x, flip_test=False):
        """Per-op elapsed milliseconds (hipEvents around every launch, eager) and the op table:
        returns (ms ndarray [n_ops], describe() list)."""
        import numpy as np
        n, _, h, w = x.shape
        handle, _, prog = self._compiled.get((h, w)) or self._compile(h, w)
        xin, out = self._stage(handle, x, flip_test)
        ms = (C.c_float * _lib.lib().udp_hrnet_num_launches(handle))()
        _lib.check(_lib.lib().udp_hrnet_profile(handle, _lib.ptr(xin), n, int(flip_test), _lib.ptr(self._ws),
                                                self._ws.numel(), _lib.ptr(out), ms, _lib.stream_ptr()))
        return np.frombuffer(ms, dtype=np.float32).copy(), prog.describe()

    def __call__(self, x):
        if self.training:
            return self.trainer().forward(x.contiguous())
        return self.raw_forward(x, flip_test=False)

    forward = __call__


class _Trainable:
    """The training surface function.train drives (tools/train.py:91,116-125), shared by the nets that have a trainer:
    ``trainer()`` (created on first use from the current state_dict by ``_make_trainer``), ``parameters()``, and the
    staleness handling that re-reads the weights from the trainer once it has stepped."""

    _trainer = None              # the train.Trainer over the same weights (created by .train())
    _stale = False               # legacy flag (function.train sets it); the trainer's version counter decides
    _seen_version = 0            # trainer.version the inference program / state_dict were last synced at

    def _make_trainer(self):
        raise NotImplementedError

    def trainer(self):
        """The trainer over this model's weights (created on first use from the current state_dict)."""
        if self._trainer is None:
            if self._sd is None:
                raise RuntimeError("load_state_dict() or init_weights() first")
            if self.device is None:
                self.to("cuda")
            self._trainer = self._make_trainer()
        return self._trainer

    def parameters(self):
        """What ``optim.Adam(model.parameters(), lr=...)`` (utils.py:70-74) takes: ONE flat fp32 device tensor
        holding every parameter in named_parameters() order (the trainer's master copy)."""
        t = self.trainer()
        return [t.flat[:t._n_param]]

    def _trainer_moved(self):
        """True when the trainer has stepped (by whatever route: function.train, train_step, adam_step) since the
        compiled inference program and ``_sd`` were last read from it."""
        return self._trainer is not None and (self._stale or self._trainer.version != self._seen_version)

    def _sync_from_trainer(self):
        self._sd = self._trainer.state_dict()
        self._stale = False
        self._seen_version = self._trainer.version
        self._release()

    def _refresh(self):
        if self._trainer_moved():
            self._sync_from_trainer()                      # weights moved since the program was compiled

    def _set_weights(self, sd):
        """Fresh weights (init_weights): any trainer over the old ones is dropped."""
        self._sd = sd
        self._trainer, self._seen_version, self._stale = None, 0, False
        self._release()
        return self


class PoseHighResolutionNetHip(_Trainable, PoseNetHip):
    """HRNet (UDP variant) on MI355X through the C ABI: inference, plus the training surface function.train drives."""

    NAME = "pose_hrnet"
    _LACKS = "state_dict lacks %d tensors the forward needs, e.g. %s"

    def __init__(self, cfg, dtype="f32", psa=False):
        super().__init__(cfg, dtype)
        self.psa = bool(psa)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        # same checks as HighResolutionModule._check_branches (pose_hrnet.py:121-139)
        hrnet_param_shapes(self.extra, self.num_joints, self.target_type)

    def param_shapes(self):
        return hrnet_param_shapes(self.extra, self.num_joints, self.target_type, psa=self.psa)

    def _make_program(self, h, w):
        return HRNetProgram(self._sd, self.extra, h, w, self.dtype)

    def init_weights(self, pretrained=""):
        """pose_hrnet.py:473-505: conv weights ~ N(0, 0.001), conv biases 0, BatchNorm (weight 1, bias 0; running
        statistics at their nn.BatchNorm2d defaults 0 / 1), then the layers of a pretrained file named by
        MODEL.EXTRA.PRETRAINED_LAYERS ('*' = all; 'stage4.2.fuse_layers' keys skipped as :492-493 does).  Draws come
        from torch's global generator like nn.init.normal_ (module iteration order is not reproduced, so the
        values differ from the reference's for the same seed; the distribution is the same)."""
        import os
        shapes = self.param_shapes()
        sd = {}
        for k, shape in shapes.items():
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif k.endswith("running_var"):
                sd[k] = torch.ones(shape)
            elif k.endswith("running_mean"):
                sd[k] = torch.zeros(shape)
            elif len(shape) == 4:
                sd[k] = torch.randn(shape) * 0.001
            elif k.endswith(".weight") and ((k[:-7] + ".running_mean") in shapes or k.endswith(".deattn.conv_up.1.weight")):
                # BatchNorm weight; the attention block's nn.LayerNorm keeps its default (weight 1, bias 0):
                # pose_hrnet_psa.py:473-490 re-initialises Conv2d / BatchNorm2d / ConvTranspose2d only
                sd[k] = torch.ones(shape)
            else:
                sd[k] = torch.zeros(shape)                # BatchNorm / conv bias
        if pretrained and os.path.isfile(pretrained):
            layers = list(self.extra.get("PRETRAINED_LAYERS", ["*"]))
            for name, v in torch.load(pretrained, map_location="cpu", weights_only=True).items():
                name = name[7:] if name.startswith("module.") else name
                if "stage4.2.fuse_layers" in name or name not in sd:
                    continue
                if layers[0] == "*" or name.split(".")[0] in layers:
                    if tuple(v.shape) != tuple(sd[name].shape):
                        raise RuntimeError("size mismatch for %s: %s vs %s" % (name, tuple(v.shape), tuple(sd[name].shape)))
                    sd[name] = v
        elif pretrained:
            raise ValueError("%s is not exist!" % pretrained)       # pose_hrnet.py:503-505
        return self._set_weights(sd)

    def _make_trainer(self):
        from .train import HRNetTrainer
        return HRNetTrainer(self.cfg, self._sd, device=self.device, dtype="bf16" if self.dtype == "bf16" else "f32", psa=self.psa)


class RSN18Hip(PoseNetHip):
    """RSN-18 (RSN/exps/RSN18.coco/network.py, STAGE_NUM = 1) inference through the same C ABI;
    ``state_dict`` in the reference module's key format; returns ``outputs[-1][-1]`` ([N,C,H/4,W/4]).
    ``se`` / ``prm``: the SELayer in every Bottleneck and the Pose Refine Machine on the finest level, as in
    RSN/exps/RSN18.coco.e1.se.36x8x132000_prm/network.py.  ``stem``: ``"pool"`` is RSN18.coco's ResNet_top (7x7 s2 conv +
    max-pool), ``"conv7"`` that experiment's own (3x3 s2, 7x7 s1 64 -> 64, 3x3 s2; keys ``top.conv.{0,1,2}.*``):
    ``RSN18Hip(17, dtype, se=True, prm=True, stem="conv7")`` loads that experiment's checkpoints as they are, and
    ``RSN18Hip.from_state_dict(sd)`` reads all of this off a checkpoint.  se, prm and the conv7 stem run in the storage
    modes f32 and f16x2; bf16 is outside their contract."""

    NAME = "RSN-18"

    def __init__(self, out_channels=17, dtype="f32", chl_num=256, se=False, prm=False, stem="pool"):
        if stem not in ("pool", "conv7"):
            raise ValueError("RSN-18 stem must be 'pool' or 'conv7' (got %r)" % (stem,))
        if (se or prm) and dtype not in ("f32", "f16x2"):
            raise ValueError("RSN-18 with se / prm: storage modes 'f32' and 'f16x2' only (got %r)" % (dtype,))
        if stem == "conv7" and dtype not in ("f32", "f16x2"):
            raise ValueError("RSN-18 with the conv7 stem: storage modes 'f32' and 'f16x2' only (got %r)" % (dtype,))
        super().__init__(None, dtype)
        self.out_channels = int(out_channels)
        self.chl_num = chl_num
        self.se, self.prm = bool(se), bool(prm)
        self.stem = stem

    @classmethod
    def from_state_dict(cls, state_dict, dtype="f32"):
        """The loaded model for a checkpoint of either experiment, its flags read off the keys and shapes: ``stem`` from
        ``top.conv.1.conv.weight`` ([64,64,7,7]: "conv7"; absent: "pool"), ``se`` from ``*.se.fc.0.weight``, ``prm`` from
        ``*.prm.*``, ``out_channels`` and ``chl_num`` from the head conv ``stage0.upsample.up4.res_conv2``.  The strict
        load that follows refuses whatever else does not fit."""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        head = "stage0.upsample.up4.res_conv2.conv.weight"
        if head not in sd or len(sd[head].shape) != 4:
            raise ValueError("not an RSN-18 state_dict: no %s" % head)
        top1 = sd.get("top.conv.1.conv.weight")
        if top1 is not None and tuple(top1.shape) != (64, 64, 7, 7):
            raise ValueError("top.conv.1.conv.weight must be [64, 64, 7, 7], got %s" % (list(top1.shape),))
        if top1 is None and "top.conv.conv.weight" not in sd:
            raise ValueError("not an RSN-18 state_dict: neither top.conv.conv.weight nor top.conv.1.conv.weight")
        net = cls(int(sd[head].shape[0]), dtype, chl_num=int(sd[head].shape[1]),
                  se=any(k.endswith(".se.fc.0.weight") for k in sd), prm=any(".prm." in k for k in sd),
                  stem="pool" if top1 is None else "conv7")
        return net.load_state_dict(sd, strict=True)

    def param_shapes(self):
        from .synth import rsn18_param_shapes, rsn18_se_prm_param_shapes
        if self.se or self.prm or self.stem != "pool":
            return rsn18_se_prm_param_shapes(self.out_channels, self.chl_num, self.se, self.prm, self.stem)
        return rsn18_param_shapes(self.out_channels, self.chl_num)

    def _make_program(self, h, w):
        from .rsn_plan import RSNProgram
        return RSNProgram(self._sd, h, w, self.dtype, self.chl_num, self.se, self.prm, self.stem)


def get_pose_net(cfg, is_train, **kwargs):
    """pose_hrnet.py:508-514: ``init_weights(cfg.MODEL.PRETRAINED)`` when ``is_train and cfg.MODEL.INIT_WEIGHTS``."""
    model = PoseHighResolutionNetHip(cfg, **kwargs)
    if is_train:
        try:
            init = bool(_get(cfg, "MODEL", "INIT_WEIGHTS"))
        except (KeyError, AttributeError):
            init = False
        if init:
            try:
                pretrained = _get(cfg, "MODEL", "PRETRAINED")
            except (KeyError, AttributeError):
                pretrained = ""
            model.init_weights(pretrained or "")
    return model


def get_pose_net_psa(cfg, is_train, **kwargs):
    """pose_hrnet_psa.py get_pose_net: same plan, every BasicBlock carries "<block>.deattn.*" (PSA_s)
    parameters and the planner emits the attention ops for them."""
    return get_pose_net(cfg, is_train, psa=True, **kwargs)


class PoseResNetHip(_Trainable, PoseNetHip):
    """pose_resnet / SimpleBaseline (deep_hrnet/lib/models/pose_resnet.py:105-273: ResNet-50 / 101 / 152, three
    ConvTranspose2d(4, 2, 1) + BN + ReLU, ``final_layer``) through the same C ABI; ``state_dict`` in the reference
    module's key format.  Storage modes "f32" and "f16x2" (the deconv kernel has no bf16 form).  ``trainable`` (what
    ``MODELS["pose_resnet"](cfg, is_train=True)`` sets): the model also has the training surface of
    ``PoseHighResolutionNetHip`` -- ``init_weights``, ``train()``, ``parameters()``, ``trainer()`` (a
    train.PoseResNetTrainer, fp32 whatever the storage mode of the inference program)."""

    NAME = "pose_resnet"
    DTYPES = ("f32", "f16x2")
    TRAINS = True                # a net of this class can be built trainable

    def __init__(self, cfg, dtype="f32", trainable=False):
        if dtype not in self.DTYPES:
            raise ValueError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.spec = self._spec_of(self.extra)             # NotImplementedError for depths / kernels without a kernel
        self.trainable = bool(trainable) and self.TRAINS

    @staticmethod
    def _spec_of(extra):
        from .resnet_plan import pose_resnet_spec
        return pose_resnet_spec(extra)

    def param_shapes(self):
        from .synth_resnet import pose_resnet_param_shapes
        sp = self.spec
        return pose_resnet_param_shapes(layers=sp["layers"], num_joints=self.num_joints, deconv_filters=sp["deconv_filters"],
                                        deconv_kernel=4, final_kernel=sp["final_kernel"],
                                        deconv_with_bias=sp["deconv_with_bias"])

    def init_weights(self, pretrained=""):
        """pose_resnet.py:211-251.  With a pretrained file: the deconv and final convs ~ N(0, 0.001), their biases 0, the
        deconv BatchNorms 1 / 0, then a non-strict load of the file (the ImageNet backbone; what it lacks keeps the
        values above, and what the file does not cover of the backbone the nn.Module defaults reduced to BatchNorm 1 / 0,
        convs ~ N(0, 0.001)).  Without one: every conv and deconv ~ N(0, 0.001), every BatchNorm 1 / 0.  Draws come from
        torch's global generator like nn.init.normal_ (module iteration order is not reproduced)."""
        import os
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); load a state_dict" % self.NAME)
        shapes = self.param_shapes()
        sd = {}
        for k, shape in shapes.items():
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif k.endswith("running_var"):
                sd[k] = torch.ones(shape)
            elif k.endswith("running_mean"):
                sd[k] = torch.zeros(shape)
            elif len(shape) == 4:
                sd[k] = torch.randn(shape) * 0.001            # Conv2d / ConvTranspose2d
            elif k.endswith(".weight") and (k[:-7] + ".running_mean") in shapes:
                sd[k] = torch.ones(shape)                     # BatchNorm weight
            else:
                sd[k] = torch.zeros(shape)                    # BatchNorm / deconv / final conv bias
        if pretrained and os.path.isfile(pretrained):
            for name, v in torch.load(pretrained, map_location="cpu", weights_only=True).items():
                name = name[7:] if name.startswith("module.") else name
                if name not in sd:
                    continue                                  # strict=False: the classifier of an ImageNet file
                if tuple(v.shape) != tuple(sd[name].shape):
                    raise RuntimeError("size mismatch for %s: %s vs %s" % (name, tuple(v.shape), tuple(sd[name].shape)))
                sd[name] = v
        return self._set_weights(sd)

    def trainer(self):
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); MODELS[%r](cfg, is_train=True) "
                                      "returns the trainable model" % (self.NAME, self.NAME))
        return super().trainer()

    def _make_trainer(self):
        from .train import PoseResNetTrainer
        return PoseResNetTrainer(self.spec, self.num_joints, _get(self.cfg, "MODEL", "TARGET_TYPE"), self._sd,
                                 device=self.device, dtype="f32")

    def _make_program(self, h, w):
        from .resnet_plan import PoseResNetProgram
        return PoseResNetProgram(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_resnet(cfg, is_train, **kwargs):
    """pose_resnet.py:263-273 (``get_pose_net``): the model for MODEL.EXTRA.NUM_LAYERS, trainable under ``is_train``
    (``init_weights(cfg.MODEL.PRETRAINED)`` when cfg.MODEL.INIT_WEIGHTS says so, :270-271)."""
    model = PoseResNetHip(cfg, trainable=bool(is_train), **kwargs)
    if is_train:
        try:
            init = bool(_get(cfg, "MODEL", "INIT_WEIGHTS"))
        except (KeyError, AttributeError):
            init = False
        if init:
            try:
                pretrained = _get(cfg, "MODEL", "PRETRAINED")
            except (KeyError, AttributeError):
                pretrained = ""
            model.init_weights(pretrained or "")
    return model


class PoseResNetPsaHip(PoseResNetHip):
    """pose_resnet_psa (deep_hrnet/lib/models/pose_resnet_psa.py:105-273): NUM_LAYERS 18 / 34 are BasicBlock ResNets
    with a polarized self-attention block (PSA_s, 64 to 512 channels) after bn1 of every block; 50 / 101 / 152 are the
    reference's plain Bottleneck nets (only its BasicBlock carries the attention), the programs of ``PoseResNetHip``.
    The same deconv head, ``final_layer``, storage modes and refusals."""

    NAME = "pose_resnet_psa"
    TRAINS = False               # inference only whatever is_train says: no backward for its BasicBlock + PSA stages

    @staticmethod
    def _spec_of(extra):
        from .resnet_plan import pose_resnet_psa_spec
        return pose_resnet_psa_spec(extra)

    def param_shapes(self):
        if not self.spec["basic"]:
            return super().param_shapes()
        from .synth_resnet import pose_resnet_psa_param_shapes
        sp = self.spec
        return pose_resnet_psa_param_shapes(layers=sp["layers"], num_joints=self.num_joints, deconv_filters=sp["deconv_filters"],
                                            deconv_kernel=4, final_kernel=sp["final_kernel"],
                                            deconv_with_bias=sp["deconv_with_bias"])

    def _make_program(self, h, w):
        from .resnet_plan import PoseResNetPsaProgram
        return PoseResNetPsaProgram(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_resnet_psa(cfg, is_train, **kwargs):
    """pose_resnet_psa.py:263-273 (``get_pose_net``); inference only -- the weights come from ``load_state_dict``."""
    return PoseResNetPsaHip(cfg, **kwargs)


class PoseShuffleNetV2Hip(_Trainable, PoseNetHip):
    """pose_shufflenetv2_10x_pixel_shuffle (deep_hrnet/lib/models/pose_shufflenetv2_10x_pixel_shuffle.py:23-53: the
    ShuffleNetV2 0.5x / 1.0x / 1.5x backbone, the pixel-shuffle (DUC) decoder, ``final_layer``) through the same C ABI;
    ``state_dict`` in the reference module's key format.  Storage modes "f32" and "f16x2" (the depthwise kernel has no
    bf16 form).  ``trainable`` (what ``MODELS[NAME](cfg, is_train=True)`` sets): the model also has the training surface
    of ``PoseResNetHip`` -- ``init_weights``, ``train()``, ``parameters()``, ``trainer()`` (a train.ShuffleNetV2Trainer,
    fp32 whatever the storage mode of the inference program)."""

    NAME = "pose_shufflenetv2_10x_pixel_shuffle"
    DTYPES = ("f32", "f16x2")
    TRAINS = True                # a net of this class can be built trainable
    TRAINER = "ShuffleNetV2Trainer"

    def __init__(self, cfg, dtype="f32", trainable=False):
        if dtype not in self.DTYPES:
            raise ValueError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        self.spec = self._spec_of(self.extra, self.num_joints, self.target_type)   # NotImplementedError for 2.0x ...
        self.trainable = bool(trainable) and self.TRAINS

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .shufflenet_plan import shufflenet_spec
        return shufflenet_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_shufflenet import shufflenet_param_shapes
        sp = self.spec
        return shufflenet_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                       start_channels=sp["start_channels"], architecture=sp["architecture"],
                                       final_kernel=sp["final_kernel"])

    def init_weights(self, pretrained=""):
        """What the reference's constructor leaves behind (the pose modules have no ``init_weights`` of their own).  The
        backbone is ``ShuffleNetV2._initialize_weights`` (backbones/shufflenetv2.py:168-190): the first conv ~ N(0, 0.01),
        every other conv ~ N(0, 1 / cin_per_group), BatchNorm weight 1, bias 1e-4, running mean 0, the classifier ~
        N(0, 0.01).  Decoder / deconv head / ``final_layer`` keep torch's nn.Conv2d / ConvTranspose2d / BatchNorm2d
        defaults (kaiming_uniform(a = sqrt 5) = U(+-1 / sqrt(fan_in)), the same bound for a bias; BatchNorm 1 / 0).  A
        ``pretrained`` file is read like ``load_checkpoint`` (:6-31): ``checkpoint["state_dict"]``, ``module.`` stripped,
        the keys are the backbone's own (no ``backbone.`` prefix), non-strict -- a tensor of another size keeps its
        initialised value.  Draws come from torch's global generator."""
        import math
        import os
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); load a state_dict" % self.NAME)
        shapes = self.param_shapes()
        sd = {}
        for k, shape in shapes.items():
            backbone = k.startswith("backbone.")
            bn = (k.rsplit(".", 1)[0] + ".running_mean") in shapes
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif k.endswith("running_var"):
                sd[k] = torch.ones(shape)
            elif k.endswith("running_mean"):
                sd[k] = torch.zeros(shape)
            elif bn:
                sd[k] = torch.ones(shape) if k.endswith(".weight") else torch.full(shape, 1e-4 if backbone else 0.0)
            elif backbone and len(shape) == 4:
                sd[k] = torch.randn(shape) * (0.01 if "first" in k else 1.0 / shape[1])
            elif backbone:
                sd[k] = torch.randn(shape) * 0.01             # the classifier's Linear (no bias)
            else:                                             # nn.Conv2d / nn.ConvTranspose2d defaults, weight before bias
                w = shapes[k.rsplit(".", 1)[0] + ".weight"]
                bound = 1.0 / math.sqrt(w[1] * w[2] * w[3])   # (ConvTranspose2d: torch takes fan_in from dim 1 there too)
                sd[k] = (torch.rand(shape) * 2 - 1) * bound
        if pretrained and os.path.isfile(pretrained):
            ckpt = torch.load(pretrained, map_location="cpu", weights_only=True)["state_dict"]
            for name, v in ckpt.items():
                name = "backbone." + (name[7:] if name.startswith("module.") else name)
                if name in sd and tuple(v.shape) == tuple(sd[name].shape):
                    sd[name] = v                              # non-strict: a missing or differently sized tensor keeps its init
        return self._set_weights(sd)

    def trainer(self):
        if not self.trainable:
            if not self.TRAINS:
                return PoseNetHip.trainer(self)
            raise NotImplementedError("%s: built with is_train=False (inference only); MODELS[%r](cfg, is_train=True) "
                                      "returns the trainable model" % (self.NAME, self.NAME))
        return super().trainer()

    def _make_trainer(self):
        from . import train
        return getattr(train, self.TRAINER)(self.spec, self.num_joints, self.target_type, self._sd, device=self.device,
                                            dtype="f32")

    def _make_program(self, h, w):
        from .shufflenet_plan import ShuffleNetV2Program
        return ShuffleNetV2Program(self._sd, self.spec, h, w, self.dtype)


def _init_under_is_train(model, cfg, is_train):
    """``if is_train and cfg.MODEL.INIT_WEIGHTS: model.init_weights(cfg.MODEL.PRETRAINED)`` of the reference's factories."""
    if is_train:
        try:
            init = bool(_get(cfg, "MODEL", "INIT_WEIGHTS"))
        except (KeyError, AttributeError):
            init = False
        if init:
            try:
                pretrained = _get(cfg, "MODEL", "PRETRAINED")
            except (KeyError, AttributeError):
                pretrained = ""
            model.init_weights(pretrained or "")
    return model


def get_pose_net_shufflenetv2(cfg, is_train, **kwargs):
    """pose_shufflenetv2_10x_pixel_shuffle.py:56-65 (``get_pose_net``): trainable under ``is_train``
    (``init_weights(cfg.MODEL.PRETRAINED)`` when cfg.MODEL.INIT_WEIGHTS says so); otherwise the weights come from
    ``load_state_dict``."""
    return _init_under_is_train(PoseShuffleNetV2Hip(cfg, trainable=bool(is_train), **kwargs), cfg, is_train)


class PoseShuffleNetV2PlusHip(PoseNetHip):
    """pose_shufflenetv2_plus_pixel_shuffle (deep_hrnet/lib/models/pose_shufflenetv2_plus_pixel_shuffle.py:23-55: the
    ShuffleNetV2+ Small / Medium / Large backbone -- 3x3 / 5x5 / 7x7 depthwise convs, hard-swish, squeeze-and-excitation
    --, the pixel-shuffle (DUC) decoder, ``final_layer``) inference through the same C ABI; ``state_dict`` in the
    reference module's key format (``LastSE`` / ``fc`` / ``classifier`` are accepted and unused, as in the reference's
    forward).  Storage modes "f32" and "f16x2" (the depthwise and squeeze-excitation kernels have no bf16 form)."""

    NAME = "pose_shufflenetv2_plus_pixel_shuffle"
    DTYPES = ("f32", "f16x2")

    def __init__(self, cfg, dtype="f32"):
        if dtype not in self.DTYPES:
            raise ValueError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        self.spec = self._spec_of(self.extra, self.num_joints, self.target_type)   # NotImplementedError for an unknown size ...

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .shufflenet_plus_plan import shufflenet_plus_spec
        return shufflenet_plus_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_shufflenet_plus import shufflenet_plus_param_shapes
        sp = self.spec
        return shufflenet_plus_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                            start_channels=sp["start_channels"], architecture=sp["architecture"],
                                            final_kernel=sp["final_kernel"])

    def init_weights(self, pretrained=""):
        raise NotImplementedError("%s: training (and its weight initialisation) is out of scope; load a state_dict" % self.NAME)

    def _make_program(self, h, w):
        from .shufflenet_plus_plan import ShuffleNetV2PlusProgram
        return ShuffleNetV2PlusProgram(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_shufflenetv2_plus(cfg, is_train, **kwargs):
    """pose_shufflenetv2_plus_pixel_shuffle.py:58-67 (``get_pose_net``); inference only -- the weights come from
    ``load_state_dict``."""
    return PoseShuffleNetV2PlusHip(cfg, **kwargs)


class PoseMobileViTv2Hip(_Trainable, PoseNetHip):
    """pose_mobilevitv2_pixel_shuffle (deep_hrnet/lib/models/pose_mobilevitv2_pixel_shuffle.py:23-60: the MobileViTv2
    0.5 / 0.75 / 1.0 backbone -- MobileNetV2 blocks with SiLU, GroupNorm(1, C) and separable self-attention on 2x2
    patches --, the pixel-shuffle (DUC) decoder, ``final_layer``) through the same C ABI; ``state_dict`` in
    the reference module's key format (``backbone.classifier`` is accepted and unused, as in the reference's forward).
    The width comes from MODEL.EXTRA.MODEL_SIZE; MODEL.CONFIG (the reference's second YAML) is accepted and ignored.
    Storage modes "f32" and "f16x2"; input height and width must be multiples of 64.  ``trainable`` (what
    ``MODELS[NAME](cfg, is_train=True)`` sets): the model also has the training surface of ``PoseShuffleNetV2Hip`` --
    ``init_weights``, ``train()``, ``parameters()``, ``trainer()`` (a train.MobileViTv2Trainer, fp32 whatever the storage
    mode of the inference program)."""

    NAME = "pose_mobilevitv2_pixel_shuffle"
    DTYPES = ("f32", "f16x2")
    TRAINS = True                # a net of this class can be built trainable
    TRAINER = "MobileViTv2Trainer"

    def __init__(self, cfg, dtype="f32", trainable=False):
        from .mobilevitv2_plan import mobilevitv2_spec
        if dtype not in self.DTYPES:
            raise NotImplementedError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        self.spec = mobilevitv2_spec(self.extra, self.num_joints, self.target_type)   # NotImplementedError for an unknown size ...
        self.trainable = bool(trainable) and self.TRAINS

    def param_shapes(self):
        from .synth_mobilevitv2 import mobilevitv2_param_shapes
        sp = self.spec
        return mobilevitv2_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                        start_channels=sp["start_channels"], architecture=sp["architecture"],
                                        final_kernel=sp["final_kernel"])

    def init_weights(self, pretrained=""):
        """What the reference's constructor leaves behind (the pose module has no ``init_weights`` of its own).  The
        backbone is ``MobileViTv2.reset_parameters`` = ``initialize_weights`` (backbones/utils/init_utils.py:218-235) under
        backbones/configs/mobilevitv2-*.yaml, which set no ``model.layer.conv_init`` / ``linear_init``: every nn.Conv2d --
        depthwise, qkv_proj, out_proj and the FFN included -- ``kaiming_normal_(mode="fan_out")`` = N(0, 2 / (shape[0] k k))
        with a zero bias, every BatchNorm and GroupNorm weight 1 / bias 0, the classifier's LinearLayer N(0, 0.01) with a
        zero bias.  Decoder / ``final_layer`` keep torch's nn.Conv2d / BatchNorm2d defaults, as in
        ``PoseShuffleNetV2Hip.init_weights``.  A ``pretrained`` that names a local file is read by the rules of the
        reference's ``load_pretrained_model`` (backbones/mobilevitv2.py:55-64): ``torch.load`` gives a bare state_dict
        with the backbone's own keys (no ``backbone.`` prefix) that is loaded STRICTLY -- a missing, unexpected or
        differently sized tensor is a RuntimeError.  Any other truthy value is a FileNotFoundError (the reference logs
        the path and fails in ``torch.load``); nothing is ever downloaded.  Draws come from torch's global generator."""
        import math
        import os
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); load a state_dict" % self.NAME)
        shapes = self.param_shapes()
        sd = {}
        for k, shape in shapes.items():
            backbone = k.startswith("backbone.")
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif k.endswith("running_var"):
                sd[k] = torch.ones(shape)
            elif k.endswith("running_mean"):
                sd[k] = torch.zeros(shape)
            elif backbone and len(shape) == 4:
                sd[k] = torch.randn(shape) * math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
            elif backbone and len(shape) == 2:
                sd[k] = torch.randn(shape) * 0.01             # the classifier's LinearLayer
            elif backbone:                                    # 1-d: a norm's weight / bias, or the bias of a conv / the classifier
                norm = k.endswith(".weight")                  # (no conv or linear weight is 1-d)
                sd[k] = torch.ones(shape) if norm else torch.zeros(shape)
            elif (k.rsplit(".", 1)[0] + ".running_mean") in shapes:
                sd[k] = torch.ones(shape) if k.endswith(".weight") else torch.zeros(shape)
            else:                                             # nn.Conv2d defaults, weight before bias
                w = shapes[k.rsplit(".", 1)[0] + ".weight"]
                bound = 1.0 / math.sqrt(w[1] * w[2] * w[3])
                sd[k] = (torch.rand(shape) * 2 - 1) * bound
        if pretrained:
            if not (isinstance(pretrained, str) and os.path.isfile(pretrained)):
                raise FileNotFoundError("%s: MODEL.PRETRAINED=%r is not a local file (nothing is downloaded)" % (self.NAME, pretrained))
            wts = torch.load(pretrained, map_location="cpu", weights_only=True)
            want = [k[len("backbone."):] for k in shapes if k.startswith("backbone.")]
            missing = [k for k in want if k not in wts and not k.endswith("num_batches_tracked")]
            unexpected = [k for k in wts if k not in want]
            if missing or unexpected:
                raise RuntimeError("%s: pretrained backbone state_dict mismatch: missing %s unexpected %s"
                                   % (self.NAME, missing[:5], unexpected[:5]))
            for k, v in wts.items():
                if tuple(v.shape) != tuple(shapes["backbone." + k]):
                    raise RuntimeError("%s: size mismatch for %s: %s vs %s" % (self.NAME, k, tuple(v.shape), tuple(shapes["backbone." + k])))
                sd["backbone." + k] = v
        return self._set_weights(sd)

    def trainer(self):
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); MODELS[%r](cfg, is_train=True) "
                                      "returns the trainable model" % (self.NAME, self.NAME))
        return super().trainer()

    def _make_trainer(self):
        from . import train
        return getattr(train, self.TRAINER)(self.spec, self.num_joints, self.target_type, self._sd, device=self.device,
                                            dtype="f32")

    def _make_program(self, h, w):
        from .mobilevitv2_plan import MobileViTv2Program
        return MobileViTv2Program(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_mobilevitv2(cfg, is_train, **kwargs):
    """pose_mobilevitv2_pixel_shuffle.py:63-72 (``get_pose_net``): trainable under ``is_train``
    (``init_weights(cfg.MODEL.PRETRAINED)`` when cfg.MODEL.INIT_WEIGHTS says so); otherwise the weights come from
    ``load_state_dict``."""
    return _init_under_is_train(PoseMobileViTv2Hip(cfg, trainable=bool(is_train), **kwargs), cfg, is_train)


class PoseMobileViTHip(PoseNetHip):
    """pose_mobilevit_pixel_shuffle (deep_hrnet/lib/models/pose_mobilevit_pixel_shuffle.py:23-60: the MobileViT xxs / xs /
    s backbone -- MobileNetV2 blocks with SiLU, per-token LayerNorm and four-head soft-max self-attention on 2x2
    patches, fused with the local features by a 3x3 conv --, the pixel-shuffle (DUC) decoder, ``final_layer``) inference
    through the same C ABI; ``state_dict`` in the reference module's key format (``backbone.classifier`` is accepted and
    unused, as in the reference's forward).  The width comes from MODEL.EXTRA.MODEL_SIZE; MODEL.CONFIG (the reference's
    second YAML) is accepted and ignored.  Storage modes "f32" and "f16x2"; input height and width must be multiples
    of 64."""

    NAME = "pose_mobilevit_pixel_shuffle"
    DTYPES = ("f32", "f16x2")

    def __init__(self, cfg, dtype="f32"):
        from .mobilevit_plan import mobilevit_spec
        if dtype not in self.DTYPES:
            raise NotImplementedError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        self.spec = mobilevit_spec(self.extra, self.num_joints, self.target_type)   # NotImplementedError for an unknown size ...

    def param_shapes(self):
        from .synth_mobilevit import mobilevit_param_shapes
        sp = self.spec
        return mobilevit_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                      start_channels=sp["start_channels"], architecture=sp["architecture"],
                                      final_kernel=sp["final_kernel"])

    def init_weights(self, pretrained=""):
        raise NotImplementedError("%s: training (and its weight initialisation) is out of scope; load a state_dict" % self.NAME)

    def _make_program(self, h, w):
        from .mobilevit_plan import MobileViTProgram
        return MobileViTProgram(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_mobilevit(cfg, is_train, **kwargs):
    """pose_mobilevit_pixel_shuffle.py:63-72 (``get_pose_net``); inference only -- the weights come from
    ``load_state_dict``."""
    return PoseMobileViTHip(cfg, **kwargs)


class PoseShuffleNetV2DeconvHip(PoseShuffleNetV2Hip):
    """pose_shufflenetv2_10x (deep_hrnet/lib/models/pose_shufflenetv2_10x.py:22-97): the ShuffleNetV2 backbone of
    ``PoseShuffleNetV2Hip`` with the deconv head of pose_resnet behind ``conv_last`` -- three ConvTranspose2d(4, 2, 1) +
    BN + ReLU, ``final_layer``; spec keys NUM_DECONV_*, DECONV_WITH_BIAS, FINAL_CONV_KERNEL.  The same storage modes and
    MODEL_SIZE refusals."""

    NAME = "pose_shufflenetv2_10x"
    TRAINER = "ShuffleNetV2DeconvTrainer"

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .shufflenet_plan import shufflenet_deconv_spec
        return shufflenet_deconv_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_shufflenet import shufflenet_deconv_param_shapes
        sp = self.spec
        return shufflenet_deconv_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                              deconv_filters=sp["deconv_filters"], final_kernel=sp["final_kernel"],
                                              deconv_with_bias=sp["deconv_with_bias"])


def get_pose_net_shufflenetv2_deconv(cfg, is_train, **kwargs):
    """pose_shufflenetv2_10x.py:100-109 (``get_pose_net``): trainable under ``is_train``, like the pixel-shuffle net."""
    return _init_under_is_train(PoseShuffleNetV2DeconvHip(cfg, trainable=bool(is_train), **kwargs), cfg, is_train)


class PoseShuffleNetV2PlusDeconvHip(PoseShuffleNetV2PlusHip):
    """pose_shufflenetv2_plus (deep_hrnet/lib/models/pose_shufflenetv2_plus.py:22-99): the ShuffleNetV2+ backbone of
    ``PoseShuffleNetV2PlusHip`` with the deconv head of pose_resnet behind ``conv_last`` (1280 channels).  The same
    storage modes and MODEL_SIZE refusal."""

    NAME = "pose_shufflenetv2_plus"

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .shufflenet_plus_plan import shufflenet_plus_deconv_spec
        return shufflenet_plus_deconv_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_shufflenet_plus import shufflenet_plus_deconv_param_shapes
        sp = self.spec
        return shufflenet_plus_deconv_param_shapes(model_size=sp["model_size"], num_joints=self.num_joints, target_type=self.target_type,
                                                   deconv_filters=sp["deconv_filters"], final_kernel=sp["final_kernel"],
                                                   deconv_with_bias=sp["deconv_with_bias"])


def get_pose_net_shufflenetv2_plus_deconv(cfg, is_train, **kwargs):
    """pose_shufflenetv2_plus.py:102-111 (``get_pose_net``); inference only -- the weights come from ``load_state_dict``."""
    return PoseShuffleNetV2PlusDeconvHip(cfg, **kwargs)


class PoseMobileNetV3PixelShuffleHip(_Trainable, PoseNetHip):
    """pose_mobilenetv3_small_pixel_shuffle (deep_hrnet/lib/models/pose_mobilenetv3_small_pixel_shuffle.py:23-52:
    torchvision's MobileNetV3-small ``features`` -- hard-swish, 3x3 / 5x5 depthwise convs, squeeze-excitation with
    biases, BatchNorm eps 1e-3 --, the pixel-shuffle (DUC) decoder, ``final_layer``) through the same C ABI;
    ``state_dict`` in the reference module's key format (``backbone.0.*``).  MODEL_SIZE 'large' is refused (the
    reference cannot run it either).  Storage modes "f32" and "f16x2".  ``trainable`` (what
    ``MODELS[NAME](cfg, is_train=True)`` sets): the model also has the training surface of ``PoseShuffleNetV2Hip`` --
    ``init_weights``, ``train()``, ``parameters()``, ``trainer()`` (a train.MobileNetV3Trainer, fp32 whatever the
    storage mode of the inference program)."""

    NAME = "pose_mobilenetv3_small_pixel_shuffle"
    DTYPES = ("f32", "f16x2")
    TRAINS = True                # a net of this class can be built trainable
    TRAINER = "MobileNetV3Trainer"

    def __init__(self, cfg, dtype="f32", trainable=False):
        if dtype not in self.DTYPES:
            raise NotImplementedError("%s: dtype %r is not supported; supported modes: %s" % (self.NAME, dtype, ", ".join(self.DTYPES)))
        super().__init__(cfg, dtype)
        self.extra = _get(cfg, "MODEL", "EXTRA")
        self.num_joints = int(_get(cfg, "MODEL", "NUM_JOINTS"))
        self.target_type = _get(cfg, "MODEL", "TARGET_TYPE")
        self.spec = self._spec_of(self.extra, self.num_joints, self.target_type)   # NotImplementedError for 'large' ...
        self.trainable = bool(trainable) and self.TRAINS

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .mobilenetv3_plan import mobilenetv3_ps_spec
        return mobilenetv3_ps_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_mobilenetv3 import mobilenetv3_ps_param_shapes
        sp = self.spec
        return mobilenetv3_ps_param_shapes(num_joints=self.num_joints, target_type=self.target_type, start_channels=sp["start_channels"],
                                           architecture=sp["architecture"], final_kernel=sp["final_kernel"])

    def init_weights(self, pretrained=""):
        """What the reference's constructor leaves behind (the pose modules have no ``init_weights`` of their own).  The
        backbone is torchvision's ``MobileNetV3.__init__``: every Conv2d -- depthwise and squeeze-excitation included --
        ``kaiming_normal_(mode="fan_out")`` = N(0, 2 / (shape[0] k k)), conv biases 0, BatchNorm 1 / 0.  Decoder / deconv
        head / ``final_layer`` keep torch's nn.Conv2d / ConvTranspose2d / BatchNorm2d defaults, as in
        ``PoseShuffleNetV2Hip.init_weights``.  The reference hands any truthy ``PRETRAINED`` to torchvision, which
        downloads ImageNet weights (backbones/mobilenetv3.py:5-10; the recipe's value is the string "yes please"); this
        code never reaches for the network: a ``pretrained`` that names a file on disk is read as torchvision's own
        checkpoint -- a bare state_dict or one under "state_dict", ``module.`` stripped, ``features.N.`` ->
        ``backbone.0.N.``, ``classifier.*`` ignored, non-strict by name and size --, any other truthy value keeps the
        constructor initialisation and logs one warning.  Draws come from torch's global generator."""
        import logging
        import math
        import os
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); load a state_dict" % self.NAME)
        shapes = self.param_shapes()
        sd = {}
        for k, shape in shapes.items():
            backbone = k.startswith("backbone.")
            bn = (k.rsplit(".", 1)[0] + ".running_mean") in shapes
            if k.endswith("num_batches_tracked"):
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif k.endswith("running_var"):
                sd[k] = torch.ones(shape)
            elif k.endswith("running_mean"):
                sd[k] = torch.zeros(shape)
            elif bn:
                sd[k] = torch.ones(shape) if k.endswith(".weight") else torch.zeros(shape)
            elif backbone and len(shape) == 4:
                sd[k] = torch.randn(shape) * math.sqrt(2.0 / (shape[0] * shape[2] * shape[3]))
            elif backbone:
                sd[k] = torch.zeros(shape)                    # the squeeze-excitation's conv biases
            else:                                             # nn.Conv2d / nn.ConvTranspose2d defaults, weight before bias
                w = shapes[k.rsplit(".", 1)[0] + ".weight"]
                bound = 1.0 / math.sqrt(w[1] * w[2] * w[3])   # (ConvTranspose2d: torch takes fan_in from dim 1 there too)
                sd[k] = (torch.rand(shape) * 2 - 1) * bound
        if pretrained and isinstance(pretrained, str) and os.path.isfile(pretrained):
            ckpt = torch.load(pretrained, map_location="cpu", weights_only=True)
            if isinstance(ckpt, dict) and isinstance(ckpt.get("state_dict"), dict):
                ckpt = ckpt["state_dict"]
            for name, v in ckpt.items():
                name = name[7:] if name.startswith("module.") else name
                if not name.startswith("features."):
                    continue                                  # classifier.* and anything else that is not the backbone
                name = "backbone.0." + name[len("features."):]
                if name in sd and tuple(v.shape) == tuple(sd[name].shape):
                    sd[name] = v                              # non-strict: a missing or differently sized tensor keeps its init
        elif pretrained:
            logging.getLogger(__name__).warning(
                "%s: MODEL.PRETRAINED=%r is not a file; the reference would download torchvision's ImageNet weights here -- "
                "keeping the constructor initialisation", self.NAME, pretrained)
        return self._set_weights(sd)

    def trainer(self):
        if not self.trainable:
            raise NotImplementedError("%s: built with is_train=False (inference only); MODELS[%r](cfg, is_train=True) "
                                      "returns the trainable model" % (self.NAME, self.NAME))
        return super().trainer()

    def _make_trainer(self):
        from . import train
        return getattr(train, self.TRAINER)(self.spec, self.num_joints, self.target_type, self._sd, device=self.device,
                                            dtype="f32")

    def _make_program(self, h, w):
        from .mobilenetv3_plan import MobileNetV3Program
        return MobileNetV3Program(self._sd, self.spec, h, w, self.dtype)


def get_pose_net_mobilenetv3_pixel_shuffle(cfg, is_train, **kwargs):
    """pose_mobilenetv3_small_pixel_shuffle.py:55-64 (``get_pose_net``): trainable under ``is_train``
    (``init_weights(cfg.MODEL.PRETRAINED)`` when cfg.MODEL.INIT_WEIGHTS says so -- without the reference's download);
    otherwise the weights come from ``load_state_dict``."""
    return _init_under_is_train(PoseMobileNetV3PixelShuffleHip(cfg, trainable=bool(is_train), **kwargs), cfg, is_train)


class PoseMobileNetV3Hip(PoseMobileNetV3PixelShuffleHip):
    """pose_mobilenetv3_small (deep_hrnet/lib/models/pose_mobilenetv3_small.py): the same backbone with the deconv head
    of pose_resnet -- three ConvTranspose2d(4, 2, 1) + BN + ReLU, ``final_layer``."""

    NAME = "pose_mobilenetv3_small"
    TRAINER = "MobileNetV3DeconvTrainer"

    @staticmethod
    def _spec_of(extra, num_joints, target_type):
        from .mobilenetv3_plan import mobilenetv3_deconv_spec
        return mobilenetv3_deconv_spec(extra, num_joints, target_type)

    def param_shapes(self):
        from .synth_mobilenetv3 import mobilenetv3_deconv_param_shapes
        sp = self.spec
        return mobilenetv3_deconv_param_shapes(num_joints=self.num_joints, target_type=self.target_type, deconv_filters=sp["deconv_filters"],
                                               final_kernel=sp["final_kernel"], deconv_with_bias=sp["deconv_with_bias"])


def get_pose_net_mobilenetv3(cfg, is_train, **kwargs):
    """pose_mobilenetv3_small.py (``get_pose_net``): trainable under ``is_train``, like the pixel-shuffle net."""
    return _init_under_is_train(PoseMobileNetV3Hip(cfg, trainable=bool(is_train), **kwargs), cfg, is_train)


MODELS = {"pose_hrnet": get_pose_net, "pose_hrnet_psa": get_pose_net_psa, "pose_resnet": get_pose_net_resnet,
          "pose_resnet_psa": get_pose_net_resnet_psa,
          "pose_shufflenetv2_10x_pixel_shuffle": get_pose_net_shufflenetv2,
          "pose_shufflenetv2_plus_pixel_shuffle": get_pose_net_shufflenetv2_plus,
          "pose_mobilevitv2_pixel_shuffle": get_pose_net_mobilevitv2,
          "pose_mobilevit_pixel_shuffle": get_pose_net_mobilevit,
          "pose_shufflenetv2_10x": get_pose_net_shufflenetv2_deconv,
          "pose_shufflenetv2_plus": get_pose_net_shufflenetv2_plus_deconv,
          "pose_mobilenetv3_small_pixel_shuffle": get_pose_net_mobilenetv3_pixel_shuffle,
          "pose_mobilenetv3_small": get_pose_net_mobilenetv3}
