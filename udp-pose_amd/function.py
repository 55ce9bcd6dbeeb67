"""``train`` / ``validate`` with the reference's call shapes (deep_hrnet/lib/core/function.py:27-111,
:114-255) and the criteria of lib/core/loss.py, all arithmetic in libudp_pose_hip.so.

* ``JointsMSELoss`` / ``JointsMSELoss_offset`` (loss.py:15-39 / :41-76): callables returning the loss
  value(s) as device fp64 scalars (``udp_mse_loss``); ``.last_grad`` holds d loss / d output.
* ``train(config, train_loader, model, criterion, optimizer, epoch, ...)``: ``model`` is what
  ``MODELS[name](cfg, is_train=True)`` returned; its trainer (a ``train.Trainer``: HRNet or pose_resnet) owns parameters, Adam moments and the
  backward.  ``criterion`` and ``optimizer`` are honoured (use_target_weight; lr / betas / eps per batch) and
  anything the kernels do not implement (another loss, SGD, weight decay) raises instead of being ignored.
* ``validate(config, val_loader, val_dataset, model, criterion, ...)``: forward + mirrored forward in one
  launch sequence, ``udp_flip_fuse``, loss, ``get_final_preds``; fills ``all_preds`` / ``all_boxes`` exactly as
  :212-221 does and hands them to ``val_dataset.evaluate`` when the dataset has one.
Logging / tensorboard / debug images of the reference are out of scope.
"""
import os

import numpy as np
import torch

from . import _lib
from .inference import get_final_preds
from .transforms import flip_fuse


def _cfg(config, *path, default=None):
    cur = config
    for p in path:
        try:
            cur = cur[p] if isinstance(cur, dict) else getattr(cur, p)
        except (KeyError, AttributeError):
            return default
    return cur


class JointsMSELoss:
    """loss.py:15-39.  ``use_target_weight=False`` weights every joint with 1."""
    is_offset = False

    def __init__(self, use_target_weight=True):
        self.use_target_weight = use_target_weight
        self.last_grad = None

    def _run(self, output, target, target_weight):
        if not output.is_cuda:
            raise RuntimeError("udp-pose_amd has no CPU path: the criterion needs device tensors")
        output, target = output.contiguous(), target.contiguous()
        b, c = output.shape[:2]
        j = c // 3 if self.is_offset else c
        w = target_weight.reshape(b, j).to(torch.float32).contiguous() if self.use_target_weight else \
            torch.ones(b, j, dtype=torch.float32, device=output.device)
        loss = torch.zeros(2, dtype=torch.float64, device=output.device)
        self.last_grad = torch.empty_like(output)
        _lib.check(_lib.lib().udp_mse_loss(output.data_ptr(), target.data_ptr(), w.data_ptr(), b, j,
                                           output.shape[2] * output.shape[3], int(self.is_offset), loss.data_ptr(),
                                           self.last_grad.data_ptr(), _lib.stream_ptr()))
        return loss

    def __call__(self, output, target, target_weight):
        return self._run(output, target, target_weight)[0]


class JointsMSELoss_offset(JointsMSELoss):
    """loss.py:41-76: returns (loss_hm, loss_os)."""
    is_offset = True

    def __call__(self, output, target, target_weight):
        loss = self._run(output, target, target_weight)
        return loss[0], loss[1]


def accuracy(output, target, hm_type="gaussian", thr=0.5):
    """lib/core/evaluate.py:40-73: PCK on heat-maps (prediction arg-max vs ground-truth arg-max, distances in
    units of a tenth of the map size, joints whose target arg-max is at x <= 1 or y <= 1 ignored).  The two
    arg-max passes run on the device (udp_decode_gaussian); the [N,J] bookkeeping is host NumPy as there.
    Returns (acc [J+1], avg_acc, cnt, pred [N,J,2])."""
    from .inference import decode_device
    if hm_type != "gaussian":
        raise NotImplementedError("accuracy: hm_type %r (the reference only ever passes 'gaussian')" % hm_type)

    def max_preds(hm):
        hm = hm if isinstance(hm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hm, dtype=np.float32))
        hm = hm.cuda() if not hm.is_cuda else hm
        n, j, h, w = hm.shape
        one = torch.ones(n, 2, dtype=torch.float64)
        _, maxvals, _, idx = decode_device(hm, one, one, "gaussian", False, 4.0, True)
        idx, mv = idx.cpu().numpy().astype(np.int64), maxvals.cpu().numpy()[..., 0]
        p = np.stack([idx % w, idx // w], axis=2).astype(np.float32)
        return p * (mv > 0.0)[..., None].astype(np.float32)                # get_max_preds: zero where max <= 0
    n, j, h, w = output.shape
    pred, tgt = max_preds(output), max_preds(target)
    norm = np.ones((n, 2)) * np.array([h, w]) / 10
    dists = np.full((j, n), -1.0)
    ok = (tgt[..., 0] > 1) & (tgt[..., 1] > 1)
    d = np.linalg.norm(pred / norm[:, None, :] - tgt / norm[:, None, :], axis=2)
    dists[ok.T] = d.T[ok.T]
    acc = np.zeros(j + 1)
    avg, cnt = 0.0, 0
    for i in range(j):
        valid = dists[i] != -1
        acc[i + 1] = (dists[i][valid] < thr).sum() * 1.0 / valid.sum() if valid.sum() > 0 else -1
        if acc[i + 1] >= 0:
            avg += acc[i + 1]
            cnt += 1
    avg = avg / cnt if cnt else 0
    if cnt:
        acc[0] = avg
    return acc, avg, cnt, pred


def get_optimizer(cfg, model):
    """lib/utils/utils.py:60-76.  TRAIN.OPTIMIZER 'adam' -> ``Adam(model.parameters(), lr=cfg.TRAIN.LR)``.  'sgd' is
    refused: the training step implements the Adam rule only."""
    name = str(_cfg(cfg, "TRAIN", "OPTIMIZER", default="adam")).lower()
    if name != "adam":
        raise NotImplementedError("TRAIN.OPTIMIZER=%r: the HIP training step implements Adam (utils.py:70-74) only" % name)
    return Adam(model.parameters(), lr=float(_cfg(cfg, "TRAIN", "LR", default=1e-3)))


class Adam:
    """Stand-in for ``torch.optim.Adam(params, lr)`` with its defaults: holds the hyper-parameters in
    ``param_groups`` (so ``MultiStepLR``-style schedulers can rewrite ``lr``); the moments live in the trainer and
    the update itself is ``udp_adam_step``.  A real ``torch.optim.Adam`` over ``model.parameters()`` is accepted
    by ``train`` too."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        self.param_groups = [dict(params=list(params), lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                  amsgrad=amsgrad)]

    def zero_grad(self):
        pass                                               # every gradient is overwritten by the backward


def _adam_hyper(optimizer):
    """(lr, betas, eps) of the optimizer handed to train(); anything the Adam kernel does not implement is refused."""
    if type(optimizer).__name__ != "Adam" or len(optimizer.param_groups) != 1:
        raise NotImplementedError("train(): optimizer %s is not supported -- pass Adam over model.parameters() "
                                  "(one parameter group)" % type(optimizer).__name__)
    g = optimizer.param_groups[0]
    if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
        raise NotImplementedError("train(): Adam with weight_decay / amsgrad / maximize is not implemented")
    return float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"])


def _check_criterion(criterion, target_type):
    """The backward starts from the gradient of JointsMSELoss / JointsMSELoss_offset (loss.py:15-76); any other
    criterion (e.g. JointsOHKMMSELoss) would silently train a different objective -> refused."""
    name = type(criterion).__name__
    want = "JointsMSELoss_offset" if target_type == "offset" else "JointsMSELoss"
    if name != want:
        raise NotImplementedError("train(): criterion %s is not supported with TARGET_TYPE=%s (expected %s)"
                                  % (name, target_type, want))
    return bool(getattr(criterion, "use_target_weight", True))


def train(config, train_loader, model, criterion, optimizer, epoch=0, output_dir=None, tb_log_dir=None,
          writer_dict=None, world_size=1):
    """function.py:27-111: ``model.train()``, then per batch forward -> criterion -> backward -> optimizer step.
    ``model`` is what ``MODELS[name](cfg, is_train=True)`` returned (or any train.Trainer); ``criterion`` must be
    JointsMSELoss / JointsMSELoss_offset and ``optimizer`` Adam over ``model.parameters()`` -- their
    hyper-parameters (use_target_weight; lr, betas, eps, re-read every batch) are honoured, anything else raises.
    Returns the sample-weighted mean loss of the epoch (what ``losses.avg`` holds)."""
    from .train import Trainer
    if isinstance(model, Trainer):
        trainer = model
    else:
        model.train()
        trainer = model.trainer()
    use_tw = _check_criterion(criterion, trainer.target_type)
    total, count = torch.zeros(2, dtype=torch.float64, device=trainer.device), 0
    for input, target, target_weight, meta in train_loader:
        n = input.shape[0]
        trainer.lr, trainer.betas, trainer.eps = _adam_hyper(optimizer)
        tw = target_weight.to(trainer.device, non_blocking=True) if use_tw else \
            torch.ones(n, trainer.num_joints, 1, dtype=torch.float32, device=trainer.device)
        x, tg = input.to(trainer.device, non_blocking=True).contiguous(), target.to(trainer.device, non_blocking=True)
        if os.environ.get("UDP_POSE_NO_TRAIN_GRAPH") is None:
            # the step replayed as hipGraph(s) (same results); N > 1: in segments between the gradient buckets'
            # all-reduces, which the host issues while the next segment runs
            loss = trainer.train_step_graphed(x, tg, tw, world_size=world_size)
        else:
            loss = trainer.train_step(x, tg, tw, world_size=world_size)
        if not isinstance(model, Trainer):
            model._stale = True
        total += loss * n
        count += n
    return float(total.sum().item()) / max(count, 1)


def validate(config, val_loader, val_dataset, model, criterion=None, output_dir=None, tb_log_dir=None, writer_dict=None):
    """function.py:114-255.  Returns ``val_dataset.evaluate(...)``'s (name_values, perf_indicator) when the dataset
    provides it, else (all_preds, all_boxes, image_path, mean_loss)."""
    num_joints = int(_cfg(config, "MODEL", "NUM_JOINTS"))
    tt = _cfg(config, "MODEL", "TARGET_TYPE", default="gaussian")
    flip_test = bool(_cfg(config, "TEST", "FLIP_TEST", default=False))
    flip_pairs = getattr(val_dataset, "flip_pairs", None)
    num_samples = len(val_dataset)
    all_preds = np.zeros((num_samples, num_joints, 3), dtype=np.float32)
    all_boxes = np.zeros((num_samples, 6))
    image_path, idx = [], 0
    loss_sum, loss_n = 0.0, 0
    if hasattr(model, "eval"):
        model.eval()                                       # function.py:121: switch to evaluate mode
    for input, target, target_weight, meta in val_loader:
        x = input.to(model.device if model.device is not None else "cuda").contiguous()
        n = x.shape[0]
        if flip_test:
            raw = model.raw_forward(x, flip_test=True)
            output = flip_fuse(raw[:n], raw[n:], flip_pairs, tt == "offset")
        else:
            output = model(x).clone()
        if criterion is not None:
            loss = criterion(output, target.to(output.device), target_weight.to(output.device))
            loss = loss[0] + loss[1] if isinstance(loss, tuple) else loss
            loss_sum += float(loss.item()) * n
            loss_n += n
        c = np.asarray(meta["center"])
        s = np.asarray(meta["scale"])
        score = np.asarray(meta["score"]) if "score" in meta else np.ones(n)
        preds, maxvals, _ = get_final_preds(config, output, c, s)
        all_preds[idx:idx + n, :, 0:2] = preds[:, :, 0:2]
        all_preds[idx:idx + n, :, 2:3] = maxvals
        all_boxes[idx:idx + n, 0:2] = c[:, 0:2]
        all_boxes[idx:idx + n, 2:4] = s[:, 0:2]
        all_boxes[idx:idx + n, 4] = np.prod(s * 200, 1)
        all_boxes[idx:idx + n, 5] = score
        image_path.extend(meta["image"] if "image" in meta else [""] * n)
        idx += n
    mean_loss = loss_sum / max(loss_n, 1)
    if hasattr(val_dataset, "evaluate"):
        return val_dataset.evaluate(config, all_preds, output_dir, all_boxes, image_path, [], [])
    return all_preds, all_boxes, image_path, mean_loss
