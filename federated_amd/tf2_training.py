"""The local batches of a device-resident TF2 LeNet-1 population: the gradient on the device.

Between two consensus rounds every device of the reference runs ``number_of_batches`` local
updates: ``loss = reduce_mean(-sum(onehot * log(model(x))))``, ``tape.gradient`` and
``optimizer.apply_gradients``
(``federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:321-337``),
and in the gradient-exchange variants it evaluates a neighbour's model on a batch of its own data
and publishes that gradient (``:360-385``). The drivers without ``crossentropy`` in their name
train on ``keras.losses.Huber()`` between the label and the true class's probability instead
(``federated_learning_keras_consensus_FL_MNIST.py:369-377``): ``loss="huber"``. ``LenetTraining`` holds what those steps need (the
training set, the batch size, each device's position in its set, the gradient and loss buffers)
and computes all D gradients in one ``cfa_lenet_grad_loss_f32`` call, for the model family, geometry and
row layout of ``tf2_validation`` (``lenet_layer_shapes``); ``pool="max"`` serves the drivers'
max-pool CNNs (``MNIST_CNN32``, ``MNIST_CNN14``) through ``cfa_lenet_max_grad_loss_f32``, and a
geometry of seven numbers the CIFAR drivers' hidden-layer LeNet (``CIFAR_LENET``, images
``[side, side, channels]``) through ``cfa_lenet_hidden_grad_loss_f32``. With ``PopulationOptimizer`` and
``LenetValidation`` one epoch of a population stays on the device::

    val.validate(pop.models, skip=pop.ended, ended=pop.ended)
    train.epoch(pop.models, opt, number_of_batches, skip=pop.ended)
    pop.rounds(1)

and all of it may be captured into a graph once the buffers exist (``allocate``): nothing is read
back, and the batch positions advance on the device.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import lenet_loss_kind, lenet_pool

from .tf2_validation import (CIFAR_LENET, LENET1, MAX_CLASSES, MNIST_CNN14, MNIST_CNN32, _family, _stages,
                             lenet_layer_shapes, lenet_size)

__all__ = ["LenetTraining", "lenet_size", "lenet_layer_shapes", "LENET1", "MNIST_CNN32", "MNIST_CNN14",
           "CIFAR_LENET"]


class LenetTraining:
    """The minibatch loss and gradient of D LeNet-family models, on the GPU."""

    @staticmethod
    def check(geom: Sequence[int], x_shape: Sequence[int], labels_shape: Sequence[int], batch: int,
              labels: Optional[np.ndarray] = None, src: Optional[np.ndarray] = None,
              D: Optional[int] = None, loss: str = "xent", pool: str = "avg") -> dict:
        """The host half: validates geometry, shapes and the batch without touching a device and
        returns geom, P, Nt, batch and per_device (D, or 0 for the shared set). ``x_shape`` is
        [Nt, side, side] (the set all devices share) or [D, Nt, side, side], and ``labels_shape``
        [Nt] or [D, Nt]. ``labels`` (a host array, optional) is checked to lie in [0, classes);
        ``src`` (a host array, optional; needs ``D`` or a per-device set) to be one integer per
        device in [0, D). ValueError for a geometry without a model (p2 < 1) or with more than
        64 classes, mismatched shapes, ``batch`` below 1 or above Nt, a label or a ``src`` out of
        range, a ``D`` that disagrees with a per-device set, a ``loss`` other than "xent" or
        "huber" (the plan is the same for both) and a ``pool`` other than "avg" or "max". A
        ``geom`` of seven numbers (``CIFAR_LENET``) takes ``x_shape`` [Nt, side, side, channels] or
        [D, Nt, side, side, channels]; ``hidden < 1``, a missing channel axis and ``pool="max"``
        are ValueErrors."""
        lenet_loss_kind(loss)
        lenet_pool(pool)
        classes = _stages(geom)[4]
        geom, image, text = _family(geom, pool)
        if classes > MAX_CLASSES:
            raise ValueError(f"more than {MAX_CLASSES} classes")
        xs, ls = tuple(int(v) for v in x_shape), tuple(int(v) for v in labels_shape)
        n = len(image)
        if len(xs) not in (n + 1, n + 2) or xs[-n:] != image or ls != xs[:-n] or min(xs) < 1:
            raise ValueError(f"x must be [Nt, {text}] with labels [Nt], or [D, Nt, {text}] with "
                             f"labels [D, Nt]; got {xs} and {ls}")
        Nt, per_device = xs[-n - 1], xs[0] if len(xs) == n + 2 else 0
        batch = int(batch)
        if batch < 1 or batch > Nt:
            raise ValueError(f"a batch of {batch} samples does not fit the {Nt} of the training set")
        if D is not None and (int(D) < 1 or (per_device and int(D) != per_device)):
            raise ValueError(f"D = {D} with a training set of {per_device or 'shared'} devices' samples")
        if labels is not None:
            lab = np.asarray(labels)
            if tuple(lab.shape) != ls or not np.issubdtype(lab.dtype, np.integer):
                raise ValueError(f"labels must be an integer array of shape {ls}")
            if lab.size and (lab.min() < 0 or lab.max() >= classes):
                raise ValueError(f"labels must lie in [0, {classes})")
        if src is not None:
            n = per_device if D is None else int(D)
            if not n:
                raise ValueError("checking src needs D (the set is shared)")
            s = np.asarray(src)
            if s.shape != (n,) or not np.issubdtype(s.dtype, np.integer):
                raise ValueError(f"src must hold one integer per device ({n})")
            if s.min() < 0 or s.max() >= n:
                raise ValueError(f"src must lie in [0, {n})")
        return {"geom": geom, "P": lenet_size(geom), "Nt": Nt, "batch": batch,
                "per_device": per_device}

    def __init__(self, engine, geom: Sequence[int], x_train: torch.Tensor, labels: torch.Tensor, batch: int,
                 loss: str = "xent", pool: str = "avg"):
        """``x_train`` [Nt, side, side] fp32 / ``labels`` [Nt] int32 (contiguous CUDA): the
        training set every device draws its batches from, or [D, Nt, side, side] / [D, Nt] with
        one set per device (the drivers' case). The labels are checked once, here, to lie in
        [0, classes) (reads two values back: synchronises). ``loss``: the drivers' objective,
        "xent" (``*_crossentropy*``) or "huber" (the others, e.g.
        ``federated_learning_keras_consensus_FL_MNIST.py:369-377``: ``keras.losses.Huber()``
        between the integer label itself and the softmax probability of the true class); it is
        kept as ``loss_kind`` (``loss`` is the buffer of the batch losses). ``pool``: "avg"
        (LeNet-1) or "max" (``MNIST_CNN32``, ``MNIST_CNN14``). With a geometry of seven numbers
        (``CIFAR_LENET``) ``x_train`` is [Nt, side, side, channels] or [D, Nt, side, side, channels]."""
        info = self.check(geom, x_train.shape, labels.shape, batch, loss=loss, pool=pool)
        self.engine, self.geom, self.P, self.loss_kind, self.pool = engine, info["geom"], info["P"], loss, pool
        self.x_train, self.labels = x_train, labels
        self.Nt, self.batch, self.per_device = info["Nt"], info["batch"], info["per_device"]
        if labels.dtype != torch.int32 or not labels.is_cuda:
            raise TypeError("labels must be an int32 CUDA tensor")
        lo, hi = int(labels.min().item()), int(labels.max().item())
        if lo < 0 or hi >= self.geom[-1]:
            raise ValueError(f"labels must lie in [0, {self.geom[-1]})")
        self.D = 0  # set by allocate(), or by the first gradients()
        self.grads = self.loss = self.cursor = self.workspace = None

    def allocate(self, D: int) -> "LenetTraining":
        """Allocates ``grads`` [D, P] fp32 (rows pitched to 16 bytes, the populations' pitch),
        ``loss`` [D] fp32, ``cursor`` [D] int64 (zeros: every device starts at its first sample)
        and the workspace for D devices now (the first ``gradients`` does it otherwise; a captured
        one must not allocate)."""
        D = int(D)
        if self.D == D:
            return self
        if D < 1 or (self.per_device and D != self.per_device):
            raise ValueError(f"the training set holds {self.per_device or 'shared'} devices' samples, "
                             f"the models {D} devices")
        dev = self.engine.device
        self.D = D
        self.grads = torch.zeros(D, (self.P + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :self.P]
        self.loss = torch.zeros(D, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(D, dtype=torch.int64, device=dev)
        self.workspace = self.engine.lenet_grad_workspace(D, self.batch, self.geom, self.pool)
        return self

    def gradients(self, models: torch.Tensor, src=None, skip: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                  stream=None) -> torch.Tensor:
        """The gradient of every device's batch loss at ``models`` [D, P]: written to ``out``
        (default ``grads``) and returned, the losses to ``loss``. Device d's batch is samples
        ``first[d] .. first[d] + batch - 1`` (mod Nt) of its set; ``first`` ([D] int64 CUDA)
        defaults to ``cursor``. ``src``: device d evaluates row ``src[d]`` of ``models`` on its
        own data (an int32 [D] CUDA tensor, taken as it is, or a host array, checked against
        [0, D) and copied: not capture-safe). ``skip``: int32 [D] CUDA flags, a flagged device's
        row and loss are not touched. No host read: capture-safe once the buffers exist
        (``allocate``)."""
        if models.dim() != 2 or int(models.shape[1]) != self.P:
            raise ValueError(f"models must be [D, {self.P}], got {tuple(models.shape)}")
        self.allocate(int(models.shape[0]))
        if src is not None and not isinstance(src, torch.Tensor):
            self.check(self.geom, self.x_train.shape, self.labels.shape, self.batch, src=np.asarray(src), D=self.D)
            src = torch.as_tensor(np.asarray(src, dtype=np.int32), device=self.engine.device)
        return self.engine.lenet_grad(self.geom, self.x_train, self.labels, models, self.batch,
                                      self.grads if out is None else out, self.workspace, self.loss, src,
                                      self.cursor if first is None else first, skip, stream,
                                      loss_kind=self.loss_kind, pool=self.pool)

    def advance(self, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``cursor[d] = (cursor[d] + batch) % Nt`` for every device not flagged in ``skip``, on
        the device (no host read: capture-safe)."""
        nxt = (self.cursor + self.batch) % self.Nt
        self.cursor.copy_(nxt if skip is None else torch.where(skip != 0, self.cursor, nxt))
        return self.cursor

    def epoch(self, models: torch.Tensor, opt, batches: int, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The driver's local update (``:321-337``): ``batches`` times ``gradients(models,
        skip=skip)``, ``opt.step(models, grads, skip)`` (a ``PopulationOptimizer``) and
        ``advance(skip)``. Returns ``models``."""
        for _ in range(int(batches)):
            grads = self.gradients(models, skip=skip)
            opt.step(models, grads, skip)
            self.advance(skip)
        return models
