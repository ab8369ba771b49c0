"""The validation pass of a device-resident TF2 LeNet-1 population, and the flag it raises.

In the reference a device raises ``training_end`` from its own validation loss: once per epoch
it runs its Keras model forward over the shared test set in batches, averages the batch losses
and ends when the average falls under ``target_loss``
(``federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:430-455``;
the model is ``create_q_model``, condition 0, ``:158-194``: LeNet-1, 2 202 parameters; the drivers
without ``crossentropy`` in their name validate on their Huber objective,
``federated_learning_keras_consensus_FL_MNIST.py:481-483``: ``loss="huber"``).
``LenetValidation`` holds what that pass needs (the test set, the batching, the target and the
cost buffers) and runs it for all D devices in one ``cfa_lenet_eval_loss_f32`` call: every device's
model stays in LDS for its batches, and the flags are written where the populations keep them.

The model family is the "LeNet-1 family" ``geom = (side, kernel, c1, c2, classes)``::

    [side, side, 1] -> Conv2D(c1, kernel, valid, relu) -> AveragePooling2D(2)
                    -> Conv2D(c2, kernel, valid, relu) -> AveragePooling2D(2)
                    -> Flatten -> Dense(classes, softmax)

or, with ``pool="max"``, the same chain with ``MaxPooling2D(2)`` in both places: the drivers'
other two models, ``MNIST_CNN32`` (``-modelselection 1``) and ``MNIST_CNN14`` (any other value),
through ``cfa_lenet_max_eval_loss_f32``, whose kernels read the model from global memory instead
of holding it in LDS. A geometry of seven numbers, ``(side, channels, kernel, c1, c2, hidden, classes)``,
is the CIFAR drivers' hidden-layer LeNet (``CIFAR_LENET``,
``federated_learning_keras_consensus_FL_threads_CIFAR_crossentropy.py:179-186``): images
``[side, side, channels]``, the average-pool chain, then ``Dense(hidden, relu) -> Dense(classes,
softmax)``, through ``cfa_lenet_hidden_eval_loss_f32``. A model row is in ``get_weights()`` order (``lenet_layer_shapes``), the row layout
``PopulationOptimizer`` and the populations already use. The populations are not edited; the
chain of one epoch is::

    val.validate(pop.models, skip=pop.ended, ended=pop.ended)
    grads = train.gradients(pop.models, skip=pop.ended)      # tf2_training.LenetTraining
    opt.step(pop.models, grads, pop.ended)
    train.advance(pop.ended)
    pop.rounds(1)

and all of it may be captured into a graph: ``validate`` reads nothing back.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import lenet_family, lenet_loss_kind, lenet_pool

__all__ = ["LenetValidation", "lenet_size", "lenet_layer_shapes", "LENET1", "MNIST_CNN32", "MNIST_CNN14",
           "CIFAR_LENET"]

LENET1 = (28, 5, 4, 8, 10)        # create_q_model, condition 0: pool="avg"
MNIST_CNN32 = (28, 3, 32, 64, 10)  # condition 1 (``:170-182``), 34 826 parameters: pool="max"
MNIST_CNN14 = (28, 3, 14, 64, 10)  # any other -modelselection, 24 278 parameters: pool="max"
# the CIFAR_crossentropy drivers' -modelselection 1, seven numbers (side, channels, kernel, c1, c2, hidden,
# classes), 28 130 parameters: a hidden Dense(128, relu) before the output layer, pool="avg"
CIFAR_LENET = (32, 3, 5, 4, 8, 128, 10)
MAX_CLASSES = 64            # the library's limit (CFA_E_UNSUPPORTED beyond)


def _stages(geom: Sequence[int]) -> tuple:
    """(side, kernel, c1, c2, classes, p2) of a geometry of five numbers, or of seven (side,
    channels, kernel, c1, c2, hidden, classes: the hidden-layer family, see ``_family``);
    ValueError for one without a model."""
    if len(geom) == 7:
        side, channels, k, c1, c2, hidden, classes = (int(v) for v in geom)
        if min(side, channels, k, c1, c2, hidden, classes) < 1:
            raise ValueError("side, channels, kernel, c1, c2, hidden and classes must be >= 1")
    else:
        if len(geom) != 5:
            raise ValueError("geom must be (side, kernel, c1, c2, classes)")
        side, k, c1, c2, classes = (int(v) for v in geom)
        if min(side, k, c1, c2, classes) < 1:
            raise ValueError("side, kernel, c1, c2 and classes must be >= 1")
    s1 = side - k + 1
    p1 = s1 // 2 if s1 > 0 else 0
    s2 = p1 - k + 1
    p2 = s2 // 2 if s2 > 0 else 0
    if p2 < 1:
        raise ValueError(f"geometry {tuple(geom)} leaves no second pooled map (p2 < 1)")
    return side, k, c1, c2, classes, p2


def _family(geom: Sequence[int], pool: str = "avg") -> tuple:
    """(geom as ints, an image's shape, its text) of a geometry: [side, side] for five numbers,
    [side, side, channels] for seven (the channel axis is always there, also at channels == 1).
    ValueError for a geometry without a model, and for seven numbers with ``pool="max"`` (the
    drivers build no such model)."""
    _stages(geom)
    geom, _, image = lenet_family(geom, pool)
    return geom, image, ", ".join(str(v) for v in image)


def lenet_layer_shapes(geom: Sequence[int]) -> list:
    """The six ``get_weights()`` shapes of the family: K1 (k, k, 1, c1), b1, K2 (k, k, c1, c2), b2,
    Wd (flat, classes), bd, with flat = p2 * p2 * c2; or the eight of a seven-number geometry:
    K1 (k, k, channels, c1), b1, K2, b2, Wh (flat, hidden), bh, Wd (hidden, classes), bd. They feed
    ``local_optim.layer_offsets``."""
    _, k, c1, c2, classes, p2 = _stages(geom)
    if len(geom) == 7:
        channels, hidden = int(geom[1]), int(geom[5])
        return [(k, k, channels, c1), (c1,), (k, k, c1, c2), (c2,), (p2 * p2 * c2, hidden), (hidden,),
                (hidden, classes), (classes,)]
    return [(k, k, 1, c1), (c1,), (k, k, c1, c2), (c2,), (p2 * p2 * c2, classes), (classes,)]


def lenet_size(geom: Sequence[int]) -> int:
    """Parameters of a model of the family (LeNet-1: 2 202; ``CIFAR_LENET``: 28 130)."""
    return sum(int(np.prod(s, dtype=np.int64)) for s in lenet_layer_shapes(geom))


class LenetValidation:
    """The validation cost of D LeNet-family models and their ``training_end`` flags, on the GPU."""

    @staticmethod
    def check(geom: Sequence[int], x_shape: Sequence[int], labels_shape: Sequence[int], batch: int,
              batches: Optional[int] = None, target: Optional[float] = None, log_cap: int = 0,
              labels: Optional[np.ndarray] = None, loss: str = "xent", pool: str = "avg") -> dict:
        """The host half: validates geometry, shapes and batching without touching a device and
        returns geom, P, Nt, batch, batches, per_device (D, or 0 for the shared set) and target.
        ``x_shape`` is [Nt, side, side] (the set all devices share) or [D, Nt, side, side], and
        ``labels_shape`` [Nt] or [D, Nt]. ``batches=None`` is the driver's ``int(Nt / batch)``.
        ``labels`` (a host array, optional) is checked to lie in [0, classes). ValueError for a
        geometry without a model (p2 < 1) or with more than 64 classes, mismatched shapes,
        ``batch * batches > Nt``, a non-finite target, a negative ``log_cap``, a label out of
        range, a ``loss`` other than "xent" or "huber" (the plan is the same for both) and a
        ``pool`` other than "avg" or "max". A ``geom`` of seven numbers (``CIFAR_LENET``) takes
        ``x_shape`` [Nt, side, side, channels] or [D, Nt, side, side, channels]; ``hidden < 1``, a
        missing channel axis and ``pool="max"`` are ValueErrors."""
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
        Nt = xs[-n - 1]
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        batches = Nt // batch if batches is None else int(batches)
        if batches < 1 or batch * batches > Nt:
            raise ValueError(f"{batches} batches of {batch} samples do not fit the {Nt} of the test set")
        if target is not None and not np.isfinite(float(target)):
            raise ValueError("target must be finite, or None")
        if int(log_cap) < 0:
            raise ValueError("log_cap must be >= 0")
        if labels is not None:
            lab = np.asarray(labels)
            if tuple(lab.shape) != ls or not np.issubdtype(lab.dtype, np.integer):
                raise ValueError(f"labels must be an integer array of shape {ls}")
            if lab.size and (lab.min() < 0 or lab.max() >= classes):
                raise ValueError(f"labels must lie in [0, {classes})")
        return {"geom": geom, "P": lenet_size(geom), "Nt": Nt, "batch": batch,
                "batches": batches, "per_device": xs[0] if len(xs) == n + 2 else 0,
                "target": None if target is None else float(target)}

    def __init__(self, engine, geom: Sequence[int], x_test: torch.Tensor, labels: torch.Tensor, batch: int,
                 batches: Optional[int] = None, target: Optional[float] = None, log_cap: int = 0,
                 loss: str = "xent", pool: str = "avg"):
        """``x_test`` [Nt, side, side] fp32 / ``labels`` [Nt] int32 (contiguous CUDA): the test
        set every device validates on, or [D, Nt, side, side] / [D, Nt] with one set per device.
        ``target``: the driver's ``target_loss``, needed to raise flags. ``log_cap`` > 0 keeps a
        [log_cap, D] log of the cost on the device: call e goes to row min(e, log_cap - 1). The
        labels are checked once, here, to lie in [0, classes) (reads two values back:
        synchronises). ``loss``: the drivers' objective, "xent" (``*_crossentropy*``:
        ``-log softmax(z)[label]``) or "huber" (the others, e.g.
        ``federated_learning_keras_consensus_FL_MNIST.py:481-483``: ``keras.losses.Huber()``
        between the integer label itself and the softmax probability of the true class).
        ``pool``: "avg" (LeNet-1) or "max" (``MNIST_CNN32``, ``MNIST_CNN14``). With a geometry of
        seven numbers (``CIFAR_LENET``) ``x_test`` is [Nt, side, side, channels] or
        [D, Nt, side, side, channels]."""
        info = self.check(geom, x_test.shape, labels.shape, batch, batches, target, log_cap, loss=loss, pool=pool)
        self.engine, self.geom, self.P, self.loss_kind, self.pool = engine, info["geom"], info["P"], loss, pool
        self.x_test, self.labels = x_test, labels
        self.Nt, self.batch, self.batches, self.target = info["Nt"], info["batch"], info["batches"], info["target"]
        self.per_device, self.log_cap = info["per_device"], int(log_cap)
        if labels.dtype != torch.int32 or not labels.is_cuda:
            raise TypeError("labels must be an int32 CUDA tensor")
        lo, hi = int(labels.min().item()), int(labels.max().item())
        if lo < 0 or hi >= self.geom[-1]:
            raise ValueError(f"labels must lie in [0, {self.geom[-1]})")
        self.D = 0  # set by the first validate(): the buffers follow the population's size
        self.val_cost = self.val_log = self.workspace = None
        self.epoch_counter = torch.zeros(1, dtype=torch.int64, device=engine.device)

    def _buffers(self, D: int) -> None:
        if self.per_device and D != self.per_device:
            raise ValueError(f"the test set holds {self.per_device} devices' samples, the models {D} devices")
        dev = self.engine.device
        self.D = D
        self.val_cost = torch.zeros(D, dtype=torch.float64, device=dev)
        self.val_log = torch.zeros(self.log_cap, D, dtype=torch.float64, device=dev) if self.log_cap > 0 else None
        family = (self.geom,) if len(self.geom) == 7 else ()  # the hidden-layer entries' own workspace
        self.workspace = self.engine.lenet_workspace(D, self.batches, self.pool, *family)

    def allocate(self, D: int) -> "LenetValidation":
        """Allocates ``val_cost`` [D] fp64, ``val_log`` and the workspace for D devices now (the
        first ``validate`` does it otherwise; a captured ``validate`` must not allocate)."""
        if self.D != int(D):
            self._buffers(int(D))
        return self

    @property
    def epochs_done(self) -> int:
        """Calls logged so far (reads the device counter back: synchronises)."""
        return int(self.epoch_counter[0].item())

    def validate(self, models: torch.Tensor, skip: Optional[torch.Tensor] = None,
                 ended: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """The validation pass of every device of ``models`` [D, P]: ``val_cost`` [D] written (and
        its row of ``val_log``), ``models`` untouched. ``skip``: int32 [D] CUDA flags, a flagged
        device has left its loop and its cost and flag are not touched. ``ended``: int32 [D] CUDA,
        ``ended[d] |= val_cost[d] < target``; it may be ``skip`` itself
        (``PopulationRound.ended``, ``FedAvgPopulation.ended``). No host read: capture-safe once
        the buffers exist (``allocate``)."""
        if models.dim() != 2 or int(models.shape[1]) != self.P:
            raise ValueError(f"models must be [D, {self.P}], got {tuple(models.shape)}")
        if ended is not None and self.target is None:
            raise ValueError("raising flags needs a target")
        self.allocate(int(models.shape[0]))
        logged = self.val_log is not None
        return self.engine.lenet_eval(self.geom, self.x_test, self.labels, models, self.batch, self.batches,
                                      self.val_cost, self.workspace, skip, self.target or 0.0, ended,
                                      self.val_log, self.epoch_counter if logged else None, stream,
                                      loss=self.loss_kind, pool=self.pool)
