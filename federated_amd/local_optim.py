"""The local optimizer step of a device-resident TF2 population between two consensus rounds.

Every TF2 driver of the reference runs, on every device and between two calls of the consensus
class, ``optimizer.apply_gradients(zip(grads, model.trainable_variables))``
(``federated_learning_keras_consensus_FL_MNIST.py:363-381`` and its copies) with one of three
optimizers: ``Adam(learning_rate=mu, clipnorm=1.0)``, ``SGD(learning_rate=mu, momentum=0.9)`` or
``SGD(learning_rate=mu2)``. ``PopulationOptimizer`` holds what that step needs for D devices
(the layer table, the Adam / momentum state, the per-device step counters) and steps the whole
[D, P] stack in one ``cfa_optim_step_f32`` call. The gradients stay the caller's: the Keras models
are not part of this library.

A device that ended, or that saw an ended neighbour, takes no more local steps
(``training_signal``, ``:361``, ``:416-418``): ``step(..., skip=pop.ended)`` with the flags a
``PopulationRound`` or ``FedAvgPopulation`` keeps on the device. The caller's loop is::

    grads = ...                                  # the caller's models, [D, P]
    opt.step(pop.models, grads, pop.ended)
    pop.rounds(1)

and the whole of it may be captured into a graph by the caller: ``step`` reads nothing back.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["PopulationOptimizer", "layer_offsets"]

_RULES = {"sgd": _lib.OPTIM_SGD, "momentum": _lib.OPTIM_MOMENTUM, "adam": _lib.OPTIM_ADAM}


def layer_offsets(shapes) -> np.ndarray:
    """The int32 [n + 1] layer table of a model bucket from its layers' shapes in
    ``get_weights()`` order (a scalar layer, shape ``()``, holds one element). ValueError for no
    layer, an empty layer or a bucket beyond int32."""
    sizes = []
    for s in shapes:
        dims = [int(d) for d in (s if isinstance(s, (tuple, list)) else tuple(np.atleast_1d(s)))]
        sizes.append(int(np.prod(dims, dtype=np.int64)) if dims else 1)
    if not sizes or min(sizes) < 1:
        raise ValueError("a layer table needs at least one layer and no empty layer")
    ptr = np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64))))
    if ptr[-1] > np.iinfo(np.int32).max:
        raise ValueError("the bucket does not fit an int32 layer table")
    return ptr.astype(np.int32)


class PopulationOptimizer:
    """The local optimizer (SGD, Keras momentum SGD, Keras Adam) of D devices, on the GPU."""

    @staticmethod
    def check(D: int, layers, rule: str, lr: float, momentum: float = 0.0, beta_1: float = 0.9,
              beta_2: float = 0.999, epsilon: float = 1e-7, clipnorm: Optional[float] = None,
              trainable: Optional[Sequence] = None, P: Optional[int] = None) -> dict:
        """The host half: validates the arguments without touching a device and returns
        D, P, n, rule (the library's constant), layer_ptr (int32 [n + 1]), trainable (int32 [n]),
        state (how many [D, P] state arrays the rule keeps) and clipnorm (0.0: no clip).
        ``layers`` is a list of layer shapes or an offsets table; an offsets table must start at
        0, increase strictly and, with ``P`` given, end at P. ValueError for anything else that
        is out of range (an unknown rule, D < 1, a beta outside [0, 1), a non-finite lr or
        momentum, a negative epsilon or clipnorm, a ``trainable`` of the wrong length)."""
        if rule not in _RULES:
            raise ValueError("rule must be 'sgd', 'momentum' or 'adam'")
        D = int(D)
        if D < 1:
            raise ValueError("D must be >= 1")
        # an offsets table: a numpy array, or a list of plain integers that starts at 0 (no layer is empty)
        is_table = isinstance(layers, np.ndarray) or (
            len(layers) > 0 and all(isinstance(s, (int, np.integer)) for s in layers) and int(layers[0]) == 0)
        if is_table:
            table = np.asarray(layers)
            if table.ndim != 1 or table.size < 2 or not np.issubdtype(table.dtype, np.integer):
                raise ValueError("an offsets table is a 1-D integer array of n + 1 >= 2 entries")
            table = table.astype(np.int64)
            if table[0] != 0 or np.any(np.diff(table) <= 0):
                raise ValueError("the layer table must start at 0 and increase strictly")
            if table[-1] > np.iinfo(np.int32).max:
                raise ValueError("the bucket does not fit an int32 layer table")
            table = table.astype(np.int32)
        else:
            table = layer_offsets(layers)
        n = table.size - 1
        if P is not None and int(table[-1]) != int(P):
            raise ValueError(f"the layer table ends at {int(table[-1])}, not at P = {int(P)}")
        if trainable is None:
            flags = np.ones(n, dtype=np.int32)
        else:
            flags = (np.asarray(trainable).reshape(-1) != 0).astype(np.int32)
            if flags.size != n:
                raise ValueError(f"trainable holds {flags.size} flags for {n} layers")
        with np.errstate(over="ignore"):
            if not np.isfinite(np.float32(lr)):
                raise ValueError("lr must be finite in fp32")
            if rule == "momentum" and not np.isfinite(np.float32(momentum)):
                raise ValueError("momentum must be finite in fp32")
        clip = 0.0
        if rule == "adam":
            for name, b in (("beta_1", beta_1), ("beta_2", beta_2)):
                if not 0.0 <= float(b) < 1.0:
                    raise ValueError(f"{name} must lie in [0, 1)")
            if not float(epsilon) >= 0.0:
                raise ValueError("epsilon must be >= 0")
            if clipnorm is not None:
                clip = float(clipnorm)
                if not clip > 0.0 or not np.isfinite(clip):
                    raise ValueError("clipnorm must be positive and finite, or None")
        elif clipnorm is not None:
            raise ValueError("clipnorm belongs to the 'adam' rule (the reference clips nothing else)")
        return {"D": D, "P": int(table[-1]), "n": n, "rule": _RULES[rule], "layer_ptr": table, "trainable": flags,
                "state": {"sgd": 0, "momentum": 1, "adam": 2}[rule], "clipnorm": clip}

    def __init__(self, engine, D: int, layers, rule: str, lr: float, *, momentum: float = 0.0, beta_1: float = 0.9,
                 beta_2: float = 0.999, epsilon: float = 1e-7, clipnorm: Optional[float] = None,
                 trainable: Optional[Sequence] = None):
        """``layers``: the model's layer shapes in ``get_weights()`` order, or its offsets table;
        ``trainable``: one flag per layer (None: all), a layer with 0 is never touched. Allocates
        the rule's state (rows padded to 16 bytes, so that aligned models are streamed in
        vectors), the counters and, for Adam with ``clipnorm``, the workspace on the engine's
        device."""
        info = self.check(D, layers, rule, lr, momentum, beta_1, beta_2, epsilon, clipnorm, trainable)
        self.engine, self.rule_name = engine, rule
        self.D, self.P, self.n_layers, self.rule = info["D"], info["P"], info["n"], info["rule"]
        self.lr, self.momentum, self.beta_1, self.beta_2 = float(lr), float(momentum), float(beta_1), float(beta_2)
        self.epsilon, self.clipnorm = float(epsilon), info["clipnorm"]
        dev = engine.device
        self.layer_ptr = torch.from_numpy(info["layer_ptr"]).to(dev)
        self.trainable = torch.from_numpy(info["trainable"]).to(dev)
        self._trainable_elems = int(np.diff(info["layer_ptr"].astype(np.int64))[info["trainable"] != 0].sum())
        pitch = (self.P + 3) // 4 * 4
        self._state = torch.zeros(info["state"], self.D, pitch, dtype=torch.float32, device=dev)
        self.m = self._state[0, :, :self.P] if info["state"] >= 1 else None
        self.v = self._state[1, :, :self.P] if info["state"] >= 2 else None
        self.t = torch.zeros(self.D, dtype=torch.int64, device=dev)
        self.pow = torch.ones(self.D, 2, dtype=torch.float64, device=dev) if rule == "adam" else None
        self.workspace = engine.optim_workspace(self.D, self.P, self.n_layers) if self.clipnorm > 0.0 else None

    @property
    def steps_done(self) -> np.ndarray:
        """Steps every device has taken, int64 [D] (reads ``t`` back: synchronises)."""
        return self.t.cpu().numpy()

    def step(self, models: torch.Tensor, grads: torch.Tensor, skip: Optional[torch.Tensor] = None,
             stream=None) -> torch.Tensor:
        """One optimizer step of every device: ``models`` [D, P] in place with ``grads`` [D, P]
        (fp32 CUDA, unit element stride, any row pitch). ``skip``: int32 [D] CUDA flags, a
        flagged device is not touched at all (``PopulationRound.ended``,
        ``FedAvgPopulation.ended``). No host read: capture-safe."""
        if tuple(models.shape) != (self.D, self.P):
            raise ValueError(f"models must be [{self.D}, {self.P}], got {tuple(models.shape)}")
        return self.engine.optim_step(self.rule, models, grads, self.layer_ptr, self.trainable, self.t, self.lr,
                                      self.m, self.v, self.pow, skip, self.momentum, self.beta_1, self.beta_2,
                                      self.epsilon, self.clipnorm, self.workspace, stream)

    def reset(self) -> None:
        """State and counters back to those of a new optimizer, in the order of the current stream."""
        self._state.zero_()
        self.t.zero_()
        if self.pow is not None:
            self.pow.fill_(1.0)

    def state_dict(self) -> dict:
        """Copies of the state: ``m`` / ``v`` [D, P] (None where the rule keeps none), ``t`` [D]
        int64 and ``pow`` [D, 2] fp64, as tensors on the device."""
        return {"m": None if self.m is None else self.m.clone(), "v": None if self.v is None else self.v.clone(),
                "t": self.t.clone(), "pow": None if self.pow is None else self.pow.clone()}

    def load_state_dict(self, state: dict) -> None:
        """Takes back what ``state_dict`` returned (in the order of the current stream)."""
        for name in ("m", "v", "t", "pow"):
            mine, theirs = getattr(self, name), state.get(name)
            if (mine is None) != (theirs is None):
                raise ValueError(f"state '{name}' does not belong to the '{self.rule_name}' rule")
            if mine is not None:
                if tuple(theirs.shape) != tuple(mine.shape) or theirs.dtype != mine.dtype:
                    raise ValueError(f"state '{name}' must be {tuple(mine.shape)} {mine.dtype}")
                mine.copy_(theirs)

    def bytes_per_step(self) -> int:
        """Algorithmic bytes of one step with no device skipped: per trainable parameter, w read
        and written and g read (SGD, 12 B), plus the accumulator read and written (momentum,
        20 B), plus v read and written (Adam, 28 B), plus g read once more under the clip (32 B)."""
        per = {"sgd": 12, "momentum": 20, "adam": 28}[self.rule_name] + (4 if self.clipnorm > 0.0 else 0)
        return per * self.D * self._trainable_elems
