"""FedAvg parameter-server rounds on a device-resident population.

The reference's PS drivers (``federated_learning_keras_PS_MNIST.py`` and its CIFAR / radar copies,
the MQTT ``PS_server.py`` + ``learner_consensus.py`` pair) run one round as: the server folds the
epoch's active devices' models into the global model in list order
(``parameter_server_v2.py:146-161``, ``p <- p + u * (x_k - p) / C``; the transfer-learning step
``:150-157`` once a folded device reported ``training_end``), then every device takes the
published model, as a copy (``federated_learning_keras_PS_MNIST.py:307-309``) or by the MQTT
learner's mix (``learner_consensus.py:151-152``). ``FedAvgPopulation`` runs that round as ONE
launch (``cfa_fedavg_population_round_f32``) on a [D, P] stack: the active lists of every epoch
(``indexes_tx``), the ended flags and the round counter live in device memory, so rounds replay
as graphs with no host work between them, and the fold is the reference's fp32 chain bit for bit.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._graphs import RoundGraphs
from .engine import Engine
from .topology import _RoundCounter, _check_sched, active_schedule

_CLIENTS = {"none": _lib.CLIENT_NONE, "copy": _lib.CLIENT_COPY, "mix": _lib.CLIENT_MIX}


class FedAvgPopulation(_RoundCounter):
    """D simulated devices' models ``models`` [D, P] and the server's global model ``params`` [P]
    (fp32 CUDA tensors on the engine's device, both updated in place), one launch per round."""

    def __init__(self, engine: Engine, models: torch.Tensor, params: torch.Tensor, update_factor: float):
        if not isinstance(models, torch.Tensor) or models.dim() != 2 or models.dtype != torch.float32 \
                or not models.is_cuda:
            raise ValueError("models must be a [D, P] fp32 CUDA tensor")
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or not params.is_cuda \
                or params.dim() != 1 or params.numel() != models.shape[1] or not params.is_contiguous():
            raise ValueError("params must be a contiguous fp32 CUDA tensor of P elements")
        self.engine, self.models, self.params = engine, models, params
        self.update_factor = float(update_factor)
        self.ended = torch.zeros(models.shape[0], dtype=torch.int32, device=models.device)
        self._tables = None  # (act_ptr, act_idx, act_div, act_rdiv) device tensors
        self._client = (_lib.CLIENT_COPY, 1.0, 1.0)
        self._graphs: Optional[RoundGraphs] = None

    def set_schedule(self, lists_per_table, sched: Optional[Sequence[int]] = None, client: str = "copy",
                     client_factor: float = 1.0, client_divisor: float = 1.0) -> None:
        """``lists_per_table``: the reference's ``indexes_tx`` ([A, E] integer array, column e =
        the active devices of epoch e, parameter_server_v2.py:88) or a list of ragged lists of
        device ids, in fold order, duplicates allowed; round r folds list ``sched[r % S]``
        (``sched=None``: every list in turn). ``client``: "copy" (every device loads the published
        model), "mix" (``w + client_factor * (g - w) / client_divisor``, the MQTT learner with
        factor 1 and divisor 2; divisor 1 is the plain ``w + eps * (g - w)``) or "none" (only
        ``params`` is written). The counter starts at 0 (``reset_round``, ``round_index``). A
        refused schedule leaves the population as it was."""
        dev = self.models.device
        tables, sched, client = self.check_schedule(self.models.shape[0], lists_per_table, sched, client,
                                                    client_factor, client_divisor)
        self._counts = np.diff(tables[0])
        self._slots = sched
        self._tables = tuple(torch.from_numpy(a).to(dev) for a in tables)
        self._client = client
        self._new_schedule(torch.tensor(sched, dtype=torch.int32, device=dev))

    @staticmethod
    def check_schedule(devices: int, lists_per_table, sched=None, client: str = "copy", client_factor: float = 1.0,
                       client_divisor: float = 1.0):
        """The host half of ``set_schedule`` (no device is touched): the arguments checked, and
        ((act_ptr, act_idx, act_div, act_rdiv) numpy tables, sched as a list, (client rule,
        factor, divisor)) as the upload takes them. ValueError for an unknown client rule, a
        client divisor that is zero or not finite in fp32, a device id outside [0, devices), no
        table, no slot, or a slot outside the tables."""
        if client not in _CLIENTS:
            raise ValueError("client must be 'copy', 'mix' or 'none'")
        if client == "mix":
            with np.errstate(over="ignore"):
                d32 = np.float32(client_divisor)
            if not np.isfinite(d32) or d32 == 0:
                raise ValueError("client_divisor must be finite and non-zero in fp32")
        ptr, idx, div, rdiv = active_schedule(lists_per_table, devices)
        T = ptr.size - 1
        if T < 1:
            raise ValueError("a schedule needs at least one table")
        sched = _check_sched(sched, T)
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.int32)  # never read: a device array cannot be empty
        return (ptr, idx, div, rdiv), sched, (_CLIENTS[client], float(client_factor), float(client_divisor))

    def set_ended(self, ids) -> None:
        """The devices that reported ``training_end`` (all others are cleared). Written in the
        order of the current stream: rounds already enqueued or replayed there see the old flags,
        later ones the new."""
        D = self.models.shape[0]
        flags = np.zeros(D, dtype=np.int32)
        for k in ids:
            if not 0 <= int(k) < D:
                raise ValueError(f"device id {k} is outside [0, {D})")
            flags[int(k)] = 1
        self.ended.copy_(torch.from_numpy(flags), non_blocking=False)

    def round(self, stream=None) -> None:
        """One round on ``stream`` (None: the current stream)."""
        if self._tables is None:
            raise RuntimeError("set_schedule() first")
        client, factor, divisor = self._client
        self.engine.fedavg_round(self.models, self.params, *self._tables, self.update_factor, *self._sched,
                                 self.ended, client, factor, divisor, stream)

    def rounds(self, R: int, graph: bool = True) -> None:
        """R rounds on the current stream; ``graph=True`` replays captured rounds (hipGraph)
        instead of launching each from Python, with the same results bit for bit."""
        if self._tables is None:
            raise RuntimeError("set_schedule() first")
        if not graph:
            for _ in range(R):
                self.round()
            return
        if self._graphs is None:
            self._graphs = RoundGraphs(self.models.device, self.round, 1, lambda: 0)
        self._graphs.run(R)

    def bytes_per_round(self) -> int:
        """Bytes the next round moves (reads the round counter back: synchronises): the global
        model read and written once, the C active rows read, and per client rule D rows written
        ("copy"), read and written ("mix") or nothing ("none"). The ended flags are not looked at
        (a transfer-learning round reads one row instead of C)."""
        D, P = self.models.shape
        C = int(self._counts[self._slots[self.round_index % len(self._slots)]])
        client = self._client[0]
        reads = (C + 1) + (D if client == _lib.CLIENT_MIX else 0)
        writes = (1 if C else 0) + (D if client != _lib.CLIENT_NONE else 0)
        return (reads + writes) * P * 4
