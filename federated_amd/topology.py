"""Topology service: the reference's neighbour-selection rules emitted as CSR
tables for the one-launch population kernel (``cfa_mix_population_f32``).

The reference computes each device's neighbour list inside that device's process
(TF1 ``cfa.py:14-32``, ``cfa_ongraphs.py:18-52``; TF2 ``consensus_v3.py:44-70``,
``consensus_v4.py:111-173``) and its mixing coefficients from an eps policy. For a simulated
population resident on one GPU, this module builds, for all D devices at once:

    csr_ptr[D+1], csr_idx[E], csr_coef[E]  (first entry of each row = the device itself)

with the same ordered neighbour lists (the same random draws when the rule is random, using
the same RNG calls) and the same per-step alphas, so one launch reproduces D per-device calls.
"""
from __future__ import annotations

import random
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .consensus import _tf1, _tf2
from ._graphs import RoundGraphs
from .engine import Engine
from .local_training import LocalTrainingHooks

RULE_SEQUENTIAL = 0
# auto-select the window round above this bucket size: below it the whole population sits in
# the 256 MB Infinity Cache and the single CSR launch already reuses rows (tools/probe/
# window_threshold.py, profiles/r01_window_threshold.jsonl: 32 devices, K = 4: CSR 24.9 vs
# window 34.5 us at P = 262K; window 73 vs CSR 133 us at 1.07M, 123 vs 256 at 2M)
WINDOW_MIN_P = 1 << 19


# -- neighbour lists for every device ---------------------------------------------------------
def kregular_tf1(devices: int, neighbors: int) -> List[List[int]]:
    """cfa.py:14-32 for every device."""
    return [_tf1.kregular(ii, neighbors, devices).tolist() for ii in range(devices)]


def kregular_v3(devices: int, neighbors: int) -> List[List[int]]:
    """consensus_v3.py:44-70 for every device (at least 2 neighbours)."""
    return [_tf2.kregular_v3(ii, neighbors, devices).tolist() for ii in range(devices)]


def ring_v4(devices: int, neighbors: int) -> List[List[int]]:
    """consensus_v4.py:111-141 for every device (N < 2: in-neighbour ii-1)."""
    return [np.atleast_1d(_tf2.kregular_ring(ii, neighbors, devices)).tolist() for ii in range(devices)]


def mobile(graph: np.ndarray, g: int, max_neighbors: Optional[int] = None, devices: Optional[int] = None,
           rng: Optional[random.Random] = None) -> List[List[int]]:
    """Row ii of adjacency ``graph[:, :, g]`` for every device (cfa_mobilenet.py:36-47); with
    ``max_neighbors`` the cfa_ongraphs.py:46-48 draw ``random.choices(k=max_neighbors)`` (with
    replacement) is applied per device in device order, on ``rng`` (default: the global
    ``random`` module, as the reference)."""
    devices = graph.shape[0] if devices is None else devices
    draw = (rng or random).choices
    out = []
    for ii in range(devices):
        row = graph[ii, :, g]
        nb = [kk for kk in range(devices) if row[kk] == 1]
        if max_neighbors is not None and len(nb) > max_neighbors:
            nb = [int(x) for x in draw(np.asarray(nb, dtype=np.uint8), k=max_neighbors)]
        out.append(nb)
    return out


# -- eps policies: per-step alphas of the sequential rule -------------------------------------
def alphas_tf2(nbrs: Sequence[int], ii: int, devices: int) -> List[float]:
    """TF2 weights (consensus_v3.py:145): eps = 1/(n+1) for every step."""
    n = len(nbrs)
    return [1 / (n + 1)] * n


def alphas_tf1_cfa(eps: float, neighbors: int) -> Callable:
    """cfa.py:66-69: eps * b/(b + (N-1) b) with N the configured neighbour count."""
    return lambda nbrs, ii, devices: [eps * _tf1.weight_factor(devices, ii, int(j), neighbors - 1) for j in nbrs]


def alphas_tf1_ongraphs(eps: float) -> Callable:
    """cfa_ongraphs.py:109-113: eps * b/(b + n b) with n this call's neighbour count."""
    return lambda nbrs, ii, devices: [eps * _tf1.weight_factor(devices, ii, int(j), len(nbrs)) for j in nbrs]


def csr(lists: Sequence[Sequence[int]], policy: Callable, devices: Optional[int] = None, coef_dtype=np.float32):
    """(ptr, idx, coef) numpy arrays; row d = [d] + lists[d], coef = [1] + alphas."""
    return schedule_csr([lists], policy, devices, coef_dtype)


def schedule_csr(lists_per_table: Sequence[Sequence[Sequence[int]]], policy: Callable, devices: Optional[int] = None,
                 coef_dtype=np.float32, neighbor_base: int = 0, self_coef: float = 1.0):
    """The CSR tables of a topology schedule (``cfa_mix_population_sched_f32``), one per entry of
    ``lists_per_table``: (ptr[T * (D+1)], idx, coef) numpy arrays. Table t is
    ptr[t*(D+1) : (t+1)*(D+1)], its offsets absolute positions in the idx / coef all tables
    share: ``csr(lists_per_table[t], policy)`` with ptr shifted by the entries before it.
    Row d = [d] + [neighbor_base + j for j in its list], coef = [self_coef] + alphas.
    ``neighbor_base=D, self_coef=0.0`` is the ``Tf1PopulationRound`` layout (the neighbours'
    published models are rows D .. 2D-1 of its source table; the local entry's coefficient is
    unused)."""
    ptr, idx, coef = [], [], []
    for lists in lists_per_table:
        D = len(lists) if devices is None else devices
        ptr.append(len(idx))
        for d, nb in enumerate(lists):
            idx += [d] + [neighbor_base + int(j) for j in nb]
            coef += [float(self_coef)] + [float(a) for a in policy(nb, d, D)]
            ptr.append(len(idx))
    return (np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32),
            np.asarray(coef, dtype=coef_dtype))


def active_schedule(lists_per_table, devices: int):
    """The active tables of a FedAvg parameter-server schedule
    (``cfa_fedavg_population_round_f32``): (act_ptr[T + 1] int32, act_idx int32, act_div[T] fp32,
    act_rdiv[T] fp64) numpy arrays. ``lists_per_table`` is the reference's ``indexes_tx`` as an
    [A, E] integer array (column e is table e: parameter_server_v2.py:88, ``active_devices =
    self.indexes_tx[:, epoch]``), or a list of ragged lists; table t's device ids, in fold order
    and with duplicates kept, are act_idx[act_ptr[t] : act_ptr[t + 1]] (absolute offsets, as
    ``schedule_csr``). act_div[t] is the list's length C as fp32 and act_rdiv[t] the fp64
    reciprocal 1.0 / act_div[t] the kernel divides with; an empty list takes the divisor 1, which
    is never used. Ids outside [0, devices) are refused."""
    if isinstance(lists_per_table, np.ndarray):
        if lists_per_table.ndim != 2 or lists_per_table.dtype.kind not in "iu":
            raise ValueError("an indexes_tx array must be a 2-D [A, E] integer array")
        lists_per_table = [lists_per_table[:, e].tolist() for e in range(lists_per_table.shape[1])]
    ptr, idx = [0], []
    for t, ids in enumerate(lists_per_table):
        for k in ids:
            if int(k) != k or not 0 <= int(k) < devices:
                raise ValueError(f"table {t}: device id {k} is outside [0, {devices})")
            idx.append(int(k))
        ptr.append(len(idx))
    if len(idx) >= 2 ** 31:
        raise ValueError("the active lists hold more than 2^31 - 1 entries")
    div = np.asarray([max(b - a, 1) for a, b in zip(ptr, ptr[1:])], dtype=np.float32)
    return (np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32), div, 1.0 / div.astype(np.float64))


def _check_sched(sched, T: int) -> List[int]:
    """``sched`` as a list of table indices checked against the table count on the host (the
    kernels trust it); None = every table in turn."""
    sched = list(range(T)) if sched is None else [int(t) for t in sched]
    if not sched:
        raise ValueError("a schedule needs at least one slot")
    for i, t in enumerate(sched):
        if not 0 <= t < T:
            raise ValueError(f"sched[{i}] = {t} is outside the {T} tables")
    return sched


def _upload_schedule(lists_per_table, policy, sched, D, dev, **layout):
    """Device tensors of a schedule: ((ptr, idx, coef), sched [S] int32), ``sched`` checked
    against the table count on the host (the kernel trusts it); None = every table in turn."""
    T = len(lists_per_table)
    if T < 1 or any(len(lists) != D for lists in lists_per_table):
        raise ValueError(f"a schedule needs at least one table, each of {D} neighbour lists")
    sched = _check_sched(sched, T)
    tables = tuple(torch.from_numpy(a).to(dev) for a in schedule_csr(lists_per_table, policy, D, **layout))
    return tables, torch.tensor(sched, dtype=torch.int32, device=dev)


def window_shape(lists: Sequence[Sequence[int]], alphas: Sequence[Sequence[float]], max_side: int = 4):
    """(hl, hr) when every device d's list is the ring window [d-hl .. d-1, d+1 .. d+hr] (mod D)
    in that order and its alphas are one value, else None: such populations mix with
    cfa_mix_window_f32 passes instead of the CSR kernel."""
    D = len(lists)
    if D == 0:
        return None
    nb0 = [int(j) for j in lists[0]]
    for cand_hl in range(0, min(len(nb0), max_side) + 1):
        cand_hr = len(nb0) - cand_hl
        if cand_hr > max_side or cand_hl + cand_hr >= D:
            continue
        ok = True
        for d in range(D):
            want = [(d + o) % D for o in list(range(-cand_hl, 0)) + list(range(1, cand_hr + 1))]
            if [int(j) for j in lists[d]] != want or len(set(float(a) for a in alphas[d])) > 1:
                ok = False
                break
        if ok:
            return cand_hl, cand_hr
    return None


def _zero_on(t: torch.Tensor, stream) -> None:
    """Zero ``t`` in the order of ``stream`` (the stream the kernel that accumulates into it runs
    on; None = the current stream), so the reset cannot race a launch on another stream."""
    if stream is None:
        t.zero_()
        return
    with torch.cuda.stream(stream):
        t.zero_()


def _mix_tf1(engine: Engine, dst, src, tables, sched, compress, kept, D: int, P: int, stream) -> None:
    """One TF1 population round: ``compress`` = (mode, cbegin, cend), ``kept`` zeroed ahead of a
    compressing launch, under the schedule ``sched`` = (sched, round) or, with None, one table."""
    mode, cb, ce = compress
    if mode:
        _zero_on(kept, stream)
    if sched is not None:
        engine.population_sched_tf1(dst, src, *tables, *sched, D, P, stream, mode, cb, ce, kept if mode else None)
    else:
        engine.population_tf1(dst, src, *tables, D, P, stream, mode, cb, ce, kept if mode else None)


class _RoundCounter:
    """The round counter of a scheduled population: one device word that the scheduled kernels
    read (round r mixes with table sched[r % S]) and advance, so it needs no host between rounds.
    Each population owns its own."""

    _sched = None  # (sched [S] int32, round [1] int64) device tensors under set_schedule()

    def _new_schedule(self, sched: torch.Tensor) -> None:
        self._sched = (sched, torch.zeros(1, dtype=torch.int64, device=sched.device))
        self._graphs = None
        self._epoch_graphs = None

    def reset_round(self, r: int = 0) -> None:
        """The next round is round ``r`` (it mixes with table sched[r % S]); written in the order
        of the current stream, so rounds already enqueued there keep their tables."""
        if self._sched is None:
            raise RuntimeError("set_schedule() first")
        if r < 0:
            raise ValueError("the round index must be >= 0")
        self._sched[1].fill_(int(r))

    @property
    def round_index(self) -> int:
        """The number of the next round: rounds run since the last ``reset_round`` plus its
        ``r`` (reads the device word back: synchronises)."""
        if self._sched is None:
            raise RuntimeError("set_schedule() first")
        return int(self._sched[1].item())


_ENDED_RULES = {"copy": _lib.ENDED_COPY, "truncate": _lib.ENDED_TRUNCATE, "truncate_eps": _lib.ENDED_TRUNCATE_EPS}


def ended_rule_code(rule: Optional[str]) -> Optional[int]:
    """The library's constant of a ``set_ended_rule`` rule name; None stays None (the rule off)."""
    if rule is not None and rule not in _ENDED_RULES:
        raise ValueError("rule must be None, 'copy', 'truncate' or 'truncate_eps'")
    return None if rule is None else _ENDED_RULES[rule]


def ended_flags(ids, devices: int) -> np.ndarray:
    """int32 [devices] flags, 1 for every id in ``ids``; an id outside [0, devices) is refused."""
    flags = np.zeros(devices, dtype=np.int32)
    for k in ids:
        if int(k) != k or not 0 <= int(k) < devices:
            raise ValueError(f"device id {k} is outside [0, {devices})")
        flags[int(k)] = 1
    return flags


class PopulationRound(_RoundCounter):
    """A population of D device buckets resident in HBM, mixed in ONE launch per round."""

    _ended_rule = None  # (library constant, propagate) under set_ended_rule()

    def __init__(self, engine: Engine, models: torch.Tensor, out: Optional[torch.Tensor] = None):
        if models.dim() != 2 or models.dtype != torch.float32 or not models.is_cuda:
            raise ValueError("models must be a [D, P] fp32 CUDA tensor")
        self.engine = engine
        self.models = models
        self.out = torch.empty_like(models) if out is None else out
        D = models.shape[0]
        dev = models.device
        self.src = torch.tensor([models[d].data_ptr() for d in range(D)], dtype=torch.int64, device=dev)
        self.dst = torch.tensor([self.out[d].data_ptr() for d in range(D)], dtype=torch.int64, device=dev)
        self.tables = None
        self.window = None  # (hl, hr, per-device alphas) when the topology is a ring window
        self._graphs: Optional[RoundGraphs] = None  # captured rounds, rebuilt per topology
        self._parity = 0
        self._tf1 = False
        # rows 0 / 1: the ended flags, double-buffered as models / out; row 2: saw_ended
        self._flags = torch.zeros(3, D, dtype=torch.int32, device=dev)

    def set_ended_rule(self, rule: Optional[str], propagate: bool = False) -> None:
        """The TF2 protocol's ``training_end`` rule on the device, for the last rounds of a CFA
        run. A device flagged in ``ended`` has left its loop and keeps its model
        (federated_learning_keras_consensus_FL_threads_MNIST.py:501-546). Every other device
        collects its neighbours in list order, stops after the first flagged one
        (consensus_v3.py:139-141; consensus_v4.py:191-193, :234-236) and, by ``rule``,

        - "copy": takes that neighbour's model as it is, bit for bit (federated weights,
          consensus_v3.py:147-152, consensus_v4.py:205-210);
        - "truncate": mixes the collected prefix with the topology's coefficients (federated
          gradients of v4: the caller's eps, consensus_v4.py:248);
        - "truncate_eps": mixes it with eps = 1 / (prefix length + 1), and a device without a
          flagged neighbour its whole list with 1 / (n + 1), whatever the policy gave
          (federated gradients of v3, consensus_v3.py:233).

        With "copy" and "truncate" a device without a flagged neighbour mixes as with the rule
        off, bit for bit. ``saw_ended`` holds every device's
        ``getTrainingStatusFromNeightbor()`` of the last round. ``None`` (the default) turns the
        rule off: today's rounds on today's kernels. With a rule on a round is always one
        cfa_mix_population_ended_f32 launch on the CSR tables, never the window or ring round,
        under ``set_topology`` and ``set_schedule`` alike (the setting survives both), and
        ``run()``, ``rounds(R, graph=False)`` and the replay of ``rounds(R)`` need no host work
        between rounds. ``numerics="tf1"`` has no such rule: ValueError, here or there.

        ``propagate=False``: the flags change only through ``set_ended``. ``propagate=True``:
        ``ended`` after a round is ``ended | saw_ended``, every device of round r reading round
        r - 1's flags. That is the driver's chain of :423-425 (a device that saw training_end
        stops learning) and :501-509 (it then validates the model it copied and ends), taken for
        granted: a simulation convenience for a population whose devices copy an already solved
        model bit for bit, not something the reference's consensus modules do themselves. After
        ``run()`` and after ``rounds(R)`` for any R, ``ended`` holds the flags after the last
        round.

        Not covered: ``Tf1PopulationRound``, ``CfaGePopulation`` and the sharded populations."""
        code = ended_rule_code(rule)
        if code is not None and self._tf1:
            raise ValueError("the training_end rule belongs to the TF2 numerics, not numerics='tf1'")
        self._ended_rule = None if code is None else (code, bool(propagate))
        self._graphs = None  # captured rounds hold the kernels they were captured with

    @property
    def ended(self) -> torch.Tensor:
        """The current ``training_end`` flags: int32 [D] on the device, all zero at the start."""
        return self._flags[0]

    @property
    def saw_ended(self) -> torch.Tensor:
        """int32 [D]: 1 where the device collected a flagged neighbour in the last round with a
        rule on (its ``getTrainingStatusFromNeightbor()``)."""
        return self._flags[2]

    def set_ended(self, ids) -> None:
        """The devices that reported ``training_end`` (all others are cleared). Written in the
        order of the current stream: rounds already enqueued or replayed there see the old flags,
        later ones the new."""
        self._flags[0].copy_(torch.from_numpy(ended_flags(ids, self.models.shape[0])), non_blocking=False)

    def set_topology(self, lists, policy, use_window: Optional[bool] = None, numerics: str = "fp32",
                     compression: Optional[Tuple[int, int, int]] = None) -> None:
        """CSR tables for the one-launch population kernel. A ring-window topology with one
        coefficient per device (ring / wrap-around windows under every reference eps policy) can
        run as window passes instead (rows loaded once per 8 devices; same results), all in one
        cfa_mix_ring_round_f32 launch when rows are 16-byte aligned.
        ``use_window=None`` picks the window round only for buckets above WINDOW_MIN_P (512K
        elements); below that the CSR launch reuses rows from the Infinity Cache.
        ``numerics="tf1"``: the TF1 modules' arithmetic (fp32 first subtraction, fp64 chain with
        the fp64 coefficients, one rounding: cfa_mix_population_tf1_f32), for populations run
        with ``alphas_tf1_cfa`` / ``alphas_tf1_ongraphs``; "fp32": the TF2 rule.
        ``compression=(mode, cbegin, cend)`` (TF1 numerics only): the cfa_ongraphs epilogue on
        every device's [cbegin, cend) segment; ``kept`` then holds each device's counter_param
        after a round."""
        self._set_numerics(numerics, compression)
        self._sched = None
        if use_window is None:
            use_window = self.models.shape[1] > WINDOW_MIN_P
        if self._tf1:
            use_window = False
        D = self.models.shape[0]
        ptr, idx, coef = csr(lists, policy, D, np.float64 if self._tf1 else np.float32)
        dev = self.models.device
        self.tables = tuple(torch.from_numpy(a).to(dev) for a in (ptr, idx, coef))
        alphas = [list(policy(nb, d, D)) for d, nb in enumerate(lists)]
        shape = window_shape(lists, alphas) if use_window else None
        self.window = (shape[0], shape[1], alphas) if shape else None
        # one coefficient per device for the one-launch ring round (the window rule has one)
        self._ring_alphas = (torch.tensor([a[0] if a else 0.0 for a in alphas], dtype=torch.float32, device=dev)
                             if shape else None)
        self._graphs = None

    def _set_numerics(self, numerics: str, compression) -> None:
        if numerics not in ("fp32", "tf1"):
            raise ValueError("numerics must be 'fp32' or 'tf1'")
        if numerics == "tf1" and self._ended_rule is not None:
            raise ValueError("the training_end rule (set_ended_rule) belongs to the TF2 numerics, not numerics='tf1'")
        self._tf1 = numerics == "tf1"
        if compression is not None and not self._tf1:
            raise ValueError("the compression epilogue belongs to the TF1 (cfa_ongraphs) numerics")
        self._compress = tuple(int(v) for v in compression) if compression else (0, 0, 0)
        self.kept = torch.zeros(self.models.shape[0], dtype=torch.int64, device=self.models.device)

    def set_schedule(self, lists_per_table, policy, sched: Optional[Sequence[int]] = None, numerics: str = "fp32",
                     compression: Optional[Tuple[int, int, int]] = None) -> None:
        """A topology that changes from round to round (cfa_mobilenet.py:136-138: each epoch's
        graph; cfa_ongraphs.py:33-52: neighbours redrawn at every call): ``lists_per_table[t]``
        is table t's neighbour lists (``mobile(graph, t)``), and round r mixes with table
        ``sched[r % S]`` (``sched=None``: every table in turn, S = T). All tables and the round
        counter live on the device and the kernel looks its table up itself
        (cfa_mix_population_sched_f32 / _sched_tf1_f32), so ``run()``, ``rounds(R, graph=False)``
        and the graph replay of ``rounds(R)`` need no host work between rounds. Always the CSR
        kernel, never the window or ring round. ``numerics`` / ``compression`` as
        ``set_topology``; the counter starts at 0 (``reset_round``, ``round_index``).
        ``set_topology`` returns the population to one fixed table.
        Not covered: ``CfaGePopulation`` (its slot and gradient-pair tables depend on the topology
        too) and the sharded ``RingPopulationShard`` (ring windows only)."""
        tables, sched_t = _upload_schedule(lists_per_table, policy, sched, self.models.shape[0], self.models.device,
                                           coef_dtype=np.float64 if numerics == "tf1" else np.float32)
        self._set_numerics(numerics, compression)  # a refused schedule leaves the population as it was
        self.tables = tables
        self.window = self._ring_alphas = None
        self._new_schedule(sched_t)

    def run(self, stream=None) -> torch.Tensor:
        """One round: every device's mix of ``models`` into ``out``."""
        self._launch(self.models, self.out, self.src, self.dst, stream)
        if self._propagates():
            self._keep_flags(stream)
        return self.out

    def _propagates(self) -> bool:
        return self._ended_rule is not None and self._ended_rule[1]

    def _keep_flags(self, stream=None) -> None:
        """The flags a round from ``models`` left in the other buffer become ``ended``."""
        with torch.cuda.stream(stream or torch.cuda.current_stream(self.models.device)):
            self._flags[0].copy_(self._flags[1])

    def _launch(self, models, out, src, dst, stream=None) -> None:
        if self.tables is None:
            raise RuntimeError("set_topology() or set_schedule() first")
        D, P = models.shape
        if self._ended_rule is not None:
            code, propagate = self._ended_rule
            # propagated flags rotate with models / out; otherwise only set_ended writes them
            cur = 0 if models is self.models or not propagate else 1
            self.engine.population_ended(dst, src, *self.tables, self._flags[cur],
                                         self._flags[cur ^ 1] if propagate else None, self._flags[2], code, D, P,
                                         *(self._sched or (None, None)), stream)
            return
        if self._tf1:  # never a window round (set_topology)
            _mix_tf1(self.engine, dst, src, self.tables, self._sched, self._compress, self.kept, D, P, stream)
            return
        if self._sched is not None:
            self.engine.population_sched(dst, src, *self.tables, *self._sched, D, RULE_SEQUENTIAL, P, stream)
            return
        if self.window is not None:
            hl, hr, alphas = self.window
            if P % 4 == 0:  # 16-byte rows: every pass in one cfa_mix_ring_round_f32 launch
                self.engine.ring_round(out, models, self._ring_alphas, hl, hr, stream)
                return
            for s in range(0, D, 8):
                devs = list(range(s, min(s + 8, D)))
                rows = [models[(s + o) % D] for o in range(-hl, len(devs) + hr)]
                self.engine.mix_window([out[d] for d in devs], rows, [alphas[d] for d in devs], hl, hr, stream)
            return
        self.engine.population(dst, src, *self.tables, D, RULE_SEQUENTIAL, P, stream)

    def rounds(self, R: int, graph: bool = True) -> torch.Tensor:
        """R consecutive rounds on the current stream, each mixing the previous round's output
        (the per-device reference run, repeated: every device's round r reads its neighbours'
        round r-1 models). ``models`` and ``out`` alternate as source and destination; the
        result is left in ``models`` (one extra copy when R is odd) and returned.
        ``graph=True`` replays captured pairs of rounds (hipGraph) instead of launching each
        round from Python; the results are the same bit for bit."""
        if R <= 0:
            return self.models
        if not graph:
            for r in range(R):
                self._step_pair(r & 1)
        else:
            if self._graphs is None:
                self._graphs = RoundGraphs(self.models.device, self._graph_step, 2, lambda: self._parity)
            self._parity = 0
            self._graphs.run(R)
        if R & 1:
            self.models.copy_(self.out)
            if self._propagates():
                self._keep_flags()
        return self.models

    def _step_pair(self, parity: int) -> None:
        if parity == 0:
            self._launch(self.models, self.out, self.src, self.dst)
        else:
            self._launch(self.out, self.models, self.dst, self.src)

    def _graph_step(self) -> None:
        self._step_pair(self._parity)
        self._parity ^= 1


class Tf1PopulationRound(_RoundCounter, LocalTrainingHooks):
    """A device-resident population on the TF1 protocol (cfa.py:105-154, cfa_ongraphs.py): at
    epoch e every device mixes its own epoch-e model with the models its neighbours PUBLISHED at
    epoch e-1 (their pre-mix inputs of e-1, cfa.py:131-139), with the TF1 numerics (fp64 chain,
    one rounding to fp32: what the driver's fp32 TF variables hold after the assignment).

    Three [D, P] buffers rotate through (current, previous, out): a round mixes current with
    previous into out, then (current, previous, out) <- (out, current, previous). One
    ``cfa_mix_population_tf1_f32`` launch per round over the source table [current | previous]."""

    def __init__(self, engine: Engine, D: int, P: int, device=None, placement_candidates: int = 0):
        """``placement_candidates`` > 3: the three stacks are placement-calibrated
        (``placement.calibrated_rotation``: each stack is in turn read and written, so every
        candidate is scored in both roles) when a stack is 1 GiB or more; ``self.placement``
        holds the probe."""
        dev = engine.device if device is None else torch.device(device)
        self.engine, self.D, self.P = engine, int(D), int(P)
        self.placement = None
        if placement_candidates > 3 and dev.type == "cuda" and self.D * self.P * 4 >= (1 << 30):
            from .placement import calibrated_rotation
            self._bufs, self.placement = calibrated_rotation(3, self.D, self.P, dev, engine, placement_candidates)
            for b in self._bufs:
                b.zero_()
        else:
            self._bufs = [torch.zeros(self.D, self.P, device=dev) for _ in range(3)]
        self._rot = 0
        self._tables = []
        for r in range(3):
            cur, prev, out = (self._bufs[(r + k) % 3] for k in range(3))
            src = torch.tensor([cur[d].data_ptr() for d in range(self.D)] + [prev[d].data_ptr() for d in range(self.D)],
                               dtype=torch.int64, device=dev)
            dst = torch.tensor([out[d].data_ptr() for d in range(self.D)], dtype=torch.int64, device=dev)
            self._tables.append((src, dst))
        self._csr = None
        self._graphs: Optional[RoundGraphs] = None
        self._compress = (0, 0, 0)
        self.kept = torch.zeros(self.D, dtype=torch.int64, device=dev)

    @property
    def current(self) -> torch.Tensor:
        return self._bufs[self._rot]

    @property
    def previous(self) -> torch.Tensor:
        return self._bufs[(self._rot + 1) % 3]

    # the source table is [current | previous]: the local entry is row d, neighbour j's published
    # model row D + j (neighbor_base=D); fp64 coefficients, the local entry's unused
    _LAYOUT = dict(coef_dtype=np.float64, self_coef=0.0)

    def set_topology(self, lists, policy, compression: Optional[Tuple[int, int, int]] = None) -> None:
        """Neighbour lists and an eps policy (``alphas_tf1_cfa`` / ``alphas_tf1_ongraphs``); the
        fp64 coefficients go to the device as they are. ``compression=(mode, cbegin, cend)``:
        the cfa_ongraphs epilogue on every device's [cbegin, cend) (its W2 segment); ``kept``
        holds each device's counter_param after a round."""
        self._compress = tuple(int(v) for v in compression) if compression else (0, 0, 0)
        dev = self._bufs[0].device
        self._csr = tuple(torch.from_numpy(a).to(dev)
                          for a in schedule_csr([lists], policy, self.D, neighbor_base=self.D, **self._LAYOUT))
        self._sched = None
        self._graphs = None  # captured rounds hold the tables they were captured with
        self._epoch_graphs = None

    def set_schedule(self, lists_per_table, policy, sched: Optional[Sequence[int]] = None,
                     compression: Optional[Tuple[int, int, int]] = None) -> None:
        """A topology that changes from round to round: ``lists_per_table[t]`` is table t's
        neighbour lists (``mobile(graph, t)`` for cfa_mobilenet.py:136-138) and round r mixes
        with table ``sched[r % S]`` (``sched=None``: every table in turn). Tables and round
        counter live on the device (cfa_mix_population_sched_tf1_f32), so ``round()`` and
        ``rounds()``, eager or replayed from graphs, need no host work between rounds; the
        counter starts at 0 (``reset_round``, ``round_index``). ``set_topology`` returns the
        population to one fixed table. Not covered: ``CfaGePopulation`` and the sharded
        ``RingPopulationShard`` (see ``PopulationRound.set_schedule``)."""
        self._csr, sched_t = _upload_schedule(lists_per_table, policy, sched, self.D, self._bufs[0].device,
                                              neighbor_base=self.D, **self._LAYOUT)
        self._compress = tuple(int(v) for v in compression) if compression else (0, 0, 0)
        self._new_schedule(sched_t)

    def load(self, current: torch.Tensor, previous: torch.Tensor) -> None:
        """current [D, P]: every device's epoch-e model; previous [D, P]: the models published at
        epoch e-1."""
        self.current.copy_(current)
        self.previous.copy_(previous)

    def round(self, stream=None) -> None:
        if self._csr is None:
            raise RuntimeError("set_topology() or set_schedule() first")
        src, dst = self._tables[self._rot]
        _mix_tf1(self.engine, dst, src, self._csr, self._sched, self._compress, self.kept, self.D, self.P, stream)
        self._rot = (self._rot + 2) % 3  # (current, previous, out) <- (out, current, previous)

    # local training between rounds (``set_local_training``, ``epoch``, ``epochs``): the devices train
    # on ``current``; an epoch advances the same rotation as a round
    def _training_stack(self) -> torch.Tensor:
        return self.current

    def _epoch_period(self):
        return 3, lambda: self._rot

    def rounds(self, R: int, graph: bool = True) -> None:
        """R rounds; ``graph=True`` replays captured 3-round periods (hipGraph), same results."""
        if not graph:
            for _ in range(R):
                self.round()
            return
        if self._graphs is None:
            self._graphs = RoundGraphs(self._bufs[0].device, self.round, 3, lambda: self._rot)
        self._graphs.run(R)
