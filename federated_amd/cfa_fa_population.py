"""The TF1 CFA-FA driver's server federation on a device-resident population.

``federated_sample_CNN_CFA_FA.py`` alternates blocks of server-federation epochs with blocks of
consensus epochs. In a server epoch every device publishes the model it trained (``cfa.py:146-153``
with consensus disabled), the server process folds the D published models, in device order, into
its fp64 model (``:86-89`` at epoch 0, ``:103-110`` / ``:130-133`` later) and, from epoch 1 on,
every device pulls its model toward the folded one (``:280-283``). A consensus epoch is the plain
``cfa.py`` round. ``CfaFaPopulation`` runs a server epoch as ONE launch
(``cfa_fa_population_round_f32``) on the ``Tf1PopulationRound`` stacks and a consensus epoch as the
inherited CSR round; both advance the same three-buffer rotation, so a whole run (local training
included, ``set_local_training``) replays from hipGraphs with no host work between epochs.

``cfa_fa_cycle`` derives which epochs are server epochs from the driver's own flag logic.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._graphs import RoundGraphs
from .engine import Engine
from .topology import Tf1PopulationRound

__all__ = ["cfa_fa_cycle", "CfaFaPopulation", "PHASES"]

PHASES = ("server", "consensus")


def cfa_fa_cycle(consensus_epochs: int, server_duration: int, server_epochs: int = 1) -> List[str]:
    """One period of the driver's phases, ``"server"`` / ``"consensus"`` per epoch from epoch 0,
    for ``-Con consensus_epochs -Ser server_duration -S server_epochs``: the client's flags
    (``federated_sample_CNN_CFA_FA.py:264-292``) simulated against the epochs at which the server
    loop (``:70-137``) writes its model. ValueError, naming the epoch, when a client would wait
    (``:270``) for a server file that is never written: the driver deadlocks there (every
    ``server_epochs`` > 1 with a server block of more than one epoch, and ``server_duration`` < 2,
    whose counter test ``:285`` sits under ``epoch > 0`` and never fires)."""
    con, ser, S = int(consensus_epochs), int(server_duration), int(server_epochs)
    if con < 0 or ser < 1 or S < 1:
        raise ValueError("need consensus_epochs >= 0, server_duration >= 1 and server_epochs >= 1")
    period = con + ser
    T = 3 * period + 1  # training_epochs: three periods show the cycle and that it repeats
    written = set()  # epochs with a server_datamat file (:91, :118)
    for start in range(0, T, period):
        written.update(range(start + 1 if start == 0 else start, ser + start, S))
    phases, federation, counter = [], False, 0
    for epoch in range(T):
        if epoch % period == 0 or federation:  # :264
            federation = True
            counter += 1
            phases.append("server")
            if epoch > 0:
                if epoch not in written:
                    raise ValueError(f"-Con {con} -Ser {ser} -S {S} deadlocks the driver: at epoch {epoch} the "
                                     f"devices wait for a server model that the server never writes")
                if counter == ser:  # :285
                    federation, counter = False, 0
        else:
            counter = 0
            phases.append("consensus")
    cycle = phases[:period]
    if any(phases[k * period:(k + 1) * period] != cycle for k in (1, 2)):
        raise ValueError(f"-Con {con} -Ser {ser} -S {S}: the driver's phases do not repeat with period {period}")
    return cycle


class CfaFaPopulation(Tf1PopulationRound):
    """A ``Tf1PopulationRound`` whose epochs follow a cycle of server and consensus phases.

    ``server`` [P] fp64 is the server process's model (zeros at construction, ``:73-76``);
    ``epoch_index`` the epoch the next ``round()`` runs. A server epoch folds ``current`` (the
    models the devices just trained, which it also publishes: they become ``previous``) into
    ``server`` and writes the devices' next models; epoch 0 is the driver's initialisation
    (``s <- s + b_d * x_d``, the devices keep their models)."""

    def __init__(self, engine: Engine, D: int, P: int, eps: float, eps2: float,
                 balancing: Optional[Sequence[float]] = None, device=None, placement_candidates: int = 0):
        """``eps`` / ``eps2``: the driver's ``-eps`` (server fold) and ``-eps2`` (client pull);
        ``balancing`` [D]: its ``balancing_vect`` (``None``: ``1 / D`` each, ``:67-68``)."""
        bal = self.check(D, balancing, eps, eps2)
        super().__init__(engine, D, P, device, placement_candidates)
        dev = self._bufs[0].device
        self.eps, self.eps2, self.balancing = float(eps), float(eps2), bal
        self.server = torch.zeros(self.P, dtype=torch.float64, device=dev)
        # b_d (:86-89) and the one fp64 product eps * b_d (:103) per device, formed as the driver does
        rnd = np.asarray([self.eps * bal[d] for d in range(self.D)], dtype=np.float64)
        self._coef = {_lib.FA_INIT: torch.from_numpy(bal.copy()).to(dev), _lib.FA_ROUND: torch.from_numpy(rnd).to(dev)}
        self._cycle: Optional[List[str]] = None
        self._epoch = 0

    @staticmethod
    def check(D: int, balancing=None, eps: float = 1.0, eps2: float = 0.5, cycle=None) -> np.ndarray:
        """The host half (no device is touched): the arguments checked, ``balancing`` returned as
        the fp64 [D] vector the fold uses. ValueError for D < 1, a ``balancing`` that does not hold
        one finite value per device, ``eps`` / ``eps2`` that are not finite, and (when given) a
        ``cycle`` that is empty, names an unknown phase or does not start with a server epoch."""
        D = int(D)
        if D < 1:
            raise ValueError("a population needs at least one device")
        bal = np.ones(D) * (1 / D) if balancing is None else np.asarray(balancing, dtype=np.float64)
        if bal.shape != (D,) or not np.all(np.isfinite(bal)):
            raise ValueError(f"balancing must hold one finite value for each of the {D} devices")
        if not (math.isfinite(float(eps)) and math.isfinite(float(eps2))):
            raise ValueError("eps and eps2 must be finite")
        if cycle is not None:
            cycle = list(cycle)
            if not cycle:
                raise ValueError("a cycle needs at least one epoch")
            if any(p not in PHASES for p in cycle):
                raise ValueError('a cycle holds "server" and "consensus" phases only')
            if cycle[0] != "server":
                raise ValueError('cycle[0] must be "server": the driver starts with its server initialisation')
        return bal

    def set_cycle(self, cycle: Sequence[str]) -> None:
        """The phases of one period (``cfa_fa_cycle``): epoch e runs ``cycle[e % len(cycle)]``. A
        refused cycle leaves the population as it was."""
        self.check(self.D, self.balancing, self.eps, self.eps2, cycle)
        self._cycle = list(cycle)
        self._graphs = None
        self._epoch_graphs = None

    @property
    def epoch_index(self) -> int:
        """The epoch the next ``round()`` runs."""
        return self._epoch

    def reset_epoch(self, e: int = 0) -> None:
        """The next ``round()`` runs epoch ``e`` (epoch 0 is the server initialisation). The
        buffers and ``server`` stay as they are (``load``)."""
        if int(e) < 0:
            raise ValueError("the epoch index must be >= 0")
        self._epoch = int(e)

    def load(self, current: torch.Tensor, previous: torch.Tensor, server: Optional[torch.Tensor] = None) -> None:
        """``current`` / ``previous`` as ``Tf1PopulationRound.load``; ``server`` [P] (fp64): the
        server model (None: left as it is)."""
        super().load(current, previous)
        if server is not None:
            self.server.copy_(server)

    def phase(self, e: Optional[int] = None) -> str:
        """The phase of epoch ``e`` (None: the next one)."""
        if self._cycle is None:
            raise RuntimeError("set_cycle() first")
        return self._cycle[(self._epoch if e is None else int(e)) % len(self._cycle)]

    def round(self, stream=None) -> None:
        """Epoch ``epoch_index``'s phase on ``stream`` (None: the current stream): a server epoch
        is one ``cfa_fa_population_round_f32`` launch from ``current`` into the spare stack, a
        consensus epoch the inherited round. Both rotate (current, previous, out) <- (out,
        current, previous) and advance ``epoch_index``."""
        if self.phase() == "server":
            mode = _lib.FA_INIT if self._epoch == 0 else _lib.FA_ROUND
            self.engine.cfa_fa_round(self._bufs[(self._rot + 2) % 3], self._bufs[self._rot], self.server,
                                     self._coef[mode], self.eps2, mode, stream)
            self._rot = (self._rot + 2) % 3
        else:
            super().round(stream)
        self._epoch += 1

    # Graph replay: the unit is one cycle of epochs captured from a given rotation; after it the
    # cycle position is the same and the rotation has moved by 2 * len(cycle) mod 3, so there are
    # at most three graphs per starting position, and rotation and cycle together return after
    # lcm(3, len(cycle)) epochs. A replay advances only the device state: the host's rotation and
    # epoch index are set after it. Epoch 0 (the one epoch in init mode) always runs outside the
    # graphs, so every captured server epoch is a CFA_FA_ROUND launch.
    def _epoch_period(self):
        n = len(self._cycle)
        return math.lcm(3, n), lambda: (self._rot, self._epoch % n)

    def _replay(self, graphs_attr: str, step, R: int) -> None:
        if R < 0:
            raise ValueError("R must be >= 0")
        self.phase()
        if "consensus" in self._cycle and self._csr is None:
            raise RuntimeError("set_topology() or set_schedule() first: the cycle has consensus epochs")
        n, L = int(R), len(self._cycle)
        if n and self._epoch == 0:
            step()
            n -= 1
        by_rot = getattr(self, graphs_attr)
        if by_rot is None:
            by_rot = {}
            setattr(self, graphs_attr, by_rot)
        while n >= L:
            rot, e = self._rot, self._epoch
            if rot not in by_rot:
                by_rot[rot] = RoundGraphs(self._bufs[0].device, step, L, lambda: self._epoch % L)
            by_rot[rot].run(L)  # one replay; a first use also captures, which steps the host state
            self._rot, self._epoch = (rot + 2 * L) % 3, e + L
            n -= L
        for _ in range(n):
            step()

    def rounds(self, R: int, graph: bool = True) -> None:
        """R epochs' rounds from ``epoch_index`` on; ``graph=True`` replays captured periods
        (hipGraph) with the results of R ``round()`` calls bit for bit."""
        if not graph:
            for _ in range(R):
                self.round()
            return
        self._replay("_graphs", self.round, R)

    def epochs(self, R: int, graph: bool = True) -> None:
        """R ``epoch()`` calls (local training, validation, then the epoch's phase); ``graph=True``
        replays captured periods, cost logs included, bit for bit."""
        if self._local is None:
            raise RuntimeError("set_local_training() first")
        if not graph:
            for _ in range(R):
                self.epoch()
            return
        self._replay("_epoch_graphs", self.epoch, R)

    def bytes_per_round(self) -> int:
        """Algorithmic bytes of the next epoch's phase. Server: D rows read, D written, the fp64
        server model read and written, ``2 * D * P * 4 + 16 * P``. Consensus: every CSR entry's
        row read and one row written per device (under a schedule the round counter is read
        back: synchronises)."""
        if self.phase() == "server":
            return 2 * self.D * self.P * 4 + 16 * self.P
        if self._csr is None:
            raise RuntimeError("set_topology() or set_schedule() first")
        ptr = self._csr[0].cpu().numpy().reshape(-1, self.D + 1)
        t = 0 if self._sched is None else int(self._sched[0][self.round_index % self._sched[0].numel()].item())
        return (int(ptr[t, -1] - ptr[t, 0]) + self.D) * self.P * 4
