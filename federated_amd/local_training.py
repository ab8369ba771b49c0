"""Local training of a device-resident TF1 population between two consensus rounds.

The reference's TF1 drivers run, on every device and before every call of the consensus class,
one local epoch of plain minibatch SGD on the device's own samples and then measure the
validation cost (``federated_sample_CNN_CFA-GE.py:137-173``; the assignment
``W <- W_ext - learning_rate * grad`` is ``:114-118``; ``federated_sample_2NN_CFA.py:97-101``
is the same loop around the 2NN graph). ``LocalSgd`` holds what that loop needs (every
device's samples, the minibatch slicing, the learning rate and the cost buffers) and runs the
epoch of the whole population as ONE ``cfa_local_sgd_{cnn,2nn}_f32`` launch (plus one for the
validation pass): each device's model stays in LDS for all its minibatches.

Chained to a population (``CfaGePopulation.set_local_training``,
``Tf1PopulationRound.set_local_training``) an epoch "train, validate, consensus round" is a
graph-replayable unit: ``epochs(R)`` replays whole periods as hipGraphs and leaves the cost
curves in ``train_log`` / ``val_log`` on the device.

The drivers' slice ``i*batch_size : (i+1)*batch_size - 1`` with batch_size 5 takes FOUR rows
at a stride of five; that is the default slicing here (``batch_stride=5, batch_rows=4``), and
``steps`` defaults to their ``total_batch = int(samples / batch_size)``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

__all__ = ["LocalSgd", "model_size"]


def model_size(ml_model: int, geom: dict, L: int, classes: int) -> int:
    """Parameters of a TF1 model bucket (W1, b1, W2, b2): ``geom`` holds filter / number / stride
    (CNN, ml_model 1) or intermediate_nodes (2NN, ml_model 2)."""
    if ml_model == 1:
        F, NC, S = int(geom["filter"]), int(geom["number"]), int(geom["stride"])
        if F < 1 or NC < 1 or S < 1:
            raise ValueError("filter, number and stride must be >= 1")
        L2 = -(-(-(-L // S)) // S)
        return F * NC + NC + L2 * NC * classes + classes
    if ml_model == 2:
        H = int(geom["intermediate_nodes"])
        if H < 1:
            raise ValueError("intermediate_nodes must be >= 1")
        return L * H + H + H * classes + classes
    raise ValueError("ml_model must be 1 (CNN) or 2 (2NN)")


class LocalSgd:
    """One local SGD epoch (and its validation pass) for D devices, on the GPU."""

    @staticmethod
    def check(ml_model: int, geom: dict, x_shape: Sequence[int], y_shape: Sequence[int], batch_stride: int = 5,
              batch_rows: int = 4, steps: Optional[int] = None, x_test_shape: Optional[Sequence[int]] = None,
              y_test_shape: Optional[Sequence[int]] = None, test_steps: Optional[int] = None) -> dict:
        """The host half: validates shapes and slicing without touching a device and returns
        D, Ns, L, classes, P, steps (and Nt, test_steps with a test set). ``steps=None`` is
        the drivers' ``int(samples / batch_size)`` with batch_size = ``batch_stride``. Raises
        ValueError for mismatched shapes, a slicing that runs past the samples and an unknown
        ``ml_model``."""
        if ml_model not in (1, 2):
            raise ValueError("ml_model must be 1 (CNN) or 2 (2NN)")
        if len(x_shape) != 3 or len(y_shape) != 3:
            raise ValueError("x must be [D, Ns, L] and y [D, Ns, classes]")
        D, Ns, L = (int(v) for v in x_shape)
        Dy, Nsy, C = (int(v) for v in y_shape)
        if (Dy, Nsy) != (D, Ns) or min(D, Ns, L, C) < 1:
            raise ValueError("x [D, Ns, L] and y [D, Ns, classes] must agree on D and Ns, all >= 1")
        batch_stride, batch_rows = int(batch_stride), int(batch_rows)
        if batch_stride < 1 or batch_rows < 1:
            raise ValueError("batch_stride and batch_rows must be >= 1")

        def fit(n, what, rows):
            n = rows // batch_stride if n is None else int(n)
            if n < 1 or (n - 1) * batch_stride + batch_rows > rows:
                raise ValueError(f"{what} = {n} minibatches of {batch_rows} rows at a stride of {batch_stride} "
                                 f"do not fit {rows} samples")
            return n

        info = {"D": D, "Ns": Ns, "L": L, "classes": C, "P": model_size(ml_model, geom, L, C),
                "steps": fit(steps, "steps", Ns)}
        if (x_test_shape is None) != (y_test_shape is None):
            raise ValueError("x_test and y_test are given together or not at all")
        if x_test_shape is not None:
            if len(x_test_shape) != 3 or len(y_test_shape) != 3:
                raise ValueError("x_test must be [D, Nt, L] and y_test [D, Nt, classes]")
            Dt, Nt, Lt = (int(v) for v in x_test_shape)
            if (Dt, Lt) != (D, L) or tuple(int(v) for v in y_test_shape) != (D, Nt, C) or Nt < 1:
                raise ValueError("the test set must be [D, Nt, L] / [D, Nt, classes] like the training set")
            info["Nt"], info["test_steps"] = Nt, fit(test_steps, "test_steps", Nt)
        return info

    def __init__(self, engine, ml_model: int, geom: dict, x: torch.Tensor, y: torch.Tensor, lr: float,
                 x_test: Optional[torch.Tensor] = None, y_test: Optional[torch.Tensor] = None,
                 batch_stride: int = 5, batch_rows: int = 4, steps: Optional[int] = None,
                 test_steps: Optional[int] = None, log_cap: int = 0):
        """``x`` [D, Ns, L] / ``y`` [D, Ns, classes]: every device's training samples and one-hot
        labels (fp32 CUDA); ``x_test`` / ``y_test`` [D, Nt, .]: every device's validation set, or
        None. ``log_cap`` > 0 keeps a [log_cap, D] log of each cost on the device: epoch e goes to
        row min(e, log_cap - 1)."""
        info = self.check(ml_model, geom, x.shape, y.shape, batch_stride, batch_rows, steps,
                          None if x_test is None else x_test.shape, None if y_test is None else y_test.shape,
                          test_steps)
        self.engine, self.ml_model, self.geom = engine, int(ml_model), dict(geom)
        self.x, self.y, self.x_test, self.y_test = x, y, x_test, y_test
        self.D, self.P, self.steps = info["D"], info["P"], info["steps"]
        self.test_steps = info.get("test_steps")
        self.batch_stride, self.batch_rows, self.lr = int(batch_stride), int(batch_rows), float(lr)
        dev = engine.device
        self.train_cost = torch.zeros(self.D, dtype=torch.float64, device=dev)
        self.val_cost = torch.zeros(self.D, dtype=torch.float64, device=dev) if x_test is not None else None
        cap = int(log_cap)
        self.train_log = torch.zeros(cap, self.D, dtype=torch.float64, device=dev) if cap > 0 else None
        self.val_log = (torch.zeros(cap, self.D, dtype=torch.float64, device=dev)
                        if cap > 0 and x_test is not None else None)
        # one counter per log: each logged launch leaves its own one higher
        self.epoch_counter = torch.zeros(2, dtype=torch.int64, device=dev)

    @property
    def epochs_done(self) -> int:
        """Epochs logged so far (reads the device counter back: synchronises)."""
        return int(self.epoch_counter[0].item())

    def train(self, models: torch.Tensor, stream=None) -> None:
        """The training pass: ``models`` [D, P] stepped in place, ``train_cost`` written."""
        logged = self.train_log is not None
        self.engine.local_sgd(self.ml_model, self.x, self.y, models, self.geom, self.batch_stride, self.batch_rows,
                              self.steps, self.lr, True, self.train_cost, self.train_log,
                              self.epoch_counter[0:1] if logged else None, stream)

    def validate(self, models: torch.Tensor, stream=None) -> None:
        """The validation pass on the test set: ``val_cost`` written, ``models`` untouched."""
        if self.x_test is None:
            raise RuntimeError("no test set was given")
        logged = self.val_log is not None
        self.engine.local_sgd(self.ml_model, self.x_test, self.y_test, models, self.geom, self.batch_stride,
                              self.batch_rows, self.test_steps, self.lr, False, self.val_cost, self.val_log,
                              self.epoch_counter[1:2] if logged else None, stream)

    def epoch(self, models: torch.Tensor, stream=None) -> None:
        """One local epoch of every device (eager): train, then validate if a test set was given."""
        self.train(models, stream)
        if self.x_test is not None:
            self.validate(models, stream)


class LocalTrainingHooks:
    """``set_local_training`` / ``epoch`` / ``epochs`` of a population class that has ``round()``,
    a rotation period and phase for ``RoundGraphs``, and names the stack its devices train on."""

    _local: Optional[LocalSgd] = None
    _epoch_graphs = None

    def _training_stack(self) -> torch.Tensor:
        raise NotImplementedError

    def _epoch_period(self):
        """(period, phase callable) of the population's buffer rotation."""
        raise NotImplementedError

    def set_local_training(self, local_sgd: Optional[LocalSgd]) -> None:
        """The local training that ``epoch()`` runs before each round (None: none)."""
        if local_sgd is not None:
            stack = self._training_stack()
            if (local_sgd.D, local_sgd.P) != tuple(stack.shape):
                raise ValueError(f"local training of {local_sgd.D} devices with {local_sgd.P} parameters does not "
                                 f"match the population's {tuple(stack.shape)}")
        self._local = local_sgd
        self._epoch_graphs = None

    def epoch(self, stream=None) -> None:
        """One simulated epoch in the reference's order: every device's local epoch (and its
        validation pass), then the consensus round."""
        if self._local is None:
            raise RuntimeError("set_local_training() first")
        self._local.epoch(self._training_stack(), stream)
        self.round(stream)

    def epochs(self, R: int, graph: bool = True) -> None:
        """R consecutive ``epoch()`` calls on the current stream; ``graph=True`` replays captured
        periods of the buffer rotation as hipGraphs, with the results of R eager epochs bit for
        bit (the cost logs included: their rows are chosen by a counter on the device)."""
        if self._local is None:
            raise RuntimeError("set_local_training() first")
        if not graph:
            for _ in range(R):
                self.epoch()
            return
        if self._epoch_graphs is None:
            from ._graphs import RoundGraphs
            period, phase = self._epoch_period()
            self._epoch_graphs = RoundGraphs(self._training_stack().device, self.epoch, period, phase)
        self._epoch_graphs.run(R)
