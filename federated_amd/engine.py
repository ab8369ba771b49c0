"""Device-level consensus engine: the libcfa kernels on PyTorch-ROCm tensors.

PyTorch provides device memory and streams only; all arithmetic runs in the HIP kernels of
``libcfa.so`` (``federated_amd/csrc/cfa_*.hip``). Every call is asynchronous on the
given stream (default: torch's current stream on the tensor's device).

A *bucket* is a 1-D contiguous fp32 CUDA tensor holding one model (or gradient) flattened
layer by layer in the order the reference passes its tensors; ``BucketLayout`` maps the
reference's per-layer arrays to and from that flat form.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["Engine", "BucketLayout", "get_engine"]


def _require_gpu(device: Optional[torch.device]) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("federated_amd: no ROCm GPU visible; the consensus engine runs only on "
                           "MI355X (gfx950) through libcfa.so and has no CPU fallback")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"engine device must be a cuda device, got {device}")
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _check_bucket(t: torch.Tensor, name: str, P: Optional[int] = None, dtype=torch.float32) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device})")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    n = t.numel()
    if P is not None and n != P:
        raise ValueError(f"{name} has {n} elements, expected {P}")
    return n


def _check_fanin(out: torch.Tensor, local: torch.Tensor, nbrs, dtype=torch.float32) -> int:
    """The buckets of one fold: ``local``, ``out`` and every neighbour, all of local's P elements."""
    P = _check_bucket(local, "local", dtype=dtype)
    _check_bucket(out, "out", P, dtype)
    for j, x in enumerate(nbrs):
        _check_bucket(x, f"nbrs[{j}]", P, dtype)
    return P


_FP = {torch.float32: "fp32", torch.float64: "fp64"}


def _check_mewma(W: torch.Tensor, s, g, dtype) -> tuple:
    """The buckets of a MEWMA update: ``W`` and one state bucket per gradient, which may be an
    element-strided 1-D view. Returns (P, the gradients' element strides)."""
    P = _check_bucket(W, "W", dtype=dtype)
    if len(s) != len(g):
        raise ValueError("one state bucket per gradient bucket")
    strides = []
    for j in range(len(g)):
        _check_bucket(s[j], f"s[{j}]", P, dtype)
        gj = g[j]
        if not gj.is_cuda or gj.dtype != dtype or gj.dim() != 1 or gj.numel() != P:
            raise ValueError(f"g[{j}] must be a 1-D {_FP[dtype]} CUDA view of {P} elements")
        strides.append(int(gj.stride(0)))
    return P, strides


def _check_tables(*tables) -> None:
    """Device tables, each given as (name, tensor, dtype)."""
    for name, t, dt in tables:
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {dt} CUDA tensor")


def _foreign(objs, index: int):
    """The first CUDA tensor or stream in ``objs`` (tensors, streams, and lists / tuples of them)
    that is not on GPU ``index``, else None."""
    for a in objs:
        for t in (a if isinstance(a, (list, tuple)) else (a,)):
            if isinstance(t, torch.Tensor):
                if t.is_cuda and t.device.index != index:
                    return t.device
            elif isinstance(t, torch.cuda.Stream) and t.device.index != index:
                return t.device
    return None


def _same_device(fn):
    """Engine method guard: every CUDA tensor and stream argument must be on the engine's GPU. A
    kernel enqueued on this GPU's stream with another GPU's pointers would fault (no peer mapping)
    or, with one, silently run over xGMI; both are caller errors, refused before any launch."""
    @functools.wraps(fn)
    def checked(self, *args, **kwargs):
        dev = _foreign(list(args) + list(kwargs.values()), self.device.index)
        if dev is not None:
            raise ValueError(f"{fn.__name__}: argument on {dev}, but this engine runs on {self.device}")
        return fn(self, *args, **kwargs)
    return checked


def _check_nd(t: torch.Tensor, name: str, nd: int = 2, what: Optional[str] = None, pitched: bool = False) -> tuple:
    """Shape of an fp32 CUDA tensor of ``nd`` dimensions that is contiguous (named ``what`` in
    the error, by default "nd-D") or, ``pitched``, has unit element stride and any row pitch."""
    ok = isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == nd
    if pitched:
        if not ok or (t.shape[1] > 1 and t.stride(1) != 1):
            raise TypeError(f"{name} must be a {nd}-D fp32 CUDA tensor with unit element stride")
    elif not ok or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous {what or f'{nd}-D'} fp32 CUDA tensor")
    return tuple(int(d) for d in t.shape)


def _check_2d(t: torch.Tensor, name: str):
    return _check_nd(t, name)


TF1_STATE_F32, TF1_GRAD_F32, TF1_W_F32 = 1, 2, 4  # cfa_mewma_tf1_f64 dtype mask


class BucketLayout:
    """Offsets of a list of tensors flattened into one bucket (layer order preserved)."""

    def __init__(self, shapes: Iterable[Sequence[int]]):
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.sizes = [int(np.prod(s)) if len(s) else 1 for s in self.shapes]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.P = int(self.offsets[-1])

    @classmethod
    def of(cls, arrays) -> "BucketLayout":
        return cls([np.shape(a) for a in arrays])

    def segment(self, k: int) -> tuple:
        return int(self.offsets[k]), int(self.offsets[k + 1])

    def pack(self, arrays, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Flatten per-layer arrays into ``out`` (length P; fp32 unless ``out`` says otherwise),
        converting dtype if needed."""
        if out is None:
            out = np.empty(self.P, dtype=np.float32)
        if len(arrays) != len(self.sizes):
            raise ValueError(f"expected {len(self.sizes)} tensors, got {len(arrays)}")
        for k, a in enumerate(arrays):
            a = np.asarray(a)
            if a.size != self.sizes[k]:
                raise ValueError(f"tensor {k} has {a.size} elements, layout expects {self.sizes[k]}")
            b, e = self.segment(k)
            out[b:e] = a.reshape(-1)
        return out

    def unpack(self, flat: np.ndarray, copy: bool = True) -> list:
        res = []
        for k, shp in enumerate(self.shapes):
            b, e = self.segment(k)
            v = flat[b:e].reshape(shp)
            res.append(v.copy() if copy else v)
        return res


class Engine:
    """libcfa kernels bound to one GPU."""

    def __init__(self, device=None):
        self.device = _require_gpu(device)
        self.lib = _lib.load()
        # device attributes cached and kernel LDS limits raised now, so no launch queries the
        # device (hipGraph captures of engine launches run in the strict mode)
        _lib.call("cfa_device_prepare", int(self.device.index))

    # -- helpers ---------------------------------------------------------------------------
    def stream_handle(self, stream: Optional[torch.cuda.Stream] = None) -> int:
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return int(s.cuda_stream)

    def empty(self, P: int) -> torch.Tensor:
        return torch.empty(P, dtype=torch.float32, device=self.device)

    def counter(self) -> torch.Tensor:
        return torch.zeros(1, dtype=torch.int64, device=self.device)

    # -- mixing ----------------------------------------------------------------------------
    def mix_seq(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                alphas: Sequence[float], stream=None, launch: Optional[tuple] = None) -> torch.Tensor:
        """out = fold_j(w <- w + alphas[j]*(nbrs[j] - w)), w0 = local (sequential CFA rule).
        ``launch`` = (blocks_per_cu, vec_per_lane, nontemporal) overrides the launch shape."""
        P = _check_fanin(out, local, nbrs)
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        table = _lib.ptr_table([x.data_ptr() for x in nbrs])
        if launch is None:
            _lib.call("cfa_mix_seq_f32", out.data_ptr(), local.data_ptr(), table,
                      _lib.float_array(alphas), len(nbrs), P, self.stream_handle(stream))
        else:
            lc = _lib.Launch(*launch)
            _lib.call("cfa_mix_seq_ex_f32", out.data_ptr(), local.data_ptr(), table,
                      _lib.float_array(alphas), len(nbrs), P, ctypes.addressof(lc),
                      self.stream_handle(stream))
        return out

    def prepare_mix_seq(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                        alphas: Sequence[float]):
        """mix_seq with its checks and ctypes tables done once: returns ``launch(stream=None)``,
        which enqueues the same kernel with one foreign call. For rounds that repeat the same
        mixes on resident buffers (population shards), where per-launch Python work would
        otherwise approach the kernel time at small buckets. The tensors must stay alive."""
        P = _check_fanin(out, local, nbrs)
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        table = _lib.ptr_table([x.data_ptr() for x in nbrs])
        coeff = _lib.float_array(alphas)
        fn = self.lib.cfa_mix_seq_f32
        args = (out.data_ptr(), local.data_ptr(), table, coeff, len(nbrs), P)
        keep = (out, local, tuple(nbrs), table, coeff)
        dev = self.device

        def launch(stream=None):
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            rc = fn(*args, s.cuda_stream)
            if rc != _lib.CFA_OK:
                msg = self.lib.cfa_last_error()
                raise _lib.CFAError("cfa_mix_seq_f32", rc, msg.decode() if msg else "")

        launch.keep = keep
        return launch

    @staticmethod
    def host_device_ptr(t: torch.Tensor) -> int:
        """Device address of a pinned host tensor (cfa_host_device_pointer)."""
        if not isinstance(t, torch.Tensor) or t.is_cuda or not t.is_pinned():
            raise ValueError("expected a pinned host tensor (pin_memory=True)")
        if not t.is_contiguous():
            raise TypeError("expected a contiguous tensor")
        dev = ctypes.c_void_p()
        _lib.call("cfa_host_device_pointer", ctypes.c_void_p(t.data_ptr()), ctypes.byref(dev))
        return int(dev.value)

    def mix_seq_pinned(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                       alphas: Sequence[float], stream=None) -> torch.Tensor:
        """mix_seq on buckets that live in pinned HOST memory (f2): the kernel reads them over
        PCIe and writes ``out`` (pinned host) directly, with no staging copies, so the link's
        read and write directions overlap. Asynchronous on ``stream`` like mix_seq; the caller
        synchronises before reading ``out``. Results equal mix_seq on device copies."""
        P = local.numel()
        for name, t in [("out", out), ("local", local)] + [(f"nbrs[{j}]", x) for j, x in enumerate(nbrs)]:
            if t.dtype != torch.float32:
                raise TypeError(f"{name} must be fp32 (got {t.dtype})")
            if t.numel() != P:
                raise ValueError(f"{name} has {t.numel()} elements, expected {P}")
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        table = _lib.ptr_table([self.host_device_ptr(x) for x in nbrs])
        _lib.call("cfa_mix_seq_f32", self.host_device_ptr(out), self.host_device_ptr(local), table,
                  _lib.float_array(alphas), len(nbrs), P, self.stream_handle(stream))
        return out

    def mix_seq_div(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                    alphas: Sequence[float], divisors: Sequence[float], stream=None) -> torch.Tensor:
        """out = fold_j(w <- w + (alphas[j]*(nbrs[j] - w)) / divisors[j]) (FedAvg form)."""
        P = _check_fanin(out, local, nbrs)
        if not (len(alphas) == len(divisors) == len(nbrs)):
            raise ValueError("one alpha and one divisor per neighbour required")
        _lib.call("cfa_mix_seq_div_f32", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.float_array(alphas),
                  _lib.float_array(divisors), len(nbrs), P, self.stream_handle(stream))
        return out

    def mix_linear(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                   coeff: Sequence[float], stream=None) -> torch.Tensor:
        """out = coeff[0]*local + sum_j coeff[j+1]*nbrs[j]."""
        P = _check_fanin(out, local, nbrs)
        if len(coeff) != len(nbrs) + 1:
            raise ValueError("len(coeff) must be len(nbrs) + 1")
        _lib.call("cfa_mix_f32", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.float_array(coeff),
                  len(nbrs), P, self.stream_handle(stream))
        return out

    def mix_seq_compress(self, out: torch.Tensor, local: torch.Tensor,
                         nbrs: Sequence[torch.Tensor], alphas: Sequence[float], mode: int,
                         cbegin: int, cend: int, kept: torch.Tensor, stream=None) -> torch.Tensor:
        """Sequential mix fused with the cfa_ongraphs compression epilogue on [cbegin, cend).
        Adds the kept-parameter count to ``kept`` (int64 CUDA tensor of one element)."""
        P = _check_fanin(out, local, nbrs)
        self._check_counter(kept)
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        _lib.call("cfa_mix_seq_compress_f32", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.float_array(alphas),
                  len(nbrs), P, int(mode), int(cbegin), int(cend), kept.data_ptr(),
                  self.stream_handle(stream))
        return out

    def mix_tf1(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                alphas: Sequence[float], mode: int = 0, cbegin: int = 0, cend: int = 0,
                kept: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """TF1 mix with the reference's numpy-2 numerics (fp32 first subtraction, fp64 chain,
        fp64 compression epilogue on [cbegin, cend), one rounding to fp32). ``alphas`` are the
        float64 products eps * wf_j. ``kept`` (int64 CUDA tensor of one element) is required
        when ``mode`` != 0."""
        P = _check_fanin(out, local, nbrs)
        if kept is not None:
            self._check_counter(kept)
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        # above CFA_MAX_FANIN the passes chain through an fp64 scratch bucket from torch's
        # allocator (stream-ordered, and capturable), not a library allocation. It is allocated
        # on the stream the kernel writes it on: a block from another stream's pool could still
        # be in use by work queued there.
        scratch = None
        if len(nbrs) > _lib.CFA_MAX_FANIN:
            ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
            with ctx:
                scratch = torch.empty(P, dtype=torch.float64, device=self.device)
        _lib.call("cfa_mix_tf1_ex_f32", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.double_array(alphas),
                  len(nbrs), P, int(mode), int(cbegin), int(cend),
                  kept.data_ptr() if kept is not None else None,
                  scratch.data_ptr() if scratch is not None else None, self.stream_handle(stream))
        return out

    def mix_tf1_f64(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                    alphas: Sequence[float], step0_f32: bool, mode: int = 0, cbegin: int = 0,
                    cend: int = 0, kept: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """TF1 mix on fp64 buckets (cfa_mix_tf1_f64): the reference's fp64 chain, unrounded.
        ``step0_f32``: the reference's local and first-neighbour arrays are both fp32."""
        P = _check_fanin(out, local, nbrs, torch.float64)
        if kept is not None:
            self._check_counter(kept)
        if len(alphas) != len(nbrs):
            raise ValueError("one alpha per neighbour required")
        _lib.call("cfa_mix_tf1_f64", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.double_array(alphas), len(nbrs),
                  int(bool(step0_f32)), P, int(mode), int(cbegin), int(cend),
                  kept.data_ptr() if kept is not None else None, self.stream_handle(stream))
        return out

    def fold_f64(self, out: torch.Tensor, local: torch.Tensor, nbrs: Sequence[torch.Tensor],
                 alphas: Sequence[float], rule: int, divisors: Optional[Sequence[float]] = None,
                 stream=None) -> torch.Tensor:
        """fp64 fold (cfa_fold_f64): SEQUENTIAL, SEQUENTIAL_DIV (``divisors``) or ACCUMULATE."""
        P = _check_fanin(out, local, nbrs, torch.float64)
        if len(alphas) != len(nbrs) or (divisors is not None and len(divisors) != len(nbrs)):
            raise ValueError("one alpha (and one divisor, when given) per neighbour required")
        _lib.call("cfa_fold_f64", out.data_ptr(), local.data_ptr(),
                  _lib.ptr_table([x.data_ptr() for x in nbrs]), _lib.double_array(alphas),
                  _lib.double_array(divisors) if divisors is not None else None, len(nbrs), int(rule), P,
                  self.stream_handle(stream))
        return out

    def mewma_tf1_f64(self, W: torch.Tensor, s: Sequence[torch.Tensor], g: Sequence[torch.Tensor],
                      rho: float, lr1: float, lr2: float, lr_split: int, init: bool,
                      use_filtered: bool, f32_mask: int = 0, stream=None) -> torch.Tensor:
        """CFA-GE MEWMA on fp64 buckets (cfa_mewma_tf1_f64); W and s_j in place. ``g`` may be
        element-strided 1-D fp64 views. ``f32_mask``: which reference arrays are fp32
        (TF1_STATE_F32 | TF1_GRAD_F32 | TF1_W_F32)."""
        P, strides = _check_mewma(W, s, g, torch.float64)
        _lib.call("cfa_mewma_tf1_f64", W.data_ptr(), _lib.ptr_table([x.data_ptr() for x in s]),
                  _lib.ptr_table([x.data_ptr() for x in g]), _lib.int64_array(strides), len(g),
                  float(rho), float(lr1), float(lr2), int(lr_split), int(bool(init)),
                  int(bool(use_filtered)), int(f32_mask), P, self.stream_handle(stream))
        return W

    def compress(self, y: torch.Tensor, ref: Optional[torch.Tensor], mode: int,
                 kept: torch.Tensor, stream=None) -> torch.Tensor:
        P = _check_bucket(y, "y")
        if ref is not None:
            _check_bucket(ref, "ref", P)
        self._check_counter(kept)
        _lib.call("cfa_compress_epilogue_f32", y.data_ptr(), ref.data_ptr() if ref is not None else None,
                  int(mode), P, kept.data_ptr(), self.stream_handle(stream))
        return y

    @staticmethod
    def _check_counter(kept: torch.Tensor) -> None:
        if not (isinstance(kept, torch.Tensor) and kept.is_cuda and kept.dtype == torch.int64
                and kept.numel() >= 1):
            raise TypeError("kept must be an int64 CUDA tensor")

    # -- CFA-GE ----------------------------------------------------------------------------
    def mewma(self, W: torch.Tensor, s: Sequence[torch.Tensor], g: Sequence[torch.Tensor],
              rho: float, lr1: float, lr2: float, lr_split: int, init: bool, use_filtered: bool,
              stream=None) -> torch.Tensor:
        """CFA-GE update: for each j, s_j <- init ? g_j : rho*g_j + (1-rho)*s_j;
        W <- W - lr*(use_filtered ? s_j : g_j) with lr = lr1 below lr_split, lr2 above."""
        P, strides = _check_mewma(W, s, g, torch.float32)
        _lib.call("cfa_mewma_update_f32", W.data_ptr(), _lib.ptr_table([x.data_ptr() for x in s]),
                  _lib.ptr_table([x.data_ptr() for x in g]), _lib.int64_array(strides), len(g),
                  float(rho), float(lr1), float(lr2), int(lr_split), int(bool(init)),
                  int(bool(use_filtered)), P, self.stream_handle(stream))
        return W

    # -- CFA-GE neighbour gradients (f3) ---------------------------------------------------
    def _grad_args(self, x, y, models, grads):
        B, L = _check_2d(x, "x")
        By, C = _check_2d(y, "y")
        M, P = _check_2d(models, "models")
        if By != B:
            raise ValueError("x and y must hold the same number of samples")
        if tuple(grads.shape) != (M, P):
            raise ValueError("grads must have the shape of models")
        _check_2d(grads, "grads")
        return B, L, C, M, P

    def grad_cnn(self, x: torch.Tensor, y: torch.Tensor, models: torch.Tensor, grads: torch.Tensor,
                 filter: int, number: int, stride: int, stream=None) -> torch.Tensor:
        """Gradients of the CNN cost (cfa_ge_2stage.py:392-405, :425-430) at each row of
        ``models`` [M, P] (TF1 bucket order W1 b1 W2 b2) into ``grads`` [M, P]."""
        B, L, C, M, P = self._grad_args(x, y, models, grads)
        L2 = -(-(-(-L // stride)) // stride)
        if P != filter * number + number + L2 * number * C + C:
            raise ValueError(f"CNN bucket of {P} parameters does not match filter {filter}, number {number}, "
                             f"stride {stride}, {L} inputs, {C} classes (multip must be {L2})")
        _lib.call("cfa_ge_grad_cnn_f32", x.data_ptr(), y.data_ptr(), B, L, C, int(filter), int(number),
                  int(stride), models.data_ptr(), grads.data_ptr(), M, self.stream_handle(stream))
        return grads

    def grad_2nn(self, x: torch.Tensor, y: torch.Tensor, models: torch.Tensor, grads: torch.Tensor,
                 hidden: int, stream=None) -> torch.Tensor:
        """Gradients of the 2NN cost (cfa_ge_2stage.py:407-420, :425-430); see grad_cnn."""
        B, L, C, M, P = self._grad_args(x, y, models, grads)
        if P != L * hidden + hidden + hidden * C + C:
            raise ValueError(f"2NN bucket of {P} parameters does not match {L} inputs, {hidden} hidden, {C} classes")
        _lib.call("cfa_ge_grad_2nn_f32", x.data_ptr(), y.data_ptr(), B, L, int(hidden), C, models.data_ptr(),
                  grads.data_ptr(), M, self.stream_handle(stream))
        return grads

    def grad_workspace(self, M: int, B: int, P: int) -> torch.Tensor:
        """Workspace for the batch-split gradient launch (cfa_ge_grad_workspace_elems)."""
        n = int(_lib.load().cfa_ge_grad_workspace_elems(int(M), int(B), int(P)))
        return torch.empty(max(n, 1), dtype=torch.float32, device=self.device)

    def grad_splits(self, M: int, B: int, P: int) -> int:
        """Workgroups per evaluation of a split gradient launch (cfa_ge_grad_splits)."""
        return int(_lib.load().cfa_ge_grad_splits(int(M), int(B), int(P)))

    def grad_rows(self, ml_model: int, x: torch.Tensor, y: torch.Tensor, models: torch.Tensor,
                  model_row: torch.Tensor, data_row: torch.Tensor, grads: Optional[torch.Tensor], geom: dict,
                  stream=None, workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """Population form (cfa_ge_grad_{cnn,2nn}_rows_f32): evaluation m = gradient of data row
        data_row[m] (x [Dx, B, L], y [Dx, B, C]) at model row model_row[m] of models [Dm, P],
        into grads [M, P]. ``geom``: filter/number/stride (CNN) or intermediate_nodes (2NN).
        ``workspace`` (``grad_workspace``) lets each evaluation's batch spread over workgroups.
        ``grads=None``: partials only, [M][grad_splits(M, B, P)][P] into ``workspace`` (at least
        that size), summed later by ``ge_population_step(..., reduce=...)``."""
        Dx, B, L = _check_nd(x, "x", 3)
        C = _check_nd(y, "y", 3)[2]
        Dm, P = _check_2d(models, "models")
        if grads is None:
            if workspace is None:
                raise ValueError("a partials-only launch (grads=None) needs a workspace")
            M, Pg = int(model_row.numel()), P
            need = M * self.grad_splits(M, B, P) * P
            if workspace.numel() < need:
                raise ValueError(f"partials-only launch needs a workspace of {need} floats")
        else:
            M, Pg = _check_2d(grads, "grads")
        for name, t in (("model_row", model_row), ("data_row", data_row)):
            if not t.is_cuda or t.dtype != torch.int32 or t.numel() != M or not t.is_contiguous():
                raise TypeError(f"{name} must be a contiguous int32 CUDA tensor of {M} entries")
        if tuple(y.shape[:2]) != (Dx, B) or Pg != P:
            raise ValueError("y must be [Dx, B, C] and grads [M, P]")
        ws_ptr, ws_n = None, 0
        if workspace is not None:
            if not workspace.is_cuda or workspace.dtype != torch.float32 or not workspace.is_contiguous():
                raise TypeError("workspace must be a contiguous fp32 CUDA tensor")
            ws_ptr, ws_n = workspace.data_ptr(), workspace.numel()
        if ml_model == 1:
            F, NC, S = int(geom["filter"]), int(geom["number"]), int(geom["stride"])
            L2 = -(-(-(-L // S)) // S)
            if P != F * NC + NC + L2 * NC * C + C:
                raise ValueError("CNN bucket size does not match the geometry")
            _lib.call("cfa_ge_grad_cnn_rows_f32", x.data_ptr(), y.data_ptr(), B, L, C, F, NC, S, models.data_ptr(),
                      model_row.data_ptr(), data_row.data_ptr(), None if grads is None else grads.data_ptr(), ws_ptr,
                      ws_n, M, self.stream_handle(stream))
        elif ml_model == 2:
            H = int(geom["intermediate_nodes"])
            if P != L * H + H + H * C + C:
                raise ValueError("2NN bucket size does not match the geometry")
            _lib.call("cfa_ge_grad_2nn_rows_f32", x.data_ptr(), y.data_ptr(), B, L, H, C, models.data_ptr(),
                      model_row.data_ptr(), data_row.data_ptr(), None if grads is None else grads.data_ptr(), ws_ptr,
                      ws_n, M, self.stream_handle(stream))
        else:
            raise ValueError("ml_model must be 1 (CNN) or 2 (2NN)")
        return grads

    # -- local training between rounds (f3/f4) ----------------------------------------------
    def local_sgd(self, ml_model: int, x: torch.Tensor, y: torch.Tensor, models: torch.Tensor, geom: dict,
                  batch_stride: int, batch_rows: int, steps: int, lr: float, update: bool = True,
                  cost: Optional[torch.Tensor] = None, cost_log: Optional[torch.Tensor] = None,
                  epoch: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """One local epoch of minibatch SGD for every device in one launch
        (cfa_local_sgd_{cnn,2nn}_f32): device d steps row d of ``models`` [D, P] (fp32 CUDA, unit
        element stride, any row pitch; TF1 order W1 b1 W2 b2) through ``steps`` minibatches of its
        own samples x [D, Ns, L] / y [D, Ns, C], minibatch i = rows [i * batch_stride,
        i * batch_stride + batch_rows), with w <- w - lr * grad. ``update=False`` is the validation
        pass: forward only, ``models`` untouched. ``cost`` [D] fp64 CUDA receives each device's
        mean minibatch cost. ``cost_log`` [cap, D] fp64 CUDA and ``epoch`` (one-element int64
        CUDA counter), given together: the cost also goes to row min(epoch, cap - 1) of the log
        and the counter is left one higher, in stream order. ``geom`` as ``grad_rows``."""
        D, Ns, L = _check_nd(x, "x", 3)
        Dy, Nsy, C = _check_nd(y, "y", 3)
        Dm, P = _check_nd(models, "models", pitched=True)
        if (Dy, Nsy) != (D, Ns) or Dm != D:
            raise ValueError("x [D, Ns, L], y [D, Ns, C] and models [D, P] must agree on D and Ns")
        batch_stride, batch_rows, steps = int(batch_stride), int(batch_rows), int(steps)
        if steps < 1 or batch_rows < 1 or batch_stride < 1:
            raise ValueError("steps, batch_rows and batch_stride must be >= 1")
        if (steps - 1) * batch_stride + batch_rows > Ns:
            raise ValueError(f"minibatch {steps - 1} ends at row {(steps - 1) * batch_stride + batch_rows} "
                             f"of {Ns} samples")
        if cost is not None:
            _check_bucket(cost, "cost", D, torch.float64)
        if (cost_log is None) != (epoch is None):
            raise ValueError("cost_log and epoch are given together or not at all")
        cap = 0
        if cost_log is not None:
            _check_tables(("cost_log", cost_log, torch.float64), ("epoch", epoch, torch.int64))
            if cost_log.dim() != 2 or cost_log.shape[1] != D or cost_log.shape[0] < 1 or epoch.numel() != 1:
                raise ValueError("cost_log must be [cap >= 1, D] and epoch a one-element counter")
            cap = int(cost_log.shape[0])
        pitch = int(models.stride(0)) if D > 1 else P
        if pitch < P:
            raise ValueError("models rows overlap (pitch below P)")
        tail = (pitch, D, batch_stride, batch_rows, steps, float(lr), int(bool(update)),
                cost.data_ptr() if cost is not None else None,
                cost_log.data_ptr() if cost_log is not None else None, cap,
                epoch.data_ptr() if epoch is not None else None, self.stream_handle(stream))
        if ml_model == 1:
            F, NC, S = int(geom["filter"]), int(geom["number"]), int(geom["stride"])
            L2 = -(-(-(-L // S)) // S)
            if P != F * NC + NC + L2 * NC * C + C:
                raise ValueError("CNN bucket size does not match the geometry")
            _lib.call("cfa_local_sgd_cnn_f32", x.data_ptr(), y.data_ptr(), Ns, L, C, F, NC, S, models.data_ptr(), *tail)
        elif ml_model == 2:
            H = int(geom["intermediate_nodes"])
            if P != L * H + H + H * C + C:
                raise ValueError("2NN bucket size does not match the geometry")
            _lib.call("cfa_local_sgd_2nn_f32", x.data_ptr(), y.data_ptr(), Ns, L, H, C, models.data_ptr(), *tail)
        else:
            raise ValueError("ml_model must be 1 (CNN) or 2 (2NN)")
        return models

    # -- validation pass of a TF2 LeNet-1 population ------------------------------------------
    def lenet_params(self, geom: Sequence[int]) -> int:
        """Parameters of a LeNet-family model (cfa_lenet_params); 0 for a geometry without one."""
        geom = tuple(int(v) for v in geom)
        if len(geom) == 7:
            return int(_lib.load().cfa_lenet_hidden_params(*geom))
        return int(_lib.load().cfa_lenet_params(*geom))

    @staticmethod
    def _lenet_sets(geom: Sequence[int], pool: str, x: torch.Tensor, labels: torch.Tensor,
                    models: torch.Tensor) -> tuple:
        """What lenet_eval and lenet_grad take from their geometry, set and models: (geom, entry-point
        infix, D, P, Nt, x_stride, label_stride), with the set shared ([Nt, image]: strides 0) or one
        per device ([D, Nt, image]); image is [side, side], or [side, side, channels] for seven numbers."""
        geom, infix, image = _lib.lenet_family(geom, pool)
        D, P = _check_nd(models, "models", pitched=True)
        nd = 1 + len(image)  # 3, or 4 with the channel axis of the hidden-layer family
        if x.dim() == nd:
            Nt = _check_nd(x, "x", nd)[0]
            x_stride = label_stride = 0
            shapes = ((Nt,) + image, (Nt,))
        else:
            what = "[Nt, side, side] or [D, Nt, side, side]" if nd == 3 else \
                "[Nt, side, side, channels] or [D, Nt, side, side, channels]"
            Nt = _check_nd(x, "x", nd + 1, what=what)[1]
            x_stride, label_stride = Nt * int(np.prod(image)), Nt
            shapes = ((D, Nt) + image, (D, Nt))
        _check_tables(("labels", labels, torch.int32))
        if (tuple(x.shape), tuple(labels.shape)) != shapes:
            raise ValueError(f"x and labels must be {shapes[0]} and {shapes[1]} for these models and this geometry")
        return geom, infix, D, P, Nt, x_stride, label_stride

    def lenet_workspace(self, D: int, batches: int, pool: str = "avg",
                        geom: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Workspace of the batch losses (cfa_lenet_eval_workspace_bytes, cfa_lenet_max_eval_workspace_bytes
        for ``pool="max"``, or cfa_lenet_hidden_eval_workspace_bytes for a seven-number ``geom``)."""
        infix = _lib.lenet_pool(pool) if geom is None else _lib.lenet_family(geom, pool)[1]
        fn = getattr(_lib.load(), f"cfa_lenet_{infix}eval_workspace_bytes")
        n = int(fn(int(D), int(batches)))
        return torch.empty(max(n // 4, 1), dtype=torch.float32, device=self.device)

    def lenet_eval(self, geom: Sequence[int], x: torch.Tensor, labels: torch.Tensor, models: torch.Tensor,
                   batch: int, batches: int, cost: torch.Tensor, workspace: torch.Tensor,
                   skip: Optional[torch.Tensor] = None, target: float = 0.0, ended: Optional[torch.Tensor] = None,
                   cost_log: Optional[torch.Tensor] = None, epoch: Optional[torch.Tensor] = None,
                   stream=None, loss: str = "xent", pool: str = "avg") -> torch.Tensor:
        """cfa_lenet_eval_loss_f32: the validation cost of every device of ``models`` [D, P] (fp32 CUDA,
        unit element stride, any row pitch, read only; get_weights() order) on the LeNet-family
        ``geom`` = (side, kernel, c1, c2, classes), over ``batches`` batches of ``batch`` samples
        of the test set ``x`` [Nt, side, side] fp32 / ``labels`` [Nt] int32 that all devices share,
        or ``x`` [D, Nt, side, side] / ``labels`` [D, Nt] with one set per device (all contiguous
        CUDA). ``cost`` [D] fp64 CUDA receives each device's mean batch loss. ``skip`` [D] int32
        CUDA flags or None: a flagged device's cost and flag are not touched. ``ended`` [D] int32
        CUDA or None: ``ended[d] |= cost[d] < target``; it may be ``skip`` itself. ``cost_log``
        [cap, D] fp64 CUDA and ``epoch`` (one-element int64 CUDA counter), given together: as
        ``local_sgd``. ``workspace``: ``lenet_workspace(D, batches)``. ``loss``: "xent" (the
        cross-entropy drivers' objective) or "huber" (the Huber drivers': Huber(label,
        softmax(z)[label])); ValueError for any other, before any device call. ``pool``: "avg"
        (LeNet-1's AveragePooling2D) or "max" (cfa_lenet_max_eval_loss_f32: the drivers' max-pool
        CNNs, ``workspace`` from ``lenet_workspace(D, batches, "max")``); ValueError for any
        other. A ``geom`` of seven numbers (side, channels, kernel, c1, c2, hidden, classes) is the
        hidden-layer family (cfa_lenet_hidden_eval_loss_f32: the CIFAR drivers' ``CIFAR_LENET``):
        ``x`` is [Nt, side, side, channels] or [D, Nt, side, side, channels], always with the
        channel axis, ``workspace`` from ``lenet_workspace(D, batches, geom=geom)``, and
        ``pool="max"`` a ValueError. The library validates the rest (CFAError)."""
        kind = _lib.lenet_loss_kind(loss)
        geom, infix, D, P, Nt, x_stride, label_stride = self._lenet_sets(geom, pool, x, labels, models)
        if P != self.lenet_params(geom):
            raise ValueError("models' row size does not match the geometry")
        batch, batches = int(batch), int(batches)
        if batch < 1 or batches < 1 or batch * batches > Nt:
            raise ValueError(f"{batches} batches of {batch} samples do not fit the {Nt} of the test set")
        _check_bucket(cost, "cost", D, torch.float64)
        for name, t in (("skip", skip), ("ended", ended)):
            if t is not None:
                _check_tables((name, t, torch.int32))
                if t.numel() != D:
                    raise ValueError(f"{name} must hold one int32 flag per device")
        if (cost_log is None) != (epoch is None):
            raise ValueError("cost_log and epoch are given together or not at all")
        cap = 0
        if cost_log is not None:
            _check_tables(("cost_log", cost_log, torch.float64), ("epoch", epoch, torch.int64))
            if cost_log.dim() != 2 or cost_log.shape[1] != D or cost_log.shape[0] < 1 or epoch.numel() != 1:
                raise ValueError("cost_log must be [cap >= 1, D] and epoch a one-element counter")
            cap = int(cost_log.shape[0])
        _check_tables(("workspace", workspace, torch.float32))
        pitch = int(models.stride(0)) if D > 1 else P
        if pitch < P:
            raise ValueError("models rows overlap (pitch below P)")
        _lib.call(f"cfa_lenet_{infix}eval_loss_f32", x.data_ptr(), x_stride, labels.data_ptr(), label_stride, Nt, *geom,
                  models.data_ptr(), pitch, D, batch, batches, skip.data_ptr() if skip is not None else None,
                  float(target), ended.data_ptr() if ended is not None else None, cost.data_ptr(),
                  cost_log.data_ptr() if cost_log is not None else None, cap,
                  epoch.data_ptr() if epoch is not None else None, workspace.data_ptr(), workspace.numel() * 4,
                  kind, self.stream_handle(stream))
        return cost

    # -- minibatch gradient of a TF2 LeNet-1 population ---------------------------------------
    def lenet_grad_workspace(self, D: int, batch: int, geom: Sequence[int], pool: str = "avg") -> torch.Tensor:
        """Workspace of the sample groups' partial gradients (cfa_lenet_grad_workspace_bytes, or
        cfa_lenet_max_grad_workspace_bytes for ``pool="max"``)."""
        geom, infix, _ = _lib.lenet_family(geom, pool)
        fn = getattr(_lib.load(), f"cfa_lenet_{infix}grad_workspace_bytes")
        n = int(fn(int(D), int(batch), *geom))
        return torch.empty(max(n // 4, 1), dtype=torch.float32, device=self.device)

    def lenet_grad(self, geom: Sequence[int], x: torch.Tensor, labels: torch.Tensor, models: torch.Tensor,
                   batch: int, grads: torch.Tensor, workspace: torch.Tensor, loss: Optional[torch.Tensor] = None,
                   src: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                   skip: Optional[torch.Tensor] = None, stream=None, loss_kind: str = "xent",
                   pool: str = "avg") -> torch.Tensor:
        """cfa_lenet_grad_loss_f32: the mean loss and its gradient over one batch of ``batch`` samples
        for every device of ``models`` [D, P] (fp32 CUDA, unit element stride, any row pitch, read
        only) on the LeNet-family ``geom``, with the training set ``x`` [Nt, side, side] fp32 /
        ``labels`` [Nt] int32 all devices share, or [D, Nt, side, side] / [D, Nt] with one set per
        device (contiguous CUDA). ``grads`` [D, P] fp32 CUDA (unit element stride, any row pitch)
        receives the gradients and ``loss`` ([D] fp32 CUDA, or None) the batch losses. ``src``
        ([D] int32 CUDA, or None): device d evaluates row ``src[d]`` of ``models`` on its own
        data; values outside [0, D) are the caller's error. ``first`` ([D] int64 CUDA, or None
        for 0): the first sample of every device's batch; a batch past the set's end wraps.
        ``skip`` ([D] int32 CUDA, or None): a flagged device's row and loss are not touched.
        ``workspace``: ``lenet_grad_workspace(D, batch, geom)``. ``loss_kind``: the objective,
        "xent" or "huber" as ``lenet_eval``'s ``loss`` (here ``loss`` is the output buffer);
        ValueError for any other, before any device call. ``pool``: "avg" or "max" as
        ``lenet_eval``'s (cfa_lenet_max_grad_loss_f32, ``workspace`` from
        ``lenet_grad_workspace(D, batch, geom, "max")``). A ``geom`` of seven numbers is the
        hidden-layer family as in ``lenet_eval`` (cfa_lenet_hidden_grad_loss_f32), with ``x``
        [Nt, side, side, channels] or [D, Nt, side, side, channels]. The library validates the
        rest (CFAError)."""
        kind = _lib.lenet_loss_kind(loss_kind)
        geom, infix, D, P, Nt, x_stride, label_stride = self._lenet_sets(geom, pool, x, labels, models)
        if P != self.lenet_params(geom):
            raise ValueError("models' row size does not match the geometry")
        batch = int(batch)
        if batch < 1 or batch > Nt:
            raise ValueError(f"a batch of {batch} samples does not fit the {Nt} of the training set")
        if _check_nd(grads, "grads", pitched=True) != (D, P):
            raise ValueError(f"grads must be [{D}, {P}]")
        if loss is not None:
            _check_bucket(loss, "loss", D, torch.float32)
        for name, t, dt in (("src", src, torch.int32), ("first", first, torch.int64), ("skip", skip, torch.int32)):
            if t is not None:
                _check_tables((name, t, dt))
                if t.numel() != D:
                    raise ValueError(f"{name} must hold one {dt} entry per device")
        _check_tables(("workspace", workspace, torch.float32))
        pitch = int(models.stride(0)) if D > 1 else P
        gpitch = int(grads.stride(0)) if D > 1 else P
        if pitch < P or gpitch < P:
            raise ValueError("models or grads rows overlap (pitch below P)")
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.call(f"cfa_lenet_{infix}grad_loss_f32", x.data_ptr(), x_stride, labels.data_ptr(), label_stride, Nt, *geom,
                  models.data_ptr(), pitch, D, ptr(src), ptr(first), batch, ptr(skip), grads.data_ptr(), gpitch,
                  ptr(loss), workspace.data_ptr(), workspace.numel() * 4, kind, self.stream_handle(stream))
        return grads

    # -- local optimizer step of a TF2 population ---------------------------------------------
    def optim_tile(self) -> int:
        """Elements of a tile of the optimizer step (cfa_optim_tile)."""
        return int(_lib.load().cfa_optim_tile())

    def optim_workspace(self, D: int, P: int, n_layers: int) -> torch.Tensor:
        """Workspace of the Adam clip's partial sums (cfa_optim_workspace_bytes)."""
        n = int(_lib.load().cfa_optim_workspace_bytes(int(D), int(P), int(n_layers)))
        return torch.empty(max(n // 8, 1), dtype=torch.float64, device=self.device)

    def optim_step(self, rule: int, models: torch.Tensor, grads: torch.Tensor, layer_ptr: torch.Tensor,
                   trainable: torch.Tensor, t: torch.Tensor, lr: float, m: Optional[torch.Tensor] = None,
                   v: Optional[torch.Tensor] = None, pow: Optional[torch.Tensor] = None,
                   skip: Optional[torch.Tensor] = None, momentum: float = 0.0, beta_1: float = 0.9,
                   beta_2: float = 0.999, epsilon: float = 1e-7, clipnorm: float = 0.0,
                   workspace: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        """cfa_optim_step_f32: one local optimizer step of every device of ``models`` [D, P], in
        place, with the gradients ``grads`` [D, P] (both fp32 CUDA, unit element stride, any row
        pitch). ``rule``: _lib.OPTIM_SGD (w - lr * g), OPTIM_MOMENTUM (Keras momentum, the
        accumulator in ``m``) or OPTIM_ADAM (Keras Adam on ``m`` / ``v``, after tf.clip_by_norm per
        device and layer when ``clipnorm`` > 0, which needs ``workspace`` from
        ``optim_workspace``). ``layer_ptr`` [n + 1] and ``trainable`` [n] are int32 CUDA tables (a
        layer with 0 is not touched; the caller checks the table before the upload), ``skip`` [D]
        int32 CUDA flags or None (a flagged device is not touched), ``t`` [D] int64 CUDA step
        counters and ``pow`` [D, 2] fp64 CUDA running powers of the betas (Adam), both left one
        step on for every device stepped, in stream order. ``m`` / ``v`` [D, P] are the caller's
        state, pitched like ``models``. The library validates the rest (CFAError)."""
        D, P = _check_nd(models, "models", pitched=True)
        if _check_nd(grads, "grads", pitched=True) != (D, P):
            raise ValueError("grads must be [D, P] like models")
        need = {_lib.OPTIM_SGD: (), _lib.OPTIM_MOMENTUM: ("m",), _lib.OPTIM_ADAM: ("m", "v")}.get(int(rule))
        if need is None:
            raise ValueError(f"unknown optimizer rule {rule}")
        state = {"m": m, "v": v}
        spitch = P
        for name in need:
            s = state[name]
            if s is None or _check_nd(s, name, pitched=True) != (D, P):
                raise ValueError(f"{name} must be a [D, P] fp32 CUDA tensor for this rule")
        if len(need) == 2 and D > 1 and m.stride(0) != v.stride(0):
            raise ValueError("m and v must have the same row pitch")
        if need and D > 1:
            spitch = int(m.stride(0))
        _check_tables(("layer_ptr", layer_ptr, torch.int32), ("trainable", trainable, torch.int32),
                      ("t", t, torch.int64))
        n = trainable.numel()
        if n < 1 or layer_ptr.numel() != n + 1 or t.numel() != D:
            raise ValueError("layer_ptr must hold n + 1 offsets, trainable n >= 1 flags and t one counter per device")
        if skip is not None:
            _check_tables(("skip", skip, torch.int32))
            if skip.numel() != D:
                raise ValueError("skip must hold one int32 flag per device")
        adam = int(rule) == _lib.OPTIM_ADAM
        if adam:
            if pow is None:
                raise ValueError("Adam needs the running powers pow [D, 2]")
            _check_tables(("pow", pow, torch.float64))
            if tuple(pow.shape) != (D, 2):
                raise ValueError("pow must be [D, 2]")
        ws_ptr, ws_bytes = None, 0
        if workspace is not None:
            _check_tables(("workspace", workspace, torch.float64))
            ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel() * 8
        _lib.call("cfa_optim_step_f32", models.data_ptr(), int(models.stride(0)) if D > 1 else P, grads.data_ptr(),
                  int(grads.stride(0)) if D > 1 else P, state["m"].data_ptr() if need else None,
                  state["v"].data_ptr() if len(need) == 2 else None, spitch, layer_ptr.data_ptr(),
                  trainable.data_ptr(), n, skip.data_ptr() if skip is not None else None, t.data_ptr(),
                  pow.data_ptr() if adam else None, int(rule), float(lr), float(momentum), float(beta_1),
                  float(beta_2), float(epsilon), float(clipnorm), ws_ptr, ws_bytes, D, P, self.stream_handle(stream))
        return models

    # -- population ------------------------------------------------------------------------
    def mix_window(self, outs: Sequence[torch.Tensor], rows: Sequence[torch.Tensor], alphas: Sequence[Sequence[float]],
                   hl: int, hr: int, stream=None) -> None:
        """One sliding-window pass (cfa_mix_window_f32): len(outs) consecutive devices, rows =
        the window's len(outs) + hl + hr buckets in device order, alphas[b] = device b's step
        coefficients (hl + hr values, all equal: the kernel takes one per device)."""
        nb = len(outs)
        if len(rows) != nb + hl + hr or len(alphas) != nb:
            raise ValueError("window needs nb + hl + hr rows and one alpha list per device")
        P = _check_bucket(rows[0], "rows[0]")
        for k, r in enumerate(rows):
            _check_bucket(r, f"rows[{k}]", P)
        for b, o in enumerate(outs):
            _check_bucket(o, f"outs[{b}]", P)
        per_dev = []
        for b, al in enumerate(alphas):
            al = [float(a) for a in al]
            if len(al) != hl + hr or len(set(al)) > 1:
                raise ValueError(f"device {b}: the window pass needs hl + hr equal alphas, got {al}")
            per_dev.append(al[0] if al else 0.0)
        _lib.call("cfa_mix_window_f32", _lib.ptr_table([o.data_ptr() for o in outs]),
                  _lib.ptr_table([r.data_ptr() for r in rows]), _lib.float_array(per_dev), nb, int(hl), int(hr), P,
                  self.stream_handle(stream))
    def ring_round(self, out: torch.Tensor, models: torch.Tensor, alphas: torch.Tensor, hl: int, hr: int,
                   stream=None) -> torch.Tensor:
        """cfa_mix_ring_round_f32: one launch mixing every device of a stacked [D, P] population
        with its ring window [d-hl .. d-1, d+1 .. d+hr] (mod D); ``alphas`` [D] fp32 CUDA (one
        coefficient per device); out [D, P] must not overlap models."""
        D, P = _check_2d(models, "models")
        if _check_nd(out, "out", what="[D, P]") != (D, P):
            raise TypeError("out must be a contiguous [D, P] fp32 CUDA tensor")
        if not alphas.is_cuda or alphas.dtype != torch.float32 or alphas.numel() != D or not alphas.is_contiguous():
            raise TypeError("alphas must be a contiguous fp32 CUDA tensor of D entries")
        _lib.call("cfa_mix_ring_round_f32", out.data_ptr(), models.data_ptr(), P, alphas.data_ptr(), D, int(hl),
                  int(hr), P, self.stream_handle(stream))
        return out

    def ring_slide(self, out: torch.Tensor, models: torch.Tensor, alphas: torch.Tensor, first: int, count: int,
                   hl: int, hr: int, stream=None) -> torch.Tensor:
        """cfa_mix_ring_slide_f32: devices first .. first+count-1 of a stacked [rows, P] population,
        each mixed with its ring window [d-hl .. d-1, d+1 .. d+hr] (mod rows), every row read once
        and every output row written once. ``out`` and ``models`` are [rows, P] fp32 CUDA with unit
        element stride (their row pitches may differ); ``alphas`` [count] fp32 CUDA, one coefficient
        per device of the run; rows of ``out`` outside the run are left as they are. The library
        validates the run and the layout (CFAError: CFA_E_INVALID / CFA_E_UNSUPPORTED)."""
        out_shape = _check_nd(out, "out", pitched=True)
        rows, P = _check_nd(models, "models", pitched=True)
        if out_shape != (rows, P):
            raise TypeError("out must have the shape of models")
        if not alphas.is_cuda or alphas.dtype != torch.float32 or alphas.numel() < max(int(count), 1) \
                or not alphas.is_contiguous():
            raise TypeError("alphas must be a contiguous fp32 CUDA tensor of at least count entries")
        out_pitch = int(out.stride(0)) if rows > 1 else P
        in_pitch = int(models.stride(0)) if rows > 1 else P
        _lib.call("cfa_mix_ring_slide_f32", out.data_ptr(), out_pitch, models.data_ptr(), in_pitch,
                  alphas.data_ptr(), rows, int(first), int(count), int(hl), int(hr), P, self.stream_handle(stream))
        return out

    def ge_population_step(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, state_ptrs: torch.Tensor,
                           grad_ptrs: torch.Tensor, csr_ptr: torch.Tensor, csr_idx: torch.Tensor,
                           csr_coef: torch.Tensor, D: int, rho: float, lr1: float, lr2: float, lr_split: int,
                           use_filtered: bool, P: int, stream=None, reduce=None) -> None:
        """cfa_ge_population_step_f32: stage-1 mix + MEWMA gradient step of D devices in one
        launch; pointer tables are int64 CUDA tensors aligned with the CSR entries.
        ``reduce=(workspace, out [M, P], splits)``: the same launch also sums a partials-only
        gradient launch's [M][splits][P] workspace into ``out``."""
        _check_tables(("out_ptrs", out_ptrs, torch.int64), ("src_ptrs", src_ptrs, torch.int64),
                      ("state_ptrs", state_ptrs, torch.int64), ("grad_ptrs", grad_ptrs, torch.int64),
                      ("csr_ptr", csr_ptr, torch.int32), ("csr_idx", csr_idx, torch.int32),
                      ("csr_coef", csr_coef, torch.float32))
        E = csr_idx.numel()
        if csr_ptr.numel() != D + 1 or out_ptrs.numel() != D or state_ptrs.numel() != E or grad_ptrs.numel() != E:
            raise ValueError("tables: D+1 row pointers, D outputs, one state and one gradient slot per CSR entry")
        r_ws = r_out = None
        r_M = r_sp = 0
        if reduce is not None:
            ws, out, r_sp = reduce
            r_M, Po = _check_2d(out, "reduce out")
            r_sp = int(r_sp)
            if Po != P or r_sp < 1 or not ws.is_cuda or ws.dtype != torch.float32 or ws.numel() < r_M * r_sp * P:
                raise ValueError("reduce: out [M, P] and a workspace of M * splits * P fp32 elements")
            r_ws, r_out = ws.data_ptr(), out.data_ptr()
        _lib.call("cfa_ge_population_step_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(), state_ptrs.data_ptr(),
                  grad_ptrs.data_ptr(), csr_ptr.data_ptr(), csr_idx.data_ptr(), csr_coef.data_ptr(), int(D),
                  float(rho), float(lr1), float(lr2), int(lr_split), int(bool(use_filtered)), int(P), r_ws, r_out,
                  int(r_M), int(r_sp), self.stream_handle(stream))

    @staticmethod
    def _check_csr(out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor, csr_idx: torch.Tensor,
                   csr_coef: torch.Tensor, coef_dtype, D: int, sched: Optional[torch.Tensor] = None,
                   round: Optional[torch.Tensor] = None) -> tuple:
        """The five tables of a CSR round (int64 pointers, int32 CSR, ``coef_dtype`` coefficients)
        and their sizes: one table of D+1 row offsets, or with ``sched`` and ``round`` the T tables
        of a schedule (``_check_schedule``). Returns (S, T), (0, 0) without a schedule."""
        _check_tables(("out_ptrs", out_ptrs, torch.int64), ("src_ptrs", src_ptrs, torch.int64),
                      ("csr_ptr", csr_ptr, torch.int32), ("csr_idx", csr_idx, torch.int32),
                      ("csr_coef" if coef_dtype == torch.float32 else "csr_coef64", csr_coef, coef_dtype))
        if sched is not None:
            return Engine._check_schedule(csr_ptr, out_ptrs, sched, round, D)
        if csr_ptr.numel() != D + 1 or out_ptrs.numel() != D:
            raise ValueError("csr_ptr must have D+1 entries and out_ptrs D entries")
        return 0, 0

    @staticmethod
    def _kept_ptr(mode: int, kept: Optional[torch.Tensor], D: int):
        """The address of a TF1 round's ``kept`` counters (None without them), which a compression
        ``mode`` needs: an int64 CUDA tensor of D counters."""
        if mode and (kept is None or not kept.is_cuda or kept.dtype != torch.int64 or kept.numel() != D):
            raise TypeError("compression needs kept: an int64 CUDA tensor of D counters")
        return kept.data_ptr() if kept is not None else None

    def population_tf1(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor,
                       csr_idx: torch.Tensor, csr_coef64: torch.Tensor, D: int, P: int, stream=None,
                       mode: int = 0, cbegin: int = 0, cend: int = 0,
                       kept: Optional[torch.Tensor] = None) -> None:
        """One launch mixing D devices with the TF1 numerics (cfa_mix_population_tf1_f32):
        fp32 first subtraction, fp64 chain with fp64 coefficients, one rounding to fp32.
        ``mode`` != 0: the compression epilogue on [cbegin, cend) of every device, counts added
        to ``kept`` (int64 CUDA tensor of D zeroed counters)."""
        self._check_csr(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef64, torch.float64, D)
        _lib.call("cfa_mix_population_tf1_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(), csr_ptr.data_ptr(),
                  csr_idx.data_ptr(), csr_coef64.data_ptr(), int(D), int(P), int(mode), int(cbegin), int(cend),
                  self._kept_ptr(mode, kept, D), self.stream_handle(stream))

    def population(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor,
                   csr_idx: torch.Tensor, csr_coef: torch.Tensor, D: int, rule: int, P: int,
                   stream=None) -> None:
        """One launch mixing D devices; tables are device tensors (int64 pointers, int32 CSR,
        fp32 coefficients). See cfa_mix_population_f32."""
        self._check_csr(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, torch.float32, D)
        _lib.call("cfa_mix_population_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(),
                  csr_ptr.data_ptr(), csr_idx.data_ptr(), csr_coef.data_ptr(), int(D), int(rule),
                  int(P), self.stream_handle(stream))

    @staticmethod
    def _check_schedule(csr_ptr: torch.Tensor, out_ptrs: torch.Tensor, sched: torch.Tensor, round: torch.Tensor,
                        D: int) -> tuple:
        """(S, T) of a topology schedule: ``csr_ptr`` holds T tables of D+1 row offsets, ``sched``
        S table indices (int32 CUDA, checked against T by whoever uploaded them), ``round`` the
        one-element int64 CUDA round counter."""
        _check_tables(("sched", sched, torch.int32), ("round", round, torch.int64))
        if round.numel() != 1:
            raise TypeError("round must be a one-element int64 CUDA tensor")
        T, rest = divmod(csr_ptr.numel(), D + 1)
        if T < 1 or rest or out_ptrs.numel() != D:
            raise ValueError("csr_ptr must hold T >= 1 tables of D+1 entries and out_ptrs D entries")
        return sched.numel(), T

    def population_sched(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor,
                         csr_idx: torch.Tensor, csr_coef: torch.Tensor, sched: torch.Tensor, round: torch.Tensor,
                         D: int, rule: int, P: int, stream=None) -> None:
        """``population`` under a topology schedule (cfa_mix_population_sched_f32): mixes with
        table ``sched[round % S]`` of the T tables in ``csr_ptr`` (absolute offsets into the
        shared ``csr_idx`` / ``csr_coef``) and leaves ``round`` one higher, in stream order."""
        S, T = self._check_csr(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, torch.float32, D, sched, round)
        _lib.call("cfa_mix_population_sched_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(), csr_ptr.data_ptr(),
                  csr_idx.data_ptr(), csr_coef.data_ptr(), sched.data_ptr(), S, T, round.data_ptr(), int(D),
                  int(rule), int(P), self.stream_handle(stream))

    def population_sched_tf1(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor,
                             csr_idx: torch.Tensor, csr_coef64: torch.Tensor, sched: torch.Tensor,
                             round: torch.Tensor, D: int, P: int, stream=None, mode: int = 0, cbegin: int = 0,
                             cend: int = 0, kept: Optional[torch.Tensor] = None) -> None:
        """``population_tf1`` under a topology schedule (cfa_mix_population_sched_tf1_f32); the
        schedule arguments as ``population_sched``, the rest as ``population_tf1``."""
        S, T = self._check_csr(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef64, torch.float64, D, sched, round)
        _lib.call("cfa_mix_population_sched_tf1_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(), csr_ptr.data_ptr(),
                  csr_idx.data_ptr(), csr_coef64.data_ptr(), sched.data_ptr(), S, T, round.data_ptr(), int(D),
                  int(P), int(mode), int(cbegin), int(cend), self._kept_ptr(mode, kept, D),
                  self.stream_handle(stream))

    def population_ended(self, out_ptrs: torch.Tensor, src_ptrs: torch.Tensor, csr_ptr: torch.Tensor,
                         csr_idx: torch.Tensor, csr_coef: torch.Tensor, ended: torch.Tensor,
                         ended_next: Optional[torch.Tensor], saw: Optional[torch.Tensor], ended_rule: int, D: int,
                         P: int, sched: Optional[torch.Tensor] = None, round: Optional[torch.Tensor] = None,
                         stream=None) -> None:
        """``population`` (sequential rule) with the training_end rule on device-resident flags
        (cfa_mix_population_ended_f32). ``ended`` [D] int32 CUDA: the round's input flags;
        ``ended_next`` (``ended | saw``) and ``saw`` (a flagged neighbour was collected) are int32
        CUDA tensors of D entries or None, written by the launch. ``ended_rule``:
        _lib.ENDED_COPY / ENDED_TRUNCATE / ENDED_TRUNCATE_EPS. With ``sched`` and ``round`` the
        tables and the counter are those of ``population_sched``; with neither, one table."""
        if (sched is None) != (round is None):
            raise ValueError("sched and round are given together or not at all")
        S, T = self._check_csr(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, torch.float32, D, sched, round)
        for name, t in (("ended", ended), ("ended_next", ended_next), ("saw", saw)):
            if t is not None:
                _check_tables((name, t, torch.int32))
                if t.numel() != D:
                    raise ValueError(f"{name} must hold one int32 flag per device")
        _lib.call("cfa_mix_population_ended_f32", out_ptrs.data_ptr(), src_ptrs.data_ptr(), csr_ptr.data_ptr(),
                  csr_idx.data_ptr(), csr_coef.data_ptr(), sched.data_ptr() if sched is not None else None, S, T,
                  round.data_ptr() if round is not None else None, ended.data_ptr(),
                  ended_next.data_ptr() if ended_next is not None else None,
                  saw.data_ptr() if saw is not None else None, int(ended_rule), int(D), int(P),
                  self.stream_handle(stream))

    def fedavg_round(self, models: torch.Tensor, params: torch.Tensor, act_ptr: torch.Tensor, act_idx: torch.Tensor,
                     act_div: torch.Tensor, act_rdiv: torch.Tensor, update_factor: float, sched: torch.Tensor,
                     round: torch.Tensor, ended: Optional[torch.Tensor] = None, client: int = _lib.CLIENT_COPY,
                     client_factor: float = 1.0, client_divisor: float = 1.0, stream=None) -> None:
        """cfa_fedavg_population_round_f32: one FedAvg parameter-server round on ``models`` [D, P]
        (fp32 CUDA, unit element stride, any row pitch) and the global model ``params`` [P], both
        in place. The round's active list is list ``sched[round % S]`` of the T lists in
        ``act_ptr`` [T + 1] / ``act_idx`` (int32 CUDA, ``topology.active_schedule``), with its
        divisor ``act_div`` [T] fp32 and reciprocal ``act_rdiv`` [T] fp64; ``round`` is left one
        higher in stream order. ``ended`` [D] int32 CUDA or None: the training_end flags.
        ``client``: _lib.CLIENT_NONE / CLIENT_COPY / CLIENT_MIX (w + client_factor * (g - w) /
        client_divisor). The library validates alignment and pitch (CFAError)."""
        D, P = _check_nd(models, "models", pitched=True)
        _check_bucket(params, "params", P)
        _check_tables(("act_ptr", act_ptr, torch.int32), ("act_idx", act_idx, torch.int32),
                      ("act_div", act_div, torch.float32), ("act_rdiv", act_rdiv, torch.float64),
                      ("sched", sched, torch.int32), ("round", round, torch.int64))
        if round.numel() != 1:
            raise TypeError("round must be a one-element int64 CUDA tensor")
        T = act_ptr.numel() - 1
        if T < 1 or act_div.numel() != T or act_rdiv.numel() != T or act_idx.numel() < 1:
            raise ValueError("act_ptr must hold T + 1 >= 2 offsets, act_div and act_rdiv T entries each, and "
                             "act_idx at least one entry")
        if ended is not None:
            _check_tables(("ended", ended, torch.int32))
            if ended.numel() != D:
                raise ValueError("ended must hold one int32 flag per device")
        cd = float(np.float32(client_divisor))
        _lib.call("cfa_fedavg_population_round_f32", models.data_ptr(), int(models.stride(0)) if D > 1 else P,
                  params.data_ptr(), act_ptr.data_ptr(), act_idx.data_ptr(), act_div.data_ptr(), act_rdiv.data_ptr(),
                  float(update_factor), sched.data_ptr(), sched.numel(), T, round.data_ptr(),
                  ended.data_ptr() if ended is not None else None, int(client), float(client_factor), cd,
                  1.0 / cd if cd else 0.0, D, P, self.stream_handle(stream))

    def cfa_fa_round(self, out: torch.Tensor, models: torch.Tensor, server: torch.Tensor, coef: torch.Tensor,
                     eps2: float, mode: int = _lib.FA_ROUND, stream=None) -> None:
        """cfa_fa_population_round_f32: one server epoch of the TF1 CFA-FA driver. ``models``
        [D, P] (fp32 CUDA, unit element stride, any row pitch): the models the devices published,
        only read; ``out`` [D, P] likewise: every device's model after the epoch (must not overlap
        ``models``); ``server`` [P] fp64 CUDA: the server model, folded in place; ``coef`` [D] fp64
        CUDA: ``b_d`` under ``_lib.FA_INIT``, ``eps * b_d`` under ``_lib.FA_ROUND``. The library
        validates pitches and the overlap (CFAError)."""
        D, P = _check_nd(models, "models", pitched=True)
        if _check_nd(out, "out", pitched=True) != (D, P):
            raise ValueError(f"out must be [{D}, {P}] like models")
        _check_bucket(server, "server", P, torch.float64)
        _check_tables(("coef", coef, torch.float64))
        if coef.numel() != D:
            raise ValueError("coef must hold one fp64 coefficient per device")
        if mode not in (_lib.FA_INIT, _lib.FA_ROUND):
            raise ValueError("mode must be _lib.FA_INIT or _lib.FA_ROUND")
        _lib.call("cfa_fa_population_round_f32", out.data_ptr(), int(out.stride(0)) if D > 1 else P,
                  models.data_ptr(), int(models.stride(0)) if D > 1 else P, server.data_ptr(), coef.data_ptr(),
                  float(eps2), int(mode), D, P, self.stream_handle(stream))


_engines: dict = {}


for _name, _fn in list(vars(Engine).items()):
    if (callable(_fn) and not isinstance(_fn, (staticmethod, classmethod)) and not _name.startswith("_")
            and _name not in ("empty", "counter", "stream_handle", "grad_workspace", "grad_splits", "optim_tile",
                              "optim_workspace", "lenet_params", "lenet_workspace", "lenet_grad_workspace")):
        setattr(Engine, _name, _same_device(_fn))


def get_engine(device=None) -> Engine:
    """Process-wide engine per device (the engine object itself holds no mutable state)."""
    dev = _require_gpu(device)
    eng = _engines.get(dev.index)
    if eng is None:
        eng = _engines[dev.index] = Engine(dev)
    return eng
