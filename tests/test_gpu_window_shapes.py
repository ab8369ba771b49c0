"""Every launch shape of the window pass (cfa_mix_window_f32) and the one-launch ring round
(cfa_mix_ring_round_f32): one and two float4 per lane, nontemporal and sc1 write-through stores,
reached through CFA_WINDOW_VEC / CFA_WINDOW_SC1. Each must give the per-device numpy fp32 fold
(the sequential-mix oracle) bit for bit."""
import numpy as np
import pytest
import torch

from oracle.cfa_oracle import sequential_mix

pytestmark = pytest.mark.gpu

WINDOWS = [(4, 4), (1, 0), (0, 2)]
SHAPES = [(vec, sc1) for vec in (1, 2) for sc1 in (0, 1)]

_cache = {}


def _alphas(n):
    return [0.5 / (d + 2) for d in range(n)]  # distinct per device, so an index slip shows


def _rows(n, P):
    """Seeded random rows [n, P], computed once per shape and left unchanged."""
    if (n, P) not in _cache:
        h = np.random.default_rng(n * 100003 + P).standard_normal((n, P)).astype(np.float32)
        h.setflags(write=False)
        _cache[n, P] = h
    return _cache[n, P]


def _fold(h, local, nbrs, a):
    key = (h.shape, local, tuple(nbrs), a)
    if key not in _cache:
        ref = sequential_mix(h[local], [h[j] for j in nbrs], [a] * len(nbrs))
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(params=SHAPES, ids=lambda s: "vec%d-sc1_%d" % s)
def shape(request, monkeypatch):
    vec, sc1 = request.param
    monkeypatch.setenv("CFA_WINDOW_VEC", str(vec))
    monkeypatch.setenv("CFA_WINDOW_SC1", str(sc1))
    monkeypatch.setenv("CFA_WINDOW_BLOCKS_PER_CU", "1")
    return request.param


# 6164 = 1541 float4: three full 512-vector tiles at two float4 per lane and a partial tile of 5;
# 6167 adds the 3-element scalar tail
@pytest.mark.parametrize("P", [6164, 6167])
@pytest.mark.parametrize("hl,hr", WINDOWS)
@pytest.mark.parametrize("nb", [1, 3, 8])
def test_window_pass_equals_numpy_fold(gpu, shape, nb, hl, hr, P):
    h = _rows(nb + hl + hr, P)
    al = _alphas(nb)
    rows = [torch.tensor(r).cuda() for r in h]  # one allocation per row: each 16-byte aligned
    outs = [torch.full((P,), float("nan"), device="cuda") for _ in range(nb)]
    gpu.mix_window(outs, rows, [[a] * (hl + hr) for a in al], hl, hr)
    torch.cuda.synchronize()
    for b in range(nb):
        nbrs = list(range(b, b + hl)) + list(range(b + hl + 1, b + hl + 1 + hr))
        np.testing.assert_array_equal(_bits(outs[b].cpu().numpy()), _bits(_fold(h, b + hl, nbrs, al[b])), str(b))


# two passes each: the second holds 1 and 5 devices
@pytest.mark.parametrize("hl,hr", WINDOWS)
@pytest.mark.parametrize("D", [9, 13])
def test_ring_round_equals_numpy_fold(gpu, shape, D, hl, hr):
    P = 6164
    h = _rows(D, P)
    al = _alphas(D)
    out = torch.full((D, P), float("nan"), device="cuda")
    gpu.ring_round(out, torch.tensor(h).cuda(), torch.tensor(al, dtype=torch.float32, device="cuda"), hl, hr)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for d in range(D):
        nbrs = [(d + o) % D for o in list(range(-hl, 0)) + list(range(1, hr + 1))]
        np.testing.assert_array_equal(_bits(got[d]), _bits(_fold(h, d, nbrs, al[d])), str(d))
