"""Every column-tile width of the sliding ring round (cfa_mix_ring_slide_f32): one, two and four
float4 per lane and row (CFA_SLIDE_U) at one and four workgroups per CU (CFA_SLIDE_WG_PER_CU), on
rows whose last tile has full, partial and empty stripes. Each must give the per-device numpy fp32
fold (the sequential-mix oracle) bit for bit, read nothing outside the window's rows and write
nothing outside the run's P elements."""
import numpy as np
import pytest
import torch

from oracle.cfa_oracle import sequential_mix

pytestmark = pytest.mark.gpu

SLIDE_ENV = ("CFA_SLIDE_SEGMENTS", "CFA_SLIDE_PF", "CFA_SLIDE_WG_PER_CU", "CFA_SLIDE_SC1", "CFA_SLIDE_U")

# P in floats. At four float4 per lane a tile is 1024 float4 in four stripes of 256:
P_STRIPES = 4 * (1024 + 256 + 3)  # the last tile: one stripe full, one of 3 vectors, two empty
P_LONE = 4 * 3                    # a lone partial first stripe
P_EXACT = 4 * 2048                # whole tiles at every width
P_STRIDE = 4 * (1024 * 257 + 5)   # more four-wide tiles (258) than CUs: at one workgroup per CU
                                  # the grid-stride loop iterates, then a partial tile

# (rows, first, count, hl, hr, P): each ring and each window once, every P at every width
CASES = [
    (13, 0, 13, 4, 4, P_STRIPES),  # the whole ring: the window wraps at both ends
    (13, 5, 2, 4, 4, P_LONE),      # a run shorter than the register ring
    (16, 2, 12, 4, 4, P_EXACT),    # a run that is no multiple of W + PF
    (13, 0, 13, 0, 4, P_EXACT),
    (16, 2, 12, 4, 0, P_STRIPES),
    (13, 5, 2, 1, 2, P_STRIPES),
]

_cache = {}


def _alpha(d):
    return 0.5 / (d + 2)  # distinct per device, so an index slip shows


def _window(d, rows, hl, hr):
    return [(d + o) % rows for o in list(range(-hl, 0)) + list(range(1, hr + 1))]


def _case(rows, first, count, hl, hr, P):
    """(host rows, oracle rows of the run's devices), computed once per case and left unchanged."""
    key = (rows, first, count, hl, hr, P)
    if key not in _cache:
        h = np.random.default_rng(rows * 100003 + P * 7 + 10 * hl + hr).standard_normal((rows, P)).astype(np.float32)
        ref = {}
        for n in range(count):
            d = (first + n) % rows
            ref[d] = sequential_mix(h[d], [h[j] for j in _window(d, rows, hl, hr)], [_alpha(d)] * (hl + hr))
            ref[d].setflags(write=False)
        h.setflags(write=False)
        _cache[key] = (h, ref)
    return _cache[key]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check(gpu, rows, first, count, hl, hr, P):
    """One call on stacks with differing pitches (in P + 8, out P + 20): rows the run's windows do
    not reach and the pitch padding are NaN, the output starts as a sentinel."""
    h, ref = _case(rows, first, count, hl, hr, P)
    run = [(first + n) % rows for n in range(count)]
    read = set(run) | {j for d in run for j in _window(d, rows, hl, hr)}
    inbuf = torch.full((rows, P + 8), float("nan"), device="cuda")
    for d in read:
        inbuf[d, :P].copy_(torch.tensor(h[d]))
    outbuf = torch.full((rows, P + 20), -7.0, device="cuda")
    al = torch.tensor([_alpha(d) for d in run], dtype=torch.float32, device="cuda")
    gpu.ring_slide(outbuf[:, :P], inbuf[:, :P], al, first, count, hl, hr)
    torch.cuda.synchronize()
    got = outbuf.cpu().numpy()
    for d in range(rows):
        if d in ref:
            np.testing.assert_array_equal(_bits(got[d, :P]), _bits(ref[d]), str(d))
        else:
            assert (got[d, :P] == -7.0).all(), d
    assert (got[:, P:] == -7.0).all()


@pytest.fixture
def slide_env(monkeypatch):
    """Sets the slide overrides of one case; monkeypatch restores the environment after it."""
    for k in SLIDE_ENV:
        monkeypatch.delenv(k, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setenv("CFA_SLIDE_" + k.upper(), str(v))
    return set_


@pytest.mark.parametrize("rows,first,count,hl,hr,P", CASES)
@pytest.mark.parametrize("wg", [1, 4])
@pytest.mark.parametrize("u", [1, 2, 4])
def test_every_tile_width_equals_numpy_fold(gpu, slide_env, u, wg, rows, first, count, hl, hr, P):
    slide_env(u=u, wg_per_cu=wg)
    _check(gpu, rows, first, count, hl, hr, P)


@pytest.mark.parametrize("u", [1, 2, 4])
def test_segment_halos_at_every_tile_width(gpu, slide_env, u):
    """13 devices in 3 segments (5, 5, 3): every segment re-reads its halo rows into wide slots."""
    slide_env(u=u, segments=3)
    _check(gpu, 13, 0, 13, 4, 4, P_STRIPES)


@pytest.mark.parametrize("u", [2, 4])
def test_wide_tiles_stride_over_the_grid(gpu, slide_env, u):
    slide_env(u=u, wg_per_cu=1)
    _check(gpu, 9, 0, 9, 4, 4, P_STRIDE)


def test_invalid_tile_width_falls_back_to_the_default(gpu, slide_env):
    for bad in ("3", "0", "-4", "8", "wide"):
        slide_env(u=bad)
        _check(gpu, 13, 0, 13, 4, 4, P_STRIPES)
