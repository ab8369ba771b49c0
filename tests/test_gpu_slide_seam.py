"""The seam-retaining walk of the sliding ring round (cfa_mix_ring_slide_f32 on a full ring in one
segment: the stream's last hl + hr rows are the lane's retained copies of its first ones, not
loads). Every case runs with CFA_SLIDE_SEAM forced to 1 and to 0 at both tile widths that have a
seam kernel (CFA_SLIDE_U = 2, 4) and must give the per-device numpy fp32 fold (the sequential-mix
oracle) bit for bit, on stacks of differing pitches whose padding and unreached rows are NaN on
the input side and a sentinel on the output side."""
import numpy as np
import pytest
import torch

from oracle.cfa_oracle import sequential_mix

pytestmark = pytest.mark.gpu

SLIDE_ENV = ("CFA_SLIDE_SEGMENTS", "CFA_SLIDE_PF", "CFA_SLIDE_WG_PER_CU", "CFA_SLIDE_SC1", "CFA_SLIDE_U",
             "CFA_SLIDE_SEAM")
WIDTHS = [2, 4]
SEAM = [1, 0]
P_SMALL = 4 * (1024 + 256 + 3)  # two tiles at U = 4, the last with a full, a partial and two empty stripes

_cache = {}


def _alpha(d):
    return 0.5 / (d + 2)  # distinct per device, so an index slip shows


def _window(d, rows, hl, hr):
    return [(d + o) % rows for o in list(range(-hl, 0)) + list(range(1, hr + 1))]


def _case(rows, first, count, hl, hr, P):
    """(host rows, oracle rows of the run's devices), computed once per case and left unchanged."""
    key = (rows, first, count, hl, hr, P)
    if key not in _cache:
        h = np.random.default_rng(rows * 100019 + P * 11 + 10 * hl + hr).standard_normal((rows, P)).astype(np.float32)
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


# The seam kernel's register ring holds RS = hl + hr + 2 rows (10 at 4/4), the plain default's 11:
# streams shorter than, equal to and longer than either ring, so priming and tail overlap.
@pytest.mark.parametrize("rows", [9, 10, 11, 12, 23, 25])
@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_full_rings_around_the_register_ring(gpu, slide_env, seam, u, rows):
    slide_env(seam=seam, u=u)
    _check(gpu, rows, 0, rows, 4, 4, P_SMALL)


@pytest.mark.parametrize("hl,hr", [(4, 0), (0, 4), (1, 0), (0, 1), (2, 3)])
@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_one_sided_and_narrow_windows(gpu, slide_env, seam, u, hl, hr):
    slide_env(seam=seam, u=u)
    _check(gpu, 13, 0, 13, hl, hr, P_SMALL)


@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_full_ring_from_a_later_first_device(gpu, slide_env, seam, u):
    """first = 3, count == rows: the input and the output pointers wrap mid-walk."""
    slide_env(seam=seam, u=u)
    _check(gpu, 13, 3, 13, 4, 4, P_SMALL)


@pytest.mark.parametrize("shape", ["one", "255", "tile+1", "3tiles-1"])
@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_row_lengths_at_the_tile_edges(gpu, slide_env, seam, u, shape):
    """One vector; a partial first stripe; a tile and one vector (stripes wholly past the end);
    three tiles less one vector (a lane without its last vector)."""
    P = {"one": 4, "255": 4 * 255, "tile+1": 4 * 256 * u + 4, "3tiles-1": 4 * (3 * 256 * u - 1)}[shape]
    slide_env(seam=seam, u=u)
    _check(gpu, 11, 0, 11, 4, 4, P)


@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_more_tiles_than_workgroups(gpu, slide_env, seam, u):
    """One workgroup per CU and three tiles more than CUs: a workgroup primes and retains again for
    a second column tile, where stale retained rows of its first would show."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slide_env(seam=seam, u=u, wg_per_cu=1)
    _check(gpu, 10, 0, 10, 4, 4, 4 * 256 * u * (cus + 3))


@pytest.mark.parametrize("u", WIDTHS)
@pytest.mark.parametrize("seam", SEAM)
def test_partial_run_and_two_segments_take_the_plain_walk(gpu, slide_env, seam, u):
    """count = rows - 1, and a full ring in two segments: no seam to retain, whatever is forced."""
    slide_env(seam=seam, u=u)
    _check(gpu, 13, 0, 12, 4, 4, P_SMALL)
    _check(gpu, 13, 1, 12, 4, 4, P_SMALL)
    slide_env(seam=seam, u=u, segments=2)
    _check(gpu, 13, 0, 13, 4, 4, P_SMALL)
    _check(gpu, 13, 3, 13, 4, 4, P_SMALL)
