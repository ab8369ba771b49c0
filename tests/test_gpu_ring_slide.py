"""cfa_mix_ring_slide_f32 (a run of consecutive ring devices, every row read once through a
sliding register window) against the sequential-mix oracle, bit for bit: whole rings with
wrap-around, sub-runs with differing pitches, every launch shape, and the error returns."""
import numpy as np
import pytest
import torch

from oracle.cfa_oracle import sequential_mix

pytestmark = pytest.mark.gpu

# (rows, hl, hr, P) mixed on the whole ring
CASES = [
    (9, 4, 4, 1028),        # every row is everyone's neighbour, wrap on both sides
    (13, 4, 4, 24624),
    (12, 2, 2, 4100),
    (10, 1, 0, 4096),
    (7, 0, 2, 1028),
    (5, 0, 0, 260),         # a pure copy
    (128, 4, 4, 4096),      # the bench's device count
    (9, 4, 4, 4),           # less than one tile
    (9, 4, 4, 2_000_148),   # more tiles than the grid cap: the grid-stride loop iterates
]
SLIDE_ENV = ("CFA_SLIDE_SEGMENTS", "CFA_SLIDE_PF", "CFA_SLIDE_WG_PER_CU", "CFA_SLIDE_SC1")

_cache = {}


def _alphas(n):
    return [0.5 / (d + 2) for d in range(n)]  # distinct per device, so an index slip shows


def _window(d, rows, hl, hr):
    return [(d + o) % rows for o in list(range(-hl, 0)) + list(range(1, hr + 1))]


def _case(rows, hl, hr, P):
    """(host models, per-device alphas, oracle of the whole ring), computed once per shape."""
    key = (rows, hl, hr, P)
    if key not in _cache:
        rng = np.random.default_rng(rows * 100003 + P * 7 + 10 * hl + hr)
        h = rng.standard_normal((rows, P)).astype(np.float32)
        al = _alphas(rows)
        ref = np.stack([sequential_mix(h[d], [h[j] for j in _window(d, rows, hl, hr)], [al[d]] * (hl + hr))
                        for d in range(rows)])
        h.setflags(write=False)
        ref.setflags(write=False)
        _cache[key] = (h, al, ref)
    return _cache[key]


def _slide_whole(gpu, rows, hl, hr, P):
    h, al, _ = _case(rows, hl, hr, P)
    models = torch.tensor(h).cuda()
    out = torch.full((rows, P), float("nan"), device="cuda")
    gpu.ring_slide(out, models, torch.tensor(al, dtype=torch.float32, device="cuda"), 0, rows, hl, hr)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture
def clean_env(monkeypatch):
    for k in SLIDE_ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("rows,hl,hr,P", CASES)
def test_whole_ring_equals_oracle(gpu, clean_env, rows, hl, hr, P):
    got = _slide_whole(gpu, rows, hl, hr, P)
    ref = _case(rows, hl, hr, P)[2]
    for d in range(rows):
        assert np.array_equal(got[d], ref[d]), d


@pytest.mark.parametrize("first", [0, 5, 12])
def test_whole_ring_from_any_first_device(gpu, clean_env, first):
    """count == rows with first > 0: the run passes the last row and wraps."""
    rows, hl, hr, P = 13, 4, 4, 24624
    h, al, ref = _case(rows, hl, hr, P)
    out = torch.full((rows, P), float("nan"), device="cuda")
    run_al = [al[(first + n) % rows] for n in range(rows)]
    gpu.ring_slide(out, torch.tensor(h).cuda(), torch.tensor(run_al, dtype=torch.float32, device="cuda"),
                   first, rows, hl, hr)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("rows,hl,hr,P", [(13, 4, 4, 24624), (12, 2, 2, 4100), (10, 1, 0, 4096), (7, 0, 2, 1028)])
def test_sub_run_reads_and_writes_only_its_rows(gpu, clean_env, rows, hl, hr, P):
    """first = hl, count = rows - hl - hr (no wrap): what the run must not read is NaN, the output
    rows outside the run keep their sentinel, and the pitches differ (in P + 8, out P + 20). The
    run reads rows 0 .. rows-1, so it runs twice: on a stack of exactly those rows (only the
    pitch padding is NaN) and on a stack three rows taller whose extra rows are NaN."""
    h, al, ref = _case(rows, hl, hr, P)
    first, count = hl, rows - hl - hr
    inbuf = torch.full((rows, P + 8), float("nan"), device="cuda")
    outbuf = torch.full((rows, P + 20), -7.0, device="cuda")
    models, out = inbuf[:, :P], outbuf[:, :P]
    models.copy_(torch.tensor(h))
    big_in = torch.full((rows + 3, P + 8), float("nan"), device="cuda")
    big_in[:rows, :P].copy_(torch.tensor(h))
    big_out = torch.full((rows + 3, P + 20), -7.0, device="cuda")
    run_al = torch.tensor(al[first:first + count], dtype=torch.float32, device="cuda")
    gpu.ring_slide(big_out[:, :P], big_in[:, :P], run_al, first, count, hl, hr)
    gpu.ring_slide(out, models, run_al, first, count, hl, hr)
    torch.cuda.synchronize()
    for got in (out.cpu().numpy(), big_out[:rows, :P].cpu().numpy()):
        for d in range(rows):
            if first <= d < first + count:
                assert np.array_equal(got[d], ref[d]), d
            else:
                assert (got[d] == -7.0).all(), d
    assert (big_out[rows:].cpu().numpy() == -7.0).all()
    assert (outbuf[:, P:].cpu().numpy() == -7.0).all() and (big_out[:, P:].cpu().numpy() == -7.0).all()


@pytest.mark.parametrize("segments", [1, 2, 4, 40])
@pytest.mark.parametrize("pf", [1, 2, 3, 4])
def test_every_launch_shape_is_bit_identical(gpu, clean_env, segments, pf):
    """Segment counts 1, 2, 4 (13 devices in 4 segments: not a divisor) and one above the device
    count, at every prefetch depth, with both store policies and two grid caps."""
    clean_env.setenv("CFA_SLIDE_SEGMENTS", str(segments))
    clean_env.setenv("CFA_SLIDE_PF", str(pf))
    for rows, hl, hr, P in [(13, 4, 4, 24624), (12, 2, 2, 4100), (10, 1, 0, 4096), (7, 0, 2, 1028), (5, 0, 0, 260)]:
        ref = _case(rows, hl, hr, P)[2]
        for sc1, wg in ((0, 8), (1, 1)):
            clean_env.setenv("CFA_SLIDE_SC1", str(sc1))
            clean_env.setenv("CFA_SLIDE_WG_PER_CU", str(wg))
            assert np.array_equal(_slide_whole(gpu, rows, hl, hr, P), ref), (rows, hl, hr, P, sc1, wg)


def test_error_returns_leave_out_unchanged(gpu, clean_env):
    from federated_amd import _lib
    rows, P = 8, 1024
    models = torch.randn(rows, P, device="cuda")
    out = torch.full((rows, P), 3.0, device="cuda")
    al = torch.full((rows,), 0.25, device="cuda")
    st = gpu.stream_handle(None)

    def raw(o=None, op=P, i=None, ip=P, a=None, r=rows, first=0, count=rows, hl=1, hr=1, p=P):
        _lib.call("cfa_mix_ring_slide_f32", out.data_ptr() if o is None else o, op,
                  models.data_ptr() if i is None else i, ip, al.data_ptr() if a is None else a,
                  r, first, count, hl, hr, p, st)

    invalid = [dict(o=0), dict(i=0), dict(a=0), dict(count=0), dict(count=-2), dict(first=-1), dict(first=rows),
               dict(count=rows + 1), dict(first=3, count=6), dict(hl=5), dict(hr=5), dict(hl=-1), dict(hr=-1),
               dict(hl=4, hr=4), dict(op=P - 4), dict(ip=P - 4), dict(o=models.data_ptr()),
               dict(o=models.data_ptr() + 4 * P * (rows - 1))]
    for kw in invalid:
        with pytest.raises(_lib.CFAError) as e:
            raw(**kw)
        assert e.value.code == _lib.CFA_E_INVALID, kw
    wide = torch.full((rows, P + 2), 3.0, device="cuda")
    unsupported = [dict(o=out.data_ptr() + 4, r=rows - 1, count=rows - 1), dict(i=models.data_ptr() + 4, r=rows - 1,
                                                                                count=rows - 1),
                   dict(p=P - 2), dict(o=wide.data_ptr(), op=P + 2), dict(i=wide.data_ptr(), ip=P + 2)]
    for kw in unsupported:
        with pytest.raises(_lib.CFAError) as e:
            raw(**kw)
        assert e.value.code == _lib.CFA_E_UNSUPPORTED, kw
    raw(p=0)  # nothing to mix: OK, nothing written
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 3.0).all() and (wide.cpu().numpy() == 3.0).all()
    # the engine wrapper raises the same errors
    with pytest.raises(_lib.CFAError, match="overlaps"):
        gpu.ring_slide(models, models, al, 0, rows, 1, 1)
    with pytest.raises(_lib.CFAError, match="16-byte"):
        gpu.ring_slide(torch.zeros(4, 1002, device="cuda"), torch.zeros(4, 1002, device="cuda"), al, 0, 4, 1, 1)
