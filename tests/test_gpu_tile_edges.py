"""The edges of the shared tile walk (cfa_internal.h TileWalk: full tiles of kBlock * U vectors
grid-stride, the partial tile by workgroup `full % grid`), for each kernel that uses it, bit for
bit against numpy at three sizes derived from the kernel's tile and its launch's grid:
  (a) less than one full tile, with a ragged scalar tail (only the partial-tile loop runs);
  (b) three full tiles plus a partial one (the partial tile's owner is workgroup 3, not 0);
  (c) three more full tiles than the grid has workgroups, plus a partial one (workgroups 0..2
      walk two tiles, the owner is workgroup 3).
The larger suites reach some of these ((c) for the epilogue and fold_f64 at 4M elements); here
every kernel meets all three, at no more than 9 MB a bucket."""
import numpy as np
import pytest
import torch

from oracle import cfa_oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 256  # kBlock


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sizes(tile_vecs, width, grid):
    """Element counts of the three regimes for tiles of tile_vecs vectors of `width` elements."""
    ragged = width - 1
    return [width * (tile_vecs - 5) + ragged,
            width * (3 * tile_vecs + tile_vecs // 2 + 3) + ragged,
            width * ((grid + 3) * tile_vecs + 77) + ragged]


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("vec", [1, 2, 4])
def test_mix_seq_tile_edges(gpu, cus, vec):
    """cfa_mix_seq_ex_f32 at one workgroup per CU and `vec` float4 per lane: the grid is the CU
    count, so 259 tiles at vec = 4 on 256 CUs exceed it."""
    n = 3
    rng = np.random.default_rng(2100 + vec)
    for P in _sizes(BLOCK * vec, 4, cus):
        local = rng.standard_normal(P).astype(np.float32)
        nbrs = [rng.standard_normal(P).astype(np.float32) for _ in range(n)]
        alphas = [0.3, 0.25, 0.2]
        out = torch.empty(P, dtype=torch.float32, device="cuda")
        gpu.mix_seq(out, _dev(local), [_dev(x) for x in nbrs], alphas, launch=(1, vec, 1))
        assert np.array_equal(out.cpu().numpy(), O.sequential_mix(local, nbrs, alphas)), (vec, P)


@pytest.mark.parametrize("mode", [1, 2])
def test_compress_epilogue_tile_edges(gpu, cus, mode):
    """The standalone epilogue (four float4 per lane, two workgroups per CU), sparse and DPCM."""
    rng = np.random.default_rng(2200 + mode)
    for P in _sizes(BLOCK * 4, 4, 2 * cus):
        ref = (rng.standard_normal(P) * 1e-2).astype(np.float32)
        y = (ref + rng.standard_normal(P).astype(np.float32) * np.float32(2e-4)) if mode == 2 else \
            (rng.standard_normal(P) * 1e-3).astype(np.float32)
        expect = y.copy().reshape(1, -1)
        cnt = O.tf1_compress(expect, (ref if mode == 2 else y).reshape(1, -1), mode)
        dy = _dev(y)
        kept = gpu.counter()
        gpu.compress(dy, _dev(ref) if mode == 2 else None, mode, kept)
        assert np.array_equal(dy.cpu().numpy(), expect.reshape(-1)), (mode, P)
        assert int(kept.item()) == cnt and 0 < cnt < P, (mode, P)


def _tf1_case(rng, P, n):
    local = (rng.standard_normal(P) * 1e-2).astype(np.float32)
    nbrs = [local + (rng.standard_normal(P) * 1e-3).astype(np.float32) for _ in range(n)]
    alphas = [0.7 * O.tf1_weight_factor(8, 1, j % 8, n - 1) for j in range(n)]
    return local, nbrs, alphas, O.tf1_mix_flat(local, nbrs, alphas)


def test_mix_tf1_f32_tile_edges(gpu, cus):
    """cfa_mix_tf1_f32: two float4 per lane at two workgroups per CU."""
    rng = np.random.default_rng(2300)
    for P in _sizes(BLOCK * 2, 4, 2 * cus):
        local, nbrs, alphas, ref = _tf1_case(rng, P, 3)
        out = torch.empty(P, dtype=torch.float32, device="cuda")
        gpu.mix_tf1(out, _dev(local), [_dev(x) for x in nbrs], alphas)
        assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32)), P


def test_mix_tf1_wide_tile_edges(gpu, cus):
    """cfa_mix_tf1_wide_f32 (unrounded fp64 out): four float2 per lane at one workgroup per CU; the
    host counts the body in float4, so the ragged tail is up to three elements."""
    from federated_amd import _lib
    rng = np.random.default_rng(2400)
    for P in [p + 2 for p in _sizes(BLOCK * 4, 2, cus)]:
        local, nbrs, alphas, ref = _tf1_case(rng, P, 3)
        out = torch.full((P,), float("nan"), dtype=torch.float64, device="cuda")
        dl, dn = _dev(local), [_dev(x) for x in nbrs]
        _lib.call("cfa_mix_tf1_wide_f32", out.data_ptr(), dl.data_ptr(), _lib.ptr_table([x.data_ptr() for x in dn]),
                  _lib.double_array(alphas), len(dn), P, 0, 0, 0, None, gpu.stream_handle())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref), P


@pytest.mark.parametrize("rule", [0, 2])
def test_fold_f64_tile_edges(gpu, cus, rule):
    """cfa_fold_f64: two double2 per lane at two workgroups per CU, the odd last element apart."""
    rng = np.random.default_rng(2500 + rule)
    n, a, d = 3, [0.2, 0.3, 0.25], [4.0, 3.0, 7.0]
    for P in _sizes(BLOCK * 2, 2, 2 * cus):
        local = rng.standard_normal(P)
        xs = [rng.standard_normal(P) for _ in range(n)]
        ref = local.copy()
        for j in range(n):
            ref = ref + a[j] * (xs[j] - ref) / d[j] if rule == 2 else ref + a[j] * (xs[j] - ref)
        out = torch.empty(P, dtype=torch.float64, device="cuda")
        gpu.fold_f64(out, _dev(local), [_dev(x) for x in xs], a, rule, d if rule == 2 else None)
        assert np.array_equal(out.cpu().numpy(), ref), (rule, P)
