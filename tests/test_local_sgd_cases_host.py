"""The cases of tests/local_sgd_cases.py, checked without a GPU: what tests/test_gpu_local_sgd_paths.py
relies on before it launches holds from the mirror of the launch plan and the float64 reference
alone -- the condition that puts each case on its path, the spread ``s`` of the allowance, the
margin guard over the whole trajectory, and what the built cases were built for."""
import pytest

import local_sgd_cases as lc


def test_mirror_of_the_launch_plan():
    """The mirror against figures worked out by hand from cfa_local_sgd.hip."""
    assert [lc.softmax_width(C) for C in (1, 2, 3, 8, 10, 33, 64)] == [1, 2, 4, 8, 16, 64, 64]
    assert lc.taps_in_regs(16, 8) and lc.taps_in_regs(32, 2) and not lc.taps_in_regs(33, 4) and not lc.taps_in_regs(16, 6)
    c3 = lc.plan(1, lc._cnn(16, 5, 8, 512, 8))  # the CFA-GE CNN: L1 103, L2 21, P 1 488, 1 689 floats per sample
    assert (c3.L1, c3.L2, c3.LN, c3.pl, c3.ql, c3.P) == (103, 21, 168, 7, 1, 1488)  # pl = (102 * 5 + 16 - 512) / 2
    assert lc.cnn_sgd_lds(c3, 4) == 1488 + 4 * 1689
    c1 = lc.plan(2, lc._nn(512, 32, 8))  # the 2NN: G 16, P 16 680, 1 625 floats per sample
    assert (c1.G, c1.P) == (16, 16680) and lc.nn_sgd_lds(c1, 4) == 16680 + 4 * (2 * 520 + 64 + 8 + 512 + 1)
    assert (lc.K_BLOCK, lc.K_PRE_X, lc.K_PRE_Y, lc.K_MAX_TAPS, lc.K_SPAN) == (512, 8, 2, 32, 32)


@pytest.mark.parametrize("name", list(lc.TABLE))
def test_table_case(name):
    """Path conditions from the mirror, s < 1e-4, and the margin guard on the float64 reference."""
    c = lc.TABLE[name]
    assert c.D == 2 and c.build is None
    lc.assert_path(c)
    lc.assert_guarded(c)
    ref = lc.reference(c)
    print(f"{name}: margin {lc.margin(c):.2e}, s {ref['s']:.2e}, LDS {c.lds} B")
    assert all(a == 1e-5 for dev in ref["allow"] for a in dev)  # 4 * s < 1e-5: the standing bar throughout


def test_table_covers_the_listed_paths():
    """Across the table: both store tails in each kernel family, both CNN instantiations with and
    without register taps, softmax widths 2 to 64, and the raised LDS limit in a CNN launch."""
    T = lc.TABLE
    assert {c.plan.SW for c in T.values()} >= {2, 4, 8, 16, 64}
    assert {(c.plan.fast, c.plan.taps_in_regs) for c in T.values() if c.ml == 1} == {(True, True), (True, False),
                                                                                     (False, True), (False, False)}
    for ml in (1, 2):
        assert any(c.rows * c.plan.L > lc.K_PRE_X * lc.K_BLOCK for c in T.values() if c.ml == ml)
    assert any(c.ml == 1 and c.lds > lc.LDS_DEFAULT for c in T.values())
    assert all(c.lds <= 66756 for c in T.values())


@pytest.mark.parametrize("ml", [1, 2])
def test_clip_above_construction(ml):
    effect = lc.assert_clip_above(lc.CLIP_ABOVE[ml])
    print(f"clip above ml={ml}: an open gate moves W1 b1 W2 b2 by", " ".join(f"{v:.2e}" for v in effect))


@pytest.mark.parametrize("ml", [1, 2])
def test_clip_below_construction(ml):
    lc.assert_clip_below(lc.CLIP_BELOW[ml])


@pytest.mark.parametrize("ml", [1, 2])
def test_one_class_construction(ml):
    lc.assert_one_class(lc.ONE_CLASS[ml])


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_tie_construction(fast):
    c, ties, zero = lc.TIES[fast]
    assert c.plan.fast == fast and (c.plan.taps_in_regs or not fast) and c.steps == 1
    lc.assert_tie(c, ties, zero)


@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_dead_relu_construction(fast):
    c = lc.DEAD[fast]
    assert c.plan.fast == fast
    lc.assert_dead(c)


def test_many_devices_case():
    c = lc.MANY
    assert c.D == 300 > 256 and c.steps == 1  # more workgroups than the card has compute units
    lc.assert_guarded(c)
    assert all(a == 1e-5 for dev in lc.reference(c)["allow"] for a in dev)
    print(f"D=300: margin {lc.margin(c):.2e}, s {lc.reference(c)['s']:.2e}")


def test_refused_launches_are_refused_from_the_mirror():
    for ml, geom, rows in lc.TOO_MUCH_LDS:
        assert lc.lds_bytes(ml, geom, rows) > lc.LDS_DEVICE
        assert lc.lds_bytes(ml, geom, 4) <= lc.LDS_DEFAULT  # the geometry itself is an ordinary one
