"""cfa_mix_population_ended_f32 and the host half of ``PopulationRound``'s training_end rule,
without a GPU: the entry refuses bad arguments on the host, before any device work, and the rule
names and device ids are checked before anything is uploaded."""
import ctypes

import numpy as np
import pytest

FAKE = 1 << 20  # a non-null "device pointer": validation never dereferences it
GAP = 1 << 20   # between the three flag arrays: more than the 65 536 flags of the largest D tried
ENDED = FAKE + GAP


def _call(**over):
    """The entry with well-formed arguments (static form, D = 2, P = 16), ``over`` replacing some."""
    from federated_amd import _lib
    a = dict(out_ptrs=FAKE, src_ptrs=FAKE, csr_ptr=FAKE, csr_idx=FAKE, csr_coef=FAKE, sched=None, S=0, T=0,
             round=None, ended=ENDED, ended_next=ENDED + GAP, saw=ENDED + 2 * GAP, ended_rule=_lib.ENDED_COPY,
             D=2, P=16, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    _lib.call("cfa_mix_population_ended_f32", *a.values())


@pytest.mark.parametrize("over,message", [
    (dict(ended_rule=3), "unknown ended rule 3"),
    (dict(ended_rule=-1), "unknown ended rule -1"),
    (dict(ended=None), "null ended flags"),
    (dict(ended_next=ENDED), "ended_next or saw aliases ended"),
    (dict(saw=ENDED), "ended_next or saw aliases ended"),
    (dict(saw=ENDED + 4), "ended_next or saw aliases ended"),  # overlaps the second flag
    (dict(out_ptrs=None), "null population table"),
    (dict(src_ptrs=None), "null population table"),
    (dict(csr_ptr=None), "null population table"),
    (dict(csr_idx=None), "null population table"),
    (dict(csr_coef=None), "null population table"),
    (dict(D=-1), "negative device count"),
    (dict(D=65536), "exceeds grid.y limit"),
    (dict(sched=FAKE, S=1, T=1), "null schedule or round counter"),
    (dict(round=FAKE, S=1, T=1), "null schedule or round counter"),
    (dict(sched=FAKE, round=FAKE, S=0, T=1), "schedule of 0 slots over 1 tables"),
    (dict(sched=FAKE, round=FAKE, S=1, T=0), "schedule of 1 slots over 0 tables"),
])
def test_entry_refuses_bad_arguments_before_any_device_work(over, message):
    from federated_amd import _lib
    with pytest.raises(_lib.CFAError, match=message) as err:
        _call(**over)
    assert err.value.code == _lib.CFA_E_INVALID


def test_empty_population_is_ok_and_leaves_the_counter():
    """D == 0 or P == 0 returns CFA_OK without a launch; a scheduled call does not advance a
    counter it never reads (here a host word, which a launch could not touch anyway)."""
    word = (ctypes.c_ulonglong * 1)(5)
    for over in (dict(D=0), dict(P=0), dict(D=0, ended_next=None, saw=None)):
        _call(**over)
        _call(sched=FAKE, round=ctypes.addressof(word), S=1, T=1, **over)
    assert word[0] == 5


def test_constants_match_the_header():
    import os
    import re

    from conftest import ROOT
    from federated_amd import _lib
    text = open(os.path.join(ROOT, "include", "cfa_engine.h")).read()
    for name in ("COPY", "TRUNCATE", "TRUNCATE_EPS"):
        m = re.search(r"\bCFA_ENDED_%s\s*=\s*(\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "ENDED_" + name), name


def test_rule_names_and_device_ids_are_checked_on_the_host():
    from federated_amd import _lib
    from federated_amd import topology as T
    assert T.ended_rule_code(None) is None
    assert [T.ended_rule_code(r) for r in ("copy", "truncate", "truncate_eps")] == [
        _lib.ENDED_COPY, _lib.ENDED_TRUNCATE, _lib.ENDED_TRUNCATE_EPS]
    for bad in ("COPY", "", "tf1", 0):
        with pytest.raises(ValueError, match="rule must be None"):
            T.ended_rule_code(bad)
    assert T.ended_flags([], 4).tolist() == [0, 0, 0, 0]
    flags = T.ended_flags([3, 0, 3], 4)
    assert flags.dtype == np.int32 and flags.tolist() == [1, 0, 0, 1]
    for bad in ([4], [-1], [1.5]):
        with pytest.raises(ValueError, match="outside \\[0, 4\\)"):
            T.ended_flags(bad, 4)
