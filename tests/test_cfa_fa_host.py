"""Host half of the CFA-FA population (federated_amd/cfa_fa_population.py): the cycle of server and
consensus epochs derived from the driver's flags (federated_sample_CNN_CFA_FA.py:264-292 against
the server loop :70-137), and the argument checks that need no device."""
import numpy as np
import pytest

from federated_amd.cfa_fa_population import CfaFaPopulation, cfa_fa_cycle


def _client_phases(con, ser, epochs):
    """The client's flag logic of :264-292, transcribed line by line for -S 1 (the server then
    writes its model at every epoch the client waits for)."""
    server_federation, server_counter, out = False, 0, []
    for epoch in range(epochs):
        if (epoch % (con + ser) == 0) | (server_federation):
            server_federation = True
            server_counter = server_counter + 1
            out.append("server")
            if epoch > 0:
                if (server_counter == ser):
                    server_federation = False
                    server_counter = 0
        else:
            server_counter = 0
            out.append("consensus")
    return out


def test_driver_default_cycle():
    assert cfa_fa_cycle(10, 10) == ["server"] * 10 + ["consensus"] * 10


@pytest.mark.parametrize("con,ser", [(10, 10), (3, 3), (1, 2), (5, 2), (2, 7), (0, 4)])
def test_cycle_agrees_with_the_clients_flags_over_three_cycles(con, ser):
    cycle = cfa_fa_cycle(con, ser)
    assert len(cycle) == con + ser and cycle[0] == "server"
    assert cycle * 3 == _client_phases(con, ser, 3 * (con + ser))


@pytest.mark.parametrize("args,epoch", [((10, 10, 2), 2), ((3, 1), 1), ((3, 1, 3), 1), ((4, 5, 4), 2)])
def test_settings_that_deadlock_the_driver_are_refused(args, epoch):
    with pytest.raises(ValueError, match=f"at epoch {epoch} "):
        cfa_fa_cycle(*args)
    with pytest.raises(ValueError, match="need consensus_epochs"):
        cfa_fa_cycle(3, 0)


def test_check_is_host_only():
    bal = CfaFaPopulation.check(5)
    assert bal.dtype == np.float64 and np.array_equal(bal, np.ones(5) * (1 / 5))
    assert np.array_equal(CfaFaPopulation.check(3, [0.5, 0.25, 0.25], 1.0, 0.5, cfa_fa_cycle(3, 3)), [0.5, 0.25, 0.25])
    with pytest.raises(ValueError, match="each of the 5 devices"):
        CfaFaPopulation.check(5, [0.5, 0.5])
    with pytest.raises(ValueError, match="each of the 2 devices"):
        CfaFaPopulation.check(2, [0.5, float("nan")])
    with pytest.raises(ValueError, match='must be "server"'):
        CfaFaPopulation.check(5, None, 1.0, 0.5, ["consensus", "server"])
    with pytest.raises(ValueError, match="at least one epoch"):
        CfaFaPopulation.check(5, None, 1.0, 0.5, [])
    with pytest.raises(ValueError, match="phases only"):
        CfaFaPopulation.check(5, None, 1.0, 0.5, ["server", "fedavg"])
    with pytest.raises(ValueError, match="finite"):
        CfaFaPopulation.check(5, None, float("inf"), 0.5)
    with pytest.raises(ValueError, match="at least one device"):
        CfaFaPopulation.check(0)


def test_library_exports_the_round():
    from federated_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "cfa_fa_population_round_f32")
    assert (_lib.FA_INIT, _lib.FA_ROUND) == (0, 1)
    assert lib.cfa_fa_round_tile(1488, 1) % (256 * 4) == 0 and lib.cfa_fa_round_tile(1488, 0) % 256 == 0
