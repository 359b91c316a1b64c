"""The scenario table of tests/migrate_cases.py without a GPU: every scenario's call lists through the reference chains alone, and at
every move the state the scenario is named for -- the held-back count in its range, an open outgoing frame with 0 < pending < F, an
open collector slot with at least one block (or no collector at all), what the replaced destination stream held, the frames each
stream completed before the move (the windows of scenario 7), and afterwards at least two frames completed in the destination, the
first of which was opened in the source.  This is what keeps tests/test_gpu_stream_migrate_states.py from quietly testing another
state after an edit of a seed or a cut point: the conditions are asserted, nothing here skips.

The compiled reference collector has no decoder without a device, so the chains collect with the oracle's restatement here (held
against the compiled class by tests/test_fecbuf_edges_model.py); the GPU tests use the compiled class."""
import pytest

import migrate_cases as mc


@pytest.mark.parametrize("case", mc.RX_CASES, ids=lambda c: c.id)
def test_rx_scenario_reaches_its_state(oracle, case):
    mc.check_conditions(case, case.run(mc.RxRun(oracle, None, case.id)))


@pytest.mark.parametrize("case", mc.TX_CASES, ids=lambda c: c.id)
def test_tx_scenario_reaches_its_state(oracle, case):
    mc.check_conditions(case, case.run(mc.TxRun(oracle, None, case.id)))


def test_the_table_names_every_state():
    """every scenario of the issue is in the table, with the variants the GPU file parametrises over"""
    rx = {c.fn.__name__ for c in mc.RX_CASES}
    tx = {c.fn.__name__ for c in mc.TX_CASES}
    assert len(rx) == 11 and len(tx) == 7, (sorted(rx), sorted(tx))
    assert len({c.id for c in mc.RX_CASES + mc.TX_CASES}) == len(mc.RX_CASES) + len(mc.TX_CASES)
