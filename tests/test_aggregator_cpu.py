"""The Aggregator (temp_amd.aggregator) and its frozen-ensemble loss node without a GPU: the cases of tests/aggregator_cases.py driven
through the CPU test backend, which has no frozen_mix_ce -- the node takes the plain-torch composite of the same formula
(link_loss.frozen_mix_ce_rows and its autograd)."""
import pytest
import torch

from temp_amd import backend as TB
from tests import aggregator_cases as AC
from tests.cpu_backend import CpuTestBackend

DEV = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


def test_aggregator_is_exported():
    import temp_amd
    from temp_amd import _lib
    assert temp_amd.Aggregator is AC.Aggregator
    assert "temp_frozen_mix_ce" in _lib.SYMBOLS and _lib.FROZEN_KINDS == {"dot": 0, "l1": 1}
    assert not hasattr(CpuTestBackend(), "frozen_mix_ce") and hasattr(TB.HipBackend, "frozen_mix_ce")


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("score,temporal", [("distmult", "GRRGCN"), ("complex", "BiGRRGCN"), ("transE", "GRRGCN"), ("distmult", "SARGCN")])
def test_fused_vs_literal(score, temporal, B):
    AC.check_fused_vs_literal(DEV, score, temporal, B)


@pytest.mark.parametrize("temporal", ["SARGCN", "BiSARGCN"])
def test_attention_temporal_against_literal_composition(temporal):
    AC.check_literal_composition(DEV, temporal)


@pytest.mark.parametrize("which", ["uni", "bi"])
def test_golden_G30_loss(which):
    AC.check_golden_loss("G30_aggregator_" + which, DEV)


def test_golden_G30_loss_through_run_directories(tmp_path):
    AC.check_golden_loss("G30_aggregator_bi", DEV, tmp_path)


@pytest.mark.parametrize("which", ["uni", "bi"])
def test_golden_G31_ranks(which):
    AC.check_golden_ranks("G31_eval_aggregator_" + which, DEV)


def test_two_widths_fused_vs_literal():
    AC.check_fused_vs_literal(DEV, "distmult", "GRRGCN", 3, temporal_width=24)


def test_node_vs_composite():
    AC.check_node_vs_composite(DEV)


def test_state_dict_keys_and_order():
    AC.check_state_dict(DEV)


def test_checkpoint_directory_round_trip(tmp_path):
    AC.check_checkpoint_round_trip(DEV, tmp_path)


def test_refusals(tmp_path):
    AC.check_refusals(DEV, tmp_path)


def test_debug_constructor():
    AC.check_debug_constructor(DEV)


def test_evaluate_against_brute_force():
    AC.check_evaluate(DEV)


def test_predict_gated_against_brute_force():
    AC.check_predict_gated(DEV)


def test_optimizer_step_moves_only_the_mlps():
    AC.check_optimizer_step(DEV)
