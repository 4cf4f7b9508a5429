"""--module RRGCN with both layers recurrent on the MI355X (DynamicRGCN._run_lin_stack: two temp_lin_chain launches over one program,
the pair rows of the all-entity pass on temp_lin_rows_fwd / _bwd): the cases of tests/lin_stack_cases.py -- flags, loss, gradients
and encode() against use_lin_stack = False and the float64 oracle at check_window_model's bars (loss 2e-5 relative; gradients rtol
1e-4 / atol 3e-6 . max(1, max |ref|); encode rows 1e-5 / 2e-6), evaluate() ranks, the dropout layout, --learnable-lambda, BiRRGCN
unchanged -- and the backend calls of a training step.  Runs on poisoned allocations.  Every comparison prints its figure before it
asserts (pytest -s).

Measured on the MI355X: loss 24.35153770 on both routes, float64 oracle 24.35153886 (4.7e-8 relative); gradients at most 0.23 of the
bar against use_lin_stack = False and 0.058 against the oracle; evaluate(): 176 ranks, none differ, 0.222 of the rows with a competitor
inside the tie band; backend calls of a step 43 against 262."""
from collections import Counter

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import lin_stack_cases as C
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def test_stack_model():
    c0 = _lib.load().temp_lin_chain_launches()
    C.check_stack_model(DEV)
    assert _lib.load().temp_lin_chain_launches() - c0 == 2 + 2 + 2          # two chains forward + backward, two more in encode(train=False)


def test_evaluate_ranks():
    C.check_evaluate(DEV)


def test_dropout_all_entity_pass_keeps_windows_apart():
    C.check_dropout(DEV)


def test_learnable_lambda_takes_the_chain_routes():
    C.check_learnable_lambda(DEV)


def test_birrgcn_both_layers_keeps_its_path():
    C.check_bi_unchanged(DEV)


def test_step_calls():
    """The new route: exactly two chain launches and two pair-row launches each way, no decay_rows at all, one fused loss node.
    use_lin_stack = False: the reference-granular list -- linear + decay_rows per position, window and layer, the per-graph loss."""
    calls, L, B = C.step_calls(DEV, True)
    n = Counter(calls)
    assert n["lin_chain_fwd"] == 2 and n["lin_chain_bwd"] == 2 and n["lin_rows_fwd"] == 2 and n["lin_rows_bwd"] == 2, n
    assert n["decay_rows"] == 0 and n["gather_ce_fwd"] == 1, n
    calls, L, B = C.step_calls(DEV, False)
    m = Counter(calls)
    assert m["lin_chain_fwd"] == 0 and m["lin_chain_bwd"] == 0 and m["lin_rows_fwd"] == 0 and m["lin_rows_bwd"] == 0, m
    assert m["decay_rows"] == 2 * (2 * L + 2 * B) and m["gather_ce_fwd"] == B, m
    print("backend calls of the step: new route %d, reference-granular %d" % (sum(n.values()), sum(m.values())))
