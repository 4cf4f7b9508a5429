"""--module RRGCN with both layers recurrent without a GPU (test backend): the route's flags, loss, gradients and encode() against
use_lin_stack = False and the float64 oracle, evaluate() ranks, the dropout layout, --learnable-lambda, BiRRGCN unchanged, and the
backend calls of a training step.  The test backend has neither the chain kernels nor temp_lin_rows_fwd / _bwd, so both nodes run
their torch forms (the per-instance loop of linear_chain, the composition of lin_step_rows); the composition is compared with the
float64 restatement of tests/lin_stack_cases.py here as well.

Measured: loss 24.35153580 on the new route, 24.35153961 reference-granular, float64 oracle 24.35153886 (1.3e-7 relative); gradients at
most 0.055 of the bar between the routes and 0.042 against the oracle; evaluate(): 176 ranks, none differ, 0.222 of the rows with a
competitor inside the tie band on either route."""
from collections import Counter

import pytest
import torch

from temp_amd import backend as TB
from tests import lin_stack_cases as C
from tests.cpu_backend import CpuTestBackend

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("n", C.ROW_NS)
@pytest.mark.parametrize("d", C.WIDTHS)
def test_rows_composition_vs_fp64(d, n, act):
    assert not C.TF.lin_rows_usable(d)
    C.check_rows_node(n, d, act, CPU)


def test_stack_model():
    C.check_stack_model(CPU)


def test_evaluate_ranks():
    C.check_evaluate(CPU)


def test_dropout_all_entity_pass_keeps_windows_apart():
    C.check_dropout(CPU)


def test_learnable_lambda_takes_the_chain_routes():
    C.check_learnable_lambda(CPU)


def test_birrgcn_both_layers_keeps_its_path():
    C.check_bi_unchanged(CPU)


def test_step_calls():
    """No kernels on this backend: linear + decay_rows per position with a previous state and layer (the torch loop of both chains),
    plus one pair launch per layer in the all-entity pass; the fused loss node comes along with the batched all-entity pass."""
    calls, L, B = C.step_calls(CPU, True)
    n = Counter(calls)
    assert n["lin_chain_fwd"] == 0 and n["lin_rows_fwd"] == 0 and n["gather_ce_fwd"] == 1, n
    fwd = 2 * (L - 1) + 2
    assert n["decay_rows"] == 2 * fwd, (n["decay_rows"], fwd)
    calls, L, B = C.step_calls(CPU, False)
    m = Counter(calls)
    assert m["lin_chain_fwd"] == 0 and m["lin_rows_fwd"] == 0 and m["gather_ce_fwd"] == B, m          # (the per-graph loss)
    assert m["decay_rows"] == 2 * (2 * L + 2 * B), (m["decay_rows"], L, B)       # every position and every window's isolated pass, both layers
