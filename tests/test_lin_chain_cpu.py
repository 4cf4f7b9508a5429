"""The linear window chain without a GPU (test backend): linear_chain's torch route against the float64 loop of
tests/lin_chain_cases.py, and --module RRGCN / BiRRGCN on the batched path -- flags, loss and gradients against the reference-granular
route, the per-position loop and the float64 oracle, and the backend calls of a training step.  The test backend has no chain kernels,
so the node runs its per-instance loop: the step's call list is the per-position one on both settings of use_lin_chain.

Measured (max err / bar; bars rtol 1e-5 / atol 2e-6 . max(1, max |ref|) for the states, 1e-4 / 2e-5 . max(1, max |ref|) for d_x, d_W):
  d = 20   states 0.041  d_x 0.0021  d_W 0.0071        d = 32   states 0.066  d_x 0.0047  d_W 0.0063
  d = 200  states 0.11   d_x 0.0093  d_W 0.012         d = 220  states 0.13   d_x 0.010   d_W 0.011      (largest over act and want)
Window models (D = 32, ICEWS14 slice): RRGCN loss 18.26619911 on all three routes, float64 oracle within 7.2e-9 relative; BiRRGCN
24.35783386, oracle within 2.9e-8."""
from collections import Counter

import pytest
import torch

from temp_amd import backend as TB
from tests import lin_chain_cases as C
from tests.cpu_backend import CpuTestBackend

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


@pytest.mark.parametrize("want_last", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("d", C.WIDTHS)
def test_torch_route_vs_fp64_loop(d, act, want_last):
    C.check_node(d, act, want_last, CPU)


def test_zero_weight_returns_x():
    prog, n_x = C.program()
    x, ws = C.inputs(n_x, 32, 2)
    res = C.run_node(prog, x, [torch.zeros_like(w) for w in ws], 0, None, CPU)
    assert torch.equal(torch.cat(res["outs"]), x)


def test_empty_program_and_single_position():
    """No recurrence step at all: the node is the activation of x."""
    from temp_amd import lin_chain as LC
    from temp_amd.gru_chain import GruInstance, GruProgram
    import numpy as np
    prog = GruProgram([GruInstance(5, 0, 0, -1, np.full(5, -1, dtype=np.int64), np.zeros(5, dtype=np.float32))])
    x = torch.randn(5, 8)
    (h,) = LC.linear_chain(x, prog, [torch.randn(8, 8)], 0.1, 1, want=[0])
    assert torch.equal(h, torch.relu(x))
    assert LC.linear_chain(x[:0], GruProgram([]), [torch.randn(8, 8)], 0.1, 1, want=[]) == ()


@pytest.mark.parametrize("module,golden", C.MODELS)
def test_window_models(module, golden):
    C.check_window_model(module, golden, CPU)


def test_dropout_all_entity_pass_keeps_windows_apart():
    C.check_dropout_all_entity(CPU)


@pytest.mark.parametrize("lin_chain", [True, False])
@pytest.mark.parametrize("module,golden", C.MODELS)
def test_step_calls(module, golden, lin_chain):
    """No chain kernels on this backend: one linear + decay_rows per history position with a previous state on either setting,
    plus the centre's two (Bi) and the all-entity pass (one pair launch for RRGCN; two per window for BiRRGCN, whose pass stays per
    window)."""
    calls, L = C.step_calls(module, golden, CPU, lin_chain)
    n = Counter(calls)
    assert n["lin_chain_fwd"] == 0 and n["lin_chain_bwd"] == 0
    B = 4
    fwd = (2 * (L - 2) + 2 + 2 * B) if module.startswith("Bi") else (L - 1) + 1
    # (`linear` also serves the per-graph loss of BiRRGCN: one product forward and one backward per window)
    assert n["decay_rows"] == 2 * fwd and n["linear"] == 2 * fwd + (2 * B if module.startswith("Bi") else 0), (n["decay_rows"], n["linear"], fwd)
    assert (n["gather_ce_fwd"] == 1) == (module == "RRGCN")          # the fused loss node comes along with the batched all-entity pass
