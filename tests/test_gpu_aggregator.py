"""The Aggregator (temp_amd.aggregator) on the GPU: the cases of tests/aggregator_cases.py under the HIP backend, where the loss of
all windows is one temp_frozen_mix_ce launch (the kernel itself: tests/test_gpu_frozen_mix_ce.py), and the node's launch lists."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import aggregator_cases as AC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _traced(fn):
    lib = _lib.load()
    ids, ms, cnt = (ctypes.c_int32 * 256)(), (ctypes.c_float * 256)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(256), "temp_trace_begin")
    try:
        out = fn()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 256, ctypes.byref(cnt)), "temp_trace_end")
    return out, [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)]


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("score,temporal", [("distmult", "GRRGCN"), ("complex", "BiGRRGCN"), ("transE", "GRRGCN"), ("distmult", "SARGCN")])
def test_fused_vs_literal(score, temporal, B):
    AC.check_fused_vs_literal(DEV, score, temporal, B)


@pytest.mark.parametrize("temporal", ["SARGCN", "BiSARGCN"])
def test_attention_temporal_against_literal_composition(temporal):
    AC.check_literal_composition(DEV, temporal)


def test_debug_constructor():
    AC.check_debug_constructor(DEV)


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


def test_node_launches():
    """The node's forward ends in exactly one k_frozen_mix_ce and forms no score matrix; its backward records no library launch."""
    from temp_amd.tkg_module import TKG_Module
    rng = np.random.default_rng(2)
    N, n, P, C, n_rel = 16, 7, 5, 9, 3
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32) * 0.5).to(DEV)
    trip = torch.from_numpy(np.stack([rng.integers(0, n, P), rng.integers(0, n_rel, P), rng.integers(0, n, P)], axis=1))
    smp = [(trip, torch.from_numpy(rng.integers(0, N, (P, C))), torch.from_numpy(rng.integers(0, N, (P, C))))]
    inp = TKG_Module.loss_inputs([0], smp, DEV)
    w = torch.full((2 * P, 1), 0.3, device=DEV, requires_grad=True)
    args = (f(n, 8), f(n_rel, 8), f(N, 8), f(n, 12), f(n_rel, 12), f(N, 12))
    loss, fwd = _traced(lambda: TF.frozen_ensemble_link_prediction(*args, w, "distmult", inp))
    # (the two query folds, k_bilinear_query, are traced under the candidate-CE id "k_gather_ce": loss_kernels.hip)
    assert fwd == ["k_gather_ce", "k_gather_ce", "k_frozen_mix_ce"], fwd
    _, bwd = _traced(lambda: loss.backward())
    torch.cuda.synchronize()
    assert bwd == [], bwd
    assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0


def test_state_dict_keys_and_order():
    AC.check_state_dict(DEV)


def test_checkpoint_directory_round_trip(tmp_path):
    AC.check_checkpoint_round_trip(DEV, tmp_path)


def test_refusals(tmp_path):
    AC.check_refusals(DEV, tmp_path)


def test_evaluate_against_brute_force():
    AC.check_evaluate(DEV)


def test_predict_gated_against_brute_force():
    AC.check_predict_gated(DEV)


def test_optimizer_step_moves_only_the_mlps():
    AC.check_optimizer_step(DEV)
