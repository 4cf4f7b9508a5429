"""The mixed filtered top-k selection without a GPU (tests/topk_mix_cases.py): the composite route -- mixed_scores + topk_composite,
the reference of the kernel's tests -- against a python sort of the mixed row; the two mixed filters' topk_single_graph and
predict_gated through the test backends, which have no `filtered_topk_mix` and therefore take that route; the input conditions
(ambiguity cap) of the GPU model tests."""
import numpy as np
import pytest
import torch

from temp_amd import backend as TB
from temp_amd import evaluation
from temp_amd.evaluation import mixed_scores, topk_composite
from tests import topk_cases as KC
from tests import topk_mix_cases as MC
from tests.cpu_backend import CpuTestBackend
from tests.test_gated_transe_cpu import GatedL1CpuBackend
from tests.test_post_attention_cpu import SplitCpuBackend
from tests.test_transe_cpu import L1CpuBackend

DEV = torch.device("cpu")
ident = lambda t: t


@pytest.fixture(autouse=True)
def cpu_backend():
    TB.set_backend(SplitCpuBackend())
    yield
    TB.set_backend(None)


def composite_select(k):
    be = TB.get_backend()
    assert not hasattr(be, "filtered_topk_mix") and not hasattr(be, "filtered_topk")
    return evaluation._select_mixed(be, k), evaluation._select(be, k)


def _sets(ptr, ids, P):
    if ptr is None:
        return None
    return [set(int(x) for x in ids[int(ptr[p]):int(ptr[p + 1])]) for p in range(P)]


@pytest.mark.parametrize("N", [3, 4, 1025])
@pytest.mark.parametrize("k", [1, 10, 65])
def test_reference_equals_python_sort(k, N):
    """mixed_scores + topk_composite == the contract applied entity by entity to the mixed row formed in python floats: a column
    that is -inf in either operand is never returned whatever the weight, no NaN, every filter variant with and without keep."""
    P = 5
    a, b, w, mixed = MC.mix_inputs(P, N)
    m64 = MC.brute_mixed(a, b, w, N)
    assert not bool(torch.isnan(mixed[:, :N]).any())
    assert torch.equal(mixed[:, :N].double(), m64)
    assert torch.equal(mixed[:, :N] == KC.NINF, MC.dead_columns(a, b, N))
    for kind in MC.FILTERS:
        for with_keep in (False, True):
            ptr, ids, keep = KC.filter_lists(kind, mixed, N, with_keep)
            val, idx = topk_composite(mixed_scores(a, b, w), k, ptr, ids, keep, n=N)
            want_val, want_idx = KC.brute_topk(m64, k, _sets(ptr, ids, P), keep, n=N)
            assert torch.equal(idx, want_idx) and torch.equal(val.double(), want_val), (kind, with_keep)


@pytest.mark.parametrize("N", [4, 1025])
@pytest.mark.parametrize("k", [1, 10])
def test_composite_route_cases(k, N):
    MC.check_selection(composite_select(k)[0], ident, k, N)


@pytest.mark.parametrize("order", ["asc", "shuffled"])
def test_composite_route_panels_and_identity(order):
    sel, plain = composite_select(10)
    MC.check_panels(sel, plain, ident, 1000, order)
    MC.check_panels(sel, plain, ident, 1000, order, alternate=True)
    MC.check_identity(sel, plain, ident)


@pytest.mark.parametrize("panel", [None, 64])
@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("mode", ["tail", "head"])
@pytest.mark.parametrize("N", [204, 203])
@pytest.mark.parametrize("name", ["distmult", "complex", "transE"])
@pytest.mark.parametrize("family", ["ensemble", "aggregation"])
def test_evaluater_exact_on_integer_tables(family, name, N, mode, filtered, panel):
    TB.set_backend(GatedL1CpuBackend() if name == "transE" else CpuTestBackend())
    MC.check_evaluater(DEV, family, name, N, 8, mode, filtered, panel)


def test_evaluater_literal_route():
    """A backend without l1_mix_scores sends the embedding-level TransE gate down the literal calc_score route."""
    TB.set_backend(L1CpuBackend())
    assert not hasattr(TB.get_backend(), "l1_mix_scores")
    MC.check_evaluater(DEV, "aggregation", "transE", 203, 8, "head", True, 64)


def test_evaluater_routes_and_panel_rule():
    """A backend with `filtered_topk_mix` is asked for k <= TEMP_TOPK_MAX and not above; two matrices are alive at once, so
    panel=None stays one panel while 2 Q ld 4 bytes fit the budget and splits above it; bad weights, panel and mode are refused;
    no queries give empty results."""
    from temp_amd import _lib

    class Counting(CpuTestBackend):
        calls = 0

        def filtered_topk_mix(self, s_a, s_b, w, k, filt_ptr=None, filt_ids=None, keep=None, col0=0, n=None, carry=None):
            Counting.calls += 1
            assert s_a.shape == s_b.shape and s_a.shape[1] % 4 == 0 and w.shape == (s_a.shape[0],)
            return topk_composite(mixed_scores(s_a, s_b, w), k, filt_ptr, filt_ids, keep, col0, n, carry)

    TB.set_backend(Counting())
    ev = MC.check_evaluater(DEV, "ensemble", "distmult", 204, 8, "tail", True, None)
    assert Counting.calls == 3                                   # one panel per timestamp
    loc, rel_rows = KC.integer_tables(204, 8, 6)
    rec, _ = KC.integer_tables(204, 8, 6, seed=1)
    known, rel, w = np.array([3, 9]), np.array([1, 2]), torch.tensor([0.25, 0.75])
    ev.topk_single_graph(loc, rec, rel_rows, known, rel, w, "tail", 0, _lib.TOPK_MAX + 1)
    assert Counting.calls == 3
    budget = evaluation.TOPK_PANEL_BYTES
    try:
        evaluation.TOPK_PANEL_BYTES = 2 * 2 * 204 * 4           # both matrices of two queries fit exactly: one panel
        a = ev.topk_single_graph(loc, rec, rel_rows, known, rel, w, "tail", 0, 10)
        assert Counting.calls == 3 + 1
        evaluation.TOPK_PANEL_BYTES = 2 * 2 * 204 * 4 - 1       # no longer: panels of (budget // 16) // 4 * 4 = 200 columns
        b = ev.topk_single_graph(loc, rec, rel_rows, known, rel, w, "tail", 0, 10)
        assert Counting.calls == 3 + 1 + 2
    finally:
        evaluation.TOPK_PANEL_BYTES = budget
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        ev.topk_single_graph(loc, rec, rel_rows, known, rel, w, "tail", 0, 10, panel=6)
    with pytest.raises(ValueError):
        ev.topk_single_graph(loc, rec, rel_rows, known, rel, w, "single", 0, 10)
    with pytest.raises(ValueError):
        ev.topk_single_graph(loc, rec, rel_rows, known, rel, w[:1], "tail", 0, 10)
    ids, vals = ev.topk_single_graph(loc, rec, rel_rows, known[:0], rel[:0], w[:0], "head", 0, 10)
    assert tuple(ids.shape) == tuple(vals.shape) == (0, 10)


@pytest.mark.parametrize("kind", MC.MODELS)
def test_predict_gated_against_fp64_tables(kind):
    MC.check_predict_gated(kind, DEV)


def test_predict_gated_distmult():
    MC.check_predict_gated("PostEnsembleGRRGCN", DEV, "distmult")


@pytest.mark.parametrize("kind", MC.MODELS)
def test_weight_extremes_are_the_single_tables(kind):
    MC.check_weight_extremes(kind, DEV)


@pytest.mark.parametrize("kind", MC.MODELS)
def test_own_gates_state_dict_and_predict_refusal(kind):
    MC.check_own_gates(kind, DEV)


def test_injected_weights_are_checked():
    m, s = MC.build_model("PostBiGRRGCN", DEV)
    q = MC.model_queries(s, "tail")
    with pytest.raises(ValueError):
        m.predict_gated(q, weights=torch.rand(q.shape[0]))      # the embedding-level gate takes a pair
    with pytest.raises(ValueError):
        m.predict_gated(q, weights=(torch.rand(3), torch.rand(3)))
    with pytest.raises(ValueError):
        m.predict_gated(q, mode="single")


def test_impute_models_have_no_gated_route():
    from temp_amd.post_dynamic_rgcn import ImputeDynamicRGCN
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    m = ImputeDynamicRGCN(make_args(module="GRRGCN", rec_only_last_layer=True, impute=True), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    with pytest.raises(NotImplementedError, match="no gates"):
        m.predict_gated(np.array([[20, 5, 1]]))
