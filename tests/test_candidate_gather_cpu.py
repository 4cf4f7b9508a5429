"""The candidate-gather route of the bilinear scorers without a GPU: the torch form of the dot contract (what a backend without the
dot methods runs on route "gather") against the fp64 references and derived bounds of tests/candidate_gather_cases.py, the three
batched nodes and the two unbatched ones on the CPU test backend, the route rule, and the route through the models."""
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import link_loss as LL
from temp_amd.tkg_module import TKG_Module
from tests import candidate_gather_cases as GC
from tests import transe_cases as TC
from tests.chain_route_cases import Launches
from tests.cpu_backend import CpuTestBackend

CPU = torch.device("cpu")
SMALL = [c for c in GC.CANDIDATE_CASES if c[0] * c[1] * c[2] <= 200 * 101 * 67]          # (the torch form gathers (P, C, d))


@pytest.fixture(autouse=True)
def cpu_backend():
    be = CpuTestBackend()
    TB.set_backend(be)
    yield be
    TB.set_backend(None)


@pytest.fixture
def dot_calls(monkeypatch):
    """Counts the calls of the torch dot functions (the gather route's launches on this backend)."""
    calls = []
    for name, fn in list(LL._DOT_TORCH.items()):
        monkeypatch.setitem(LL._DOT_TORCH, name, lambda *a, _fn=fn, _n=name, **k: (calls.append(_n), _fn(*a, **k))[1])
    return calls


def test_backend_has_no_dot_kernels(cpu_backend):
    """The CPU test backend stays without the dot methods: auto keeps "gemm" at any N, "gather" runs the contract in torch."""
    assert not LL.dot_gather_supported(cpu_backend)
    assert _lib.GATHER_CE_BWD_MAX_N == GC.CEILING
    for n in (64, GC.CEILING, GC.BIG_N, 1 << 19):
        assert LL.bilinear_route(None, n) == "gemm"
        assert LL.bilinear_route("gather", n) == "gather" and LL.bilinear_route("gemm", n) == "gemm"
    with pytest.raises(ValueError):
        LL.bilinear_route("dense", 64)


@pytest.mark.parametrize("d,C,P,rows,windows", SMALL)
def test_torch_contract_against_fp64(d, C, P, rows, windows):
    """_torch_dot_ce_* in fp32 inside the kernels' derived bounds; the slot lists of l1_slots meet transe_cases.slot_lists' contract."""
    case = GC.dot_case(d, C, P, rows, windows)
    f = LL._DOT_TORCH
    slot_ptr, slot = TF.l1_slots(case["cand"], case["base"], case["n_rows"])
    want_ptr, want_slot = TC.slot_lists(case)
    assert torch.equal(slot_ptr, want_ptr) and torch.equal(slot, want_slot)
    for use_rs in (True, False):
        ref = GC.dot_reference(case, use_rs)
        s, loss, lse = f["dot_ce_fwd"](case["q"], case["table"], case["base"], case["cand"])
        g, d_q = f["dot_ce_bwd_q"](case["q"], case["table"], case["base"], case["cand"], s, lse, case["scale"], case["inv_rows"],
                                   case["row_scale"] if use_rs else None)
        d_t = f["dot_ce_bwd_table"](case["q"], case["table"], slot_ptr, slot, g)
        what = "torch d=%d C=%d P=%d " % (d, C, P)
        GC.within(s, ref["s"], ref["tol_s"], what + "scores")
        GC.within(loss, ref["loss"], ref["tol_loss"], what + "loss")
        GC.within(g, ref["g"], ref["eps"] * ref["a_g"], what + "g")
        GC.within(d_q, ref["d_q"], ref["eps"] * ref["a_q"], what + "d_q")
        GC.within(d_t, ref["d_table"], ref["eps"] * ref["a_table"], what + "d_table")
        assert float(s[0].abs().max()) == 0.0, "the zero query row scores exactly 0"
        if C == 1:
            assert float(loss.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and float(d_t.abs().max()) == 0.0


@pytest.mark.parametrize("d,C,P,rows,windows", SMALL[:6])
def test_torch_mix_contract_against_fp64(d, C, P, rows, windows):
    case = GC.dot_mix_case(d, C, P, rows, windows)
    f = LL._DOT_TORCH
    ref = GC.dot_mix_reference(case, True)
    args = (case["q"], case["table_a"], case["table_b"], case["w"])
    s, loss, lse = f["dot_mix_ce_fwd"](*args, case["base"], case["cand"])
    g, d_q, d_w = f["dot_mix_ce_bwd_q"](*args, case["base"], case["cand"], s, lse, case["scale"], case["inv_rows"], case["row_scale"])
    slot_ptr, slot = TF.l1_slots(case["cand"], case["base"], case["n_rows"])
    d_a, d_b = f["dot_mix_ce_bwd_table"](*args, slot_ptr, slot, g)
    what = "torch mix d=%d C=%d P=%d " % (d, C, P)
    GC.within(s, ref["s"], ref["tol_s"], what + "scores")
    GC.within(loss, ref["loss"], ref["tol_loss"], what + "loss")
    GC.within(d_q, ref["d_q"], ref["tol_q"], what + "d_q")
    GC.within(d_w, ref["d_w"], ref["tol_w"], what + "d_w")
    GC.within(d_a, ref["d_table_a"], ref["tol_ta"], what + "d_table_a")
    GC.within(d_b, ref["d_table_b"], ref["tol_tb"], what + "d_table_b")


@pytest.mark.parametrize("kind", GC.NODE_KINDS)
@pytest.mark.parametrize("node", GC.NODES)
def test_nodes_against_literal_fp64(node, kind, dot_calls):
    GC.check_node(node, kind, CPU, "gather")
    assert dot_calls, "route 'gather' runs the dot contract"


def test_both_windows_live():
    GC.check_node("plain", "complex", CPU, "gather", both_live=True)
    GC.check_node("gated", "distmult", CPU, "gather", both_live=True)


@pytest.mark.parametrize("node", GC.NODES)
def test_node_launches(node, cpu_backend, dot_calls):
    """Route "gather" makes no score GEMM and no gather_ce_* call; route None on this backend is today's GEMM list."""
    for route, gather in (("gather", True), (None, False)):
        rec = Launches(cpu_backend)
        TB.set_backend(rec)
        del dot_calls[:]
        GC.run_node(node, "complex", CPU, route)
        names = [c[0] for c in rec.calls]
        dense = [n for n in names if n.startswith(("linear", "gather_ce"))]
        assert bool(dot_calls) == gather and bool(dense) != gather, (route, names, dot_calls)
    if node == "plain":
        assert dot_calls == [] and names[:4] == ["bilinear_query_fwd", "linear_multi", "gather_ce_fwd", "gather_ce_bwd"], names


def test_unbatched_nodes_route():
    """candidate_cross_entropy / _mixed: route "gather" against route "gemm" on the same inputs (bars of check_node)."""
    g = torch.Generator().manual_seed(9)
    P, N, D, C = 7, 64, 8, 6
    mk = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).requires_grad_(True)
    cand = torch.randint(0, N, (P, C), generator=g).int()
    cand[2, 3] = cand[2, 1]
    leaves = [mk(P, D), mk(N, D), mk(P, D), mk(N, D), torch.rand(P, 1, generator=g).requires_grad_(True)]
    res = {}
    for route in ("gemm", "gather"):
        outs = []
        for fn, xs in ((TF.candidate_cross_entropy, leaves[:2]), (TF.candidate_cross_entropy_mixed, leaves)):
            for x in leaves:
                x.grad = None
            loss = fn(*xs, cand, route=route)
            loss.backward()
            outs.append([loss.detach()] + [x.grad.clone() for x in xs])
        res[route] = outs
    for a, b, what in zip(res["gather"], res["gemm"], ("candidate_cross_entropy", "candidate_cross_entropy_mixed")):
        GC.compare(a, b, what)


def test_window_model_gather_equals_tensor_path(dot_calls):
    m = GC.check_window_model(CPU, "gather")
    assert "dot_ce_fwd" in dot_calls and "dot_ce_bwd_table" in dot_calls
    assert m.candidate_route == "gather" and TKG_Module.candidate_route is None


def test_big_static_model_gather(dot_calls):
    """num_ents = 40 708 on route "gather" (auto stays "gemm" on this backend): the step against fused_loss = False."""
    GC.check_big_static_model(CPU, "gather")
    assert "dot_ce_bwd_q" in dot_calls


@pytest.mark.parametrize("kind", ["complex", "distmult"])
def test_post_aggregation_model_gather(kind, monkeypatch, dot_calls):
    """PostDynamicRGCN (the gated node) under its existing fused-against-literal check, every model on route "gather"."""
    from tests import post_aggregation_cases as PA
    monkeypatch.setattr(TKG_Module, "candidate_route", "gather")
    PA.check_per_window_equals_batched(CPU, kind)
    assert "dot_mix_ce_fwd" in dot_calls and "dot_mix_ce_bwd_table" in dot_calls


def test_post_ensemble_model_gather(monkeypatch, dot_calls):
    """PostEnsembleBiDynamicRGCN (the ensemble node) under its existing definition check, on route "gather"."""
    from tests.window_cases import check_post_ensemble_loss
    monkeypatch.setattr(TKG_Module, "candidate_route", "gather")
    check_post_ensemble_loss(CPU)
    assert dot_calls.count("dot_ce_fwd") == 2 and dot_calls.count("dot_ce_bwd_q") == 2
