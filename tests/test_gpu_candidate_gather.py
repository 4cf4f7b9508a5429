"""The candidate-gather route of the bilinear scorers on the MI355X: the dot candidate kernels (temp_dot_ce_* / temp_dot_mix_ce_*)
against the fp64 references and derived bounds of tests/candidate_gather_cases.py, their entry-point conditions and trace names,
the three batched nodes on route "gather" against the literal fp64 expression and against route "gemm", the nodes and a model above
the LDS ceiling of temp_gather_ce_bwd (N = 40 708: what raised before the route existed), the auto rule, and the models."""
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
from tests.test_gpu_row_loss_routes import _p, _traced
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
within = GC.within
L1_NAMES = ("k_gather_ce", "k_gather_ce_mix")             # the trace names the L1 instantiations (and the GEMM route's CE) keep
PLAIN_GEMM = ["bilinear_query_fwd", "linear_multi", "gather_ce_fwd", "gather_ce_bwd", "linear_multi", "linear_tn_multi", "bilinear_query_bwd",
              "segment_sum_rows", "segment_sum_rows"]     # the sampled plain node's list, tests/test_gpu_loss_routes.py 'plain-distmult'
PLAIN_GATHER = ["bilinear_query_fwd", "dot_ce_fwd", "dot_ce_bwd_q", "dot_ce_bwd_table", "bilinear_query_bwd", "segment_sum_rows", "segment_sum_rows"]
GATED_GATHER = ["gated_query_fwd", "dot_mix_ce_fwd", "dot_mix_ce_bwd_q", "dot_mix_ce_bwd_table", "gated_query_bwd", "segment_sum_rows",
                "segment_sum_rows", "segment_sum_rows"]


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def dv(t):
    return None if t is None else t.to(DEV)


def recorded(be, fn):
    rec = Launches(be)
    TB.set_backend(rec)
    try:
        out = fn()
    finally:
        TB.set_backend(None)
    return out, [c[0] for c in rec.calls]


# ---- 1. kernels against fp64 ---------------------------------------------------------------------------------------------------
def run_plain(be, case, use_rs):
    q, table, base, cand = dv(case["q"]), dv(case["table"]), dv(case["base"]), dv(case["cand"])
    s, loss, lse = be.dot_ce_fwd(q, table, base, cand)
    g, d_q = be.dot_ce_bwd_q(q, table, base, cand, s, lse, dv(case["scale"]), case["inv_rows"], dv(case["row_scale"]) if use_rs else None)
    slot_ptr, slot = TF.l1_slots(cand, base, case["n_rows"])
    d_table = be.dot_ce_bwd_table(q, table, slot_ptr, slot, g)
    return dict(s=s, loss=loss, lse=lse, g=g, d_q=d_q, d_table=d_table, slot_ptr=slot_ptr, slot=slot)


def run_mix(be, case, use_rs, w=None):
    q, ta, tb, base, cand = dv(case["q"]), dv(case["table_a"]), dv(case["table_b"]), dv(case["base"]), dv(case["cand"])
    w = dv(case["w"] if w is None else w)
    s, loss, lse = be.dot_mix_ce_fwd(q, ta, tb, w, base, cand)
    g, d_q, d_w = be.dot_mix_ce_bwd_q(q, ta, tb, w, base, cand, s, lse, dv(case["scale"]), case["inv_rows"], dv(case["row_scale"]) if use_rs else None)
    slot_ptr, slot = TF.l1_slots(cand, base, case["n_rows"])
    d_a, d_b = be.dot_mix_ce_bwd_table(q, ta, tb, w, slot_ptr, slot, g)
    return dict(s=s, loss=loss, lse=lse, g=g, d_q=d_q, d_w=d_w, d_table_a=d_a, d_table_b=d_b)


def _unused_rows(case):
    used = torch.zeros(case["n_rows"], dtype=torch.bool)
    used[TC.table_rows(case).reshape(-1)] = True
    return ~used


@pytest.mark.parametrize("d,C,P,rows,windows", GC.CANDIDATE_CASES)
def test_dot_kernels_against_fp64(d, C, P, rows, windows, hip_backend):
    """temp_dot_ce_fwd / _bwd_q / _bwd_table: scores, loss, softmax gradient and both adjoints inside the derived bounds, with the
    per-row weights (one of them 0) and with the uniform one; bit-equal when run again; the slot lists' contract; the zero query row,
    C == 1, the weight-0 row and the table rows without slots give exact zeros."""
    case = GC.dot_case(d, C, P, rows, windows)
    want_ptr, want_slot = TC.slot_lists(case)
    unused = _unused_rows(case)
    for use_rs in (True, False):
        ref = GC.dot_reference(case, use_rs)
        a, b = run_plain(hip_backend, case, use_rs), run_plain(hip_backend, case, use_rs)
        for k in a:
            assert torch.equal(a[k], b[k]), "%s is not bit-repeatable" % k
        assert torch.equal(a["slot_ptr"].cpu(), want_ptr) and torch.equal(a["slot"].cpu(), want_slot), "slot lists"
        what = "dot d=%d C=%d P=%d rows=%d windows=%d row_scale=%s " % (d, C, P, rows, windows, use_rs)
        within(a["s"], ref["s"], ref["tol_s"], what + "scores")
        within(a["lse"], ref["lse"], ref["tol_loss"], what + "lse")
        within(a["loss"], ref["loss"], ref["tol_loss"], what + "loss")
        eps = ref["eps"]
        within(a["g"], ref["g"], eps * ref["a_g"], what + "g")
        within(a["d_q"], ref["d_q"], eps * ref["a_q"], what + "d_q")
        within(a["d_table"], ref["d_table"], eps * ref["a_table"], what + "d_table")
        assert float(a["s"][0].abs().max()) == 0.0, "the zero query row scores exactly 0"
        assert float(a["d_table"].cpu()[unused].abs().max() if bool(unused.any()) else 0.0) == 0.0, "rows without slots"
        if use_rs:                                           # the weight-0 row: nothing of it anywhere
            assert float(a["g"][P - 1].abs().max()) == 0.0 and float(a["d_q"][P - 1].abs().max()) == 0.0
        if C == 1:
            assert float(a["loss"].abs().max()) == 0.0, "C == 1: the loss must be exactly 0"
            assert float(a["g"].abs().max()) == 0.0 and float(a["d_q"].abs().max()) == 0.0 and float(a["d_table"].abs().max()) == 0.0


@pytest.mark.parametrize("d,C,P,rows,windows", GC.CANDIDATE_CASES)
def test_dot_mix_kernels_against_fp64(d, C, P, rows, windows, hip_backend):
    """temp_dot_mix_ce_fwd / _bwd_q / _bwd_table inside the derived bounds (d_w and both table adjoints included); bit-repeatable;
    exact zeros as for the one-table kernels; w all 1 resp. all 0 agrees with the one-table kernel on table_a resp. table_b."""
    case = GC.dot_mix_case(d, C, P, rows, windows)
    unused = _unused_rows(case)
    for use_rs in (True, False):
        ref = GC.dot_mix_reference(case, use_rs)
        a, b = run_mix(hip_backend, case, use_rs), run_mix(hip_backend, case, use_rs)
        for k in a:
            assert torch.equal(a[k], b[k]), "%s is not bit-repeatable" % k
        what = "dot mix d=%d C=%d P=%d rows=%d windows=%d row_scale=%s " % (d, C, P, rows, windows, use_rs)
        within(a["s"], ref["s"], ref["tol_s"], what + "scores")
        within(a["lse"], ref["lse"], ref["tol_loss"], what + "lse")
        within(a["loss"], ref["loss"], ref["tol_loss"], what + "loss")
        within(a["g"], ref["g"], ref["eps"] * ref["a_g"], what + "g")
        within(a["d_q"], ref["d_q"], ref["tol_q"], what + "d_q")
        within(a["d_w"], ref["d_w"], ref["tol_w"], what + "d_w")
        within(a["d_table_a"], ref["d_table_a"], ref["tol_ta"], what + "d_table_a")
        within(a["d_table_b"], ref["d_table_b"], ref["tol_tb"], what + "d_table_b")
        if bool(unused.any()):
            assert float(a["d_table_a"].cpu()[unused].abs().max()) == 0.0 and float(a["d_table_b"].cpu()[unused].abs().max()) == 0.0
        if use_rs:
            assert float(a["g"][P - 1].abs().max()) == 0.0 and float(a["d_q"][P - 1].abs().max()) == 0.0 and float(a["d_w"][P - 1]) == 0.0
        if C == 1:
            assert float(a["loss"].abs().max()) == 0.0 and float(a["g"].abs().max()) == 0.0 and float(a["d_w"].abs().max()) == 0.0
            assert float(a["d_table_a"].abs().max()) == 0.0 and float(a["d_table_b"].abs().max()) == 0.0
    for wv, name in ((1.0, "table_a"), (0.0, "table_b")):
        one = hip_backend.dot_ce_fwd(dv(case["q"]), dv(case[name]), dv(case["base"]), dv(case["cand"]))[0]
        mixed = run_mix(hip_backend, case, False, torch.full((P,), wv))
        for k, v in mixed.items():
            assert bool(torch.isfinite(v).all()), "w = %g: %s" % (wv, k)
        q64, t64 = case["q"].double(), case[name].double()[TC.table_rows(case)]
        tol = (d + 2) * GC.U * (q64.unsqueeze(1) * t64).abs().sum(dim=-1)
        within(mixed["s"], one.cpu(), 2 * tol, "w = %g against the one-table kernel" % wv)


# ---- 2. entry-point conditions --------------------------------------------------------------------------------------------------
ENTRY = ("temp_dot_ce_fwd", "temp_dot_ce_bwd_q", "temp_dot_ce_bwd_table", "temp_dot_mix_ce_fwd", "temp_dot_mix_ce_bwd_q",
         "temp_dot_mix_ce_bwd_table")


def _raw(name, P, C, d, n_rows, tables=True, null_all=False):
    """One raw call of entry point `name` on zero-filled operands (P rows, C candidates, width d, n_rows table rows) -> return code."""
    lib = _lib.load()
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    zi = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=DEV)
    q, ta, tb, w, cand = z(max(P, 1), d), z(max(n_rows, 1), d), z(max(n_rows, 1), d), z(max(P, 1)), zi(max(P, 1), C)
    s, lse, loss, g, d_q, d_w, scale = z(max(P, 1), C), z(max(P, 1)), z(max(P, 1)), z(max(P, 1), C), z(max(P, 1), d), z(max(P, 1)), z(1)
    slot_ptr, slot = zi(n_rows + 1), zi(max(P, 1) * C)
    d_a, d_b = z(max(n_rows, 1), d), z(max(n_rows, 1), d)
    p = (lambda t: None) if null_all else _p
    tabs = [p(ta) if tables else None] + ([p(tb) if tables else None, p(w)] if "mix" in name else [])
    if name.endswith("ce_fwd"):
        args = [P, C, d, p(q)] + tabs + [None, p(cand), p(s), p(loss), p(lse)]
    elif name.endswith("bwd_q"):
        args = [P, C, d, p(q)] + tabs + [None, p(cand), p(s), p(lse), _p(scale), 1.0, None, p(g), p(d_q)] + ([p(d_w)] if "mix" in name else [])
    else:
        args = [n_rows, d, C, p(q)] + tabs + [p(slot_ptr), p(slot), p(g), p(d_a)] + ([p(d_b)] if "mix" in name else [])
    return getattr(lib, name)(*args, None)


@pytest.mark.parametrize("name", ENTRY)
def test_entry_point_conditions(name):
    """P == 0 / n_rows == 0 succeed without a launch (before the pointer checks); d % 4 != 0 is TEMP_E_UNSUPPORTED; NULL tables with
    work are TEMP_E_BADARG; a live call records one launch under the entry point's own name, which is not an L1 name."""
    BADARG, UNSUPPORTED = 1, 2
    rc, names = _traced(lambda: _raw(name, 0, 3, 8, 0, null_all=True))
    assert rc == 0 and names == [], (rc, names)
    rc, names = _traced(lambda: _raw(name, 2, 3, 6, 5))
    assert rc == UNSUPPORTED and names == [], (rc, names)
    rc, names = _traced(lambda: _raw(name, 2, 3, 8, 5, tables=False))
    assert rc == BADARG and names == [], (rc, names)
    assert _raw(name, -1, 3, 8, -1) == BADARG and _raw(name, 2, 0, 8, 5) == BADARG
    rc, names = _traced(lambda: _raw(name, 2, 3, 8, 5))
    torch.cuda.synchronize()
    assert rc == 0 and names == [name.replace("temp_", "k_")], (rc, names)
    assert names[0] not in L1_NAMES


# ---- 3. nodes against the literal fp64 expression -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GC.NODE_KINDS)
@pytest.mark.parametrize("node", GC.NODES)
def test_nodes_against_literal_fp64(node, kind):
    if node == "gated" and kind == "simple":
        # no gated SimplE node exists on the library, on either route: temp_gated_query_* do not take the kind (include/temp_amd.h,
        # the folded-query block), which is outside the candidate stage this route replaces -- the refusal is the behaviour to hold
        for route in ("gather", "gemm"):
            with pytest.raises(_lib.TempAmdError, match="temp_gated_query_fwd"):
                GC.run_node(node, kind, DEV, route)
        return
    GC.check_node(node, kind, DEV, "gather")


def test_node_launches(hip_backend):
    """Route "gather": the plain node's list and the gated node's *_mix_* triple; no linear_multi and no gather_ce_*."""
    _, plain = recorded(hip_backend, lambda: GC.run_node("plain", "complex", DEV, "gather"))
    assert plain == PLAIN_GATHER, plain
    _, gated = recorded(hip_backend, lambda: GC.run_node("gated", "complex", DEV, "gather"))
    assert gated == GATED_GATHER, gated
    _, ens = recorded(hip_backend, lambda: GC.run_node("ensemble", "distmult", DEV, "gather"))
    assert ens.count("dot_ce_fwd") == 2 and ens.count("dot_ce_bwd_q") == 2 and ens.count("dot_ce_bwd_table") == 2, ens
    for names in (plain, gated, ens):
        assert not [n for n in names if n.startswith(("linear", "gather_ce"))], names


# ---- 4. above the ceiling -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", ["plain", "gated"])
def test_nodes_above_the_ceiling(node, hip_backend):
    """N = 40 708 per window, two live windows, 8 rows, C = 21, D = 8, route None: forward and backward succeed on the dot kernels and
    hold the literal fp64 expression; d_big is exactly 0 off the candidate rows.  Route "gemm" still raises in backward."""
    _, names = _traced(lambda: GC.check_node(node, "distmult", DEV, None, N=GC.BIG_N, C=21, both_live=True, against_gemm=False))
    want = {"plain": "k_dot_ce", "gated": "k_dot_mix_ce"}[node]
    assert [n for n in names if n.startswith("k_dot")][:3] == [want + "_fwd", want + "_bwd_q", want + "_bwd_table"], names
    plan = GC.node_plan(DEV, GC.BIG_N, 21, True)
    leaves = GC.node_leaves(node, DEV, GC.BIG_N)
    if node == "plain":
        loss = TF.batched_link_prediction(*leaves, "distmult", plan, route="gemm")
    else:
        loss = TF.batched_gated_link_prediction(*leaves, "distmult", TF.gated_loss_inputs(plan, GC.NODE_ENT, DEV), route="gemm")
    with pytest.raises(_lib.TempAmdError):
        loss.backward()


# ---- 5. auto rule -------------------------------------------------------------------------------------------------------------
def test_auto_rule(hip_backend):
    """route None: at N = 40 704 exactly the plain node's launch list of today, at N = 40 708 the gather list."""
    assert LL.dot_gather_supported(hip_backend) and _lib.GATHER_CE_BWD_MAX_N == GC.CEILING
    assert LL.bilinear_route(None, GC.CEILING) == "gemm" and LL.bilinear_route(None, GC.BIG_N) == "gather"
    _, at = recorded(hip_backend, lambda: GC.run_node("plain", "distmult", DEV, None, N=GC.CEILING, C=21, both_live=True))
    assert at == PLAIN_GEMM, at
    _, above = recorded(hip_backend, lambda: GC.run_node("plain", "distmult", DEV, None, N=GC.BIG_N, C=21, both_live=True))
    assert above == PLAIN_GATHER, above


# ---- 6. models ----------------------------------------------------------------------------------------------------------------
def test_window_model_gather_equals_tensor_path(hip_backend):
    _, names = recorded(hip_backend, lambda: GC.check_window_model(DEV, "gather"))
    assert "dot_ce_fwd" in names and "dot_ce_bwd_table" in names and "gather_ce_fwd" not in names, names


@pytest.mark.parametrize("kind", ["complex", "distmult"])
def test_post_aggregation_model_gather(kind, monkeypatch, hip_backend):
    """PostDynamicRGCN (the gated node) under its existing fused-against-literal check, every model on route "gather"."""
    from tests import post_aggregation_cases as PA
    monkeypatch.setattr(TKG_Module, "candidate_route", "gather")
    _, names = recorded(hip_backend, lambda: PA.check_per_window_equals_batched(DEV, kind))
    assert "dot_mix_ce_fwd" in names and "dot_mix_ce_bwd_table" in names and "gather_ce_mix_fwd" not in names, names


def test_post_ensemble_model_gather(monkeypatch, hip_backend):
    """PostEnsembleBiDynamicRGCN (the ensemble node) under its existing definition check, on route "gather"."""
    from tests.window_cases import check_post_ensemble_loss
    monkeypatch.setattr(TKG_Module, "candidate_route", "gather")
    _, names = recorded(hip_backend, lambda: check_post_ensemble_loss(DEV))
    assert names.count("dot_ce_fwd") == 2 and names.count("dot_ce_bwd_q") == 2 and "gather_ce_fwd" not in names, names


def test_model_above_the_ceiling(hip_backend):
    """A StaticRGCN over 40 708 entities, candidate_route None: one training step's backward succeeds (it raised before the route
    existed) and matches the fused_loss = False step on the same samples."""
    _, names = recorded(hip_backend, lambda: GC.check_big_static_model(DEV, None))
    assert "dot_ce_fwd" in names and "dot_ce_bwd_q" in names and "gather_ce_bwd" not in names, names
