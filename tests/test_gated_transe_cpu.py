"""Gated TransE (the post-aggregation and post-ensemble losses and PostEvaluationFilter with --score-function transE) without a
GPU: the fp64 references of tests/gated_transe_cases.py (their own consistency and the input conditions the GPU tests rely on), the
autograd nodes against torch autograd of the fp64 restatement of the reference formula, and the dispatch of the models and the
evaluation filter, driven through a test backend that implements the gated L1 methods in torch."""
import numpy as np
import pytest
import torch

from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import scores as SC
from tests import gated_transe_cases as GC
from tests import post_aggregation_cases as PA
from tests import transe_cases as TC
from tests.cpu_backend import CpuTestBackend
from tests.golden_util import assert_close, load
from tests.test_transe_cpu import L1CpuBackend, _eval_inputs
from tests.window_cases import build_post_model, make_args, window_inputs


class GatedL1CpuBackend(L1CpuBackend):
    """CpuTestBackend + the L1 methods + the contract of the gated entry points (include/temp_amd.h: temp_gated_query_* of kind
    transE, temp_l1_mix_*) in torch."""
    name = "cpu-test-gated-l1"

    @staticmethod
    def _known(a_rows, a_idx, b_rows, b_idx, w):
        gated = (a_idx >= 0).view(-1, 1)
        b = b_rows.detach()[b_idx.long()]
        a = a_rows.detach()[a_idx.long().clamp(min=0)]
        return torch.where(gated, GC.mix32(w.detach().reshape(-1), a, b), b), a, b, gated

    def gated_query_fwd(self, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail):
        self.calls.append("gated_query_fwd")
        assert kind == "transE"
        known = self._known(a_rows, a_idx, b_rows, b_idx, w)[0]
        r = rel.detach()[rel_idx.long()]
        return torch.where(is_tail.view(-1, 1) != 0, known + r, known - r)

    def gated_query_bwd(self, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail, d_q):
        self.calls.append("gated_query_bwd")
        _, a, b, gated = self._known(a_rows, a_idx, b_rows, b_idx, w)
        wc = w.detach().reshape(-1, 1)
        zero = torch.zeros_like(d_q)
        return (torch.where(gated, wc * d_q, zero), torch.where(gated, (1 - wc) * d_q, d_q), torch.where(is_tail.view(-1, 1) != 0, d_q, -d_q),
                torch.where(gated, d_q * (a - b), zero).sum(dim=1))

    def _cands(self, table_a, table_b, w, rows):
        return GC.mix32(w.detach().reshape(-1), table_a.detach()[rows], table_b.detach()[rows])

    def l1_mix_ce_fwd(self, q, table_a, table_b, w, base, cand):
        self.calls.append("l1_mix_ce_fwd")
        s = -(q.detach().unsqueeze(1) - self._cands(table_a, table_b, w, self._rows(base, cand))).abs().sum(dim=-1)
        lse = torch.logsumexp(s, dim=1)
        return s, lse - s[:, 0], lse

    def l1_mix_ce_bwd_q(self, q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale=None):
        self.calls.append("l1_mix_ce_bwd_q")
        g = torch.exp(s - lse.view(-1, 1))
        g[:, 0] -= 1.0
        g = g * (scale.reshape(-1)[0] * (row_scale.view(-1, 1) if row_scale is not None else inv_rows))
        rows = self._rows(base, cand)
        gs = g.unsqueeze(-1) * torch.sign(q.detach().unsqueeze(1) - self._cands(table_a, table_b, w, rows))
        return g, -gs.sum(dim=1), (gs * (table_a.detach()[rows] - table_b.detach()[rows])).sum(dim=(1, 2))

    def l1_mix_ce_bwd_table(self, q, table_a, table_b, w, slot_ptr, slot, g):
        self.calls.append("l1_mix_ce_bwd_table")
        C = g.shape[1]
        cnt = (slot_ptr[1:] - slot_ptr[:-1]).long()
        assert int(cnt.sum()) == slot.numel() == g.numel()
        n = torch.repeat_interleave(torch.arange(table_a.shape[0]), cnt)
        sl = slot.long()
        same = n[1:] == n[:-1]
        assert bool((sl[1:][same] > sl[:-1][same]).all()), "slots must ascend within a table row"
        wp = w.detach().reshape(-1)[sl // C]
        e = GC.mix32(wp, table_a.detach()[n], table_b.detach()[n])
        terms = g.reshape(-1)[sl].view(-1, 1) * torch.sign(q.detach()[sl // C] - e)
        return (torch.zeros_like(table_a).index_add_(0, n, wp.view(-1, 1) * terms),
                torch.zeros_like(table_b).index_add_(0, n, (1 - wp).view(-1, 1) * terms))

    def l1_mix_scores(self, q, table_a, table_b, w):
        self.calls.append("l1_mix_scores")
        N = table_a.shape[0]
        wv = w.detach().reshape(-1)
        s = torch.stack([-(q.detach()[p].view(1, -1) - GC.mix32(wv[p:p + 1].expand(N), table_a.detach(), table_b.detach())).abs().sum(dim=1)
                         for p in range(q.shape[0])])
        pad = (-N) % 4
        return torch.cat([s, s.new_full((s.shape[0], pad), float("-inf"))], dim=1) if pad else s


@pytest.fixture
def gated_backend():
    be = GatedL1CpuBackend()
    TB.set_backend(be)
    yield be
    TB.set_backend(None)


# ---- the references ----------------------------------------------------------------------------------------------------------------
def test_fma32_is_the_fused_multiply_add():
    """mix32's building block against exact rational arithmetic, on products whose double-rounded sum differs from the fused one."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(4000, generator=g), torch.randn(4000, generator=g)
    c = (-(a.double() * b.double())).float() * (1 + 2.0 ** -12 * torch.randn(4000, generator=g))      # heavy cancellation
    c[:1000] = torch.randn(1000, generator=g)
    got = GC.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = float(np.nextafter(got[i].numpy(), np.float32(-np.inf)))
        hi = float(np.nextafter(got[i].numpy(), np.float32(np.inf)))
        err = abs(exact - Fraction(float(got[i])))
        assert err <= abs(exact - Fraction(lo)) and err <= abs(exact - Fraction(hi)), "element %d is not the nearest fp32" % i
    one, zero = torch.ones(5), torch.zeros(5)
    x, y = torch.randn(5, generator=g), torch.randn(5, generator=g)
    assert torch.equal(GC.mix32(one, x, y), x) and torch.equal(GC.mix32(zero, x, y), y), "w == 1 gives a, w == 0 gives b"


@pytest.mark.parametrize("d,C,P,rows,windows", GC.CANDIDATE_CASES)
def test_reference_consistency_and_undetermined_share(d, C, P, rows, windows):
    """Every case: the planted rows are what the docstring says, the reference is consistent with itself, and at most 0.1 % of the
    elements of each gradient output carry a widened bound (the condition the GPU test's bounds rest on)."""
    case = GC.gated_case(d, C, P, rows, windows)
    tr = TC.table_rows(case)
    assert float(case["w"][0]) == 1.0 and torch.equal(case["q"][0], case["table_a"][tr[0, 0]])
    if P > 1:
        half = torch.arange(d) % 2 == 0
        assert float(case["w"][1]) == 0.0 and torch.equal(case["q"][1][half], case["table_b"][tr[1, 0]][half])
    assert float(case["row_scale"][P - 1]) == 0.0
    if C >= 3:                                               # (C == 2: the last row's second candidate is its duplicate instead)
        assert bool((case["cand"][:, C - 1] == 3).all())
    for use_rs in (True, False):
        ref = GC.gated_reference(case, use_rs)
        assert float(ref["s"][0, 0]) == 0.0, "s[0, 0] is exactly 0"
        shares = GC.widened_shares(ref)
        print("d=%d C=%d P=%d rows=%d: %d undetermined components, widened shares %s" % (d, C, P, rows, ref["n_undetermined"], shares))
        assert all(v <= GC.WIDENED_SHARE for v in shares.values()), shares
        if C == 1:
            for k in ("loss", "g", "d_q", "d_w", "d_table_a", "d_table_b"):
                assert float(ref[k].abs().max()) == 0.0, k
        if use_rs:
            assert float(ref["g"][P - 1].abs().max()) == 0.0 and float(ref["d_q"][P - 1].abs().max()) == 0.0
        # d_TA + d_TB is the adjoint of the mixed candidate: the ungated reference of the same scores' gradient
        both = ref["d_table_a"] + ref["d_table_b"]
        assert float((both.sum(dim=0) + ref["d_q"].sum(dim=0)).abs().max()) <= 1e-9 * max(1.0, float(ref["a_g"].sum()))


SMALL = [c for c in GC.CANDIDATE_CASES if c[0] * c[1] * c[2] <= 200 * 101 * 67]


@pytest.mark.parametrize("d,C,P,rows,windows", SMALL)
def test_reference_against_autograd_and_backend(d, C, P, rows, windows):
    """gated_reference == torch autograd of the fp64 formula (q, both tables and the gates as leaves); the torch test backend and
    the slot lists of functional.l1_slots satisfy the same contract inside the derived bounds."""
    case = GC.gated_case(d, C, P, rows, windows)
    idx = TC.table_rows(case)
    for use_rs in (True, False):
        ref = GC.gated_reference(case, use_rs)
        q, ta, tb, w = (case[k].double().requires_grad_(True) for k in ("q", "table_a", "table_b", "w"))
        e = w.view(-1, 1, 1) * ta[idx] + (1 - w.view(-1, 1, 1)) * tb[idx]
        s = -(q.unsqueeze(1) - e).abs().sum(dim=-1)
        assert_close(s, ref["s"], 1e-13, 1e-13, "scores")
        loss_rows = torch.logsumexp(s, dim=1) - s[:, 0]
        rw = case["row_scale"].double() if use_rs else torch.full((P,), case["inv_rows"], dtype=torch.float64)
        (float(case["scale"][0]) * (rw * loss_rows).sum()).backward()
        for got, k in ((q.grad, "d_q"), (w.grad, "d_w"), (ta.grad, "d_table_a"), (tb.grad, "d_table_b")):
            assert_close(got, ref[k], 1e-10, 1e-12, k)
        be = GatedL1CpuBackend()
        args = (case["q"], case["table_a"], case["table_b"], case["w"])
        s32, loss, lse = be.l1_mix_ce_fwd(*args, case["base"], case["cand"])
        g, d_q, d_w = be.l1_mix_ce_bwd_q(*args, case["base"], case["cand"], s32, lse, case["scale"], case["inv_rows"],
                                         case["row_scale"] if use_rs else None)
        ptr, slot = TF.l1_slots(case["cand"], case["base"], case["n_rows"])
        want_ptr, want_slot = TC.slot_lists(case)
        assert torch.equal(ptr, want_ptr) and torch.equal(slot, want_slot)
        d_ta, d_tb = be.l1_mix_ce_bwd_table(*args, ptr, slot, g)
        assert float((s32.double() - ref["s"]).abs().sub(4 * ref["tol_s"]).max()) <= 0
        assert float(s32[0, 0]) == 0.0
        for got, k, t in ((d_q, "d_q", "tol_q"), (d_w, "d_w", "tol_w"), (d_ta, "d_table_a", "tol_ta"), (d_tb, "d_table_b", "tol_tb")):
            assert bool((got.double() - ref[k]).abs().le(4 * ref[t] + 1e-30).all()), "backend " + k


@pytest.mark.parametrize("P,N,d,ld", GC.SCORE_CASES)
def test_dense_score_reference(P, N, d, ld):
    """The dense reference equals the candidate formula, stays above the fp32 sigmoid's underflow, and a sequential fp32 sum of the
    fp32 mix (the dense kernel's order) stays inside the bound."""
    c = GC.gated_score_case(P, N, d)
    assert float(c["s64"].min()) > -100.0
    seq = torch.zeros(P, N)
    e = GC.mix32(c["w"], c["table_a"].unsqueeze(0).expand(P, N, d), c["table_b"].unsqueeze(0).expand(P, N, d)) if P * N * d < 2e7 else None
    if e is not None:
        for k in range(d):
            seq = seq + (c["q"][:, k:k + 1] - e[:, :, k]).abs()
        assert bool(((-seq).double() - c["s64"]).abs().le(c["tol"]).all())


@pytest.mark.parametrize("P,N,d,ld", GC.SCORE_CASES[:2])
@pytest.mark.parametrize("filtered", [False, True])
def test_rank_band_input_condition(P, N, d, ld, filtered):
    """At most 25 % of the rows have a band wider than one rank; the fp32 test backend's ranks lie inside it."""
    c = GC.gated_score_case(P, N, d)
    target, ptr, ids = TC.rank_inputs(P, N)
    if not filtered:
        ptr = ids = None
    lo, hi = TC.rank_band(c["s64"], c["tol"], target, ptr, ids)
    print("ambiguous rows: %.1f %%" % (100 * float((lo != hi).float().mean())))
    assert bool((lo <= hi).all()) and float((lo != hi).float().mean()) <= 0.25
    be = GatedL1CpuBackend()
    ranks = be.filtered_rank(be.l1_mix_scores(c["q"], c["table_a"], c["table_b"], c["w"]), target, ptr, ids)
    assert bool(((ranks >= lo) & (ranks <= hi)).all())


@pytest.mark.parametrize("d", [8, 200])
def test_gated_query_reference(d):
    """gated_query_case: the bit-exact q equals the fp64 mix to rounding, the temporal-only rows are the B row +- r exactly."""
    c = GC.gated_query_case(d)
    a, b, r = c["A"][c["ia"].long().clamp(min=0)].double(), c["B"][c["ib"].long()].double(), c["rel"][c["ridx"].long()].double()
    w = c["w"].double().view(-1, 1)
    known = torch.where(c["gated"].view(-1, 1), w * a + (1 - w) * b, b)
    q64 = torch.where(c["is_tail"].view(-1, 1) != 0, known + r, known - r)
    assert_close(c["q"], q64, 1e-6, 1e-6, "q")
    be = GatedL1CpuBackend()
    q = be.gated_query_fwd("transE", c["A"], c["ia"], c["B"], c["ib"], c["w"], c["rel"], c["ridx"], c["is_tail"])
    assert torch.equal(q, c["q"])


# ---- the functional nodes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bi", [True, False])
def test_gated_node_against_fp64_restatement(gated_backend, bi):
    """functional.batched_gated_link_prediction with kind transE (through model.batched_gated_loss, several windows, one empty)
    against autograd of post_aggregation_cases.reference_loss64: the loss, every gradient, and the w_sqo quirk."""
    gated_backend.calls.clear()
    PA.check_gated_loss_definition(torch.device("cpu"), "transE", bi)
    assert gated_backend.calls[:4] == ["gated_query_fwd", "l1_mix_ce_fwd", "l1_mix_ce_bwd_q", "l1_mix_ce_bwd_table"], gated_backend.calls


def test_per_window_node_equals_literal(gated_backend):
    """gated_loss (the unbatched path's per-window node) == the literal reference formula == the batched node; no N % 4 condition."""
    PA.check_per_window_equals_batched(torch.device("cpu"), "transE")
    assert "l1_mix_ce_fwd" in gated_backend.calls


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------
def _post_model(name, cls_name, **flags):
    from temp_amd import post_dynamic_rgcn as PD
    z = load(name)
    m = build_post_model(z, torch.device("cpu"), getattr(PD, cls_name), True, **flags)
    m.args.score_function = "transE"
    m.calc_score = SC.transE
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    wb = m.prepare(t_list, int(z["L"]), True, edge_ids)
    return m, wb, samples


def _step(m, wb, samples, weights=None):
    for p in m.parameters():
        p.grad = None
    loss = m.run_loss(wb, samples, weights)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name,cls", [("G20_post_agg_uni", "PostDynamicRGCN"), ("G20_post_agg_bi", "PostBiDynamicRGCN")])
def test_post_aggregation_dispatch(gated_backend, name, cls):
    """The post-aggregation models with transE: one call of each gated entry point per step, the slot lists of a fixed sample set
    built once, the same loss and gradients as the tensor path; a backend without the methods takes the tensor path."""
    m, wb, samples = _post_model(name, cls, post_aggregation=True)
    assert m._gated_fused_ok() and not m.bilinear_loss_ok(m.embed_size)
    _step(m, wb, samples)
    gated_backend.calls.clear()
    loss, grads = _step(m, wb, samples)
    watched = [c for c in gated_backend.calls if c.startswith(("gated_query", "l1_"))]
    assert watched == ["gated_query_fwd", "l1_mix_ce_fwd", "l1_mix_ce_bwd_q", "l1_mix_ce_bwd_table", "gated_query_bwd"], watched
    slots = wb._agg_inputs[1]["_l1_slots"]
    _step(m, wb, samples)
    assert wb._agg_inputs[1]["_l1_slots"] is slots, "the slot lists of a fixed sample set are built once"
    m.fused_loss = False
    gated_backend.calls.clear()
    ref, gref = _step(m, wb, samples)
    assert [c for c in gated_backend.calls if c.startswith(("gated_query", "l1_"))] == []
    assert abs(loss.item() - ref.item()) < 2e-5 * abs(ref.item())
    assert sorted(grads) == sorted(gref)
    for k in gref:
        assert_close(grads[k], gref[k], 1e-4, 1e-5 * float(gref[k].abs().max()), k)
    m.fused_loss = True
    TB.set_backend(L1CpuBackend())                            # the L1 methods alone: no gated node
    try:
        assert not TF.gated_translation_supported() and not m._gated_fused_ok()
        plain, _ = _step(m, wb, samples)
    finally:
        TB.set_backend(gated_backend)
    assert abs(plain.item() - ref.item()) < 2e-5 * abs(ref.item())


@pytest.mark.parametrize("name,cls", [("G19_post_ratio_uni", "PostEnsembleDynamicRGCN"), ("G19_post_ratio_bi", "PostEnsembleBiDynamicRGCN")])
def test_post_ensemble_dispatch(gated_backend, name, cls):
    """The post-ensemble models with transE take the L1 kernels per stream (two forward calls, two of each backward call) and give
    the tensor path's loss and gradients; the ensemble weights' gradient reaches the frequency MLPs."""
    m, wb, samples = _post_model(name, cls, post_ensemble=True)
    _step(m, wb, samples)
    gated_backend.calls.clear()
    loss, grads = _step(m, wb, samples)
    watched = [c for c in gated_backend.calls if c.startswith("l1_")]
    assert watched == ["l1_ce_fwd", "l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table", "l1_ce_bwd_q", "l1_ce_bwd_table"], watched
    assert any(k.startswith("subject_linear") for k in grads) and any(k.startswith("object_linear") for k in grads)
    m.fused_loss = False
    gated_backend.calls.clear()
    ref, gref = _step(m, wb, samples)
    assert [c for c in gated_backend.calls if c.startswith("l1_")] == []
    assert abs(loss.item() - ref.item()) < 2e-5 * abs(ref.item())
    assert sorted(grads) == sorted(gref)
    for k in gref:
        assert_close(grads[k], gref[k], 1e-4, 1e-5 * float(gref[k].abs().max()), k)


def test_post_evaluation_filter_dispatch(gated_backend):
    """PostEvaluationFilter with transE calls l1_mix_scores twice (one pass per mode); ranks equal the chunked literal route on the
    rows the fp64 band marks unambiguous, inside the band elsewhere; a backend without the method keeps the literal route."""
    from temp_amd.evaluation import PostEvaluationFilter
    s, t, g, N, all_e, rel, ent, samples = _eval_inputs()
    gen = torch.Generator().manual_seed(9)
    all_r, ent_r = all_e + 0.3 * torch.randn(all_e.shape, generator=gen), ent + 0.3 * torch.randn(ent.shape, generator=gen)
    P = samples.shape[0]
    ws = [torch.rand(P, 1, generator=gen) for _ in range(4)]
    ev = PostEvaluationFilter(make_args(score_function="transE"), SC.transE, s["tr"], s["va"], s["te"])
    gated_backend.calls.clear()
    new = ev.calc_metrics_single_graph(ent, ent_r, rel, all_e, all_r, samples, *ws, g, t)
    assert gated_backend.calls == ["l1_mix_scores", "l1_mix_scores"], gated_backend.calls
    TB.set_backend(L1CpuBackend())
    try:
        old = ev.calc_metrics_single_graph(ent, ent_r, rel, all_e, all_r, samples, *ws, g, t)
    finally:
        TB.set_backend(gated_backend)
    lo, hi = GC.post_eval_band(ev, samples, g, t, N, ent, ent_r, rel, all_e, all_r, ws)
    sure = lo == hi
    assert float((~sure).float().mean()) <= 0.25
    assert torch.equal(new[sure], old[sure]) and torch.equal(new[sure], lo[sure])
    assert bool(((new >= lo) & (new <= hi)).all()) and bool(((old >= lo) & (old <= hi)).all())
