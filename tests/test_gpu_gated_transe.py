"""The gated TransE kernels on the GPU against the fp64 references and derived bounds of tests/gated_transe_cases.py: the gated
candidate loss kernels (temp_l1_mix_ce_fwd / _bwd_q / _bwd_table), the gated translation query, the dense gated scores and the
filtered rank over them; the post-aggregation and post-ensemble models' TransE loss against the tensor path; PostEvaluationFilter's
route against the chunked one."""
import numpy as np
import pytest
import torch

from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import scores as SC
from tests import gated_transe_cases as GC
from tests import post_aggregation_cases as PA
from tests import transe_cases as TC
from tests.golden_util import assert_close, load
from tests.test_gpu_transe import _near_zero_head_slots, dv, within
from tests.window_cases import build_post_model, make_args, slice_snapshots, window_inputs
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
U = GC.U


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def run_gated(case, use_row_scale):
    be = TB.get_backend()
    q, ta, tb, w = dv(case["q"]), dv(case["table_a"]), dv(case["table_b"]), dv(case["w"])
    base, cand = dv(case["base"]), dv(case["cand"])
    s, loss, lse = be.l1_mix_ce_fwd(q, ta, tb, w, base, cand)
    g, d_q, d_w = be.l1_mix_ce_bwd_q(q, ta, tb, w, base, cand, s, lse, dv(case["scale"]), case["inv_rows"],
                                     dv(case["row_scale"]) if use_row_scale else None)
    slot_ptr, slot = TF.l1_slots(cand, base, case["n_rows"])
    d_ta, d_tb = be.l1_mix_ce_bwd_table(q, ta, tb, w, slot_ptr, slot, g)
    return dict(s=s, loss=loss, lse=lse, g=g, d_q=d_q, d_w=d_w, d_table_a=d_ta, d_table_b=d_tb, slot_ptr=slot_ptr, slot=slot)


@pytest.mark.parametrize("d,C,P,rows,windows", GC.CANDIDATE_CASES)
def test_gated_candidate_kernels_against_fp64(d, C, P, rows, windows):
    """temp_l1_mix_ce_fwd / _bwd_q / _bwd_table: scores, loss, softmax gradient, d_q, d_w and both table adjoints inside the derived
    bounds, with the per-row weights (one of them 0) and with the uniform one, with base (two windows) and without; bit-equal when
    run again; the slot lists are functional.l1_slots'; the planted rows are exact."""
    case = GC.gated_case(d, C, P, rows, windows)
    want_ptr, want_slot = TC.slot_lists(case)
    for use_rs in (True, False):
        ref = GC.gated_reference(case, use_rs)
        assert all(v <= GC.WIDENED_SHARE for v in GC.widened_shares(ref).values())
        a = run_gated(case, use_rs)
        b = run_gated(case, use_rs)
        for k in a:
            assert torch.equal(a[k], b[k]), "%s is not bit-repeatable" % k
        assert torch.equal(a["slot_ptr"].cpu(), want_ptr) and torch.equal(a["slot"].cpu(), want_slot), "slot lists"
        what = "d=%d C=%d P=%d rows=%d windows=%d row_scale=%s " % (d, C, P, rows, windows, use_rs)
        within(a["s"], ref["s"], ref["tol_s"], what + "scores")
        within(a["lse"], ref["lse"], ref["tol_loss"], what + "lse")
        within(a["loss"], ref["loss"], ref["tol_loss"], what + "loss")
        within(a["g"], ref["g"], ref["eps"] * ref["a_g"], what + "g")
        within(a["d_q"], ref["d_q"], ref["tol_q"], what + "d_q")
        within(a["d_w"], ref["d_w"], ref["tol_w"], what + "d_w")
        within(a["d_table_a"], ref["d_table_a"], ref["tol_ta"], what + "d_table_a")
        within(a["d_table_b"], ref["d_table_b"], ref["tol_tb"], what + "d_table_b")
        assert float(a["s"][0, 0]) == 0.0, "w = 1 and q[0] = its candidate's table_a row: the score is exactly 0"
        if use_rs:                                           # the weight-0 row: nothing of it anywhere
            assert float(a["g"][P - 1].abs().max()) == 0.0 and float(a["d_q"][P - 1].abs().max()) == 0.0 and float(a["d_w"][P - 1]) == 0.0
        if C == 1:
            assert float(a["loss"].abs().max()) == 0.0, "C == 1: the loss must be exactly 0"
            for k in ("g", "d_q", "d_w", "d_table_a", "d_table_b"):
                assert float(a[k].abs().max()) == 0.0, "C == 1: %s must be exactly 0" % k


def test_weight_zero_row_contributes_nothing():
    """The last row (row_scale = 0) leaves both table adjoints bit-equal to those of the case without it."""
    case = GC.gated_case(200, 101, 67, 515, 2)
    a = run_gated(case, True)
    cut = dict(case)
    for k in ("q", "w", "cand", "row_scale", "base"):
        cut[k] = case[k][:-1].contiguous()
    cut["P"] = case["P"] - 1
    b = run_gated(cut, True)
    assert torch.equal(a["d_table_a"], b["d_table_a"]) and torch.equal(a["d_table_b"], b["d_table_b"])
    assert torch.equal(a["d_q"][:-1], b["d_q"]) and torch.equal(a["d_w"][:-1], b["d_w"])


def test_gated_kernels_empty_and_unsupported():
    """P == 0 succeeds without output; d = 6 is refused by every new entry point and by the gated query of kind transE."""
    from temp_amd import _lib
    be = TB.get_backend()
    z = lambda *s: torch.zeros(*s, device=DEV)
    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    q, t = z(0, 8), z(7, 8)
    s, loss, lse = be.l1_mix_ce_fwd(q, t, t, z(0), None, zi(0, 3))
    assert s.shape == (0, 3) and loss.shape == (0,)
    g, d_q, d_w = be.l1_mix_ce_bwd_q(q, t, t, z(0), None, zi(0, 3), s, lse, z(1), 1.0)
    assert g.shape == (0, 3) and d_q.shape == (0, 8) and d_w.shape == (0,)
    d_a, d_b = be.l1_mix_ce_bwd_table(q, t, t, z(0), zi(8), zi(0), g)
    assert float(d_a.abs().max()) == 0.0 and float(d_b.abs().max()) == 0.0, "rows without slots are zeros"
    assert be.l1_mix_scores(q, t, t, z(0)).shape == (0, 8)
    assert be.gated_query_fwd("transE", t, zi(0), t, zi(0), z(0), t, zi(0), zi(0)).shape == (0, 8)
    q6, t6, w2, c2 = z(2, 6), z(7, 6), z(2), zi(2, 3)
    with pytest.raises(_lib.TempAmdError):
        be.l1_mix_ce_fwd(q6, t6, t6, w2, None, c2)
    with pytest.raises(_lib.TempAmdError):
        be.l1_mix_ce_bwd_q(q6, t6, t6, w2, None, c2, z(2, 3), z(2), z(1), 1.0)
    with pytest.raises(_lib.TempAmdError):
        be.l1_mix_ce_bwd_table(q6, t6, t6, w2, zi(8), zi(6), z(2, 3))
    with pytest.raises(_lib.TempAmdError):
        be.l1_mix_scores(q6, t6, t6, w2)
    with pytest.raises(_lib.TempAmdError):
        be.gated_query_fwd("transE", t6, zi(2), t6, zi(2), w2, t6, zi(2), zi(2))
    with pytest.raises(_lib.TempAmdError):
        be.gated_query_bwd("transE", t6, zi(2), t6, zi(2), w2, t6, zi(2), zi(2), q6)


@pytest.mark.parametrize("d", [8, 200, 260])
def test_gated_translation_query(d):
    """kind transE of temp_gated_query_fwd / _bwd under mixed is_tail and mixed temporal-only rows: q bit-equal to the mix followed
    by +-r; d_rel exact; d_a_rows / d_b_rows exact where the gate is 0 or 1 or the row temporal-only, inside 8 u of their terms
    elsewhere; d_w inside (d + 8) u sum |terms|, exactly 0 on temporal-only rows."""
    c = GC.gated_query_case(d)
    be = TB.get_backend()
    args = [dv(c[k]) for k in ("A", "ia", "B", "ib", "w", "rel", "ridx", "is_tail")]
    q = be.gated_query_fwd("transE", *args)
    assert torch.equal(q.cpu(), c["q"]), "q is not bit-equal to mix followed by +-r: %d elements differ" % int((q.cpu() != c["q"]).sum())
    da, db, dr, dw = (x.cpu() for x in be.gated_query_bwd("transE", *args, dv(c["d_q"])))
    assert torch.equal(dr.double(), c["d_rel"]), "d_rel = +-d_q exactly"
    ex = c["exact"]
    assert torch.equal(da[ex].double(), c["d_a"][ex]) and torch.equal(db[ex].double(), c["d_b"][ex]), "exact rows"
    assert bool((da.double() - c["d_a"]).abs().le(8 * U * c["d_a"].abs()).all()), "d_a_rows"
    assert bool((db.double() - c["d_b"]).abs().le(8 * U * c["d_b"].abs()).all()), "d_b_rows"
    assert bool((dw.double() - c["d_w"]).abs().le((d + 8) * U * c["a_w"]).all()), "d_w"
    assert float(dw[~c["gated"]].abs().max()) == 0.0 and float(da[~c["gated"]].abs().max()) == 0.0


@pytest.mark.parametrize("P,N,d,ld", GC.SCORE_CASES)
def test_gated_dense_scores_against_fp64(P, N, d, ld):
    """temp_l1_mix_scores inside (d + 2) u |s64| + 2 T; the pad columns -inf; bit-repeatable."""
    c = GC.gated_score_case(P, N, d)
    be = TB.get_backend()
    args = [dv(c[k]) for k in ("q", "table_a", "table_b", "w")]
    out = be.l1_mix_scores(*args)
    assert out.shape == (P, ld) and torch.equal(out, be.l1_mix_scores(*args))
    within(out[:, :N], c["s64"], c["tol"], "l1_mix_scores P=%d N=%d d=%d" % (P, N, d))
    assert ld == N or bool((out[:, N:] == float("-inf")).all()), "pad columns"


@pytest.mark.parametrize("P,N,d,ld", GC.SCORE_CASES[:2])
@pytest.mark.parametrize("filtered", [False, True])
def test_gated_ranks_inside_fp64_band(P, N, d, ld, filtered):
    """temp_filtered_rank over temp_l1_mix_scores, filtered and raw: every row's rank inside the fp64 band; at most 25 % of the rows
    have a band wider than one rank (checked without a GPU in tests/test_gated_transe_cpu.py as well)."""
    c = GC.gated_score_case(P, N, d)
    target, ptr, ids = TC.rank_inputs(P, N)
    if not filtered:
        ptr = ids = None
    lo, hi = TC.rank_band(c["s64"], c["tol"], target, ptr, ids)
    assert float((lo != hi).float().mean()) <= 0.25
    be = TB.get_backend()
    scores = be.l1_mix_scores(*[dv(c[k]) for k in ("q", "table_a", "table_b", "w")])
    ranks = be.filtered_rank(scores, dv(target), dv(ptr), dv(ids)).cpu()
    print("ranks: %d of %d rows ambiguous" % (int((lo != hi).sum()), P))
    assert bool(((ranks >= lo) & (ranks <= hi)).all()), (ranks, lo, hi)


@pytest.mark.parametrize("bi", [True, False])
def test_gated_transe_loss_definition_and_w_sqo_quirk_gpu(bi):
    """The fused node over several windows (one empty) against autograd of the fp64 restatement of the reference formula, and the
    quirk post_aggregation_cases pins for the bilinear scorers: w_sqo's gradient is exactly zero and perturbing it leaves the loss
    bit-identical."""
    PA.check_gated_loss_definition(DEV, "transE", bi)


# ---- model level ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Backend view that keeps the operands of the loss node's candidate launches (for the input conditions below)."""

    def __init__(self, be):
        self._be, self.mix, self.query, self.ce = be, None, [], []

    def __getattr__(self, name):
        return getattr(self._be, name)

    def l1_mix_ce_fwd(self, q, table_a, table_b, w, base, cand):
        self.mix = (q.detach(), table_a.detach(), table_b.detach(), w.detach().reshape(-1), base, cand)
        return self._be.l1_mix_ce_fwd(q, table_a, table_b, w, base, cand)

    def bilinear_query_fwd(self, kind, ent_rows, known_idx, rel, rel_idx, is_tail):
        self.query.append((ent_rows.detach(), known_idx, rel.detach(), rel_idx, is_tail))
        return self._be.bilinear_query_fwd(kind, ent_rows, known_idx, rel, rel_idx, is_tail)

    def l1_ce_fwd(self, q, table, base, cand):
        self.ce.append((table.detach(), base, cand))
        return self._be.l1_ce_fwd(q, table, base, cand)


def _recorded_forward(model, wb, samples, weights):
    rec = _Recorder(TB.get_backend())
    TB.set_backend(rec)
    try:
        with torch.no_grad():
            model.run_loss(wb, samples, weights)
    finally:
        TB.set_backend(rec._be)
    return rec


def _gated_near_zero_slots(rec):
    """(rows, C) bool over the recorded operands of the gated node, 256 rows at a time: the slots with a component of q - e inside
    the band of gated_transe_cases.near_zero_mask."""
    q, ta, tb, w, base, cand = rec.mix
    out = []
    for rows in torch.arange(q.shape[0], device=q.device).split(256):
        idx = cand[rows].long() + base[rows].long().view(-1, 1)
        out.append(GC.near_zero_mask(q[rows], w[rows], ta[idx], tb[idx]).any(dim=-1).cpu())
    return torch.cat(out)


def _ensemble_near_zero_slots(rec):
    """The head-mode condition of tests/test_gpu_transe.py on BOTH streams of the ensemble node, as a (rows, C) mask over all rows
    (tail rows never hinge on a rounding: both paths compute (s + r) - c)."""
    is_tail = rec.query[0][4]
    head = torch.nonzero(is_tail == 0).view(-1).cpu()
    bad = torch.zeros(is_tail.shape[0], rec.ce[0][2].shape[1], dtype=torch.bool)
    if head.numel():
        for query, ce in zip(rec.query, rec.ce):
            one = type("R", (), dict(query=query, ce=ce))
            bad[head] |= _near_zero_head_slots(one, DEV)
    return bad


def _condition_samples(model, wb, samples, weights, slots_of, rounds=8):
    """Seeded samples that meet the input condition of the comparison with the tensor path (see the callers): a negative whose
    slot has a component within rounding of zero is replaced by the next entity id, a positive whose TRUE candidate has one by
    the graph's next positive, until none is left (as tests/test_gpu_transe._condition_samples).  Stacked rows per graph: its tail
    rows, then its head rows.  -> (samples, slots redrawn); the caller asserts the condition on the result."""
    N, redrawn = model.num_ents, 0
    for _ in range(rounds):
        bad = slots_of(_recorded_forward(model, wb, samples, weights))
        if not bool(bad.any()):
            break
        redrawn += int(bad.sum())
        out, row = [], 0
        for trip, neg_tail, neg_head in samples:
            P = trip.shape[0]
            bt, bh = bad[row:row + P].to(neg_tail.device), bad[row + P:row + 2 * P].to(neg_head.device)
            row += 2 * P
            trip, neg_tail, neg_head = trip.clone(), neg_tail.clone(), neg_head.clone()
            for neg, b in ((neg_tail, bt), (neg_head, bh)):
                redraw = b.clone()
                redraw[:, 0] = False
                neg[redraw] = (neg[redraw] + 1) % N
            for i in torch.nonzero(bt[:, 0] | bh[:, 0]).view(-1).tolist():
                j = (i + 1) % P
                trip[i], neg_tail[i], neg_head[i] = trip[j], neg_tail[j], neg_head[j]
            out.append((trip, neg_tail, neg_head))
        samples = out
    return samples, redrawn


def _switch_to_transe(m, negative_rate=500):
    m.args.score_function = "transE"
    m.calc_score = SC.transE
    m.args.negative_rate = m.negative_rate = negative_rate


def _draw_samples(m, wb, z, seed):
    """The golden's positives with 500 uniform negatives per positive and side (column 0 = the true entity, global id)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for (trip, _, _), g in zip(window_inputs(z)[1], wb.graphs):
        P, K = trip.shape[0], m.args.negative_rate
        gid = torch.from_numpy(np.asarray(g.gids)).long()
        nt, nh = (torch.randint(0, m.num_ents, (P, K + 1), generator=gen) for _ in range(2))
        nt[:, 0], nh[:, 0] = gid[trip[:, 2]], gid[trip[:, 0]]
        out.append(tuple(x.to(DEV) for x in (trip, nt, nh)))
    return out


def _loss_properties(model, wb, samples, weights, rows, slots_of):
    """fused against fused_loss = False on the same samples and weights, after the bars of tests/test_gpu_transe._loss_properties:
    the input condition asserted, the loss within 2e-5 relative, every parameter's gradient and the injected weights' with
    assert_close(1e-4, 1e-5 max|ref|), bit-repeatable outputs, and the peak memory around run_loss below the tensor path's and
    below the bytes of one (rows, C, D) tensor."""
    C, D = model.args.negative_rate + 1, model.embed_size
    leaves = [w for ws in (weights or []) for w in ws if torch.is_tensor(w) and w.requires_grad]

    def run(fused):
        model.fused_loss = fused
        for p in list(model.parameters()) + leaves:
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = model.run_loss(wb, samples, weights)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        loss.backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        grads.update({"weight %d" % i: w.grad.clone() for i, w in enumerate(leaves)})
        return loss.detach().clone(), grads, peak

    near = int(slots_of(_recorded_forward(model, wb, samples, weights)).sum())
    print("slots with a component within 2^-20 of zero: %d" % near)
    assert near == 0, "input condition: %d slots have a component within rounding of zero" % near
    la, ga, _ = run(True)                                    # (first call: the caches of the sample set fill)
    lb, gb, peak = run(True)
    assert torch.equal(la, lb) and sorted(ga) == sorted(gb) and all(torch.equal(ga[k], gb[k]) for k in ga), "not bitwise repeatable"
    lr, gr, peak_ref = run(False)
    model.fused_loss = True
    one_tensor = rows * C * D * 4
    print("peak delta around run_loss: fused %.1f MB, tensor path %.1f MB; one (rows, C, D) tensor %.1f MB"
          % (peak / 2 ** 20, peak_ref / 2 ** 20, one_tensor / 2 ** 20))
    assert peak < peak_ref, "the fused loss does not allocate less than the tensor path"
    assert peak < one_tensor, "the fused loss allocates as much as a (rows, C, D) tensor"
    assert abs(la.item() - lr.item()) < 2e-5 * abs(lr.item()), (la.item(), lr.item())
    assert sorted(ga) == sorted(gr), (sorted(ga), sorted(gr))
    for k in gr:
        assert_close(ga[k], gr[k], 1e-4, 1e-5 * float(gr[k].abs().max()), k + ", fused vs tensor path")
    return ga


def _count_calls(names, fn):
    be = TB.get_backend()
    calls = {}
    for nm in names:
        orig = getattr(be, nm)

        def wrap(*a, _nm=nm, _orig=orig, **k):
            calls[_nm] = calls.get(_nm, 0) + 1
            return _orig(*a, **k)
        setattr(be, nm, wrap)
    try:
        fn()
    finally:
        for nm in names:
            be.__dict__.pop(nm, None)
    return calls


@pytest.mark.parametrize("name", ["G20_post_agg_uni", "G20_post_agg_bi"])
def test_post_aggregation_transe_loss_gpu(name):
    """PostDynamicRGCN / PostBiDynamicRGCN (G20's small models switched to transE, 500 negatives): run_loss fused against the tensor
    path on the same samples -- once with injected gates (the gradients of all four gate tensors) and once with the model's own
    gate MLPs (their gradients) -- under the input condition that no component of q - e lies within
    2^-20 (|q| + |w a| + |(1 - w) b|) of zero unless it is exactly zero; one call of each gated entry point per step."""
    z = load(name)
    m = PA.load_golden_model(z, DEV, True)
    _switch_to_transe(m)
    edge_ids, _ = window_inputs(z)
    wb = m.prepare(torch.tensor([int(t) for t in z["t_list"]]), int(z["L"]), True, edge_ids)
    samples = _draw_samples(m, wb, z, 11)
    rows = sum(2 * s[0].shape[0] for s in samples)
    gen = torch.Generator().manual_seed(12)
    gates = [tuple(torch.rand(s[0].shape[0], 1, generator=gen).to(DEV).requires_grad_(True) for _ in range(4)) for s in samples]
    assert m._gated_fused_ok()
    for weights in (gates, None):
        cond, redrawn = _condition_samples(m, wb, samples, weights, _gated_near_zero_slots)
        print("%s, %s gates: %d slots redrawn" % (name, "injected" if weights is not None else "own", redrawn))
        grads = _loss_properties(m, wb, cond, weights, rows, _gated_near_zero_slots)
        if weights is not None:
            assert all("weight %d" % i in grads for i in range(4 * len(samples))), sorted(grads)
            assert all(float(grads["weight %d" % (4 * b + 1)].abs().max()) == 0.0 for b in range(len(samples))), "w_sqo gradient"
        else:
            assert any(k.startswith("subject_query_subject_embed_linear") for k in grads)
            assert any(k.startswith("object_query_subject_embed_linear") for k in grads)
            assert not any("_object_embed_linear" in k for k in grads)
        calls = _count_calls(("gated_query_fwd", "gated_query_bwd", "l1_mix_ce_fwd", "l1_mix_ce_bwd_q", "l1_mix_ce_bwd_table", "l1_ce_fwd",
                              "gather_ce_mix_fwd"), lambda: m.run_loss(wb, cond, weights).backward())
        assert calls == {"gated_query_fwd": 1, "gated_query_bwd": 1, "l1_mix_ce_fwd": 1, "l1_mix_ce_bwd_q": 1, "l1_mix_ce_bwd_table": 1}, calls


@pytest.mark.parametrize("name,cls", [("G19_post_ratio_uni", "PostEnsembleDynamicRGCN"), ("G19_post_ratio_bi", "PostEnsembleBiDynamicRGCN")])
def test_post_ensemble_transe_loss_gpu(name, cls):
    """PostEnsembleDynamicRGCN / PostEnsembleBiDynamicRGCN with transE and 500 negatives: the per-stream L1 kernels with the mix on
    the (rows, C) scores against the tensor path, same bars, the gradient of the injected ensemble weights included."""
    from temp_amd import post_dynamic_rgcn as PD
    z = load(name)
    torch.manual_seed(3)
    m = build_post_model(z, DEV, getattr(PD, cls), True, post_ensemble=True)
    _switch_to_transe(m)
    edge_ids, _ = window_inputs(z)
    wb = m.prepare(torch.tensor([int(t) for t in z["t_list"]]), int(z["L"]), True, edge_ids)
    samples = _draw_samples(m, wb, z, 21)
    rows = sum(2 * s[0].shape[0] for s in samples)
    gen = torch.Generator().manual_seed(22)
    weights = [tuple(torch.rand(s[0].shape[0], 1, generator=gen).to(DEV).requires_grad_(True) for _ in range(2)) for s in samples]
    cond, redrawn = _condition_samples(m, wb, samples, weights, _ensemble_near_zero_slots)
    print("%s: %d slots redrawn" % (name, redrawn))
    grads = _loss_properties(m, wb, cond, weights, rows, _ensemble_near_zero_slots)
    assert all("weight %d" % i in grads and float(grads["weight %d" % i].abs().max()) > 0 for i in range(2 * len(samples)))
    calls = _count_calls(("l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table", "gather_ce_fwd"), lambda: m.run_loss(wb, cond, weights).backward())
    assert calls == {"l1_ce_fwd": 2, "l1_ce_bwd_q": 2, "l1_ce_bwd_table": 2}, calls


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
class _NoMixScores:
    """Backend view without temp_l1_mix_scores: what forces PostEvaluationFilter's chunked literal route."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name == "l1_mix_scores":
            raise AttributeError(name)
        return getattr(self._be, name)


def test_post_evaluation_filter_route_against_chunked_gpu():
    """PostEvaluationFilter.calc_metrics_single_graph with transE on the icews14 slice (D = 16, for which the fp64 reference leaves
    under 25 % of the rows ambiguous): the l1_mix_scores route (two calls, one per mode) against the chunked broadcast route --
    equal ranks on every row whose fp64 band is one rank wide, inside the band elsewhere."""
    from temp_amd.evaluation import PostEvaluationFilter
    s = slice_snapshots()
    t = s["times"][14]
    g = s["va"][t]
    N, D = s["num_e"], 16
    torch.manual_seed(5)
    all_e = torch.randn(N, D) * 0.5
    rel = torch.randn(2 * s["num_r"], D) * 0.5
    ent = all_e[torch.from_numpy(g.gids)]
    samples = torch.from_numpy(np.stack([g.src, g.rel, g.dst], axis=1))
    gen = torch.Generator().manual_seed(9)
    all_r, ent_r = all_e + 0.3 * torch.randn(all_e.shape, generator=gen), ent + 0.3 * torch.randn(ent.shape, generator=gen)
    P = samples.shape[0]
    ws = [torch.rand(P, 1, generator=gen) for _ in range(4)]
    ev = PostEvaluationFilter(make_args(score_function="transE"), SC.transE, s["tr"], s["va"], s["te"])
    be = TB.get_backend()
    args = [dv(x) for x in (ent, ent_r, rel, all_e, all_r, samples)] + [dv(w) for w in ws]
    out = {}
    calls = _count_calls(("l1_mix_scores",), lambda: out.setdefault("new", ev.calc_metrics_single_graph(*args, g, t).cpu()))
    assert calls == {"l1_mix_scores": 2}, calls
    new = out["new"]
    TB.set_backend(_NoMixScores(be))
    try:
        old = ev.calc_metrics_single_graph(*args, g, t).cpu()
    finally:
        TB.set_backend(be)
    lo, hi = GC.post_eval_band(ev, samples, g, t, N, ent, ent_r, rel, all_e, all_r, ws, device=DEV)
    sure = lo == hi
    print("evaluation: %d of %d rows ambiguous" % (int((~sure).sum()), 2 * P))
    assert float((~sure).float().mean()) <= 0.25
    assert torch.equal(new[sure], old[sure]) and torch.equal(new[sure], lo[sure])
    assert bool(((new >= lo) & (new <= hi)).all()) and bool(((old >= lo) & (old <= hi)).all())
