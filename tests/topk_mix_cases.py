"""Cases of the mixed filtered top-k selection (include/temp_amd.h: temp_filtered_topk_mix), of the two mixed filters'
topk_single_graph and of predict_gated, shared by the CPU (test backends: the composite route, mixed_scores + topk_composite) and
GPU (HIP kernel) suites.  The helpers and conventions are tests/topk_cases.py's.

  * selection cases: two score matrices drawn as multiples of 2^-3 in [-1, 1] from different seeds and row weights that are
    multiples of 2^-3 in [0, 1]: w a and (1 - w) b are multiples of 2^-6 below 2 in magnitude and so is their sum, so every product
    and the sum are exact in fp32 under any contraction, and the kernel must equal mixed_scores + topk_composite in ids AND values.
    Row 1 of a has -inf in every third column, row 3 of b in every fifth; rows 1, 2, 3 carry the weights 0, 1, 1, so a naive mix
    meets 0 * inf in rows 1 and 3 -- the case the admissibility rule exists for;
  * evaluater cases: integer tables for both streams and weights in {0, 1/4, 1/2, 3/4, 1}: every score, every mixed known row
    and every mix is a multiple of 1/16 far below 2^24 / 16, exact on every route;
  * model cases: predict_gated of a freshly initialised model on the ICEWS14 slice against the fp64 gated scores of its own
    all_entity_table_pairs, inside the band of topk_cases.band_check with the bounds derived at ensemble_bound / aggregation_bound."""
import types

import numpy as np
import pytest
import torch

from temp_amd import scores as SC
from temp_amd.evaluation import EvaluationFilter, PostEnsembleEvaluationFilter, PostEvaluationFilter, mixed_scores, topk_composite
from tests import topk_cases as KC

NINF, U = KC.NINF, KC.U
K_VALUES = (1, 10, 256)
N_VALUES = KC.N_VALUES                      # 3, 4, 1023, 1024, 1025 (the pruning threshold), 4100 (past the 4096-column chunk)
FILTERS = KC.FILTERS
SCORERS = {"distmult": SC.distmult, "complex": SC.complex, "transE": SC.transE}


# ---------------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------------
_MIX = {}


def mix_inputs(P, N, finite=False):
    """(a, b [P, ld] float32, w [P] float32, mixed [P, ld] = mixed_scores(a, b, w)), computed once per shape and shared: callers
    must not modify them.  ld = N rounded up to a multiple of 4 plus 4, +inf behind column N in both matrices (those columns must
    never reach a result).  finite: no -inf inside N (the identity cases)."""
    key = (P, N, finite)
    if key not in _MIX:
        ld = (N + 3) // 4 * 4 + 4
        mats = []
        for seed in (1, 2):
            g = torch.Generator().manual_seed(100003 * P + 17 * N + seed)
            s = torch.full((P, ld), float("inf"))
            s[:, :N] = torch.randint(-8, 9, (P, N), generator=g).float() / 8.0
            mats.append(s)
        a, b = mats
        if not finite:
            if P > 1:
                a[1, 0:N:3] = NINF
            if P > 3:
                b[3, 0:N:5] = NINF
        w = (torch.tensor([3, 0, 8, 8, 5, 1, 7, 2])[torch.arange(P) % 8]).float() / 8.0
        _MIX[key] = (a, b, w, mixed_scores(a, b, w))
    return _MIX[key]


def brute_mixed(a, b, w, N):
    """The mixed row entity by entity in python floats (exact for the fixtures): [P, N] float64, -inf where either operand is."""
    P = a.shape[0]
    m = torch.full((P, N), NINF, dtype=torch.float64)
    for p in range(P):
        wp = float(w[p])
        for j in range(N):
            x, y = float(a[p, j]), float(b[p, j])
            if x != NINF and y != NINF:
                m[p, j] = wp * x + (1.0 - wp) * y
    return m


def dead_columns(a, b, N):
    return (a[:, :N] == NINF) | (b[:, :N] == NINF)


def check_selection(select, to_dev, k, N):
    """Five rows under every filter variant with and without keep: ids and values equal mixed_scores + topk_composite, twice; no
    NaN and no column that is -inf in either operand comes back."""
    P = 5
    a, b, w, mixed = mix_inputs(P, N)
    a_d, b_d, w_d = to_dev(a), to_dev(b), to_dev(w)
    dead = dead_columns(a, b, N)
    assert bool(dead[1].any()) and bool(dead[3].any()) and float(w[1]) == 0.0 and float(w[3]) == 1.0
    for kind in FILTERS:
        for with_keep in (False, True):
            ptr, ids, keep = KC.filter_lists(kind, mixed, N, with_keep)           # "top": the 12 best of the MIXED scores
            want = topk_composite(mixed, k, ptr, ids, keep, n=N)
            what = "k=%d N=%d %s keep=%s" % (k, N, kind, with_keep)
            got = select(a_d, b_d, w_d, k, to_dev(ptr), to_dev(ids), to_dev(keep), n=N)
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
            val, idx = got[0].cpu(), got[1].cpu()
            assert not bool(torch.isnan(val).any()), what + ": NaN"
            rows = torch.arange(P).view(-1, 1).expand_as(idx)
            assert not bool(dead[rows[idx >= 0], idx[idx >= 0]].any()), what + ": a -inf column returned"
            assert torch.equal(idx, want[1]), what + ": ids"
            assert torch.equal(val, want[0]), what + ": values"
            assert KC.ordered(val, idx), what
            again = select(a_d, b_d, w_d, k, to_dev(ptr), to_dev(ids), to_dev(keep), n=N)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), what + ": not bit-repeatable"
            if kind == "all" and not with_keep:
                assert bool((idx == -1).all()) and bool((val == NINF).all())


def check_panels(select, plain, to_dev, width, order, alternate=False):
    """The same pair of matrices in one call and in column panels (pointer slices with the wide ld and matching col0) in the given
    order: equal, bit for bit.  alternate: every second panel goes through the PLAIN selection fed the torch-mixed slice -- lists of
    either entry point merge."""
    P, N = 5, 4100
    a, b, w, mixed = mix_inputs(P, N)
    a_d, b_d, w_d, m_d = to_dev(a), to_dev(b), to_dev(w), to_dev(mixed)
    for k in (10, 256):
        ptr, ids, keep = KC.filter_lists("top", mixed, N, True)
        want = topk_composite(mixed, k, ptr, ids, keep, n=N)
        f = (to_dev(ptr), to_dev(ids), to_dev(keep))
        one = select(a_d, b_d, w_d, k, *f, n=N)
        assert torch.equal(one[1].cpu(), want[1]) and torch.equal(one[0].cpu(), want[0]), "one call k=%d" % k
        carry = None
        for i, (c0, c1) in enumerate(KC.panels(N, width, order)):
            if alternate and i % 2:
                carry = plain(m_d[:, c0:], k, *f, col0=c0, n=c1 - c0, carry=carry)
            else:
                carry = select(a_d[:, c0:], b_d[:, c0:], w_d, k, *f, col0=c0, n=c1 - c0, carry=carry)
        what = "panels of %d, %s, k=%d, alternate=%s" % (width, order, k, alternate)
        assert torch.equal(carry[1].cpu(), want[1]), what + ": ids"
        assert torch.equal(carry[0].cpu(), want[0]), what + ": values"


def check_identity(select, plain, to_dev):
    """Finite operands: w = 1 is the plain selection over a, w = 0 the plain selection over b, bit for bit."""
    P = 5
    for N in (1025, 4100):
        a, b, _, _ = mix_inputs(P, N, finite=True)
        a_d, b_d = to_dev(a), to_dev(b)
        ptr, ids, keep = KC.filter_lists("top", a, N, True)
        f = (to_dev(ptr), to_dev(ids), to_dev(keep))
        for k in (10, 256):
            for wv, src in ((1.0, a_d), (0.0, b_d)):
                got = select(a_d, b_d, to_dev(torch.full((P,), wv)), k, *f, n=N)
                want = plain(src, k, *f, n=N)
                assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), "w=%g N=%d k=%d" % (wv, N, k)


# ---------------------------------------------------------------------------------------------------------------------
# evaluater level
# ---------------------------------------------------------------------------------------------------------------------
def _quarters(Q, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 5, Q) / 4.0).float()


def gated64(name, loc, rec, rel_rows, known, rel, w_known, w_cand, mode):
    """fp64 scores of the embedding-level gate, literally: the mixed known row against every mixed candidate -> [Q, N]."""
    l64, r64 = loc.double().cpu(), rec.double().cpu()
    wk, wc = w_known.double().cpu().view(-1, 1), w_cand.double().cpu().view(-1, 1, 1)
    ki = torch.as_tensor(known)
    kn = wk * l64[ki] + (1 - wk) * r64[ki]
    cand = wc * l64.unsqueeze(0) + (1 - wc) * r64.unsqueeze(0)
    rr = rel_rows.double().cpu()[torch.as_tensor(rel)]
    fn = SCORERS[name]
    return fn(kn, rr, cand, mode="tail") if mode == "tail" else fn(cand, rr, kn, mode="head")


def ensemble64(name, loc, rec, rel_rows, known, rel, w, mode):
    """fp64 scores of the score-level ensemble -> [Q, N]."""
    wc = w.double().cpu().view(-1, 1)
    return wc * KC.scores64(name, loc, rel_rows, known, rel, mode) + (1 - wc) * KC.scores64(name, rec, rel_rows, known, rel, mode)


def transe_gated_bound(loc, rec, rel_rows, known, rel, w_known, w_cand, mode, s64):
    """tol [Q, N] of the gated TransE score through temp_l1_mix_scores, u = 2^-24 (tests/gated_transe_cases.py: (d + 2) u |s64| +
    2 T for a query given in fp32, T = sum_d 3 u (|w a| + |(1 - w) b|) the three roundings of the candidate mix), plus the query's
    own roundings: the mixed known row in torch is four roundings (w a, 1 - w, (1 - w) b, the sum) of terms bounded by
    kabs = w |a| + (1 - w) |b|, and q = known +- r is one more: Tq = sum_d (4 u kabs + u (kabs + |r|)), the same for every
    candidate."""
    la, ra = loc.double().cpu().abs(), rec.double().cpu().abs()
    wk, wc = w_known.double().cpu().view(-1, 1), w_cand.double().cpu().view(-1, 1)
    ki = torch.as_tensor(known)
    kabs = wk * la[ki] + (1 - wk) * ra[ki]
    rr = rel_rows.double().cpu().abs()[torch.as_tensor(rel)]
    d = loc.shape[1]
    T = 3 * U * (wc * la.sum(dim=1).view(1, -1) + (1 - wc) * ra.sum(dim=1).view(1, -1))
    Tq = (4 * U * kabs + U * (kabs + rr)).sum(dim=1, keepdim=True)
    return (d + 2) * U * s64.abs() + 2 * T + Tq


def check_evaluater(device, family, name, N, d, mode, filtered, panel, k=10):
    """topk_single_graph of a mixed filter on integer tables == topk_composite on the fp64 mixed scores and the triple-by-triple
    filter, exactly; TransE through the embedding-level gate inside the fp64 band with transe_gated_bound (no cap on ambiguous
    rows here: integer scores tie at the k-th place by construction)."""
    R = 5
    splits = KC.synthetic_splits(N)
    loc, rel_rows = KC.integer_tables(N, d, R + 1, seed=0)
    rec, _ = KC.integer_tables(N, d, R + 1, seed=1)
    assert not torch.equal(loc, rec)
    args = types.SimpleNamespace(score_function=name)
    cls = PostEnsembleEvaluationFilter if family == "ensemble" else PostEvaluationFilter
    ev = cls(args, SCORERS[name], *splits)
    for time in (0, 3, 4):
        known, rel = KC.queries_at(splits, time, R)
        Q = known.shape[0]
        keep = np.full(Q, -1, dtype=np.int64)
        sets = KC.true_sets(splits, time, known, rel, mode)
        assert sum(len(x) for x in sets) > 0
        for i in range(0, Q, 4):
            if sets[i]:
                keep[i] = sorted(sets[i])[0]
        w1, w2 = _quarters(Q, 11 + time), _quarters(Q, 23 + time)
        assert 0.0 in w1.tolist() and 1.0 in w1.tolist()
        if family == "ensemble":
            s64, gates = ensemble64(name, loc, rec, rel_rows, known, rel, w1, mode), (w1.to(device),)
        else:
            s64, gates = gated64(name, loc, rec, rel_rows, known, rel, w1, w2, mode), (w1.to(device), w2.to(device))
        ptr, ids = KC.sets_to_csr(sets) if filtered else (None, None)
        got_idx, got_val = ev.topk_single_graph(loc.to(device), rec.to(device), rel_rows.to(device), known, rel, *gates, mode, time, k,
                                                filtered=filtered, keep=keep if filtered else None, panel=panel)
        assert got_idx.dtype == torch.int64 and got_val.dtype == torch.float32 and tuple(got_idx.shape) == (Q, k)
        what = "%s %s N=%d %s filtered=%s panel=%s t=%d" % (family, name, N, mode, filtered, panel, time)
        if family == "aggregation" and name == "transE":
            tol = transe_gated_bound(loc, rec, rel_rows, known, rel, w1, w2, mode, s64)
            adm = s64.clone()
            if filtered:                         # the kept id stays admissible: take it out of the list the band check masks with
                kept = [set(x) - {int(keep[i])} for i, x in enumerate(sets)]
                ptr, ids = KC.sets_to_csr(kept)
            KC.band_check(adm, tol, k, got_val, got_idx, ptr, ids, what)
        else:
            want_val, want_idx = topk_composite(s64, k, ptr, ids, torch.from_numpy(keep) if filtered else None)
            assert torch.equal(got_idx.cpu(), want_idx), what
            assert torch.equal(got_val.cpu().double(), want_val), what
        if filtered:
            hit = [int(e) for i, x in enumerate(sets) for e in got_idx[i].tolist() if e in x and e != keep[i]]
            assert not hit, what + ": a known-true entity returned"
    return ev


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
MODELS = ("PostEnsembleGRRGCN", "PostBiGRRGCN", "PostSARGCN")
TIMES = [20, 9, 15]


def build_model(kind, device, score_function="complex", seed=5):
    from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN, PostEnsembleDynamicRGCN
    from temp_amd.post_self_attention_rgcn import PostSelfAttentionRGCN
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    cls, kw = {"PostEnsembleGRRGCN": (PostEnsembleDynamicRGCN, dict(module="GRRGCN", post_ensemble=True)),
               "PostBiGRRGCN": (PostBiDynamicRGCN, dict(module="BiGRRGCN", post_aggregation=True)),
               "PostSARGCN": (PostSelfAttentionRGCN, dict(module="SARGCN", post_aggregation=True, EMA=False))}[kind]
    torch.manual_seed(seed)
    m = cls(make_args(score_function=score_function, train_seq_len=3, test_seq_len=3, rec_only_last_layer=True, **kw),
            s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(device)
    with torch.no_grad():                       # as topk_cases.build_model: the init's entries give scores of 1e-4
        m.ent_embeds.mul_(8.0)
        m.rel_embeds.mul_(8.0)
    return m.eval(), s


def injected_weights(m, Q, seed=2):
    g = torch.Generator().manual_seed(seed)
    w = tuple(torch.rand(Q, generator=g) for _ in range(m._gate_count))
    return w[0] if m._gate_count == 1 else w


def _fold_abs(name, k, r, d):
    """|terms| of the folded bilinear query of |known| = k and |relation| = r (topk_cases.bilinear_bound)."""
    if name == "distmult":
        return k * r
    h = d // 2
    return torch.cat([k[:, :h] * r[:, :h] + k[:, h:] * r[:, h:], k[:, :h] * r[:, h:] + k[:, h:] * r[:, :h]], dim=1)


C_DOT = lambda d: max((d + 8) * U, 1e-6 + 4 * U)       # topk_cases.bilinear_bound's factor of one fp32 score of a rounded query


def _mix_bound(w, b_a, b_b, s_a, s_b):
    """Bound of the mix w a + (1 - w) b of two fp32 scores a, b within b_a, b_b of their fp64 values s_a, s_b: the inherited
    w b_a + (1 - w) b_b, and the mix's own roundings -- at most four on a term whichever route forms it (the kernel's
    fmaf(w, a, (1 - w) * b): 1 - w, the product, the fused sum; the composite's w * a + (1 - w) * b: one more product) -- each
    relative u of a partial result bounded by w (|s_a| + b_a) + (1 - w) (|s_b| + b_b)."""
    return w * b_a + (1 - w) * b_b + 4 * U * (w * (s_a.abs() + b_a) + (1 - w) * (s_b.abs() + b_b))


def ensemble_bound(name, loc, rec, rel_rows, known, rel, w, mode):
    """tol [Q, N] of the score-level ensemble: topk_cases.bilinear_bound of each stream's score, mixed by _mix_bound."""
    d = loc.shape[1]
    wc = w.double().cpu().view(-1, 1)
    return _mix_bound(wc, KC.bilinear_bound(name, loc, rel_rows, known, rel, mode, d), KC.bilinear_bound(name, rec, rel_rows, known, rel, mode, d),
                      KC.scores64(name, loc, rel_rows, known, rel, mode), KC.scores64(name, rec, rel_rows, known, rel, mode))


def aggregation_scores_and_bound(name, loc, rec, rel_rows, known, rel, w_known, w_cand, mode):
    """(s64, tol) [Q, N] of the embedding-level gate with a bilinear scorer.  The known row kn = w_known loc + (1 - w_known) rec is
    formed in fp32 by torch: four roundings (w a, 1 - w, (1 - w) b, the sum), |kn32 - kn64| <= 4 u kabs per component, kabs =
    w |loc| + (1 - w) |rec|.  A bilinear score is linear in the known row, so against one table with rows t that costs at most
    4 u (fold(kabs, |r|) . |t|), and the fp32 evaluation of the folded query of kn32 (|kn32| <= (1 + 4 u) kabs) costs
    topk_cases.bilinear_bound's factor C_DOT(d) of the same sum: per table B = (C_DOT(d) (1 + 4 u) + 4 u) fold(kabs, |r|) . |t|.  The
    candidate mix of the two score matrices is _mix_bound's."""
    d = loc.shape[1]
    l64, r64 = loc.double().cpu(), rec.double().cpu()
    wk, wc = w_known.double().cpu().view(-1, 1), w_cand.double().cpu().view(-1, 1)
    ki = torch.as_tensor(known)
    kn = wk * l64[ki] + (1 - wk) * r64[ki]
    kabs = wk * l64[ki].abs() + (1 - wk) * r64[ki].abs()
    rr = rel_rows.double().cpu()[torch.as_tensor(rel)]
    fn = SCORERS[name]
    s = [fn(kn, rr, t, mode="tail") if mode == "tail" else fn(t, rr, kn, mode="head") for t in (l64, r64)]
    qa = _fold_abs(name, kabs, rr.abs(), d)
    bnd = [(C_DOT(d) * (1 + 4 * U) + 4 * U) * (qa @ t.abs().t()) for t in (l64, r64)]
    return wc * s[0] + (1 - wc) * s[1], _mix_bound(wc, bnd[0], bnd[1], s[0], s[1])


def model_queries(s, mode):
    """KC.model_queries names the SUBJECTS of test triples; a head query names an object."""
    q = KC.model_queries(s, TIMES)
    if mode == "head":
        rng = np.random.default_rng(0)
        rows = []
        for t in TIMES:
            g = s["te"][t]
            pick = rng.choice(g.number_of_edges(), 6, replace=False)
            rows += [(t, int(g.gids[g.dst[i]]), int(g.rel[i])) for i in pick]
        rows = np.array(rows, dtype=np.int64)
        q = rows[np.argsort(np.arange(len(rows)) % 6, kind="stable")]
    return q


def table_pairs(m):
    with torch.no_grad():
        pairs = {int(t): (a.detach().cpu(), b.detach().cpu()) for t, a, b in m.all_entity_table_pairs(sorted(TIMES))}
    assert sorted(pairs) == sorted(TIMES)
    return pairs


def check_predict_gated(kind, device, score_function="complex", k=10):
    """predict_gated with injected random weights against the fp64 gated scores of the model's own table pairs: tail and head,
    filtered and raw, inside the fp64 band; permuted queries come back in the permuted order bit for bit; the filtered lists name
    no known-true entity; at most 0.25 of a timestamp's rows ambiguous (a condition on the inputs: the CPU suite runs the same
    cases)."""
    m, s = build_model(kind, device, score_function)
    splits = (s["tr"], s["va"], s["te"])
    pairs = table_pairs(m)
    assert all(tuple(x.shape) == (s["num_e"], m.rel_embeds.shape[1]) for p in pairs.values() for x in p)
    rel_rows = m.rel_embeds.detach().cpu()
    worst = 0.0
    for mode in ("tail", "head"):
        q = model_queries(s, mode)
        weights = injected_weights(m, q.shape[0])
        wt = (weights,) if torch.is_tensor(weights) else weights
        for filtered in (True, False):
            ids, vals = m.predict_gated(q, mode=mode, k=k, filtered=filtered, weights=weights)
            assert tuple(ids.shape) == tuple(vals.shape) == (q.shape[0], k) and ids.dtype == torch.int64 and vals.dtype == torch.float32
            perm = np.random.default_rng(1).permutation(q.shape[0])
            pt = torch.from_numpy(perm)
            p_w = weights[pt] if torch.is_tensor(weights) else tuple(w[pt] for w in weights)
            p_ids, p_vals = m.predict_gated(q[perm], mode=mode, k=k, filtered=filtered, weights=p_w)
            sel = pt.to(ids.device)
            assert torch.equal(p_ids, ids[sel]) and torch.equal(p_vals, vals[sel]), "%s %s filtered=%s: query order" % (kind, mode, filtered)
            for t in TIMES:
                rows = np.nonzero(q[:, 0] == t)[0]
                loc, rec = pairs[t]
                w_rows = [w[torch.from_numpy(rows)] for w in wt]
                if m._gate_count == 1:
                    s64 = ensemble64(score_function, loc, rec, rel_rows, q[rows, 1], q[rows, 2], w_rows[0], mode)
                    tol = ensemble_bound(score_function, loc, rec, rel_rows, q[rows, 1], q[rows, 2], w_rows[0], mode)
                else:
                    s64, tol = aggregation_scores_and_bound(score_function, loc, rec, rel_rows, q[rows, 1], q[rows, 2], *w_rows, mode)
                sets = KC.true_sets(splits, t, q[rows, 1], q[rows, 2], mode)
                ptr, fid = KC.sets_to_csr(sets) if filtered else (None, None)
                what = "%s %s %s filtered=%s t=%d" % (kind, score_function, mode, filtered, t)
                worst = max(worst, KC.band_check(s64, tol, k, vals[rows], ids[rows], ptr, fid, what))
                if filtered:
                    assert all(len(x) > 0 for x in sets), "the test triples' own answers are known-true"
                    assert not any(set(ids[r].tolist()) & sets[i] for i, r in enumerate(rows)), what + ": a known-true entity returned"
    print("%s: at most %.2f of a timestamp's rows ambiguous" % (kind, worst))
    assert worst <= 0.25
    return m, s


def check_weight_extremes(kind, device):
    """Injected w = 1 is EvaluationFilter.topk_single_graph over all_loc alone, w = 0 over all_rec alone, ids and values (for the
    embedding-level gate w_known = w_cand)."""
    m, s = build_model(kind, device)
    q = model_queries(s, "tail")
    Q = q.shape[0]
    base = EvaluationFilter(m.args, m.calc_score, m.graph_dict_train, m.graph_dict_val, m.graph_dict_test)
    with torch.no_grad():
        pairs = {int(t): (a, b) for t, a, b in m.all_entity_table_pairs(sorted(TIMES))}
    for mode in ("tail", "head"):
        for wv, which in ((1.0, 0), (0.0, 1)):
            w = torch.full((Q,), wv)
            ids, vals = m.predict_gated(q, mode=mode, k=10, weights=w if m._gate_count == 1 else (w, w))
            for t in TIMES:
                rows = np.nonzero(q[:, 0] == t)[0]
                i, v = base.topk_single_graph(pairs[t][which], m.rel_embeds, q[rows, 1], q[rows, 2], mode, t, 10)
                assert torch.equal(ids[rows], i) and torch.equal(vals[rows], v), "%s %s w=%g t=%d" % (kind, mode, wv, t)


def own_gates(m, q, mode, crossed=False):
    """The model's own weights of queries q, computed here from frequency_tables().features and the MLPs the training loss pairs
    with the mode: the object MLP(s) on the object features for a tail query, the subject MLP(s) on the subject features for a
    head query.  crossed: the OTHER side's MLP on the same features."""
    dev = m.rel_embeds.device
    ws = torch.zeros(q.shape[0], device=dev)
    if m._gate_count == 1:
        mlp = m.object_linear if (mode == "tail") != crossed else m.subject_linear
    else:
        mlp = m.object_query_subject_embed_linear if (mode == "tail") != crossed else m.subject_query_subject_embed_linear
    for t in sorted(set(q[:, 0].tolist())):
        rows = np.nonzero(q[:, 0] == t)[0]
        sub_f, obj_f = m.frequency_tables().features(t, q[rows, 1], q[rows, 2], q[rows, 1])
        f = torch.from_numpy(obj_f if mode == "tail" else sub_f).to(dev)
        assert float(f.abs().sum()) > 0, "the queries' known sides occur in the train window"
        with torch.no_grad():
            ws[torch.from_numpy(rows).to(dev)] = torch.sigmoid(mlp(f)).reshape(-1)
    return ws


def check_own_gates(kind, device):
    """weights=None == the call with the weights computed in the test; for the score-level ensemble the tail weights are
    object_linear's, not subject_linear's; the state dict is unchanged by the calls; predict() still refuses."""
    m, s = build_model(kind, device)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for mode in ("tail", "head"):
        q = model_queries(s, mode)
        w = own_gates(m, q, mode)
        got = m.predict_gated(q, mode=mode, k=10)
        want = m.predict_gated(q, mode=mode, k=10, weights=w if m._gate_count == 1 else (w, w))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "%s %s" % (kind, mode)
        if m._gate_count == 1 and mode == "tail":                 # object_linear's weights, which subject_linear's are far from
            assert float((own_gates(m, q, mode, crossed=True) - w).abs().max()) > 1e-3
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    with pytest.raises(NotImplementedError, match="two all-entity tables"):
        m.predict(model_queries(s, "tail"))
