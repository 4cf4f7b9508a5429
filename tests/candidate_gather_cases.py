"""Cases of the candidate-gather route of the bilinear scorers shared by the CPU (test backend) and GPU (HIP) suites: seeded inputs,
fp64 references and bounds of the dot candidate kernels (temp_dot_ce_* / temp_dot_mix_ce_*, include/temp_amd.h), hand-built loss plans
for the three batched nodes with their literal fp64 expressions, and the model checks.  Every function runs under the backend that the
calling suite installed.

The kernel references take q, the table(s) and w as GIVEN fp32 data and compute in fp64.  Bounds (u = 2^-24), derived, not measured:
  score     d products and a d-term sum in any order, on the sum of absolute terms because the terms are signed:
              |s - s64| <= (d + 2) u sum_d |q_d e_d|
  lse/loss  2 max_k tol_s[p, k] + (C + 8) u
  gradient  per output element, A = the fp64 sum of the absolute values of its additive terms (scale w softmax_k x and
            scale w [k == 0] x, x = e_kj for d_q and q_pj for d_table, each counted on its own):
              |err| <= eps A,  eps = 2 max tol_s + (C + L + 18) u,  L = the longest slot list
            (the L1 kernels' bound, tests/transe_cases.py, plus one rounding for the product g e resp. g q and one for its fused add)
  mix       e = fmaf(w, a, (1 - w) * b) carries THREE roundings per element (1 - w, its product with b, the fused add):
              tau_e = 3 u (|w a| + |(1 - w) b|) per component, and the score bound gains sum_d |q_d| tau_e[d] with
              sum_d |q_d e_d| taken as sum_d |q_d| (|w a_d| + |(1 - w) b_d|)
            d_q: the terms are g w a and g (1 - w) b, each on its own in A; eps_mix = eps + 3 u (the mix's roundings)
            d_TA / d_TB: terms w g q resp. (1 - w) g q: the rounding of g q, of 1 - w and of the fused add: eps_mix again
            d_w[p] = sum_k g_k sum_d q_d (a - b)_d: A_w = sum_k a_g[k] sum_d |q_d| (|a_d| + |b_d|); per term one subtraction, one
              product, three adds inside a float4, the product with g, then at most C / 4 + 2 adds per thread and the 8 levels of
              the block sum: eps_w = eps + 8 u covers them with room (C / 4 + 16 <= C + L + 18 + 8 - the g error's C + 8)
Node and model bars are those of tests/all_entity_cases.check_node (loss 2e-5 relative, gradients 1e-4 |want| + 1e-5 max |want|: at
D = 8 a score carries at most 8 roundings and a gradient entry at most C + 8 terms) and of the window models' fused-against-literal
checks (tests/test_transe_cpu.py::test_window_model_nodes_equal_tensor_path: loss 1e-5, gradients (1e-4, 1e-5 max |want|))."""
import numpy as np
import torch

from temp_amd import functional as TF
from temp_amd import scores as SC
from tests import transe_cases as TC
from tests.golden_util import load

U = TC.U
CANDIDATE_CASES = TC.CANDIDATE_CASES          # (d, C, P, table rows per window, windows), as they are
CEILING = 40704                               # temp_gather_ce_bwd's LDS ceiling (include/temp_amd.h), restated by _lib.GATHER_CE_BWD_MAX_N


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def within(got, want, tol, what):
    """|got - want| <= tol element by element (tol a tensor or a number); a shape mismatch or a non-finite element fails."""
    g, w = got.detach().cpu().double(), want.double()
    assert g.shape == w.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(w.shape))
    assert bool(torch.isfinite(g).all()), "%s: non-finite output" % what
    err = (g - w).abs()
    bad = err > tol
    if bool(bad.any()):
        i = int(torch.argmax((err - tol).reshape(-1)))
        t = tol.reshape(-1)[i] if torch.is_tensor(tol) else tol
        raise AssertionError("%s: %d of %d outside the bound; worst |err| %.3e against %.3e (want %.6e)"
                             % (what, int(bad.sum()), bad.numel(), float(err.reshape(-1)[i]), float(t), float(w.reshape(-1)[i])))
    print("%s: max |err| / bound = %.3f" % (what, float((err / (tol + 1e-300)).max())))


def dot_case(d, C, P, rows, windows, seed=0):
    """transe_cases.candidate_case adapted to a dot product: its table, candidates (a duplicate within a row, one entity in every
    row's list), base and row weights (the last row's is 0); a query of its own scaled so that the scores are of order 1 (a softmax
    that is not one-hot), and query row 0 all zeros -- every score of that row is exactly 0, its softmax uniform."""
    case = dict(TC.candidate_case(d, C, P, rows, windows, seed))
    g = torch.Generator().manual_seed(31 + 1000 * d + 10 * C + P + seed)
    q = (torch.randn(P, d, generator=g) * 0.75).float()
    q[0] = 0.0
    case["q"] = q
    return case


def dot_mix_case(d, C, P, rows, windows, seed=0):
    """dot_case (its table is table_a) plus table_b of the same scale and w uniform in (0, 1); row 0 has w = 1, row 1 w = 0."""
    case = dot_case(d, C, P, rows, windows, seed)
    g = torch.Generator().manual_seed(77 + 1000 * d + 10 * C + P + seed)
    table_b = (torch.randn(case["n_rows"], d, generator=g) * (2.0 / np.sqrt(d))).float()
    w = torch.rand(P, generator=g).float().clamp(2.0 ** -20, 1 - 2.0 ** -20)
    w[0] = 1.0
    if P > 1:
        w[1] = 0.0
    case.update(table_a=case.pop("table"), table_b=table_b, w=w)
    return case


_REF = {}


def _softmax_parts(case, s, tol_s, use_row_scale):
    P, C = case["P"], case["C"]
    lse = torch.logsumexp(s, dim=1)
    rw = case["row_scale"].double() if use_row_scale else torch.full((P,), case["inv_rows"], dtype=torch.float64)
    rw = rw * float(case["scale"][0])
    soft = torch.exp(s - lse.view(-1, 1))
    onehot = torch.zeros(P, C, dtype=torch.float64)
    onehot[:, 0] = 1.0
    rows = TC.table_rows(case)
    L = int(torch.bincount(rows.reshape(-1), minlength=case["n_rows"]).max())
    return dict(s=s, tol_s=tol_s, lse=lse, loss=lse - s[:, 0], tol_loss=2.0 * tol_s.max(dim=1).values + (C + 8) * U,
                g=rw.view(-1, 1) * (soft - onehot), a_g=rw.abs().view(-1, 1) * (soft + onehot), L=L,
                eps=2.0 * float(tol_s.max()) + (C + L + 18) * U)


def dot_reference(case, use_row_scale):
    """fp64 reference of temp_dot_ce_fwd / _bwd_q / _bwd_table on `case` (CPU) with its bounds; computed once per (case, weights)."""
    key = ("plain", case["d"], case["C"], case["P"], case["n_rows"], use_row_scale)
    if key in _REF:
        return _REF[key]
    q, table = case["q"].double(), case["table"].double()
    P, C, d, n_rows = case["P"], case["C"], case["d"], case["n_rows"]
    rows = TC.table_rows(case)
    s, sa = torch.empty(P, C, dtype=torch.float64), torch.empty(P, C, dtype=torch.float64)
    for p in range(P):                                       # row by row: (C, d) at a time
        t = q[p].view(1, d) * table[rows[p]]
        s[p], sa[p] = t.sum(dim=1), t.abs().sum(dim=1)
    ref = _softmax_parts(case, s, (d + 2) * U * sa, use_row_scale)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    d_q, a_q, d_t, a_t = z(P, d), z(P, d), z(n_rows, d), z(n_rows, d)
    for p in range(P):
        e = table[rows[p]]
        d_q[p] = (ref["g"][p].view(-1, 1) * e).sum(dim=0)
        a_q[p] = (ref["a_g"][p].view(-1, 1) * e.abs()).sum(dim=0)
        d_t.index_add_(0, rows[p], ref["g"][p].view(-1, 1) * q[p].view(1, d))
        a_t.index_add_(0, rows[p], ref["a_g"][p].view(-1, 1) * q[p].abs().view(1, d))
    ref.update(d_q=d_q, a_q=a_q, d_table=d_t, a_table=a_t)
    _REF[key] = ref
    return ref


def dot_mix_reference(case, use_row_scale):
    """fp64 reference of temp_dot_mix_ce_fwd / _bwd_q / _bwd_table on `case` (CPU) with its bounds (module docstring: mix)."""
    key = ("mix", case["d"], case["C"], case["P"], case["n_rows"], use_row_scale)
    if key in _REF:
        return _REF[key]
    q, ta, tb, wc = case["q"].double(), case["table_a"].double(), case["table_b"].double(), case["w"].double()
    P, C, d, n_rows = case["P"], case["C"], case["d"], case["n_rows"]
    rows = TC.table_rows(case)
    s, tol = torch.empty(P, C, dtype=torch.float64), torch.empty(P, C, dtype=torch.float64)
    for p in range(P):
        wa, wb = wc[p] * ta[rows[p]], (1 - wc[p]) * tb[rows[p]]
        mag = wa.abs() + wb.abs()
        qa = q[p].abs().view(1, d)
        s[p] = (q[p].view(1, d) * (wa + wb)).sum(dim=1)
        tol[p] = (d + 2) * U * (qa * mag).sum(dim=1) + (qa * 3 * U * mag).sum(dim=1)
    ref = _softmax_parts(case, s, tol, use_row_scale)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    d_q, a_q, d_w, a_w = z(P, d), z(P, d), z(P), z(P)
    d_ta, a_ta, d_tb, a_tb = z(n_rows, d), z(n_rows, d), z(n_rows, d), z(n_rows, d)
    for p in range(P):
        a, b, w = ta[rows[p]], tb[rows[p]], wc[p]
        g, ag = ref["g"][p].view(-1, 1), ref["a_g"][p].view(-1, 1)
        d_q[p] = (g * (w * a + (1 - w) * b)).sum(dim=0)
        a_q[p] = (ag * ((w * a).abs() + ((1 - w) * b).abs())).sum(dim=0)
        d_w[p] = (g * (q[p].view(1, d) * (a - b)).sum(dim=1, keepdim=True)).sum()
        a_w[p] = (ag * (q[p].abs().view(1, d) * (a.abs() + b.abs())).sum(dim=1, keepdim=True)).sum()
        gq, agq = g * q[p].view(1, d), ag * q[p].abs().view(1, d)
        for out, acc, f in ((d_ta, a_ta, w), (d_tb, a_tb, 1 - w)):
            out.index_add_(0, rows[p], f * gq)
            acc.index_add_(0, rows[p], f * agq)
    eps_mix = ref["eps"] + 3 * U
    ref.update(d_q=d_q, tol_q=eps_mix * a_q, d_w=d_w, tol_w=(ref["eps"] + 8 * U) * a_w, d_table_a=d_ta, tol_ta=eps_mix * a_ta,
               d_table_b=d_tb, tol_tb=eps_mix * a_tb)
    _REF[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the three batched nodes on a hand-built plan against the literal fp64 expression
# ---------------------------------------------------------------------------------------------------------------------
NODE_D, NODE_REL, NODE_ROWS, NODE_ENT = 8, 6, 8, 70
NODE_KINDS = ("distmult", "complex", "simple")
NODES = ("plain", "ensemble", "gated")
_SCORE = {"distmult": SC.distmult, "complex": SC.complex, "simple": SC.simple_pair}


def node_plan(device, N=64, C=6, both_live=False):
    """What TKG_Module.loss_inputs hands a node, built by hand: two windows over N entities each, 8 query rows.  both_live False: the
    first window has 5 rows (3 tail, 2 head) and 3 weight-0 pad rows, the second is EMPTY; True: 4 rows each, the last a weight-0 pad.
    Candidates (rows, C): column 0 the truth, a duplicate within rows 1 and 4, entity N - 1 in every row's list."""
    rng = np.random.default_rng(23 + N + C)
    known = np.array([3, 17, 40, 9, 63, 0, 0, 0])
    rel = np.array([0, 5, 2, 5, 1, 0, 0, 0])
    is_tail = np.array([1, 1, 1, 0, 0, 1, 1, 1])
    cand = rng.integers(0, N, (NODE_ROWS, C))
    cand[:, C - 1] = N - 1
    cand[1, 2] = cand[1, 1]
    cand[4, 3] = cand[4, 0]                                  # the truth again among the negatives
    if both_live:
        window = np.array([0, 0, 0, 0, 1, 1, 1, 1])
        weights, splits = [0.25, 0.25, 0.5, 0.0, 0.5, 0.3, 0.2, 0.0], [(0, 4), (4, 8)]
    else:
        window = np.zeros(NODE_ROWS, dtype=np.int64)
        weights, splits = [1 / 3.0] * 3 + [0.5] * 2 + [0.0] * 3, [(0, 8), (8, 8)]
    i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(device)
    return dict(known=i32(known), rel=i32(rel), is_tail=i32(is_tail), cand=i32(cand), window=i32(window), splits=splits,
                weights=torch.tensor(weights, dtype=torch.float32, device=device),
                known_inv=TF.gather_inverse(known.astype(np.int64), NODE_ENT, device),
                rel_inv=TF.gather_inverse(rel.astype(np.int64), NODE_REL, device))


def node_leaves(node, device, N, dtype=torch.float32):
    """Seeded leaves of `node`: plain (ent, rel, big); ensemble (loc, rec, rel, big_loc, big_rec, w); gated (loc, rec, rel, big_loc,
    big_rec, w_known, w_cand).  The weights lie in (0, 1)."""
    g = torch.Generator().manual_seed(41)
    leaf = lambda *shape: (torch.randn(*shape, generator=g) * 0.5).to(device=device, dtype=dtype).requires_grad_(True)
    gate = lambda: torch.sigmoid(torch.randn(NODE_ROWS, 1, generator=g)).to(device=device, dtype=dtype).requires_grad_(True)
    if node == "plain":
        return [leaf(NODE_ENT, NODE_D), leaf(NODE_REL, NODE_D), leaf(2 * N, NODE_D)]
    out = [leaf(NODE_ENT, NODE_D), leaf(NODE_ENT, NODE_D), leaf(NODE_REL, NODE_D), leaf(2 * N, NODE_D), leaf(2 * N, NODE_D), gate()]
    return out + ([gate()] if node == "gated" else [])


def _row_scores(score, k, r, tab, tail):
    k, r, tab = k.unsqueeze(0), r.unsqueeze(0), tab.unsqueeze(0)
    return (score(k, r, tab, mode="tail") if tail else score(tab, r, k, mode="head")).view(-1)


def node_literal(node, kind, plan, N):
    """The node's loss as the literal expression in fp64 with autograd: the reference's scorer on the gathered rows against the
    gathered candidate rows, logsumexp minus the truth's score, the weighted sum -> [loss, gradients of node_leaves in order]."""
    leaves = node_leaves(node, torch.device("cpu"), N, torch.float64)
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in plan.items()}
    score = _SCORE[kind]
    loss = 0
    for p in range(NODE_ROWS):
        rows = int(cpu["window"][p]) * N + cpu["cand"][p].long()
        kn, tail = int(cpu["known"][p]), bool(int(cpu["is_tail"][p]))
        if node == "plain":
            ent, rel, big = leaves
            s = _row_scores(score, ent[kn], rel[int(cpu["rel"][p])], big[rows], tail)
        elif node == "ensemble":
            loc, rec, rel, big_loc, big_rec, w = leaves
            r = rel[int(cpu["rel"][p])]
            s = w[p, 0] * _row_scores(score, loc[kn], r, big_loc[rows], tail) + (1 - w[p, 0]) * _row_scores(score, rec[kn], r, big_rec[rows], tail)
        else:
            loc, rec, rel, big_loc, big_rec, wk, wc = leaves
            k = wk[p, 0] * loc[kn] + (1 - wk[p, 0]) * rec[kn] if tail else rec[kn]       # head rows: the temporal row alone
            s = _row_scores(score, k, rel[int(cpu["rel"][p])], wc[p, 0] * big_loc[rows] + (1 - wc[p, 0]) * big_rec[rows], tail)
        loss = loss + cpu["weights"][p].double() * (torch.logsumexp(s, 0) - s[0])
    loss.backward()
    return [loss.detach()] + [torch.zeros_like(x) if x.grad is None else x.grad for x in leaves]


def run_node(node, kind, device, route, N=64, C=6, both_live=False):
    """-> ([loss, gradients of node_leaves in order] on the CPU, the plan)."""
    plan = node_plan(device, N, C, both_live)
    leaves = node_leaves(node, device, N)
    if node == "plain":
        loss = TF.batched_link_prediction(*leaves, kind, plan, route=route)
    elif node == "ensemble":
        loss = TF.batched_ensemble_link_prediction(*leaves, kind, plan, route=route)
    else:
        loss = TF.batched_gated_link_prediction(*leaves, kind, TF.gated_loss_inputs(plan, NODE_ENT, device), route=route)
    loss.backward()
    return [loss.detach().cpu()] + [x.grad.cpu() for x in leaves], plan


def _big_slots(node):
    return {"plain": (3,), "ensemble": (4, 5), "gated": (4, 5)}[node]


def compare(got, want, what):
    """check_node's bars: loss 2e-5 relative, every gradient 1e-4 |want| + 1e-5 max |want|; everything finite."""
    assert bool(torch.isfinite(got[0])) and abs(float(got[0]) - float(want[0])) <= 2e-5 * abs(float(want[0])), (what, float(got[0]), float(want[0]))
    for i, (g, w) in enumerate(zip(got[1:], want[1:])):
        assert g.shape == w.shape and bool(torch.isfinite(g).all()), (what, i)
        err = (g.double() - w.double()).abs()
        bar = 1e-4 * w.double().abs() + 1e-5 * float(w.abs().max())
        print("%s gradient %d: max err / bar %.3g" % (what, i, float((err / (bar + 1e-300)).max())))
        assert bool((err <= bar).all()), (what, i, float(err.max()))


def check_node(node, kind, device, route="gather", N=64, C=6, both_live=False, against_gemm=True):
    """Loss and every gradient of `node` on `route` against the literal fp64 expression and (against_gemm) against route "gemm" on
    the same inputs; two runs bit-equal; d_big exactly 0 off the candidate rows (the empty window's block with it)."""
    got, plan = run_node(node, kind, device, route, N, C, both_live)
    what = "%s node %s N=%d route=%s" % (node, kind, N, route)
    compare(got, node_literal(node, kind, plan, N), what + " vs literal")
    if against_gemm:
        compare(got, run_node(node, kind, device, "gemm", N, C, both_live)[0], what + " vs gemm")
    again, _ = run_node(node, kind, device, route, N, C, both_live)
    for a, b in zip(got, again):
        assert torch.equal(a, b), what + ": two runs of the node differ"
    off = torch.ones(2 * N, dtype=torch.bool)
    off[(plan["window"].cpu().long().view(-1, 1) * N + plan["cand"].cpu().long()).reshape(-1)] = False
    for i in _big_slots(node):
        assert bool((got[i][off] == 0).all()), what + ": d_big off the candidate rows"
    if not both_live:
        for i in _big_slots(node):
            assert bool((got[i][N:] == 0).all()), what + ": the empty window's block of d_big"
    return got


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def grads(m):
    return {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None}


def close(got, want, rtol, atol, what):
    err = (got.double().cpu() - want.double().cpu()).abs()
    bar = atol + rtol * want.double().cpu().abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= bar).all()), "%s: max |err| %.3e, max err / bar %.3g" % (what, float(err.max()), float((err / bar).max()))


def fused_against_literal(m, step, what):
    """step() -> loss of one training step on fixed samples.  The fused step (m.fused_loss as it stands, m.candidate_route as set)
    against fused_loss = False on the same samples: loss at 1e-5, gradients at (1e-4, 1e-5 max |want|)."""
    m.zero_grad(set_to_none=True)
    fused = step()
    fused.backward()
    gf = grads(m)
    m.zero_grad(set_to_none=True)
    m.fused_loss = False
    try:
        ref = step()
        ref.backward()
    finally:
        m.fused_loss = True
    gr = grads(m)
    assert abs(fused.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (what, fused.item(), ref.item())
    assert sorted(gf) == sorted(gr)
    for k in gr:
        close(gf[k], gr[k], 1e-4, 1e-5 * float(gr[k].abs().max()), what + " " + k)


def check_window_model(device, route="gather"):
    """DynamicRGCN (golden G10_uni_grrgcn_rol, complex) with candidate_route = `route` on the golden's injected samples."""
    from tests.window_cases import build_window_model, window_inputs
    z = load("G10_uni_grrgcn_rol")
    m = build_window_model(z, device)
    m.candidate_route = route
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    fused_against_literal(m, lambda: m(t_list, target_edge_ids=edge_ids, samples=samples), "DynamicRGCN route=%s" % route)
    return m


BIG_N = CEILING + 4                            # 40 708: the first entity count (a multiple of 4) that temp_gather_ce_bwd refuses


def big_static_model(device, num_ents=BIG_N):
    """A StaticRGCN over `num_ents` entities and three tiny hand-built snapshots (40 train facts each over 25 entities spread up to
    the last id; embed_size = hidden_size = 8, negative_rate = 20, num_pos_facts = 30) -> (model, timestamps, target edge ids)."""
    from temp_amd.dataset import build_interpolation_snapshots
    from temp_amd.static_rgcn import StaticRGCN
    from tests.window_cases import make_args
    rng = np.random.default_rng(5)
    ents = np.unique(np.concatenate([rng.integers(0, num_ents, 23), [0, num_ents - 1]]))
    quads = []
    for t in range(3):
        for n in (40, 4, 4):                                  # train, valid, test
            quads.append(np.stack([rng.choice(ents, n), rng.integers(0, 5, n), rng.choice(ents, n), np.full(n, t)], axis=1))
    tr, va, te = build_interpolation_snapshots(np.concatenate(quads[0::3]), np.concatenate(quads[1::3]), np.concatenate(quads[2::3]))
    args = make_args(module="SRGCN", embed_size=8, hidden_size=8, n_bases=4, negative_rate=20, num_pos_facts=30, score_function="distmult")
    torch.manual_seed(2)
    m = StaticRGCN(args, num_ents, 5, tr, va, te).to(device)
    tl = [0, 1, 2]
    rng = np.random.default_rng(1)
    edge_ids = [rng.choice(tr[t].number_of_edges(), size=tr[t].number_of_edges() // 2, replace=False) for t in tl]
    return m, tl, edge_ids


def check_big_static_model(device, route=None):
    """One training step of big_static_model with candidate_route = `route`: the batched node's loss.backward() succeeds, and the
    step matches fused_loss = False on the same samples (the fused step's own plan and draw, re-injected into the per-graph route)."""
    m, tl, edge_ids = big_static_model(device)
    m.candidate_route = route
    fused = m(torch.tensor(tl), target_edge_ids=edge_ids)
    plan, cand = m._last_plan
    fused.backward()
    gf = grads(m)
    samples = []
    for trip, (a0, _) in zip(plan["triples"], plan["splits"]):
        P = trip.shape[0]
        samples.append((torch.from_numpy(trip), cand[a0:a0 + P].long(), cand[a0 + P:a0 + 2 * P].long()))
    m.zero_grad(set_to_none=True)
    m.fused_loss = False
    ref = m(torch.tensor(tl), target_edge_ids=edge_ids, samples=samples)
    ref.backward()
    gr = grads(m)
    m.fused_loss = True
    assert abs(fused.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (fused.item(), ref.item())
    assert sorted(gf) == sorted(gr)
    for k in gr:
        close(gf[k], gr[k], 1e-4, 1e-5 * float(gr[k].abs().max()), "StaticRGCN N=%d route=%s %s" % (m.num_ents, route, k))
    # the per-graph fused node (candidate_cross_entropy) on the same samples
    fused_against_literal(m, lambda: m(torch.tensor(tl), target_edge_ids=edge_ids, samples=samples), "StaticRGCN per graph N=%d route=%s" % (m.num_ents, route))
    return m
