"""Shared fp64 references, bounds and seeded inputs of the gated TransE kernels: temp_l1_mix_ce_fwd / _bwd_q / _bwd_table,
temp_l1_mix_scores, the filtered rank over them and temp_gated_query_fwd / _bwd of kind transE (include/temp_amd.h).

The candidate of row p is e[p,k] = mix(w[p], table_a[row], table_b[row]), mix(w, a, b) = fmaf(w, a, (1 - w) * b) in the kernels.
The references take q, both tables and w as GIVEN fp32 data and form e64 = w a + (1 - w) b in fp64.

Bounds (u = 2^-24), derived, not measured:
  mix       per component tau_e = 3 u (|w a| + |(1 - w) b|): the three roundings of mix;  T[p,k] = sum_d tau_e
  sign      a component is DETERMINED when |q - e64| > tau_e, or when w is 0 or 1 (then e is exact and q - e has the exact fp32
            sign); otherwise the fp32 sign may be any of -1, 0, +1
  score     |s - s64| <= (d + 2) u |s64| + 2 T
  lse/loss  2 max_k tol_s + (C + 8) u
  gradient  |err| <= eps A + the allowance of the undetermined terms; A = the fp64 sum of the absolute values of the element's
            additive terms (softmax part and one-hot part each on their own), eps = 2 max tol_s + (C + L + 16) u, L = the longest
            slot list; an undetermined term widens the bound by 2 a_g (d_q), 2 w a_g (d_TA), 2 (1 - w) a_g (d_TB),
            2 a_g |a - b| (d_w)
  condition at most 0.1 % of the elements of each gradient output carry a widened bound (asserted on the CPU)
  rank      transe_cases.rank_band with tau = tol_s[j] + tol_s[t] + 2^-22; at most 25 % of the rows wider than one rank."""
import numpy as np
import torch

from tests import transe_cases as TC

U = TC.U
CANDIDATE_CASES = TC.CANDIDATE_CASES          # (d, C, P, table rows per window, windows); (260, 1025, 67, 515, 2) among them
SCORE_CASES = TC.SCORE_CASES                  # (P, N, d, ld); the first two carry the rank tests
WIDENED_SHARE = 1e-3


def fma32(a, b, c):
    """Elementwise fp32 fmaf(a, b, c) of fp32 tensors, exactly: the product of two fp32 values is exact in fp64; the fp64 sum is
    rounded to odd (the error of the sum from TwoSum), after which the rounding to fp32 is the correctly rounded one."""
    p = a.double().numpy() * b.double().numpy()
    c = np.broadcast_to(c.double().numpy(), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                           # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where((err > 0) == (s > 0), 1, -1)            # the odd neighbour lies on the side of the error
    toward = np.where(s == 0, 0, toward)
    s = np.where(fix, (bits + toward).view(np.float64), s)
    return torch.from_numpy(s.astype(np.float32))


def mix32(w, a, b):
    """The kernels' mix1 in fp32, bit for bit: fmaf(w, a, (1 - w) * b); w broadcasts over the rows of a and b."""
    w = w.float().reshape(-1, *([1] * (a.dim() - 1))).expand_as(a).contiguous()
    return fma32(w, a, (1.0 - w) * b)


def gated_case(d, C, P, rows, windows, seed=0):
    """transe_cases.candidate_case (its table is table_a) plus table_b of the same scale and w uniform in (0, 1).  Planted: row 0
    has w = 1 and q[0] equal to its true candidate's table_a row (a whole row of sgn(0)); row 1 has w = 0 and half its components
    equal to its true candidate's table_b row; the duplicate candidate, the entity in every row's list and the weight-0 last row
    are candidate_case's."""
    case = dict(TC.candidate_case(d, C, P, rows, windows, seed))
    g = torch.Generator().manual_seed(77 + 1000 * d + 10 * C + P + seed)
    sc = 2.0 / np.sqrt(d)
    table_b = (torch.randn(windows * rows, d, generator=g) * sc).float()
    w = torch.rand(P, generator=g).float().clamp(2.0 ** -20, 1 - 2.0 ** -20)
    w[0] = 1.0
    q = case["q"].clone()
    if P > 1:
        w[1] = 0.0
        t = int(case["cand"][1, 0]) + (int(case["base"][1]) if case["base"] is not None else 0)
        q[1] = (torch.randn(d, generator=g) * sc).float()
        half = torch.arange(d) % 2 == 0
        q[1, half] = table_b[t][half]
    case.update(q=q, table_a=case.pop("table"), table_b=table_b, w=w)
    return case


_REF = {}


def gated_reference(case, use_row_scale):
    """fp64 reference of the three gated candidate kernels on `case` (CPU), with bounds; computed once per (case, weights)."""
    key = (case["d"], case["C"], case["P"], case["n_rows"], use_row_scale)
    if key in _REF:
        return _REF[key]
    q, ta, tb, wc = case["q"].double(), case["table_a"].double(), case["table_b"].double(), case["w"].double()
    P, C, d, n_rows = case["P"], case["C"], case["d"], case["n_rows"]
    rows = TC.table_rows(case)
    s = torch.empty(P, C, dtype=torch.float64)
    T = torch.empty(P, C, dtype=torch.float64)
    diffs, undet = [], []
    for p in range(P):                                       # row by row: (C, d) at a time
        a, b, w = ta[rows[p]], tb[rows[p]], wc[p]
        e = w * a + (1 - w) * b
        tau = 3 * U * ((w * a).abs() + ((1 - w) * b).abs())
        diff = q[p].view(1, d) - e
        s[p] = -diff.abs().sum(dim=1)
        T[p] = tau.sum(dim=1)
        und = diff.abs() <= tau
        if float(w) in (0.0, 1.0):
            und = torch.zeros_like(und)
        diffs.append(torch.sign(diff).to(torch.int8))
        undet.append(und)
    tol_s = (d + 2) * U * s.abs() + 2 * T
    lse = torch.logsumexp(s, dim=1)
    loss = lse - s[:, 0]
    rw = case["row_scale"].double() if use_row_scale else torch.full((P,), case["inv_rows"], dtype=torch.float64)
    rw = rw * float(case["scale"][0])
    soft = torch.exp(s - lse.view(-1, 1))
    onehot = torch.zeros(P, C, dtype=torch.float64)
    onehot[:, 0] = 1.0
    g = rw.view(-1, 1) * (soft - onehot)
    a_g = rw.abs().view(-1, 1) * (soft + onehot)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    d_q, a_q, x_q = z(P, d), z(P, d), z(P, d)                 # value, sum of |terms|, allowance of the undetermined terms
    d_w, a_w, x_w = z(P), z(P), z(P)
    d_ta, a_ta, x_ta = z(n_rows, d), z(n_rows, d), z(n_rows, d)
    d_tb, a_tb, x_tb = z(n_rows, d), z(n_rows, d), z(n_rows, d)
    n_undet = 0
    for p in range(P):
        sg, und, w = diffs[p].double(), undet[p].double(), wc[p]
        n_undet += int(und.sum())
        amb = ta[rows[p]] - tb[rows[p]]
        gs = g[p].view(-1, 1) * sg
        ab = a_g[p].view(-1, 1) * sg.abs()
        wide = 2 * a_g[p].view(-1, 1) * und
        d_q[p], a_q[p], x_q[p] = -gs.sum(dim=0), ab.sum(dim=0), wide.sum(dim=0)
        d_w[p], a_w[p], x_w[p] = (gs * amb).sum(), (ab * amb.abs()).sum(), (wide * amb.abs()).sum()
        for out, acc, wid, f in ((d_ta, a_ta, x_ta, w), (d_tb, a_tb, x_tb, 1 - w)):
            out.index_add_(0, rows[p], f * gs)
            acc.index_add_(0, rows[p], f * ab)
            wid.index_add_(0, rows[p], f * wide)
    L = int(torch.bincount(rows.reshape(-1), minlength=n_rows).max())
    eps = 2.0 * float(tol_s.max()) + (C + L + 16) * U
    ref = dict(s=s, tol_s=tol_s, lse=lse, loss=loss, tol_loss=2.0 * tol_s.max(dim=1).values + (C + 8) * U, g=g, a_g=a_g, eps=eps, L=L,
               d_q=d_q, tol_q=eps * a_q + x_q, wide_q=x_q > 0, d_w=d_w, tol_w=eps * a_w + x_w, wide_w=x_w > 0,
               d_table_a=d_ta, tol_ta=eps * a_ta + x_ta, wide_ta=x_ta > 0, d_table_b=d_tb, tol_tb=eps * a_tb + x_tb, wide_tb=x_tb > 0,
               n_undetermined=n_undet)
    _REF[key] = ref
    return ref


def widened_shares(ref):
    """Share of the elements of each gradient output whose bound carries an undetermined term's allowance."""
    return {k: float(ref["wide_" + k].double().mean()) for k in ("q", "w", "ta", "tb")}


_SCORE = {}


def gated_score_case(P, N, d, seed=0):
    """transe_cases.score_case (its table is table_a) with a second table and uniform gates, and the fp64 reference of the dense
    gated scores with tol = (d + 2) u |s64| + 2 T (computed once, shared, never modified)."""
    key = (P, N, d, seed)
    if key not in _SCORE:
        c = TC.score_case(P, N, d, seed)
        g = torch.Generator().manual_seed(13 * P + 5 * N + d + seed)
        sc = 2.0 / np.sqrt(d)
        table_b = (torch.randn(N, d, generator=g) * sc).float()
        w = torch.rand(P, generator=g).float().clamp(2.0 ** -20, 1 - 2.0 ** -20)
        a64, b64 = c["table"].double(), table_b.double()
        s64 = torch.empty(P, N, dtype=torch.float64)
        T = torch.empty(P, N, dtype=torch.float64)
        for p in range(P):
            wp = w[p].double()
            s64[p] = -(c["q"][p].double().view(1, d) - (wp * a64 + (1 - wp) * b64)).abs().sum(dim=1)
            T[p] = (3 * U * ((wp * a64).abs() + ((1 - wp) * b64).abs())).sum(dim=1)
        _SCORE[key] = dict(q=c["q"], table_a=c["table"], table_b=table_b, w=w, s64=s64, tol=(d + 2) * U * s64.abs() + 2 * T)
    return _SCORE[key]


def gated_query_case(d, P=133, seed=0):
    """Seeded operands of temp_gated_query_fwd / _bwd, kind transE: mixed is_tail, mixed temporal-only rows (ia < 0), gates of 0
    and 1 among uniform ones -- and the references: q bit for bit (mix32 followed by one fp32 add / subtract), the backward in
    fp64 with the magnitudes of its terms."""
    g = torch.Generator().manual_seed(31 * d + P + seed)
    na, nb, R2 = 40, 45, 9
    A, B, rel = (torch.randn(n, d, generator=g).float() for n in (na, nb, R2))
    ia = torch.randint(0, na, (P,), generator=g).int()
    ib = torch.randint(0, nb, (P,), generator=g).int()
    ia[torch.arange(P) % 4 == 1] = -1
    ridx = torch.randint(0, R2, (P,), generator=g).int()
    is_tail = (torch.arange(P) % 3 != 0).int()
    w = torch.rand(P, generator=g).float()
    w[::7] = 0.0
    w[3::7] = 1.0
    d_q = torch.randn(P, d, generator=g).float()
    gated = (ia >= 0).view(-1, 1)
    a, b, r = A[ia.long().clamp(min=0)], B[ib.long()], rel[ridx.long()]
    known = torch.where(gated, mix32(w, a, b), b)
    q = torch.where(is_tail.view(-1, 1) != 0, known + r, known - r)
    w64, dk = w.double().view(-1, 1), d_q.double()
    zero = torch.zeros_like(dk)
    terms = dk * (a.double() - b.double())
    return dict(A=A, ia=ia, B=B, ib=ib, w=w, rel=rel, ridx=ridx, is_tail=is_tail, d_q=d_q, gated=gated.view(-1), q=q,
                d_a=torch.where(gated, w64 * dk, zero), d_b=torch.where(gated, (1 - w64) * dk, dk),
                d_rel=torch.where(is_tail.view(-1, 1) != 0, dk, -dk),
                d_w=torch.where(gated.view(-1), terms.sum(dim=1), torch.zeros(P, dtype=torch.float64)),
                a_w=torch.where(gated.view(-1), terms.abs().sum(dim=1), torch.zeros(P, dtype=torch.float64)),
                exact=(~gated.view(-1)) | (w == 0) | (w == 1))


def near_zero_mask(q, wa, a, b):
    """bool (R, C, D): the components of q - e, e = w a + (1 - w) b (fp64 from the fp32 rows; q (R, D), wa (R,), a and b (R, C, D)),
    that lie within 2^-20 (|q| + |w a| + |(1 - w) b|) of zero without being exactly zero: where the tensor path's and the
    kernels' expressions would have to agree on a sign that hinges on a rounding."""
    q, w, a, b = q.double().unsqueeze(1), wa.double().view(-1, 1, 1), a.double(), b.double()
    v = q - (w * a + (1 - w) * b)
    return (v != 0) & (v.abs() < 2.0 ** -20 * (q.abs() + (w * a).abs() + ((1 - w) * b).abs()))


def post_eval_band(ev, samples, g, t, N, ent, ent_r, rel, all_e, all_r, ws, device=None):
    """The fp64 rank band of PostEvaluationFilter's rows (subject-corruption first): the known mix and the query are the filter's
    own fp32 expressions, the candidate mix and the distance fp64, tol = (D + 2) u |s64| + 2 T."""
    D = all_e.shape[1]
    lo, hi = [], []
    w_sqs, w_sqo, w_oqs, w_oqo = ws
    for mode, w_s, w_o in (("head", w_sqs, w_sqo), ("tail", w_oqs, w_oqo)):
        target, ptr, ids = (x.cpu() for x in ev._mode_inputs(mode, samples if device is None else samples.to(device), g, int(t), N,
                                                             all_e.device if device is None else device))
        sel = samples[:, 0] if mode == "tail" else samples[:, 2]
        w_known, w_cand = (w_s, w_o) if mode == "tail" else (w_o, w_s)
        on = (lambda x: x) if device is None else (lambda x: x.to(device))       # the filter's fp32 query, formed where it forms it
        known = on(w_known) * on(ent[sel]) + (1 - on(w_known)) * on(ent_r[sel])
        r = on(rel[samples[:, 1]])
        q = (known + r if mode == "tail" else known - r).cpu().double()
        s64 = torch.empty(q.shape[0], N, dtype=torch.float64)
        T = torch.empty_like(s64)
        a64, b64 = all_e.double(), all_r.double()
        for p in range(q.shape[0]):
            wp = w_cand[p].double()
            s64[p] = -(q[p].view(1, D) - (wp * a64 + (1 - wp) * b64)).abs().sum(dim=1)
            T[p] = (3 * U * ((wp * a64).abs() + ((1 - wp) * b64).abs())).sum(dim=1)
        a, b = TC.rank_band(s64, (D + 2) * U * s64.abs() + 2 * T, target, ptr, ids)
        lo.append(a); hi.append(b)
    return torch.cat(lo), torch.cat(hi)
