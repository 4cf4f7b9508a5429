"""Shared fp64 references, tolerances and seeded inputs of the TransE (L1) kernels: temp_l1_ce_fwd / _bwd_q / _bwd_table,
temp_l1_scores and the filtered rank over them (include/temp_amd.h).

The references take the query `q` as GIVEN fp32 data -- it is an input of the kernels -- so q - e has the exact sign in fp32 and
no sign can disagree with fp64; everything after that is fp64.

Tolerances (u = 2^-24), derived, not measured:
  score     d subtractions and a d-term sum of non-negative terms in any order:    |s - s64| <= (d + 2) u |s64|
  loss      |loss - loss64| <= 2 max_k tol_s[p, k] + (C + 8) u
  gradient  per output element, A = the fp64 sum of the absolute values of its additive terms (scale w softmax_k sgn and
            scale w [k == 0] sgn, each counted on its own):
            |err| <= eps A,  eps = 2 max tol_s + (C + L + 16) u,  L = the longest slot list
  rank      the fp64 band lo <= rank <= hi: lo counts s_j > s_t + tau, hi counts s_j >= s_t - tau,
            tau = tol_s[j] + tol_s[t] + 2^-22 (the fp32 sigmoid)."""
import numpy as np
import torch

U = 2.0 ** -24

# (d, C, P, table rows per window, windows): windows == 1 runs with base = NULL, 2 with two stacked windows.  Every value of each
# axis appears (d: below one lane group / the workload's 200 / the 256 line / past it; C: 1, 2, 101, 1025; P: 1, 5, 67; rows 7, 515)
# and (d = 260, C = 1025) together.  The forward keeps the query in 1 to 4 float4 per lane for d <= 64, 128, 192, 256 and re-reads it
# beyond: d = 8, 100, 132, 200 / 256 and 260 take the five routes in that order.  The two cases at d = 100 and d = 132 also end in
# a partial float4 pass (d mod 64 != 0), and their C = 33 and C = 17 leave a 16-lane group with a paired second candidate
# (k0 + 16 < C) and with a dangling one.
CANDIDATE_CASES = [
    (8, 1, 1, 7, 1),
    (8, 2, 5, 7, 2),
    (8, 101, 67, 515, 1),
    (200, 101, 67, 515, 2),
    (200, 1025, 5, 7, 1),
    (200, 1, 5, 515, 2),
    (256, 101, 5, 7, 2),
    (256, 2, 67, 515, 1),
    (260, 1025, 67, 515, 2),
    (260, 101, 1, 7, 1),
    (100, 33, 5, 7, 2),
    (132, 17, 5, 7, 1),
]

# (P, N, d, ld) of the dense scores; the first two also carry the rank tests (a larger N at d = 200 makes the band uninformative)
SCORE_CASES = [(37, 203, 8, 204), (64, 400, 200, 400), (5, 4100, 260, 4100)]


def candidate_case(d, C, P, rows, windows, seed=0):
    """Seeded inputs of one candidate-kernel case.  Row 0's true candidate equals q[0] exactly (sgn(0) on a whole row); the row
    after it (or, with one row, its second candidate) equals q in half the components; a duplicate candidate within a row; one
    entity that is a candidate of every row (a long slot list); the last row has row_scale = 0."""
    g = torch.Generator().manual_seed(1000 * d + 10 * C + P + seed)
    sc = 2.0 / np.sqrt(d)                                    # score differences of order 1: a softmax that is not one-hot
    table = (torch.randn(windows * rows, d, generator=g) * sc).float()
    q = (torch.randn(P, d, generator=g) * sc).float()
    cand = torch.randint(0, rows, (P, C), generator=g).int()
    base = None
    if windows > 1:
        base = (torch.arange(P) % windows * rows).int()     # rows alternate between the stacked windows
    if C >= 2:
        cand[:, C - 1] = 3                                   # in every row's list
    if C >= 3:
        cand[P // 2, 2] = cand[P // 2, 1]                    # a duplicate
    elif C == 2:
        cand[P - 1, 1] = cand[P - 1, 0]
    row_of = lambda p, k: int(cand[p, k]) + (int(base[p]) if base is not None else 0)
    q[0] = table[row_of(0, 0)]
    half = torch.arange(d) % 2 == 0
    if P > 1:
        q[1, half] = table[row_of(1, 0)][half]
    elif C >= 3:
        t = row_of(0, 1)
        if t != row_of(0, 0):
            table[t, half] = q[0, half]
    row_scale = (torch.rand(P, generator=g) + 0.5).float() / P
    row_scale[P - 1] = 0.0
    return dict(q=q, table=table, base=base, cand=cand, row_scale=row_scale, scale=torch.tensor([0.75]), inv_rows=1.0 / P,
                d=d, C=C, P=P, n_rows=windows * rows)


def table_rows(case):
    c = case["cand"].long()
    return c if case["base"] is None else c + case["base"].long().view(-1, 1)


def candidate_reference(case, use_row_scale):
    """fp64 reference of the three candidate kernels on `case` (CPU): s, lse, loss, g, d_q, d_table with their tolerances."""
    q, table = case["q"].double(), case["table"].double()
    P, C, d = case["P"], case["C"], case["d"]
    rows = table_rows(case)
    s = torch.empty(P, C, dtype=torch.float64)
    for p in range(P):                                       # row by row: (C, d) at a time
        s[p] = -(q[p].view(1, d) - table[rows[p]]).abs().sum(dim=1)
    tol_s = (d + 2) * U * s.abs()
    lse = torch.logsumexp(s, dim=1)
    loss = lse - s[:, 0]
    w = case["row_scale"].double() if use_row_scale else torch.full((P,), case["inv_rows"], dtype=torch.float64)
    w = w * float(case["scale"][0])
    soft = torch.exp(s - lse.view(-1, 1))
    onehot = torch.zeros(P, C, dtype=torch.float64)
    onehot[:, 0] = 1.0
    g = w.view(-1, 1) * (soft - onehot)
    a_g = w.abs().view(-1, 1) * (soft + onehot)
    d_q = torch.zeros(P, d, dtype=torch.float64)
    a_q = torch.zeros(P, d, dtype=torch.float64)
    d_t = torch.zeros(case["n_rows"], d, dtype=torch.float64)
    a_t = torch.zeros(case["n_rows"], d, dtype=torch.float64)
    for p in range(P):
        sg = torch.sign(q[p].view(1, d) - table[rows[p]])   # (C, d); sign(0) = 0
        gs = g[p].view(-1, 1) * sg
        ab = a_g[p].view(-1, 1) * sg.abs()                   # the additive terms: scale w softmax_k sgn and scale w [k == 0] sgn
        d_q[p] = -gs.sum(dim=0)
        a_q[p] = ab.sum(dim=0)
        d_t.index_add_(0, rows[p], gs)
        a_t.index_add_(0, rows[p], ab)
    L = int(torch.bincount(rows.reshape(-1), minlength=case["n_rows"]).max())
    eps = 2.0 * float(tol_s.max()) + (C + L + 16) * U
    return dict(s=s, tol_s=tol_s, lse=lse, loss=loss, tol_loss=2.0 * tol_s.max(dim=1).values + (C + 8) * U, g=g, a_g=a_g, d_q=d_q, a_q=a_q,
                d_table=d_t, a_table=a_t, eps=eps, L=L)


def slot_lists(case):
    """(slot_ptr int32 [n_rows + 1], slot int32 [P C]) on the host: the contract of temp_l1_ce_bwd_table."""
    keys = table_rows(case).reshape(-1).numpy()
    order = np.argsort(keys, kind="stable")
    ptr = np.zeros(case["n_rows"] + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys, minlength=case["n_rows"]), out=ptr[1:])
    return torch.from_numpy(ptr.astype(np.int32)), torch.from_numpy(order.astype(np.int32))


_SCORE = {}


def score_case(P, N, d, seed=0):
    """Seeded (q, table) of a dense-score case and its fp64 reference (computed once, shared, never modified):
    q (P, d), table (N, d), s64 (P, N), tol (P, N).  Scaled so that the scores stay above the fp32 sigmoid's underflow (-104)."""
    key = (P, N, d, seed)
    if key not in _SCORE:
        g = torch.Generator().manual_seed(7 * P + 3 * N + d + seed)
        sc = 2.0 / np.sqrt(d)
        q = (torch.randn(P, d, generator=g) * sc).float()
        table = (torch.randn(N, d, generator=g) * sc).float()
        s64 = torch.empty(P, N, dtype=torch.float64)
        t64 = table.double()
        for p in range(P):
            s64[p] = -(q[p].double().view(1, d) - t64).abs().sum(dim=1)
        _SCORE[key] = dict(q=q, table=table, s64=s64, tol=(d + 2) * U * s64.abs())
    return _SCORE[key]


def rank_inputs(P, N, seed=0):
    """Seeded targets and filter lists (unique ascending ids per row, some rows empty, the target sometimes listed)."""
    g = torch.Generator().manual_seed(11 * P + N + seed)
    target = torch.randint(0, N, (P,), generator=g).int()
    cnt = torch.randint(0, 9, (P,), generator=g)
    lists = []
    for p, c in enumerate(cnt.tolist()):
        ids = torch.randperm(N, generator=g)[:c]
        if p % 3 == 0 and c > 0:
            ids[0] = target[p]
        lists.append(torch.unique(ids))
    ptr = torch.zeros(P + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.tensor([x.numel() for x in lists]), 0).int()
    return target, ptr, torch.cat(lists).int()


def rank_band(s64, tol, target, filt_ptr=None, filt_ids=None):
    """(lo, hi) int64 [P]: the ranks every fp32 evaluation within `tol` of s64 must lie between (see the module docstring).
    Filtered entities other than the target have value sigmoid(-10e6) = 0 and are never ahead of a target with a positive sigmoid."""
    P, N = s64.shape
    tgt = target.long()
    live = torch.ones(P, N, dtype=torch.bool)
    if filt_ptr is not None:
        ptr = filt_ptr.long()
        rows = torch.repeat_interleave(torch.arange(P), ptr[1:] - ptr[:-1])
        live[rows, filt_ids.long()] = False
    live[torch.arange(P), tgt] = False
    st = s64.gather(1, tgt.view(-1, 1))
    tau = tol + tol.gather(1, tgt.view(-1, 1)) + 2.0 ** -22
    lo = 1 + ((s64 > st + tau) & live).sum(dim=1)
    hi = 1 + ((s64 >= st - tau) & live).sum(dim=1)
    return lo, hi


def near_zero_mask(c, r, o):
    """bool (R, C, D): the components of the head-mode difference c + r - o (fp64 from the fp32 rows; c (R, C, D), r and o (R, D))
    that lie within 2^-20 (|c| + |r| + |o|) of zero without being exactly zero: where the tensor path's c + (r - o) and the
    kernels' (o - r) - c would have to agree on a sign that hinges on a rounding."""
    c, r, o = c.double(), r.double().unsqueeze(1), o.double().unsqueeze(1)
    v = c + r - o
    return (v != 0) & (v.abs() < 2.0 ** -20 * (c.abs() + r.abs() + o.abs()))


def near_zero_components(c, r, o):
    return int(near_zero_mask(c, r, o).sum())
