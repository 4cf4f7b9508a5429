"""The link-prediction loss: torch.autograd nodes around the loss kernels (through temp_amd.backend).  temp_amd.functional re-exports
the public functions; the private names (_TALL_SCORES, _L1_METHODS, _L1_MIX_METHODS, _cached_l1_slots, the node classes) live here.

Three batched nodes, each written once over a scorer (_GemmScorer: distmult / complex / simple, scores against ALL entities of a
window; _GatherScorer: the score at the candidates alone, as _L1Scorer -- transE, L1 distances -- and as _DotGatherScorer -- the
bilinear scorers' route "gather", inner products; bilinear_route picks between GEMM and DOT: None = GEMM up to the LDS ceiling of
temp_gather_ce_bwd, DOT above it).  The backend calls of every node x scorer, forward | backward:

  _BatchedLinkPredictionFn            sum over windows of CE_tail + CE_head (models/DynamicRGCN.py:186-193)
    both     bilinear_query_fwd                                  | ... bilinear_query_bwd, segment_sum_rows x 2 (known, rel)
    GEMM     linear_multi, gather_ce_fwd                         | gather_ce_bwd, linear_multi, linear_tn_multi
             (TEMP_LOSS_TALL=1: linear_t per window)             |   (tall: linear_tn + linear per window)
    L1       l1_ce_fwd                                           | l1_ce_bwd_q, l1_ce_bwd_table
    DOT      dot_ce_fwd                                          | dot_ce_bwd_q, dot_ce_bwd_table
  _BatchedAllEntityLinkPredictionFn   the same sum with EVERY entity outside the row's known-true list as a negative ("1-vs-all",
    GEMM     bilinear_query_fwd; per column panel linear_multi,  | per panel (linear_multi again unless the panel is the whole row),
    only     filtered_ce_fwd with the carry                      |   filtered_ce_bwd, linear_multi, linear_tn_multi; bilinear_query_bwd,
             (filtered_ce_rows_torch on a backend without them)  |   segment_sum_rows x 2.  No candidate lists: reads the plan's truth / lo / hi / ids
  _BatchedEnsembleLinkPredictionFn    score-level ensemble of two streams (models/PostDynamicRGCN.py:404-406, 425-428)
    both     per stream: bilinear_query_fwd + its scores         | per stream: ..., bilinear_query_bwd, segment_sum_rows (known);
             (mix = one torch.lerp)                              |   then segment_sum_rows (rel) of the streams' sum
    GEMM     linear_multi per stream, gather_ce_fwd of the mix   | gather_ce_bwd once; per stream linear_multi, linear_tn_multi
    L1       l1_ce_fwd per stream (logsumexp of the mix: torch)  | per stream l1_ce_bwd_q (the MIXED softmax, row_scale = weights * w
                                                                 |   resp. weights * (1 - w)), l1_ce_bwd_table
    DOT      the L1 rows with dot_ce_fwd                         | ... dot_ce_bwd_q, dot_ce_bwd_table
  _BatchedGatedLinkPredictionFn       embedding-level gate of the post-aggregation models (models/PostDynamicRGCN.py:261-282)
    both     gated_query_fwd                                     | ... gated_query_bwd, segment_sum_rows x 3 (known_a, known, rel)
    GEMM     linear_multi x 2 (one q), gather_ce_mix_fwd         | gather_ce_mix_bwd, linear_multi x 2, linear_tn_multi x 2
    L1       l1_mix_ce_fwd                                       | l1_mix_ce_bwd_q, l1_mix_ce_bwd_table
    DOT      dot_mix_ce_fwd                                      | dot_mix_ce_bwd_q, dot_mix_ce_bwd_table
  _FrozenMixCEFn                      score-level ensemble of two FROZEN models (models/aggregator.py:185-208): two relation tables,
    both     bilinear_query_fwd x 2, frozen_mix_ce               | (nothing: d_w came out of the forward launch)
             (no (rows, N) matrix; frozen_mix_ce_rows in torch on a backend without the kernel)

(linear_tn_multi: one linear_tn per live window on a backend without it; gated_query_* / gather_ce_mix_*: through bilinear_query_* /
gather_ce_* and torch on a backend without them; dot_*: dot_ce_rows_torch and its hand-written adjoints -- the CPU test backend.)  `big` is the (B * N, D) stack of the windows' all-entity
matrices, inp = TKG_Module.loss_inputs(...) (gated_loss_inputs for the gated node); every gradient of a gathered operand is a
deterministic segment sum over the static index lists.  The unbatched nodes (one target graph, the query rows given):
  _CandidateCEFn       linear, gather_ce_fwd | gather_ce_bwd, linear, linear_tn
                       (route "gather": dot_ce_fwd | dot_ce_bwd_q, dot_ce_bwd_table, base = None)
  _MixedCandidateCEFn  linear x 2, gather_ce_fwd | gather_ce_bwd, (linear, linear_tn) x 2
                       (route "gather": dot_ce_fwd x 2, the mix and its logsumexp in torch | (dot_ce_bwd_q, dot_ce_bwd_table) x 2)
  _TranslationCEFn     l1_ce_fwd | l1_ce_bwd_q, l1_ce_bwd_table
"""
import os

import torch

from ._lib import GATHER_CE_BWD_MAX_N
from .backend import get_backend

# Entity-major score GEMMs of the plain node (_GemmScorer.ce_fwd): 10 % less device time on ICEWS-shaped steps (3.51 -> 3.18 ms under
# graph replay), but ~30 more launches per step, which makes an eager, host-bound training loop SLOWER (5.7 -> 6.8 ms/step measured).
# Off unless TEMP_LOSS_TALL=1.
_TALL_SCORES = os.environ.get("TEMP_LOSS_TALL", "0") == "1"

_L1_METHODS = ("l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table", "l1_scores")
_L1_MIX_METHODS = ("l1_mix_ce_fwd", "l1_mix_ce_bwd_q", "l1_mix_ce_bwd_table", "l1_mix_scores")
_DOT_METHODS = ("dot_ce_fwd", "dot_ce_bwd_q", "dot_ce_bwd_table")
_DOT_MIX_METHODS = ("dot_mix_ce_fwd", "dot_mix_ce_bwd_q", "dot_mix_ce_bwd_table")


def translation_supported(be=None):
    """True when the installed backend has the L1 (TransE) kernels; a backend without them keeps the tensor path."""
    be = get_backend() if be is None else be
    return all(hasattr(be, m) for m in _L1_METHODS)


def gated_translation_supported(be=None):
    """True when the installed backend has the gated L1 (post-aggregation TransE) kernels; without them the tensor path stays."""
    be = get_backend() if be is None else be
    return all(hasattr(be, m) for m in _L1_MIX_METHODS)


def l1_slots(cand, base, n_rows):
    """The slot lists of temp_l1_ce_bwd_table, built on the device: (slot_ptr int32 [n_rows + 1], slot int32 [P * C]) = the flat
    positions p * C + k of `cand` grouped by their table row base[p] + cand[p, k] (base None = 0), ascending within a row (one
    stable sort of the int32 row keys; the CSR by a binary search of the sorted keys: no host round trip)."""
    keys = (cand if base is None else cand + base.view(-1, 1)).reshape(-1)
    skeys, order = torch.sort(keys, stable=True)
    edges = torch.arange(n_rows + 1, dtype=keys.dtype, device=keys.device)
    return torch.searchsorted(skeys, edges, out_int32=True), order.to(torch.int32)


def _cached_l1_slots(holder, cand, base, n_rows):
    """l1_slots kept in `holder` = the loss inputs of a sample set (TKG_Module.loss_inputs documents the key; per_sample_set keeps
    the dict for as long as the caller injects the same samples).  The entry is valid for the candidate matrix and the table size
    it was built from: `base` is holder["window"] times the entities per window, so it follows from those two.  Fresh negatives
    are a new candidate tensor and sort again every step."""
    c = holder.get("_l1_slots")
    if c is None or c[0] is not cand or c[1] != n_rows:
        c = holder["_l1_slots"] = (cand, n_rows) + l1_slots(cand, base, n_rows)
    return c[2], c[3]


# -- stages every node shares ---------------------------------------------------------------------------------------------------
def _scale(d_loss):
    return d_loss.reshape(1).contiguous()


def _segment_sum(be, rows, inverse, n):
    return be.segment_sum_rows(rows, inverse[0], inverse[1], n)


def _query_fwd(be, kind, rows, rel, inp):
    return be.bilinear_query_fwd(kind, rows, inp["known"], rel, inp["rel"], inp["is_tail"])


def _query_bwd(be, kind, rows, rel, inp, d_q):
    """-> (d_rows: the known rows' gradient summed over the static index list, the per-row gradient of the relation rows)."""
    dk, dr = be.bilinear_query_bwd(kind, rows, inp["known"], rel, inp["rel"], inp["is_tail"], d_q)
    return _segment_sum(be, dk, inp["known_inv"], rows.shape[0]), dr


def _mix_adjoint(d_m, w):
    """The adjoint of lerp(s_rec, s_loc, w) on the two score matrices."""
    d_sl = d_m * w
    return d_sl, d_m - d_sl


def _mix_weight_grad(G, s_l, s_r):
    """d_w = sum_k G_k (s_loc - s_rec), G the gradient of the mixed scores."""
    return (G * (s_l - s_r)).sum(dim=1, keepdim=True)


# -- the gated stages on a backend without the gated kernels (the CPU test backend) -----------------------------------------------
def _gated_query_fwd(be, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail):
    if hasattr(be, "gated_query_fwd"):
        return be.gated_query_fwd(kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail)
    # the mix in torch, the fold through bilinear_query
    known = _gated_known(a_rows, a_idx, b_rows, b_idx, w)[0]
    rows = torch.arange(known.shape[0], dtype=torch.int32, device=known.device)
    return be.bilinear_query_fwd(kind, known, rows, rel, rel_idx, is_tail)


def _gated_known(a_rows, a_idx, b_rows, b_idx, w):
    gated = (a_idx >= 0).view(-1, 1)
    b = b_rows[b_idx.long()]
    a = a_rows[a_idx.long().clamp(min=0)]
    wc = w.reshape(-1, 1)
    return torch.where(gated, wc * a + (1 - wc) * b, b), a, b, gated


def _gated_query_bwd(be, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail, d_q):
    if hasattr(be, "gated_query_bwd"):
        return be.gated_query_bwd(kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail, d_q)
    known, a, b, gated = _gated_known(a_rows, a_idx, b_rows, b_idx, w)
    rows = torch.arange(known.shape[0], dtype=torch.int32, device=known.device)
    dk, dr = be.bilinear_query_bwd(kind, known, rows, rel, rel_idx, is_tail, d_q)
    wc = w.reshape(-1, 1)
    zero = torch.zeros_like(dk)
    return (torch.where(gated, wc * dk, zero), torch.where(gated, (1 - wc) * dk, dk), dr,
            torch.where(gated, dk * (a - b), zero).sum(dim=1))


def _gather_ce_mix_fwd(be, s_a, s_b, w, cand):
    if hasattr(be, "gather_ce_mix_fwd"):
        return be.gather_ce_mix_fwd(s_a, s_b, w, cand)
    return be.gather_ce_fwd(torch.lerp(s_b, s_a, w.reshape(-1, 1)), cand)


def _gather_ce_mix_bwd(be, s_a, s_b, w, cand, lse, scale, inv_rows, row_scale):
    if hasattr(be, "gather_ce_mix_bwd"):
        return be.gather_ce_mix_bwd(s_a, s_b, w, cand, lse, scale, inv_rows, row_scale)
    wc = w.reshape(-1, 1)
    g = be.gather_ce_bwd(torch.lerp(s_b, s_a, wc), cand, lse, scale, inv_rows, row_scale)
    d_a = g * wc
    return d_a, g - d_a, (g * (s_a - s_b)).sum(dim=1)


# -- the dot candidate calls on a backend without them (the CPU test backend): the kernels' contract in torch -----------------------
def _cand_rows(base, cand):
    return cand.long() if base is None else cand.long() + base.long().view(-1, 1)


def dot_ce_rows_torch(q, table, base, cand, table_b=None, w=None):
    """The contract of temp_dot_ce_fwd (table_b and w given: temp_dot_mix_ce_fwd, table = table_a) in plain torch, differentiable and
    in the dtype of its inputs -> (s [P, C], loss_rows [P], lse [P]).  The reference of the kernels' tests (in float64, with autograd)
    and, with the hand-written adjoints below, the gather route of a backend without the dot methods."""
    rows = _cand_rows(base, cand)
    e = table[rows]                                                                   # (P, C, d)
    if table_b is not None:
        wc = w.reshape(-1, 1, 1)
        e = wc * e + (1 - wc) * table_b[rows]
    s = (q.unsqueeze(1) * e).sum(dim=-1)
    lse = torch.logsumexp(s, dim=1)
    return s, lse - s[:, 0], lse


def _dot_g(s, lse, scale, inv_rows, row_scale):
    g = torch.exp(s - lse.view(-1, 1))
    g[:, 0] -= 1.0
    f = scale.reshape(-1)[0] * (row_scale if row_scale is not None else torch.full_like(lse, float(inv_rows)))
    return g * f.view(-1, 1)


def _torch_dot_ce_fwd(q, table, base, cand):
    return dot_ce_rows_torch(q.detach(), table.detach(), base, cand)


def _torch_dot_mix_ce_fwd(q, table_a, table_b, w, base, cand):
    return dot_ce_rows_torch(q.detach(), table_a.detach(), base, cand, table_b.detach(), w.detach())


def _torch_dot_ce_bwd_q(q, table, base, cand, s, lse, scale, inv_rows, row_scale=None):
    g = _dot_g(s, lse, scale, inv_rows, row_scale)
    return g, torch.einsum("pk,pkd->pd", g, table.detach()[_cand_rows(base, cand)])


def _torch_dot_mix_ce_bwd_q(q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale=None):
    g = _dot_g(s, lse, scale, inv_rows, row_scale)
    rows, wc = _cand_rows(base, cand), w.detach().reshape(-1, 1, 1)
    ea, eb = table_a.detach()[rows], table_b.detach()[rows]
    d_q = torch.einsum("pk,pkd->pd", g, wc * ea + (1 - wc) * eb)
    return g, d_q, (g * torch.einsum("pd,pkd->pk", q.detach(), ea - eb)).sum(dim=1)


def _slot_terms(q, n_rows, slot_ptr, slot, g):
    """Per slot, in list order: (its table row, its query row p = slot // C, g[slot] q[p])."""
    sl = slot.long()
    p = sl // g.shape[1]
    row = torch.repeat_interleave(torch.arange(n_rows, device=q.device), (slot_ptr[1:] - slot_ptr[:-1]).long())
    return row, p, g.reshape(-1)[sl].view(-1, 1) * q.detach()[p]


def _torch_dot_ce_bwd_table(q, table, slot_ptr, slot, g):
    row, _, t = _slot_terms(q, table.shape[0], slot_ptr, slot, g)
    return torch.zeros_like(table).index_add_(0, row, t)


def _torch_dot_mix_ce_bwd_table(q, table_a, table_b, w, slot_ptr, slot, g):
    row, p, t = _slot_terms(q, table_a.shape[0], slot_ptr, slot, g)
    wp = w.detach().reshape(-1)[p].view(-1, 1)
    return torch.zeros_like(table_a).index_add_(0, row, wp * t), torch.zeros_like(table_b).index_add_(0, row, (1 - wp) * t)


_DOT_TORCH = {f.__name__[len("_torch_"):]: f for f in (_torch_dot_ce_fwd, _torch_dot_ce_bwd_q, _torch_dot_ce_bwd_table, _torch_dot_mix_ce_fwd,
                                                       _torch_dot_mix_ce_bwd_q, _torch_dot_mix_ce_bwd_table)}


def _dot_fn(be, name):
    """The backend's dot candidate method `name`, or its torch form on a backend without it."""
    return getattr(be, name) if hasattr(be, name) else _DOT_TORCH[name]


# -- the two scorers ------------------------------------------------------------------------------------------------------------
# A scorer is made in a node's forward from the loss inputs and the all-entity stack and kept on the node (the one tensor it holds,
# the L1 scorer's `base`, is saved by the node as well).  Every *_fwd also returns what the node saves for the matching *_bwd (`saved`).
class _GemmScorer:
    """distmult / complex: the score is bilinear in (query, candidate), so every live window's rows are scored against ALL its
    entities (one multi-problem launch over the windows) and the candidate CE reads the (rows, N) matrix."""

    def __init__(self, kind, inp, big):
        self.kind, self.inp, self.tall = kind, inp, False
        self.N = big.shape[0] // len(inp["splits"])
        self.live = [(b, a0, a1) for b, (a0, a1) in enumerate(inp["splits"]) if a1 > a0]     # the windows that have rows

    def _rows(self, x):
        return [x[a0:a1] for _, a0, a1 in self.live]

    def _blocks(self, big, cols=None):
        """Every live window's block of the stack; cols = (c0, c1): its entities c0 .. c1 - 1 alone (a column panel of the scores)."""
        c0, c1 = (0, self.N) if cols is None else cols
        return [big[b * self.N + c0:b * self.N + c1] for b, _, _ in self.live]

    def _dbig_like(self, big):
        """The gradient buffer of `big`: every live window's block is written whole, so only a batch with an empty window needs zeros."""
        return torch.empty_like(big) if len(self.live) == len(self.inp["splits"]) else torch.zeros_like(big)

    def scores(self, be, q, big, cols=None):
        """scores = q[rows of window b] . big_b^T for every live window -> (rows, N), one launch (cols: (rows, c1 - c0), see _blocks)."""
        scores = torch.empty(q.shape[0], self.N if cols is None else cols[1] - cols[0], dtype=torch.float32, device=q.device)
        be.linear_multi(self._rows(q), self._blocks(big, cols), True, scores)
        return scores

    def dq(self, be, d_s, q, big, cols=None):
        """d_q = d_scores_b . big_b for every live window, one launch (cols: the panel's share of it)."""
        d_q = torch.empty_like(q)
        be.linear_multi(self._rows(d_s), self._blocks(big, cols), False, d_q)
        return d_q

    def dbig(self, be, d_s, q, big, cols=None, out=None):
        """d_big_b = d_scores_b^T . q_b for every live window (cols: the panel's rows of every block, written into `out`)."""
        d_big = self._dbig_like(big) if out is None else out
        if hasattr(be, "linear_tn_multi"):                                                    # one launch
            be.linear_tn_multi(self._rows(d_s), self._rows(q), self._blocks(d_big, cols))
        else:
            for (_, a0, a1), dst in zip(self.live, self._blocks(d_big, cols)):
                be.linear_tn(d_s[a0:a1], q[a0:a1], out=dst)
        return d_big

    def ce_fwd(self, be, q, big):
        # few positives against many entities (ICEWS-like: ~200 rows x 10 000 entities per window): the ENTITY axis is made the
        # tall one of every GEMM -- scores = (all_b . q_b^T)^T through a transposed-store epilogue, and the backward products
        # from d_scores^T.  (The planner pads every window's block to a multiple of 4 rows so it can be an N / K extent.)
        self.tall = _TALL_SCORES and all((a1 - a0) % 4 == 0 and 8 * (a1 - a0) <= self.N for _, a0, a1 in self.live)
        if self.tall:
            scores = torch.empty(q.shape[0], self.N, dtype=torch.float32, device=q.device)
            for (_, a0, a1), all_b in zip(self.live, self._blocks(big)):
                be.linear_t(all_b, q[a0:a1], True, scores[a0:a1])
        else:
            scores = self.scores(be, q, big)
        loss_rows, lse = be.gather_ce_fwd(scores, self.inp["cand"])
        return loss_rows, (scores, lse)

    def ce_bwd(self, be, q, big, saved, scale):
        scores, lse = saved
        d_scores = be.gather_ce_bwd(scores, self.inp["cand"], lse, scale, 1.0, self.inp["weights"])
        if not self.tall:
            return self.dq(be, d_scores, q, big), self.dbig(be, d_scores, q, big)
        d_q = torch.empty_like(q)
        d_big = self._dbig_like(big)
        for (_, a0, a1), all_b, d_all in zip(self.live, self._blocks(big), self._blocks(d_big)):
            dst = d_scores[a0:a1].t().contiguous()                                        # (N, rows of window b)
            be.linear_tn(dst, all_b, out=d_q[a0:a1])                                      # d_q   = d_scores . all_b
            d_all.copy_(be.linear(dst, q[a0:a1], False))                                  # d_all = d_scores^T . q
        return d_q, d_big

    def mixed_ce_fwd(self, be, mixed):
        loss_rows, lse = be.gather_ce_fwd(mixed, self.inp["cand"])
        return loss_rows, lse, ()

    def mixed_ce_bwd(self, be, mixed, lse, w, saved, scale):
        """-> (the gradient of the mixed scores, each stream's share of it)."""
        d_m = be.gather_ce_bwd(mixed, self.inp["cand"], lse, scale, 1.0, self.inp["weights"])
        return d_m, _mix_adjoint(d_m, w)

    def stream_bwd(self, be, q, big, d_s, mixed, lse, saved, scale):
        return None, self.dq(be, d_s, q, big), self.dbig(be, d_s, q, big)

    def mixed_grad(self, d_m, gs):
        return d_m

    def gated_ce_fwd(self, be, q, big_loc, big_rec, w_cand):
        # the candidate mix is linear in the candidate, so it lives on the two score matrices (the same q for both)
        s_a, s_b = [self.scores(be, q, big) for big in (big_loc, big_rec)]
        loss_rows, lse = _gather_ce_mix_fwd(be, s_a, s_b, w_cand, self.inp["cand"])
        return loss_rows, (s_a, s_b, lse)

    def gated_ce_bwd(self, be, q, big_loc, big_rec, w_cand, saved, scale):
        s_a, s_b, lse = saved
        d_sa, d_sb, d_wc = _gather_ce_mix_bwd(be, s_a, s_b, w_cand, self.inp["cand"], lse, scale, 1.0, self.inp["weights"])
        d_q = self.dq(be, d_sa, q, big_loc)
        d_q2 = self.dq(be, d_sb, q, big_rec)
        d_q += d_q2
        return d_q, self.dbig(be, d_sa, q, big_loc), self.dbig(be, d_sb, q, big_rec), d_wc


class _GatherScorer:
    """The score at the candidates alone, s[row, k] = op(q[row], big[window(row) * N + cand[row, k]]), ALL windows' rows in one launch;
    the candidate side of the adjoint runs over the slot lists (_cached_l1_slots).  op "l1": transE, -|q - e|_1, which is not linear in
    the candidate, so the gated mix cannot live on two score matrices: the mix kernels read both all-entity rows of every candidate.
    op "dot": the bilinear scorers' <q, e> through the same three kernels (route "gather"): no (rows, N) matrix and no ceiling on N."""
    op = "l1"

    def __init__(self, kind, inp, big):
        self.kind, self.inp, self.n_rows = kind, inp, big.shape[0]
        self.base = inp["window"] * (big.shape[0] // len(inp["splits"]))             # every row's offset into the all-entity stack

    def _fn(self, be, name):
        """The backend's method of this operation (l1_ce_fwd, dot_mix_ce_bwd_q, ...); the dot form on a backend without it -- the
        CPU test backend -- is the same contract in torch (dot_ce_rows_torch and its adjoints, below)."""
        m = "%s_%s" % (self.op, name)
        return _dot_fn(be, m) if self.op == "dot" else getattr(be, m)

    def _slots(self, base):
        return _cached_l1_slots(self.inp, self.inp["cand"], base, self.n_rows)

    def ce_fwd(self, be, q, big):
        s, loss_rows, lse = self._fn(be, "ce_fwd")(q, big, self.base, self.inp["cand"])
        return loss_rows, (s, lse, self.base)

    def ce_bwd(self, be, q, big, saved, scale):
        s, lse, base = saved
        g, d_q = self._fn(be, "ce_bwd_q")(q, big, base, self.inp["cand"], s, lse, scale, 1.0, self.inp["weights"])
        slot_ptr, slot = self._slots(base)
        return d_q, self._fn(be, "ce_bwd_table")(q, big, slot_ptr, slot, g)

    def scores(self, be, q, big):
        return self._fn(be, "ce_fwd")(q, big, self.base, self.inp["cand"])[0]               # (its lse and loss are not used)

    def mixed_ce_fwd(self, be, mixed):
        lse = torch.logsumexp(mixed, dim=1)
        return lse - mixed[:, 0], lse, (self.base,)

    def mixed_ce_bwd(self, be, mixed, lse, w, saved, scale):
        """-> (nothing yet, each stream's row scale): the kernels get the MIXED softmax, so row_scale = weights * w resp.
        weights * (1 - w) gives each stream's score gradient."""
        wv = w.reshape(-1)
        self._slots(saved[0])                                                        # (sorted here, before the first stream)
        return None, (self.inp["weights"] * wv, self.inp["weights"] * (1 - wv))

    def stream_bwd(self, be, q, big, rs, mixed, lse, saved, scale):
        base, = saved
        g, d_q = self._fn(be, "ce_bwd_q")(q, big, base, self.inp["cand"], mixed, lse, scale, 1.0, rs.contiguous())
        slot_ptr, slot = self._slots(base)
        return g, d_q, self._fn(be, "ce_bwd_table")(q, big, slot_ptr, slot, g)

    def mixed_grad(self, _, gs):
        return gs[0] + gs[1]                                                         # g_loc + g_rec = the unsplit mixed-score gradient

    def gated_ce_fwd(self, be, q, big_loc, big_rec, w_cand):
        s, loss_rows, lse = self._fn(be, "mix_ce_fwd")(q, big_loc, big_rec, w_cand, self.base, self.inp["cand"])
        return loss_rows, (s, lse, self.base)

    def gated_ce_bwd(self, be, q, big_loc, big_rec, w_cand, saved, scale):
        s, lse, base = saved
        g, d_q, d_wc = self._fn(be, "mix_ce_bwd_q")(q, big_loc, big_rec, w_cand, base, self.inp["cand"], s, lse, scale, 1.0, self.inp["weights"])
        slot_ptr, slot = self._slots(base)
        d_big_loc, d_big_rec = self._fn(be, "mix_ce_bwd_table")(q, big_loc, big_rec, w_cand, slot_ptr, slot, g)
        return d_q, d_big_loc, d_big_rec, d_wc


class _L1Scorer(_GatherScorer):
    """transE (the L1 kernels)."""


class _DotGatherScorer(_GatherScorer):
    """distmult / complex / simple on the gather route (the dot kernels)."""
    op = "dot"


ROUTES = (None, "gemm", "gather")


def dot_gather_supported(be=None):
    """True when the installed backend has the inner-product candidate kernels (the gather route's own launches)."""
    be = get_backend() if be is None else be
    return all(hasattr(be, m) for m in _DOT_METHODS + _DOT_MIX_METHODS)


def bilinear_route(route, n_ents, be=None):
    """The route of a bilinear scorer's sampled loss: "gemm" (scores against all entities, _GemmScorer) or "gather" (the candidates
    alone, _DotGatherScorer).  None = auto: "gemm" unless the per-window entity count is above the LDS ceiling of temp_gather_ce_bwd
    (_lib.GATHER_CE_BWD_MAX_N) and the backend has the dot kernels."""
    if route not in ROUTES:
        raise ValueError("route must be None, 'gemm' or 'gather', not %r" % (route,))
    if route is None:
        return "gather" if n_ents > GATHER_CE_BWD_MAX_N and dot_gather_supported(be) else "gemm"
    return route


def _scorer(kind, inp, big, route=None):
    if kind == "transE":
        return _L1Scorer(kind, inp, big)
    gather = bilinear_route(route, big.shape[0] // len(inp["splits"])) == "gather"
    return (_DotGatherScorer if gather else _GemmScorer)(kind, inp, big)


# -- the batched nodes ----------------------------------------------------------------------------------------------------------
class _BatchedLinkPredictionFn(torch.autograd.Function):
    """The whole batched link-prediction loss as ONE autograd node:
        q    = bilinear_query(ent_rows[known], rel[rel_idx])                     (gathers fused, temp_bilinear_query_fwd)
        loss = sum_rows w_row * CE(score(q[row], candidates of the row), label 0)     (the scorer's ce_fwd)
    The backward mirrors it and reduces the per-row gradients of the gathered operands with deterministic segment sums."""

    @staticmethod
    def forward(ctx, ent_rows, rel, big, kind, inp, route=None):
        be = get_backend()
        sc = _scorer(kind, inp, big, route)
        q = _query_fwd(be, kind, ent_rows, rel, inp)
        loss_rows, saved = sc.ce_fwd(be, q, big)
        ctx.save_for_backward(ent_rows, rel, big, q, *saved)
        ctx.scorer = sc
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        ent_rows, rel, big, q = ctx.saved_tensors[:4]
        sc, be = ctx.scorer, get_backend()
        d_q, d_big = sc.ce_bwd(be, q, big, ctx.saved_tensors[4:], _scale(d_loss))
        d_ent, dr = _query_bwd(be, sc.kind, ent_rows, rel, sc.inp, d_q)
        return d_ent, _segment_sum(be, dr, sc.inp["rel_inv"], rel.shape[0]), d_big, None, None, None


class _BatchedEnsembleLinkPredictionFn(torch.autograd.Function):
    """_BatchedLinkPredictionFn for the score-level ensemble of the post-ensemble models (combined_scores,
    models/PostDynamicRGCN.py:404-406, 425-428): TWO streams (local = pre-GRU, temporal = post-GRU) score their own query against
    their own all-entity stack with the plain node's launches, the scores are mixed row by row with w (local) and 1 - w
    (temporal), then the candidate cross-entropy of the mix."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w, kind, inp, route=None):
        be = get_backend()
        sc = _scorer(kind, inp, big_loc, route)
        qs, ss = [], []
        for rows, big in ((loc_rows, big_loc), (rec_rows, big_rec)):
            qs.append(_query_fwd(be, kind, rows, rel, inp))
            ss.append(sc.scores(be, qs[-1], big))
        mixed = torch.lerp(ss[1], ss[0], w)                          # w (rows, 1): w * local + (1 - w) * temporal
        loss_rows, lse, saved = sc.mixed_ce_fwd(be, mixed)
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w, qs[0], qs[1], ss[0], ss[1], mixed, lse, *saved)
        ctx.scorer = sc
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w, q_l, q_r, s_l, s_r, mixed, lse = ctx.saved_tensors[:12]
        saved = ctx.saved_tensors[12:]
        sc, be = ctx.scorer, get_backend()
        scale = _scale(d_loss)
        d_m, parts = sc.mixed_ce_bwd(be, mixed, lse, w, saved, scale)
        outs, d_rel, gs = [], None, []
        for rows, big, q, part in ((loc_rows, big_loc, q_l, parts[0]), (rec_rows, big_rec, q_r, parts[1])):
            g, d_q, d_big = sc.stream_bwd(be, q, big, part, mixed, lse, saved, scale)
            gs.append(g)
            d_rows, dr = _query_bwd(be, sc.kind, rows, rel, sc.inp, d_q)
            outs.append((d_rows, d_big))
            d_rel = dr if d_rel is None else d_rel + dr
        d_rel = _segment_sum(be, d_rel, sc.inp["rel_inv"], rel.shape[0])
        d_w = _mix_weight_grad(sc.mixed_grad(d_m, gs), s_l, s_r) if ctx.needs_input_grad[5] else None
        return outs[0][0], outs[1][0], d_rel, outs[0][1], outs[1][1], d_w, None, None, None


class _BatchedGatedLinkPredictionFn(torch.autograd.Function):
    """The embedding-level gated loss of the post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN.train_link_prediction,
    models/PostDynamicRGCN.py:261-282) over ALL windows as one autograd node:
        q    = fold(w_known * loc_rows[known_a] + (1 - w_known) * rec_rows[known], rel)      (temp_gated_query_fwd; known_a < 0:
                                                                                           the temporal row alone -- the head rows)
        loss = sum_rows w_row * CE(score(q[row], w_cand * big_loc[c] + (1 - w_cand) * big_rec[c]) over the row's candidates c, label 0)
    The backward: the scorer's gated_ce_bwd (d_q, both stacks' gradients, d_w_cand), one gated-query pass, three segment sums."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, kind, inp, route=None):
        be = get_backend()
        sc = _scorer(kind, inp, big_loc, route)
        q = _gated_query_fwd(be, kind, loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"], inp["is_tail"])
        loss_rows, saved = sc.gated_ce_fwd(be, q, big_loc, big_rec, w_cand)
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q, *saved)
        ctx.scorer = sc
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q = ctx.saved_tensors[:8]
        sc, be = ctx.scorer, get_backend()
        inp = sc.inp
        d_q, d_big_loc, d_big_rec, d_wc = sc.gated_ce_bwd(be, q, big_loc, big_rec, w_cand, ctx.saved_tensors[8:], _scale(d_loss))
        da, db, dr, d_wk = _gated_query_bwd(be, sc.kind, loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"],
                                            inp["is_tail"], d_q)
        d_loc = _segment_sum(be, da, inp["known_a_inv"], loc_rows.shape[0])
        d_rec = _segment_sum(be, db, inp["known_inv"], rec_rows.shape[0])
        d_rel = _segment_sum(be, dr, inp["rel_inv"], rel.shape[0])
        return (d_loc, d_rec, d_rel, d_big_loc, d_big_rec, d_wk.reshape(w_known.shape) if ctx.needs_input_grad[5] else None,
                d_wc.reshape(w_cand.shape) if ctx.needs_input_grad[6] else None, None, None, None)


def batched_link_prediction(ent_rows, rel, big, kind, inputs, route=None):
    """sum over windows of CE_tail + CE_head (models/DynamicRGCN.py:186-193) for scorer `kind` ('distmult' | 'complex' | 'simple': the
    GEMM scorer or, by `route` (bilinear_route: None | 'gemm' | 'gather'), the candidate-gather scorer; 'transE': the L1 scorer);
    `inputs` = TKG_Module.loss_inputs(...)."""
    return _BatchedLinkPredictionFn.apply(ent_rows, rel, big, kind, inputs, route)


# -- the all-entity ("1-vs-all") objective ------------------------------------------------------------------------------------------
# A live (rows, N) score matrix of the all-entity node stays at or under this many bytes (evaluation.TOPK_PANEL_BYTES, the project's
# bound for one); above it the node works in column panels with the carry of temp_filtered_ce_fwd.
ALL_ENTITY_PANEL_BYTES = 256 << 20


def _filtered_columns(P, n, truth, lo, hi, ids, col0, device):
    """bool (P, n): column j of row p is FILTERED -- entity col0 + j is in ids[lo[p] .. hi[p]) and is not truth[p]."""
    mask = torch.zeros(P, n, dtype=torch.bool, device=device)
    if lo is not None and P:
        cnt = (hi - lo).long()
        row = torch.repeat_interleave(torch.arange(P, device=device), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        pos = lo.long()[row] + torch.arange(row.shape[0], device=device) - first[row]
        col = ids.long()[pos] - col0
        ok = (col >= 0) & (col < n) & (ids.long()[pos] != truth.long()[row])
        mask[row[ok], col[ok]] = True
    return mask


def filtered_ce_rows_torch(scores, truth, lo, hi, ids, col0=0, n=None):
    """The contract of temp_filtered_ce_fwd (one call, carry = 0) in plain torch, differentiable and in the dtype of `scores`
    -> (loss_rows [P], lse_rows [P]): the filtered columns (in the row's list ids[lo[p] .. hi[p]) and not the truth; lo None: none)
    and the columns from n on masked to -inf, logsumexp, minus the truth's score (0 when the truth lies outside col0 .. col0 + n - 1).
    The reference of the kernels' tests (in float64, with autograd for d_scores) and, through _filtered_ce_fwd / _filtered_ce_bwd,
    the route of a backend without them."""
    P, n = scores.shape[0], scores.shape[1] if n is None else int(n)
    x = scores[:, :n].masked_fill(_filtered_columns(P, n, truth, lo, hi, ids, col0, scores.device), float("-inf"))
    lse = torch.logsumexp(x, dim=1)
    jt = truth.long() - col0
    inside = (jt >= 0) & (jt < n)
    ts = torch.where(inside, scores.gather(1, jt.clamp(0, n - 1).view(-1, 1)).view(-1), torch.zeros_like(lse))
    return lse - ts, lse


def _filtered_ce_fwd(be, scores, truth, lo, hi, ids, col0, carry):
    """backend.filtered_ce_fwd, or -- on a backend without it, the CPU test backend -- its contract in torch, the carry included."""
    if hasattr(be, "filtered_ce_fwd"):
        return be.filtered_ce_fwd(scores, truth, lo, hi, ids, col0=col0, carry=carry)
    scores = scores.detach()
    P, n = scores.shape
    x = scores.masked_fill(_filtered_columns(P, n, truth, lo, hi, ids, col0, scores.device), float("-inf"))
    m = x.max(dim=1).values if n else x.new_full((P,), float("-inf"))
    s = torch.where(m > float("-inf"), torch.exp(x - m.clamp(min=torch.finfo(x.dtype).min).view(-1, 1)).sum(dim=1), torch.zeros_like(m))
    jt = truth.long() - col0
    inside = (jt >= 0) & (jt < n)
    here = scores.gather(1, jt.clamp(0, n - 1).view(-1, 1)).view(-1)
    if carry is None:
        ts = torch.where(inside, here, torch.zeros_like(here))
    else:
        om, os_, ots = carry[0], carry[1], carry[2]
        nm = torch.maximum(om, m)
        ref = nm.clamp(min=torch.finfo(x.dtype).min)
        s = (torch.where(om > float("-inf"), os_ * torch.exp(om - ref), torch.zeros_like(s))
             + torch.where(m > float("-inf"), s * torch.exp(m - ref), torch.zeros_like(s)))
        m, ts = nm, torch.where(inside, here, ots)
    lse = m + torch.log(s)
    return lse - ts, lse, torch.stack([m, s, ts])


def _filtered_ce_bwd(be, scores, truth, lo, hi, ids, col0, lse, scale, row_scale):
    if hasattr(be, "filtered_ce_bwd"):
        return be.filtered_ce_bwd(scores, truth, lo, hi, ids, lse, scale, 1.0, row_scale, col0=col0)
    scores = scores.detach()
    P, n = scores.shape
    filt = _filtered_columns(P, n, truth, lo, hi, ids, col0, scores.device)
    g = torch.exp(scores - lse.view(-1, 1)).masked_fill(filt, 0.0)
    jt = truth.long() - col0
    inside = ((jt >= 0) & (jt < n)).nonzero().view(-1)
    g[inside, jt[inside]] -= 1.0
    w = (scale.reshape(-1)[0] * row_scale).view(-1, 1)
    return torch.where(w != 0, g * w, torch.zeros_like(g))


def all_entity_panel(panel, rows, N):
    """Columns per pass of the all-entity node: `panel` when given (a positive multiple of 4), else all N while the (rows, N)
    score matrix stays at or under ALL_ENTITY_PANEL_BYTES, else as many columns as do."""
    if panel is None:
        per = 4 * max(rows, 1)
        panel = N if per * N <= ALL_ENTITY_PANEL_BYTES else max(4, ALL_ENTITY_PANEL_BYTES // per // 4 * 4)
    if panel <= 0 or panel % 4:
        raise ValueError("batched_all_entity_link_prediction: panel must be a positive multiple of 4")
    return min(int(panel), N)


class _BatchedAllEntityLinkPredictionFn(torch.autograd.Function):
    """_BatchedLinkPredictionFn with the all-entity objective in the place of the candidate lists:
        q    = bilinear_query(ent_rows[known], rel[rel_idx])
        loss = sum_rows w_row * CE(score(q[row], e) over EVERY entity e of the row's window outside its known-true list, label = truth)
    (temp_filtered_ce_*: the row's list is the plan's ids[lo .. hi), the truth stays in).  Per column panel, forward and backward in
    the same order: linear_multi over the live windows' sub-blocks, filtered_ce_fwd with the carry | the panel's scores again (kept
    when the panel is the whole row), filtered_ce_bwd, d_q += linear_multi (a plain add, panel by panel), d_big[panel] =
    linear_tn_multi; then bilinear_query_bwd and the two segment sums.  Nothing is drawn: same inputs, same bits."""

    @staticmethod
    def forward(ctx, ent_rows, rel, big, kind, inp, panel):
        be = get_backend()
        sc = _GemmScorer(kind, inp, big)
        if sc.N % 4:
            raise ValueError("batched_all_entity_link_prediction: the entity count must be a multiple of 4")
        q = _query_fwd(be, kind, ent_rows, rel, inp)
        panel = all_entity_panel(panel, q.shape[0], sc.N)
        state = kept = None
        for c0 in range(0, sc.N, panel):
            cols = (c0, min(sc.N, c0 + panel))
            kept = sc.scores(be, q, big, cols)
            loss_rows, lse, state = _filtered_ce_fwd(be, kept, inp["truth"], inp["lo"], inp["hi"], inp["ids"], c0, state)
        whole = panel >= sc.N
        ctx.save_for_backward(ent_rows, rel, big, q, lse, *([kept] if whole else []))
        ctx.scorer, ctx.panel = sc, panel
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        ent_rows, rel, big, q, lse = ctx.saved_tensors[:5]
        sc, be, panel = ctx.scorer, get_backend(), ctx.panel
        inp, scale = sc.inp, _scale(d_loss)
        d_big, d_q = sc._dbig_like(big), None
        for c0 in range(0, sc.N, panel):
            cols = (c0, min(sc.N, c0 + panel))
            s = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else sc.scores(be, q, big, cols)
            d_s = _filtered_ce_bwd(be, s, inp["truth"], inp["lo"], inp["hi"], inp["ids"], c0, lse, scale, inp["weights"])
            part = sc.dq(be, d_s, q, big, cols)
            d_q = part if d_q is None else d_q.add_(part)
            sc.dbig(be, d_s, q, big, cols, out=d_big)
        d_ent, dr = _query_bwd(be, sc.kind, ent_rows, rel, inp, d_q)
        return d_ent, _segment_sum(be, dr, inp["rel_inv"], rel.shape[0]), d_big, None, None, None


def batched_all_entity_link_prediction(ent_rows, rel, big, kind, inputs, panel=None):
    """sum over windows of CE_tail + CE_head against ALL entities outside each row's known-true list ("1-vs-all", see
    _BatchedAllEntityLinkPredictionFn) for a bilinear scorer `kind` (scores.BILINEAR); `inputs` = sampling.plan_batch_loss(...):
    known / rel / is_tail / weights / splits / the inverses, and truth, lo, hi, ids in the place of candidate lists.  `panel`: score
    columns per pass (a multiple of 4; default all_entity_panel)."""
    from .scores import BILINEAR
    if kind not in BILINEAR:
        raise ValueError("batched_all_entity_link_prediction: no all-entity node for the scorer %r" % (kind,))
    return _BatchedAllEntityLinkPredictionFn.apply(ent_rows, rel, big, kind, inputs, panel)


def batched_ensemble_link_prediction(loc_rows, rec_rows, rel, big_loc, big_rec, w, kind, inputs, route=None):
    """sum over windows of the ensemble CE_tail + CE_head; `w` (rows, 1) = weight of the LOCAL stream of every stacked query row
    (per window: [tail rows: weight_object ; head rows: weight_subject]); `inputs` = TKG_Module.loss_inputs(...); `route` as in
    batched_link_prediction."""
    w = w.reshape(-1, 1).to(loc_rows.dtype).contiguous()
    return _BatchedEnsembleLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(), big_rec.contiguous(),
                                                  w, kind, inputs, route)


def gated_loss_inputs(inp, n_loc_rows, device):
    """The loss inputs of TKG_Module.loss_inputs (head rows NOT scored as tails) completed for the gated node: known_a = the row of
    the LOCAL stream every query row mixes in -- the known subject's for tail rows, -1 (temporal only) for head rows, whose known
    object is the temporal row alone in the reference (models/PostDynamicRGCN.py:276-277) -- and its segment-sum inverse."""
    if inp is None:
        return None
    from .functional import gather_inverse
    out = dict(inp)
    ka = torch.where(inp["is_tail"] != 0, inp["known"], torch.full_like(inp["known"], -1)).contiguous()
    out["known_a"] = ka
    out["known_a_inv"] = gather_inverse(ka.cpu().numpy(), n_loc_rows, device)
    return out


def batched_gated_link_prediction(loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, kind, inputs, route=None):
    """sum over windows of the post-aggregation CE_tail + CE_head (see _BatchedGatedLinkPredictionFn).  w_known / w_cand (rows, 1):
    per window [tail rows: w_oqs / w_oqo ; head rows: w_sqo / w_sqs]; `inputs` = gated_loss_inputs(TKG_Module.loss_inputs(...)).
    big_loc / big_rec: the (B * N_ents, D) stacks of the windows' all-entity matrices.  kind 'distmult' | 'complex' | 'transE';
    `route` as in batched_link_prediction."""
    f = lambda t: t.reshape(-1, 1).to(loc_rows.dtype).contiguous()
    return _BatchedGatedLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(), big_rec.contiguous(),
                                               f(w_known), f(w_cand), kind, inputs, route)


def gated_link_prediction(loc, rec, rel, all_loc, all_rec, triplets, neg_tail, neg_head, w_sqs, w_sqo, w_oqs, w_oqo, kind, route=None):
    """loss_tail + loss_head of ONE target graph (models/PostDynamicRGCN.py:200-202): the per-window form of
    batched_gated_link_prediction for the unbatched path (one window, its own all-entity matrices)."""
    from .tkg_module import TKG_Module
    dev = loc.device
    smp = [(triplets.to(torch.int64), neg_tail, neg_head)]
    inp = gated_loss_inputs(TKG_Module.loss_inputs([0], smp, dev, loc.shape[0], rel.shape[0]), loc.shape[0], dev)
    if inp is None:
        return loc.sum() * 0.0
    w_known = torch.cat([w_oqs.reshape(-1, 1), w_sqo.reshape(-1, 1)])
    w_cand = torch.cat([w_oqo.reshape(-1, 1), w_sqs.reshape(-1, 1)])
    return batched_gated_link_prediction(loc, rec, rel, all_loc, all_rec, w_known, w_cand, kind, inp, route)


# -- two FROZEN streams: the only gradient is the mixing weight's ---------------------------------------------------------------------
FROZEN_KIND = {"distmult": "dot", "complex": "dot", "transE": "l1"}       # scorer -> the candidate score of frozen_mix_ce


def frozen_mix_ce_rows(q_a, T_a, q_b, T_b, w, cand, kind="dot", chunk=1 << 22):
    """The formula of temp_frozen_mix_ce in plain torch, differentiable and in the dtype of its inputs -> loss_rows [P]:
    a = score(q_a, T_a[cand]) ("dot": the inner product, "l1": -|q - row|_1), b likewise, CE(w a + (1 - w) b, label 0) per row.  The
    candidate rows are gathered `chunk` elements of (rows, C, D) at a time.  The route of a backend without `frozen_mix_ce` and the
    reference of the kernel's tests (in float64, with autograd for d_w)."""
    if kind not in ("dot", "l1"):
        raise ValueError("frozen_mix_ce_rows: kind must be 'dot' or 'l1'")
    P, C = cand.shape
    idx = cand.long()
    wc = w.reshape(-1, 1)
    out = []
    step = max(1, chunk // max(1, C * max(T_a.shape[1], T_b.shape[1])))
    for p0 in range(0, P, step):
        sl = slice(p0, p0 + step)
        ss = []
        for q, T in ((q_a, T_a), (q_b, T_b)):
            rows = T[idx[sl]]                                                        # (rows, C, D)
            qs = q[sl].unsqueeze(1)
            ss.append((qs * rows).sum(dim=-1) if kind == "dot" else -(qs - rows).abs().sum(dim=-1))
        x = wc[sl] * ss[0] + (1 - wc[sl]) * ss[1]
        out.append(torch.nn.functional.cross_entropy(x, torch.zeros(x.shape[0], dtype=torch.int64, device=x.device), reduction="none"))
    return torch.cat(out) if out else w.new_zeros(0)


def frozen_mix_ce(be, q_a, T_a, q_b, T_b, w, cand, row_scale=None, inv_rows=None, kind="dot"):
    """-> (loss_rows [P] unscaled, d_w [P] = scale_p * d loss_rows[p] / d w[p]): the backend's one-launch kernel, or -- on a backend
    without `frozen_mix_ce`, the CPU test backend -- frozen_mix_ce_rows and its autograd."""
    if hasattr(be, "frozen_mix_ce"):
        return be.frozen_mix_ce(q_a, T_a, q_b, T_b, w, cand, row_scale, inv_rows, kind)
    scale = row_scale if row_scale is not None else (1.0 / max(cand.shape[0], 1) if inv_rows is None else float(inv_rows))
    with torch.enable_grad():
        wv = w.detach().reshape(-1).clone().requires_grad_(True)
        loss_rows = frozen_mix_ce_rows(q_a.detach(), T_a.detach(), q_b.detach(), T_b.detach(), wv, cand, kind)
        d_w, = torch.autograd.grad((loss_rows * scale).sum(), wv)
    return loss_rows.detach(), d_w


def _frozen_cand(inp, n_ents):
    """The candidate lists of the loss inputs as rows of the (B * n_ents, D) stacks: cand + window * n_ents, kept in the dict (which
    callers cache per sample set) for the candidate tensor and the table size it was built from."""
    c = inp.get("_frozen_cand")
    if c is None or c[0] is not inp["cand"] or c[1] != n_ents:
        c = inp["_frozen_cand"] = (inp["cand"], n_ents, (inp["cand"] + (inp["window"] * n_ents).view(-1, 1)).contiguous())
    return c[2]


def _frozen_query(be, kind, rows, rel, inp):
    """The folded query of one frozen stream: the bilinear fold through the backend; the translation query known + r (tail) /
    known - r (head) as the tensor expression it is bit-equal to (one IEEE add or subtract), so that a backend without the L1
    kernels serves TransE too."""
    if kind != "transE":
        return _query_fwd(be, kind, rows, rel, inp)
    known, r = be.gather_rows(rows, inp["known"]), be.gather_rows(rel, inp["rel"])
    return torch.where(inp["is_tail"].view(-1, 1) != 0, known + r, known - r).contiguous()


class _FrozenMixCEFn(torch.autograd.Function):
    """The ensemble loss of two FROZEN streams (Aggregator, models/aggregator.py:185-208) over ALL windows as one node:
        q_x  = fold(rows_x[known], rel_x[rel])        per stream x in (a = local, b = temporal), its own relation table and width
        loss = sum_rows w_row * CE(mix(w, score(q_a, big_a[c]), score(q_b, big_b[c])) over the row's candidates c, label 0)
    Forward: bilinear_query_fwd x 2, frozen_mix_ce (ONE launch: the loss rows and d loss / d w together).  Backward: grad_out * d_w,
    no backend call -- nothing else has a gradient."""

    @staticmethod
    def forward(ctx, rows_a, rel_a, big_a, rows_b, rel_b, big_b, w, kind, inp):
        be = get_backend()
        q_a = _frozen_query(be, kind, rows_a, rel_a, inp)
        q_b = _frozen_query(be, kind, rows_b, rel_b, inp)
        cand = _frozen_cand(inp, big_a.shape[0] // len(inp["splits"]))
        loss_rows, d_w = frozen_mix_ce(be, q_a, big_a, q_b, big_b, w.reshape(-1), cand, inp["weights"], None, FROZEN_KIND[kind])
        ctx.save_for_backward(d_w)
        ctx.w_shape = w.shape
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        d_w, = ctx.saved_tensors
        return None, None, None, None, None, None, (d_loss * d_w).reshape(ctx.w_shape), None, None


def frozen_ensemble_link_prediction(rows_a, rel_a, big_a, rows_b, rel_b, big_b, w, kind, inputs):
    """sum over windows of the ensemble CE_tail + CE_head of two frozen models (see _FrozenMixCEFn).  rows_x: the concatenation of
    the per-graph target rows of stream x, rel_x its relation table, big_x the (B * N_ents, D_x) stack of its all-entity matrices
    (the two streams may differ in width); `w` (rows, 1) = weight of stream a of every stacked query row (per window: [tail rows:
    weight_object ; head rows: weight_subject]); kind 'distmult' | 'complex' | 'transE'; `inputs` = TKG_Module.loss_inputs(...).
    None of the six row / table arguments may require grad: the node returns no gradient for them."""
    if kind not in FROZEN_KIND:
        raise ValueError("frozen_ensemble_link_prediction: no frozen node for the scorer %r" % (kind,))
    for name, t in (("rows_a", rows_a), ("rel_a", rel_a), ("big_a", big_a), ("rows_b", rows_b), ("rel_b", rel_b), ("big_b", big_b)):
        assert not t.requires_grad, "frozen_ensemble_link_prediction: %s requires grad, but both streams are frozen" % name
    w = w.reshape(-1, 1).to(rows_a.dtype).contiguous()
    return _FrozenMixCEFn.apply(rows_a.contiguous(), rel_a.contiguous(), big_a.contiguous(), rows_b.contiguous(), rel_b.contiguous(),
                                big_b.contiguous(), w, kind, inputs)


# -- the unbatched nodes: one target graph, the query rows given -------------------------------------------------------------------
class _CandidateCEFn(torch.autograd.Function):
    """mean_p CE(query[p] . all_embeds[cand[p, :]]^T, label 0) without materialising (P, C, D)."""

    @staticmethod
    def forward(ctx, query, all_embeds, cand, route=None):
        be = get_backend()
        ctx.gather = bilinear_route(route, all_embeds.shape[0], be) == "gather"
        if ctx.gather:                                               # the candidates alone: the dot kernels with base = None
            scores, loss_rows, lse = _dot_fn(be, "dot_ce_fwd")(query, all_embeds, None, cand)
        else:
            scores = be.linear(query, all_embeds, True)              # (P, N): every positive against ALL entities
            loss_rows, lse = be.gather_ce_fwd(scores, cand)
        ctx.save_for_backward(query, all_embeds, scores, lse, cand)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, d_loss):
        query, all_embeds, scores, lse, cand = ctx.saved_tensors
        be = get_backend()
        if ctx.gather:
            g, d_query = _dot_fn(be, "dot_ce_bwd_q")(query, all_embeds, None, cand, scores, lse, _scale(d_loss), 1.0 / max(query.shape[0], 1))
            slot_ptr, slot = l1_slots(cand, None, all_embeds.shape[0])
            return d_query, _dot_fn(be, "dot_ce_bwd_table")(query, all_embeds, slot_ptr, slot, g), None, None
        d_scores = be.gather_ce_bwd(scores, cand, lse, _scale(d_loss), 1.0 / max(scores.shape[0], 1))
        d_query = be.linear(d_scores, all_embeds, False)             # (P,N) . (N,D)
        d_all = be.linear_tn(d_scores, query)                        # (N,P) . (P,D)
        return d_query, d_all, None, None


def candidate_cross_entropy(query, all_embeds, cand, route=None):
    """F.cross_entropy(score(query, all_embeds[cand]), 0) for scorers that are bilinear in (query, candidate) -- DistMult and ComplEx
    (utils/scores.py:4-44).  cand: int32 (P, C), column 0 is the true entity.  `route` (bilinear_route): scores against all entities
    ('gemm') or at the candidates alone ('gather'; None: above the LDS ceiling of temp_gather_ce_bwd)."""
    return _CandidateCEFn.apply(query, all_embeds, cand, route)


class _MixedCandidateCEFn(torch.autograd.Function):
    """mean_p CE( w_p * (q_loc[p] . A_loc[cand[p, :]]^T) + (1 - w_p) * (q_rec[p] . A_rec[cand[p, :]]^T), label 0 ): the score-level
    ensemble of the post-ensemble models (combined_scores, models/PostDynamicRGCN.py:404-406, 425-428) without the
    (P, 1 + neg, D) gathers: both streams score against ALL entities (two small GEMMs), the mix is one pass over the (P, N) score
    matrices, the candidate CE reads the mixed matrix."""

    @staticmethod
    def forward(ctx, q_loc, all_loc, q_rec, all_rec, w, cand, route=None):
        be = get_backend()
        ctx.gather = bilinear_route(route, all_loc.shape[0], be) == "gather"
        if ctx.gather:                                               # per-stream dot scores at the candidates, the mix in torch
            s_loc = _dot_fn(be, "dot_ce_fwd")(q_loc, all_loc, None, cand)[0]           # (P, C)
            s_rec = _dot_fn(be, "dot_ce_fwd")(q_rec, all_rec, None, cand)[0]
            mixed = torch.lerp(s_rec, s_loc, w)
            lse = torch.logsumexp(mixed, dim=1)
            loss_rows = lse - mixed[:, 0]
        else:
            s_loc = be.linear(q_loc, all_loc, True)                  # (P, N)
            s_rec = be.linear(q_rec, all_rec, True)
            mixed = torch.lerp(s_rec, s_loc, w)                      # w (P, 1): w * loc + (1 - w) * rec
            loss_rows, lse = be.gather_ce_fwd(mixed, cand)
        ctx.save_for_backward(q_loc, all_loc, q_rec, all_rec, w, cand, s_loc, s_rec, mixed, lse)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, d_loss):
        q_loc, all_loc, q_rec, all_rec, w, cand, s_loc, s_rec, mixed, lse = ctx.saved_tensors
        be = get_backend()
        if ctx.gather:                                               # the MIXED softmax into each stream's kernels, row_scale = w / P resp. (1 - w) / P
            inv, wv, scale = 1.0 / max(mixed.shape[0], 1), w.reshape(-1), _scale(d_loss)
            slot_ptr, slot = l1_slots(cand, None, all_loc.shape[0])
            outs, gs = [], []
            for q, table, rs in ((q_loc, all_loc, wv * inv), (q_rec, all_rec, (1 - wv) * inv)):
                g, d_q = _dot_fn(be, "dot_ce_bwd_q")(q, table, None, cand, mixed, lse, scale, 1.0, rs.contiguous())
                outs += [d_q, _dot_fn(be, "dot_ce_bwd_table")(q, table, slot_ptr, slot, g)]
                gs.append(g)
            d_w = _mix_weight_grad(gs[0] + gs[1], s_loc, s_rec) if ctx.needs_input_grad[4] else None
            return outs[0], outs[1], outs[2], outs[3], d_w, None, None
        d_mixed = be.gather_ce_bwd(mixed, cand, lse, _scale(d_loss), 1.0 / max(mixed.shape[0], 1))
        d_loc, d_rec = _mix_adjoint(d_mixed, w)
        d_w = _mix_weight_grad(d_mixed, s_loc, s_rec) if ctx.needs_input_grad[4] else None
        return (be.linear(d_loc, all_loc, False), be.linear_tn(d_loc, q_loc), be.linear(d_rec, all_rec, False), be.linear_tn(d_rec, q_rec),
                d_w, None, None)


def candidate_cross_entropy_mixed(q_loc, all_loc, q_rec, all_rec, w, cand, route=None):
    """Score-level ensemble CE (see _MixedCandidateCEFn).  w: (P, 1) mixing weight of the local stream; cand: int32 (P, C), column
    0 is the true entity; `route` as in candidate_cross_entropy."""
    return _MixedCandidateCEFn.apply(q_loc.contiguous(), all_loc.contiguous(), q_rec.contiguous(), all_rec.contiguous(),
                                     w.reshape(-1, 1).to(q_loc.dtype).contiguous(), cand, route)


class _TranslationCEFn(torch.autograd.Function):
    """mean_p CE(-|q[p] - all_embeds[cand[p, :]]|_1, label 0) without materialising (P, C, D)."""

    @staticmethod
    def forward(ctx, q, all_embeds, cand):
        s, loss_rows, lse = get_backend().l1_ce_fwd(q, all_embeds, None, cand)
        ctx.save_for_backward(q, all_embeds, cand, s, lse)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, d_loss):
        q, all_embeds, cand, s, lse = ctx.saved_tensors
        be = get_backend()
        g, d_q = be.l1_ce_bwd_q(q, all_embeds, None, cand, s, lse, _scale(d_loss), 1.0 / max(q.shape[0], 1))
        slot_ptr, slot = l1_slots(cand, None, all_embeds.shape[0])
        return d_q, be.l1_ce_bwd_table(q, all_embeds, slot_ptr, slot, g), None


def translation_cross_entropy(q, all_embeds, cand):
    """F.cross_entropy(transE score of the translation query q = s + r (tail) / o - r (head) against all_embeds[cand], 0)
    (utils/scores.py:46-55).  cand: int32 (P, C), column 0 is the true entity."""
    return _TranslationCEFn.apply(q.contiguous(), all_embeds.contiguous(), cand)
