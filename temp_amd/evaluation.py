"""Filtered link-prediction ranking with the interface of the reference's EvaluationFilter
(utils/evaluation.py:6-106): for every test triple, score the true subject (resp. object) against
ALL entities, mask the other entities known to be true for the same (relation, object) (resp.
(subject, relation)) at that timestamp in train+valid+test, and report the 1-indexed rank.

Restructured for the device:
  * the known-true sets are sorted composite keys, the per-triple filter lists come out of two
    `searchsorted` calls (no per-triple Python dict lookups) and are cached per (timestamp, split, mode)
    on the device;
  * DistMult / ComplEx are bilinear, so the P x N score matrix is ONE GEMM of the folded query against the
    all-entity table (`temp_linear`), never a (P, N, D) broadcast;
  * TransE is not bilinear: its P x N matrix of negative L1 distances is one register-tiled pass (`temp_l1_scores`) over the
    translation query, in place of the (100, N, D) broadcast per chunk of 100 triples;
  * the rank is the target's position in a stable descending order, computed by counting
    (`temp_filtered_rank`) instead of sorting; with `panel=` the count is carried across column panels
    (`temp_filtered_rank_stream`, `_mix` for the two-table models: the gate mix happens in registers), so the P x N matrix never
    exists at once -- every panel is then scored twice, once for the targets' scores and once for the count;
  * the ANSWERS of a query (s, r, ?, t) / (?, r, o, t) -- `topk_single_graph`, which the reference has no counterpart of -- are
    one selection pass over the same score rows (`temp_filtered_topk`): filter, total order (score, then entity id) and a
    list that is carried across column panels, so the Q x N matrix never has to exist at once;
  * the two-table post models score against a local and a temporal all-entity table and mix by per-query gates: their
    `topk_single_graph` hands the selection both score matrices and the weights (`temp_filtered_topk_mix`), and the mix happens
    in registers."""
import numpy as np
import torch

from . import _lib
from . import scores as S
from .backend import get_backend

# topk_single_graph scores all N entities in one matrix while Q * ld * 4 bytes stay under this; above it, panels of this many bytes
TOPK_PANEL_BYTES = 256 << 20


def _l1_route(name, be, d):
    """TransE scores come from the dense L1 kernel: a backend that has it, rows of whole float4s."""
    return name == "transE" and hasattr(be, "l1_scores") and d % 4 == 0


def _translation_query(known, r, mode):
    """q with transE(known, r, c) = -|q - c|_1: s + r for the tail mode, o - r for the head mode."""
    return (known + r if mode == "tail" else known - r).contiguous()


def topk_composite(scores, k, filt_ptr=None, filt_ids=None, keep=None, col0=0, n=None, carry=None):
    """The contract of `temp_filtered_topk` in plain torch: mask to -inf, stable descending sort.  -> (top_val [P, k] in the dtype
    of `scores`, top_idx [P, k] int64).  The reference of the kernel's tests, and the route of a backend without `filtered_topk` or
    of a k above TEMP_TOPK_MAX."""
    s = scores.detach()
    n = s.shape[1] if n is None else int(n)
    s = s[:, :n].clone()
    P, dev = s.shape[0], s.device
    if filt_ptr is not None and filt_ids is not None and filt_ids.numel():
        ptr, fid = filt_ptr.long(), filt_ids.long()
        rows = torch.repeat_interleave(torch.arange(P, device=dev), ptr[1:] - ptr[:-1])
        m = (fid >= col0) & (fid < col0 + n)
        if keep is not None:
            m &= fid != keep.long()[rows]
        s[rows[m], fid[m] - col0] = float("-inf")
    idx = (col0 + torch.arange(n, device=dev)).view(1, n).expand(P, n)
    if carry is not None:                                   # ids no longer ascend along the row: order by id first, then by score
        s, idx = torch.cat([carry[0].to(s.dtype), s], dim=1), torch.cat([carry[1].long(), idx], dim=1)
        idx, o = torch.sort(idx, dim=1, stable=True)
        s = s.gather(1, o)
    val, o = torch.sort(s, dim=1, descending=True, stable=True)
    idx = idx.gather(1, o).masked_fill(val == float("-inf"), -1)
    if val.shape[1] < k:
        val = torch.cat([val, val.new_full((P, k - val.shape[1]), float("-inf"))], dim=1)
        idx = torch.cat([idx, idx.new_full((P, k - idx.shape[1]), -1)], dim=1)
    return val[:, :k].contiguous(), idx[:, :k].contiguous()


def mixed_scores(a, b, w):
    """The mixed score rows of `temp_filtered_topk_mix` in plain torch: w[p] a[p, j] + (1 - w[p]) b[p, j], and -inf wherever EITHER
    operand is -inf -- masked before the arithmetic, so a weight of 0 or 1 never meets an infinity (0 * inf = NaN).  With
    topk_composite it is the route of a backend without `filtered_topk_mix` or of a k above TEMP_TOPK_MAX, and the reference of
    the kernel's tests.  -> [P, ld] in the dtype of `a`."""
    a, b = a.detach(), b.detach()
    dead = (a == float("-inf")) | (b == float("-inf"))
    wc = torch.as_tensor(w, dtype=a.dtype, device=a.device).reshape(-1, 1)
    m = wc * a.masked_fill(dead, 0.0) + (1 - wc) * b.masked_fill(dead, 0.0)
    return m.masked_fill(dead, float("-inf"))


def _select(be, k):
    """The plain selection of topk_single_graph: the backend's kernel up to TEMP_TOPK_MAX answers, else the composite."""
    return be.filtered_topk if hasattr(be, "filtered_topk") and k <= _lib.TOPK_MAX else topk_composite


def _select_mixed(be, k):
    """select(s_a, s_b, w, k, ...) over mix(w, s_a, s_b): the backend's mixed kernel, else the composite on mixed_scores."""
    if hasattr(be, "filtered_topk_mix") and k <= _lib.TOPK_MAX:
        return be.filtered_topk_mix
    return lambda s_a, s_b, w, k, *args, **kw: topk_composite(mixed_scores(s_a, s_b, w), k, *args, **kw)


def rank_stream_torch(scores, target, filt_ptr=None, filt_ids=None, mode=_lib.RANK_WHOLE, col0=0, n=None, carry=None, scores_b=None, w=None):
    """The contract of `temp_filtered_rank_stream` (scores_b, w given: of `temp_filtered_rank_stream_mix`, on w a + (1 - w) b) in
    plain torch, all four modes -> (ranks [P] int64 | None, carry), carry = (target_score [P], count [P] int32) updated in place as by
    the backend's entry points.  The other known-true entities of the panel get -10e6 before torch.sigmoid (tests/cpu_backend.py's
    filtered_rank: their value is 0 and they are still compared), columns >= n are dropped by index.  The reference of the kernel's
    tests, and the route of a backend without `filtered_rank_stream`."""
    s = scores.detach()
    n = s.shape[1] if n is None else int(n)
    s = s[:, :n]
    if scores_b is not None:
        wc = torch.as_tensor(w, dtype=s.dtype, device=s.device).reshape(-1, 1)
        s = wc * s + (1 - wc) * scores_b.detach()[:, :n]
    P, dev = s.shape[0], s.device
    tgt = target.long()
    inside = (tgt >= col0) & (tgt < col0 + n)
    if mode == _lib.RANK_COLLECT:
        if carry is None:
            carry = (torch.zeros(P, dtype=s.dtype, device=dev), torch.zeros(P, dtype=torch.int32, device=dev))
        rows = torch.nonzero(inside).reshape(-1)
        carry[0][rows] = s[rows, tgt[rows] - col0]
        return None, carry
    if mode == _lib.RANK_WHOLE:
        if not bool(inside.all()):
            raise ValueError("rank_stream_torch: TEMP_RANK_WHOLE needs every row's target inside the panel")
        raw, carry = s.gather(1, (tgt - col0).view(-1, 1)), None
    else:
        if carry is None:
            raise ValueError("rank_stream_torch: the counting modes need the carry of the TEMP_RANK_COLLECT sweep")
        raw = carry[0].view(-1, 1)
    s = s.clone()
    if filt_ptr is not None and filt_ids is not None and filt_ids.numel():
        ptr, fid = filt_ptr.long(), filt_ids.long()
        rows = torch.repeat_interleave(torch.arange(P, device=dev), ptr[1:] - ptr[:-1])
        m = (fid >= col0) & (fid < col0 + n) & (fid != tgt[rows])
        s[rows[m], fid[m] - col0] = -10e6
    # the sigmoid of every distinct score ONCE: equal scores must tie, and torch.sigmoid on the CPU rounds an element of a vector
    # body and one of a scalar tail differently in the last bit -- the target's score is not where its column is
    vals, inv = torch.unique(torch.cat([s.reshape(-1), raw.reshape(-1)]), return_inverse=True)
    sig = torch.sigmoid(vals)[inv]
    v, tv = sig[:s.numel()].view_as(s), sig[s.numel():].view(-1, 1)
    ent = col0 + torch.arange(n, device=dev).view(1, n)
    ahead = ((v > tv) | ((v == tv) & (ent < tgt.view(-1, 1)))).sum(dim=1)
    if mode == _lib.RANK_WHOLE:
        return ahead + 1, None
    if mode == _lib.RANK_COUNT_FIRST:
        carry[1].copy_(ahead)
    else:
        carry[1].add_(ahead.to(carry[1].dtype))
    return carry[1].long() + 1, carry


def _rank_plain(be):
    """rank(scores, target, ptr, ids, mode=, col0=, n=, carry=): the backend's streamed rank, else its contract in torch."""
    return be.filtered_rank_stream if hasattr(be, "filtered_rank_stream") else rank_stream_torch


def _rank_mixed(be):
    """rank(s_a, s_b, w, target, ptr, ids, mode=, col0=, n=, carry=) over mix(w, s_a, s_b): the backend's mixed kernel, else torch."""
    if hasattr(be, "filtered_rank_stream_mix"):
        return be.filtered_rank_stream_mix
    return lambda s_a, s_b, w, *args, **kw: rank_stream_torch(s_a, *args, scores_b=s_b, w=w, **kw)


def _rank_panel(panel, P, num_ent, matrices):
    """Columns per pass of the streamed rank: `panel` as the caller gave it, "auto" as _topk_panel(None, ...) sizes it."""
    return _topk_panel(None if isinstance(panel, str) and panel == "auto" else panel, P, num_ent, matrices)


def _streamed_rank(rank, produce, num_ent, panel, target, ptr, ids):
    """The filtered ranks of rows whose scores exist one column panel at a time.  produce(c0, c1) -> the leading operands of `rank`
    for the entities c0 .. c1 - 1: (scores,) or (scores_a, scores_b, w), [P, ld] with c1 - c0 <= ld.  One panel: TEMP_RANK_WHOLE.
    More: a TEMP_RANK_COLLECT sweep for the targets' scores, then a counting sweep that scores every panel AGAIN -- by the same
    calls on the same inputs, so the target's column has the bits the first sweep saw."""
    spans = [(c0, min(num_ent, c0 + panel)) for c0 in range(0, num_ent, panel)]
    if len(spans) == 1:
        return rank(*produce(0, num_ent), target, ptr, ids, mode=_lib.RANK_WHOLE, col0=0, n=num_ent)[0]
    carry = None
    for c0, c1 in spans:
        carry = rank(*produce(c0, c1), target, ptr, ids, mode=_lib.RANK_COLLECT, col0=c0, n=c1 - c0, carry=carry)[1]
    for i, (c0, c1) in enumerate(spans):
        ranks, carry = rank(*produce(c0, c1), target, ptr, ids, mode=_lib.RANK_COUNT_ADD if i else _lib.RANK_COUNT_FIRST, col0=c0, n=c1 - c0,
                            carry=carry)
    return ranks


class EvaluationFilter:
    def __init__(self, args, calc_score, graph_dict_train, graph_dict_val, graph_dict_test):
        self.args = args
        self.calc_score = calc_score
        self.graph_dicts = (graph_dict_train, graph_dict_val, graph_dict_test)
        self._keys = {}
        self._global_keys = {}

    def _true_keys(self, time, num_ent):
        """Sorted keys (h*R + r)*N + global(t) and (t*R + r)*N + global(h) over the three splits at `time`."""
        k = self._keys.get(time)
        if k is None:
            trip = [np.stack([g[time].src, g[time].rel, g[time].dst], axis=1) for g in self.graph_dicts if time in g]
            trip = np.concatenate(trip, axis=0) if trip else np.zeros((0, 3), np.int64)
            gid = next(g[time].gids for g in self.graph_dicts if time in g)
            R = int(trip[:, 1].max()) + 1 if trip.shape[0] else 1
            tails = np.unique((trip[:, 0] * R + trip[:, 1]) * num_ent + gid[trip[:, 2]])
            heads = np.unique((trip[:, 2] * R + trip[:, 1]) * num_ent + gid[trip[:, 0]])
            k = self._keys[time] = (R, tails, heads)
        return k

    def _true_keys_global(self, time, num_ent):
        """_true_keys with the known side in GLOBAL entity ids as well: sorted (global(h)*R + r)*N + global(t) and
        (global(t)*R + r)*N + global(h) -- what a query that names its entity by global id is looked up in."""
        k = self._global_keys.get(time)
        if k is None:
            trip = [np.stack([g[time].gids[g[time].src], g[time].rel, g[time].gids[g[time].dst]], axis=1).astype(np.int64)
                    for g in self.graph_dicts if time in g]
            trip = np.concatenate(trip, axis=0) if trip else np.zeros((0, 3), np.int64)
            R = int(trip[:, 1].max()) + 1 if trip.shape[0] else 1
            tails = np.unique((trip[:, 0] * R + trip[:, 1]) * num_ent + trip[:, 2])
            heads = np.unique((trip[:, 2] * R + trip[:, 1]) * num_ent + trip[:, 0])
            k = self._global_keys[time] = (R, tails, heads)
        return k

    @staticmethod
    def filter_lists(prefix, keys, num_ent):
        """CSR lists of the global entity ids that form a known-true triple with every `prefix`:
        -> (ptr [P+1] int32, ids [ptr[-1]] int32), each row's ids unique and ascending."""
        lo = np.searchsorted(keys, prefix * num_ent, side="left")
        hi = np.searchsorted(keys, (prefix + 1) * num_ent, side="left")
        cnt = hi - lo
        ptr = np.zeros(prefix.shape[0] + 1, dtype=np.int64)
        np.cumsum(cnt, out=ptr[1:])
        pos = np.repeat(lo - ptr[:-1], cnt) + np.arange(int(ptr[-1]), dtype=np.int64)
        return ptr.astype(np.int32), (keys[pos] % num_ent).astype(np.int32)

    def _mode_inputs(self, mode, samples, graph, time, num_ent, dev):
        """(target [P], filt_ptr [P+1], filt_ids) on `dev` for one corruption mode.  Cached ON the graph object (so the entry
        dies with the graph: no id() reuse) together with the sample tensor it was built from; any other `samples` -- a
        subset, a re-ordering, different triples -- rebuilds the lists."""
        cache = graph.__dict__.setdefault("_filter_lists", {})
        key = (id(self), time, mode, str(dev))
        got = cache.get(key)
        if got is not None:
            ref = got[0]
            same = ref is samples or (ref.shape == samples.shape and ref.device == samples.device and bool(torch.equal(ref, samples)))
            if not same:
                got = None
        if got is None:
            samples_np = samples.detach().cpu().numpy().astype(np.int64)
            R, tails, heads = self._true_keys(time, num_ent)
            gid = graph.gids
            if mode == "tail":
                prefix, keys, tgt = samples_np[:, 0] * R + samples_np[:, 1], tails, gid[samples_np[:, 2]]
            else:
                prefix, keys, tgt = samples_np[:, 2] * R + samples_np[:, 1], heads, gid[samples_np[:, 0]]
            ptr, ids = self.filter_lists(prefix, keys, num_ent)
            got = cache[key] = (samples.detach().clone(), torch.from_numpy(tgt.astype(np.int32)).to(dev), torch.from_numpy(ptr).to(dev),
                                torch.from_numpy(ids).to(dev))
        target, ptr, ids = got[1:]
        assert target.shape[0] == samples.shape[0] and ptr.shape[0] == samples.shape[0] + 1, "filter lists do not match the samples"
        return target, ptr, ids

    def calc_metrics_single_graph(self, ent_mean, rel_enc_means, all_ent_embeds, samples, graph, time, eval_bz=100, panel=None):
        """-> ranks (2P,) int64, subject-corruption ranks first, then object-corruption (reference order).
        panel: None scores all N entities at once and ranks with `temp_filtered_rank`.  A positive multiple of 4, or "auto" (the
        widest panel that keeps the live score matrix at or under TOPK_PANEL_BYTES), takes the streamed rank (_streamed_rank) over
        that many entities per pass: the [P, N] matrix never exists at once, at the price of scoring every panel twice when there
        is more than one."""
        with torch.no_grad():
            dev = all_ent_embeds.device
            num_ent = all_ent_embeds.shape[0]
            time = int(time)
            P = samples.shape[0]
            if P == 0:
                return torch.zeros(0, dtype=torch.int64, device=dev)
            name = getattr(self.args, "score_function", None)
            fused = name in S.BILINEAR and num_ent % 4 == 0 and all_ent_embeds.shape[1] % 4 == 0
            l1 = _l1_route(name, get_backend(), all_ent_embeds.shape[1])
            out = {}
            for mode in ("head", "tail"):
                target, ptr, ids = self._mode_inputs(mode, samples, graph, time, num_ent, dev)
                known = ent_mean[samples[:, 0] if mode == "tail" else samples[:, 2]]
                r = rel_enc_means[samples[:, 1]]
                if panel is not None:
                    be = get_backend()
                    if fused:
                        q = S.bilinear_query(name, known, r, mode).contiguous()
                        produce = lambda c0, c1: (be.linear(q, all_ent_embeds[c0:c1].contiguous(), True),)
                    elif l1:
                        q = _translation_query(known, r, mode)
                        produce = lambda c0, c1: (be.l1_scores(q, all_ent_embeds[c0:c1].contiguous()),)
                    else:
                        produce = lambda c0, c1: (self._literal_scores(known, r, all_ent_embeds[c0:c1], mode),)
                    out[mode] = _streamed_rank(_rank_plain(be), produce, num_ent, _rank_panel(panel, P, num_ent, 1), target, ptr, ids)
                    continue
                if fused:
                    q = S.bilinear_query(name, known, r, mode).contiguous()
                    score = get_backend().linear(q, all_ent_embeds.contiguous(), True)
                    out[mode] = get_backend().filtered_rank(score, target, ptr, ids)
                    continue
                if l1:                                     # one pass over all P triples, the pad columns already -inf
                    score = get_backend().l1_scores(_translation_query(known, r, mode), all_ent_embeds.contiguous())
                    out[mode] = get_backend().filtered_rank(score, target, ptr, ids)
                    continue
                ranks = []
                for a in range(0, P, eval_bz):
                    b = min(P, a + eval_bz)
                    if mode == "tail":
                        score = self.calc_score(known[a:b], r[a:b], all_ent_embeds, mode="tail")
                    else:
                        score = self.calc_score(all_ent_embeds, r[a:b], known[a:b], mode="head")
                    lo, hi = int(ptr[a]), int(ptr[b])
                    ranks.append(get_backend().filtered_rank(_pad4(score), target[a:b], ptr[a:b + 1] - lo, ids[lo:hi]))
                out[mode] = torch.cat(ranks)
            return torch.cat([out["head"], out["tail"]])

    def topk_single_graph(self, all_ent_embeds, rel_enc_means, known, rel, mode, time, k, filtered=True, keep=None, panel=None):
        """The k best answers of Q queries at `time`: (known[i], rel[i], ?) for mode "tail", (?, rel[i], known[i]) for "head".
        -> (ids [Q, k] int64 global entity ids, scores [Q, k] float32), best first: higher score, then smaller id; rows with fewer
        than k admissible entities end in (-1, -inf).

        `known` holds GLOBAL entity ids -- their rows are read from `all_ent_embeds` [N, D], which already carries the convolved rows
        of the active entities -- and `rel` rows of `rel_enc_means`.  filtered: every entity that completes a known triple with
        (known, rel) at `time` in train + valid + test is left out, except the row's `keep` id (nullable [Q], -1 = none); a known
        entity or a relation that never occurs at `time` has nothing to leave out.  The scores come from the routes of
        calc_metrics_single_graph; `panel` (a multiple of 4) scores that many entities at a time and carries the lists, None does so
        only when the whole [Q, N] matrix would pass TOPK_PANEL_BYTES."""
        with torch.no_grad():
            dev, (num_ent, d) = all_ent_embeds.device, all_ent_embeds.shape
            known, rel, ptr, ids, keep = self._topk_queries(dev, num_ent, known, rel, mode, time, filtered, keep)
            Q = known.shape[0]
            if Q == 0:
                return _topk_empty(k, dev)
            be = get_backend()
            name = getattr(self.args, "score_function", None)
            kn, r = all_ent_embeds[known], rel_enc_means[rel]
            fused = name in S.BILINEAR and num_ent % 4 == 0 and d % 4 == 0
            l1 = _l1_route(name, be, d)
            if fused:
                q = S.bilinear_query(name, kn, r, mode).contiguous()
            elif l1:
                q = _translation_query(kn, r, mode)
            panel = _topk_panel(panel, Q, num_ent, 1)
            select = _select(be, k)
            carry = None
            for c0 in range(0, num_ent, panel):
                table = all_ent_embeds[c0:min(num_ent, c0 + panel)].contiguous()
                if fused:
                    score = be.linear(q, table, True)
                elif l1:
                    score = be.l1_scores(q, table)                       # the pad columns already -inf
                else:
                    score = self._literal_scores(kn, r, table, mode)
                carry = select(score, k, ptr, ids, keep, col0=c0, n=table.shape[0], carry=carry)
            return carry[1], carry[0].float()

    def _topk_queries(self, dev, num_ent, known, rel, mode, time, filtered, keep):
        """The front half of every topk_single_graph: -> (known [Q] int64, rel [Q] int64, filt_ptr, filt_ids, keep) on `dev` -- the
        queries' GLOBAL ids, their filter lists out of _true_keys_global (None, None when not filtered) and the int32 keep ids."""
        if mode not in ("head", "tail"):
            raise ValueError("topk_single_graph: mode must be 'head' or 'tail'")
        known = torch.as_tensor(known, dtype=torch.int64, device=dev).reshape(-1)
        rel = torch.as_tensor(rel, dtype=torch.int64, device=dev).reshape(-1)
        ptr = ids = None
        if filtered and known.shape[0]:
            R, tails, heads = self._true_keys_global(int(time), num_ent)
            known_np, rel_np = known.cpu().numpy(), rel.cpu().numpy()
            prefix = np.where((rel_np >= 0) & (rel_np < R), known_np * R + rel_np, -1)      # a relation unseen at `time`: no key below 0
            ptr, ids = self.filter_lists(prefix, tails if mode == "tail" else heads, num_ent)
            ptr, ids = torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev)
        if keep is not None:
            keep = torch.as_tensor(keep, device=dev).to(torch.int32).reshape(-1)
        return known, rel, ptr, ids, keep

    def _literal_scores(self, kn, r, table, mode):
        """calc_score of every query against the rows of `table` ([n, D], or [Q, n, D]: its own candidates per query), 100 queries at
        a time, padded to whole float4s with -inf."""
        rows = []
        for a in range(0, kn.shape[0], 100):
            cand = table if table.dim() == 2 else table[a:a + 100]
            rows.append(self.calc_score(kn[a:a + 100], r[a:a + 100], cand, mode="tail") if mode == "tail"
                        else self.calc_score(cand, r[a:a + 100], kn[a:a + 100], mode="head"))
        return _pad4(torch.cat(rows))


def _topk_empty(k, dev):
    return torch.zeros(0, k, dtype=torch.int64, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev)


def _topk_panel(panel, Q, num_ent, matrices):
    """Columns scored per selection call.  `panel` as the caller gave it (a positive multiple of 4); None: all N at once while the
    `matrices` [Q, ld] score matrices alive at that moment stay at or under TOPK_PANEL_BYTES, else as many columns as do."""
    ld = (num_ent + 3) // 4 * 4
    if panel is None:
        per = 4 * Q * matrices
        panel = ld if per * ld <= TOPK_PANEL_BYTES else max(4, TOPK_PANEL_BYTES // per // 4 * 4)
    if panel <= 0 or panel % 4:
        raise ValueError("topk_single_graph: panel must be a positive multiple of 4")
    return panel


def _w_col(w, P, like):
    """Per-triple mixing weight as a (P, 1) column (the reference passes (P, 1) tensors; scalars and (P,) vectors broadcast)."""
    w = torch.as_tensor(w, dtype=like.dtype, device=like.device)
    if w.dim() == 0:
        return w.view(1, 1).expand(P, 1)
    return w.reshape(P, 1)


class _MixedRankFilter(EvaluationFilter):
    """Shared part of the two post-ensemble filters: for one corruption mode, the score matrix of the mixed (local, temporal)
    representation, then the filtered rank (the filter list replaces the reference's -10e6 overwrite, as in the base class)."""

    def _score_matrix(self, known, r, all_embeds, mode, eval_bz, padded=False):
        """[P, N] scores of the known rows against every row of all_embeds; padded: [P, N rounded up to a multiple of 4], the pad
        columns -inf (what the selection kernels take)."""
        name = getattr(self.args, "score_function", None)
        P, num_ent = known.shape[0], all_embeds.shape[0]
        if name in S.BILINEAR and num_ent % 4 == 0 and all_embeds.shape[1] % 4 == 0:
            q = S.bilinear_query(name, known, r, mode).contiguous()
            return get_backend().linear(q, all_embeds.contiguous(), True)
        if _l1_route(name, get_backend(), all_embeds.shape[1]):
            score = get_backend().l1_scores(_translation_query(known, r, mode), all_embeds.contiguous())
            return score if padded else score[:, :num_ent]
        rows = []
        for a in range(0, P, eval_bz):
            b = min(P, a + eval_bz)
            rows.append(self.calc_score(known[a:b], r[a:b], all_embeds, mode="tail") if mode == "tail"
                        else self.calc_score(all_embeds, r[a:b], known[a:b], mode="head"))
        return _pad4(torch.cat(rows)) if padded else torch.cat(rows)

    def _mixed_topk(self, known_loc, known_rec, r, all_loc, all_rec, w, mode, k, ptr, ids, keep, panel, r_rec=None):
        """The selection over mix(w, score(known_loc, all_loc), score(known_rec, all_rec)), the two score matrices from the routes
        of _score_matrix panel by panel.  Two matrices are alive at once: all N columns in one go while 2 Q ld 4 bytes stay at or
        under TOPK_PANEL_BYTES, else panels with the carry.  r_rec: the second stream's own relation rows (two models), else `r`."""
        Q, num_ent = known_loc.shape[0], all_loc.shape[0]
        panel = _topk_panel(panel, Q, num_ent, 2)
        select = _select_mixed(get_backend(), k)
        w = w.reshape(-1).contiguous()
        carry = None
        for c0 in range(0, num_ent, panel):
            c1 = min(num_ent, c0 + panel)
            s_loc = self._score_matrix(known_loc, r, all_loc[c0:c1], mode, 100, padded=True)
            s_rec = self._score_matrix(known_rec, r if r_rec is None else r_rec, all_rec[c0:c1], mode, 100, padded=True)
            carry = select(s_loc, s_rec, w, k, ptr, ids, keep, col0=c0, n=c1 - c0, carry=carry)
        return carry[1], carry[0].float()

    def _rank(self, score, mode, samples, graph, time, num_ent, dev):
        target, ptr, ids = self._mode_inputs(mode, samples, graph, time, num_ent, dev)
        return get_backend().filtered_rank(_pad4(score), target, ptr, ids)

    def _mixed_rank_streamed(self, known_loc, known_rec, r, r_rec, all_loc, all_rec, w, mode, eval_bz, panel, inputs):
        """The streamed rank over mix(w, score(known_loc, all_loc), score(known_rec, all_rec)): both panel matrices, from the routes of
        _score_matrix, and the gate go to the mixed entry (`temp_filtered_rank_stream_mix`), so the mixed matrix is never written.
        Two matrices are alive at once (what "auto" sizes the panel by)."""
        P, num_ent = known_loc.shape[0], all_loc.shape[0]
        w = w.reshape(-1).contiguous()
        produce = lambda c0, c1: (self._score_matrix(known_loc, r, all_loc[c0:c1], mode, eval_bz, padded=True),
                                  self._score_matrix(known_rec, r_rec, all_rec[c0:c1], mode, eval_bz, padded=True), w)
        return _streamed_rank(_rank_mixed(get_backend()), produce, num_ent, _rank_panel(panel, P, num_ent, 2), *inputs)


class PostEnsembleEvaluationFilter(_MixedRankFilter):
    """utils/post_evaluation.py:63-134: SCORE-level ensemble.  score = w * score(local) + (1 - w) * score(temporal), per triple
    (the reference masks each score matrix before mixing; both masked values are -10e6, so filtering after the mix is the
    same).  As in the reference, the object-corruption ranks use `weight_subject`, the subject-corruption ranks `weight_object`.
    rel_enc_temporal: the temporal stream's own relation table when the streams are two models (Aggregator,
    models/aggregator.py:259-296; the two tables may differ in width); None, the default, scores both streams with `rel_enc_mean`."""

    def calc_metrics_single_graph(self, ent_embed_local, ent_embed_temporal, rel_enc_mean, all_embeds_g_local, all_embeds_g_temporal,
                                  weight_subject, weight_object, samples, graph, time, eval_bz=100, rel_enc_temporal=None, panel=None):
        """-> ranks (2P,) int64 as the base class's.  panel: as in EvaluationFilter.calc_metrics_single_graph; the streamed route
        hands both streams' panel matrices and the weights to the mixed rank, so no mixed matrix is written."""
        with torch.no_grad():
            dev, num_ent, time, P = all_embeds_g_local.device, all_embeds_g_local.shape[0], int(time), samples.shape[0]
            if P == 0:
                return torch.zeros(0, dtype=torch.int64, device=dev)
            r = rel_enc_mean[samples[:, 1]]
            r_tmp = r if rel_enc_temporal is None else rel_enc_temporal[samples[:, 1]]
            out = {}
            for mode, w in (("head", weight_object), ("tail", weight_subject)):
                sel = samples[:, 0] if mode == "tail" else samples[:, 2]
                if panel is not None:
                    out[mode] = self._mixed_rank_streamed(ent_embed_local[sel], ent_embed_temporal[sel], r, r_tmp, all_embeds_g_local, all_embeds_g_temporal,
                                                          _w_col(w, P, all_embeds_g_local), mode, eval_bz, panel,
                                                          self._mode_inputs(mode, samples, graph, time, num_ent, dev))
                    continue
                s_loc = self._score_matrix(ent_embed_local[sel], r, all_embeds_g_local, mode, eval_bz)
                s_tmp = self._score_matrix(ent_embed_temporal[sel], r_tmp, all_embeds_g_temporal, mode, eval_bz)
                wc = _w_col(w, P, s_loc)
                out[mode] = self._rank(wc * s_loc + (1 - wc) * s_tmp, mode, samples, graph, time, num_ent, dev)
            return torch.cat([out["head"], out["tail"]])

    def topk_single_graph(self, all_loc, all_rec, rel_enc_means, known, rel, w, mode, time, k, filtered=True, keep=None, panel=None,
                          rel_enc_temporal=None):
        """EvaluationFilter.topk_single_graph for the score-level ensemble: the k best answers under
        w[i] * score(all_loc[known[i]], rel[i], all_loc[e]) + (1 - w[i]) * score(all_rec[known[i]], rel[i], all_rec[e]),
        w [Q] the queries' mixing weights.  all_loc / all_rec [N, D] are the local and the temporal all-entity table; `known` holds
        GLOBAL ids, and the filter lists, `keep`, `panel` and the returned (ids [Q, k] int64, scores [Q, k] float32) are the base
        class's.  The mix is formed inside the selection (`temp_filtered_topk_mix`): the mixed [Q, N] matrix is never written.
        rel_enc_temporal: as in calc_metrics_single_graph (the second term then uses rel_enc_temporal[rel[i]])."""
        with torch.no_grad():
            dev, num_ent = all_loc.device, all_loc.shape[0]
            known, rel, ptr, ids, keep = self._topk_queries(dev, num_ent, known, rel, mode, time, filtered, keep)
            if known.shape[0] == 0:
                return _topk_empty(k, dev)
            w = torch.as_tensor(w, dtype=torch.float32, device=dev).reshape(-1)
            if w.shape[0] != known.shape[0]:
                raise ValueError("topk_single_graph: w must have one entry per query")
            return self._mixed_topk(all_loc[known], all_rec[known], rel_enc_means[rel], all_loc, all_rec, w, mode, k, ptr, ids, keep, panel,
                                    None if rel_enc_temporal is None else rel_enc_temporal[rel])


class PostEvaluationFilter(_MixedRankFilter):
    """utils/post_evaluation.py:7-60: EMBEDDING-level ensemble with four per-triple weights.  The known entity is mixed as
    w * local + (1 - w) * temporal; every candidate likewise with the other weight.  distmult / complex are linear in the
    candidate, so the candidate mix is applied to the two score matrices instead of materialising (P, N_ents, D) candidates;
    transE is not: its scores are one dense pass that mixes the two all-entity rows per (triple, entity) in registers
    (`temp_l1_mix_scores`); any other scorer, or a backend without that kernel, takes the reference's literal route."""

    def calc_metrics_single_graph(self, ent_embed_loc, ent_embed_rec, rel_enc_means, all_embeds_g_loc, all_embeds_g_rec, samples,
                                  weight_subject_query_subject_embed, weight_subject_query_object_embed,
                                  weight_object_query_subject_embed, weight_object_query_object_embed, graph, time, eval_bz=100, panel=None):
        """-> ranks (2P,) int64 as the base class's.  panel: as in EvaluationFilter.calc_metrics_single_graph.  On the streamed route
        the bilinear scorers hand the ONE folded query's two panel matrices and the candidate gate to the mixed rank; transE scores
        each panel through `temp_l1_mix_scores` and takes the plain rank, as does the literal route over the mixed candidates."""
        with torch.no_grad():
            dev, num_ent, time, P = all_embeds_g_loc.device, all_embeds_g_loc.shape[0], int(time), samples.shape[0]
            if P == 0:
                return torch.zeros(0, dtype=torch.int64, device=dev)
            r = rel_enc_means[samples[:, 1]]
            name = getattr(self.args, "score_function", None)
            out = {}
            for mode, w_s, w_o in (("head", weight_subject_query_subject_embed, weight_subject_query_object_embed),
                                   ("tail", weight_object_query_subject_embed, weight_object_query_object_embed)):
                ws, wo = _w_col(w_s, P, ent_embed_loc), _w_col(w_o, P, ent_embed_loc)
                sel = samples[:, 0] if mode == "tail" else samples[:, 2]
                w_known, w_cand = (ws, wo) if mode == "tail" else (wo, ws)     # tail: subject known; head: object known
                known = w_known * ent_embed_loc[sel] + (1 - w_known) * ent_embed_rec[sel]
                be = get_backend()
                if panel is not None:
                    out[mode] = self._gated_rank_streamed(be, name, known, r, all_embeds_g_loc, all_embeds_g_rec, w_cand, mode, eval_bz, panel,
                                                          self._mode_inputs(mode, samples, graph, time, num_ent, dev))
                    continue
                if _l1_route(name, be, all_embeds_g_loc.shape[1]) and hasattr(be, "l1_mix_scores"):
                    # one pass over all P triples: the candidate mix formed inside the dense L1 kernel, the pad columns already -inf
                    score = be.l1_mix_scores(_translation_query(known, r, mode), all_embeds_g_loc.contiguous(), all_embeds_g_rec.contiguous(),
                                             w_cand.contiguous())
                elif name in S.BILINEAR:
                    score = w_cand * self._score_matrix(known, r, all_embeds_g_loc, mode, eval_bz) \
                        + (1 - w_cand) * self._score_matrix(known, r, all_embeds_g_rec, mode, eval_bz)
                else:
                    rows = []
                    for a in range(0, P, eval_bz):
                        b = min(P, a + eval_bz)
                        cand = w_cand[a:b].unsqueeze(-1) * all_embeds_g_loc.unsqueeze(0) + (1 - w_cand[a:b]).unsqueeze(-1) * all_embeds_g_rec.unsqueeze(0)
                        rows.append(self.calc_score(known[a:b], r[a:b], cand, mode="tail") if mode == "tail"
                                    else self.calc_score(cand, r[a:b], known[a:b], mode="head"))
                    score = torch.cat(rows)
                out[mode] = self._rank(score, mode, samples, graph, time, num_ent, dev)
            return torch.cat([out["head"], out["tail"]])

    def _gated_rank_streamed(self, be, name, known, r, all_loc, all_rec, w_cand, mode, eval_bz, panel, inputs):
        """The streamed rank of the mixed known rows against the candidates w_cand all_loc + (1 - w_cand) all_rec, panel by panel, by
        the score routes of topk_single_graph."""
        P, (num_ent, d) = known.shape[0], all_loc.shape
        if name in S.BILINEAR:
            return self._mixed_rank_streamed(known, known, r, r, all_loc, all_rec, w_cand, mode, eval_bz, panel, inputs)
        l1 = _l1_route(name, be, d) and hasattr(be, "l1_mix_scores")
        if l1:
            q, wc = _translation_query(known, r, mode), w_cand.contiguous()
            produce = lambda c0, c1: (be.l1_mix_scores(q, all_loc[c0:c1].contiguous(), all_rec[c0:c1].contiguous(), wc),)       # the pad columns -inf
        else:
            wc = w_cand.unsqueeze(-1)
            produce = lambda c0, c1: (self._literal_scores(known, r, wc * all_loc[c0:c1].unsqueeze(0) + (1 - wc) * all_rec[c0:c1].unsqueeze(0), mode),)
        # one score matrix at a time; the literal route also holds the [P, panel, D] mixed candidates
        return _streamed_rank(_rank_plain(be), produce, num_ent, _rank_panel(panel, P, num_ent, 1 if l1 else 1 + d), *inputs)

    def topk_single_graph(self, all_loc, all_rec, rel_enc_means, known, rel, w_known, w_cand, mode, time, k, filtered=True, keep=None,
                          panel=None):
        """EvaluationFilter.topk_single_graph for the embedding-level gate, as in calc_metrics_single_graph: the known row is
        w_known[i] * all_loc[known[i]] + (1 - w_known[i]) * all_rec[known[i]], candidate e is w_cand[i] * all_loc[e] +
        (1 - w_cand[i]) * all_rec[e]; w_known, w_cand [Q].  distmult / complex are linear in the candidate: the ONE folded query
        against both tables gives two score matrices and the selection mixes them in registers (`temp_filtered_topk_mix`); transE
        takes `temp_l1_mix_scores` and the plain selection; any other scorer, or a backend without that kernel, the literal
        calc_score route over the mixed candidates.  Everything else is the base class's."""
        with torch.no_grad():
            dev, (num_ent, d) = all_loc.device, all_loc.shape
            known, rel, ptr, ids, keep = self._topk_queries(dev, num_ent, known, rel, mode, time, filtered, keep)
            Q = known.shape[0]
            if Q == 0:
                return _topk_empty(k, dev)
            w_known = torch.as_tensor(w_known, dtype=torch.float32, device=dev).reshape(-1, 1)
            w_cand = torch.as_tensor(w_cand, dtype=torch.float32, device=dev).reshape(-1, 1)
            if w_known.shape[0] != Q or w_cand.shape[0] != Q:
                raise ValueError("topk_single_graph: w_known and w_cand must have one entry per query")
            kn = w_known * all_loc[known] + (1 - w_known) * all_rec[known]
            r = rel_enc_means[rel]
            name = getattr(self.args, "score_function", None)
            if name in S.BILINEAR:
                return self._mixed_topk(kn, kn, r, all_loc, all_rec, w_cand, mode, k, ptr, ids, keep, panel)
            be = get_backend()
            l1 = _l1_route(name, be, d) and hasattr(be, "l1_mix_scores")
            if l1:
                q = _translation_query(kn, r, mode)
            # one score matrix at a time; the literal route also holds the [Q, panel, D] mixed candidates
            panel = _topk_panel(panel, Q, num_ent, 1 if l1 else 1 + d)
            select = _select(be, k)
            carry = None
            for c0 in range(0, num_ent, panel):
                t_loc, t_rec = all_loc[c0:min(num_ent, c0 + panel)].contiguous(), all_rec[c0:min(num_ent, c0 + panel)].contiguous()
                if l1:
                    score = be.l1_mix_scores(q, t_loc, t_rec, w_cand.contiguous())       # the pad columns already -inf
                else:
                    score = self._literal_scores(kn, r, w_cand.unsqueeze(-1) * t_loc.unsqueeze(0) + (1 - w_cand).unsqueeze(-1) * t_rec.unsqueeze(0),
                                                 mode)
                carry = select(score, k, ptr, ids, keep, col0=c0, n=t_loc.shape[0], carry=carry)
            return carry[1], carry[0].float()


def _pad4(score):
    """Score rows padded to a multiple of 4 columns with -inf (sigmoid 0 at ids above every target: never ahead)."""
    n = score.shape[1]
    if n % 4 == 0:
        return score.contiguous()
    pad = score.new_full((score.shape[0], 4 - n % 4), float("-inf"))
    return torch.cat([score, pad], dim=1).contiguous()
