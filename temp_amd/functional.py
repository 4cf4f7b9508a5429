"""torch.autograd wrappers around the HIP kernels (through temp_amd.backend).

Each Function is one reference op with its hand-written backward:
  rgcn_layer      RGCNLayer.forward            models/RGCN.py:53-104
  rgcn_isolated   RGCNLayer.forward_isolated   models/RGCN.py:78-89
  gru_step        decay + single GRU step      models/RRGCN.py:79-85, models/GRU_cell.py:18-30
  gather_rows     ent_embeds[id] / history gather   models/DynamicRGCN.py:41-43,93
  linear          nn.Linear without bias (q/k/v projections)   models/SARGCN.py:16-18,32-34
  history_attention   SARGCNLayer.attention over the active history rows   models/SARGCN.py:25-53
  split_history_attention  the same for current rows that are a sum of two table rows (post-aggregation attention models)
"""
import numpy as np
import torch

from . import _lib
from .backend import get_backend

ACTS = {None: _lib.ACT_NONE, "relu": _lib.ACT_RELU}


class _RGCNLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, loop_w, bias, dg, num_bases, act, drop, grad_premasked, dest):
        be = get_backend()
        out = be.rgcn_fwd(dg, h, None, weight, loop_w, bias, num_bases, act, drop, out=dest)
        ctx.save_for_backward(h, weight, loop_w, out)
        ctx.dg, ctx.num_bases, ctx.has_bias, ctx.drop = dg, num_bases, bias is not None, drop
        # grad_premasked: the ONLY consumer of `out` folds the activation's adjoint into the gradient it returns
        # (gather_rows(..., relu_table=True)), so the backward kernels take d_out as the pre-activation gradient
        ctx.act = _lib.ACT_NONE if grad_premasked else act
        return out

    @staticmethod
    def backward(ctx, d_out):
        h, weight, loop_w, out = ctx.saved_tensors
        d_h, d_w, d_loop, d_bias = get_backend().rgcn_bwd(ctx.dg, h, out, d_out.contiguous(), weight, loop_w, ctx.has_bias,
                                                          ctx.num_bases, ctx.act, ctx.drop)
        return d_h, d_w, d_loop, d_bias, None, None, None, None, None, None


def rgcn_layer(h, dg, weight, loop_w, bias, num_bases, act=None, drop=None, grad_premasked=False, out=None):
    """out = act(nnorm^2 * sum_in h_u BD(W_r) [+bias] + dropout(h W_loop)) on a device graph `dg`.
    drop = (p, seed) or None: dropout of the self-loop message (models/RGCN.py:57-59), mask = hash(seed, row, col).
    out: optional caller-owned contiguous (n_nodes, d_out) destination that no autograd graph knows (e.g. this rank's row range
    of the exchange buffer of temp_amd.dist): the layer writes its result there instead of allocating."""
    return _RGCNLayerFn.apply(h, weight, loop_w, bias, dg, num_bases, ACTS[act], drop, bool(grad_premasked and act == "relu"),
                              None if out is None else out.detach())


class _RGCNTableLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, weight, loop_w, bias, ids, inverse, dg, num_bases, act, drop, pv):
        be = get_backend()
        if pv is not None and be.pair_mode()[1]:
            out = be.rgcn_pair_fwd(dg, pv, table, ids, weight, loop_w, bias, num_bases, act, drop)
        else:
            out = be.rgcn_table_fwd(dg, table, ids, weight, loop_w, bias, num_bases, act, drop)
        ctx.save_for_backward(table, weight, loop_w, out, ids)
        ctx.dg, ctx.num_bases, ctx.act, ctx.has_bias, ctx.inverse, ctx.drop, ctx.pv = dg, num_bases, act, bias is not None, inverse, drop, pv
        return out

    @staticmethod
    def backward(ctx, d_out):
        table, weight, loop_w, out, ids = ctx.saved_tensors
        be = get_backend()
        if ctx.pv is not None and be.pair_mode()[2]:
            d_t, d_w, d_loop, d_bias = be.rgcn_pair_bwd(ctx.dg, ctx.pv, table, ids, ctx.inverse, out, d_out.contiguous(), weight, loop_w,
                                                        ctx.has_bias, ctx.num_bases, ctx.act, ctx.drop)
        else:
            d_t, d_w, d_loop, d_bias = be.rgcn_table_bwd(ctx.dg, table, ids, ctx.inverse, out, d_out.contiguous(), weight, loop_w,
                                                         ctx.has_bias, ctx.num_bases, ctx.act, ctx.drop)
        return d_t, d_w, d_loop, d_bias, None, None, None, None, None, None, None


def pair_view_for(dg, ids, n_table, d_in, d_out, num_bases, build=False):
    """The pair view (pair_view.DevicePairView) of device graph `dg` under the node -> table row map `ids` when a table-fed layer
    of this shape takes the pair route on it (include/temp_amd.h: TempPairView; the switch is TEMP_OPT_RGCN_PAIR), else None:
      - the backend has the route (the HIP backend; test backends without it keep the table route);
      - the kernels take the shape;
      - the graph has at least PAIR_MIN_RATIO edges per (relation row, table row) pair -- or the option forces the route.
    The view is cached on `dg` under the address of `ids`, which it keeps alive: `ids` must not be rewritten in place afterwards
    (the node -> table row map of a prepared batch is static).  It is built here only with build=True -- prepare time (RGCNLayer.prepare_table) -- or when the
    option forces the route outside a graph capture: a step never sorts edges."""
    from . import pair_view as PV
    be = get_backend()
    if not hasattr(be, "rgcn_pair_fwd") or ids is None or not ids.is_cuda:
        return None
    mode = be.pair_mode()[0]
    if mode == 0 or not be.pair_supported(d_in, d_out, num_bases):
        return None
    if mode == 1 and dg.n_edges < PV.PAIR_MIN_RATIO * dg.n_rel_rows * int(n_table):
        return None
    cache = dg.__dict__.setdefault("_pair_views", {})
    key = (ids.data_ptr(), int(ids.shape[0]), int(n_table))
    pv = cache.get(key)
    if pv is None and (build or mode == 2) and not torch.cuda.is_current_stream_capturing():
        pv = cache[key] = PV.DevicePairView(dg, ids, n_table, dg.n_rel_rows, expand=be.expand_chunk_segments)
    return pv


def rgcn_layer_table(table, ids, inverse, dg, weight, loop_w, bias, num_bases, act=None, drop=None):
    """rgcn_layer on h = table[ids] (ids int32, static; inverse = gather_inverse(ids, rows)) without materialising h:
    the self-loop product and its gradients run over the table's rows, not over every node row.  Where pair_view_for finds a
    prepared pair view the relational term runs over (relation, table row) pairs as well."""
    pv = pair_view_for(dg, ids, table.shape[0], loop_w.shape[0], loop_w.shape[1], num_bases)
    return _RGCNTableLayerFn.apply(table, weight, loop_w, bias, ids, inverse, dg, num_bases, ACTS[act], drop, pv)


class _RGCNIsolatedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, loop_w, bias, act, drop):
        out = get_backend().rgcn_isolated_fwd(e, loop_w, bias, act, drop)
        ctx.save_for_backward(e, loop_w, out)
        ctx.act, ctx.has_bias, ctx.drop = act, bias is not None, drop
        return out

    @staticmethod
    def backward(ctx, d_out):
        e, loop_w, out = ctx.saved_tensors
        d_e, d_loop, d_bias = get_backend().rgcn_isolated_bwd(e, out, d_out.contiguous(), loop_w, ctx.has_bias, ctx.act, ctx.drop)
        return d_e, d_loop, d_bias, None, None


def rgcn_isolated(e, loop_w, bias, act=None, drop=None):
    """out = act(e + dropout(e W_loop) [+bias])."""
    return _RGCNIsolatedFn.apply(e, loop_w, bias, ACTS[act], drop)


class _GRUStepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, prev, dt, w_ih, w_hh, b_ih, b_hh, decay_w, decay_b, prev_idx, lam, variant, prev_inv=None):
        be = get_backend()
        wb = None
        if decay_w is not None:
            wb = torch.cat([decay_w.detach().reshape(1), decay_b.detach().reshape(1)]).contiguous()
        dt = dt.reshape(-1).contiguous()
        h_out, saved = be.gru_fwd(x, prev, prev_idx, dt, lam, wb, w_ih, w_hh, b_ih, b_hh, variant)
        ctx.save_for_backward(x, prev, dt, w_ih, w_hh, saved, wb if wb is not None else x.new_zeros(0))
        ctx.prev_idx, ctx.lam, ctx.variant, ctx.learn = prev_idx, lam, variant, wb is not None
        ctx.prev_inv = prev_inv
        ctx.wshape = decay_w.shape if decay_w is not None else None
        ctx.bshape = decay_b.shape if decay_b is not None else None
        return h_out

    @staticmethod
    def backward(ctx, d_h):
        x, prev, dt, w_ih, w_hh, saved, wb = ctx.saved_tensors
        be = get_backend()
        d_x, d_prev_rows, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_wb = be.gru_bwd(
            x, prev, ctx.prev_idx, dt, ctx.lam, wb if ctx.learn else None, w_ih, w_hh, saved, d_h.contiguous(), ctx.variant)
        if ctx.prev_idx is None:
            d_prev = d_prev_rows
        elif ctx.prev_inv is not None:                        # injective row map: the adjoint of the gather is a gather through the
            d_prev = be.gather_rows(d_prev_rows, ctx.prev_inv)   # inverse map (-1 -> zero row): one pass, no atomics, no zero fill
        else:
            d_prev = torch.zeros_like(prev)
            be.scatter_add_rows(d_prev_rows, ctx.prev_idx, d_prev)
        d_dw = d_wb[0].reshape(ctx.wshape) if ctx.learn else None
        d_db = d_wb[1].reshape(ctx.bshape) if ctx.learn else None
        return d_x, d_prev, None, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_dw, d_db, None, None, None, None


def gru_step(x, prev, dt, w_ih, w_hh, b_ih, b_hh, lam, decay=None, prev_idx=None, type1=False, prev_inv=None):
    """h' = GRU(x, prev[prev_idx] * exp(-lam*dt))  (learnable decay when `decay` = (weight, bias)).
    prev_idx: optional int32 tensor, -1 => zero previous state.
    prev_inv: optional int32 tensor [rows of prev], the inverse of an INJECTIVE prev_idx (prev_inv[prev_idx[i]] = i, -1 for rows
    nobody continues from; injective_inverse()): the gradient of `prev` is then one gather instead of a zero fill + atomic scatter."""
    dw, db = decay if decay is not None else (None, None)
    return _GRUStepFn.apply(x, prev, dt, w_ih, w_hh, b_ih, b_hh, dw, db, prev_idx, float(lam),
                            _lib.GRU_TYPE1 if type1 else _lib.GRU_TORCH, prev_inv)


def injective_inverse(idx_np, n_rows, device):
    """int32 device tensor inv [n_rows] with inv[idx[i]] = i (-1 where no i maps) for a host index list whose non-negative
    entries are pairwise distinct, or None when they are not (the caller then keeps the scatter-add adjoint)."""
    idx = np.asarray(idx_np).reshape(-1)
    ok = idx >= 0
    inv = np.full(int(n_rows), -1, dtype=np.int32)
    inv[idx[ok]] = np.nonzero(ok)[0].astype(np.int32)
    if int((inv >= 0).sum()) != int(ok.sum()):
        return None
    return _lib.to_device(inv, device)


class _GatherRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, idx, inverse, relu_table):
        ctx.rows = table.shape[0]
        ctx.inverse = inverse
        ctx.relu_table = relu_table
        ctx.save_for_backward(idx, table.detach()) if relu_table else ctx.save_for_backward(idx)
        return get_backend().gather_rows(table, idx)

    @staticmethod
    def backward(ctx, d_out):
        idx = ctx.saved_tensors[0]
        be = get_backend()
        if ctx.relu_table:                                # (only offered with an inverse: see gather_rows)
            seg_ptr, order = ctx.inverse
            return be.segment_sum_rows(d_out.contiguous(), seg_ptr, order, ctx.rows, relu_of=ctx.saved_tensors[1]), None, None, None
        if ctx.inverse is not None and d_out.shape[1] % 4 == 0 and d_out.shape[1] <= 256:
            seg_ptr, order = ctx.inverse
            return be.segment_sum_rows(d_out.contiguous(), seg_ptr, order, ctx.rows), None, None, None
        d_table = torch.zeros(ctx.rows, d_out.shape[1], dtype=d_out.dtype, device=d_out.device)
        be.scatter_add_rows(d_out.contiguous(), idx, d_table)
        return d_table, None, None, None


class _GatherRowsKeysFn(torch.autograd.Function):
    """_GatherRowsFn that also returns the magnitude keys of its output (row keys [n], column keys [d]; int32, not differentiable):
    the f16 products that read the gathered rows scale them by these (include/temp_amd.h: temp_gather_rows_keys)."""

    @staticmethod
    def forward(ctx, table, idx, inverse, relu_table):
        ctx.rows = table.shape[0]
        ctx.inverse = inverse
        ctx.relu_table = relu_table
        ctx.save_for_backward(idx, table.detach()) if relu_table else ctx.save_for_backward(idx)
        out, rk, ck = get_backend().gather_rows_keys(table, idx)
        ctx.mark_non_differentiable(rk, ck)
        ctx.set_materialize_grads(False)                  # (else autograd zero-fills "gradients" for the two key tensors every step)
        return out, rk, ck

    @staticmethod
    def backward(ctx, d_out, _drk, _dck):
        if d_out is None:
            return None, None, None, None
        return _GatherRowsFn.backward(ctx, d_out)


def gather_keys_supported(d):
    """True when gather_rows(..., keys=True) is available and of use for width d on the installed backend."""
    be = get_backend()
    return hasattr(be, "gather_rows_keys") and be.keys_supported(d)


def relu_gather_supported(table, inverse):
    """True when gather_rows(table, ., inverse, relu_table=True) is available for this table (a tensor, or its width)."""
    d = table if isinstance(table, int) else table.shape[1]
    return inverse is not None and d % 4 == 0 and d <= 256


def gather_rows(table, idx, inverse=None, relu_table=False, keys=False):
    """out[i] = table[idx[i]] (idx int32, -1 => zero row).  Backward: atomic scatter-add, or -- when the caller
    supplies `inverse` = gather_inverse(idx, rows) for a static index list -- a deterministic segment sum.
    relu_table=True: `table` is the ReLU output of the layer before and this gather is its ONLY consumer: the backward returns
    the gradient with that ReLU's adjoint already applied (zero where table <= 0), in the same kernel; the producing layer must
    then run its own backward with grad_premasked=True (rgcn_layer)."""
    if relu_table and not relu_gather_supported(table, inverse):
        raise ValueError("relu_table needs a static inverse and a width the segment-sum kernels take")
    if keys:                                              # -> (out, (row_keys, col_keys)): see _GatherRowsKeysFn
        out, rk, ck = _GatherRowsKeysFn.apply(table, idx, inverse, bool(relu_table))
        return out, (rk, ck)
    return _GatherRowsFn.apply(table, idx, inverse, bool(relu_table))


def row_spans(y, spans):
    """Row ranges [(row0, n), ...] of `y` for several consumers.  When the ranges tile y in order they come from ONE split -- its
    adjoint is one concatenation of the consumers' gradients; separate slices each cost a zero-filled full-size gradient, a copy
    and an addition in the backward (the per-position loops hand every position its rows of one layer output)."""
    off = 0
    for r0, n in spans:
        if r0 != off:
            return [y[r0:r0 + n] for r0, n in spans]
        off += n
    if off != y.shape[0]:
        return [y[r0:r0 + n] for r0, n in spans]
    return list(y.split([n for _, n in spans]))


def gather_inverse(idx_np, n_rows, device):
    """(seg_ptr int32 [n_rows+1], order int32) grouping the positions of a gather index list by table row
    (positions of negative entries are left out): a stable counting sort in the host planner library
    (temp_host_gather_inverse), one upload."""
    from . import _hostlib
    both, _ = _hostlib.gather_inverse(idx_np, n_rows)
    dev = _lib.to_device(both, device)
    return dev[:n_rows + 1], dev[n_rows + 1:]


class _CandidateCEFn(torch.autograd.Function):
    """mean_p CE(query[p] . all_embeds[cand[p, :]]^T, label 0) without materialising (P, C, D)."""

    @staticmethod
    def forward(ctx, query, all_embeds, cand):
        be = get_backend()
        scores = be.linear(query, all_embeds, True)                  # (P, N): every positive against ALL entities
        loss_rows, lse = be.gather_ce_fwd(scores, cand)
        ctx.save_for_backward(query, all_embeds, scores, lse, cand)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, d_loss):
        query, all_embeds, scores, lse, cand = ctx.saved_tensors
        be = get_backend()
        d_scores = be.gather_ce_bwd(scores, cand, lse, d_loss.reshape(1).contiguous(), 1.0 / max(scores.shape[0], 1))
        d_query = be.linear(d_scores, all_embeds, False)             # (P,N) . (N,D)
        d_all = be.linear_tn(d_scores, query)                        # (N,P) . (P,D)
        return d_query, d_all, None


class _BatchedCandidateCEFn(torch.autograd.Function):
    """sum_b mean_{rows of window b} CE(query[p] . all_embeds_b[cand[p, :]]^T, label 0): the row-wise work (candidate CE
    forward / backward) runs once over ALL windows' rows; only the three GEMMs are per window, because every window scores
    against its own all-entity matrix."""

    @staticmethod
    def forward(ctx, query, cand, splits, row_w, *all_embeds):
        be = get_backend()
        scores = torch.cat([be.linear(query[a:b], e, True) for (a, b), e in zip(splits, all_embeds)], dim=0)    # (sum P, N)
        loss_rows, lse = be.gather_ce_fwd(scores, cand)
        ctx.save_for_backward(query, scores, lse, cand, row_w, *all_embeds)
        ctx.splits = splits
        return (loss_rows * row_w).sum()

    @staticmethod
    def backward(ctx, d_loss):
        query, scores, lse, cand, row_w = ctx.saved_tensors[:5]
        all_embeds = ctx.saved_tensors[5:]
        be = get_backend()
        d_scores = be.gather_ce_bwd(scores, cand, lse, d_loss.reshape(1).contiguous(), 1.0, row_w)
        d_query = torch.cat([be.linear(d_scores[a:b], e, False) for (a, b), e in zip(ctx.splits, all_embeds)], dim=0)
        d_all = tuple(be.linear_tn(d_scores[a:b], query[a:b]) for (a, b) in ctx.splits)
        return (d_query, None, None, None) + d_all


# Entity-major score GEMMs (see forward): 10 % less device time on ICEWS-shaped steps (3.51 -> 3.18 ms under graph replay), but
# ~30 more launches per step, which makes an eager, host-bound training loop SLOWER (5.7 -> 6.8 ms/step measured).  Off unless
# TEMP_LOSS_TALL=1.
_TALL_SCORES = __import__("os").environ.get("TEMP_LOSS_TALL", "0") == "1"


# -- the per-window products of the three batched loss nodes ------------------------------------------------------------------
# `big` is the (B * N, D) stack of the windows' all-entity matrices, `splits` the [row_begin, row_end) of every window's block of
# the stacked query rows, `live` the windows that have rows.
def _live_windows(splits):
    return [(b, a0, a1) for b, (a0, a1) in enumerate(splits) if a1 > a0]


def _window_scores(be, q, big, live, N):
    """scores = q[rows of window b] . big_b^T for every live window -> (rows, N), one multi-problem launch."""
    scores = torch.empty(q.shape[0], N, dtype=torch.float32, device=q.device)
    be.linear_multi([q[a0:a1] for _, a0, a1 in live], [big[b * N:(b + 1) * N] for b, _, _ in live], True, scores)
    return scores


def _window_dq(be, d_s, big, live, N, like):
    """d_q = d_scores_b . big_b for every live window, one launch."""
    d_q = torch.empty_like(like)
    be.linear_multi([d_s[a0:a1] for _, a0, a1 in live], [big[b * N:(b + 1) * N] for b, _, _ in live], False, d_q)
    return d_q


def _dbig_like(big, live, n_windows):
    """The gradient buffer of `big`: every live window's block is written whole, so only a batch with an empty window needs zeros."""
    return torch.empty_like(big) if len(live) == n_windows else torch.zeros_like(big)


def _window_dbig(be, d_s, q, big, live, N, n_windows):
    """d_big_b = d_scores_b^T . q_b for every live window."""
    d_big = _dbig_like(big, live, n_windows)
    if hasattr(be, "linear_tn_multi"):                                                        # one launch
        be.linear_tn_multi([d_s[a0:a1] for _, a0, a1 in live], [q[a0:a1] for _, a0, a1 in live], [d_big[b * N:(b + 1) * N] for b, _, _ in live])
    else:
        for b, a0, a1 in live:
            be.linear_tn(d_s[a0:a1], q[a0:a1], out=d_big[b * N:(b + 1) * N])
    return d_big


class _BatchedLinkPredictionFn(torch.autograd.Function):
    """The whole batched link-prediction loss as ONE autograd node:
        q      = bilinear_query(ent_rows[known], rel[rel_idx])                 (gathers fused, temp_bilinear_query_fwd)
        scores = q[rows of window b] . all_b^T   for every window b             (temp_linear_multi, 4 windows per launch)
        loss   = sum_rows w_row * CE(scores[row, cand[row, :]], label 0)        (temp_gather_ce_fwd)
    `big` is the (B * N, D) stack of the windows' all-entity matrices.  The backward mirrors it and reduces the per-row
    gradients of the gathered operands with deterministic segment sums over the static index lists."""

    @staticmethod
    def forward(ctx, ent_rows, rel, big, kind, inp):
        be = get_backend()
        N = big.shape[0] // len(inp["splits"])
        q = be.bilinear_query_fwd(kind, ent_rows, inp["known"], rel, inp["rel"], inp["is_tail"])
        live = _live_windows(inp["splits"])
        # few positives against many entities (ICEWS-like: ~200 rows x 10 000 entities per window): the ENTITY axis is made the
        # tall one of every GEMM -- scores = (all_b . q_b^T)^T through a transposed-store epilogue, and the backward products
        # from d_scores^T.  (The planner pads every window's block to a multiple of 4 rows so it can be an N / K extent.)
        tall = _TALL_SCORES and all((a1 - a0) % 4 == 0 and 8 * (a1 - a0) <= N for _, a0, a1 in live)
        if tall:
            scores = torch.empty(q.shape[0], N, dtype=torch.float32, device=q.device)
            for b, a0, a1 in live:
                be.linear_t(big[b * N:(b + 1) * N], q[a0:a1], True, scores[a0:a1])
        else:
            scores = _window_scores(be, q, big, live, N)
        loss_rows, lse = be.gather_ce_fwd(scores, inp["cand"])
        ctx.save_for_backward(ent_rows, rel, big, q, scores, lse)
        ctx.kind, ctx.inp, ctx.live, ctx.N, ctx.tall = kind, inp, live, N, tall
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        ent_rows, rel, big, q, scores, lse = ctx.saved_tensors
        inp, live, N = ctx.inp, ctx.live, ctx.N
        be = get_backend()
        d_scores = be.gather_ce_bwd(scores, inp["cand"], lse, d_loss.reshape(1).contiguous(), 1.0, inp["weights"])
        if ctx.tall:
            d_q = torch.empty_like(q)
            d_big = _dbig_like(big, live, len(inp["splits"]))
            for b, a0, a1 in live:
                dst = d_scores[a0:a1].t().contiguous()                                        # (N, rows of window b)
                be.linear_tn(dst, big[b * N:(b + 1) * N], out=d_q[a0:a1])                     # d_q   = d_scores . all_b
                d_big[b * N:(b + 1) * N].copy_(be.linear(dst, q[a0:a1], False))               # d_all = d_scores^T . q
        else:
            d_q = _window_dq(be, d_scores, big, live, N, q)
            d_big = _window_dbig(be, d_scores, q, big, live, N, len(inp["splits"]))
        dk, dr = be.bilinear_query_bwd(ctx.kind, ent_rows, inp["known"], rel, inp["rel"], inp["is_tail"], d_q)
        d_ent = be.segment_sum_rows(dk, inp["known_inv"][0], inp["known_inv"][1], ent_rows.shape[0])
        d_rel = be.segment_sum_rows(dr, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        return d_ent, d_rel, d_big, None, None


class _BatchedEnsembleLinkPredictionFn(torch.autograd.Function):
    """_BatchedLinkPredictionFn for the score-level ensemble of the post-ensemble models (combined_scores,
    models/PostDynamicRGCN.py:404-406, 425-428): TWO streams (local = pre-GRU, temporal = post-GRU) score against their own
    all-entity stacks, the scores are mixed row by row with w (local) and 1 - w (temporal) on the (rows, N) matrices, then the
    candidate cross-entropy.  Same launches per stream as the plain node (folded query, score GEMMs of all windows as
    multi-problem launches -- k-sliced where the rows are few against 10 000 entities -- one candidate CE), one mix pass."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w, kind, inp):
        be = get_backend()
        N = big_loc.shape[0] // len(inp["splits"])
        live = _live_windows(inp["splits"])
        qs, sc = [], []
        for rows, big in ((loc_rows, big_loc), (rec_rows, big_rec)):
            q = be.bilinear_query_fwd(kind, rows, inp["known"], rel, inp["rel"], inp["is_tail"])
            qs.append(q)
            sc.append(_window_scores(be, q, big, live, N))
        mixed = torch.lerp(sc[1], sc[0], w)                          # w (rows, 1): w * local + (1 - w) * temporal
        loss_rows, lse = be.gather_ce_fwd(mixed, inp["cand"])
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w, qs[0], qs[1], sc[0], sc[1], mixed, lse)
        ctx.kind, ctx.inp, ctx.live, ctx.N = kind, inp, live, N
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w, q_l, q_r, s_l, s_r, mixed, lse = ctx.saved_tensors
        inp, live, N = ctx.inp, ctx.live, ctx.N
        be = get_backend()
        d_m = be.gather_ce_bwd(mixed, inp["cand"], lse, d_loss.reshape(1).contiguous(), 1.0, inp["weights"])
        d_sl = d_m * w
        d_sr = d_m - d_sl
        d_w = (d_m * (s_l - s_r)).sum(dim=1, keepdim=True) if ctx.needs_input_grad[5] else None
        outs, d_rel = [], None
        for rows, big, q, d_s in ((loc_rows, big_loc, q_l, d_sl), (rec_rows, big_rec, q_r, d_sr)):
            d_q = _window_dq(be, d_s, big, live, N, q)
            d_big = _window_dbig(be, d_s, q, big, live, N, len(inp["splits"]))
            dk, dr = be.bilinear_query_bwd(ctx.kind, rows, inp["known"], rel, inp["rel"], inp["is_tail"], d_q)
            outs.append((be.segment_sum_rows(dk, inp["known_inv"][0], inp["known_inv"][1], rows.shape[0]), d_big))
            d_rel = dr if d_rel is None else d_rel + dr
        d_rel = be.segment_sum_rows(d_rel, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        return outs[0][0], outs[1][0], d_rel, outs[0][1], outs[1][1], d_w, None, None


def batched_ensemble_link_prediction(loc_rows, rec_rows, rel, big_loc, big_rec, w, kind, inputs):
    """sum over windows of the ensemble CE_tail + CE_head; `w` (rows, 1) = weight of the LOCAL stream of every stacked query row
    (per window: [tail rows: weight_object ; head rows: weight_subject]); `inputs` = TKG_Module.loss_inputs(...)."""
    w = w.reshape(-1, 1).to(loc_rows.dtype).contiguous()
    if kind == "transE":
        return _BatchedEnsembleTranslationLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(),
                                                                 big_rec.contiguous(), w, inputs)
    return _BatchedEnsembleLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(), big_rec.contiguous(),
                                                  w, kind, inputs)


def _gated_query_fwd(be, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail):
    if hasattr(be, "gated_query_fwd"):
        return be.gated_query_fwd(kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail)
    # backends without the gated kernels (the CPU test backend): the mix in torch, the fold through bilinear_query
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


class _BatchedGatedLinkPredictionFn(torch.autograd.Function):
    """The embedding-level gated loss of the post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN.train_link_prediction,
    models/PostDynamicRGCN.py:261-282) over ALL windows as one autograd node:
        q      = fold(w_known * loc_rows[known_a] + (1 - w_known) * rec_rows[known], rel)      (temp_gated_query_fwd; known_a < 0:
                                                                                             the temporal row alone -- the head rows)
        s_a/b  = q[rows of window b] . big_loc_b^T / big_rec_b^T                             (temp_linear_multi, same q for both)
        loss   = sum_rows w_row * CE(w_cand * s_a + (1 - w_cand) * s_b at cand, label 0)     (temp_gather_ce_mix_fwd)
    The candidate mix is linear in the candidate, so it lives on the two score matrices; the backward is one mixed-CE pass (both
    score gradients and d_w_cand), two d_q products, two d_big products, one gated-query pass and three deterministic segment sums."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, kind, inp):
        be = get_backend()
        N = big_loc.shape[0] // len(inp["splits"])
        live = _live_windows(inp["splits"])
        q = _gated_query_fwd(be, kind, loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"], inp["is_tail"])
        sc = [_window_scores(be, q, big, live, N) for big in (big_loc, big_rec)]
        loss_rows, lse = _gather_ce_mix_fwd(be, sc[0], sc[1], w_cand, inp["cand"])
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q, sc[0], sc[1], lse)
        ctx.kind, ctx.inp, ctx.live, ctx.N = kind, inp, live, N
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q, s_a, s_b, lse = ctx.saved_tensors
        inp, live, N = ctx.inp, ctx.live, ctx.N
        be = get_backend()
        d_sa, d_sb, d_wc = _gather_ce_mix_bwd(be, s_a, s_b, w_cand, inp["cand"], lse, d_loss.reshape(1).contiguous(), 1.0, inp["weights"])
        d_q = _window_dq(be, d_sa, big_loc, live, N, q)
        d_q2 = _window_dq(be, d_sb, big_rec, live, N, q)
        d_q += d_q2
        d_bigs = [_window_dbig(be, d_s, q, big, live, N, len(inp["splits"])) for big, d_s in ((big_loc, d_sa), (big_rec, d_sb))]
        da, db, dr, d_wk = _gated_query_bwd(be, ctx.kind, loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"],
                                            inp["is_tail"], d_q)
        d_loc = be.segment_sum_rows(da, inp["known_a_inv"][0], inp["known_a_inv"][1], loc_rows.shape[0])
        d_rec = be.segment_sum_rows(db, inp["known_inv"][0], inp["known_inv"][1], rec_rows.shape[0])
        d_rel = be.segment_sum_rows(dr, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        return (d_loc, d_rec, d_rel, d_bigs[0], d_bigs[1], d_wk.reshape(w_known.shape) if ctx.needs_input_grad[5] else None,
                d_wc.reshape(w_cand.shape) if ctx.needs_input_grad[6] else None, None, None)


def gated_loss_inputs(inp, n_loc_rows, device):
    """The loss inputs of TKG_Module.loss_inputs (head rows NOT scored as tails) completed for the gated node: known_a = the row of
    the LOCAL stream every query row mixes in -- the known subject's for tail rows, -1 (temporal only) for head rows, whose known
    object is the temporal row alone in the reference (models/PostDynamicRGCN.py:276-277) -- and its segment-sum inverse."""
    if inp is None:
        return None
    out = dict(inp)
    ka = torch.where(inp["is_tail"] != 0, inp["known"], torch.full_like(inp["known"], -1)).contiguous()
    out["known_a"] = ka
    out["known_a_inv"] = gather_inverse(ka.cpu().numpy(), n_loc_rows, device)
    return out


def batched_gated_link_prediction(loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, kind, inputs):
    """sum over windows of the post-aggregation CE_tail + CE_head (see _BatchedGatedLinkPredictionFn).  w_known / w_cand (rows, 1):
    per window [tail rows: w_oqs / w_oqo ; head rows: w_sqo / w_sqs]; `inputs` = gated_loss_inputs(TKG_Module.loss_inputs(...)).
    big_loc / big_rec: the (B * N_ents, D) stacks of the windows' all-entity matrices.  kind 'distmult' | 'complex': the score-matrix
    node; 'transE': the L1 node over the mixed candidate rows (_BatchedGatedTranslationLinkPredictionFn)."""
    f = lambda t: t.reshape(-1, 1).to(loc_rows.dtype).contiguous()
    if kind == "transE":
        return _BatchedGatedTranslationLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(),
                                                              big_rec.contiguous(), f(w_known), f(w_cand), inputs)
    return _BatchedGatedLinkPredictionFn.apply(loc_rows.contiguous(), rec_rows.contiguous(), rel, big_loc.contiguous(), big_rec.contiguous(),
                                               f(w_known), f(w_cand), kind, inputs)


def gated_link_prediction(loc, rec, rel, all_loc, all_rec, triplets, neg_tail, neg_head, w_sqs, w_sqo, w_oqs, w_oqo, kind):
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
    return batched_gated_link_prediction(loc, rec, rel, all_loc, all_rec, w_known, w_cand, kind, inp)


# -- TransE: the candidate loss over L1 distances ------------------------------------------------------------------------------
_L1_METHODS = ("l1_ce_fwd", "l1_ce_bwd_q", "l1_ce_bwd_table", "l1_scores")


def translation_supported(be=None):
    """True when the installed backend has the L1 (TransE) kernels; a backend without them keeps the tensor path."""
    be = get_backend() if be is None else be
    return all(hasattr(be, m) for m in _L1_METHODS)


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
        g, d_q = be.l1_ce_bwd_q(q, all_embeds, None, cand, s, lse, d_loss.reshape(1).contiguous(), 1.0 / max(q.shape[0], 1))
        slot_ptr, slot = l1_slots(cand, None, all_embeds.shape[0])
        return d_q, be.l1_ce_bwd_table(q, all_embeds, slot_ptr, slot, g), None


def translation_cross_entropy(q, all_embeds, cand):
    """F.cross_entropy(transE score of the translation query q = s + r (tail) / o - r (head) against all_embeds[cand], 0)
    (utils/scores.py:46-55).  cand: int32 (P, C), column 0 is the true entity."""
    return _TranslationCEFn.apply(q.contiguous(), all_embeds.contiguous(), cand)


class _BatchedTranslationLinkPredictionFn(torch.autograd.Function):
    """_BatchedLinkPredictionFn for TransE, one autograd node:
        q    = ent_rows[known] +- rel[rel_idx]                                         (temp_bilinear_query_fwd, kind transE)
        s    = -|q[row] - big[window(row) * N + cand[row, :]]|_1  for ALL windows' rows    (temp_l1_ce_fwd, one launch)
        loss = sum_rows w_row * CE(s[row, :], label 0)
    The backward: the softmax gradient and d_q (temp_l1_ce_bwd_q), the candidate side into d_big over the slot lists
    (temp_l1_ce_bwd_table), the query adjoint and the deterministic segment sums over the static index lists."""

    @staticmethod
    def forward(ctx, ent_rows, rel, big, inp):
        be = get_backend()
        N = big.shape[0] // len(inp["splits"])
        q = be.bilinear_query_fwd("transE", ent_rows, inp["known"], rel, inp["rel"], inp["is_tail"])
        base = inp["window"] * N
        s, loss_rows, lse = be.l1_ce_fwd(q, big, base, inp["cand"])
        ctx.save_for_backward(ent_rows, rel, big, q, s, lse, base)
        ctx.inp = inp
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        ent_rows, rel, big, q, s, lse, base = ctx.saved_tensors
        inp = ctx.inp
        be = get_backend()
        g, d_q = be.l1_ce_bwd_q(q, big, base, inp["cand"], s, lse, d_loss.reshape(1).contiguous(), 1.0, inp["weights"])
        slot_ptr, slot = _cached_l1_slots(inp, inp["cand"], base, big.shape[0])
        d_big = be.l1_ce_bwd_table(q, big, slot_ptr, slot, g)
        dk, dr = be.bilinear_query_bwd("transE", ent_rows, inp["known"], rel, inp["rel"], inp["is_tail"], d_q)
        d_ent = be.segment_sum_rows(dk, inp["known_inv"][0], inp["known_inv"][1], ent_rows.shape[0])
        d_rel = be.segment_sum_rows(dr, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        return d_ent, d_rel, d_big, None


_L1_MIX_METHODS = ("l1_mix_ce_fwd", "l1_mix_ce_bwd_q", "l1_mix_ce_bwd_table", "l1_mix_scores")


def gated_translation_supported(be=None):
    """True when the installed backend has the gated L1 (post-aggregation TransE) kernels; without them the tensor path stays."""
    be = get_backend() if be is None else be
    return all(hasattr(be, m) for m in _L1_MIX_METHODS)


class _BatchedGatedTranslationLinkPredictionFn(torch.autograd.Function):
    """_BatchedGatedLinkPredictionFn for TransE, one autograd node over ALL windows' rows:
        q    = (w_known * loc_rows[known_a] + (1 - w_known) * rec_rows[known]) +- rel[rel_idx]     (temp_gated_query_fwd, kind transE;
                                                                                                  known_a < 0: the temporal row alone)
        e    = w_cand[row] * big_loc[window(row) * N + cand[row, :]] + (1 - w_cand[row]) * big_rec[...]   (formed in registers)
        s    = -|q[row] - e|_1,   loss = sum_rows w_row * CE(s[row, :], label 0)                    (temp_l1_mix_ce_fwd, one launch)
    |q - e|_1 is not linear in the candidate, so unlike the bilinear node the mix cannot live on two score matrices: the kernels read
    both all-entity rows of every candidate.  The backward: the softmax gradient, d_q and d_w_cand (temp_l1_mix_ce_bwd_q), both
    tables' adjoints in one pass over the slot lists (temp_l1_mix_ce_bwd_table), one gated-query pass and three segment sums."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, inp):
        be = get_backend()
        N = big_loc.shape[0] // len(inp["splits"])
        q = _gated_query_fwd(be, "transE", loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"], inp["is_tail"])
        base = inp["window"] * N
        s, loss_rows, lse = be.l1_mix_ce_fwd(q, big_loc, big_rec, w_cand, base, inp["cand"])
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q, s, lse, base)
        ctx.inp = inp
        return (loss_rows * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w_known, w_cand, q, s, lse, base = ctx.saved_tensors
        inp = ctx.inp
        be = get_backend()
        g, d_q, d_wc = be.l1_mix_ce_bwd_q(q, big_loc, big_rec, w_cand, base, inp["cand"], s, lse, d_loss.reshape(1).contiguous(), 1.0,
                                          inp["weights"])
        slot_ptr, slot = _cached_l1_slots(inp, inp["cand"], base, big_loc.shape[0])
        d_big_loc, d_big_rec = be.l1_mix_ce_bwd_table(q, big_loc, big_rec, w_cand, slot_ptr, slot, g)
        da, db, dr, d_wk = _gated_query_bwd(be, "transE", loc_rows, inp["known_a"], rec_rows, inp["known"], w_known, rel, inp["rel"],
                                            inp["is_tail"], d_q)
        d_loc = be.segment_sum_rows(da, inp["known_a_inv"][0], inp["known_a_inv"][1], loc_rows.shape[0])
        d_rec = be.segment_sum_rows(db, inp["known_inv"][0], inp["known_inv"][1], rec_rows.shape[0])
        d_rel = be.segment_sum_rows(dr, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        return (d_loc, d_rec, d_rel, d_big_loc, d_big_rec, d_wk.reshape(w_known.shape) if ctx.needs_input_grad[5] else None,
                d_wc.reshape(w_cand.shape) if ctx.needs_input_grad[6] else None, None)


class _BatchedEnsembleTranslationLinkPredictionFn(torch.autograd.Function):
    """_BatchedEnsembleLinkPredictionFn for TransE (the score-level ensemble of the post-ensemble models): each stream scores its own
    translation query against its own all-entity stack at the candidates (temp_l1_ce_fwd; its lse and loss are not used), the
    mixed score m = w s_loc + (1 - w) s_rec and its logsumexp are (rows, C) torch passes.  The backward hands the kernels the MIXED
    softmax: temp_l1_ce_bwd_q with s = m, lse = lse_m and row_scale = weights * w (resp. weights * (1 - w)) gives each stream's
    score gradient and d_q, temp_l1_ce_bwd_table its table adjoint; d_w = sum_k G_k (s_loc - s_rec) with G the unsplit gradient."""

    @staticmethod
    def forward(ctx, loc_rows, rec_rows, rel, big_loc, big_rec, w, inp):
        be = get_backend()
        N = big_loc.shape[0] // len(inp["splits"])
        base = inp["window"] * N
        qs, sc = [], []
        for rows, big in ((loc_rows, big_loc), (rec_rows, big_rec)):
            q = be.bilinear_query_fwd("transE", rows, inp["known"], rel, inp["rel"], inp["is_tail"])
            qs.append(q)
            sc.append(be.l1_ce_fwd(q, big, base, inp["cand"])[0])
        mixed = torch.lerp(sc[1], sc[0], w)                          # w (rows, 1): w * local + (1 - w) * temporal
        lse = torch.logsumexp(mixed, dim=1)
        ctx.save_for_backward(loc_rows, rec_rows, rel, big_loc, big_rec, w, qs[0], qs[1], sc[0], sc[1], mixed, lse, base)
        ctx.inp = inp
        return ((lse - mixed[:, 0]) * inp["weights"]).sum()

    @staticmethod
    def backward(ctx, d_loss):
        loc_rows, rec_rows, rel, big_loc, big_rec, w, q_l, q_r, s_l, s_r, mixed, lse, base = ctx.saved_tensors
        inp = ctx.inp
        be = get_backend()
        scale = d_loss.reshape(1).contiguous()
        wv = w.reshape(-1)
        slot_ptr, slot = _cached_l1_slots(inp, inp["cand"], base, big_loc.shape[0])
        outs, d_rel, gs = [], None, []
        for rows, big, q, rs in ((loc_rows, big_loc, q_l, inp["weights"] * wv), (rec_rows, big_rec, q_r, inp["weights"] * (1 - wv))):
            g, d_q = be.l1_ce_bwd_q(q, big, base, inp["cand"], mixed, lse, scale, 1.0, rs.contiguous())
            gs.append(g)
            d_big = be.l1_ce_bwd_table(q, big, slot_ptr, slot, g)
            dk, dr = be.bilinear_query_bwd("transE", rows, inp["known"], rel, inp["rel"], inp["is_tail"], d_q)
            outs.append((be.segment_sum_rows(dk, inp["known_inv"][0], inp["known_inv"][1], rows.shape[0]), d_big))
            d_rel = dr if d_rel is None else d_rel + dr
        d_rel = be.segment_sum_rows(d_rel, inp["rel_inv"][0], inp["rel_inv"][1], rel.shape[0])
        d_w = None
        if ctx.needs_input_grad[5]:
            d_w = ((gs[0] + gs[1]) * (s_l - s_r)).sum(dim=1, keepdim=True)           # g_loc + g_rec = the unsplit mixed-score gradient
        return outs[0][0], outs[1][0], d_rel, outs[0][1], outs[1][1], d_w, None


def batched_link_prediction(ent_rows, rel, big, kind, inputs):
    """sum over windows of CE_tail + CE_head (models/DynamicRGCN.py:186-193) for scorer `kind` ('distmult' | 'complex': the GEMM
    node; 'transE': the L1 node); `inputs` = TKG_Module.loss_inputs(...)."""
    if kind == "transE":
        return _BatchedTranslationLinkPredictionFn.apply(ent_rows, rel, big, inputs)
    return _BatchedLinkPredictionFn.apply(ent_rows, rel, big, kind, inputs)


def candidate_cross_entropy_batched(query, cand, splits, row_w, all_embeds):
    """query (R, D), cand (R, C) int32, splits = [(row_begin, row_end)] per window, row_w (R,) = weight of every row's loss
    (1 / P_b for a mean per window and direction), all_embeds = list of (N, D) per window."""
    return _BatchedCandidateCEFn.apply(query, cand, splits, row_w, *all_embeds)


class _MixedCandidateCEFn(torch.autograd.Function):
    """mean_p CE( w_p * (q_loc[p] . A_loc[cand[p, :]]^T) + (1 - w_p) * (q_rec[p] . A_rec[cand[p, :]]^T), label 0 ): the score-level
    ensemble of the post-ensemble models (combined_scores, models/PostDynamicRGCN.py:404-406, 425-428) without the
    (P, 1 + neg, D) gathers: both streams score against ALL entities (two small GEMMs), the mix is one pass over the (P, N) score
    matrices, the candidate CE reads the mixed matrix."""

    @staticmethod
    def forward(ctx, q_loc, all_loc, q_rec, all_rec, w, cand):
        be = get_backend()
        s_loc = be.linear(q_loc, all_loc, True)                      # (P, N)
        s_rec = be.linear(q_rec, all_rec, True)
        mixed = torch.lerp(s_rec, s_loc, w)                          # w (P, 1): w * loc + (1 - w) * rec
        loss_rows, lse = be.gather_ce_fwd(mixed, cand)
        ctx.save_for_backward(q_loc, all_loc, q_rec, all_rec, w, cand, s_loc, s_rec, mixed, lse)
        return loss_rows.mean()

    @staticmethod
    def backward(ctx, d_loss):
        q_loc, all_loc, q_rec, all_rec, w, cand, s_loc, s_rec, mixed, lse = ctx.saved_tensors
        be = get_backend()
        d_mixed = be.gather_ce_bwd(mixed, cand, lse, d_loss.reshape(1).contiguous(), 1.0 / max(mixed.shape[0], 1))
        d_loc = d_mixed * w
        d_rec = d_mixed - d_loc
        d_w = (d_mixed * (s_loc - s_rec)).sum(dim=1, keepdim=True) if ctx.needs_input_grad[4] else None
        return (be.linear(d_loc, all_loc, False), be.linear_tn(d_loc, q_loc), be.linear(d_rec, all_rec, False), be.linear_tn(d_rec, q_rec),
                d_w, None)


def candidate_cross_entropy_mixed(q_loc, all_loc, q_rec, all_rec, w, cand):
    """Score-level ensemble CE (see _MixedCandidateCEFn).  w: (P, 1) mixing weight of the local stream; cand: int32 (P, C), column
    0 is the true entity."""
    return _MixedCandidateCEFn.apply(q_loc.contiguous(), all_loc.contiguous(), q_rec.contiguous(), all_rec.contiguous(),
                                     w.reshape(-1, 1).to(q_loc.dtype).contiguous(), cand)


def candidate_cross_entropy(query, all_embeds, cand):
    """F.cross_entropy(score(query, all_embeds[cand]), 0) for scorers that are bilinear in
    (query, candidate) -- DistMult and ComplEx (utils/scores.py:4-44).  cand: int32 (P, C), column 0
    is the true entity."""
    return _CandidateCEFn.apply(query, all_embeds, cand)


class _LinearFn(torch.autograd.Function):
    """y = x . W^T (W stored (out, in) like nn.Linear.weight) through the MFMA panel GEMM."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return get_backend().linear(x, w, True)

    @staticmethod
    def backward(ctx, d_y):
        x, w = ctx.saved_tensors
        be = get_backend()
        d_y = d_y.contiguous()
        d_x = be.linear(d_y, w, False) if ctx.needs_input_grad[0] else None
        d_w = be.linear_tn(d_y, x) if ctx.needs_input_grad[1] else None
        return d_x, d_w


def linear(x, w):
    return _LinearFn.apply(x, w)


class _LinearNTFn(torch.autograd.Function):
    """y = x . W with W stored (in, out) -- the `time_weight` matrices of the linear-recurrence layers."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return get_backend().linear(x, w, False)

    @staticmethod
    def backward(ctx, d_y):
        x, w = ctx.saved_tensors
        be = get_backend()
        d_y = d_y.contiguous()
        d_x = be.linear(d_y, w, True) if ctx.needs_input_grad[0] else None
        d_w = be.linear_tn(x, d_y) if ctx.needs_input_grad[1] else None
        return d_x, d_w


def linear_nt(x, w):
    return _LinearNTFn.apply(x.contiguous(), w)


class _DecayRowsFn(torch.autograd.Function):
    """x[r, :] * exp(-dt[r] * lam) (temp_decay_rows); the row scale is its own adjoint."""

    @staticmethod
    def forward(ctx, x, dt, lam):
        ctx.save_for_backward(dt)
        ctx.lam = lam
        return get_backend().decay_rows(x.contiguous(), dt.contiguous().view(-1), lam)

    @staticmethod
    def backward(ctx, d_y):
        (dt,) = ctx.saved_tensors
        return get_backend().decay_rows(d_y.contiguous(), dt.contiguous().view(-1), ctx.lam), None, None


def decay_rows(x, dt, lam):
    return _DecayRowsFn.apply(x, dt, float(lam))


class _DiachronicRowsFn(torch.autograd.Function):
    """The (B N, D) stack of diachronic entity tables ent * [1 | sin(t_b w + b)] (temp_diachronic_rows_fwd); the backward recomputes
    the sines from the parameters and reduces the stack's gradient over b in the same launch (temp_diachronic_rows_bwd)."""

    @staticmethod
    def forward(ctx, ent, w, b, t):
        ctx.save_for_backward(ent, w, b, t)
        return get_backend().diachronic_rows_fwd(ent, w, b, t)

    @staticmethod
    def backward(ctx, d_out):
        ent, w, b, t = ctx.saved_tensors
        return get_backend().diachronic_rows_bwd(ent, w, b, t, d_out.contiguous()) + (None,)


def diachronic_rows(ent, w, b, t):
    """Rows b N + j of the result = DE(t[b])[j] = ent[j] * [1 (first D // 2 columns) | sin(t[b] * w[j] + b[j])]
    (baselines/DiachronicEmbedding.py:22-28, the argument rounded twice as torch rounds it).  ent (N, D), w / b (N, D - D // 2),
    t float32 (B,) on the parameters' device; t gets no gradient."""
    if t.dtype != torch.float32 or t.dim() != 1:
        raise ValueError("diachronic_rows: t must be a float32 vector (B,)")
    return _DiachronicRowsFn.apply(ent.contiguous(), w.contiguous(), b.contiguous(), t.contiguous())


class _HistoryAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, kv_hist, idx, decay, inverse):
        out, score, lse = get_backend().sa_attn_fwd(qkv, kv_hist, idx, decay)
        ctx.save_for_backward(qkv, kv_hist, idx, decay if decay is not None else qkv.new_zeros(0), out, score, lse)
        ctx.has_decay = decay is not None
        ctx.inverse = inverse
        return out

    @staticmethod
    def backward(ctx, d_out):
        qkv, kv_hist, idx, decay, out, score, lse = ctx.saved_tensors
        d_qkv, d_hist, d_decay = get_backend().sa_attn_bwd(qkv, kv_hist, idx, decay if ctx.has_decay else None, out, score, lse,
                                                           d_out.contiguous(), ctx.inverse)
        return d_qkv, d_hist, None, d_decay, None


def history_attention(qkv, kv_hist, idx, decay=None, inverse=None):
    """8-head attention of every query row over its active history rows + itself.
    qkv (n,3D) = [q | k | v] projections of the query rows' current states; kv_hist (R,2D) = [k | v]
    projections of the history table; idx (n,T-1) int32 rows of the table, -1 => masked;
    decay (T,) additive score bias (already negated / clamped) or None;
    inverse = attention_inverse(idx, R): static maps that make the backward deterministic (no atomics).
    Returns (n,D) in the reference's feature order (d * 8 + head)."""
    return _HistoryAttentionFn.apply(qkv, kv_hist, idx, decay, inverse)


class _SplitHistoryAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pa, pb, kv_hist, ia, ib, idx, decay, inverse, inv_a, inv_b):
        out, score, lse = get_backend().sa_attn_split_fwd(pa, ia, pb, ib, kv_hist, idx, decay)
        ctx.save_for_backward(pa, pb, kv_hist, ia, ib, idx, decay if decay is not None else pa.new_zeros(0), out, score, lse)
        ctx.has_decay = decay is not None
        ctx.inverse, ctx.inv_a, ctx.inv_b = inverse, inv_a, inv_b
        return out

    @staticmethod
    def backward(ctx, d_out):
        pa, pb, kv_hist, ia, ib, idx, decay, out, score, lse = ctx.saved_tensors
        be = get_backend()
        d_qkv, d_hist, d_decay = be.sa_attn_split_bwd(pa, ia, pb, ib, kv_hist, idx, decay if ctx.has_decay else None, out, score, lse,
                                                      d_out.contiguous(), ctx.inverse)
        # d_pa[r] = sum of d_qkv over the rows with ia == r (d_pb alike): the rows are summed as their three D-wide thirds
        # (split_row_inverse), which keeps the common widths on the segment-sum kernels' piece / two-stage routes
        D = d_qkv.shape[1] // 3
        thirds = d_qkv.view(-1, D)
        d_pa = be.segment_sum_rows(thirds, ctx.inv_a[0], ctx.inv_a[1], 3 * pa.shape[0]).view(pa.shape[0], 3 * D)
        d_pb = be.segment_sum_rows(thirds, ctx.inv_b[0], ctx.inv_b[1], 3 * pb.shape[0]).view(pb.shape[0], 3 * D)
        return d_pa, d_pb, d_hist, None, None, None, d_decay, None, None, None


def split_history_attention(pa, ia, pb, ib, kv_hist, idx, decay=None, inverse=None, inv_a=None, inv_b=None):
    """history_attention for current rows that are sums of two rows: row i attends with (q | k | v) = pa[ia[i]] + pb[ib[i]]
    (pa (Na,3D), pb (Nb,3D): the projections of two small tables; ia / ib (n,) int32), formed inside the kernel -- the (n,3D)
    buffer of the summed rows is never written and the projection runs over Na + Nb rows instead of n.
    inv_a / inv_b = split_row_inverse(ia, Na) / (ib, Nb): the static maps of the deterministic sums into d_pa / d_pb (required)."""
    if inv_a is None or inv_b is None:
        raise ValueError("split_history_attention needs inv_a / inv_b (split_row_inverse of ia / ib)")
    return _SplitHistoryAttentionFn.apply(pa, pb, kv_hist, ia, ib, idx, decay, inverse, inv_a, inv_b)


def split_row_inverse(idx_np, n_rows, device):
    """gather_inverse of a split-attention row list over the THIRDS of its rows: third c of query row i belongs to segment
    3 * idx[i] + c of the (3 * n_rows, D) view of the (n_rows, 3D) table gradient."""
    idx = np.asarray(idx_np, dtype=np.int64).reshape(-1, 1)
    return gather_inverse((3 * idx + np.arange(3, dtype=np.int64)[None, :]).reshape(-1), 3 * int(n_rows), device)


def attention_inverse(idx_np, n_table, device):
    """(inv_ptr int32 [n_table+1], inv_ref int32): the (query row, position) pairs of idx (n, T-1) grouped by the table
    row they point at; ref = i * (T-1) + t.  Same stable counting sort as gather_inverse, over the flattened index matrix."""
    import numpy as np
    return gather_inverse(np.asarray(idx_np).reshape(-1), n_table, device)
