"""torch.autograd wrappers around the HIP kernels (through temp_amd.backend).

Each Function is one reference op with its hand-written backward:
  rgcn_layer      RGCNLayer.forward            models/RGCN.py:53-104
  rgcn_isolated   RGCNLayer.forward_isolated   models/RGCN.py:78-89
  gru_step        decay + single GRU step      models/RRGCN.py:79-85, models/GRU_cell.py:18-30
  gather_rows     ent_embeds[id] / history gather   models/DynamicRGCN.py:41-43,93
  linear          nn.Linear without bias (q/k/v projections)   models/SARGCN.py:16-18,32-34
  lin_step_rows   the recurrent term of RRGCNLayer.forward_isolated on gathered rows   models/RRGCN.py:152-167
  lin_step_rows2  both recurrent terms of BiRRGCNLayer.forward / forward_isolated on gathered rows   models/BiRRGCN.py:102-185
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


# The link-prediction loss (its autograd nodes, scorers and private switches) is temp_amd.link_loss; the functions callers reach
# through this module are re-exported.  _TALL_SCORES, _L1_METHODS, _L1_MIX_METHODS and _cached_l1_slots are NOT: a copy of a switch
# here would be one nobody reads.
from .link_loss import (batched_all_entity_link_prediction, batched_ensemble_link_prediction, batched_gated_link_prediction,  # noqa: E402,F401
                        batched_link_prediction, bilinear_route, candidate_cross_entropy, candidate_cross_entropy_mixed,
                        dot_ce_rows_torch, dot_gather_supported, filtered_ce_rows_torch,
                        frozen_ensemble_link_prediction, frozen_mix_ce_rows,
                        gated_link_prediction, gated_loss_inputs,
                        gated_translation_supported, l1_slots, translation_cross_entropy, translation_supported)


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


LIN_ROWS_KERNEL = True      # A/B switch: False keeps lin_step_rows on the composition of the row operators


def lin_rows_usable(d):
    """True when lin_step_rows runs rows of this width through temp_lin_rows_fwd / _bwd."""
    be = get_backend()
    return bool(LIN_ROWS_KERNEL and hasattr(be, "lin_rows_fwd") and be.lin_rows_supported(d))


def _gather_adjoint(be, src, idx, inverse, rows):
    """The adjoint of out = table[idx] on the rows `src`: the deterministic segment sum through `inverse`, else zero fill + atomic scatter."""
    if inverse is not None:
        return be.segment_sum_rows(src, inverse[0], inverse[1], rows)
    d_table = torch.zeros(rows, src.shape[1], dtype=src.dtype, device=src.device)
    be.scatter_add_rows(src, idx, d_table)
    return d_table


class _LinStepRowsFn(torch.autograd.Function):
    """The kernel route of lin_step_rows (one source) and lin_step_rows2 (two): saves out (the ReLU mask is the kernel's own out > 0)
    and every source's hdec (the left factor of its d_W).  meta = (x_rows, x_inv, lam, act, [(rows, dt, inv, has)] per source); the
    tensors that may need a gradient follow: every source's H, then every source's W.  has False: a source without history, which came
    in as a one-row zero H with rows all -1 (_absent_source) and hands no gradient to its H or W."""

    @staticmethod
    def forward(ctx, meta, x, *HW):
        be = get_backend()
        x_rows, x_inv, lam, act, srcs = meta
        ns = len(srcs)
        x = x.detach().contiguous()
        Hs = [H.detach().contiguous() for H in HW[:ns]]
        rows, dts = [s[0] for s in srcs], [s[1].detach().contiguous().view(-1) for s in srcs]
        n, d = rows[0].shape[0], x.shape[1]
        packs = be.lin_chain_pack_multi([W.detach().contiguous() for W in HW[ns:]])
        out, *hdecs = (torch.empty(n, d, dtype=torch.float32, device=x.device) for _ in range(1 + ns))
        if ns == 1:
            be.lin_rows_fwd(x, x_rows, Hs[0], rows[0], dts[0], lam, packs[0], act, out, hdecs[0])
        else:
            be.lin_rows2_fwd(x, x_rows, Hs[0], rows[0], dts[0], Hs[1], rows[1], dts[1], lam, packs[0], packs[1], act, out, *hdecs)
        ctx.save_for_backward(out, *hdecs, *packs, *dts)
        ctx.meta, ctx.n_x, ctx.n_h = meta, x.shape[0], [H.shape[0] for H in Hs]
        return out

    @staticmethod
    def backward(ctx, d_out):
        be = get_backend()
        x_rows, x_inv, lam, act, srcs = ctx.meta
        ns = len(srcs)
        out, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        hdecs, packs, dts = saved[:ns], saved[ns:2 * ns], saved[2 * ns:]
        rows = [s[0] for s in srcs]
        d_pre, *d_h = (torch.empty_like(out) for _ in range(1 + ns))
        if ns == 1:
            be.lin_rows_bwd(out, d_out.contiguous(), rows[0], dts[0], lam, packs[0], act, d_pre, d_h[0])
        else:
            be.lin_rows2_bwd(out, d_out.contiguous(), rows[0], dts[0], rows[1], dts[1], lam, packs[0], packs[1], act, d_pre, *d_h)
        need = ctx.needs_input_grad[1:]
        d_x = None
        if need[0]:
            d_x = d_pre if x_rows is None else _gather_adjoint(be, d_pre, x_rows, x_inv, ctx.n_x)
        d_H = [_gather_adjoint(be, d_h[s], rows[s], srcs[s][2], ctx.n_h[s]) if need[1 + s] and srcs[s][3] else None for s in range(ns)]
        d_W = [be.linear_tn(hdecs[s], d_pre) if need[1 + ns + s] and srcs[s][3] else None for s in range(ns)]
        return (None, d_x, *d_H, *d_W)


def lin_step_rows_torch(x, x_rows, H, h_rows, dt, lam, W, act, x_inv=None, h_inv=None):
    """lin_step_rows as the composition of the row operators, each its own autograd node (RRGCNLayer.finish_rows' order: the decay
    behind the product -- the same value up to rounding)."""
    rec = decay_rows(linear_nt(gather_rows(H, h_rows, h_inv), W), dt, lam)
    out = (gather_rows(x, x_rows, x_inv) if x_rows is not None else x) + rec
    return torch.relu(out) if act else out


def lin_step_rows(x, x_rows, H, h_rows, dt, lam, W, act, x_inv=None, h_inv=None):
    """One position of the linear recurrence on gathered rows, ONE autograd node (temp_lin_rows_fwd / _bwd):
        out[i] = act(x[x_rows[i]] + (exp(-lam dt[i]) H[h_rows[i]]) . W)         (the recurrent term 0 where h_rows[i] < 0)
    x (., d) and H (., d) float32; x_rows int32 [n] or None (row i reads x[i]); h_rows int32 [n]; dt float32 (n,) or (n, 1); W (in, out);
    act 0 none, 1 ReLU.  x_inv / h_inv = gather_inverse of the two static row lists: with them the gathers' adjoints are deterministic
    segment sums (without, atomic scatters).  A backend without the kernel (the CPU test backend), LIN_ROWS_KERNEL = False, a width it
    refuses and n = 0 take lin_step_rows_torch."""
    act = int(bool(act))
    if h_rows.shape[0] == 0 or not lin_rows_usable(x.shape[1]):
        return lin_step_rows_torch(x, x_rows, H, h_rows, dt, float(lam), W, act, x_inv, h_inv)
    return _LinStepRowsFn.apply((x_rows, x_inv, float(lam), act, [(h_rows, dt, h_inv, True)]), x, H, W)


def lin_rows2_usable(d):
    """True when lin_step_rows2 runs rows of this width through temp_lin_rows2_fwd / _bwd."""
    be = get_backend()
    return bool(LIN_ROWS_KERNEL and hasattr(be, "lin_rows2_fwd") and be.lin_rows2_supported(d))


def lin_step_rows2_torch(x, x_rows, Hf, rows_f, dt_f, Hb, rows_b, dt_b, lam, Wf, Wb, act, x_inv=None, f_inv=None, b_inv=None):
    """lin_step_rows2 as the composition of the row operators, each its own autograd node, in BiRRGCNLayer.forward's order: the decay in
    front of the product, the forward term added first.  A direction whose H is None adds nothing."""
    out = gather_rows(x, x_rows, x_inv) if x_rows is not None else x
    for H, rows, dt, W, inv in ((Hf, rows_f, dt_f, Wf, f_inv), (Hb, rows_b, dt_b, Wb, b_inv)):
        if H is not None:
            out = out + linear_nt(decay_rows(gather_rows(H, rows, inv), dt, lam), W)
    return torch.relu(out) if act else out


def _absent_source(x, n):
    """What the kernel reads for a source without history: a one-row zero H, rows all -1, zero dt -> (H, (rows, dt, inv, has))."""
    return x.new_zeros(1, x.shape[1]), (torch.full((n,), -1, dtype=torch.int32, device=x.device), x.new_zeros(n), None, False)


def lin_step_rows2(x, x_rows, Hf, rows_f, dt_f, Hb, rows_b, dt_b, lam, Wf, Wb, act, x_inv=None, f_inv=None, b_inv=None):
    """One position of the bidirectional linear recurrence on gathered rows, ONE autograd node (temp_lin_rows2_fwd / _bwd):
        out[i] = act(x[x_rows[i]] + (exp(-lam dt_f[i]) Hf[rows_f[i]]) . Wf + (exp(-lam dt_b[i]) Hb[rows_b[i]]) . Wb)
    (a direction's term 0 where its row index is negative): BiRRGCNLayer's centre position and the union pair rows of its all-entity
    pass.  x, Hf, Hb (., d) float32; x_rows int32 [n] or None (row i reads x[i]); rows_s int32 [n]; dt_s float32 (n,) or (n, 1); W_s (in,
    out); act 0 none, 1 ReLU.  x_inv / f_inv / b_inv = gather_inverse of the three static row lists: with them the gathers' adjoints
    are deterministic segment sums.  H_s None (a direction without history: windows of length 1): as if every rows_s[i] were -1; rows_s
    and dt_s are then not read.  A backend without the kernel (the CPU test backend), LIN_ROWS_KERNEL = False, a width it refuses
    and n = 0 take lin_step_rows2_torch."""
    act = int(bool(act))
    n = x_rows.shape[0] if x_rows is not None else x.shape[0]
    if n == 0 or not lin_rows2_usable(x.shape[1]):
        return lin_step_rows2_torch(x, x_rows, Hf, rows_f, dt_f, Hb, rows_b, dt_b, float(lam), Wf, Wb, act, x_inv, f_inv, b_inv)
    Hs, srcs = zip(*[(H, (rows, dt, inv, True)) if H is not None else _absent_source(x, n)
                     for H, rows, dt, inv in ((Hf, rows_f, dt_f, f_inv), (Hb, rows_b, dt_b, b_inv))])
    return _LinStepRowsFn.apply((x_rows, x_inv, float(lam), act, list(srcs)), x, *Hs, Wf, Wb)


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


class _HyperplaneRowsFn(torch.autograd.Function):
    """The (B N, D) stack of `table` projected onto the B hyperplanes with normals w_b / |w_b| (temp_hyperplane_rows_fwd); the
    backward keeps nothing but its inputs and sums d_w over the N rows in a fixed order (temp_hyperplane_rows_bwd)."""

    @staticmethod
    def forward(ctx, table, w):
        ctx.save_for_backward(table, w)
        return get_backend().hyperplane_rows_fwd(table, w)

    @staticmethod
    def backward(ctx, d_out):
        table, w = ctx.saved_tensors
        return get_backend().hyperplane_rows_bwd(table, w, d_out.contiguous())


def hyperplane_rows(table, w):
    """Rows b N + i of the result = table[i] - n_b (n_b . table[i]), n_b = w[b] / |w[b]|_2 (baselines/Hyte.py:22-26 for B time rows at
    once).  table (N, D), w (B, D) float32 on one device; both get gradients."""
    if table.dim() != 2 or w.dim() != 2 or w.shape[1] != table.shape[1] or w.shape[0] < 1:
        raise ValueError("hyperplane_rows: table (N, D) and w (B >= 1, D) expected")
    return _HyperplaneRowsFn.apply(table.contiguous(), w.contiguous())


class _PairRowsFn(torch.autograd.Function):
    """The (B N, 2 D) stack of pair rows [a | a_inv] (temp_pair_rows_fwd); the backward sums the stack's gradient over the B windows
    in ascending order and splits the halves in the same launch (temp_pair_rows_bwd)."""

    @staticmethod
    def forward(ctx, a, a_inv, B):
        ctx.B = B
        return get_backend().pair_rows_fwd(a, a_inv, B)

    @staticmethod
    def backward(ctx, d_out):
        return get_backend().pair_rows_bwd(d_out.contiguous(), ctx.B) + (None,)


def pair_rows_torch(a, a_inv, B):
    """pair_rows as the torch composition: one concatenation, B - 1 more copies out of an expanded view."""
    N, D = a.shape
    return torch.cat([a, a_inv], dim=1).unsqueeze(0).expand(B, N, 2 * D).reshape(B * N, 2 * D)


def pair_rows(a, a_inv, B):
    """Rows b N + i of the result = [a[i] | a_inv[i]] for b < B (SimplE's pair layout: an entity's -- or, with B = 1, a relation's --
    forward and inverse row side by side).  a, a_inv (N, D) float32 on one device; both get gradients.  A backend without the pass
    (the CPU test backend) takes the torch composition."""
    B = int(B)
    if a.dim() != 2 or a.shape != a_inv.shape or B < 1:
        raise ValueError("pair_rows: a and a_inv (N, D) of one shape and B >= 1 expected")
    if not hasattr(get_backend(), "pair_rows_fwd"):
        return pair_rows_torch(a, a_inv, B)
    return _PairRowsFn.apply(a.contiguous(), a_inv.contiguous(), B)


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
