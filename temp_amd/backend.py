"""Kernel backend: the only place that crosses the C ABI (include/temp_amd.h).

`HipBackend` hands raw device pointers of torch tensors (+ the current HIP stream) to
libtemp_amd.so.  PyTorch is used for device memory and streams only.  There is no CPU
implementation in the product: tensors that are not on a GPU, or a missing library, raise.
(tests/ install a test-only backend through `set_backend` to exercise host logic without a GPU.)
"""
import ctypes

import torch

from . import _lib

_backend = None


def set_backend(b):
    """Install a backend object (tests only).  Passing None restores the HIP backend."""
    global _backend
    _backend = b


def get_backend():
    global _backend
    if _backend is None:
        _backend = HipBackend()
    return _backend


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _f32(t, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.TempAmdError("%s must live on the GPU (got %s): temp_amd has no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise _lib.TempAmdError("%s must be float32, got %s" % (name, t.dtype))
    return t.detach().contiguous()


def _i32(t, name):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int32:
        raise _lib.TempAmdError("%s must be an int32 GPU tensor" % name)
    return t.contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # the handle without building a Stream object (13 us -> 0.3 us;
_cur_device = getattr(torch._C, "_cuda_getDevice", None)                 # a step makes ~15 launches through here, prepare as many)


def _stream():
    """The calling thread's current HIP stream (torch's per-thread current stream) as a C handle."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _drop(drop):
    """(p, seed) or None -> ctypes TempDropout by reference (NULL for no dropout)."""
    if drop is None or drop[0] <= 0.0:
        return None
    d = _lib.TempDropout()
    d.p, d.seed = float(drop[0]), int(drop[1]) & 0xFFFFFFFFFFFFFFFF
    return ctypes.byref(d)


class HipBackend:
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()

    def _ws(self, nbytes, device):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

    # ---- RGCN layer ----------------------------------------------------------------------------
    def rgcn_fwd(self, dg, h, h_ids, weight, loop_w, bias, num_bases, act, drop=None, out=None):
        """out: optional contiguous (n_nodes, d_out) fp32 destination (e.g. a row range of a larger matrix)."""
        h, weight, loop_w, bias = _f32(h, "h"), _f32(weight, "weight"), _f32(loop_w, "loop_weight"), _f32(bias, "bias")
        h_ids = _i32(h_ids, "h_ids")
        d_in, d_out = loop_w.shape
        if out is None:
            out = torch.empty(dg.n_nodes, d_out, dtype=torch.float32, device=h.device)
        elif out.shape != (dg.n_nodes, d_out) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != h.device:
            raise _lib.TempAmdError("rgcn_fwd: `out` must be a contiguous fp32 (n_nodes, d_out) matrix on the layer's device")
        nb = self.lib.temp_rgcn_fwd_workspace(dg.ref(), d_out)
        ws = self._ws(nb, h.device)
        rc = self.lib.temp_rgcn_fwd(dg.ref(), _ptr(h), _ptr(h_ids), d_in, d_out, num_bases, weight.shape[0], _ptr(weight),
                                    _ptr(loop_w), _ptr(bias), act, _ptr(out), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_fwd")
        return out

    def rgcn_bwd(self, dg, h, out, d_out_grad, weight, loop_w, has_bias, num_bases, act, drop=None):
        h, out, g = _f32(h, "h"), _f32(out, "out"), _f32(d_out_grad, "d_out")
        weight, loop_w = _f32(weight, "weight"), _f32(loop_w, "loop_weight")
        d_in, d_out = loop_w.shape
        dev = h.device
        d_h = torch.empty(dg.n_nodes, d_in, dtype=torch.float32, device=dev)
        d_w = torch.empty_like(weight)
        d_loop = torch.empty_like(loop_w)
        d_bias = torch.empty(d_out, dtype=torch.float32, device=dev) if has_bias else None
        nb = self.lib.temp_rgcn_bwd_workspace(dg.ref(), d_in, d_out, num_bases, weight.shape[0])
        ws = self._ws(nb, dev)
        rc = self.lib.temp_rgcn_bwd(dg.ref(), _ptr(h), _ptr(out), _ptr(g), d_in, d_out, num_bases, weight.shape[0], _ptr(weight),
                                    _ptr(loop_w), int(has_bias), act, _ptr(d_h), _ptr(d_w), _ptr(d_loop), _ptr(d_bias), _ptr(ws),
                                    ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_bwd")
        return d_h, d_w, d_loop, d_bias

    def rgcn_bwd_dh(self, dg, out, d_out_grad, weight, loop_w, num_bases, act, drop=None, dz_out=None, dzm_out=None):
        """d_h of a layer only (include/temp_amd.h: temp_rgcn_bwd_dh); dz_out / dzm_out receive the masked gradients the weight
        pass (rgcn_bwd_weights) reads, where the activation / the dropout make them differ from d_out_grad."""
        g = _f32(d_out_grad, "d_out")
        weight, loop_w = _f32(weight, "weight"), _f32(loop_w, "loop_weight")
        d_in, d_out = loop_w.shape
        dev = g.device
        d_h = torch.empty(dg.n_nodes, d_in, dtype=torch.float32, device=dev)
        ws = self._ws(self.lib.temp_rgcn_bwd_workspace(dg.ref(), d_in, d_out, num_bases, weight.shape[0]), dev)
        rc = self.lib.temp_rgcn_bwd_dh(dg.ref(), _ptr(out), _ptr(g), d_in, d_out, num_bases, weight.shape[0], _ptr(weight), _ptr(loop_w), act,
                                       _ptr(d_h), _ptr(dz_out), _ptr(dzm_out), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_bwd_dh")
        return d_h

    def rgcn_bwd_weights(self, dg, h, dz, dzm, weight_like, loop_like, has_bias, num_bases):
        """(d_weight, d_loop_w, d_bias) of a layer from its input rows and the masked output gradients over ANY graph the rows
        belong to -- the union of all positions of a recurrence (include/temp_amd.h: temp_rgcn_bwd_weights)."""
        h, dz = _f32(h, "h"), _f32(dz, "dz")
        d_in, d_out = loop_like.shape
        dev = h.device
        d_w, d_loop = torch.empty_like(weight_like), torch.empty_like(loop_like)
        d_bias = torch.empty(d_out, dtype=torch.float32, device=dev) if has_bias else None
        ws = self._ws(self.lib.temp_rgcn_bwd_workspace(dg.ref(), d_in, d_out, num_bases, weight_like.shape[0]), dev)
        rc = self.lib.temp_rgcn_bwd_weights(dg.ref(), _ptr(h), _ptr(dz), _ptr(dzm), d_in, d_out, num_bases, weight_like.shape[0], int(has_bias),
                                            _ptr(d_w), _ptr(d_loop), _ptr(d_bias), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_rgcn_bwd_weights")
        return d_w, d_loop, d_bias

    def rgcn_table_fwd(self, dg, table, ids, weight, loop_w, bias, num_bases, act, drop=None):
        """Layer on h = table[ids] without materialising h (include/temp_amd.h: temp_rgcn_table_fwd)."""
        table, weight, loop_w, bias = _f32(table, "table"), _f32(weight, "weight"), _f32(loop_w, "loop_weight"), _f32(bias, "bias")
        ids = _i32(ids, "ids")
        d_in, d_out = loop_w.shape
        out = torch.empty(dg.n_nodes, d_out, dtype=torch.float32, device=table.device)
        ws = self._ws(self.lib.temp_rgcn_table_fwd_workspace(dg.ref(), table.shape[0], d_out), table.device)
        rc = self.lib.temp_rgcn_table_fwd(dg.ref(), _ptr(table), _ptr(ids), table.shape[0], d_in, d_out, num_bases, weight.shape[0],
                                          _ptr(weight), _ptr(loop_w), _ptr(bias), act, _ptr(out), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_table_fwd")
        return out

    def rgcn_table_bwd(self, dg, table, ids, inverse, out, d_out_grad, weight, loop_w, has_bias, num_bases, act, drop=None):
        """-> (d_table [n_table, d_in] fully written, d_weight, d_loop_w, d_bias)."""
        table, out, g = _f32(table, "table"), _f32(out, "out"), _f32(d_out_grad, "d_out")
        weight, loop_w = _f32(weight, "weight"), _f32(loop_w, "loop_weight")
        ids, inv_ptr, inv_order = _i32(ids, "ids"), _i32(inverse[0], "inv_ptr"), _i32(inverse[1], "inv_order")
        d_in, d_out = loop_w.shape
        dev = table.device
        d_table = torch.empty_like(table)
        d_w = torch.empty_like(weight)
        d_loop = torch.empty_like(loop_w)
        d_bias = torch.empty(d_out, dtype=torch.float32, device=dev) if has_bias else None
        ws = self._ws(self.lib.temp_rgcn_table_bwd_workspace(dg.ref(), table.shape[0], d_in, d_out, num_bases), dev)
        rc = self.lib.temp_rgcn_table_bwd(dg.ref(), _ptr(table), _ptr(ids), _ptr(inv_ptr), _ptr(inv_order), table.shape[0], _ptr(out), _ptr(g),
                                          d_in, d_out, num_bases, weight.shape[0], _ptr(weight), _ptr(loop_w), int(has_bias), act,
                                          _ptr(d_table), _ptr(d_w), _ptr(d_loop), _ptr(d_bias), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_table_bwd")
        return d_table, d_w, d_loop, d_bias

    # ---- pair route of the table-fed layer (include/temp_amd.h: TempPairView) -------------------------------------------------
    def pair_mode(self):
        """TEMP_OPT_RGCN_PAIR: (0 never / 1 where it pays / 2 wherever supported, forward allowed, backward allowed)."""
        o = self.lib.temp_get_option(_lib.OPT_RGCN_PAIR)
        return o & 3, not (o & 4), not (o & 8)

    def pair_supported(self, d_in, d_out, num_bases):
        return bool(self.lib.temp_rgcn_pair_supported(int(d_in), int(d_out), int(num_bases)))

    def expand_chunk_segments(self, chunk_seg, chunk_beg, chunk_end, n_pos):
        seg_of = torch.empty(n_pos, dtype=torch.int32, device=chunk_seg.device)
        rc = self.lib.temp_expand_chunk_segments(int(chunk_seg.shape[0]), _ptr(_i32(chunk_seg, "chunk_seg")), _ptr(_i32(chunk_beg, "chunk_beg")),
                                                 _ptr(_i32(chunk_end, "chunk_end")), int(n_pos), _ptr(seg_of), _stream())
        _lib.check(rc, "temp_expand_chunk_segments")
        return seg_of

    def rgcn_pair_fwd(self, dg, pv, table, ids, weight, loop_w, bias, num_bases, act, drop=None):
        """rgcn_table_fwd through the pair view `pv` of (dg, ids) (include/temp_amd.h: temp_rgcn_pair_fwd)."""
        table, weight, loop_w, bias = _f32(table, "table"), _f32(weight, "weight"), _f32(loop_w, "loop_weight"), _f32(bias, "bias")
        ids = _i32(ids, "ids")
        d_in, d_out = loop_w.shape
        out = torch.empty(dg.n_nodes, d_out, dtype=torch.float32, device=table.device)
        ws = self._ws(self.lib.temp_rgcn_pair_fwd_workspace(dg.ref(), pv.ref(), d_out), table.device)
        rc = self.lib.temp_rgcn_pair_fwd(dg.ref(), pv.ref(), _ptr(table), _ptr(ids), table.shape[0], d_in, d_out, num_bases, weight.shape[0],
                                         _ptr(weight), _ptr(loop_w), _ptr(bias), act, _ptr(out), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_pair_fwd")
        return out

    def rgcn_pair_bwd(self, dg, pv, table, ids, inverse, out, d_out_grad, weight, loop_w, has_bias, num_bases, act, drop=None):
        """rgcn_table_bwd through the pair view -> (d_table, d_weight, d_loop_w, d_bias)."""
        table, out, g = _f32(table, "table"), _f32(out, "out"), _f32(d_out_grad, "d_out")
        weight, loop_w = _f32(weight, "weight"), _f32(loop_w, "loop_weight")
        ids, inv_ptr, inv_order = _i32(ids, "ids"), _i32(inverse[0], "inv_ptr"), _i32(inverse[1], "inv_order")
        d_in, d_out = loop_w.shape
        dev = table.device
        d_table = torch.empty_like(table)
        d_w = torch.empty_like(weight)
        d_loop = torch.empty_like(loop_w)
        d_bias = torch.empty(d_out, dtype=torch.float32, device=dev) if has_bias else None
        ws = self._ws(self.lib.temp_rgcn_pair_bwd_workspace(dg.ref(), pv.ref(), d_in, d_out, num_bases), dev)
        rc = self.lib.temp_rgcn_pair_bwd(dg.ref(), pv.ref(), _ptr(table), _ptr(ids), _ptr(inv_ptr), _ptr(inv_order), table.shape[0], _ptr(out), _ptr(g),
                                         d_in, d_out, num_bases, weight.shape[0], _ptr(weight), _ptr(loop_w), int(has_bias), act,
                                         _ptr(d_table), _ptr(d_w), _ptr(d_loop), _ptr(d_bias), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_pair_bwd")
        return d_table, d_w, d_loop, d_bias

    def rgcn_isolated_fwd(self, e, loop_w, bias, act, drop=None):
        e, loop_w, bias = _f32(e, "e"), _f32(loop_w, "loop_weight"), _f32(bias, "bias")
        out = torch.empty_like(e)
        rc = self.lib.temp_rgcn_isolated_fwd(e.shape[0], e.shape[1], _ptr(e), _ptr(loop_w), _ptr(bias), act, _ptr(out), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_isolated_fwd")
        return out

    def rgcn_isolated_bwd(self, e, out, d_out_grad, loop_w, has_bias, act, drop=None):
        e, out, g, loop_w = _f32(e, "e"), _f32(out, "out"), _f32(d_out_grad, "d_out"), _f32(loop_w, "loop_weight")
        n, d = e.shape
        d_e = torch.empty_like(e)
        d_loop = torch.empty_like(loop_w)
        d_bias = torch.empty(d, dtype=torch.float32, device=e.device) if has_bias else None
        ws = self._ws(self.lib.temp_rgcn_isolated_bwd_workspace(n, d), e.device)
        rc = self.lib.temp_rgcn_isolated_bwd(n, d, _ptr(e), _ptr(out), _ptr(g), _ptr(loop_w), int(has_bias), act, _ptr(d_e),
                                             _ptr(d_loop), _ptr(d_bias), _ptr(ws), ws.numel(), _drop(drop), _stream())
        _lib.check(rc, "temp_rgcn_isolated_bwd")
        return d_e, d_loop, d_bias

    # ---- decay + GRU step ------------------------------------------------------------------------
    def gru_fwd(self, x, prev, prev_idx, dt, lam, decay_wb, w_ih, w_hh, b_ih, b_hh, variant):
        x, prev, dt = _f32(x, "x"), _f32(prev, "prev"), _f32(dt, "dt")
        w_ih, w_hh, b_ih, b_hh = _f32(w_ih, "w_ih"), _f32(w_hh, "w_hh"), _f32(b_ih, "b_ih"), _f32(b_hh, "b_hh")
        decay_wb, prev_idx = _f32(decay_wb, "decay_wb"), _i32(prev_idx, "prev_idx")
        n, d = x.shape
        h_out = torch.empty_like(x)
        saved = torch.empty(5, n, d, dtype=torch.float32, device=x.device)
        rc = self.lib.temp_gru_fwd(n, d, variant, _ptr(x), _ptr(prev), _ptr(prev_idx), _ptr(dt), float(lam), _ptr(decay_wb),
                                   _ptr(w_ih), _ptr(w_hh), _ptr(b_ih), _ptr(b_hh), _ptr(h_out), _ptr(saved), _stream())
        _lib.check(rc, "temp_gru_fwd")
        return h_out, saved

    def gru_bwd(self, x, prev, prev_idx, dt, lam, decay_wb, w_ih, w_hh, saved, d_h, variant):
        x, prev, dt, d_h = _f32(x, "x"), _f32(prev, "prev"), _f32(dt, "dt"), _f32(d_h, "d_h")
        w_ih, w_hh, saved = _f32(w_ih, "w_ih"), _f32(w_hh, "w_hh"), _f32(saved, "saved")
        decay_wb, prev_idx = _f32(decay_wb, "decay_wb"), _i32(prev_idx, "prev_idx")
        n, d = x.shape
        dev = x.device
        d_x = torch.empty_like(x)
        d_prev = torch.empty_like(x)
        d_w_ih, d_w_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
        d_b_ih = torch.empty(w_ih.shape[0], dtype=torch.float32, device=dev)
        d_b_hh = torch.empty(w_hh.shape[0], dtype=torch.float32, device=dev)
        d_wb = torch.empty(2, dtype=torch.float32, device=dev) if decay_wb is not None else None
        ws = self._ws(self.lib.temp_gru_bwd_workspace(n, d, variant), dev)
        rc = self.lib.temp_gru_bwd(n, d, variant, _ptr(x), _ptr(prev), _ptr(prev_idx), _ptr(dt), float(lam), _ptr(decay_wb),
                                   _ptr(w_ih), _ptr(w_hh), _ptr(saved), _ptr(d_h), _ptr(d_x), _ptr(d_prev), _ptr(d_w_ih),
                                   _ptr(d_w_hh), _ptr(d_b_ih), _ptr(d_b_hh), _ptr(d_wb), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_gru_bwd")
        return d_x, d_prev, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_wb

    # ---- window-batched recurrence (hoisted input gates, per-position cell, batched weight grads) ---
    def gru_input_gates(self, x, w_ih, b_ih, variant, out):
        x, w_ih, b_ih = _f32(x, "x"), _f32(w_ih, "w_ih"), _f32(b_ih, "b_ih")
        assert out.is_contiguous() and out.shape == (x.shape[0], w_ih.shape[0])
        rc = self.lib.temp_gru_input_gates(x.shape[0], x.shape[1], variant, _ptr(x), _ptr(w_ih), _ptr(b_ih), _ptr(out), _stream())
        _lib.check(rc, "temp_gru_input_gates")

    def gru_input_gates_multi(self, xs, w_ihs, b_ihs, variant, outs, x_idx=None, x_keys=None):
        """gi_i = x_i . W_ih_i^T + b_ih_i for every (row block, weight set) pair in one launch per four problems
        (include/temp_amd.h: temp_gru_input_gates_multi); x_idx: per problem an int32 table of the x rows to take (the out
        block has one row per entry; temp_gru_input_gates_gather_multi)."""
        k = len(xs)
        xs = [_f32(x, "x") for x in xs]
        w_ihs, b_ihs = [_f32(w, "w_ih") for w in w_ihs], [_f32(b, "b_ih") for b in b_ihs]
        d = xs[0].shape[1]
        idx = [None] * k if x_idx is None else [None if t is None else _i32(t, "x_idx") for t in x_idx]
        rows = [x.shape[0] if t is None else t.shape[0] for x, t in zip(xs, idx)]
        for x, w, o, n in zip(xs, w_ihs, outs, rows):
            assert x.shape[1] == d and o.is_contiguous() and o.shape == (n, w.shape[0]) and w.shape == w_ihs[0].shape
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        ns = (ctypes.c_int * k)(*rows)
        if x_idx is None and x_keys is None:
            rc = self.lib.temp_gru_input_gates_multi(k, ns, d, variant, arr(xs), arr(w_ihs), arr(b_ihs), arr(outs), _stream())
            _lib.check(rc, "temp_gru_input_gates_multi")
            return
        ia = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in idx])
        if x_keys is not None:                           # row keys of every xs[i] by SOURCE row (int32 [x_i rows]): f16 arithmetic
            for x, t in zip(xs, x_keys):
                assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == x.shape[0]
            ka = (ctypes.c_void_p * k)(*[t.data_ptr() for t in x_keys])
            rc = self.lib.temp_gru_input_gates_gather_multi_keys(k, ns, d, variant, arr(xs), ia if x_idx is not None else None, ka, arr(w_ihs),
                                                                 arr(b_ihs), arr(outs), _stream())
            _lib.check(rc, "temp_gru_input_gates_gather_multi_keys")
            return
        rc = self.lib.temp_gru_input_gates_gather_multi(k, ns, d, variant, arr(xs), ia, arr(w_ihs), arr(b_ihs), arr(outs), _stream())
        _lib.check(rc, "temp_gru_input_gates_gather_multi")

    def gru_cell_fwd(self, gi, prev, prev_idx, dt, lam, w_hh, b_hh, variant, h_out, saved_all, row0):
        """h_out (n,d) and rows [row0, row0+n) of every plane of saved_all (5, N, d) are written."""
        n, d = h_out.shape
        plane = saved_all.shape[1] * d
        sp = ctypes.c_void_p(saved_all.data_ptr() + 4 * row0 * d)
        rc = self.lib.temp_gru_cell_fwd(n, d, variant, _ptr(gi), _ptr(_f32(prev, "prev")), _ptr(_i32(prev_idx, "prev_idx")),
                                        _ptr(_f32(dt, "dt")), float(lam), _ptr(_f32(w_hh, "w_hh")), _ptr(_f32(b_hh, "b_hh")),
                                        _ptr(h_out), sp, plane, _stream())
        _lib.check(rc, "temp_gru_cell_fwd")

    def gru_cell_bwd(self, saved_all, row0, n, dh_up, d_prev_next, next_idx, dt, lam, w_hh, variant, dgi, dgh, decv, d_prev):
        d = saved_all.shape[2]
        plane = saved_all.shape[1] * d
        sp = ctypes.c_void_p(saved_all.data_ptr() + 4 * row0 * d)
        rc = self.lib.temp_gru_cell_bwd(n, d, variant, sp, plane, _ptr(dh_up), _ptr(d_prev_next), _ptr(_i32(next_idx, "next_idx")),
                                        _ptr(_f32(dt, "dt")), float(lam), _ptr(_f32(w_hh, "w_hh")), _ptr(dgi), _ptr(dgh), _ptr(decv),
                                        _ptr(d_prev), _stream())
        _lib.check(rc, "temp_gru_cell_bwd")

    def gru_cell_fwd_multi(self, cells, lam, variant, saved_all):
        """cells: list (<= 4) of dicts(gi, prev, prev_idx, dt, w_hh, b_hh, h_out, row0) -- one launch for all."""
        d = saved_all.shape[2]
        arr = (_lib.TempGruCellFwd * len(cells))()
        keep = []
        for a, c in zip(arr, cells):
            prev, pidx, dt = _f32(c["prev"], "prev"), _i32(c["prev_idx"], "prev_idx"), _f32(c["dt"], "dt")
            w_hh, b_hh = _f32(c["w_hh"], "w_hh"), _f32(c["b_hh"], "b_hh")
            keep += [prev, pidx, dt, w_hh, b_hh]
            a.n = c["h_out"].shape[0]
            a.gi, a.prev = c["gi"].data_ptr(), (prev.data_ptr() if prev is not None else None)      # prev None: zero-state cell
            a.prev_idx, a.dt = (pidx.data_ptr() if pidx is not None else None), dt.data_ptr()
            a.w_hh, a.b_hh, a.h_out = w_hh.data_ptr(), b_hh.data_ptr(), c["h_out"].data_ptr()
            a.saved = saved_all.data_ptr() + 4 * c["row0"] * d
        rc = self.lib.temp_gru_cell_fwd_multi(len(cells), arr, d, variant, float(lam), saved_all.shape[1] * d, _stream())
        _lib.check(rc, "temp_gru_cell_fwd_multi")

    def gru_cell_bwd_multi(self, cells, lam, variant, saved_all):
        """cells: list (<= 4) of dicts(row0, n, dh_up, d_prev_next, next_idx, dt, w_hh, dgi, dgh, decv, d_prev)."""
        d = saved_all.shape[2]
        arr = (_lib.TempGruCellBwd * len(cells))()
        keep = []
        opt = lambda t: t.data_ptr() if t is not None else None
        for a, c in zip(arr, cells):
            dt, w_hh, nidx = _f32(c["dt"], "dt"), _f32(c["w_hh"], "w_hh"), _i32(c["next_idx"], "next_idx")
            keep += [dt, w_hh, nidx]
            a.n = c["n"]
            a.saved = saved_all.data_ptr() + 4 * c["row0"] * d
            a.dh_up, a.d_prev_next, a.next_idx = opt(c["dh_up"]), opt(c["d_prev_next"]), opt(nidx)
            a.dt, a.w_hh = dt.data_ptr(), w_hh.data_ptr()
            a.dgi, a.dgh, a.decv, a.d_prev = c["dgi"].data_ptr(), c["dgh"].data_ptr(), c["decv"].data_ptr(), c["d_prev"].data_ptr()
            a.no_prev = 1 if c.get("no_prev") else 0
        rc = self.lib.temp_gru_cell_bwd_multi(len(cells), arr, d, variant, float(lam), saved_all.shape[1] * d, _stream())
        _lib.check(rc, "temp_gru_cell_bwd_multi")

    def subsample_views(self, jobs):
        """jobs: list of dicts(n_nodes, n_edges, keep, seed, parent, child, eid, offs {name: [3] | int}, n_chunks [3], keep_mask,
        scratch) -- see include/temp_amd.h: temp_subsample_views."""
        arr = (_lib.TempSubsampleJob * len(jobs))()
        for a, j in zip(arr, jobs):
            a.n_nodes, a.n_edges, a.keep, a.seed = j["n_nodes"], j["n_edges"], j["keep"], int(j["seed"]) & 0xFFFFFFFFFFFFFFFF
            a.parent, a.child = _i32(j["parent"], "parent").data_ptr(), _i32(j["child"], "child").data_ptr()
            a.eid = _i32(j["eid"], "eid").data_ptr() if j["n_edges"] else None
            for fld in ("off_a", "off_b", "off_chunk_beg", "off_chunk_end", "off_chunk_seg", "n_chunks"):
                for v in range(3):
                    getattr(a, fld)[v] = int(j[fld][v])
            a.off_in_deg, a.off_out_deg, a.off_nnorm = int(j["off_in_deg"]), int(j["off_out_deg"]), int(j["off_nnorm"])
            a.keep_mask = j["keep_mask"].data_ptr() if j.get("keep_mask") is not None else None
            a.scratch = j["scratch"].data_ptr()
        _lib.check(self.lib.temp_subsample_views(len(jobs), arr, _stream()), "temp_subsample_views")

    def decay_rows(self, x, dt, lam):
        x, dt = _f32(x, "x"), _f32(dt, "dt")
        out = torch.empty_like(x)
        _lib.check(self.lib.temp_decay_rows(x.shape[0], x.shape[1], _ptr(x), _ptr(dt), float(lam), _ptr(out), _stream()), "temp_decay_rows")
        return out

    # ---- the diachronic entity table (include/temp_amd.h: temp_diachronic_rows_fwd / _bwd) --------
    def diachronic_rows_fwd(self, ent, w, b, t):
        """-> (B N, d) stack of ent * [1 | sin(t_b w + b)] for the B device-resident times `t` (one launch)."""
        ent, w, b, t = _f32(ent, "ent"), _f32(w, "w"), _f32(b, "b"), _f32(t, "t")
        N, d = ent.shape
        if tuple(w.shape) != (N, d - d // 2) or w.shape != b.shape or t.dim() != 1:
            raise _lib.TempAmdError("diachronic_rows: ent (N, d), w / b (N, d - d // 2), t (B,) expected")
        out = torch.empty(t.shape[0] * N, d, dtype=torch.float32, device=ent.device)
        _lib.check(self.lib.temp_diachronic_rows_fwd(t.shape[0], N, d, _ptr(ent), _ptr(w), _ptr(b), _ptr(t), _ptr(out), _stream()),
                   "temp_diachronic_rows_fwd")
        return out

    def diachronic_rows_bwd(self, ent, w, b, t, d_out):
        """-> (d_ent, d_w, d_b), each overwritten whole by one launch (no zero-fill, no atomics)."""
        ent, w, b, t, d_out = _f32(ent, "ent"), _f32(w, "w"), _f32(b, "b"), _f32(t, "t"), _f32(d_out, "d_out")
        N, d = ent.shape
        if tuple(d_out.shape) != (t.shape[0] * N, d):
            raise _lib.TempAmdError("diachronic_rows_bwd: d_out must be (B N, d)")
        d_ent, d_w, d_b = torch.empty_like(ent), torch.empty_like(w), torch.empty_like(b)
        _lib.check(self.lib.temp_diachronic_rows_bwd(t.shape[0], N, d, _ptr(ent), _ptr(w), _ptr(b), _ptr(t), _ptr(d_out), _ptr(d_ent), _ptr(d_w),
                                                     _ptr(d_b), _stream()), "temp_diachronic_rows_bwd")
        return d_ent, d_w, d_b

    # ---- the hyperplane projection of a table (include/temp_amd.h: temp_hyperplane_rows_fwd / _bwd) --------
    def hyperplane_rows_fwd(self, table, w):
        """-> (B N, d) stack of table - n_b (n_b . table), n_b = w_b / |w_b|, for the B rows of `w` (one launch)."""
        table, w = _f32(table, "table"), _f32(w, "w")
        if table.dim() != 2 or w.dim() != 2 or w.shape[1] != table.shape[1]:
            raise _lib.TempAmdError("hyperplane_rows: table (N, d) and w (B, d) expected")
        N, d = table.shape
        out = torch.empty(w.shape[0] * N, d, dtype=torch.float32, device=table.device)
        _lib.check(self.lib.temp_hyperplane_rows_fwd(w.shape[0], N, d, _ptr(table), _ptr(w), _ptr(out), _stream()), "temp_hyperplane_rows_fwd")
        return out

    def hyperplane_rows_bwd(self, table, w, d_out):
        """-> (d_table, d_w), each overwritten whole (two launches, no atomics; the tile partials go through the backend's workspace)."""
        table, w, d_out = _f32(table, "table"), _f32(w, "w"), _f32(d_out, "d_out")
        N, d = table.shape
        B = w.shape[0]
        if tuple(d_out.shape) != (B * N, d):
            raise _lib.TempAmdError("hyperplane_rows_bwd: d_out must be (B N, d)")
        d_table, d_w = torch.empty_like(table), torch.empty_like(w)
        nb = self.lib.temp_hyperplane_rows_bwd_workspace(B, N, d)
        ws = self._ws(nb, table.device)
        _lib.check(self.lib.temp_hyperplane_rows_bwd(B, N, d, _ptr(table), _ptr(w), _ptr(d_out), _ptr(d_table), _ptr(d_w), _ptr(ws), nb, _stream()),
                   "temp_hyperplane_rows_bwd")
        return d_table, d_w

    # ---- the pair table of two tables (include/temp_amd.h: temp_pair_rows_fwd / _bwd) ----------------------
    def pair_rows_fwd(self, a, a_inv, B):
        """-> (B N, 2 d) stack of [a | a_inv], the same table for each of the B windows (one launch)."""
        a, a_inv = _f32(a, "a"), _f32(a_inv, "a_inv")
        if a.dim() != 2 or a.shape != a_inv.shape or int(B) < 1:
            raise _lib.TempAmdError("pair_rows: a and a_inv (N, d) of one shape and B >= 1 expected")
        N, d = a.shape
        out = torch.empty(int(B) * N, 2 * d, dtype=torch.float32, device=a.device)
        _lib.check(self.lib.temp_pair_rows_fwd(int(B), N, d, _ptr(a), _ptr(a_inv), _ptr(out), _stream()), "temp_pair_rows_fwd")
        return out

    def pair_rows_bwd(self, d_out, B):
        """-> (d_a, d_a_inv): the two halves of d_out (B N, 2 d) summed over the B windows in ascending order, each overwritten whole
        (one launch, no atomics, no workspace)."""
        d_out = _f32(d_out, "d_out")
        B = int(B)
        if d_out.dim() != 2 or B < 1 or d_out.shape[0] % B or d_out.shape[1] % 2:
            raise _lib.TempAmdError("pair_rows_bwd: d_out must be (B N, 2 d)")
        N, d = d_out.shape[0] // B, d_out.shape[1] // 2
        d_a = torch.empty(N, d, dtype=torch.float32, device=d_out.device)
        d_a_inv = torch.empty_like(d_a)
        _lib.check(self.lib.temp_pair_rows_bwd(B, N, d, _ptr(d_out), _ptr(d_a), _ptr(d_a_inv), _stream()), "temp_pair_rows_bwd")
        return d_a, d_a_inv

    # ---- persistent window chain (include/temp_amd.h: TempGruChain) -------------------------------
    def gru_chain_supported(self, d):
        return bool(self.lib.temp_gru_chain_supported(int(d)))

    def gru_chain_pack(self, w_hh):
        """W_hh [3d, d] -> the chain kernels' fragment order (one small launch; the weights change every optimiser step)."""
        w_hh = _f32(w_hh, "w_hh")
        d = w_hh.shape[1]
        out = torch.empty(self.lib.temp_gru_chain_pack_floats(d), dtype=torch.float32, device=w_hh.device)
        layout = self.lib.temp_gru_chain_pack_layout(d)
        _lib.check(self.lib.temp_gru_chain_pack(d, _ptr(w_hh), _ptr(out), _stream()), "temp_gru_chain_pack")
        out.chain_pack_layout = layout                   # (TempGruChain.pack_layout: the kernels follow the pack, not the options)
        return out

    def gru_chain_pack_multi(self, w_hhs, layout=None):
        """gru_chain_pack of several GRUs' W_hh (same width) in ONE launch -> list of packed tensors (views of one buffer).
        layout: None = what the options select, or the _lib.CHAIN_PACK_* layout to write (temp_gru_chain_pack_multi_layout)."""
        w_hhs = [_f32(w, "w_hh") for w in w_hhs]
        d = w_hhs[0].shape[1]
        n = self.lib.temp_gru_chain_pack_floats(d)
        buf = torch.empty(len(w_hhs), n, dtype=torch.float32, device=w_hhs[0].device)
        src = (ctypes.c_void_p * len(w_hhs))(*[w.data_ptr() for w in w_hhs])
        dst = (ctypes.c_void_p * len(w_hhs))(*[buf[i].data_ptr() for i in range(len(w_hhs))])
        if layout is not None:
            _lib.check(self.lib.temp_gru_chain_pack_multi_layout(int(layout), len(w_hhs), d, src, dst, _stream()), "temp_gru_chain_pack_multi_layout")
            return self._tagged([buf[i] for i in range(len(w_hhs))], int(layout))
        layout = self.lib.temp_gru_chain_pack_layout(d)
        _lib.check(self.lib.temp_gru_chain_pack_multi(len(w_hhs), d, src, dst, _stream()), "temp_gru_chain_pack_multi")
        return self._tagged([buf[i] for i in range(len(w_hhs))], layout)

    @staticmethod
    def _tagged(packs, layout):
        for pk in packs:
            pk.chain_pack_layout = layout
        return packs

    def _chain_desc(self, tabs, d, variant, lam=0.0, plane=0, packs=(), b_hhs=(), decay=None, offset=None, n_rnn=None):
        """-> (TempGruChain, the objects it points to: hold both until the call has returned).  plane = N_total * d.  Without packs:
        the tables and n_rnn alone (gru_chain_decay_reduce).
        decay (include/temp_amd.h: TempChainDecay) = a float32 device tensor {w, b} shared by all GRUs of the chain (`lam` is not read
        then); offset (TempChainOffset) = (table float32 [T, d], index int32 [N_total], -1 = none): the states handed out and carried
        on are GRU(...) + table[index]; the packs must be in gru_chain_offset_layout(d) (gru_chain_pack_multi(layout=...))."""
        c = _lib.TempGruChain()
        c.d, c.variant, c.n_panels, c.n_steps, c.max_steps = d, variant, tabs["n_panels"], tabs["n_steps"], tabs["max_steps"]
        c.panel, c.rows, c.sinfo, c.dt = (_i32(tabs[k], k).data_ptr() for k in ("panel", "rows", "sinfo", "dt_bits"))
        c.lambda_, c.saved_plane, c.n_rnn = float(lam), plane, len(packs) or n_rnn
        keep = []
        if packs:
            layouts = {getattr(pk, "chain_pack_layout", None) for pk in packs}
            assert len(layouts) == 1 and None not in layouts, "chain packs without one common layout tag (gru_chain_pack*)"
            c.pack_layout = layouts.pop()
        for i, (pk, b) in enumerate(zip(packs, b_hhs)):
            pk, b = _f32(pk, "packed"), _f32(b, "b_hh")
            keep += [pk, b]
            c.packed[i], c.b_hh[i] = pk.data_ptr(), b.data_ptr()
        if decay is not None:
            decay = _f32(decay, "decay")
            assert decay.numel() == 2
            cd = _lib.TempChainDecay()
            for i in range(c.n_rnn):
                cd.wb[i] = decay.data_ptr()
            c.decay = ctypes.pointer(cd)
            keep += [cd, decay]
        if offset is not None:
            table, index = _f32(offset[0], "offset table"), _i32(offset[1], "offset index")
            assert table.dim() == 2 and table.shape[1] == d and index.numel() * d == plane
            co = _lib.TempChainOffset()
            co.table, co.index, co.n_rows = table.data_ptr(), index.data_ptr(), table.shape[0]
            c.offset = ctypes.pointer(co)
            keep += [co, table, index]
        return c, keep

    def gru_chain_decay_supported(self, d, variant):
        return bool(self.lib.temp_gru_chain_decay_supported(int(d), int(variant)))

    def gru_chain_decay_launches(self):
        return int(self.lib.temp_gru_chain_decay_launches())

    def gru_chain_decay_reduce(self, tabs, d, variant, d_arg, n_rnn):
        """d_arg [N_total] of gru_chain_bwd*(decay=, d_arg=) -> float32 [n_rnn, 2]: per GRU (sum d_arg dt, sum d_arg) over its rows
        with a previous state, in a fixed order (temp_gru_chain_decay_reduce)."""
        c, keep = self._chain_desc(tabs, d, variant, n_rnn=n_rnn)
        d_arg = _f32(d_arg, "d_arg")
        out = torch.empty(n_rnn, 2, dtype=torch.float32, device=d_arg.device)
        nb = int(self.lib.temp_gru_chain_decay_reduce_workspace(ctypes.byref(c)))
        ws = torch.empty(max(nb, 4) // 4, dtype=torch.float32, device=d_arg.device)
        _lib.check(self.lib.temp_gru_chain_decay_reduce(ctypes.byref(c), _ptr(d_arg), _ptr(out), _ptr(ws), nb, _stream()), "temp_gru_chain_decay_reduce")
        return out

    def gru_chain_offset_supported(self, d, variant):
        return bool(self.lib.temp_gru_chain_offset_supported(int(d), int(variant)))

    def gru_chain_offset_layout(self, d):
        return int(self.lib.temp_gru_chain_offset_layout(int(d)))

    def gru_chain_offset_launches(self):
        return int(self.lib.temp_gru_chain_offset_launches())

    def gru_chain_fwd(self, tabs, gi, lam, variant, packs, b_hhs, h_out, saved_all, gi_index=None, decay=None, offset=None):
        d = saved_all.shape[2]
        c, keep = self._chain_desc(tabs, d, variant, lam, saved_all.shape[1] * d, packs, b_hhs, decay, offset)
        if gi_index is not None:
            assert gi_index.shape[0] == saved_all.shape[1]
            c.gi_index = _i32(gi_index, "gi_index").data_ptr()
        gi = _f32(gi, "gi")
        io = _lib.TempChainFwd(gi=gi.data_ptr(), h_out=h_out.data_ptr(), saved=saved_all.data_ptr())
        _lib.check(self.lib.temp_gru_chain_fwd(ctypes.byref(c), ctypes.byref(io), _stream()), "temp_gru_chain_fwd")

    def gru_chain_fwd_x_supported(self, d, variant, max_steps):
        """True when temp_gru_chain_fwd's x route takes this width, variant and longest panel (the input gates computed inside the
        chain forward; TEMP_DEBUG bit 22 turns it off)."""
        return bool(self.lib.temp_gru_chain_fwd_x_supported(int(d), int(variant), int(max_steps)))

    def gru_chain_pack_x_multi(self, w_hhs, w_ihs):
        """W_hh and W_ih of several GRUs -> the packed weights of temp_gru_chain_fwd's x route in ONE launch (list of views of one
        buffer; the chain backward takes them like gru_chain_pack_multi's)."""
        w_hhs, w_ihs = [_f32(w, "w_hh") for w in w_hhs], [_f32(w, "w_ih") for w in w_ihs]
        d = w_hhs[0].shape[1]
        k = len(w_hhs)
        n = self.lib.temp_gru_chain_pack_x_floats(d)
        buf = torch.empty(k, n, dtype=torch.float32, device=w_hhs[0].device)
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        _lib.check(self.lib.temp_gru_chain_pack_x_multi(k, d, arr(w_hhs), arr(w_ihs), arr([buf[i] for i in range(k)]), _stream()),
                   "temp_gru_chain_pack_x_multi")
        return self._tagged([buf[i] for i in range(k)], _lib.CHAIN_PACK_HX_X)

    def gru_chain_fwd_x(self, tabs, x, x_index, lam, variant, packs, b_hhs, b_ihs, h_out, saved_all, decay=None):
        """The chain forward from the x rows (x_index: int32 [N_total], x row of every chain row): no gi (temp_gru_chain_fwd's x route)."""
        d = saved_all.shape[2]
        c, keep = self._chain_desc(tabs, d, variant, lam, saved_all.shape[1] * d, packs, b_hhs, decay)
        x, x_index = _f32(x, "x"), _i32(x_index, "x_index")
        assert x.shape[1] == d and x_index.shape[0] == saved_all.shape[1]
        b_ihs = [_f32(b, "b_ih") for b in b_ihs]
        barr = (ctypes.c_void_p * len(b_ihs))(*[b.data_ptr() for b in b_ihs])
        io = _lib.TempChainFwd(x=x.data_ptr(), x_index=x_index.data_ptr(), b_ih=ctypes.addressof(barr), h_out=h_out.data_ptr(), saved=saved_all.data_ptr())
        _lib.check(self.lib.temp_gru_chain_fwd(ctypes.byref(c), ctypes.byref(io), _stream()), "temp_gru_chain_fwd (x route)")

    def _chain_bwd(self, tabs, saved_all, ups, lam, variant, packs, b_hhs, decay, d_arg, offset, d_state, **out):
        """One temp_gru_chain_bwd call; out: the members of TempChainBwd the route writes (dgi, dgh | g4, row_keys, col_keys)."""
        d = saved_all.shape[2]
        c, keep = self._chain_desc(tabs, d, variant, lam, saved_all.shape[1] * d, packs, b_hhs, decay, offset)
        ups = [_f32(u, "upstream") if u is not None else None for u in ups]      # (None: that block of rows has no upstream gradient)
        arr = (ctypes.c_void_p * max(len(ups), 1))(*[u.data_ptr() if u is not None else None for u in ups])
        d_arg = _f32(d_arg, "d_arg")
        if d_state is not None:
            assert d_state.dtype == torch.float32 and d_state.is_contiguous() and d_state.shape == saved_all.shape[1:]
        io = _lib.TempChainBwd(saved=saved_all.data_ptr(), n_up=len(ups), up=ctypes.addressof(arr))
        for name, t in dict(out, d_arg=d_arg, d_state=d_state).items():
            setattr(io, name, t.data_ptr() if t is not None else None)
        _lib.check(self.lib.temp_gru_chain_bwd(ctypes.byref(c), ctypes.byref(io), _stream()), "temp_gru_chain_bwd")

    def gru_chain_bwd(self, tabs, saved_all, ups, lam, variant, packs, b_hhs, dgi, dgh, decay=None, d_arg=None, offset=None, d_state=None):
        self._chain_bwd(tabs, saved_all, ups, lam, variant, packs, b_hhs, decay, d_arg, offset, d_state, dgi=dgi, dgh=dgh)

    def gru_chain_keys_supported(self, d):
        """True when the chain backward of this width hands out the row / column keys of g4 (f16 two-way split selected)."""
        return bool(self.lib.temp_gru_chain_keys_supported(int(d)))

    def gru_chain_bwd_g4(self, tabs, saved_all, ups, lam, variant, packs, b_hhs, g4, keys=None, decay=None, d_arg=None, offset=None, d_state=None):
        """The chain backward with the gate gradients written once: g4 [N, 4d] = [dr | dz | dn_i | dn_h] (include/temp_amd.h:
        TempChainBwd.g4; nn.GRU gate layout).  keys = (row_keys int32 [N], col_keys int32 [n_rnn + n_panels, 4d]; rows 0 .. n_rnn - 1 are
        the result): also the magnitude keys the consumers of g4 split it with."""
        row_keys, col_keys = keys if keys is not None else (None, None)
        if keys is not None:
            assert offset is None, "an offset chain hands out no keys (its states are not bounded by the f16 split's constant scale)"
            assert row_keys.dtype == torch.int32 and col_keys.dtype == torch.int32 and col_keys.is_contiguous()
            assert row_keys.numel() == saved_all.shape[1] and col_keys.numel() == (len(packs) + tabs["n_panels"]) * 4 * saved_all.shape[2]
        self._chain_bwd(tabs, saved_all, ups, lam, variant, packs, b_hhs, decay, d_arg, offset, d_state, g4=g4, row_keys=row_keys, col_keys=col_keys)

    # ---- persistent window chain of the linear recurrence (include/temp_amd.h: TempLinChain) ------
    def lin_chain_supported(self, d, max_steps=0):
        return bool(self.lib.temp_lin_chain_supported(int(d), int(max_steps)))

    def lin_chain_launches(self):
        return int(self.lib.temp_lin_chain_launches())

    def lin_chain_pack_multi(self, ws):
        """W (in, out) of several linear cells -> the chain kernels' fragment order in ONE launch (list of views of one buffer)."""
        ws = [_f32(w, "w") for w in ws]
        d, k = ws[0].shape[0], len(ws)
        assert all(tuple(w.shape) == (d, d) for w in ws)
        buf = torch.empty(k, self.lib.temp_lin_chain_pack_floats(d), dtype=torch.float32, device=ws[0].device)
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        _lib.check(self.lib.temp_lin_chain_pack_multi(k, d, arr(ws), arr([buf[i] for i in range(k)]), _stream()), "temp_lin_chain_pack_multi")
        return [buf[i] for i in range(k)]

    def _lin_desc(self, tabs, d, lam, packs, act):
        c = _lib.TempLinChain()
        c.d, c.n_panels, c.n_steps, c.max_steps = d, tabs["n_panels"], tabs["n_steps"], tabs["max_steps"]
        c.panel, c.rows, c.sinfo, c.dt = (_i32(tabs[k], k).data_ptr() for k in ("panel", "rows", "sinfo", "dt_bits"))
        c.lambda_, c.n_w, c.act = float(lam), len(packs), int(act)
        keep = [_f32(pk, "packed") for pk in packs]
        for i, pk in enumerate(keep):
            c.packed[i] = pk.data_ptr()
        return c, keep

    def lin_chain_fwd(self, tabs, x, x_index, lam, packs, act, h, hdec):
        """ALL positions of the linear recurrence in one launch: h = act(x[x_index] + hdec . W), hdec = dec . h_prev; h and hdec
        (N_total, d) are written whole.  x_index: int32 [N_total] or None (x row = chain row)."""
        x, x_index = _f32(x, "x"), _i32(x_index, "x_index")
        d = x.shape[1]
        assert h.shape == hdec.shape and h.shape[1] == d and h.is_contiguous() and hdec.is_contiguous() and h.dtype == hdec.dtype == torch.float32
        assert (x_index.shape[0] if x_index is not None else x.shape[0]) == h.shape[0]
        c, keep = self._lin_desc(tabs, d, lam, packs, act)
        _lib.check(self.lib.temp_lin_chain_fwd(ctypes.byref(c), _ptr(x), _ptr(x_index), _ptr(h), _ptr(hdec), _stream()), "temp_lin_chain_fwd")

    def lin_chain_bwd(self, tabs, h, ups, lam, packs, act, d_pre):
        """The backward of lin_chain_fwd in one launch: d_pre (N_total, d) = the gradient in front of the activation of every row (= d_x
        in chain order, and the left factor of the weight gradients).  ups: one upstream gradient per block of sinfo (None: none)."""
        h = _f32(h, "h")
        d = h.shape[1]
        assert d_pre.shape == h.shape and d_pre.is_contiguous() and d_pre.dtype == torch.float32
        ups = [_f32(u, "upstream") if u is not None else None for u in ups]
        arr = (ctypes.c_void_p * max(len(ups), 1))(*[u.data_ptr() if u is not None else None for u in ups])
        c, keep = self._lin_desc(tabs, d, lam, packs, act)
        _lib.check(self.lib.temp_lin_chain_bwd(ctypes.byref(c), _ptr(h), len(ups), arr, _ptr(d_pre), _stream()), "temp_lin_chain_bwd")

    # ---- one position of the linear recurrence on gathered rows, one or two history sources in front of one activation
    # (include/temp_amd.h: temp_lin_rows_fwd / _bwd, temp_lin_rows2_fwd / _bwd: one implementation, two C signatures) ------
    def lin_rows_supported(self, d):
        return bool(self.lib.temp_lin_rows_supported(int(d)))

    def lin_rows2_supported(self, d):
        return bool(self.lib.temp_lin_rows2_supported(int(d)))

    def _lin_rows_pack(self, pack, d, backward):
        """The forward / backward half of one matrix's lin_chain_pack_multi buffer."""
        pack, half = _f32(pack, "packed"), self.lib.temp_lin_chain_pack_floats(d) // 2
        assert pack.numel() == 2 * half
        return pack.view(-1)[half:] if backward else pack.view(-1)[:half]

    def _lin_rows_call(self, which, n, d, head, srcs, lam, packs, backward, act, outs):
        """temp_lin_rows<2>_<which>(n, d, head.., the sources' tensors source by source, lam, the packs' halves, act, outs..)."""
        for s in srcs:
            assert s[-2].shape[0] == n and s[-1].numel() == n                                      # (rows, dt)
        for t in outs:
            assert tuple(t.shape) == (n, d) and t.is_contiguous() and t.dtype == torch.float32
        name = "temp_lin_rows%s_%s" % ("" if len(srcs) == 1 else len(srcs), which)
        packs = [self._lin_rows_pack(p, d, backward) for p in packs]
        _lib.check(getattr(self.lib, name)(n, d, *[_ptr(t) for t in list(head) + [t for s in srcs for t in s]], float(lam), *[_ptr(p) for p in packs],
                                           int(act), *[_ptr(t) for t in outs], _stream()), name)

    def _lin_rows_fwd(self, x, x_rows, srcs, lam, packs, act, out, hdecs):
        """srcs: (H, rows, dt) per source."""
        x, x_rows = _f32(x, "x"), _i32(x_rows, "x_rows")
        srcs = [(_f32(H, "H"), _i32(rows, "rows"), _f32(dt, "dt")) for H, rows, dt in srcs]
        n, d = srcs[0][1].shape[0], x.shape[1]
        assert all(s[0].shape[1] == d for s in srcs) and (x_rows.shape[0] if x_rows is not None else x.shape[0]) == n
        self._lin_rows_call("fwd", n, d, (x, x_rows), srcs, lam, packs, False, act, [out] + list(hdecs))

    def _lin_rows_bwd(self, out, up, srcs, lam, packs, act, d_pre, d_hrows):
        """srcs: (rows, dt) per source."""
        out, up = _f32(out, "out"), _f32(up, "up")
        srcs = [(_i32(rows, "rows"), _f32(dt, "dt")) for rows, dt in srcs]
        n, d = up.shape
        assert out.shape == up.shape
        self._lin_rows_call("bwd", n, d, (out, up), srcs, lam, packs, True, act, [d_pre] + list(d_hrows))

    def lin_rows_fwd(self, x, x_rows, H, h_rows, dt, lam, pack, act, out, hdec):
        """out = act(x[x_rows] + hdec . W), hdec = exp(-lam dt) H[h_rows] (0 where h_rows < 0), one launch; out and hdec (n, d) are
        written whole.  x_rows: int32 [n] or None (row i reads x[i]); pack: lin_chain_pack_multi([W])[0]."""
        self._lin_rows_fwd(x, x_rows, [(H, h_rows, dt)], lam, [pack], act, out, [hdec])

    def lin_rows_bwd(self, out, up, h_rows, dt, lam, pack, act, d_pre, d_hrows):
        """The backward of lin_rows_fwd in one launch: d_pre = up . [out > 0] (act = 1) or up, d_hrows = exp(-lam dt) (d_pre . W^T) (0
        where h_rows < 0); both (n, d) are written whole."""
        self._lin_rows_bwd(out, up, [(h_rows, dt)], lam, [pack], act, d_pre, [d_hrows])

    def lin_rows2_fwd(self, x, x_rows, Hf, rows_f, dt_f, Hb, rows_b, dt_b, lam, pack_f, pack_b, act, out, hdec_f, hdec_b):
        """out = act(x[x_rows] + hdec_f . W_f + hdec_b . W_b), hdec_s = exp(-lam dt_s) H_s[rows_s] (0 where rows_s < 0), one launch; out,
        hdec_f and hdec_b (n, d) are written whole.  x_rows: int32 [n] or None (row i reads x[i]); pack_s: lin_chain_pack_multi([W_s])[0]."""
        self._lin_rows_fwd(x, x_rows, [(Hf, rows_f, dt_f), (Hb, rows_b, dt_b)], lam, [pack_f, pack_b], act, out, [hdec_f, hdec_b])

    def lin_rows2_bwd(self, out, up, rows_f, dt_f, rows_b, dt_b, lam, pack_f, pack_b, act, d_pre, d_hrows_f, d_hrows_b):
        """The backward of lin_rows2_fwd in one launch: d_pre = up . [out > 0] (act = 1) or up, d_hrows_s = exp(-lam dt_s) (d_pre . W_s^T)
        (0 where rows_s < 0); all three (n, d) are written whole."""
        self._lin_rows_bwd(out, up, [(rows_f, dt_f), (rows_b, dt_b)], lam, [pack_f, pack_b], act, d_pre, [d_hrows_f, d_hrows_b])

    def gru_grads_g4_supported(self, ns, d, variant):
        """True when gru_grads_g4 takes GRUs of these row counts and this width (then the chain backward should write g4)."""
        k = len(ns)
        if k < 1 or k > 4 or variant != _lib.GRU_TORCH:
            return False
        return self.lib.temp_gru_grads_g4_workspace(k, (ctypes.c_int * k)(*[int(n) for n in ns]), int(d)) > 0

    def gru_grads_g4(self, xs, hdecs, g4s, w_ihs, d_xs, row_keys=None, col_keys=None, x_col_keys=None):
        """Weight / bias gradients and d_x of several GRUs of one width from their gate-gradient matrices (include/temp_amd.h:
        temp_gru_grads_g4) -> [(d_w_ih, d_w_hh, d_b_ih, d_b_hh)] per GRU.  row_keys / col_keys: per GRU the int32 key tensors of
        gru_chain_bwd_g4(keys=...) ([n_i] and [4d]); with them the products run on the f16 pipe (temp_gru_grads_g4_keys)."""
        k = len(xs)
        d = xs[0].shape[1]
        dev = xs[0].device
        ns = (ctypes.c_int * k)(*[x.shape[0] for x in xs])
        nb = self.lib.temp_gru_grads_g4_workspace(k, ns, d)
        if nb == 0:
            raise ValueError("temp_gru_grads_g4: unsupported shape (check gru_grads_g4_supported first)")
        keep = [[_f32(t, "operand") for t in ts] for ts in (xs, hdecs, w_ihs)]
        for g in g4s:
            assert g.dtype == torch.float32 and g.is_contiguous() and g.shape[1] == 4 * d
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        dx = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in d_xs])
        d_w = torch.empty(2 * k, 3 * d, d, dtype=torch.float32, device=dev)
        d_b = torch.empty(2 * k, 3 * d, dtype=torch.float32, device=dev)
        ws = self._ws(nb, dev)
        if row_keys is not None and col_keys is not None:
            for rk, ck, x in zip(row_keys, col_keys, xs):
                assert rk.dtype == torch.int32 and ck.dtype == torch.int32 and rk.is_contiguous() and ck.is_contiguous()
                assert rk.numel() == x.shape[0] and ck.numel() == 4 * d
            xk = None
            if x_col_keys is not None:
                for t in x_col_keys:
                    assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == d
                xk = arr(x_col_keys)
            rc = self.lib.temp_gru_grads_g4_keys(k, ns, d, arr(keep[0]), arr(keep[1]), arr(g4s), arr(keep[2]), dx, _ptr(d_w), _ptr(d_b),
                                                 arr(row_keys), arr(col_keys), xk, _ptr(ws), ws.numel(), _stream())
            _lib.check(rc, "temp_gru_grads_g4_keys")
            return [(d_w[2 * i], d_w[2 * i + 1], d_b[2 * i], d_b[2 * i + 1]) for i in range(k)]
        rc = self.lib.temp_gru_grads_g4(k, ns, d, arr(keep[0]), arr(keep[1]), arr(g4s), arr(keep[2]), dx, _ptr(d_w), _ptr(d_b), _ptr(ws),
                                        ws.numel(), _stream())
        _lib.check(rc, "temp_gru_grads_g4")
        return [(d_w[2 * i], d_w[2 * i + 1], d_b[2 * i], d_b[2 * i + 1]) for i in range(k)]

    def gru_grads_g4_rows_supported(self, ns, d, variant, table_rows):
        """True when gru_grads_g4_rows takes GRUs of these row counts and this width over a table of `table_rows` rows."""
        k = len(ns)
        if k < 1 or k > 4 or variant != _lib.GRU_TORCH:
            return False
        return bool(self.lib.temp_gru_grads_g4_rows_supported(k, (ctypes.c_int * k)(*[int(n) for n in ns]), int(d), int(table_rows)))

    def gru_grads_g4_rows(self, table, x_rows, hdecs, g4s, w_ihs, d_xs, row_keys, col_keys, x_col_keys):
        """gru_grads_g4 on the f16 pipe with every GRU's input rows read in place: row m of GRU i's x is table[x_rows[i][m]] (x_rows:
        int32 device lists, 0 <= r < table rows; include/temp_amd.h: temp_gru_grads_g4_rows) -- bit for bit what gru_grads_g4 gives on
        the gathered rows with the same keys, all of which are required.  d_xs: in GRU row order."""
        table = _f32(table, "table")
        k, d, dev = len(x_rows), table.shape[1], table.device
        ns = (ctypes.c_int * k)(*[r.shape[0] for r in x_rows])
        nb = self.lib.temp_gru_grads_g4_workspace(k, ns, d)
        if nb == 0:
            raise ValueError("temp_gru_grads_g4_rows: unsupported shape (check gru_grads_g4_supported first)")
        x_rows = [_i32(r, "x_rows") for r in x_rows]
        keep = [[_f32(t, "operand") for t in ts] for ts in (hdecs, w_ihs)]
        for g, r, h, rk, ck, xk in zip(g4s, x_rows, keep[0], row_keys, col_keys, x_col_keys):
            assert g.dtype == torch.float32 and g.is_contiguous() and g.shape == (r.shape[0], 4 * d) and h.shape == (r.shape[0], d)
            assert all(t.dtype == torch.int32 and t.is_contiguous() for t in (rk, ck, xk))
            assert rk.numel() == r.shape[0] and ck.numel() == 4 * d and xk.numel() == d
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        dx = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in d_xs])
        d_w = torch.empty(2 * k, 3 * d, d, dtype=torch.float32, device=dev)
        d_b = torch.empty(2 * k, 3 * d, dtype=torch.float32, device=dev)
        ws = self._ws(nb, dev)
        rc = self.lib.temp_gru_grads_g4_rows(k, ns, d, _ptr(table), table.shape[0], arr(x_rows), arr(keep[0]), arr(g4s), arr(keep[1]), dx,
                                             _ptr(d_w), _ptr(d_b), arr(row_keys), arr(col_keys), arr(x_col_keys), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_gru_grads_g4_rows")
        return [(d_w[2 * i], d_w[2 * i + 1], d_b[2 * i], d_b[2 * i + 1]) for i in range(k)]

    def gru_weight_grads(self, x, hdec, dgi, dgh, w_ih, variant, d_x):
        n, d = x.shape
        w_ih = _f32(w_ih, "w_ih")
        dev = x.device
        d_w_ih = torch.empty_like(w_ih)
        d_w_hh = torch.empty(3 * d, d, dtype=torch.float32, device=dev)
        d_b_ih = torch.empty(w_ih.shape[0], dtype=torch.float32, device=dev)
        d_b_hh = torch.empty(3 * d, dtype=torch.float32, device=dev)
        ws = self._ws(self.lib.temp_gru_weight_grads_workspace(n, d, variant), dev)
        rc = self.lib.temp_gru_weight_grads(n, d, variant, _ptr(x), _ptr(hdec), _ptr(dgi), _ptr(dgh), _ptr(w_ih), _ptr(d_x),
                                            _ptr(d_w_ih), _ptr(d_w_hh), _ptr(d_b_ih), _ptr(d_b_hh), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_gru_weight_grads")
        return d_w_ih, d_w_hh, d_b_ih, d_b_hh

    def gru_weight_grads_multi(self, xs, hdecs, dgis, dghs, w_ihs, variant, d_xs):
        """Weight / bias gradients and d_x of SEVERAL GRUs of one width in one weight-gradient launch (include/temp_amd.h:
        temp_gru_weight_grads_multi) -> [(d_w_ih, d_w_hh, d_b_ih, d_b_hh)] per GRU, or None when the library takes this shape
        through the per-GRU call (nothing launched)."""
        k = len(xs)
        if k < 1 or k > 4 or variant != _lib.GRU_TORCH or any(h is None for h in hdecs):
            return None
        d = xs[0].shape[1]
        dev = xs[0].device
        ns = (ctypes.c_int * k)(*[x.shape[0] for x in xs])
        nb = self.lib.temp_gru_weight_grads_multi_workspace(k, ns, d, variant)
        if nb == 0:
            return None
        keep = [[_f32(t, "operand") for t in ts] for ts in (xs, hdecs, dgis, dghs, w_ihs)]
        arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
        dx = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in d_xs])
        d_w = torch.empty(2 * k, 3 * d, d, dtype=torch.float32, device=dev)
        d_b = torch.empty(2 * k, 3 * d, dtype=torch.float32, device=dev)
        ws = self._ws(nb, dev)
        rc = self.lib.temp_gru_weight_grads_multi(k, ns, d, variant, arr(keep[0]), arr(keep[1]), arr(keep[2]), arr(keep[3]), arr(keep[4]), dx,
                                                  _ptr(d_w), _ptr(d_b), _ptr(ws), ws.numel(), _stream())
        if rc == 2:                                   # TEMP_E_UNSUPPORTED: nothing was launched
            return None
        _lib.check(rc, "temp_gru_weight_grads_multi")
        return [(d_w[2 * i], d_w[2 * i + 1], d_b[2 * i], d_b[2 * i + 1]) for i in range(k)]

    # ---- plain GEMMs + candidate cross-entropy (link-prediction loss) ---------------------------------
    def linear(self, a, b, trans_b, out=None, a_keys=None):
        """a[M,K] . b  (b is [K,N], or [N,K] when trans_b); out: an (M, N) contiguous tensor to write into.  a_keys: int32 [M], the
        magnitude keys of a's rows (absmax_keys): the product then runs on the f16 pipe without a pass of its own (temp_linear_keys)."""
        a, b = _f32(a, "a"), _f32(b, "b")
        M, K = a.shape
        N = b.shape[0] if trans_b else b.shape[1]
        c = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=a.device)
        assert c.shape == (M, N) and c.is_contiguous() and c.dtype == torch.float32
        if a_keys is not None:
            assert a_keys.dtype == torch.int32 and a_keys.is_contiguous() and a_keys.numel() == M
            rc = self.lib.temp_linear_keys(M, N, K, _ptr(a), K, _ptr(a_keys), _ptr(b), b.shape[1], int(trans_b), _ptr(c), N, _stream())
            _lib.check(rc, "temp_linear_keys")
            return c
        rc = self.lib.temp_linear(M, N, K, _ptr(a), K, _ptr(b), b.shape[1], int(trans_b), _ptr(c), N, _stream())
        _lib.check(rc, "temp_linear")
        return c

    def absmax_keys(self, x, rows=True, cols=True):
        """Magnitude keys of a matrix (include/temp_amd.h: temp_absmax_keys) -> (row_keys int32 [n] | None, col_keys int32 [d] | None)."""
        x = _f32(x, "x")
        n, d = x.shape
        rk = torch.empty(n, dtype=torch.int32, device=x.device) if rows else None
        ck = torch.empty(self.lib.temp_keys_cols_size(d), dtype=torch.int32, device=x.device) if cols else None
        _lib.check(self.lib.temp_absmax_keys(n, d, _ptr(x), d, _ptr(rk), _ptr(ck), _stream()), "temp_absmax_keys")
        return rk, (ck[:d] if cols else None)

    def linear_t(self, a, b, trans_b, out_t):
        """out_t[N, M] = (a[M,K] . b)^T written into the contiguous matrix `out_t` (b is [K,N], or [N,K] when trans_b)."""
        a, b = _f32(a, "a"), _f32(b, "b")
        M, K = a.shape
        N = b.shape[0] if trans_b else b.shape[1]
        if out_t.shape != (N, M) or not out_t.is_contiguous() or out_t.dtype != torch.float32:
            raise ValueError("linear_t: out_t must be a contiguous float32 (N, M) matrix")
        rc = self.lib.temp_linear_t(M, N, K, _ptr(a), K, _ptr(b), b.shape[1], int(trans_b), _ptr(out_t), M, _stream())
        _lib.check(rc, "temp_linear_t")
        return out_t

    def linear_multi(self, a_list, b_list, trans_b, out):
        """out rows [r_i, r_i + M_i) = a_i[M_i,K] . b_i  for every problem i, r_i = running row offset: the per-window
        products of the loss in ceil(count / 4) launches.  `out` is a preallocated (sum M_i, N) matrix."""
        K = a_list[0].shape[1]
        N = out.shape[1]
        arr = (_lib.TempLinearProblem * len(a_list))()
        row, keep = 0, []
        for i, (a, b) in enumerate(zip(a_list, b_list)):
            a, b = _f32(a, "a"), _f32(b, "b")
            keep.append((a, b))
            if a.shape[1] != K or b.shape != ((N, K) if trans_b else (K, N)):
                raise ValueError("linear_multi: problems must share N, K and the layout of b")
            arr[i].M, arr[i].A, arr[i].B = a.shape[0], a.data_ptr(), b.data_ptr()
            arr[i].C = out.data_ptr() + row * N * 4
            row += a.shape[0]
        if row != out.shape[0] or not out.is_contiguous():
            raise ValueError("linear_multi: out must be a contiguous (sum M_i, N) matrix")
        rc = self.lib.temp_linear_multi(len(a_list), arr, N, K, K, K if trans_b else N, int(trans_b), N, _stream())
        _lib.check(rc, "temp_linear_multi")
        return out

    def bilinear_query_fwd(self, kind, ent_rows, known_idx, rel, rel_idx, is_tail):
        ent_rows, rel = _f32(ent_rows, "ent_rows"), _f32(rel, "rel")
        known_idx, rel_idx, is_tail = _i32(known_idx, "known_idx"), _i32(rel_idx, "rel_idx"), _i32(is_tail, "is_tail")
        P, d = known_idx.shape[0], ent_rows.shape[1]
        q = torch.empty(P, d, dtype=torch.float32, device=ent_rows.device)
        rc = self.lib.temp_bilinear_query_fwd(P, d, _lib.SCORE_KINDS[kind], _ptr(ent_rows), _ptr(known_idx), _ptr(rel), _ptr(rel_idx), _ptr(is_tail),
                                              _ptr(q), _stream())
        _lib.check(rc, "temp_bilinear_query_fwd")
        return q

    def bilinear_query_bwd(self, kind, ent_rows, known_idx, rel, rel_idx, is_tail, d_q):
        ent_rows, rel, d_q = _f32(ent_rows, "ent_rows"), _f32(rel, "rel"), _f32(d_q, "d_q")
        known_idx, rel_idx, is_tail = _i32(known_idx, "known_idx"), _i32(rel_idx, "rel_idx"), _i32(is_tail, "is_tail")
        P, d = known_idx.shape[0], ent_rows.shape[1]
        dk = torch.empty(P, d, dtype=torch.float32, device=ent_rows.device)
        dr = torch.empty(P, d, dtype=torch.float32, device=ent_rows.device)
        rc = self.lib.temp_bilinear_query_bwd(P, d, _lib.SCORE_KINDS[kind], _ptr(ent_rows), _ptr(known_idx), _ptr(rel), _ptr(rel_idx), _ptr(is_tail),
                                              _ptr(d_q), _ptr(dk), _ptr(dr), _stream())
        _lib.check(rc, "temp_bilinear_query_bwd")
        return dk, dr

    # ---- candidate-gather loss, one table: L1 distances (TransE; include/temp_amd.h: temp_l1_ce_fwd ...) and inner products (the
    # bilinear scorers' gather route; temp_dot_ce_fwd ...).  `op` = "l1" | "dot" picks the entry point; shapes and checks are shared ----
    def _cand_ce_fwd(self, op, q, table, base, cand):
        q, table, base, cand = _f32(q, "q"), _f32(table, "table"), _i32(base, "base"), _i32(cand, "cand")
        P, d = q.shape
        C = cand.shape[1]
        s = torch.empty(P, C, dtype=torch.float32, device=q.device)
        loss = torch.empty(P, dtype=torch.float32, device=q.device)
        lse = torch.empty(P, dtype=torch.float32, device=q.device)
        name = "temp_%s_ce_fwd" % op
        rc = getattr(self.lib, name)(P, C, d, _ptr(q), _ptr(table), _ptr(base), _ptr(cand), _ptr(s), _ptr(loss), _ptr(lse), _stream())
        _lib.check(rc, name)
        return s, loss, lse

    def _cand_ce_bwd_q(self, op, q, table, base, cand, s, lse, scale, inv_rows, row_scale):
        q, table, base, cand = _f32(q, "q"), _f32(table, "table"), _i32(base, "base"), _i32(cand, "cand")
        s, lse, scale, row_scale = _f32(s, "s"), _f32(lse, "lse"), _f32(scale, "scale"), _f32(row_scale, "row_scale")
        P, d = q.shape
        g = torch.empty_like(s)
        d_q = torch.empty_like(q)
        name = "temp_%s_ce_bwd_q" % op
        rc = getattr(self.lib, name)(P, cand.shape[1], d, _ptr(q), _ptr(table), _ptr(base), _ptr(cand), _ptr(s), _ptr(lse), _ptr(scale),
                                     float(inv_rows), _ptr(row_scale), _ptr(g), _ptr(d_q), _stream())
        _lib.check(rc, name)
        return g, d_q

    def _cand_ce_bwd_table(self, op, q, table, slot_ptr, slot, g):
        q, table, g = _f32(q, "q"), _f32(table, "table"), _f32(g, "g")
        slot_ptr, slot = _i32(slot_ptr, "slot_ptr"), _i32(slot, "slot")
        n_rows, d = table.shape
        if slot_ptr.shape[0] != n_rows + 1 or slot.numel() != g.numel():
            raise ValueError("%s_ce_bwd_table: slot lists do not match the table / the candidate matrix" % op)
        d_table = torch.empty_like(table)
        name = "temp_%s_ce_bwd_table" % op
        rc = getattr(self.lib, name)(n_rows, d, g.shape[1], _ptr(q), _ptr(table), _ptr(slot_ptr), _ptr(slot), _ptr(g), _ptr(d_table), _stream())
        _lib.check(rc, name)
        return d_table

    def l1_ce_fwd(self, q, table, base, cand):
        """-> (s [P, C], loss_rows [P], lse [P]) of the candidate CE over s[p,k] = -|q[p] - table[base[p] + cand[p,k]]|_1 (base None = 0)."""
        return self._cand_ce_fwd("l1", q, table, base, cand)

    def l1_ce_bwd_q(self, q, table, base, cand, s, lse, scale, inv_rows, row_scale=None):
        """-> (g [P, C], d_q [P, d]): the softmax gradient at the candidates and the query side of its adjoint."""
        return self._cand_ce_bwd_q("l1", q, table, base, cand, s, lse, scale, inv_rows, row_scale)

    def l1_ce_bwd_table(self, q, table, slot_ptr, slot, g):
        """-> d_table [rows, d]: the candidate side of the adjoint over the slot lists (link_loss.l1_slots)."""
        return self._cand_ce_bwd_table("l1", q, table, slot_ptr, slot, g)

    def dot_ce_fwd(self, q, table, base, cand):
        """-> (s [P, C], loss_rows [P], lse [P]) of the candidate CE over s[p,k] = <q[p], table[base[p] + cand[p,k]]> (base None = 0)."""
        return self._cand_ce_fwd("dot", q, table, base, cand)

    def dot_ce_bwd_q(self, q, table, base, cand, s, lse, scale, inv_rows, row_scale=None):
        """-> (g [P, C], d_q [P, d] = sum_k g[p,k] table[row]): the softmax gradient at the candidates and the query side of its adjoint."""
        return self._cand_ce_bwd_q("dot", q, table, base, cand, s, lse, scale, inv_rows, row_scale)

    def dot_ce_bwd_table(self, q, table, slot_ptr, slot, g):
        """-> d_table [rows, d] = sum over a row's slots of g[slot] q[slot // C] (link_loss.l1_slots); `table` gives the shape only."""
        return self._cand_ce_bwd_table("dot", q, table, slot_ptr, slot, g)

    def l1_scores(self, q, table):
        """-> scores [P, ld], ld = N rounded up to a multiple of 4: -|q[p] - table[n]|_1, the pad columns -inf (what filtered_rank takes)."""
        q, table = _f32(q, "q"), _f32(table, "table")
        P, d = q.shape
        N = table.shape[0]
        ld = (N + 3) // 4 * 4
        out = torch.empty(P, ld, dtype=torch.float32, device=q.device)
        rc = self.lib.temp_l1_scores(P, N, d, _ptr(q), _ptr(table), ld, _ptr(out), _stream())
        _lib.check(rc, "temp_l1_scores")
        return out

    def gated_query_fwd(self, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail):
        """Folded query of the mixed known rows w * a_rows[a_idx] + (1 - w) * b_rows[b_idx] (a_idx < 0: b_rows[b_idx] alone)."""
        a_rows, b_rows, w, rel = _f32(a_rows, "a_rows"), _f32(b_rows, "b_rows"), _f32(w, "w"), _f32(rel, "rel")
        a_idx, b_idx, rel_idx, is_tail = _i32(a_idx, "a_idx"), _i32(b_idx, "b_idx"), _i32(rel_idx, "rel_idx"), _i32(is_tail, "is_tail")
        P, d = b_idx.shape[0], b_rows.shape[1]
        q = torch.empty(P, d, dtype=torch.float32, device=b_rows.device)
        rc = self.lib.temp_gated_query_fwd(P, d, _lib.SCORE_KINDS[kind], _ptr(a_rows), _ptr(a_idx), _ptr(b_rows), _ptr(b_idx), _ptr(w), _ptr(rel),
                                           _ptr(rel_idx), _ptr(is_tail), _ptr(q), _stream())
        _lib.check(rc, "temp_gated_query_fwd")
        return q

    def gated_query_bwd(self, kind, a_rows, a_idx, b_rows, b_idx, w, rel, rel_idx, is_tail, d_q):
        """-> per-row (d_a_rows, d_b_rows, d_rel_rows) [P, d] and d_w [P] (include/temp_amd.h: temp_gated_query_bwd)."""
        a_rows, b_rows, w, rel, d_q = _f32(a_rows, "a_rows"), _f32(b_rows, "b_rows"), _f32(w, "w"), _f32(rel, "rel"), _f32(d_q, "d_q")
        a_idx, b_idx, rel_idx, is_tail = _i32(a_idx, "a_idx"), _i32(b_idx, "b_idx"), _i32(rel_idx, "rel_idx"), _i32(is_tail, "is_tail")
        P, d = b_idx.shape[0], b_rows.shape[1]
        da, db, dr = (torch.empty(P, d, dtype=torch.float32, device=b_rows.device) for _ in range(3))
        dw = torch.empty(P, dtype=torch.float32, device=b_rows.device)
        rc = self.lib.temp_gated_query_bwd(P, d, _lib.SCORE_KINDS[kind], _ptr(a_rows), _ptr(a_idx), _ptr(b_rows), _ptr(b_idx), _ptr(w), _ptr(rel),
                                           _ptr(rel_idx), _ptr(is_tail), _ptr(d_q), _ptr(da), _ptr(db), _ptr(dr), _ptr(dw), _stream())
        _lib.check(rc, "temp_gated_query_bwd")
        return da, db, dr, dw

    # ---- the same calls over the per-row mix of two tables: gated TransE (include/temp_amd.h: temp_l1_mix_ce_fwd ...) and the gated
    # bilinear scorers' gather route (temp_dot_mix_ce_fwd ...) ----
    def _cand_mix_ce_fwd(self, op, q, table_a, table_b, w, base, cand):
        q, table_a, table_b, w = _f32(q, "q"), _f32(table_a, "table_a"), _f32(table_b, "table_b"), _f32(w, "w")
        base, cand = _i32(base, "base"), _i32(cand, "cand")
        P, d = q.shape
        C = cand.shape[1]
        if table_a.shape != table_b.shape or w.numel() != P:
            raise ValueError("%s_mix_ce_fwd: the two tables must have one shape and w one entry per row" % op)
        s = torch.empty(P, C, dtype=torch.float32, device=q.device)
        loss = torch.empty(P, dtype=torch.float32, device=q.device)
        lse = torch.empty(P, dtype=torch.float32, device=q.device)
        name = "temp_%s_mix_ce_fwd" % op
        rc = getattr(self.lib, name)(P, C, d, _ptr(q), _ptr(table_a), _ptr(table_b), _ptr(w), _ptr(base), _ptr(cand), _ptr(s), _ptr(loss),
                                     _ptr(lse), _stream())
        _lib.check(rc, name)
        return s, loss, lse

    def _cand_mix_ce_bwd_q(self, op, q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale):
        q, table_a, table_b, w = _f32(q, "q"), _f32(table_a, "table_a"), _f32(table_b, "table_b"), _f32(w, "w")
        base, cand = _i32(base, "base"), _i32(cand, "cand")
        s, lse, scale, row_scale = _f32(s, "s"), _f32(lse, "lse"), _f32(scale, "scale"), _f32(row_scale, "row_scale")
        P, d = q.shape
        if table_a.shape != table_b.shape or w.numel() != P:
            raise ValueError("%s_mix_ce_bwd_q: the two tables must have one shape and w one entry per row" % op)
        g = torch.empty_like(s)
        d_q = torch.empty_like(q)
        d_w = torch.empty(P, dtype=torch.float32, device=q.device)
        name = "temp_%s_mix_ce_bwd_q" % op
        rc = getattr(self.lib, name)(P, cand.shape[1], d, _ptr(q), _ptr(table_a), _ptr(table_b), _ptr(w), _ptr(base), _ptr(cand), _ptr(s),
                                     _ptr(lse), _ptr(scale), float(inv_rows), _ptr(row_scale), _ptr(g), _ptr(d_q), _ptr(d_w), _stream())
        _lib.check(rc, name)
        return g, d_q, d_w

    def _cand_mix_ce_bwd_table(self, op, q, table_a, table_b, w, slot_ptr, slot, g):
        q, table_a, table_b, w, g = _f32(q, "q"), _f32(table_a, "table_a"), _f32(table_b, "table_b"), _f32(w, "w"), _f32(g, "g")
        slot_ptr, slot = _i32(slot_ptr, "slot_ptr"), _i32(slot, "slot")
        n_rows, d = table_a.shape
        if table_a.shape != table_b.shape or slot_ptr.shape[0] != n_rows + 1 or slot.numel() != g.numel() or w.numel() != g.shape[0]:
            raise ValueError("%s_mix_ce_bwd_table: slot lists / weights do not match the tables / the candidate matrix" % op)
        d_a, d_b = torch.empty_like(table_a), torch.empty_like(table_b)
        name = "temp_%s_mix_ce_bwd_table" % op
        rc = getattr(self.lib, name)(n_rows, d, g.shape[1], _ptr(q), _ptr(table_a), _ptr(table_b), _ptr(w), _ptr(slot_ptr), _ptr(slot),
                                     _ptr(g), _ptr(d_a), _ptr(d_b), _stream())
        _lib.check(rc, name)
        return d_a, d_b

    def l1_mix_ce_fwd(self, q, table_a, table_b, w, base, cand):
        """-> (s [P, C], loss_rows [P], lse [P]) over s[p,k] = -|q[p] - mix(w[p], table_a[row], table_b[row])|_1, row = base[p] + cand[p,k]."""
        return self._cand_mix_ce_fwd("l1", q, table_a, table_b, w, base, cand)

    def l1_mix_ce_bwd_q(self, q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale=None):
        """-> (g [P, C], d_q [P, d], d_w [P]): the softmax gradient, the query side of its adjoint and the candidate weight's."""
        return self._cand_mix_ce_bwd_q("l1", q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale)

    def l1_mix_ce_bwd_table(self, q, table_a, table_b, w, slot_ptr, slot, g):
        """-> (d_table_a, d_table_b) [rows, d]: the candidate side of the adjoint over the slot lists (link_loss.l1_slots)."""
        return self._cand_mix_ce_bwd_table("l1", q, table_a, table_b, w, slot_ptr, slot, g)

    def dot_mix_ce_fwd(self, q, table_a, table_b, w, base, cand):
        """-> (s [P, C], loss_rows [P], lse [P]) over s[p,k] = <q[p], mix(w[p], table_a[row], table_b[row])>, row = base[p] + cand[p,k]."""
        return self._cand_mix_ce_fwd("dot", q, table_a, table_b, w, base, cand)

    def dot_mix_ce_bwd_q(self, q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale=None):
        """-> (g [P, C], d_q [P, d], d_w [P]): the softmax gradient, the query side of its adjoint and the candidate weight's."""
        return self._cand_mix_ce_bwd_q("dot", q, table_a, table_b, w, base, cand, s, lse, scale, inv_rows, row_scale)

    def dot_mix_ce_bwd_table(self, q, table_a, table_b, w, slot_ptr, slot, g):
        """-> (d_table_a, d_table_b) [rows, d] = sum over a row's slots of (w, 1 - w)[p] g[slot] q[p], p = slot // C."""
        return self._cand_mix_ce_bwd_table("dot", q, table_a, table_b, w, slot_ptr, slot, g)

    def l1_mix_scores(self, q, table_a, table_b, w):
        """-> scores [P, ld], ld = N rounded up to a multiple of 4: -|q[p] - mix(w[p], table_a[n], table_b[n])|_1, the pad columns -inf."""
        q, table_a, table_b, w = _f32(q, "q"), _f32(table_a, "table_a"), _f32(table_b, "table_b"), _f32(w, "w")
        P, d = q.shape
        N = table_a.shape[0]
        if table_a.shape != table_b.shape or w.numel() != P:
            raise ValueError("l1_mix_scores: the two tables must have one shape and w one entry per row")
        ld = (N + 3) // 4 * 4
        out = torch.empty(P, ld, dtype=torch.float32, device=q.device)
        rc = self.lib.temp_l1_mix_scores(P, N, d, _ptr(q), _ptr(table_a), _ptr(table_b), _ptr(w), ld, _ptr(out), _stream())
        _lib.check(rc, "temp_l1_mix_scores")
        return out

    def gather_ce_mix_fwd(self, s_a, s_b, w, cand):
        """Candidate CE over the mixed scores w * s_a + (1 - w) * s_b (w [P]) -> (loss_rows, lse)."""
        s_a, s_b, w, cand = _f32(s_a, "s_a"), _f32(s_b, "s_b"), _f32(w, "w"), _i32(cand, "cand")
        P, N = s_a.shape
        loss = torch.empty(P, dtype=torch.float32, device=s_a.device)
        lse = torch.empty(P, dtype=torch.float32, device=s_a.device)
        rc = self.lib.temp_gather_ce_mix_fwd(P, cand.shape[1], N, _ptr(s_a), _ptr(s_b), _ptr(w), _ptr(cand), _ptr(loss), _ptr(lse), _stream())
        _lib.check(rc, "temp_gather_ce_mix_fwd")
        return loss, lse

    def gather_ce_mix_bwd(self, s_a, s_b, w, cand, lse, scale, inv_rows, row_scale=None):
        """-> (d_s_a, d_s_b, d_w) of the mixed candidate CE (include/temp_amd.h: temp_gather_ce_mix_bwd)."""
        s_a, s_b, w, cand, lse, scale = _f32(s_a, "s_a"), _f32(s_b, "s_b"), _f32(w, "w"), _i32(cand, "cand"), _f32(lse, "lse"), _f32(scale, "scale")
        row_scale = _f32(row_scale, "row_scale")
        P, N = s_a.shape
        d_a, d_b = torch.empty_like(s_a), torch.empty_like(s_b)
        d_w = torch.empty(P, dtype=torch.float32, device=s_a.device)
        rc = self.lib.temp_gather_ce_mix_bwd(P, cand.shape[1], N, _ptr(s_a), _ptr(s_b), _ptr(w), _ptr(cand), _ptr(lse), _ptr(scale), float(inv_rows),
                                             _ptr(row_scale), _ptr(d_a), _ptr(d_b), _ptr(d_w), _stream())
        _lib.check(rc, "temp_gather_ce_mix_bwd")
        return d_a, d_b, d_w

    def frozen_mix_ce(self, q_a, T_a, q_b, T_b, w, cand, row_scale=None, inv_rows=None, kind="dot"):
        """Candidate CE of two frozen streams mixed by w [P] (include/temp_amd.h: temp_frozen_mix_ce) -> (loss_rows [P] unscaled,
        d_w [P] scaled by row_scale[p], else by inv_rows (None: 1 / P)).  q_a [P, Da] / T_a [rows, Da] and q_b [P, Db] / T_b [rows, Db]
        may differ in width; cand [P, C] int32 holds rows of both tables, column 0 the truth.  kind "dot" | "l1".  One launch."""
        q_a, T_a, q_b, T_b, w = _f32(q_a, "q_a"), _f32(T_a, "T_a"), _f32(q_b, "q_b"), _f32(T_b, "T_b"), _f32(w, "w")
        cand, row_scale = _i32(cand, "cand"), _f32(row_scale, "row_scale")
        if kind not in _lib.FROZEN_KINDS:
            raise ValueError("frozen_mix_ce: kind must be 'dot' or 'l1'")
        P, Da = q_a.shape
        Db = q_b.shape[1]
        if (q_b.shape[0] != P or cand.dim() != 2 or cand.shape[0] != P or w.numel() != P or T_a.shape[1] != Da or T_b.shape[1] != Db
                or T_a.shape[0] != T_b.shape[0] or (row_scale is not None and row_scale.numel() != P)):
            raise ValueError("frozen_mix_ce: q_a / q_b / w / cand / row_scale must have one row per query, the tables one row count and "
                             "their query's width")
        loss = torch.empty(P, dtype=torch.float32, device=q_a.device)
        d_w = torch.empty(P, dtype=torch.float32, device=q_a.device)
        inv = 1.0 / max(P, 1) if inv_rows is None else float(inv_rows)
        rc = self.lib.temp_frozen_mix_ce(P, cand.shape[1], Da, Db, _lib.FROZEN_KINDS[kind], _ptr(q_a), _ptr(T_a), _ptr(q_b), _ptr(T_b), _ptr(w),
                                         _ptr(cand), _ptr(row_scale), inv, _ptr(loss), _ptr(d_w), _stream())
        _lib.check(rc, "temp_frozen_mix_ce")
        return loss, d_w

    def linear_tn(self, a, b, out=None):
        """a[M,Ka]^T . b[M,Nb] -> [Ka,Nb] (written into `out`, a contiguous (Ka, Nb) view, when given)."""
        a, b = _f32(a, "a"), _f32(b, "b")
        M, Ka = a.shape
        Nb = b.shape[1]
        if out is None:
            out = torch.empty(Ka, Nb, dtype=torch.float32, device=a.device)
        elif out.shape != (Ka, Nb) or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("linear_tn: out must be a contiguous float32 (Ka, Nb) matrix")
        ws = self._ws(self.lib.temp_linear_tn_workspace(M, Ka, Nb), a.device)
        rc = self.lib.temp_linear_tn(M, Ka, Nb, _ptr(a), Ka, _ptr(b), Nb, _ptr(out), Nb, _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_linear_tn")
        return out

    def linear_tn_multi(self, a_list, b_list, out_list):
        """out_i[Ka,Nb] = a_i[M_i,Ka]^T . b_i[M_i,Nb] for every problem i (contiguous (Ka, Nb) outputs): one launch for small M_i."""
        Ka, Nb = a_list[0].shape[1], b_list[0].shape[1]
        arr = (_lib.TempLinearProblem * len(a_list))()
        keep, max_m = [], 0
        for i, (a, b, o) in enumerate(zip(a_list, b_list, out_list)):
            a, b = _f32(a, "a"), _f32(b, "b")
            keep.append((a, b))
            if a.shape[1] != Ka or b.shape[1] != Nb or a.shape[0] != b.shape[0]:
                raise ValueError("linear_tn_multi: problems must share Ka and Nb")
            if o.shape != (Ka, Nb) or not o.is_contiguous() or o.dtype != torch.float32:
                raise ValueError("linear_tn_multi: outputs must be contiguous float32 (Ka, Nb) matrices")
            arr[i].M, arr[i].A, arr[i].B, arr[i].C = a.shape[0], a.data_ptr(), b.data_ptr(), o.data_ptr()
            max_m = max(max_m, a.shape[0])
        ws = self._ws(self.lib.temp_linear_tn_multi_workspace(len(a_list), max_m, Ka, Nb), a_list[0].device)
        rc = self.lib.temp_linear_tn_multi(len(a_list), arr, Ka, Nb, Ka, Nb, Nb, _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "temp_linear_tn_multi")
        return out_list

    def gather_ce_fwd(self, scores, cand):
        scores, cand = _f32(scores, "scores"), _i32(cand, "cand")
        P, N = scores.shape
        loss = torch.empty(P, dtype=torch.float32, device=scores.device)
        lse = torch.empty(P, dtype=torch.float32, device=scores.device)
        rc = self.lib.temp_gather_ce_fwd(P, cand.shape[1], N, _ptr(scores), _ptr(cand), _ptr(loss), _ptr(lse), _stream())
        _lib.check(rc, "temp_gather_ce_fwd")
        return loss, lse

    def gather_ce_bwd(self, scores, cand, lse, scale, inv_rows, row_scale=None):
        scores, cand, lse, scale = _f32(scores, "scores"), _i32(cand, "cand"), _f32(lse, "lse"), _f32(scale, "scale")
        row_scale = _f32(row_scale, "row_scale")
        P, N = scores.shape
        d = torch.empty_like(scores)
        rc = self.lib.temp_gather_ce_bwd(P, cand.shape[1], N, _ptr(scores), _ptr(cand), _ptr(lse), _ptr(scale), float(inv_rows), _ptr(row_scale),
                                         _ptr(d), _stream())
        _lib.check(rc, "temp_gather_ce_bwd")
        return d

    @staticmethod
    def _filtered_ce_args(what, scores, truth, lo, hi, ids, n):
        """The checks both all-entity CE entry points share -> (scores, P, n, ld, truth, lo, hi, ids)."""
        scores, truth = _f32(scores, "scores"), _i32(truth, "truth")
        if scores.dim() != 2 or truth.shape[0] != scores.shape[0]:
            raise ValueError("%s: scores must be [P, ld] with one truth per row" % what)
        P, ld = scores.shape
        n = ld if n is None else int(n)
        if not 0 < n <= ld:
            raise ValueError("%s: n must lie in (0, row length]" % what)
        if ld % 4:
            raise ValueError("%s: the score row length must be a multiple of 4" % what)
        if (lo is None) != (hi is None):
            raise ValueError("%s: lo and hi come together" % what)
        if lo is not None:
            lo, hi, ids = _i32(lo, "lo"), _i32(hi, "hi"), _i32(ids, "ids")
            if lo.shape[0] != P or hi.shape[0] != P:
                raise ValueError("%s: lo / hi must have one entry per row" % what)
        return scores, P, n, ld, truth, lo, hi, (ids if lo is not None else None)

    def filtered_ce_fwd(self, scores, truth, lo=None, hi=None, ids=None, col0=0, n=None, carry=None):
        """All-entity cross-entropy of the rows of scores [P, ld] under each row's known-true filter (include/temp_amd.h:
        temp_filtered_ce_fwd) -> (loss_rows [P] unscaled, lse_rows [P], state).  Column j < n (default: every column) is entity
        col0 + j.  `carry` = the state an earlier call returned over OTHER entities: the result is then that of both ranges; the
        state is updated in place and returned again."""
        scores, P, n, ld, truth, lo, hi, ids = self._filtered_ce_args("filtered_ce_fwd", scores, truth, lo, hi, ids, n)
        state = carry if carry is not None else torch.empty(3, P, dtype=torch.float32, device=scores.device)
        if state.shape != (3, P) or state.dtype != torch.float32 or not state.is_contiguous() or state.device != scores.device:
            raise ValueError("filtered_ce_fwd: carry must be the state of an earlier call over the same rows")
        out = torch.empty(2, P, dtype=torch.float32, device=scores.device)
        rc = self.lib.temp_filtered_ce_fwd(P, n, ld, int(col0), _ptr(scores), _ptr(truth), _ptr(lo), _ptr(hi), _ptr(ids), int(carry is not None),
                                           _ptr(state[0]), _ptr(state[1]), _ptr(state[2]), _ptr(out[1]), _ptr(out[0]), _stream())
        _lib.check(rc, "temp_filtered_ce_fwd")
        return out[0], out[1], state

    def filtered_ce_bwd(self, scores, truth, lo, hi, ids, lse, scale, inv_rows, row_scale=None, col0=0, n=None, out=None):
        """-> d_scores [P, ld] of the all-entity cross-entropy (include/temp_amd.h: temp_filtered_ce_bwd), fully written: 0 at the
        filtered columns and at the pad columns n <= j < ld.  `out`: a contiguous [P, ld] buffer to write instead of a new one."""
        scores, P, n, ld, truth, lo, hi, ids = self._filtered_ce_args("filtered_ce_bwd", scores, truth, lo, hi, ids, n)
        lse, scale, row_scale = _f32(lse, "lse"), _f32(scale, "scale"), _f32(row_scale, "row_scale")
        if lse.shape[0] != P or (row_scale is not None and row_scale.shape[0] != P):
            raise ValueError("filtered_ce_bwd: lse and row_scale must have one entry per row")
        d = torch.empty_like(scores) if out is None else out
        if d.shape != scores.shape or not d.is_contiguous() or d.dtype != torch.float32 or d.device != scores.device:
            raise ValueError("filtered_ce_bwd: out must be a contiguous float32 matrix of the shape of scores")
        rc = self.lib.temp_filtered_ce_bwd(P, n, ld, int(col0), _ptr(scores), _ptr(truth), _ptr(lo), _ptr(hi), _ptr(ids), _ptr(lse), _ptr(scale),
                                           float(inv_rows), _ptr(row_scale), _ptr(d), _stream())
        _lib.check(rc, "temp_filtered_ce_bwd")
        return d

    def assemble_views(self, piece_desc, piece_start, descs, table, out):
        """One launch of temp_assemble_views; all arguments are device tensors (descs: raw bytes of TempCopyDesc records)."""
        rc = self.lib.temp_assemble_views(int(piece_desc.shape[0]), _ptr(piece_desc), _ptr(piece_start), _ptr(descs), _ptr(table), _ptr(out), _stream())
        _lib.check(rc, "temp_assemble_views")
        return out

    def corrupt_sample(self, seed, truth, lo, hi, ids, K, N):
        """(R, 1+K) int32 candidate lists: column 0 = truth, the rest filtered uniform draws (see temp_corrupt_sample)."""
        truth = _i32(truth, "truth")
        R = truth.shape[0]
        cand = torch.empty(R, K + 1, dtype=torch.int32, device=truth.device)
        if lo is not None:
            lo, hi, ids = _i32(lo, "lo"), _i32(hi, "hi"), _i32(ids, "ids")
        rc = self.lib.temp_corrupt_sample(R, int(K), int(N), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(truth), _ptr(lo), _ptr(hi), _ptr(ids) if lo is not None else None,
                                          _ptr(cand), _stream())
        _lib.check(rc, "temp_corrupt_sample")
        return cand

    def filtered_rank(self, scores, target, filt_ptr=None, filt_ids=None):
        """1-indexed filtered ranks (int64) of `target` in every row of scores [P,N] (see temp_filtered_rank)."""
        scores, target = _f32(scores, "scores"), _i32(target, "target")
        P, N = scores.shape
        if N % 4:
            raise ValueError("filtered_rank: the score row length must be a multiple of 4")
        ranks = torch.empty(P, dtype=torch.int32, device=scores.device)
        if filt_ptr is not None:
            filt_ptr, filt_ids = _i32(filt_ptr, "filt_ptr"), _i32(filt_ids, "filt_ids")
        rc = self.lib.temp_filtered_rank(P, N, N, _ptr(scores), _ptr(target), _ptr(filt_ptr), _ptr(filt_ids), _ptr(ranks), _stream())
        _lib.check(rc, "temp_filtered_rank")
        return ranks.long()

    @staticmethod
    def _rank_stream_args(what, scores, target, filt_ptr, filt_ids, mode, col0, n, carry):
        """The checks and buffers both streamed-rank entry points share -> (scores, P, n, ld, target, filt_ptr, filt_ids, carry,
        ranks).  carry = (target_score [P] float32, count [P] int32): made here by a TEMP_RANK_COLLECT call without one, demanded by
        the counting modes, written in place by the kernel."""
        if scores.dim() != 2 or not scores.is_cuda or scores.dtype != torch.float32:
            raise _lib.TempAmdError("%s: scores must be a float32 [P, ld] GPU matrix" % what)
        scores, target = scores.detach(), _i32(target, "target")
        P, width = scores.shape
        n = width if n is None else int(n)
        ld = scores.stride(0) if P > 1 else max(scores.stride(0), width)
        if scores.stride(1) != 1 and width > 1:
            raise ValueError("%s: the score rows must be contiguous" % what)
        if mode not in (_lib.RANK_WHOLE, _lib.RANK_COLLECT, _lib.RANK_COUNT_FIRST, _lib.RANK_COUNT_ADD):
            raise ValueError("%s: mode must be one of the four TEMP_RANK_* modes" % what)
        if not 0 < n <= width or col0 < 0:
            raise ValueError("%s: n must lie in (0, row length] and col0 must not be negative" % what)
        if ld % 4 or scores.data_ptr() % 16:
            raise ValueError("%s: the row stride must be a multiple of 4 and the first score 16-byte aligned" % what)
        if target.shape[0] != P:
            raise ValueError("%s: target must have one entry per row" % what)
        if filt_ptr is not None:
            filt_ptr, filt_ids = _i32(filt_ptr, "filt_ptr"), _i32(filt_ids, "filt_ids")
            if filt_ptr.shape[0] != P + 1:
                raise ValueError("%s: filt_ptr must have one entry per row plus one" % what)
        if mode == _lib.RANK_WHOLE:
            carry = None
        elif carry is None:
            if mode != _lib.RANK_COLLECT:
                raise ValueError("%s: the counting modes need the carry of the TEMP_RANK_COLLECT sweep" % what)
            carry = (torch.zeros(P, dtype=torch.float32, device=scores.device), torch.zeros(P, dtype=torch.int32, device=scores.device))
        else:
            ts, cnt = carry
            if ts.shape != (P,) or cnt.shape != (P,) or ts.dtype != torch.float32 or cnt.dtype != torch.int32 or ts.device != scores.device \
                    or cnt.device != scores.device or not ts.is_contiguous() or not cnt.is_contiguous():
                raise ValueError("%s: carry must be the (target_score, count) of an earlier call over the same rows" % what)
        ranks = None if mode == _lib.RANK_COLLECT else torch.empty(P, dtype=torch.int32, device=scores.device)
        return scores, P, n, ld, target, filt_ptr, filt_ids, carry, ranks

    def filtered_rank_stream(self, scores, target, filt_ptr=None, filt_ids=None, mode=_lib.RANK_WHOLE, col0=0, n=None, carry=None):
        """The filtered rank on a column panel (see temp_filtered_rank_stream) -> (ranks [P] int64 | None, carry).  Column j < n
        (default: every column) of scores [P, ld] is entity col0 + j; `scores` may be a column slice of a wider row-major matrix (row
        stride % 4 == 0, first element 16-byte aligned).  mode RANK_WHOLE: the panel holds every target -> (ranks, None).
        RANK_COLLECT: the targets' scores go into the carry -> (None, carry), allocated when none is given.  RANK_COUNT_FIRST /
        RANK_COUNT_ADD: the panel's count is written / added to the carry -> (the ranks so far, carry).  The carry is updated in
        place and handed back."""
        what = "filtered_rank_stream"
        scores, P, n, ld, target, filt_ptr, filt_ids, carry, ranks = self._rank_stream_args(what, scores, target, filt_ptr, filt_ids, mode, col0, n, carry)
        ts, cnt = carry if carry is not None else (None, None)
        rc = self.lib.temp_filtered_rank_stream(P, n, ld, int(col0), _ptr(scores), _ptr(target), _ptr(filt_ptr), _ptr(filt_ids), int(mode), _ptr(ts),
                                                _ptr(cnt), _ptr(ranks), _stream())
        _lib.check(rc, "temp_filtered_rank_stream")
        return (None if ranks is None else ranks.long()), carry

    def filtered_rank_stream_mix(self, scores_a, scores_b, w, target, filt_ptr=None, filt_ids=None, mode=_lib.RANK_WHOLE, col0=0, n=None,
                                 carry=None):
        """filtered_rank_stream over the rows w[p] * scores_a[p] + (1 - w[p]) * scores_b[p], formed inside the kernel (see
        temp_filtered_rank_stream_mix).  The two matrices have equal shapes and strides, w has one entry per row; the carry holds the
        targets' MIXED scores."""
        what = "filtered_rank_stream_mix"
        if not torch.is_tensor(scores_b) or scores_b.dim() != 2 or not scores_b.is_cuda or scores_b.dtype != torch.float32:
            raise _lib.TempAmdError("%s: scores_b must be a float32 [P, ld] GPU matrix" % what)
        scores_a, P, n, ld, target, filt_ptr, filt_ids, carry, ranks = self._rank_stream_args(what, scores_a, target, filt_ptr, filt_ids, mode, col0, n,
                                                                                             carry)
        scores_b = scores_b.detach()
        if scores_b.shape != scores_a.shape or scores_b.stride() != scores_a.stride() or scores_b.device != scores_a.device:
            raise ValueError("%s: the two score matrices must have equal shapes and strides" % what)
        if scores_b.data_ptr() % 16:
            raise ValueError("%s: the first score of scores_b must be 16-byte aligned" % what)
        if w is None:
            raise ValueError("%s: w must have one entry per row" % what)
        w = _f32(w.detach().reshape(-1), "w")
        if w.shape[0] != P or w.device != scores_a.device:
            raise ValueError("%s: w must have one entry per row" % what)
        ts, cnt = carry if carry is not None else (None, None)
        rc = self.lib.temp_filtered_rank_stream_mix(P, n, ld, int(col0), _ptr(scores_a), _ptr(scores_b), _ptr(w), _ptr(target), _ptr(filt_ptr),
                                                    _ptr(filt_ids), int(mode), _ptr(ts), _ptr(cnt), _ptr(ranks), _stream())
        _lib.check(rc, "temp_filtered_rank_stream_mix")
        return (None if ranks is None else ranks.long()), carry

    @staticmethod
    def _topk_args(what, scores, k, filt_ptr, filt_ids, keep, col0, n, carry):
        """The checks and output buffers both selection entry points share -> (scores, P, n, ld, filt_ptr, filt_ids, keep, top_val,
        top_idx)."""
        if scores.dim() != 2 or not scores.is_cuda or scores.dtype != torch.float32:
            raise _lib.TempAmdError("%s: scores must be a float32 [P, ld] GPU matrix" % what)
        scores = scores.detach()
        P, width = scores.shape
        n = width if n is None else int(n)
        ld = scores.stride(0) if P > 1 else max(scores.stride(0), width)
        if scores.stride(1) != 1 and width > 1:
            raise ValueError("%s: the score rows must be contiguous" % what)
        if not 1 <= k <= _lib.TOPK_MAX:
            raise ValueError("%s: k must lie in [1, %d]" % (what, _lib.TOPK_MAX))
        if not 0 < n <= width or col0 < 0:
            raise ValueError("%s: n must lie in (0, row length] and col0 must not be negative" % what)
        if ld % 4 or scores.data_ptr() % 16:
            raise ValueError("%s: the row stride must be a multiple of 4 and the first score 16-byte aligned" % what)
        if filt_ptr is not None:
            filt_ptr, filt_ids = _i32(filt_ptr, "filt_ptr"), _i32(filt_ids, "filt_ids")
            if filt_ptr.shape[0] != P + 1:
                raise ValueError("%s: filt_ptr must have one entry per row plus one" % what)
        keep = _i32(keep, "keep")
        if keep is not None and keep.shape[0] != P:
            raise ValueError("%s: keep must have one entry per row" % what)
        if carry is None:
            top_val = torch.empty(P, k, dtype=torch.float32, device=scores.device)
            top_idx = torch.empty(P, k, dtype=torch.int32, device=scores.device)
        else:
            top_val, top_idx = _f32(carry[0], "carry values").clone(), carry[1].to(dtype=torch.int32, copy=True).contiguous()
            if top_val.shape != (P, k) or top_idx.shape != (P, k):
                raise ValueError("%s: carry must be the (top_val, top_idx) [P, k] of an earlier call" % what)
        return scores, P, n, ld, filt_ptr, filt_ids, keep, top_val, top_idx

    def filtered_topk(self, scores, k, filt_ptr=None, filt_ids=None, keep=None, col0=0, n=None, carry=None):
        """-> (top_val [P, k] float32, top_idx [P, k] int64): the best k admissible entities of every row of scores [P, ld] (see
        temp_filtered_topk).  Column j < n (default: every column) is entity col0 + j.  `scores` may be a column slice of a wider
        row-major matrix (row stride % 4 == 0, first element 16-byte aligned).  `carry` = the pair an earlier call returned over
        other entities: the result is then the selection over both ranges."""
        scores, P, n, ld, filt_ptr, filt_ids, keep, top_val, top_idx = self._topk_args("filtered_topk", scores, k, filt_ptr, filt_ids, keep,
                                                                                       col0, n, carry)
        rc = self.lib.temp_filtered_topk(P, n, ld, int(k), int(col0), _ptr(scores), _ptr(filt_ptr), _ptr(filt_ids), _ptr(keep),
                                         int(carry is not None), _ptr(top_val), _ptr(top_idx), _stream())
        _lib.check(rc, "temp_filtered_topk")
        return top_val, top_idx.long()

    def filtered_topk_mix(self, scores_a, scores_b, w, k, filt_ptr=None, filt_ids=None, keep=None, col0=0, n=None, carry=None):
        """filtered_topk over the rows w[p] * scores_a[p] + (1 - w[p]) * scores_b[p], formed inside the kernel (see
        temp_filtered_topk_mix): an entity whose score is -inf in EITHER matrix is inadmissible whatever w is.  The two matrices have
        equal shapes and strides (column slices of two equally wide matrices qualify), w has one entry per row; `carry` may come from
        either entry point."""
        what = "filtered_topk_mix"
        if not torch.is_tensor(scores_b) or scores_b.dim() != 2 or not scores_b.is_cuda or scores_b.dtype != torch.float32:
            raise _lib.TempAmdError("%s: scores_b must be a float32 [P, ld] GPU matrix" % what)
        scores_a, P, n, ld, filt_ptr, filt_ids, keep, top_val, top_idx = self._topk_args(what, scores_a, k, filt_ptr, filt_ids, keep, col0, n, carry)
        scores_b = scores_b.detach()
        if scores_b.shape != scores_a.shape or scores_b.stride() != scores_a.stride() or scores_b.device != scores_a.device:
            raise ValueError("%s: the two score matrices must have equal shapes and strides" % what)
        if scores_b.data_ptr() % 16:
            raise ValueError("%s: the first score of scores_b must be 16-byte aligned" % what)
        if w is None:
            raise ValueError("%s: w must have one entry per row" % what)
        w = _f32(w.detach().reshape(-1), "w")
        if w.shape[0] != P or w.device != scores_a.device:
            raise ValueError("%s: w must have one entry per row" % what)
        rc = self.lib.temp_filtered_topk_mix(P, n, ld, int(k), int(col0), _ptr(scores_a), _ptr(scores_b), _ptr(w), _ptr(filt_ptr), _ptr(filt_ids),
                                             _ptr(keep), int(carry is not None), _ptr(top_val), _ptr(top_idx), _stream())
        _lib.check(rc, "temp_filtered_topk_mix")
        return top_val, top_idx.long()

    # ---- optimizer (clipped Adam over a device table of tensors) ----------------------------------------------
    @staticmethod
    def _adam_table(table, n_tensors, n_chunks, what):
        if not torch.is_tensor(table) or not table.is_cuda or table.dtype != torch.uint8 or not table.is_contiguous():
            raise _lib.TempAmdError("%s: the table must be a contiguous uint8 GPU tensor of TempAdamTensor records" % what)
        if n_tensors < 0 or n_chunks < 0 or (n_chunks > 0 and n_tensors == 0):
            raise ValueError("%s: tensor and chunk counts must not be negative, and chunks need tensors" % what)
        if table.numel() < n_tensors * ctypes.sizeof(_lib.TempAdamTensor) or table.data_ptr() % 8:
            raise ValueError("%s: the table must hold one 72-byte record per tensor at an 8-byte aligned address" % what)

    def grad_norm_workspace(self, n_chunks):
        return int(self.lib.temp_grad_norm_workspace(int(n_chunks)))

    def grad_norm_clip(self, table, n_tensors, n_chunks, max_norm, ws, norm_coef):
        """norm_coef[0:2] (float32, device) = (sqrt(sum g^2) over the table's tensors, the clip coefficient for max_norm) -- see
        temp_grad_norm_clip.  table: uint8 device tensor of TempAdamTensor records (one per tensor, chunks numbered in row order),
        ws: uint8 device workspace of grad_norm_workspace(n_chunks) bytes.  Nothing is allocated and nothing waits."""
        n_tensors, n_chunks = int(n_tensors), int(n_chunks)
        self._adam_table(table, n_tensors, n_chunks, "grad_norm_clip")
        if not torch.is_tensor(norm_coef) or not norm_coef.is_cuda or norm_coef.dtype != torch.float32 or norm_coef.numel() < 2 \
                or not norm_coef.is_contiguous():
            raise _lib.TempAmdError("grad_norm_clip: norm_coef must be a contiguous float32 GPU tensor of two elements")
        if not torch.is_tensor(ws) or not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < self.grad_norm_workspace(n_chunks):
            raise ValueError("grad_norm_clip: the workspace must be a uint8 GPU tensor of grad_norm_workspace(n_chunks) bytes")
        if not float(max_norm) > 0.0:
            raise ValueError("grad_norm_clip: max_norm must be positive")
        rc = self.lib.temp_grad_norm_clip(n_tensors, n_chunks, _ptr(table), float(max_norm), _ptr(ws), ws.numel(), _ptr(norm_coef), _stream())
        _lib.check(rc, "temp_grad_norm_clip")
        return norm_coef

    def adam_clip_step(self, table, n_tensors, n_chunks, norm_coef=None):
        """One in-place Adam step of every tensor of the table, the gradients scaled by norm_coef[1] (None: not scaled) -- see
        temp_adam_clip_step."""
        n_tensors, n_chunks = int(n_tensors), int(n_chunks)
        self._adam_table(table, n_tensors, n_chunks, "adam_clip_step")
        if norm_coef is not None and (not norm_coef.is_cuda or norm_coef.dtype != torch.float32 or norm_coef.numel() < 2
                                      or not norm_coef.is_contiguous()):
            raise _lib.TempAmdError("adam_clip_step: norm_coef must be a contiguous float32 GPU tensor of two elements")
        rc = self.lib.temp_adam_clip_step(n_tensors, n_chunks, _ptr(table), _ptr(norm_coef), _stream())
        _lib.check(rc, "temp_adam_clip_step")

    # ---- history attention (self-attention encoder) ------------------------------------------------------
    def _attn_desc(self, qkv, kv_hist, idx, decay):
        n, D3 = qkv.shape
        D = D3 // 3
        T = idx.shape[1] + 1
        if T > 1 and kv_hist.shape[1] != 2 * D:
            raise _lib.TempAmdError("kv_hist must be [R, 2D]")
        a = _lib.TempAttn()
        a.n, a.D, a.heads, a.T = n, D, 8, T
        base = qkv.data_ptr()
        a.q, a.ldq = base, D3
        a.kc, a.vc, a.ldc = base + 4 * D, base + 8 * D, D3
        if T > 1:
            hb = kv_hist.data_ptr()
            a.kh, a.vh, a.ldh = hb, hb + 4 * D, 2 * D
        a.idx = idx.data_ptr() if T > 1 else None
        a.decay = decay.data_ptr() if decay is not None else None
        return a, n, D, T

    def sa_attn_fwd(self, qkv, kv_hist, idx, decay):
        """qkv [n,3D] = (q | k | v) of the query rows; kv_hist [R,2D] = (k | v) history table;
        idx [n,T-1] int32 rows of the table (-1 masked); decay [T] or None -> (out, score, lse)."""
        qkv, kv_hist, idx, decay = _f32(qkv, "qkv"), _f32(kv_hist, "kv_hist"), _i32(idx, "idx"), _f32(decay, "decay")
        a, n, D, T = self._attn_desc(qkv, kv_hist, idx, decay)
        out = torch.empty(n, D, dtype=torch.float32, device=qkv.device)
        score = torch.empty(n, 8, T, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(n, 8, dtype=torch.float32, device=qkv.device)
        rc = self.lib.temp_sa_attn_fwd(ctypes.byref(a), _ptr(out), _ptr(score), _ptr(lse), _stream())
        _lib.check(rc, "temp_sa_attn_fwd")
        return out, score, lse

    def sa_attn_bwd(self, qkv, kv_hist, idx, decay, out, score, lse, d_out, inverse=None):
        """-> (d_qkv [n,3D], d_kv_hist [R,2D], d_decay [T] or None).  `inverse` = (inv_ptr, inv_ref) of idx grouped by
        table row selects the deterministic two-pass form (no atomics)."""
        qkv, kv_hist, idx, decay = _f32(qkv, "qkv"), _f32(kv_hist, "kv_hist"), _i32(idx, "idx"), _f32(decay, "decay")
        d_out = _f32(d_out, "d_out")
        a, n, D, T = self._attn_desc(qkv, kv_hist, idx, decay)
        d_qkv = torch.empty_like(qkv)
        use_inv = inverse is not None and T > 1
        d_hist = torch.empty_like(kv_hist) if use_inv else torch.zeros_like(kv_hist)
        d_decay = torch.zeros(T, dtype=torch.float32, device=qkv.device) if decay is not None else None
        db, dh = d_qkv.data_ptr(), d_hist.data_ptr()
        vp = ctypes.c_void_p
        inv_ptr = inv_ref = ds_ws = None
        if use_inv:
            inv_ptr, inv_ref = _i32(inverse[0], "inv_ptr"), _i32(inverse[1], "inv_ref")
            ds_ws = torch.empty(n * 8 * T, dtype=torch.float32, device=qkv.device)
        rc = self.lib.temp_sa_attn_bwd(ctypes.byref(a), _ptr(out), _ptr(score), _ptr(lse), _ptr(d_out),
                                       vp(db), 3 * D, vp(dh), vp(dh + 4 * D), 2 * D, vp(db + 4 * D), vp(db + 8 * D), 3 * D,
                                       _ptr(d_decay), kv_hist.shape[0], _ptr(inv_ptr), _ptr(inv_ref), _ptr(ds_ws), _stream())
        _lib.check(rc, "temp_sa_attn_bwd")
        return d_qkv, d_hist, d_decay

    def _attn_split_desc(self, pa, ia, pb, ib, kv_hist, idx, decay):
        """(TempAttn of the history side, TempAttnSplit, n, D, T): row i's (q | k | v) = pa[ia[i]] + pb[ib[i]]."""
        n, D3 = ia.shape[0], pa.shape[1]
        D = D3 // 3
        T = idx.shape[1] + 1
        if pb.shape[1] != D3 or D3 != 3 * D or ib.shape[0] != n or idx.shape[0] != n:
            raise _lib.TempAmdError("split attention: pa / pb must be [*, 3D] and ia / ib / idx must list the same n rows")
        if n > 0 and (pa.shape[0] == 0 or pb.shape[0] == 0):
            raise _lib.TempAmdError("split attention: empty pa / pb table")
        if T > 1 and kv_hist.shape[1] != 2 * D:
            raise _lib.TempAmdError("kv_hist must be [R, 2D]")
        a = _lib.TempAttn()
        a.n, a.D, a.heads, a.T = n, D, 8, T
        if T > 1:
            hb = kv_hist.data_ptr()
            a.kh, a.vh, a.ldh = hb, hb + 4 * D, 2 * D
        a.idx = idx.data_ptr() if T > 1 else None
        a.decay = decay.data_ptr() if decay is not None else None
        sp = _lib.TempAttnSplit()
        sp.pa, sp.ia, sp.lda = pa.data_ptr(), ia.data_ptr(), D3
        sp.pb, sp.ib, sp.ldb = pb.data_ptr(), ib.data_ptr(), D3
        return a, sp, n, D, T

    def sa_attn_split_fwd(self, pa, ia, pb, ib, kv_hist, idx, decay):
        """sa_attn_fwd with the current rows given in two parts: pa [Na,3D], pb [Nb,3D] = (q | k | v) projections of two small
        tables, ia / ib [n] int32 their rows; row i attends as pa[ia[i]] + pb[ib[i]] (formed in the kernel) -> (out, score, lse)."""
        pa, pb, kv_hist, decay = _f32(pa, "pa"), _f32(pb, "pb"), _f32(kv_hist, "kv_hist"), _f32(decay, "decay")
        ia, ib, idx = _i32(ia, "ia"), _i32(ib, "ib"), _i32(idx, "idx")
        a, sp, n, D, T = self._attn_split_desc(pa, ia, pb, ib, kv_hist, idx, decay)
        out = torch.empty(n, D, dtype=torch.float32, device=pa.device)
        score = torch.empty(n, 8, T, dtype=torch.float32, device=pa.device)
        lse = torch.empty(n, 8, dtype=torch.float32, device=pa.device)
        rc = self.lib.temp_sa_attn_split_fwd(ctypes.byref(a), ctypes.byref(sp), _ptr(out), _ptr(score), _ptr(lse), _stream())
        _lib.check(rc, "temp_sa_attn_split_fwd")
        return out, score, lse

    def sa_attn_split_bwd(self, pa, ia, pb, ib, kv_hist, idx, decay, out, score, lse, d_out, inverse=None):
        """-> (d_qkv [n,3D] = gradient of the SUMMED current rows, d_kv_hist [R,2D], d_decay [T] or None); `inverse` as in
        sa_attn_bwd.  The caller sums d_qkv over ia / ib for d_pa / d_pb (segment_sum_rows)."""
        pa, pb, kv_hist, decay = _f32(pa, "pa"), _f32(pb, "pb"), _f32(kv_hist, "kv_hist"), _f32(decay, "decay")
        ia, ib, idx, d_out = _i32(ia, "ia"), _i32(ib, "ib"), _i32(idx, "idx"), _f32(d_out, "d_out")
        a, sp, n, D, T = self._attn_split_desc(pa, ia, pb, ib, kv_hist, idx, decay)
        d_qkv = torch.empty(n, 3 * D, dtype=torch.float32, device=pa.device)
        use_inv = inverse is not None and T > 1
        d_hist = torch.empty_like(kv_hist) if use_inv else torch.zeros_like(kv_hist)
        d_decay = torch.zeros(T, dtype=torch.float32, device=pa.device) if decay is not None else None
        dh = d_hist.data_ptr()
        vp = ctypes.c_void_p
        inv_ptr = inv_ref = ds_ws = None
        if use_inv:
            inv_ptr, inv_ref = _i32(inverse[0], "inv_ptr"), _i32(inverse[1], "inv_ref")
            ds_ws = torch.empty(n * 8 * T, dtype=torch.float32, device=pa.device)
        rc = self.lib.temp_sa_attn_split_bwd(ctypes.byref(a), ctypes.byref(sp), _ptr(out), _ptr(score), _ptr(lse), _ptr(d_out),
                                             _ptr(d_qkv), 3 * D, vp(dh), vp(dh + 4 * D), 2 * D, _ptr(d_decay), kv_hist.shape[0],
                                             _ptr(inv_ptr), _ptr(inv_ref), _ptr(ds_ws), _stream())
        _lib.check(rc, "temp_sa_attn_split_bwd")
        return d_qkv, d_hist, d_decay

    # ---- row gather / scatter ---------------------------------------------------------------------
    def gather_rows(self, table, idx):
        table, idx = _f32(table, "table"), _i32(idx, "idx")
        out = torch.empty(idx.shape[0], table.shape[1], dtype=torch.float32, device=table.device)
        rc = self.lib.temp_gather_rows(idx.shape[0], table.shape[1], _ptr(table), _ptr(idx), _ptr(out), _stream())
        _lib.check(rc, "temp_gather_rows")
        return out

    def gather_rows_keys(self, table, idx):
        """gather_rows that also returns the magnitude keys of its output: (out, row_keys int32 [n], col_keys int32 [d])."""
        table, idx = _f32(table, "table"), _i32(idx, "idx")
        n, d = idx.shape[0], table.shape[1]
        out = torch.empty(n, d, dtype=torch.float32, device=table.device)
        rk = torch.empty(n, dtype=torch.int32, device=table.device)
        ck = torch.empty(self.lib.temp_keys_cols_size(d), dtype=torch.int32, device=table.device)
        rc = self.lib.temp_gather_rows_keys(n, d, _ptr(table), _ptr(idx), _ptr(out), _ptr(rk), _ptr(ck), _stream())
        _lib.check(rc, "temp_gather_rows_keys")
        return out, rk, ck[:d]

    def keys_supported(self, d):
        """True when row / column keys of a width-d matrix are of use (f16 arithmetic on, width taken by the key kernels)."""
        return d % 4 == 0 and d <= 256 and self.lib.temp_get_option(_lib.OPT_MFMA_F16X2) != 0 and self.lib.temp_get_option(_lib.OPT_MFMA_BF16X3) != 0

    def scatter_add_rows(self, src, idx, table):
        """table[idx[i]] += src[i] in place (table must be contiguous float32)."""
        src, idx = _f32(src, "src"), _i32(idx, "idx")
        if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()):
            raise _lib.TempAmdError("scatter target must be a contiguous float32 GPU tensor")
        rc = self.lib.temp_scatter_add_rows(idx.shape[0], src.shape[1], _ptr(src), _ptr(idx), _ptr(table), _stream())
        _lib.check(rc, "temp_scatter_add_rows")
        return table

    def segment_sum_rows(self, src, seg_ptr, order, n_seg, relu_of=None):
        """out[s] = sum of src[order[seg_ptr[s]:seg_ptr[s+1]]] (deterministic adjoint of a static gather); with relu_of
        [n_seg, d] (the post-ReLU table the gather read): zero where relu_of <= 0 (that ReLU's adjoint, same kernel)."""
        src, seg_ptr, order = _f32(src, "src"), _i32(seg_ptr, "seg_ptr"), _i32(order, "order")
        if src.shape[0] == 0 or order.shape[0] == 0:
            return torch.zeros(n_seg, src.shape[1], dtype=torch.float32, device=src.device)
        out = torch.empty(n_seg, src.shape[1], dtype=torch.float32, device=src.device)
        nb = self.lib.temp_segment_sum_rows_workspace(n_seg, order.shape[0], src.shape[1])
        ws = self._ws(nb, src.device) if nb else None
        if relu_of is not None:
            relu_of = _f32(relu_of, "relu_of")
            if tuple(relu_of.shape) != (n_seg, src.shape[1]):
                raise _lib.TempAmdError("relu_of must be [n_seg, d]")
            rc = self.lib.temp_segment_sum_rows_relu(n_seg, order.shape[0], src.shape[1], _ptr(seg_ptr), _ptr(order), _ptr(src), _ptr(relu_of),
                                                     _ptr(out), _ptr(ws), nb, _stream())
        else:
            rc = self.lib.temp_segment_sum_rows(n_seg, order.shape[0], src.shape[1], _ptr(seg_ptr), _ptr(order), _ptr(src), _ptr(out),
                                                _ptr(ws), nb, _stream())
        _lib.check(rc, "temp_segment_sum_rows")
        return out

    def copy_probe(self, src, dst):
        rc = self.lib.temp_copy_probe(_ptr(src), _ptr(dst), src.numel() * src.element_size(), _stream())
        _lib.check(rc, "temp_copy_probe")
