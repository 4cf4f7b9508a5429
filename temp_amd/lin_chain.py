"""Window-batched LINEAR recurrence: one autograd node for the whole chain of window positions of --module RRGCN / BiRRGCN.

    h_p = act(x_p + (exp(-lam dt) h_{p-1}) . W)            (RRGCNLayer / BiRRGCNLayer, models/RRGCN.py:120-167, models/BiRRGCN.py:102-185)

With --rec-only-last-layer x_p (aggregation + self-loop of layer 2) is known for every position before the recurrence starts, so what
is sequential is one (n, d) x (d, d) product per position.  The programs, their panel tables and row maps are those of the GRU chain
(gru_chain.GruProgram, chain_tables, x_index: the `rnn` of an instance is the index of its weight here); the kernels are
temp_lin_chain_fwd / _bwd (one launch each for ALL positions).  The backward hands out d_pre, the gradient in front of the activation
of every row: it is d_x in chain order and the left factor of d_W_i = hdec_i^T . d_pre_i over weight i's row range (linear_tn).

The torch form -- a loop over the instances on gather_rows / decay_rows / linear_nt, each with its own autograd node -- runs on a
backend without the kernels (the CPU test backend), under CHAIN_KERNELS = False, and for a width or program the kernels refuse.
"""
import numpy as np
import torch

from . import functional as TF
from . import _lib
from . import gru_chain as GC
from .backend import get_backend


CHAIN_KERNELS = True        # A/B switch: False keeps the per-instance torch loop (linear_nt + decay_rows per position)


def lin_chain_usable(d, n_w=1, max_steps=0):
    """True when linear_chain() runs a program of this width (and longest panel) through the persistent chain kernels."""
    be = get_backend()
    return bool(CHAIN_KERNELS and n_w <= _lib.CHAIN_MAX_RNN and hasattr(be, "lin_chain_fwd") and be.lin_chain_supported(d, max_steps))


def _tables(prog, device, d, n_w, want):
    """The chain kernels' tables of this program and `want` set, or None: the torch loop runs."""
    if not lin_chain_usable(d, n_w):
        return None
    tabs = prog.chain_tables(device, want)
    return tabs if tabs is not None and lin_chain_usable(d, n_w, tabs["max_steps"]) else None


def prepare_linear_program(prog, device, d, n_w, want):
    """Host + upload half of a program, once per prepared batch: the panel tables and the x row table for the kernels (through
    gru_chain.prepare_program, as it is), else the row maps of every instance for the torch loop."""
    want = tuple(want) if want is not None else None
    if _tables(prog, device, d, n_w, want) is not None:
        GC.prepare_program(prog, device, d, n_w, want)
        prog.x_index(device)
        return
    prog.upload(device)


def _torch_chain(x_all, prog, weights, lam, act, want):
    """Instance by instance on the existing operators; the decay in front of the product, the order the kernels keep."""
    tens = prog.upload(x_all.device)
    H = []
    for i, it in enumerate(prog.inst):
        x = x_all[it.x0:it.x0 + it.n]
        if it.prev >= 0 and it.n > 0 and prog.inst[it.prev].n > 0:
            prev = TF.gather_rows(H[it.prev], tens[i][0])
            x = x + TF.linear_nt(TF.decay_rows(prev, tens[i][2], lam), weights[it.rnn])
        H.append(torch.relu(x) if act else x)
    if want is None:
        return torch.cat(H, dim=0) if H else x_all.new_zeros(0, x_all.shape[1])
    return tuple(H[i] for i in want)


class _LinChainFn(torch.autograd.Function):
    """The kernel route: tabs exist (decided by linear_chain).  Saves h (the ReLU mask is the kernel's own h > 0) and hdec."""

    @staticmethod
    def forward(ctx, x_all, prog, tabs, lam, act, want, *weights):
        be = get_backend()
        dev, d, N = x_all.device, x_all.shape[1], prog.n_total
        x_all = x_all.detach().contiguous()
        W = [w.detach().contiguous() for w in weights]
        packs = be.lin_chain_pack_multi(W)
        h, hdec = torch.empty(N, d, dtype=torch.float32, device=dev), torch.empty(N, d, dtype=torch.float32, device=dev)
        be.lin_chain_fwd(tabs, x_all, prog.x_index(dev), lam, packs, act, h, hdec)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, hdec, *packs)
        ctx.prog, ctx.tabs, ctx.lam, ctx.act, ctx.want, ctx.n_x, ctx.n_w = prog, tabs, lam, act, want, x_all.shape[0], len(W)
        if want is None:
            return h
        return tuple(h[prog.inst[i].h0:prog.inst[i].h0 + prog.inst[i].n] for i in want)

    @staticmethod
    def backward(ctx, *d_outs):
        be = get_backend()
        h, hdec = ctx.saved_tensors[:2]
        packs = list(ctx.saved_tensors[2:])
        prog, groups = ctx.prog, ctx.prog.groups
        N, d, dev = h.shape[0], h.shape[1], h.device
        if ctx.want is None:
            ups = [d_outs[0].contiguous() if d_outs[0] is not None else torch.zeros(N, d, dtype=torch.float32, device=dev)]
        else:
            given = {i: g.contiguous() for i, g in zip(ctx.want, d_outs) if g is not None}
            ups = [given.get(i) for i in ctx.want]
        d_pre = torch.empty(N, d, dtype=torch.float32, device=dev)
        be.lin_chain_bwd(ctx.tabs, h, ups, ctx.lam, packs, ctx.act, d_pre)
        # d_x: the adjoint of x_index.  A group is a run of instances with contiguous x and chain rows, so it is a block copy; where the
        # x rows ARE the chain rows nothing moves at all
        if ctx.n_x == N and all(g["x0"] == g["h0"] for g in groups):
            d_x_all = d_pre
        else:
            d_x_all = torch.empty(ctx.n_x, d, dtype=torch.float32, device=dev)
            written = np.zeros(ctx.n_x, dtype=bool)
            for g in groups:
                xs, hs = slice(g["x0"], g["x1"]), slice(g["h0"], g["h1"])
                first = not written[xs].any()
                assert first or written[xs].all()
                if first:
                    d_x_all[xs] = d_pre[hs]
                else:                                        # (groups that share x rows: a later one adds to the first one's)
                    d_x_all[xs] += d_pre[hs]
                written[xs] = True
            if not written.all():
                d_x_all[torch.from_numpy(~written).to(dev)] = 0
        # d_W_i = hdec_i^T . d_pre_i over the groups of weight i; a group whose rows all start from the zero state has hdec = 0
        live = [g for gi, g in enumerate(groups) if g["h1"] > g["h0"] and any(it.prev >= 0 for it in prog.inst if it.group == gi)]
        outs = [torch.empty(d, d, dtype=torch.float32, device=dev) for _ in live]
        if len(live) > 1 and hasattr(be, "linear_tn_multi"):
            be.linear_tn_multi([hdec[g["h0"]:g["h1"]] for g in live], [d_pre[g["h0"]:g["h1"]] for g in live], outs)
        else:
            for g, o in zip(live, outs):
                be.linear_tn(hdec[g["h0"]:g["h1"]], d_pre[g["h0"]:g["h1"]], out=o)
        grads = [None] * ctx.n_w
        for g, o in zip(live, outs):
            grads[g["rnn"]] = o if grads[g["rnn"]] is None else grads[g["rnn"]] + o
        grads = [g if g is not None else torch.zeros(d, d, dtype=torch.float32, device=dev) for g in grads]
        return (d_x_all, None, None, None, None, None) + tuple(grads)


def linear_chain(x_all, prog, weights, lam, act, want=None, table=None):
    """Run a GruProgram on linear cells: instance i computes act(x rows + decay(state of instance `prev`) . weights[it.rnn]).
    weights: the (in, out) `time_weight` matrices; act: 0 none, 1 ReLU; want: None -> H_all (prog.n_total, d), or a list of instance
    ids -> the states of just those instances (a tuple), as in gru_chain.  table: None, or (y, chain_rows, inverse, relu_table) with
    x_all = None: the x rows are y[chain_rows], gathered first (functional.gather_rows)."""
    if table is not None:
        assert x_all is None, "table=...: the x rows are the table's"
        y, chain_rows, y_inv, relu_table = table
        x_all = TF.gather_rows(y, chain_rows, y_inv, relu_table=relu_table)
    want = tuple(want) if want is not None else None
    weights, act = list(weights), int(bool(act))
    tabs = _tables(prog, x_all.device, x_all.shape[1], len(weights), want)
    if tabs is None:
        return _torch_chain(x_all, prog, weights, float(lam), act, want)
    return _LinChainFn.apply(x_all, prog, tabs, float(lam), act, want, *weights)
