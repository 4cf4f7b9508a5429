"""Window-batched GRU recurrence: one autograd node for the whole chain of window positions.

With --rec-only-last-layer the GRU input of every position is known before the recurrence starts
(models/RRGCN.py:182-187: layer 1 is a plain RGCNLayer), so the per-position work shrinks to what is
truly sequential -- hdec . W_hh^T + gates forward, gate gradients + d_prev backward -- and the
input-side GEMM, d_x, and all weight / bias gradients run once over all rows (temp_gru_input_gates,
temp_gru_weight_grads).  Previous states and their gradients move between positions through the
plan's row maps (`prev_idx` forward, its inverse `next_idx` backward), never through a dense
(bsz, N_ents, D) history (SURVEY F8 semantics kept: -1 => zero state).

A `GruProgram` is a small static DAG of *instances*; instance i applies GRU weights `rnn[i]` to
x rows [x0, x0+n) with previous state = output of instance `prev` (or none) and writes H rows
[h0, h0+n).  The bi-directional centre position is two instances over the same x rows whose
outputs the caller adds (models/BiRRGCN.py:45).
"""
import numpy as np
import torch

from . import _hostlib, _lib
from .backend import get_backend


CHAIN_KERNELS = True        # A/B switch: False keeps the per-position launches (temp_gru_cell_*_multi)
WEIGHT_GRADS_MULTI = True   # A/B switch: False computes each GRU's weight gradients with its own launches (temp_gru_weight_grads)
KEYED_GRADS = True          # A/B switch: False keeps the consumers of g4 on the six-product bf16 split (no keys from the chain backward)
GATE_GRADS_ONCE = True      # A/B switch: False keeps dgi + dgh as two matrices (temp_gru_chain_bwd + temp_gru_weight_grads_multi)
FUSED_INPUT_GATES = True    # A/B switch: False keeps the gate GEMM + gi route where temp_gru_chain_fwd's x route applies (so does TEMP_DEBUG bit 22)
ROWS_IN_PLACE = True        # A/B switch: False keeps the copy into chain order (gather_rows(keys=True)) where gru_chain(table=...) could read the rows in place


class GruInstance:
    __slots__ = ("n", "x0", "h0", "rnn", "prev", "next", "prev_idx", "next_idx", "dt", "group")

    def __init__(self, n, x0, rnn, prev, prev_idx_np, dt_np, next_idx_np=None):
        self.n, self.x0, self.rnn, self.prev = int(n), int(x0), rnn, prev
        self.h0 = 0
        self.next = -1
        self.prev_idx = prev_idx_np
        self.next_idx = next_idx_np      # inverse of the successor's prev_idx when the planner already has it
        self.dt = dt_np
        self.group = -1


class GruProgram:
    def __init__(self, instances):
        self.inst = instances
        off = 0
        for it in instances:
            it.h0 = off
            off += it.n
        self.n_total = off
        # inverse row maps: which row of the NEXT instance consumes each row of this one
        for i, it in enumerate(instances):
            if it.prev >= 0:
                p = instances[it.prev]
                assert p.next == -1, "an instance feeds at most one successor"
                p.next = i
                if p.next_idx is None:
                    inv = np.full(p.n, -1, dtype=np.int32)
                    ok = it.prev_idx >= 0
                    inv[it.prev_idx[ok]] = np.nonzero(ok)[0].astype(np.int32)
                    p.next_idx = inv
        # groups: maximal runs of instances with the same weights and contiguous x and h rows
        self.groups = []
        for i, it in enumerate(instances):
            g = self.groups[-1] if self.groups else None
            if g is not None and g["rnn"] == it.rnn and g["x1"] == it.x0 and g["h1"] == it.h0:
                g["x1"] += it.n
                g["h1"] += it.n
            else:
                self.groups.append(dict(rnn=it.rnn, x0=it.x0, x1=it.x0 + it.n, h0=it.h0, h1=it.h0 + it.n))
            it.group = len(self.groups) - 1
        # levels: instances at the same distance from their chain start are independent of each other
        # (forward-direction and backward-direction chains, the two centre cells) -> launched together
        depth = []
        for it in instances:
            depth.append(0 if it.prev < 0 else depth[it.prev] + 1)
        self.levels = []
        for lv in range(max(depth) + 1 if depth else 0):
            idx = [i for i, dp in enumerate(depth) if dp == lv and instances[i].n > 0]
            for k in range(0, len(idx), 4):
                self.levels.append(idx[k:k + 4])
        self.dev = None

    # ---- persistent chain kernels: panels of 32 entity tracks (include/temp_amd.h: TempGruChain) ------------------------
    def chain_plan(self):
        """Host half of the persistent-chain tables, independent of `want` and cached: every row of every instance gets a
        TRACK -- it inherits its predecessor's (prev_idx >= 0), otherwise takes the lowest track that no row of its instance
        inherits (a state survives exactly one position, so a track whose entity was absent is free again) -- and tracks are
        cut into panels of 32.  A panel's steps are the positions at which it has a row; a position where the whole panel is
        idle is dropped (none of its tracks can carry a state across it).
        -> None when the program is not a set of chains with one GRU each (the per-position kernels are used then), else
           dict(panel [P,4], rows [S,32], any_prev [S], step_inst [S])."""
        if getattr(self, "_chain_plan", False) is not False:
            return self._chain_plan
        self._chain_plan = self._chain_plan_host()
        return self._chain_plan

    def _chain_plan_host(self):
        """chain_plan in the C++ planner library (temp_host_chain_tracks); bit-identical to _chain_plan_numpy."""
        inst = self.inst
        if not any(it.prev >= 0 and it.n > 0 for it in inst):          # at least one real recurrence step
            return None
        chains = []
        for head, it0 in enumerate(inst):
            if it0.prev >= 0:
                continue
            chain = [head]
            while inst[chain[-1]].next >= 0:
                chain.append(inst[chain[-1]].next)
            chains.append(chain)
        res = _hostlib.chain_tracks(chains, [it.n for it in inst], [it.h0 for it in inst], [it.rnn for it in inst],
                                    [getattr(it, "prev_idx", None) if it.prev >= 0 else None for it in inst], _lib.CHAIN_TRACKS, _lib.CHAIN_MAX_STEPS)
        if res is None:
            return None
        panel, rows, anyp, sinst = res
        return dict(panel=panel, rows=rows, any_prev=anyp, step_inst=sinst)

    def _chain_plan_numpy(self):
        """The numpy formulation of chain_plan (kept as the cross-check of the planner library, tests/test_chain_cpu.py)."""
        inst = self.inst
        T = _lib.CHAIN_TRACKS
        panel, rows_tab, any_prev, step_inst = [], [], [], []
        s_base = 0
        plan = None
        ok = any(it.prev >= 0 and it.n > 0 for it in inst)            # at least one real recurrence step
        for head, it0 in enumerate(inst):
            if not ok:
                break
            if it0.prev >= 0:
                continue
            chain = [head]
            while inst[chain[-1]].next >= 0:
                chain.append(inst[chain[-1]].next)
            chain = [i for i in chain]
            if any(inst[i].rnn != it0.rnn for i in chain):
                ok = False
                break
            n_tracks, prev_tr, steps = 0, None, []
            for k, i in enumerate(chain):
                it = inst[i]
                tr = np.full(it.n, -1, dtype=np.int64)
                has = np.zeros(it.n, dtype=bool)
                if k > 0 and it.n:
                    pi = np.asarray(it.prev_idx, dtype=np.int64)
                    has = pi >= 0
                    tr[has] = prev_tr[pi[has]]
                new = np.nonzero(~has)[0]
                if new.size:
                    used = np.zeros(n_tracks, dtype=bool)
                    used[tr[has]] = True
                    free = np.nonzero(~used)[0]
                    take = min(free.size, new.size)
                    tr[new[:take]] = free[:take]
                    extra = new.size - take
                    if extra:
                        tr[new[take:]] = n_tracks + np.arange(extra)
                        n_tracks += extra
                steps.append((i, tr, has))
                prev_tr = tr
            if n_tracks == 0:
                continue
            n_pan = (n_tracks + T - 1) // T
            tab = np.full((len(chain), n_pan * T), -1, dtype=np.int64)
            for k, (i, tr, has) in enumerate(steps):
                if tr.size:
                    tab[k, tr] = (inst[i].h0 + np.arange(tr.size)) | (has.astype(np.int64) << 30)
            tab = tab.reshape(len(chain), n_pan, T)
            active = (tab >= 0).any(axis=2)                              # [K, P]
            anyp = ((tab >= 0) & ((tab >> 30) & 1).astype(bool)).any(axis=2)
            act_t = active.T                                             # panel-major, position-minor
            counts = act_t.sum(axis=1)
            if counts.max() > _lib.CHAIN_MAX_STEPS:
                ok = False
                break
            first = s_base + np.concatenate([[0], np.cumsum(counts)[:-1]])
            panel.append(np.stack([np.full(n_pan, it0.rnn), first, counts, np.zeros(n_pan, dtype=np.int64)], axis=1))
            rows_tab.append(tab.transpose(1, 0, 2)[act_t])
            any_prev.append(anyp.T[act_t])
            step_inst.append(np.broadcast_to(np.asarray(chain)[None, :], act_t.shape)[act_t])
            s_base += int(counts.sum())
        if ok and panel:
            pn = np.concatenate(panel)
            pn = pn[pn[:, 2] > 0]
            plan = dict(panel=pn.astype(np.int32), rows=np.concatenate(rows_tab).astype(np.int32),
                        any_prev=np.concatenate(any_prev), step_inst=np.concatenate(step_inst).astype(np.int64))
        return plan

    def chain_tables(self, device, want):
        """Device tables of the persistent chain kernels for one set of consumed instances (`want`: the instances whose
        states are handed out -- their rows are written to H and receive an upstream gradient; None = all rows, one dense
        gradient).  One packed upload, cached per (device, want)."""
        plan = self.chain_plan()
        _lib.pause_point()
        if plan is None or (want is not None and len(want) > _lib.CHAIN_MAX_UP):
            return None
        cache = self.__dict__.setdefault("_chain_tabs", {})
        key = (str(device), want)
        tabs = cache.get(key)
        if tabs is None:
            S = plan["rows"].shape[0]
            sinfo = np.zeros((S, 4), dtype=np.int32)
            si = plan["step_inst"]
            if want is None:
                sinfo[:, 0] = plan["any_prev"].astype(np.int32) | 2
            else:
                sel = np.full(len(self.inst), -1, dtype=np.int32)
                sel[list(want)] = np.arange(len(want), dtype=np.int32)
                h0 = np.array([it.h0 for it in self.inst], dtype=np.int32)
                sinfo[:, 0] = plan["any_prev"].astype(np.int32) | np.where(sel[si] >= 0, 2, 0)
                sinfo[:, 1] = sel[si]
                sinfo[:, 2] = np.where(sel[si] >= 0, h0[si], 0)
            dt = np.zeros(self.n_total, dtype=np.float32)
            for it in self.inst:
                if it.n:
                    dt[it.h0:it.h0 + it.n] = np.asarray(it.dt, dtype=np.float32).reshape(-1)
            _lib.pause_point()
            parts = [plan["panel"].reshape(-1), plan["rows"].reshape(-1), sinfo.reshape(-1), dt.view(np.int32)]
            buf = _lib.to_device(np.concatenate(parts), device)
            cuts = np.cumsum([0] + [p.size for p in parts])
            tabs = cache[key] = dict(n_panels=int(plan["panel"].shape[0]), n_steps=int(S), max_steps=int(plan["panel"][:, 2].max()), panel=buf[cuts[0]:cuts[1]], rows=buf[cuts[1]:cuts[2]],
                                     sinfo=buf[cuts[2]:cuts[3]], dt_bits=buf[cuts[3]:cuts[4]])
        return tabs

    def gi_shared(self, device):
        """Input-gate sharing of a program whose x rows repeat (`x_src`, set by the owner of the program: a label per x row,
        equal labels = equal rows -- e.g. the layer-output row a chain row was gathered from; an entity visited at p positions
        of a window whose snapshot at those positions is the same appears p times).  The gates are a function of the x row
        alone, so each group computes them once per DISTINCT row:
          -> dict(rep [per group: int32 device table, x row (inside the group) of every distinct row],
                  g0 [per group: first row of the group's block in the shared gi buffer], rows (total distinct rows),
                  gi_index int32 device [n_total]: gi row of chain row i  (TempGruChain.gi_index))
        or None when there is nothing to share (no labels, or fewer than 1 row in 8 repeats).  Cached per device."""
        src = getattr(self, "x_src", None)
        if src is None:
            return None
        c = getattr(self, "_gi_shared", None)
        if c is not None and c[0] == str(device):
            return c[1]
        src = np.asarray(src)
        reps, g0, index, total = [], [], np.zeros(self.n_total, dtype=np.int32), 0
        n_labels = int(src.max()) + 1 if src.size else 0
        for g in self.groups:
            assert g["x1"] - g["x0"] == g["h1"] - g["h0"]
            first, inv = _hostlib.unique_labels(src[g["x0"]:g["x1"]], n_labels)     # (numpy.unique's first / inverse, O(n))
            reps.append(first)
            g0.append(total)
            index[g["h0"]:g["h1"]] = total + inv.reshape(-1)
            total += first.size
        res = None
        if total * 8 <= self.n_total * 7:
            buf = _lib.to_device(np.concatenate(reps + [index]), device)
            cuts = np.cumsum([0] + [r.size for r in reps])
            res = dict(rep=[buf[cuts[i]:cuts[i + 1]] for i in range(len(reps))], g0=g0, rows=int(total), gi_index=buf[cuts[-1]:])
        self._gi_shared = (str(device), res)
        return res

    def x_index(self, device):
        """int32 device table [n_total]: the x row of every chain row (instance i maps rows h0 .. h0 + n to x0 .. x0 + n).  Cached."""
        c = getattr(self, "_x_index", None)
        if c is None or c[0] != str(device):
            idx = np.zeros(self.n_total, dtype=np.int32)
            for it in self.inst:
                idx[it.h0:it.h0 + it.n] = it.x0 + np.arange(it.n, dtype=np.int32)
            c = self._x_index = (str(device), _lib.to_device(idx, device))
        return c[1]

    def x_rows(self, device, chain_rows=None):
        """int32 device table [n_total]: the TABLE row of every chain row when the x rows are a selection of a table's rows,
        x_all = table[chain_rows] (gru_chain(table=...)): x_rows[i] = chain_rows[x_index[i]].  `chain_rows`: the host row list, given
        once (by whoever prepares the program); afterwards the cached table is returned.  None: never given, or the list holds a
        negative entry (a zero row: there is no table row to read in place)."""
        if chain_rows is not None:
            rows, idx = np.asarray(chain_rows).reshape(-1), np.zeros(self.n_total, dtype=np.int64)
            for it in self.inst:
                idx[it.h0:it.h0 + it.n] = it.x0 + np.arange(it.n, dtype=np.int64)
            tab = None
            if rows.size == 0 or int(rows.min()) >= 0:
                tab = _lib.to_device(rows[idx].astype(np.int32), device)
            self._x_rows = (str(device), tab, int(rows.shape[0]), int(rows.max()) + 1 if rows.size else 0)
        c = getattr(self, "_x_rows", None)
        return c[1] if c is not None and c[0] == str(device) else None

    x_rows_count = property(lambda self: self._x_rows[2], doc="rows of the chain_rows list x_rows was composed from (= x rows)")
    x_rows_max = property(lambda self: self._x_rows[3], doc="1 + the largest table row in it")

    def constants(self, device, d):
        """(zero previous-state row, all -1 row map long enough for any first-position instance), created once per program."""
        key = (str(device), int(d))
        c = getattr(self, "_const", None)
        if c is None or c[0] != key:
            n0 = max([it.n for it in self.inst if it.prev < 0] + [1])
            c = self._const = (key, torch.zeros(1, d, dtype=torch.float32, device=device), torch.full((n0,), -1, dtype=torch.int32, device=device))
        return c[1], c[2]

    def upload(self, device):
        """Row maps and time gaps of every instance on `device`: packed on the host into ONE int32 buffer (the float gaps as
        raw bits) and uploaded with one copy; the per-instance tensors are views."""
        if self.dev is not None and self.dev[0] == str(device):
            return self.dev[1]
        parts, spans, off = [], [], 0
        for it in self.inst:
            span = []
            for arr in (it.prev_idx.astype(np.int32) if it.prev >= 0 else None, it.next_idx,
                        np.ascontiguousarray(it.dt, dtype=np.float32).view(np.int32)):
                if arr is None:
                    span.append(None)
                    continue
                parts.append(arr.reshape(-1))
                span.append((off, off + arr.size))
                off += arr.size
            spans.append(span)
        buf = _lib.to_device(np.concatenate(parts) if parts else np.zeros(0, np.int32), device)
        cut = lambda sp: buf[sp[0]:sp[1]] if sp is not None else None
        t = [(cut(a), cut(b), cut(c).view(torch.float32)) for a, b, c in spans]
        self.dev = (str(device), t)
        return t


def _require_chain_kernels(what, tabs, usable, advice=""):
    """A learnable decay and a state offset run on the persistent chain kernels only: anything those refuse raises."""
    if tabs is None or not usable:
        raise _lib.TempAmdError("gru_chain: a %s runs on the persistent chain kernels only, and %s" % (
            what, "this backend / width / cell has none that take it" if not usable else
            "they refuse this program (not a set of one-GRU chains, a panel longer than %d steps, or more than %d consumed "
            "instances): use the per-position loop%s" % (_lib.CHAIN_MAX_STEPS, _lib.CHAIN_MAX_UP, advice)))


def _group_rows(groups):
    """-> (the slice of x rows, the slice of chain rows) of every group."""
    return [slice(g["x0"], g["x1"]) for g in groups], [slice(g["h0"], g["h1"]) for g in groups]


def _input_gates(be, prog, x_all, W, variant, fused, share, x_keys):
    """gi = x . W_ih^T + b_ih -> (gi, gi_index).  gi_index: the gi row of every chain row where the gates are computed once per distinct
    x row (`share`), else None (gi row = chain row).  (None, None) on the fused route: the chain forward computes the gates itself."""
    if fused:
        return None, None
    groups, (xsl, hsl) = prog.groups, _group_rows(prog.groups)
    xs, w_ih, b_ih = [x_all[a] for a in xsl], [W[g["rnn"]][0] for g in groups], [W[g["rnn"]][2] for g in groups]
    gi = torch.empty(prog.n_total if share is None else share["rows"], W[0][0].shape[0], dtype=torch.float32, device=x_all.device)
    kw = dict(x_keys=[x_keys[0][a] for a in xsl]) if x_keys is not None else {}
    if share is not None:
        cut = share["g0"] + [share["rows"]]
        be.gru_input_gates_multi(xs, w_ih, b_ih, variant, [gi[cut[i]:cut[i + 1]] for i in range(len(groups))], x_idx=share["rep"], **kw)
        return gi, share["gi_index"]
    if len(groups) > 1:                                        # both directions' input gates in one launch
        be.gru_input_gates_multi(xs, w_ih, b_ih, variant, [gi[b] for b in hsl], **kw)
    else:
        for x, w, b, rows in zip(xs, w_ih, b_ih, hsl):
            be.gru_input_gates(x, w, b, variant, gi[rows])
    return gi, None


def _chain_forward(be, prog, tabs, x_all, gi, gi_index, W, lam, variant, fused, decay, offset, H, saved):
    """Pack the recurrent weights and run ALL positions in one launch -> the packs (the chain backward takes them as they are)."""
    w_ih, w_hh, b_ih, b_hh = ([w[k] for w in W] for k in range(4))
    if fused:
        packs = be.gru_chain_pack_x_multi(w_hh, w_ih)
        be.gru_chain_fwd_x(tabs, x_all, prog.x_index(x_all.device), lam, variant, packs, b_hh, b_ih, H, saved, **decay)
        return packs
    if offset:                                                 # packed for the kernels an offset chain runs on, whatever the options select
        packs = be.gru_chain_pack_multi(w_hh, layout=be.gru_chain_offset_layout(x_all.shape[1]))
    else:
        packs = be.gru_chain_pack_multi(w_hh) if hasattr(be, "gru_chain_pack_multi") else [be.gru_chain_pack(w) for w in w_hh]
    be.gru_chain_fwd(tabs, gi, lam, variant, packs, b_hh, H, saved, gi_index=gi_index, **decay, **offset)
    return packs


def _position_forward(be, prog, gi, W, lam, variant, H, saved):
    """One launch per level of the program (the instances at the same distance from their chain start); no packs: -> None."""
    tens = prog.upload(H.device)
    _, none_idx = prog.constants(H.device, H.shape[1])
    for level in prog.levels:
        cells = []
        for i in level:
            it = prog.inst[i]
            p = prog.inst[it.prev] if it.prev >= 0 else None      # None = no history yet: every previous state is zero (pointwise cell)
            cells.append(dict(gi=gi[it.h0:it.h0 + it.n], prev=H[p.h0:p.h0 + p.n] if p is not None else None,
                              prev_idx=tens[i][0] if p is not None else none_idx[:it.n], dt=tens[i][2], w_hh=W[it.rnn][1], b_hh=W[it.rnn][3],
                              h_out=H[it.h0:it.h0 + it.n], row0=it.h0))
        be.gru_cell_fwd_multi(cells, lam, variant, saved)


def _gate_grads_g4(be, ctx, saved, ups, W, decay, offset):
    """The chain backward with its gate gradients written ONCE, g4 = [dr | dz | dn_i | dn_h] (two thirds of dgh repeat dgi) -> (g4, keys).
    keys (f16 arithmetic): the magnitude keys of g4 -- per row, per GRU and column -- that the weight-gradient and d_x products split it
    with (integer maxima, so bit-repeatable), or None.  An offset chain hands out none: saved[4] = dec . s_prev is not bounded by the
    keyed products' constant state scale."""
    N, d, dev = saved.shape[1], saved.shape[2], saved.device
    g4 = torch.empty(N, 4 * d, dtype=torch.float32, device=dev)
    keys = None
    if KEYED_GRADS and not offset and hasattr(be, "gru_chain_keys_supported") and be.gru_chain_keys_supported(d):
        keys = (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(ctx.n_rnn + ctx.tabs["n_panels"], 4 * d, dtype=torch.int32, device=dev))
    be.gru_chain_bwd_g4(ctx.tabs, saved, ups, ctx.lam, ctx.variant, ctx.packs, [w[3] for w in W], g4,
                        **({"keys": keys} if keys is not None else {}), **decay, **offset)
    return g4, keys


def _gate_grads_chain(be, ctx, saved, ups, W, decay, offset, dgi, dgh):
    """The chain backward writing the two matrices dgi [N, G] and dgh [N, 3d]."""
    be.gru_chain_bwd(ctx.tabs, saved, ups, ctx.lam, ctx.variant, ctx.packs, [w[3] for w in W], dgi, dgh, **decay, **offset)


def _gate_grads_positions(be, ctx, saved, ups, W, dgi, dgh):
    """dgi and dgh with one launch per level, last level first; d_prev carries the state gradients from position to position."""
    prog, dev = ctx.prog, saved.device
    tens = prog.upload(dev)
    decv = torch.empty(prog.n_total, dtype=torch.float32, device=dev)
    d_prev = torch.empty(prog.n_total, saved.shape[2], dtype=torch.float32, device=dev)
    given = dict(zip(ctx.want, ups)) if ctx.want is not None else None
    for level in reversed(prog.levels):
        cells = []
        for i in level:
            it = prog.inst[i]
            nxt = prog.inst[it.next] if (it.next >= 0 and prog.inst[it.next].n > 0) else None
            sl = slice(it.h0, it.h0 + it.n)
            cells.append(dict(row0=it.h0, n=it.n, dh_up=ups[0][sl] if given is None else given.get(i),
                              d_prev_next=d_prev[nxt.h0:nxt.h0 + nxt.n] if nxt is not None else None, next_idx=tens[i][1] if nxt is not None else None,
                              dt=tens[i][2], w_hh=W[it.rnn][1], dgi=dgi[sl], dgh=dgh[sl], decv=decv[sl], d_prev=d_prev[sl], no_prev=it.prev < 0))
        be.gru_cell_bwd_multi(cells, ctx.lam, ctx.variant, saved)


# the weight-gradient strategies: each -> (d_w_ih, d_w_hh, d_b_ih, d_b_hh) per group, with the d_x of the group's rows written to d_x_all
def _weight_grads_g4(be, ctx, x_all, saved, g4, keys, W, d_x_all):
    """ONE launch for all products, from g4 (temp_gru_grads_g4; on the f16 pipe where the chain backward handed out keys)."""
    groups, (xsl, hsl) = ctx.prog.groups, _group_rows(ctx.prog.groups)
    kw = dict(row_keys=[keys[0][b] for b in hsl], col_keys=[keys[1][g["rnn"]] for g in groups]) if keys is not None else {}
    if keys is not None and ctx.x_keys is not None:
        kw["x_col_keys"] = [ctx.x_keys[1]] * len(groups)       # (a bound over ALL rows of x_all bounds every group's rows)
    return be.gru_grads_g4([x_all[a] for a in xsl], [saved[4, b] for b in hsl], [g4[b] for b in hsl], [W[g["rnn"]][0] for g in groups],
                           [d_x_all[a] for a in xsl], **kw)


def _weight_grads_multi(be, ctx, x_all, saved, dgi, dgh, W, d_x_all):
    """ONE product launch, ONE reduction and ONE d_x launch from dgi and dgh; None (nothing launched): a shape left to the per-GRU call."""
    xsl, hsl = _group_rows(ctx.prog.groups)
    return be.gru_weight_grads_multi([x_all[a] for a in xsl], [saved[4, b] for b in hsl], [dgi[b] for b in hsl], [dgh[b] for b in hsl],
                                     [W[g["rnn"]][0] for g in ctx.prog.groups], ctx.variant, [d_x_all[a] for a in xsl])


def _weight_grads_per_group(be, ctx, x_all, saved, dgi, dgh, W, zero_state, d_x_all):
    """Every group with launches of its own (temp_gru_weight_grads).  Groups may share x rows (the two centre cells of a bi-directional
    window): the first one writes their d_x, a later one adds to it."""
    written, out = np.zeros(x_all.shape[0], dtype=bool), []
    for g, zero, xs, hs in zip(ctx.prog.groups, zero_state, *_group_rows(ctx.prog.groups)):
        first = not written[xs].any()
        assert first or written[xs].all()
        tgt = d_x_all[xs] if first else torch.empty_like(d_x_all[xs])
        out.append(be.gru_weight_grads(x_all[xs], None if zero else saved[4, hs], dgi[hs], dgh[hs], W[g["rnn"]][0], ctx.variant, tgt))
        if not first:
            d_x_all[xs] += tgt
        written[xs] = True
    return out


def _scatter_grads(ctx, per_group, d_x_all):
    """Per-group results -> the 4 * n_rnn gradients in weight order, the groups of one GRU summed; x rows that no group reads get d_x = 0."""
    grads, covered = [None] * (4 * ctx.n_rnn), np.zeros(d_x_all.shape[0], dtype=bool)
    for g, gw in zip(ctx.prog.groups, per_group):
        covered[g["x0"]:g["x1"]] = True
        for k in range(4):
            j = 4 * g["rnn"] + k
            grads[j] = gw[k] if grads[j] is None else grads[j] + gw[k]
    if not covered.all():
        d_x_all[torch.from_numpy(~covered).to(d_x_all.device)] = 0
    return grads


def _backward_result(be, ctx, d_x_all, grads, decay, offset):
    """The gradient of every input of _GruChainFn.forward, in its order."""
    d_dec, d_off = (None, None), (None, None, None)
    if decay:        # d_arg = dL / d(w dt + b) per row, reduced to (d_w, d_b) per GRU [n_rnn, 2]: all GRUs share the one Linear
        d_wb = be.gru_chain_decay_reduce(ctx.tabs, d_x_all.shape[1], ctx.variant, decay["d_arg"], ctx.n_rnn)
        d_dec = (d_wb[:, 0].sum().reshape(1, 1), d_wb[:, 1].sum().reshape(1))
    if offset:       # d_state = the gradient reaching every row's state: the table's gradient is the adjoint of the row gather table[index]
        seg_ptr, order = ctx.off_inverse             # applied to it (a segment sum over the static inverse: no atomics)
        d_off = (be.segment_sum_rows(offset["d_state"], seg_ptr, order, ctx.off_rows), None, None)
    return (d_x_all, None, None, None, None, None, None) + d_dec + d_off + tuple(grads)


def _grads_strategy(be, prog, d, variant, on_chain):
    """-> (zero_state per group, one_launch, once): which weight-gradient strategy a program takes.  GRUs with disjoint x rows (the two
    directions of a bidirectional chain, or the one GRU of a uni-directional one) take a one-launch strategy -- with the gate gradients
    written once where the library takes these shapes."""
    groups = prog.groups
    zero_state = [all(it.prev < 0 for it in prog.inst if it.group == gi) for gi in range(len(groups))]    # hdec = 0 on every row
    disjoint = all(groups[a]["x1"] <= groups[b]["x0"] or groups[b]["x1"] <= groups[a]["x0"] for a in range(len(groups)) for b in range(a))
    one_launch = bool(groups and disjoint and not any(zero_state) and len({g["rnn"] for g in groups}) == len(groups) and WEIGHT_GRADS_MULTI)
    once = one_launch and GATE_GRADS_ONCE and on_chain and be.gru_grads_g4_supported([g["h1"] - g["h0"] for g in groups], d, variant)
    return zero_state, one_launch, once


class _GruChainFn(torch.autograd.Function):
    """forward() decides the route once and keeps it on ctx as plain values: tabs (the chain kernels' tables; None = the per-position
    launches), fused (the chain forward reads x: no gi), share (input gates once per distinct x row) and the decay / offset keyword dicts,
    which reach the backend only when present (one without them never sees the keywords).  W = [(w_ih, w_hh, b_ih, b_hh)] per GRU."""

    @staticmethod
    def forward(ctx, x_all, prog, lam, variant, n_rnn, want, x_keys, dec_w, dec_b, off_table, off_index, off_inverse, *weights):
        be = get_backend()
        dev, d, N = x_all.device, x_all.shape[1], prog.n_total
        x_all = x_all.detach().contiguous()
        W = [tuple(w.detach().contiguous() for w in weights[4 * r:4 * r + 4]) for r in range(n_rnn)]
        # persistent chain kernels (one launch for ALL positions) when the backend has them and the program is a set of chains
        tabs = prog.chain_tables(dev, want) if chain_kernels_usable(d, n_rnn) else None
        # learnable decay (dec_w, dec_b = the layer's Linear(1, 1)): the chain kernels read {w, b} from device memory -- no host read
        decay = {}
        if dec_w is not None:
            _require_chain_kernels("learnable decay", tabs, chain_decay_usable(d, variant, n_rnn), " (run_rnn with decay_spec())")
            decay = dict(decay=torch.cat([dec_w.detach().reshape(1), dec_b.detach().reshape(1)]).to(torch.float32))
        # state offset (off_table [T, d], off_index int32 [n_total], -1 = none): row i leaves GRU(...) + off_table[off_index[i]], which
        # is also what the next position decays -- inside the chain kernels (pointers only, no host read)
        offset = {}
        if off_table is not None:
            _require_chain_kernels("state offset", tabs, chain_offset_usable(d, variant, n_rnn))
            assert off_table.shape[1] == d and off_index.dtype == torch.int32 and off_index.numel() == N
            offset = dict(offset=(off_table.detach().contiguous(), off_index))
        # nn.GRU cells on the f16 route: the chain forward computes the input gates itself from the x rows (temp_gru_chain_fwd's x route):
        # no gi, no gate GEMM.  Independent of x_src (a labelled and an unlabelled program take the same kernel); not for an offset chain,
        # whose states leave the range of the f16 state split (it keeps the gi route and the bf16 / fp32 chain kernels)
        fused = bool(tabs is not None and not offset and FUSED_INPUT_GATES and variant == _lib.GRU_TORCH and hasattr(be, "gru_chain_fwd_x")
                     and be.gru_chain_fwd_x_supported(d, variant, tabs["max_steps"]))
        share = prog.gi_shared(dev) if (tabs is not None and not fused) else None        # gates once per distinct x row (chain kernels only)
        # x_keys = (row keys [x rows], column keys [d]) of x_all from its producer (functional.gather_rows(keys=True)): the input-gate
        # product and the weight gradients then run on the f16 pipe without a pass over x of their own
        x_keys = x_keys if tabs is not None else None
        gi, gi_index = _input_gates(be, prog, x_all, W, variant, fused, share, x_keys)
        H, saved = torch.empty(N, d, dtype=torch.float32, device=dev), torch.empty(5, N, d, dtype=torch.float32, device=dev)
        if tabs is not None:
            packs = _chain_forward(be, prog, tabs, x_all, gi, gi_index, W, lam, variant, fused, decay, offset, H, saved)
        else:
            packs = _position_forward(be, prog, gi, W, lam, variant, H, saved)
        ctx.set_materialize_grads(False)             # states nobody differentiates (the history handed to the all-entity pass in an
                                                     # encoder-only step) come back as None, not as zero-filled (n, d) tensors
        ctx.save_for_backward(x_all, saved, *[w for ws in W for w in ws])
        ctx.prog, ctx.lam, ctx.variant, ctx.n_rnn, ctx.G, ctx.want = prog, lam, variant, n_rnn, weights[0].shape[0], want    # G: 3d or d (type-1)
        ctx.tabs, ctx.fused, ctx.share, ctx.decay, ctx.offset, ctx.x_keys, ctx.packs = tabs, fused, share, decay, offset, x_keys, packs
        ctx.off_inverse, ctx.off_rows = off_inverse, (off_table.shape[0] if off_table is not None else 0)
        if want is None:
            return H
        # only these instances' states are consumed downstream: hand them out as row ranges of H, so that the backward receives
        # one small gradient per range instead of autograd zero-filling and summing full-size (n_total, d) tensors per slice
        return tuple(H[prog.inst[i].h0:prog.inst[i].h0 + prog.inst[i].n] for i in want)

    @staticmethod
    def backward(ctx, *d_outs):
        be = get_backend()
        x_all, saved = ctx.saved_tensors[:2]
        W = [ctx.saved_tensors[2 + 4 * r:6 + 4 * r] for r in range(ctx.n_rnn)]
        prog, groups = ctx.prog, ctx.prog.groups
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x_all.device)
        d, N = x_all.shape[1], prog.n_total
        # upstream gradients: one dense dH (want = None), else one per wanted instance (None: none for that instance's rows)
        if ctx.want is None:
            ups = [d_outs[0].contiguous() if d_outs[0] is not None else torch.zeros(N, d, dtype=torch.float32, device=x_all.device)]
        else:
            given = {i: g.contiguous() for i, g in zip(ctx.want, d_outs) if g is not None}
            ups = [given.get(i) for i in ctx.want]
        # what the chain backward writes besides the gate gradients, for _backward_result
        decay = dict(ctx.decay, d_arg=new(N)) if ctx.decay else {}
        offset = dict(ctx.offset, d_state=new(N, d)) if ctx.offset else {}
        zero_state, one_launch, once = _grads_strategy(be, prog, d, ctx.variant, ctx.tabs is not None)
        if once:
            g4, keys = _gate_grads_g4(be, ctx, saved, ups, W, decay, offset)
            d_x_all = torch.empty_like(x_all)
            per_group = _weight_grads_g4(be, ctx, x_all, saved, g4, keys, W, d_x_all)
        else:
            dgi, dgh = new(N, ctx.G), new(N, 3 * d)
            if ctx.tabs is not None:
                _gate_grads_chain(be, ctx, saved, ups, W, decay, offset, dgi, dgh)
            else:
                _gate_grads_positions(be, ctx, saved, ups, W, dgi, dgh)
            d_x_all = torch.empty_like(x_all)
            per_group = _weight_grads_multi(be, ctx, x_all, saved, dgi, dgh, W, d_x_all) if one_launch else None
            if per_group is None:
                per_group = _weight_grads_per_group(be, ctx, x_all, saved, dgi, dgh, W, zero_state, d_x_all)
        return _backward_result(be, ctx, d_x_all, _scatter_grads(ctx, per_group, d_x_all), decay, offset)


class _GruChainRowsFn(torch.autograd.Function):
    """The fused-forward, keyed-gradient route of _GruChainFn with the x rows read IN PLACE: x_all = table[chain_rows] is never
    written.  The chain forward reads table rows through prog.x_rows (its x route takes any row table), the weight gradients through
    the same table (gru_grads_g4_rows), and the column keys of x are those of the table (one columns-only pass: every table row is a
    chain row in the models' batches, and a bound over more rows is a bound).  d_x is still written in chain order; the table's
    gradient is the segment sum over `inverse` that the gather's backward runs (functional._GatherRowsFn), ReLU fold included.
    Taken only where rows_in_place_usable() says so: no decision is left to make here."""

    @staticmethod
    def forward(ctx, table, prog, inverse, relu_table, lam, variant, n_rnn, want, *weights):
        be = get_backend()
        dev, d, N = table.device, table.shape[1], prog.n_total
        table = table.detach().contiguous()
        W = [tuple(w.detach().contiguous() for w in weights[4 * r:4 * r + 4]) for r in range(n_rnn)]
        tabs, x_rows = prog.chain_tables(dev, want), prog.x_rows(dev)
        x_col_keys = be.absmax_keys(table, rows=False)[1]
        H, saved = torch.empty(N, d, dtype=torch.float32, device=dev), torch.empty(5, N, d, dtype=torch.float32, device=dev)
        w_ih, w_hh, b_ih, b_hh = ([w[k] for w in W] for k in range(4))
        packs = be.gru_chain_pack_x_multi(w_hh, w_ih)
        be.gru_chain_fwd_x(tabs, table, x_rows, lam, variant, packs, b_hh, b_ih, H, saved)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(table, saved, x_rows, x_col_keys, *[w for ws in W for w in ws])
        ctx.prog, ctx.lam, ctx.variant, ctx.n_rnn, ctx.want, ctx.tabs, ctx.packs = prog, lam, variant, n_rnn, want, tabs, packs
        ctx.inverse, ctx.relu_table = inverse, relu_table
        if want is None:
            return H
        return tuple(H[prog.inst[i].h0:prog.inst[i].h0 + prog.inst[i].n] for i in want)

    @staticmethod
    def backward(ctx, *d_outs):
        be = get_backend()
        table, saved, x_rows, x_col_keys = ctx.saved_tensors[:4]
        W = [ctx.saved_tensors[4 + 4 * r:8 + 4 * r] for r in range(ctx.n_rnn)]
        prog, groups = ctx.prog, ctx.prog.groups
        d, N = table.shape[1], prog.n_total
        if ctx.want is None:
            ups = [d_outs[0].contiguous() if d_outs[0] is not None else torch.zeros(N, d, dtype=torch.float32, device=table.device)]
        else:
            given = {i: g.contiguous() for i, g in zip(ctx.want, d_outs) if g is not None}
            ups = [given.get(i) for i in ctx.want]
        g4, keys = _gate_grads_g4(be, ctx, saved, ups, W, {}, {})
        xsl, hsl = _group_rows(groups)
        d_x_all = torch.empty(prog.x_rows_count, d, dtype=torch.float32, device=table.device)
        per_group = be.gru_grads_g4_rows(table, [x_rows[b] for b in hsl], [saved[4, b] for b in hsl], [g4[b] for b in hsl],
                                         [W[g["rnn"]][0] for g in groups], [d_x_all[a] for a in xsl], row_keys=[keys[0][b] for b in hsl],
                                         col_keys=[keys[1][g["rnn"]] for g in groups], x_col_keys=[x_col_keys] * len(groups))
        grads = _scatter_grads(ctx, per_group, d_x_all)
        seg_ptr, order = ctx.inverse
        d_table = be.segment_sum_rows(d_x_all, seg_ptr, order, table.shape[0], relu_of=table if ctx.relu_table else None)
        return (d_table, None, None, None, None, None, None, None) + tuple(grads)


def rows_in_place_usable(prog, table, inverse, n_rnn, type1=False, want=None, decay=None, offset=None):
    """True when gru_chain(None, prog, ..., table=(table, chain_rows, inverse, .)) reads the table's rows in place (_GruChainRowsFn)
    instead of copying them into chain order first: the program's row table has been composed (GruProgram.x_rows), the chain runs on
    the fused x forward and hands out keys, the weight gradients are the one keyed launch, there is neither a learnable decay nor a
    state offset, and the table's byte offsets fit 32 bits."""
    be = get_backend()
    dev, d = table.device, table.shape[1]
    variant = _lib.GRU_TYPE1 if type1 else _lib.GRU_TORCH
    if not (ROWS_IN_PLACE and hasattr(be, "gru_grads_g4_rows") and decay is None and offset is None and variant == _lib.GRU_TORCH):
        return False
    if inverse is None or d % 4 or d > 256 or table.shape[0] * d * 4 >= 2 ** 32 or prog.x_rows(dev) is None or prog.x_rows_max > table.shape[0]:
        return False
    tabs = prog.chain_tables(dev, tuple(want) if want is not None else None) if chain_kernels_usable(d, n_rnn) else None
    if tabs is None or not (FUSED_INPUT_GATES and hasattr(be, "gru_chain_fwd_x") and be.gru_chain_fwd_x_supported(d, variant, tabs["max_steps"])):
        return False
    if not (KEYED_GRADS and hasattr(be, "gru_chain_keys_supported") and be.gru_chain_keys_supported(d) and be.keys_supported(d)):
        return False
    return bool(_grads_strategy(be, prog, d, variant, True)[2]
                and be.gru_grads_g4_rows_supported([g["h1"] - g["h0"] for g in prog.groups], d, variant, table.shape[0]))


def chain_kernels_usable(d, n_rnn=1):
    """True when gru_chain() will run a program of this width through the persistent chain kernels."""
    be = get_backend()
    return bool(CHAIN_KERNELS and n_rnn <= _lib.CHAIN_MAX_RNN and be.gru_chain_supported(d))


def chain_decay_usable(d, variant, n_rnn=1):
    """True when the chain kernels of this backend, width and cell variant take a learnable decay (gru_chain(decay=...))."""
    be = get_backend()
    return bool(chain_kernels_usable(d, n_rnn) and hasattr(be, "gru_chain_decay_supported") and be.gru_chain_decay_supported(d, variant))


def chain_offset_usable(d, variant, n_rnn=1):
    """True when the chain kernels of this backend, width and cell variant take a state offset (gru_chain(offset=...))."""
    be = get_backend()
    return bool(chain_kernels_usable(d, n_rnn) and hasattr(be, "gru_chain_offset_supported") and be.gru_chain_offset_supported(d, variant))


def offset_tables(index_np, n_rows, device):
    """Device half of gru_chain's `offset` for a static row list: (index int32 [n_total], inverse) -- the inverse is
    functional.gather_inverse's (seg_ptr, order), the deterministic adjoint of the gather table[index].  Built once per prepared batch."""
    from .functional import gather_inverse
    index_np = np.asarray(index_np).reshape(-1)
    return _lib.to_device(index_np.astype(np.int32), device), gather_inverse(index_np, int(n_rows), device)


def program_on_chain_kernels(prog, device, want):
    """True when the chain kernels take this program for this `want` set (its tables exist; prepare_program has built them)."""
    return prog.chain_tables(device, tuple(want) if want is not None else None) is not None


def prepare_program(prog, device, d, n_rnn, want, chain_rows=None):
    """Host + upload half of a program, done once per prepared batch (by the prefetch thread when there is one): the chain
    kernels' panel tables for the `want` set the run will ask for, or -- when the program goes through the per-position
    launches -- the row maps of every instance.  chain_rows: the host row list when the x rows will be table[chain_rows]
    (gru_chain(table=...)): the composed row table is built here as well."""
    if chain_kernels_usable(d, n_rnn) and prog.chain_tables(device, tuple(want) if want is not None else None) is not None:
        _lib.pause_point()
        prog.gi_shared(device)
        prog.x_index(device)
        if chain_rows is not None:
            prog.x_rows(device, chain_rows)
        return
    prog.upload(device)


def zero_state_program(n):
    """Program of ONE cell over n rows that starts from the zero state (GRU(x, 0): the once-per-entity rows of the all-entity
    pass): hoisted input-gate GEMM + pointwise cell forward; gate gradients, d_x and d_W_ih backward -- no recurrent GEMM."""
    return GruProgram([GruInstance(n, 0, 0, -1, np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.float32))])


def gru_chain(x_all, prog, rnns, lam, type1=False, want=None, x_keys=None, decay=None, offset=None, table=None):
    """Run a GruProgram.  table: None, or (table [T, d], chain_rows int32 [x rows], inverse, relu_table) with x_all = None: the x rows
    are table[chain_rows] -- the arguments of functional.gather_rows, whose result (with its keys, where they are of use) is what runs
    otherwise -- and where rows_in_place_usable() holds they are read where they lie, never copied; the table then receives its
    gradient as the gather's backward would hand it out.  offset: None, or (table [T, d], index) / (table, index, inverse) of --use-time-embedding: row i leaves
    s_i = GRU(x_i, dec . s_prev) + table[index[i]] (index: int32 [n_total] on x_all's device, -1 = no offset), the states returned and
    carried on include it and `table` receives its gradient; (index, inverse) = offset_tables(...) -- without `inverse` it is built
    here from a host copy of `index` (a sync: prepare it instead).  Chain kernels only: anything they refuse raises.  decay: None = exp(-dt lam), or the layer's decay_spec() = (weight (1, 1), bias (1,)) of --learnable-lambda:
    exp(-max(w dt + b, 0)), shared by all `rnns` (`lam` is not read; chain kernels only: anything they refuse raises).  x_keys: (row keys, column keys) of x_all from functional.gather_rows(keys=True), or None.  `rnns`: list of modules holding (weight_ih, weight_hh, bias_ih, bias_hh)
    (nn.GRU layer 0 or the type-1 GRUCell).  Returns H_all (prog.n_total, d), or -- with `want` = a list of instance ids --
    the states of just those instances (a tuple of (n_i, d) tensors; instances with 0 rows give empty tensors)."""
    ws = []
    for r in rnns:
        if type1:
            ws += [r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh]
        else:
            ws += [r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0]
    if table is not None:
        assert x_all is None and x_keys is None, "table=...: the x rows are the table's"
        y, chain_rows, y_inv, relu_table = table
        if rows_in_place_usable(prog, y, y_inv, len(rnns), type1, want, decay, offset):
            return _GruChainRowsFn.apply(y, prog, y_inv, bool(relu_table), float(lam), _lib.GRU_TORCH, len(rnns),
                                         tuple(want) if want is not None else None, *ws)
        from .functional import gather_keys_supported, gather_rows
        if gather_keys_supported(y.shape[1]) and chain_kernels_usable(y.shape[1], len(rnns)):
            x_all, x_keys = gather_rows(y, chain_rows, y_inv, relu_table=relu_table, keys=True)
        else:
            x_all = gather_rows(y, chain_rows, y_inv, relu_table=relu_table)
    off = (None, None, None)
    if offset is not None:
        off_table, index = offset[0], offset[1]
        inverse = offset[2] if len(offset) > 2 else offset_tables(index.detach().cpu().numpy(), off_table.shape[0], index.device)[1]
        off = (off_table, index, inverse)
    return _GruChainFn.apply(x_all, prog, float(lam), _lib.GRU_TYPE1 if type1 else _lib.GRU_TORCH, len(rnns),
                             tuple(want) if want is not None else None, x_keys, decay[0] if decay is not None else None,
                             decay[1] if decay is not None else None, *off, *ws)
