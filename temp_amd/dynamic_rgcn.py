"""DynamicRGCN -- the uni-directional window model with the reference's interface
(models/DynamicRGCN.py:14-220): `DynamicRGCN(args, num_ents, num_rels, graph_dict_train,
graph_dict_val, graph_dict_test)`, `.forward(t_list) -> loss`, same parameter / state_dict names.

Two execution paths, same results:
  * reference-granular: one encoder call per window position through the drop-in `RRGCN` API,
    previous states fetched by row-gather from the previous position's output (window.ChainPlan)
    instead of the reference's dense re-zeroed history;
  * batched (GRU module + --rec-only-last-layer, the paper's recommended mode): the two RGCN layers
    of EVERY visit of the step run as ONE launch each over a block-diagonal union of all visited
    snapshots, and only the fused decay+GRU kernel walks the window positions, reading its
    previous state through `prev_idx`.  --module RRGCN (the linear recurrence) takes the same path in its plain form
    (_can_batch_linear): layer 2's aggregation + self-loop of every visit at once, then lin_chain.linear_chain; with BOTH layers
    recurrent (its grid flags) one such pass and one chain per layer over the same program (_run_lin_stack).
"""
import numpy as np
import torch

from . import functional as TF
from . import _lib
from . import _hostlib
from . import snapshot as S
from .rrgcn import RRGCN, GRRGCNLayer, RRGCNLayer, run_rnn
from .tkg_module import TKG_Module
from .gru_chain import (GruInstance, GruProgram, chain_decay_usable, chain_offset_usable, gru_chain, offset_tables, prepare_program, rows_in_place_usable,
                        program_on_chain_kernels, zero_state_program)
from .gru_cell import GRUCell
from .lin_chain import linear_chain, prepare_linear_program
from .window import ChainPlan, Step, concat_steps, concat_steps_dedup, window_times


class WindowBatch:
    """Everything `run` needs for one batch of windows (plans, batched graphs, device index tensors)."""
    pass


class DynamicRGCN(TKG_Module):
    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test, evaluater_type=None):
        self.num_layers = args.num_layers
        self.train_seq_len = args.train_seq_len
        self.test_seq_len = args.train_seq_len            # --test-seq-len is ignored by the reference too (F10)
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test, evaluater_type)
        self.edge_dropout = getattr(args, "edge_dropout", False)
        self.post_aggregation = getattr(args, "post_aggregation", False)
        self.random_dropout = getattr(args, "random_dropout", False)
        if self.edge_dropout:
            raise NotImplementedError("--edge-dropout: the reference's DropEdge.sample_subgraph reads drop_rate_cache, which is never built "
                                      "(utils/DropEdge.py:31-32,126); not on the hot path (SURVEY section 2)")
        self.init_embeddings()
        self.plan_loss_in_prepare = True
        self.use_batched_path = True
        self.use_gru_chain = True
        self.dedup_snapshots = True
        self.use_rec_stack = True             # reference-default flags (both layers recurrent): one autograd node (rec_stack.py)
        self.device_subsample = True          # training-time edge subsets drawn and applied on the GPU (host sampler when False)

    def build_model(self):
        self.ent_encoder = RRGCN(self.args, self.hidden_size, self.embed_size, self.num_rels, self.total_time)

    # ---------------------------------------------------------------------------------------------
    # shared helpers
    # ---------------------------------------------------------------------------------------------
    def _dropout_active(self, train=True):
        """The self-loop dropout of the RGCN layers (models/RGCN.py:57-59) draws in this pass: training mode, p > 0."""
        return bool(train and self.training and float(getattr(self.args, "dropout", 0.0) or 0.0) > 0.0)

    def _share_visits(self, train=True):
        """May visits of one snapshot share ONE RGCN pass?  Not while dropout draws: the reference runs the encoder per window
        position (models/DynamicRGCN.py:156-174), so every (window, position) visit gets its own mask, and layer 2 aggregates
        layer-1 rows that differ per visit -- nothing of a visit is shared then.  (Round-4 verdict: de-duplication ignored it.)"""
        return self.dedup_snapshots and not self._dropout_active(train)

    # --module RRGCN / BiRRGCN (the linear recurrence) on the batched path: the whole recurrence as one linear_chain node.  False keeps
    # the per-position loop reachable ON the batched path (linear_nt + decay_rows per position), for A/B runs and tests
    use_lin_chain = True
    _linear_model_classes = ("DynamicRGCN", "BiDynamicRGCN")      # the window models proper: the Impute* / Post* / attention classes keep their paths
    _linear_layer_class = RRGCNLayer                               # (BiDynamicRGCN: BiRRGCNLayer)

    def _linear_layer(self):
        """Layer 2 is a linear-recurrence layer (RRGCNLayer / BiRRGCNLayer: a `time_weight*` matrix instead of a GRU)."""
        return isinstance(self.ent_encoder.layer_2, self._linear_layer_class)

    def _plain_linear_layer(self, layer):
        """A linear-recurrence layer in the form the chain takes: no impute, no bias, one layer, an activation the kernels know (none,
        or the fused ReLU).  --learnable-lambda does not matter: the linear layers never read `exponential_decay` (models/RRGCN.py:141,161
        decay by inv_temperature whatever the flag says), so it stays in the state dict and gets no gradient on any path."""
        return not layer.impute and not layer.bias and getattr(layer, "num_layers", 1) == 1 and layer._post_act is None

    def _can_batch_linear(self):
        """--module RRGCN / BiRRGCN with --rec-only-last-layer takes the batched path in its plain form only: no time embedding, no
        impute / post-* stream, layer 2 a _plain_linear_layer."""
        enc, args = self.ent_encoder, self.args
        return (type(self).__name__ in self._linear_model_classes and self._linear_layer()
                and not enc.use_time_embedding and not getattr(args, "post_aggregation", False)
                and not getattr(args, "post_ensemble", False) and self._plain_linear_layer(enc.layer_2))

    # --module RRGCN with BOTH layers recurrent (the reference's grid flags: no --rec-only-last-layer) on the batched path: layer 1's
    # recurrence does not read layer 2, so the window is two linear_chain nodes over ONE program (_run_lin_stack).  False keeps the
    # reference-granular path for A/B runs and tests
    use_lin_stack = True

    def _can_stack_linear(self):
        """Both layers RRGCNLayer in the chain's plain form on DynamicRGCN itself, one decay rate; the route is the chain node's alone
        (use_lin_chain = False has no per-position form of it)."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        return (type(self) is DynamicRGCN and self.use_lin_stack and self.use_lin_chain and not enc.rec_only_last_layer
                and isinstance(l1, RRGCNLayer) and isinstance(l2, RRGCNLayer) and self._can_batch_linear()
                and self._plain_linear_layer(l1) and l1.inv_temperature == l2.inv_temperature)

    def _can_batch(self):
        enc = self.ent_encoder
        if not self.use_batched_path:
            return False
        if not enc.rec_only_last_layer:
            return self._can_stack_linear()
        if self._linear_layer():
            return self._can_batch_linear()
        return (isinstance(enc.layer_2, GRRGCNLayer)
                and not (enc.layer_2.post_aggregation or enc.layer_2.post_ensemble or enc.layer_2.impute))

    def _can_stack(self):
        """Both layers recurrent (the reference's default: no --rec-only-last-layer) on the plain uni-directional GRU model:
        the position loop runs as ONE autograd node with layer 1's RGCN and all GRU GEMMs that do not depend on the
        recurrence hoisted out of it (rec_stack.py).  Anything else keeps the reference-granular loop."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        return (type(self) is DynamicRGCN and self.use_rec_stack and self.use_batched_path and not enc.rec_only_last_layer
                and isinstance(l1, GRRGCNLayer) and isinstance(l2, GRRGCNLayer) and not l1._extra() and not l2._extra()
                and l1.decay_spec() is None and l2.decay_spec() is None and not enc.use_time_embedding
                and getattr(l1, "num_layers", 1) == 1 and l1._post_act is None and l2._post_act is None
                and l1.inv_temperature == l2.inv_temperature)

    def _gather_prev(self, prev_out, idx_t, n):
        if prev_out is None:
            return self.ent_embeds.new_zeros(n, self.embed_size)
        return TF.gather_rows(prev_out, idx_t)

    def sample_target_graphs(self, graphs, rate=0.5, edge_ids=None):
        """Random edge subsample of the target snapshots with recomputed norms
        (get_batch_graph_embeds(full=False), models/DynamicRGCN.py:76-90).  `edge_ids`
        injects the kept edge ids (tests replay the reference's recorded draws)."""
        dev = self._device()
        if edge_ids is None and dev.type == "cuda" and self.device_subsample and S.DEVICE_STORE == "kernel" and graphs:
            # on the device: the subgraphs' sorted views are derived from the snapshots' resident views (temp_subsample_views) --
            # no host rebuild, no edge upload; the draw depends only on the per-graph seed
            seeds = self.sample_rng.integers(0, 1 << 62, size=len(graphs))
            return S.device_subsample(graphs, [int(rate * g.number_of_edges()) for g in graphs], seeds, dev, 2 * self.num_rels, want_mask=True)
        out = []
        for i, g in enumerate(graphs):
            E = g.number_of_edges()
            idx = edge_ids[i] if edge_ids is not None else _hostlib.sample_subset(E, int(rate * E), self.sample_rng)
            out.append(g.edge_subgraph(idx))
        return out

    def sample_history_graphs(self, plan, rate=0.8):
        """--random-dropout: every training visit of a history snapshot runs on its own random 80 % of the edges, same
        nodes, norms recomputed (get_per_graph_ent_embeds(full=False, rate=0.8) -> get_batch_graph_embeds,
        models/DynamicRGCN.py:76-90,162-171).  Row maps depend only on the node sets, so the plan is unchanged."""
        for st in plan.steps:
            st.graphs = self.sample_target_graphs(st.graphs, rate)
            st.graph = None

    def _target_step(self, plan, rows, graphs):
        L = plan.seq_len
        st = Step(L - 1, list(range(len(graphs))), graphs, [r[-1] for r in rows])
        pidx, dts = [], []
        for b, g in enumerate(graphs):
            a, d = plan.final_prev(b, g.gids, L - 1)
            pidx.append(a)
            dts.append(d)
        st.prev_idx = np.concatenate(pidx) if pidx else np.zeros(0, np.int64)
        st.dt = np.concatenate(dts) if dts else np.zeros(0, np.float32)
        return st

    # ---------------------------------------------------------------------------------------------
    # reference-granular path
    # ---------------------------------------------------------------------------------------------
    def _encode_step(self, st, prev_first, prev_second):
        dev = self._device()
        ids, pidx, dt = st.tensors(dev)
        g = st.batched()
        g.ndata['h'] = TF.gather_rows(self.ent_embeds, ids)
        fp = self._gather_prev(prev_first, pidx, st.n_rows)
        sp = self._gather_prev(prev_second, pidx, st.n_rows)
        return self.ent_encoder(g, fp, sp, dt, st.times, st.sizes)

    def pre_forward(self, plan):
        """History positions 0..L-2 (models/DynamicRGCN.py:156-174) -> outputs of the last executed one."""
        first = second = None
        for st in plan.steps:
            first, second = self._encode_step(st, first, second)
        return first, second

    def _run_generic(self, wb):
        first, second = self.pre_forward(wb.plan)
        _, out = self._encode_step(wb.target, first, second)
        return out, (first, second)

    def _run_stack(self, wb):
        """The same loop as _run_generic as one autograd node (rec_stack.py): layer 1's RGCN over the union of the distinct
        snapshots, then per position cell 1 -> RGCN 2 -> cell 2; both cells read h2 of the position before."""
        from .rec_stack import rec_stack
        enc, dev = self.ent_encoder, self._device()
        y1 = enc.layer_1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        if wb.visit_rows is not None:
            y1 = TF.gather_rows(y1, wb.visit_rows, wb.visit_inv)
        graphs = [st.batched().device_graph(dev, 2 * self.num_rels) for st in wb.steps]
        g_union = wb.g_visits.device_graph(dev, 2 * self.num_rels) if getattr(wb, "g_visits", None) is not None else None
        got = rec_stack(y1, wb.program, graphs, enc.layer_1.rnn, enc.layer_2, self._chain_want(wb), g_union)
        hist = got[1] if wb.hist_inst >= 0 else None
        return got[0], (hist, hist)

    # ---------------------------------------------------------------------------------------------
    # batched path
    # ---------------------------------------------------------------------------------------------
    # --use-time-embedding on the chain kernels and in the batched all-entity pass: DynamicRGCN / BiDynamicRGCN proper.  The
    # Impute* / Post* classes (a local stream beside the temporal one) and SelfAttentionRGCN switch it off and keep their paths.
    _chain_time_embedding = True

    def _can_chain(self):
        """The whole recurrence as one autograd node (gru_chain): single GRU layer; a learnable decay (--learnable-lambda) or
        the per-position time embedding (--use-time-embedding: a state offset of the chain) only where the backend's chain
        kernels take one (a backend without gru_chain_decay_supported / gru_chain_offset_supported keeps the per-position loop)."""
        enc = self.ent_encoder
        l2 = enc.layer_2
        if self._linear_layer():                     # the linear recurrence: one linear_chain node (lin_chain.py)
            return bool(self.use_lin_chain)
        if not (self.use_gru_chain and getattr(l2, "num_layers", 1) == 1):
            return False
        if enc.use_time_embedding and not self._chain_takes_offset():
            return False
        return l2.decay_spec() is None or self._chain_takes_decay()

    def _chain_rnns(self):
        return [self.ent_encoder.layer_2.rnn]

    def _chain_takes_decay(self):
        rnns = self._chain_rnns()
        return chain_decay_usable(self.embed_size, _lib.GRU_TYPE1 if isinstance(rnns[0], GRUCell) else _lib.GRU_TORCH, len(rnns))

    def _chain_takes_offset(self):
        """s_p = GRU(x_p, dec . s_{p-1}) + time_embed_2[t_p] (models/RRGCN.py:192-204) as the chain's state offset: this class
        (see _chain_time_embedding), only the last layer recurrent, a GRU cell, and chain kernels that take an offset."""
        if not (self._chain_time_embedding and self._can_batch()):
            return False
        rnns = self._chain_rnns()
        return chain_offset_usable(self.embed_size, _lib.GRU_TYPE1 if isinstance(rnns[0], GRUCell) else _lib.GRU_TORCH, len(rnns))

    @staticmethod
    def _step_time_rows(st):
        """The time-embedding row of every row of a step (RGCNLayer.get_time_embedding: the step's graphs in order)."""
        return np.repeat(np.array([int(t) for t in st.times], dtype=np.int64), [int(n) for n in st.sizes])

    def _chain_offset_index(self, wb):
        """Time-embedding row of every chain row, in program order: every position adds its own, the target included."""
        return np.concatenate([self._step_time_rows(st) for st in wb.steps]) if wb.steps else np.zeros(0, np.int64)

    def _chain_offset(self, wb):
        """gru_chain's `offset` under --use-time-embedding (the tables are built in `prepare`), else None."""
        if not self.ent_encoder.use_time_embedding:
            return None
        return (self.ent_encoder.layer_2.time_embed,) + wb.chain_offset

    def _visit_rows_on_device(self):
        return True

    def _build_program(self, wb):
        inst = []
        for k, st in enumerate(wb.steps):
            has_prev = k > 0
            inst.append(GruInstance(st.n_rows, st.row0, 0, k - 1 if has_prev else -1, st.prev_idx, st.dt, st.next_idx))
        wb.program = GruProgram(inst)
        wb.out_inst = [len(inst) - 1]
        wb.hist_inst = len(inst) - 2 if len(inst) > 1 else -1

    def _chain_want(self, wb):
        """Instances whose states leave the chain: the target position and the last history position."""
        return [wb.out_inst[0]] + ([wb.hist_inst] if wb.hist_inst >= 0 else [])

    # the chain reads its input rows where layer 2 wrote them (gru_chain(table=...)) instead of from a copy in visit order; False in
    # the models that read the copy themselves (wb.last_x: the post-* models)
    rows_in_place = True

    def _chain_rows_host(self, wb):
        """The host list `rows` with GRU input = y2[rows] for the chain program (None: the input is y2 itself)."""
        return wb.visit_rows_host if wb.visit_rows is not None else None

    def _chain_weights(self):
        """The `time_weight` matrices of the linear recurrence, in the order of the program's weight indices."""
        return [self.ent_encoder.layer_2.time_weight]

    def _run_lin_stack(self, wb):
        """--module RRGCN, both layers recurrent:
            h1_p = act(pre1(E on G_p) + dec . h1_{p-1}[prev] . Wt1)       h2_p = act(pre2(h1_p on G_p) + dec . h2_{p-1}[prev] . Wt2)
        pre1 of every visit in one launch group (over the distinct snapshots where visits share them), chain 1 handing out EVERY row
        (they feed layer 2), pre2 of every visit over the visit-level union, chain 2 over the same program.
        -> (target rows of chain 2, (h1, h2) rows of the last history position: the pair DenseHistory keeps for this module)."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        lam, prog = l2.inv_temperature, wb.program
        act1, act2 = (1 if l.relu_fused() else 0 for l in (l1, l2))
        y1 = l1.pre_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        wb.last_x = None
        if wb.visit_rows is not None:                 # distinct-snapshot rows -> visit rows, gathered by the node
            H1 = linear_chain(None, prog, [l1.time_weight], lam, act1, want=None, table=(y1, wb.visit_rows, wb.visit_inv, False))
        else:
            H1 = linear_chain(y1, prog, [l1.time_weight], lam, act1, want=None)
        y2 = l2.pre(wb.g_visits, H1)
        got = linear_chain(y2, prog, [l2.time_weight], lam, act2, want=self._chain_want(wb))
        if wb.hist_inst < 0:
            return got[0], (None, None)
        it = prog.inst[wb.hist_inst]
        return got[0], (H1[it.h0:it.h0 + it.n], got[1])

    def _run_batched_linear(self, wb):
        """--module RRGCN: layer 2's aggregation + self-loop of EVERY visit in one launch group (no bias, no activation: the
        activation follows the recurrent term), then h_p = act(pre_p + dec . h_{p-1} . W) over all positions as one linear_chain node."""
        if getattr(wb, "lin_stack", False):
            return self._run_lin_stack(wb)
        enc, dev = self.ent_encoder, self._device()
        l2 = enc.layer_2
        y1 = enc.layer_1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        y2 = l2.pre(wb.g_all, y1)
        act = 1 if l2.relu_fused() else 0
        wb.last_x = None
        if wb.program is not None:
            want = self._chain_want(wb)
            if wb.visit_rows is not None:             # distinct-snapshot rows -> visit rows, gathered by the node
                got = linear_chain(None, wb.program, self._chain_weights(), l2.inv_temperature, act, want=want,
                                   table=(y2, wb.visit_rows, getattr(wb, "visit_inv", None), False))
            else:
                got = linear_chain(y2, wb.program, self._chain_weights(), l2.inv_temperature, act, want=want)
            hist = got[1] if wb.hist_inst >= 0 else None
            return got[0], (hist, hist)
        if wb.visit_rows is not None:
            y2 = TF.gather_rows(y2, wb.visit_rows, getattr(wb, "visit_inv", None))
        H, hist = None, None
        for st, x in zip(wb.steps, TF.row_spans(y2, [(st.row0, st.n_rows) for st in wb.steps])):
            _, pidx, dt = st.tensors(dev)
            H = l2.finish_rows(x, H, pidx, dt)
            if st is not wb.target:
                hist = H
        return H, (hist, hist)

    def _run_batched(self, wb):
        if self._linear_layer():
            return self._run_batched_linear(wb)
        enc, dev = self.ent_encoder, self._device()
        y1 = enc.layer_1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        y2 = enc.layer_2.conv(wb.g_all, y1)
        l2 = enc.layer_2
        if wb.program is not None and wb.visit_rows is not None and self.rows_in_place:
            want, inv, type1 = self._chain_want(wb), getattr(wb, "visit_inv", None), isinstance(l2.rnn, GRUCell)
            dec, off = l2.decay_spec(), self._chain_offset(wb)
            if rows_in_place_usable(wb.program, y2, inv, 1, type1, want, dec, off):
                wb.last_x = None                      # (no copy of the GRU input rows in visit order exists on this route)
                got = gru_chain(None, wb.program, [l2.rnn], l2.inv_temperature, type1, want=want, table=(y2, wb.visit_rows, inv, False))
                hist = got[1] if wb.hist_inst >= 0 else None
                return got[0], (hist, hist)
        if wb.visit_rows is not None:                 # distinct-snapshot rows -> visit rows
            y2 = TF.gather_rows(y2, wb.visit_rows, getattr(wb, "visit_inv", None))
        wb.last_x = y2                                # GRU input rows of the step (= the "local" states of the post models)
        if wb.program is not None:
            want = self._chain_want(wb)
            got = gru_chain(y2, wb.program, [l2.rnn], l2.inv_temperature, isinstance(l2.rnn, GRUCell), want=want, decay=l2.decay_spec(),
                            offset=self._chain_offset(wb))
            hist = got[1] if wb.hist_inst >= 0 else None
            return got[0], (hist, hist)
        H, hist = None, None
        for st, x in zip(wb.steps, TF.row_spans(y2, [(st.row0, st.n_rows) for st in wb.steps])):
            _, pidx, dt = st.tensors(dev)
            prev = H if H is not None else x.new_zeros(1, x.shape[1])
            H = run_rnn(l2.rnn, x, prev, dt, l2.inv_temperature, l2.decay_spec(), pidx)
            if enc.use_time_embedding:
                H = H + l2.get_time_embedding(st.times, st.sizes)
            if st is not wb.target:
                hist = H
        return H, (hist, hist)

    # ---------------------------------------------------------------------------------------------
    def prepare(self, t_list, seq_len, train=True, target_edge_ids=None):
        """Host-side planning + upload of everything that depends only on which snapshots are
        visited (window layout, row maps, sorted/chunked edge views).  Returns a WindowBatch that
        `run` can execute any number of times."""
        dev = self._device()
        wb = WindowBatch()
        wb.rows = window_times(t_list, seq_len, self.total_time)
        wb.plan = ChainPlan(wb.rows, self.graph_dict_train, self.num_ents, seq_len)
        _lib.pause_point()                            # (between the stages of `prepare`: a prefetch worker parks here while the loop issues a step)
        if train and self.random_dropout:
            self.sample_history_graphs(wb.plan)
        wb.graphs = [self.graph_dict_train[r[-1]] for r in wb.rows]
        tgt = self.sample_target_graphs(wb.graphs, 0.5, target_edge_ids) if train else wb.graphs
        _lib.pause_point()
        wb.target = self._target_step(wb.plan, wb.rows, tgt)
        wb.batched = self._can_batch()
        wb.stack = not wb.batched and self._can_stack()
        wb.steps = wb.plan.steps + [wb.target]
        _lib.pause_point()
        self._upload(wb, dev, train)
        _lib.pause_point()
        if train:
            self._plan_loss(wb)
        return wb

    def _upload(self, wb, dev, train=True):
        wb.program = None
        wb.visit_rows = wb.visit_rows_host = None
        wb.shared_visits = self._share_visits(train)
        wb.lin_stack = bool(wb.batched and self._linear_layer() and not self.ent_encoder.rec_only_last_layer)
        if wb.batched or getattr(wb, "stack", False):
            if wb.shared_visits:
                wb.g_all, vr, wb.total_rows = concat_steps_dedup(wb.steps)
                wb.visit_rows_host = vr                  # the device copy + its inverse only where `run` gathers by them
                on_dev = vr is not None and self._visit_rows_on_device()
                wb.visit_rows = _lib.to_device(vr, dev) if on_dev else None
                wb.visit_inv = TF.gather_inverse(vr, int(wb.g_all.n), dev) if on_dev else None
            else:
                wb.g_all, wb.total_rows = concat_steps(wb.steps)
            _lib.pause_point()
            wb.ids_all = _lib.to_device(wb.g_all.gids.astype(np.int32), dev)
            wb.ids_inv = TF.gather_inverse(wb.g_all.gids, self.num_ents, dev)        # static ids: deterministic embedding gradient
            _lib.pause_point()
            self.ent_encoder.layer_1.prepare_table(wb.g_all, self.ent_embeds.shape[0], wb.ids_all)
            _lib.pause_point()
            if getattr(wb, "stack", False):          # layer 2 runs per position: every position's own union graph as well
                for st in wb.steps:
                    st.batched().device_graph(dev, 2 * self.num_rels)
                # ... and the union of ALL visits in program row order (layer 2's weight gradients in one pass, rec_stack.py): the
                # layer-1 graph itself when no snapshot is shared between visits
                wb.g_visits = wb.g_all if wb.visit_rows_host is None else concat_steps(wb.steps)[0]
                wb.g_visits.device_graph(dev, 2 * self.num_rels)
                self._build_program(wb)
                wb.program.upload(dev)
                wb.program.constants(dev, self.embed_size)
            elif wb.lin_stack:
                # layer 2 reads states, which differ between two windows' visits of one snapshot: the union of ALL visits in program
                # row order (the layer-1 graph itself when no snapshot is shared); ONE program serves both chains -- chain 1 hands out
                # every row, chain 2 the usual two instances
                wb.g_visits = wb.g_all if wb.visit_rows_host is None else concat_steps(wb.steps)[0]
                wb.g_visits.device_graph(dev, 2 * self.num_rels)
                self._build_program(wb)
                _lib.pause_point()
                for want in (None, self._chain_want(wb)):
                    prepare_linear_program(wb.program, dev, self.embed_size, 1, want)
            elif self._can_chain() and self._linear_layer():
                self._build_program(wb)
                _lib.pause_point()
                prepare_linear_program(wb.program, dev, self.embed_size, len(self._chain_weights()), self._chain_want(wb))
            elif self._can_chain():
                self._build_program(wb)
                _lib.pause_point()
                prepare_program(wb.program, dev, self.embed_size, len(wb.out_inst), self._chain_want(wb), chain_rows=self._chain_rows_host(wb))
                # a learnable decay and the time embedding run on the chain kernels only: a program they refuse (no chain tables, a
                # panel longer than their step limit) stays on the per-position loop -- decided here, not in `run`
                enc = self.ent_encoder
                if ((enc.layer_2.decay_spec() is not None or enc.use_time_embedding)
                        and not program_on_chain_kernels(wb.program, dev, self._chain_want(wb))):
                    wb.program = None
                    if wb.visit_rows_host is not None and wb.visit_rows is None:      # (the loop gathers by the visit rows on the device)
                        wb.visit_rows = _lib.to_device(wb.visit_rows_host, dev)
                        wb.visit_inv = TF.gather_inverse(wb.visit_rows_host, int(wb.g_all.n), dev)
                elif enc.use_time_embedding:
                    wb.chain_offset = offset_tables(self._chain_offset_index(wb), enc.layer_2.time_embed.shape[0], dev)
        else:
            for st in wb.steps:
                st.batched().device_graph(dev, 2 * self.num_rels)
        if wb.program is None:                       # the per-step row maps are only read outside the chain program
            for st in wb.steps:
                st.tensors(dev)
        wb.n_edge_visits = int(sum(g.number_of_edges() for st in wb.steps for g in st.graphs))
        wb.n_edges_distinct = int(wb.g_all.number_of_edges()) if wb.batched else wb.n_edge_visits
        wb.n_nodes_distinct = int(wb.g_all.n) if wb.batched else 0
        wb.n_node_visits = int(sum(st.n_rows for st in wb.steps))

    def run(self, wb):
        """Device work of one encoder pass -> (target rows (sum n_b, D), final history outputs)."""
        if getattr(wb, "stack", False):
            return self._run_stack(wb)
        return (self._run_batched if wb.batched else self._run_generic)(wb)

    def encode(self, t_list, seq_len, train=True, target_edge_ids=None):
        """Window encoder: -> (per-window target embeddings, plan, rows, target graphs, final history)."""
        wb = self.prepare(t_list, seq_len, train, target_edge_ids)
        out, hist = self.run(wb)
        return list(out.split(wb.target.sizes)), wb.plan, wb.rows, wb.graphs, hist

    def get_all_embeds_Gt(self, convoluted_embeds, g, t, plan, b, hist):
        """Isolated pass over ALL entities, then the active rows overwritten
        (models/DynamicRGCN.py:56-64).  Previous states come from the last history output by row map."""
        dev = self._device()
        L = plan.seq_len
        if getattr(self.args, "use_embed_for_non_active", False):
            all_embeds = self.ent_embeds
        else:
            row_of, dt = plan.final_all(b, L - 1)
            idx = torch.from_numpy(row_of.astype(np.int32)).to(dev)
            dt_t = torch.from_numpy(dt).view(-1, 1).to(dev)
            p1 = self._gather_prev(hist[0], idx, self.num_ents)
            p2 = p1 if hist[1] is hist[0] else self._gather_prev(hist[1], idx, self.num_ents)
            all_embeds = self.ent_encoder.forward_isolated(self.ent_embeds, p1, p2, dt_t, t)
        gid = torch.from_numpy(g.gids).to(dev)
        return all_embeds.index_copy(0, gid, convoluted_embeds)

    def evaluation_targets(self, t_list):
        """models/DynamicRGCN.py:118-144,196-220: the window on the full train graphs at test_seq_len; all windows' all-entity
        matrices in one batched pass when the model allows it (same classes as the training loss), else per window over the graph
        that is asked for."""
        wb = self.prepare(t_list, self.test_seq_len, train=False)
        out, hist = self.run(wb)
        all_b = self.all_embeds_batched(wb, out, hist) if self._fused_all_entity_ok(wb) else None
        for i, ent_embed in enumerate(out.split(wb.target.sizes)):
            t = wb.rows[i][-1]
            yield t, ent_embed, (lambda g, i=i, t=t, ent_embed=ent_embed:
                                 all_b[i] if all_b is not None else self.get_all_embeds_Gt(ent_embed, g, t, wb.plan, i, hist))

    def forward(self, t_list, reverse=False, target_edge_ids=None, samples=None):
        """models/DynamicRGCN.py:176-194.  `target_edge_ids` / `samples` inject the random draws
        (SURVEY F11); by default they are sampled here."""
        wb = self.prepare(t_list, self.train_seq_len, True, target_edge_ids)
        return self.run_loss(wb, samples)

    def _plan_loss(self, wb):
        """Host half of the fused loss, done with the rest of `prepare` (i.e. by the prefetch thread): positives, operand
        index lists, known-true slices for the device sampler, static inverses, all-entity row maps."""
        wb.loss_plan = None
        name = self.args.score_function
        if not (self.plan_loss_in_prepare and getattr(self, "use_device_sampler", True) and self.fused_loss
                and (name in ("distmult", "complex") or (name == "transE" and TF.translation_supported()))):
            return
        from .sampling import plan_batch_loss
        dev = self._device()
        sizes = self._target_sizes(wb)
        offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        wb.loss_plan = plan_batch_loss(self.true_sets(), [r[-1] for r in wb.rows], wb.graphs, offs, self.args.num_pos_facts, self.sample_rng,
                                       int(sum(sizes)), int(self.rel_embeds.shape[0]), dev)
        _lib.pause_point()
        if self._fused_all_entity_ok(wb):
            self._all_maps(wb)

    def _target_sizes(self, wb):
        return wb.target.sizes

    def _sampled_loss(self, wb, out, all_embeds):
        """Fused loss on fresh negatives: ONE sampler launch (temp_corrupt_sample) + the fused link-prediction node."""
        return self.batched_link_prediction(out, dict(wb.loss_plan, cand=self.draw_candidates(wb.loss_plan)), all_embeds)

    def _samples_from_plan(self, wb):
        """Reference-shaped samples [(triples, neg_tail, neg_head)] per target graph from the batch's loss plan: the negatives
        of all graphs come from ONE temp_corrupt_sample launch (the per-graph torch-op sampler costs ~1.4 ms per graph)."""
        plan = wb.loss_plan
        cand = self.draw_candidates(plan)
        if cand is None:                             # --all-entity-loss: the positives alone
            return [(torch.from_numpy(trip), None, None) for trip in plan["triples"]]
        out = []
        for trip, (a0, _) in zip(plan["triples"], plan["splits"]):
            P = trip.shape[0]
            out.append((torch.from_numpy(trip), cand[a0:a0 + P], cand[a0 + P:a0 + 2 * P]))
        return out

    def draw_samples(self, wb):
        """Negative samples of every target graph of a prepared batch.  On a GPU the draws and the true-triple filter
        run on the device (sampling.DeviceCorruptTriples); `use_device_sampler = False` keeps the host sampler."""
        dev = self._device()
        c = self.corrupter
        if dev.type == "cuda" and getattr(self, "use_device_sampler", True):
            from .sampling import DeviceCorruptTriples
            dc = getattr(self, "_dev_corrupter", None)
            if dc is None or dc.device != dev:
                dc = self._dev_corrupter = DeviceCorruptTriples(self.args, self.graph_dict_train, dev, seed=getattr(self.args, "seed", None))
            c = dc
        return [c.single_graph_negative_sampling(wb.rows[i][-1], g, self.num_ents)[:3] for i, g in enumerate(wb.graphs)]

    def _all_frame(self, wb, rep):
        """What every map of the all-entity pass starts from -> (act (B, N) the active entities of every window, n_out and off_out the
        encoder output's row count and window offsets, tab (B, N) every pair's row of the table, T the table's row count); sets
        wb.all_rep, wb.all_rep_ids / all_rep_inv, wb.n_inactive and clears wb.all_time."""
        dev = self._device()
        N, B = self.num_ents, len(wb.graphs)
        # rep (the self-loop dropout draws): the reference runs forward_isolated per window, each with its own mask
        # (models/DynamicRGCN.py:56-64, models/RGCN.py:78-89), so nothing of the isolated pass is shared between windows: the
        # once-per-entity table becomes a (window, entity) table of B * N_ents rows -- the kernels' masks are a function of
        # (seed, row, column), so ONE launch over those rows gives every window its own mask
        T = B * N if rep else N
        tab = (np.arange(B * N, dtype=np.int64).reshape(B, N) if rep else np.broadcast_to(np.arange(N, dtype=np.int64)[None, :], (B, N)))
        wb.all_rep = rep
        if rep:
            ids = np.tile(np.arange(N, dtype=np.int32), B)
            wb.all_rep_ids = _lib.to_device(ids, dev)
            wb.all_rep_inv = TF.gather_inverse(ids, N, dev)
        act = np.zeros((B, N), dtype=bool)
        sizes = [g.n for g in wb.graphs]
        for b, g in enumerate(wb.graphs):
            act[b, g.gids] = True
        wb.n_inactive = int(B * N - act.sum())
        wb.all_time = None
        return act, int(sum(sizes)), np.concatenate([[0], np.cumsum(sizes)]), tab, T

    def _all_asm(self, wb, has, frame):
        """has (B, N): the (window, entity) pairs with rows of their own, window-major -> (asm (B, N), n_src): the map that assembles
        every window's entities from the n_src rows [encoder output ; pair rows ; table]."""
        _, n_out, off_out, tab, T = frame
        n_prev = int(has.sum())
        asm = (n_out + n_prev + tab).copy()
        asm[has] = n_out + np.arange(n_prev)
        for b, g in enumerate(wb.graphs):
            asm[b, g.gids] = off_out[b] + np.arange(g.n)
        return asm, n_out + n_prev + T

    def _all_maps(self, wb):
        """Row maps of the batched all-entity pass (get_all_embeds_Gt for every window at once), cached on the batch.
        An entity of window b falls in one of three classes:
          active in b's target graph      -> its row of the encoder output (models/DynamicRGCN.py:60-63);
          inactive, with a previous state -> one row of a GRU pass over exactly those (window, entity) pairs;
          inactive, never seen in the window's history (previous state 0, the vast majority at ICEWS scale)
                                          -> GRU(x_e, 0), which does not depend on the window: row e of ONE N_ents-row table.
        Per chain plan (direction): the pairs with a previous state (entity, history row, time gap) and the map that assembles
        the (B, N_ents) rows from [encoder output ; pair rows ; table]; for the second direction of a bidirectional encoder
        the active rows map to -1 (the encoder output already holds both directions' sum)."""
        rep = self._all_rep()
        if getattr(wb, "all_maps", None) is None or getattr(wb, "all_rep", False) != rep:
            dev = self._device()
            N, B = self.num_ents, len(wb.graphs)
            plans = wb.plan if isinstance(wb.plan, tuple) else (wb.plan,)
            L = plans[0].seq_len
            frame = act, n_out, off_out, tab, T = self._all_frame(wb, rep)
            if self.ent_encoder.use_time_embedding and self._chain_time_embedding and wb.n_inactive:
                # forward_isolated adds time_embed_2[t_b] to all rows of window b, then the active rows are overwritten with the
                # encoder's (models/RRGCN.py:214-216, models/DynamicRGCN.py:60-63): the inactive rows' table row, -1 on the active ones
                rows_t = np.where(act, -1, np.array([int(r[-1]) for r in wb.rows], dtype=np.int64)[:, None]).reshape(-1)
                wb.all_time = offset_tables(rows_t, self.ent_encoder.layer_2.time_embed.shape[0], dev)
            host, meta = {}, []
            for d, plan in enumerate(plans):
                _lib.pause_point()
                row_of = np.stack([plan.final_all(b, L - 1)[0] for b in range(B)])
                gap = np.stack([plan.final_all(b, L - 1)[1] for b in range(B)])
                has = ~act & (row_of >= 0)
                bb, ee = np.nonzero(has)                                   # window-major
                n_prev = int(bb.shape[0])
                if d == 0:
                    asm, n_src = self._all_asm(wb, has, frame)
                else:
                    asm = (n_prev + tab).copy()
                    asm[has] = np.arange(n_prev)
                    asm[act] = -1
                    n_src = n_prev + T
                if rep:
                    ee = bb * N + ee                                           # the pair's row of the (window, entity) table
                host["ent%d" % d], host["idx%d" % d], host["asm%d" % d] = ee, row_of[bb, ee % N], asm.reshape(-1)
                host["dt%d" % d] = gap[bb, ee % N].astype(np.float32).view(np.int32)       # float bits ride in the int32 pack
                meta.append((n_prev, n_src, ee, asm.reshape(-1), row_of[bb, ee % N]))
            _lib.pause_point()
            dd = S.upload_packed(host, dev, np.int32)
            wb.all_maps = []
            for d, (n_prev, n_src, ee, asm, idx_host) in enumerate(meta):
                wb.all_maps.append(dict(n_prev=n_prev, ent=dd["ent%d" % d], idx=dd["idx%d" % d], dt=dd["dt%d" % d].view(torch.float32).view(-1, 1), idx_host=idx_host,
                                        asm=dd["asm%d" % d], ent_inv=TF.gather_inverse(ee, T, dev) if n_prev else None,
                                        asm_inv=TF.gather_inverse(asm, n_src if wb.n_inactive else n_out, dev)))
        return wb.all_maps

    @staticmethod
    def _pair_inverse(m, key, prev):
        """Inverse of the pairs' history-row map m[key] over the rows of `prev` (a (window, entity) pair continues from its OWN
        last history row, so the map is injective): the adjoint of the previous-state gather is then a gather
        (TF.gru_step prev_inv).  Built on first use, cached on the batch's map; None if the rows repeat after all."""
        c = m.setdefault("_inv", {})
        k = (key, int(prev.shape[0]))
        if k not in c:
            c[k] = TF.injective_inverse(m[key + "_host"], prev.shape[0], prev.device)
        return c[k]

    @staticmethod
    def _rows_inverse(cache, key, idx_host, H):
        """gather_inverse of a static history-row list over the rows of H, built on first use and kept with the prepared batch."""
        if H is None:
            return None
        k = (key, int(H.shape[0]))
        if k not in cache:
            cache[k] = TF.gather_inverse(idx_host, H.shape[0], H.device)
        return cache[k]

    # the head and tail every all_embeds_batched variant shares (m = the first map of _all_maps)
    def _all_from_rows(self, wb, rows, m):
        """(B, N_ents, D) through m's assembly map from `rows` (the encoder output alone when every entity is active in its window)."""
        big = TF.gather_rows(rows, m["asm"], m["asm_inv"])
        return big.view(len(wb.graphs), self.num_ents, big.shape[1])

    def _all_table_input(self, wb):
        """The entity table the isolated pass starts from: one row per entity, per (window, entity) while the dropout draws."""
        return TF.gather_rows(self.ent_embeds, wb.all_rep_ids, wb.all_rep_inv) if wb.all_rep else self.ent_embeds

    def _all_assemble(self, wb, parts, m):
        return self._all_from_rows(wb, torch.cat(parts, dim=0), m)

    def _assemble_all(self, wb, out, isolated):
        """-> (B, N_ents, D): per window the active rows from `out` (concatenated target rows), the rest from the
        isolated pass (None when every entity is active in its window's target graph).  One gather through a static map."""
        src = out if isolated is None else torch.cat([out, isolated], dim=0)
        big = TF.gather_rows(src, wb.assemble, wb.assemble_inv)
        return big.view(len(wb.graphs), self.num_ents, big.shape[1])

    def _isolated_rnns(self, hist):
        """[(GRU, final history of its direction)] of the recurrent layer."""
        return [(self.ent_encoder.layer_2.rnn, hist[1])]

    def _fused_all_entity_ok(self, wb):
        """The batched all-entity pass + fused loss apply: always on the batched path; on the reference-granular path when the
        model is the unidirectional GRU encoder with BOTH layers recurrent (the reference's default flags), where the entity
        classes of _all_maps carry over to the first layer as well."""
        enc = self.ent_encoder
        # (while the self-loop dropout draws the isolated pass runs over (window, entity) rows, every window with its own mask:
        #  _all_rep / _all_maps -- the reference's default is dropout 0.1, utils/args.py:17)
        # (--use-time-embedding: on the batched path of the classes whose all_embeds_batched adds it, see _chain_time_embedding)
        temb = not enc.use_time_embedding or (wb.batched and self._chain_time_embedding)
        plain = temb and not getattr(self.args, "use_embed_for_non_active", False) and getattr(enc.layer_2, "num_layers", 1) == 1
        if wb.batched:
            return plain
        return (plain and self.use_batched_path and not isinstance(wb.plan, tuple) and isinstance(enc.layer_1, GRRGCNLayer)
                and isinstance(enc.layer_2, GRRGCNLayer) and not (enc.layer_1._extra() or enc.layer_2._extra()))

    def _all_rep(self):
        """The batched all-entity pass keeps one row per (window, entity) instead of one per entity: while the dropout draws
        (`_force_all_rep`: tests compare the two layouts without dropout)."""
        return bool(self._dropout_active() or getattr(self, "_force_all_rep", False))

    def _zero_state_rows(self, rnn, x, layer):
        """GRU(x, 0) over all rows of x: input-gate GEMM + pointwise cell (gru_chain.zero_state_program); the general
        single-step kernel would still run its recurrent GEMM and d_prev / d_W_hh products on zeros."""
        if getattr(rnn, "num_layers", 1) != 1:
            N = x.shape[0]
            return run_rnn(rnn, x, x.new_zeros(1, x.shape[1]), x.new_zeros(N, 1), layer.inv_temperature, layer.decay_spec(),
                           torch.full((N,), -1, dtype=torch.int32, device=x.device))
        progs = self.__dict__.setdefault("_zero_progs", {})
        prog = progs.get(x.shape[0])
        if prog is None:
            prog = progs[x.shape[0]] = zero_state_program(x.shape[0])
        return gru_chain(x, prog, [rnn], layer.inv_temperature, isinstance(rnn, GRUCell), want=[0])[0]

    def all_embeds_batched(self, wb, out, hist):
        """get_all_embeds_Gt for ALL windows at once (models/DynamicRGCN.py:56-64; Bi: models/BiDynamicRGCN.py:102-112,
        models/BiRRGCN.py:65-82).  The isolated RGCN trunk e -> Iso2(Iso1(e)) does not depend on the window, so it runs ONCE
        over the N_ents entities; so does every GRU from a zero state.  Only the (window, entity) pairs that carry a previous
        state get their own GRU rows (see _all_maps) -- through BOTH layers when the first one is recurrent too
        (rec_only_last_layer = False: y1 = GRU_1(Iso1(e), prev), y2 = GRU_2(Iso2(y1), prev), models/RRGCN.py:234-253).
        `out` = the concatenated target rows of the encoder.  Returns (B, N_ents, D)."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        maps = self._all_maps(wb)
        if wb.n_inactive == 0:
            return self._all_from_rows(wb, out, maps[0])
        if self._linear_layer():
            return self._all_embeds_batched_linear(wb, out, hist, maps)
        l1_rec = isinstance(l1, GRRGCNLayer)
        iso1 = l1.conv_isolated(self._all_table_input(wb))
        t1 = self._zero_state_rows(l1.rnn, iso1, l1) if l1_rec else iso1
        x = l2.conv_isolated(t1)
        lam, dec = l2.inv_temperature, l2.decay_spec()
        big = None
        for d, (m, (rnn, H)) in enumerate(zip(maps, self._isolated_rnns(hist))):
            parts = [out] if d == 0 else []
            if m["n_prev"]:
                if l1_rec:                                    # the pair's own first-layer state, then the second layer's input
                    y1p = run_rnn(l1.rnn, TF.gather_rows(iso1, m["ent"], m["ent_inv"]), hist[0], m["dt"], l1.inv_temperature, l1.decay_spec(), m["idx"],
                                  self._pair_inverse(m, "idx", hist[0]))
                    xp = l2.conv_isolated(y1p)
                else:
                    xp = TF.gather_rows(x, m["ent"], m["ent_inv"])
                parts.append(run_rnn(rnn, xp, H, m["dt"], lam, dec, m["idx"], self._pair_inverse(m, "idx", H)))
            parts.append(self._zero_state_rows(rnn, x, l2))                      # GRU(x_e, 0): one row per entity, every window
            g = self._all_assemble(wb, parts, m)
            big = g if big is None else big + g
        if enc.use_time_embedding:                   # once per window, after the directions are summed; the active rows carry it from `out`
            big = big + TF.gather_rows(l2.time_embed, wb.all_time[0], wb.all_time[1]).view_as(big)
        return big

    def _all_embeds_batched_linear(self, wb, out, hist, maps):
        """The isolated pass of the linear recurrence (RRGCNLayer.forward_isolated) for all windows at once: x = pre2(Iso1(E)) once per
        entity (per (window, entity) while the dropout draws); an inactive entity without a previous state gets act(x[e]), a (window,
        entity) pair with one act(x[e] + decay_rows(linear_nt(H[idx], W), dt, lam)); the active rows come from `out`.  With both layers
        recurrent a pair runs through both: y1p = act(Iso1(E)[e] + dec (h1[idx] . Wt1)), then act(pre_isolated2(y1p) + dec (h2[idx] . Wt2))."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        (m,), H = maps, hist[1]
        l1_rec = isinstance(l1, RRGCNLayer)               # both layers recurrent (_run_lin_stack): hist = (h1, h2) of the last history position
        E = self._all_table_input(wb)
        iso1 = l1.pre_isolated(E) if l1_rec else None
        x = l2.pre_isolated(l1.finish_rows(iso1, None, None, None) if l1_rec else l1.conv_isolated(E))
        parts = [out]
        if m["n_prev"]:                                   # static per prepared batch: the deterministic adjoint of the history gather
            inv = self._rows_inverse(m.setdefault("_gather_inv", {}), "idx", m["idx_host"], H)
        if m["n_prev"] and l1_rec:
            # the pair's own first-layer state, then the second layer on it: one lin_step_rows node per layer (one map serves both)
            act1, act2 = (1 if l.relu_fused() else 0 for l in (l1, l2))
            y1p = TF.lin_step_rows(iso1, m["ent"], hist[0], m["idx"], m["dt"], l1.inv_temperature, l1.time_weight, act1, m["ent_inv"], inv)
            parts.append(TF.lin_step_rows(l2.pre_isolated(y1p), None, H, m["idx"], m["dt"], l2.inv_temperature, l2.time_weight, act2, None, inv))
        elif m["n_prev"]:
            prev = TF.gather_rows(H, m["idx"], inv)
            parts.append(l2.finish_rows(TF.gather_rows(x, m["ent"], m["ent_inv"]), prev, None, m["dt"]))
        parts.append(l2.finish_rows(x, None, None, None))
        return self._all_assemble(wb, parts, m)

    def run_loss(self, wb, samples=None):
        """Encoder pass + the per-window link-prediction losses (summed, as the reference does)."""
        out, hist = self.run(wb)
        per_graph = list(out.split(wb.target.sizes))
        batched = self._fused_all_entity_ok(wb)
        all_list = self.all_embeds_batched(wb, out, hist) if batched else None
        if samples is None and batched and getattr(wb, "loss_plan", None) is not None:
            fused = self._sampled_loss(wb, out, all_list)
            if fused is not None:
                return fused
        if samples is None:
            samples = self._samples_from_plan(wb) if getattr(wb, "loss_plan", None) is not None else self.draw_samples(wb)
        if batched:
            fused = self.batched_link_prediction(out, self.cached_loss_inputs(wb, "_loss_inputs", samples, wb.target.sizes), all_list)
            if fused is not None:
                return fused
        times = [r[-1] for r in wb.rows]
        return self.per_graph_loss(times, wb.graphs, samples, per_graph.__getitem__, lambda i: (
            all_list[i] if batched else self.get_all_embeds_Gt(per_graph[i], wb.graphs[i], times[i], wb.plan, i, hist)))
