"""BiDynamicRGCN -- the bi-directional window model with the reference's interface
(models/BiDynamicRGCN.py:10-208).  A forward chain over [t-L+1 .. t-1] (forward_rnn) and a backward
chain over [t+L-1 .. t+1] (backward_rnn) feed the centre step
    H = GRU_f(Y2, dec(S_f)) + GRU_b(Y2, dec(S_b))            (models/BiRRGCN.py:27-47).
The batched path runs the 2 RGCN layers of all 2(L-1)+1 positions x bsz windows as one launch
each; only the GRU cells walk the two chains.
"""
import numpy as np
import torch

from . import functional as TF
from . import _lib
from . import snapshot as S
from .birrgcn import BiGRRGCNLayer, BiRRGCN, BiRRGCNLayer
from .dynamic_rgcn import DynamicRGCN, WindowBatch
from .gru_cell import GRUCell
from .gru_chain import GruInstance, GruProgram, gru_chain, chain_kernels_usable, offset_tables, rows_in_place_usable
from .lin_chain import linear_chain
from .rrgcn import run_rnn
from .window import ChainPlan, Step, window_times


class BiDynamicRGCN(DynamicRGCN):
    def build_model(self):
        self.ent_encoder = BiRRGCN(self.args, self.hidden_size, self.embed_size, self.num_rels, self.total_time)

    _linear_layer_class = BiRRGCNLayer

    def _can_batch(self):
        enc = self.ent_encoder
        if not (self.use_batched_path and enc.rec_only_last_layer):
            return False
        if self._linear_layer():                  # --module BiRRGCN: DynamicRGCN._can_batch_linear's conditions
            return self._can_batch_linear()
        return (isinstance(enc.layer_2, BiGRRGCNLayer)
                and not (enc.layer_2.post_aggregation or enc.layer_2.post_ensemble or enc.layer_2.impute))

    @staticmethod
    def get_batch_graph_list(t_list, seq_len, graph_dict):
        """models/BiDynamicRGCN.py:17-49 -> (g_fwd[p][b], t_fwd[p][b], g_bwd[p][b], t_bwd[p][b])."""
        times = list(graph_dict.keys())
        out = []
        for asc in (False, True):
            rows = window_times(t_list, seq_len, times, ascending=asc)
            tb = [list(x) for x in zip(*rows)]
            gb = [[graph_dict[t] if t is not None else None for t in col] for col in tb]
            out += [gb, tb]
        return tuple(out)

    # -- reference-granular path ------------------------------------------------------------------------
    def _encode_step_one_direction(self, st, prev_first, prev_second, forward):
        dev = self._device()
        ids, pidx, dt = st.tensors(dev)
        g = st.batched()
        g.ndata['h'] = TF.gather_rows(self.ent_embeds, ids)
        fp = self._gather_prev(prev_first, pidx, st.n_rows)
        sp = self._gather_prev(prev_second, pidx, st.n_rows)
        return self.ent_encoder.forward_one_direction(g, fp, sp, dt, st.times, st.sizes, forward)

    def pre_forward(self, plan, forward=True):
        first = second = None
        for st in plan.steps:
            first, second = self._encode_step_one_direction(st, first, second, forward)
        return first, second

    def _bi_target(self, plan_f, plan_b, rows, graphs):
        L = plan_f.seq_len
        st = self._target_step(plan_f, rows, graphs)
        pidx, dts = [], []
        for b, g in enumerate(graphs):
            a, d = plan_b.final_prev(b, g.gids, L - 1)
            pidx.append(a)
            dts.append(d)
        st_b = Step(L - 1, st.windows, graphs, st.times)
        st_b.prev_idx = np.concatenate(pidx) if pidx else np.zeros(0, np.int64)
        st_b.dt = np.concatenate(dts) if dts else np.zeros(0, np.float32)
        st_b.graph = None
        return st, st_b

    def _run_generic(self, wb):
        dev = self._device()
        plan_f, plan_b = wb.plan
        tf, tb = wb.target, wb.target_b
        hf = self.pre_forward(plan_f, True)
        hb = self.pre_forward(plan_b, False)
        ids, pf, dtf = tf.tensors(dev)
        _, pb, dtb = tb.tensors(dev)
        g = tf.batched()
        g.ndata['h'] = TF.gather_rows(self.ent_embeds, ids)
        n = tf.n_rows
        out = self.ent_encoder(g, self._gather_prev(hf[0], pf, n), self._gather_prev(hf[1], pf, n), dtf,
                               self._gather_prev(hb[0], pb, n), self._gather_prev(hb[1], pb, n), dtb, tf.times, tf.sizes)
        return out, (hf, hb)

    # -- batched path --------------------------------------------------------------------------------------
    def _chain_weights(self):
        l2 = self.ent_encoder.layer_2
        return [l2.time_weight_forward, l2.time_weight_backward]

    def _run_batched_linear(self, wb):
        """--module BiRRGCN: layer 2's aggregation + self-loop of every visit at once, both directions' history positions as ONE
        linear_chain node (forward history on weight 0, backward history on weight 1, ReLU), and the centre position on the per-row
        operators: out = relu(pre_t + decay(Hf[pf] . W_f) + decay(Hb[pb] . W_b)) -- the ReLU follows the sum, so the centre is not
        two cells of the chain whose outputs could be added."""
        enc, dev = self.ent_encoder, self._device()
        plan_f, plan_b = wb.plan
        tf, tb = wb.target, wb.target_b
        l2 = enc.layer_2
        y1 = enc.layer_1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        y2 = l2.pre(wb.g_all, y1)
        if wb.visit_rows is not None:                         # distinct-snapshot rows -> visit rows
            y2 = TF.gather_rows(y2, wb.visit_rows, getattr(wb, "visit_inv", None))
        wb.last_x = None
        if wb.program is not None:
            x_hist, pre_t = TF.row_spans(y2, [(0, tf.row0), (tf.row0, tf.n_rows)])
            want = self._chain_want(wb)
            got = {}
            if want:
                got = dict(zip(want, linear_chain(x_hist, wb.program, self._chain_weights(), l2.inv_temperature, 1 if l2.relu_fused() else 0,
                                                  want=want)))
            Hf, Hb = got.get(wb.hist_inst[0]), got.get(wb.hist_inst[1])
        else:
            order = sorted([(st.row0, st.n_rows) for st in list(plan_f.steps) + list(plan_b.steps)] + [(tf.row0, tf.n_rows)])
            x_of = dict(zip(order, TF.row_spans(y2, order)))

            def chain(plan, forward):
                H = None
                for st in plan.steps:
                    _, pidx, dt = st.tensors(dev)
                    H = l2.finish_rows(x_of[(st.row0, st.n_rows)], H, pidx, dt, forward)
                return H

            Hf, Hb = chain(plan_f, True), chain(plan_b, False)
            pre_t = x_of[(tf.row0, tf.n_rows)]
        _, pf, dtf = tf.tensors(dev)
        _, pb, dtb = tb.tensors(dev)
        if self._bi_pair(wb):                                 # both gathers, products and decays, the sum and the ReLU as ONE node
            inv = self._centre_inverses(wb, Hf, Hb)
            out = TF.lin_step_rows2(pre_t, None, Hf, pf, dtf, Hb, pb, dtb, l2.inv_temperature, l2.time_weight_forward, l2.time_weight_backward,
                                    1 if l2.relu_fused() else 0, None, inv[0], inv[1])
        else:
            out = l2.centre_rows(pre_t, Hf, pf, dtf, Hb, pb, dtb)
        return out, ((Hf, Hf), (Hb, Hb))

    # --module BiRRGCN on the batched linear path: the all-entity pass of all windows at once over the UNION of (window, entity) pairs
    # with a previous state in either direction (_union_maps), the fused loss node and the batched evaluation path that go with it, and
    # the centre position as one lin_step_rows2 node.  Off by default: the per-window call lists of the existing suites pin that route
    bi_pair_pass = False

    def _bi_pair(self, wb):
        return bool(getattr(self, "bi_pair_pass", False) and wb.batched and self._linear_layer())

    def _centre_inverses(self, wb, Hf, Hb):
        cache = wb.__dict__.setdefault("_centre_inv", {})
        return (self._rows_inverse(cache, "f", wb.target.prev_idx, Hf), self._rows_inverse(cache, "b", wb.target_b.prev_idx, Hb))

    def _run_batched(self, wb):
        if self._linear_layer():
            return self._run_batched_linear(wb)
        enc, dev = self.ent_encoder, self._device()
        plan_f, plan_b = wb.plan
        tf, tb = wb.target, wb.target_b
        y1 = enc.layer_1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        l2 = enc.layer_2
        lam, dec = l2.inv_temperature, l2.decay_spec()
        if wb.program is not None:
            prog = wb.program
            want = self._chain_want(wb)
            # y2 = relu(.) (models/BiRRGCN.py:202-203) is read by ONE consumer here, the gather into chain order: the ReLU's
            # adjoint rides in that gather's backward (one pass less over the (n, d) gradient)
            # (support is decided BEFORE the conv: ONE flag drops the mask from the layer's backward and hands it to the gather's)
            fold = l2.relu_fused() and TF.relu_gather_supported(l2.out_feat, wb.chain_inv)
            y2 = l2.conv(wb.g_all, y1, grad_premasked=fold)
            # (the gather also hands out the magnitude keys of the rows it writes: the f16 products of the chain scale x by them)
            keyed = TF.gather_keys_supported(y2.shape[1]) and chain_kernels_usable(y2.shape[1], 2)
            x_keys = None
            type1, off = isinstance(l2.forward_rnn, GRUCell), self._chain_offset(wb)
            if keyed and self.rows_in_place and rows_in_place_usable(prog, y2, wb.chain_inv, 2, type1, want, dec, off):
                # the chain reads its rows of y2 where they lie: no copy into chain order (and none in wb.last_x)
                wb.last_x = None
                got = dict(zip(want, gru_chain(None, prog, [l2.forward_rnn, l2.backward_rnn], lam, type1, want=want,
                                               table=(y2, wb.chain_rows, wb.chain_inv, fold))))
            elif keyed:
                wb.last_x, x_keys = TF.gather_rows(y2, wb.chain_rows, wb.chain_inv, relu_table=fold, keys=True)
            else:
                wb.last_x = TF.gather_rows(y2, wb.chain_rows, wb.chain_inv, relu_table=fold)      # GRU input rows in chain order
            if wb.last_x is not None:
                got = dict(zip(want, gru_chain(wb.last_x, prog, [l2.forward_rnn, l2.backward_rnn], lam, type1, want=want, x_keys=x_keys,
                                               decay=dec, offset=off)))
            out = got[wb.out_inst[0]] + got[wb.out_inst[1]]
            if enc.use_time_embedding:                        # the centre step adds it ONCE to h_f + h_b (models/BiRRGCN.py:221-225)
                out = out + TF.gather_rows(l2.time_embed, wb.target_time[0], wb.target_time[1])
            Hf, Hb = got.get(wb.hist_inst[0]), got.get(wb.hist_inst[1])
            return out, ((Hf, Hf), (Hb, Hb))
        y2 = l2.conv(wb.g_all, y1)                            # ReLU fused (models/BiRRGCN.py:202-203)
        if wb.visit_rows is not None:                         # distinct-snapshot rows -> visit rows
            y2 = TF.gather_rows(y2, wb.visit_rows, getattr(wb, "visit_inv", None))
        wb.last_x = y2

        # every position's rows of y2 (forward steps, backward steps, target rows) from ONE split (TF.row_spans)
        order = sorted([(st.row0, st.n_rows) for st in list(plan_f.steps) + list(plan_b.steps)] + [(tf.row0, tf.n_rows)])
        x_of = dict(zip(order, TF.row_spans(y2, order)))

        def chain(plan, rnn):
            H = None
            for st in plan.steps:
                _, pidx, dt = st.tensors(dev)
                x = x_of[(st.row0, st.n_rows)]
                prev = H if H is not None else x.new_zeros(1, x.shape[1])
                H = run_rnn(rnn, x, prev, dt, lam, dec, pidx)
                if enc.use_time_embedding:
                    H = H + l2.get_time_embedding(st.times, st.sizes)
            return H

        Hf = chain(plan_f, l2.forward_rnn)
        Hb = chain(plan_b, l2.backward_rnn)
        x = x_of[(tf.row0, tf.n_rows)]
        _, pf, dtf = tf.tensors(dev)
        _, pb, dtb = tb.tensors(dev)
        zero = x.new_zeros(1, x.shape[1])
        out = run_rnn(l2.forward_rnn, x, Hf if Hf is not None else zero, dtf, lam, dec, pf) + \
            run_rnn(l2.backward_rnn, x, Hb if Hb is not None else zero, dtb, lam, dec, pb)
        if enc.use_time_embedding:
            out = out + l2.get_time_embedding(tf.times, tf.sizes)
        return out, ((Hf, Hf), (Hb, Hb))

    def _chain_rows_host(self, wb):
        return wb.chain_rows_np

    def _chain_rnns(self):
        l2 = self.ent_encoder.layer_2
        return [l2.forward_rnn, l2.backward_rnn]

    def _chain_want(self, wb):
        return [i for i in (wb.out_inst[0], wb.out_inst[1], wb.hist_inst[0], wb.hist_inst[1]) if i >= 0]

    def _chain_offset_index(self, wb):
        """Program order [forward history | target | backward history | target]: the history rows of each direction add their own
        position's row (forward_one_direction, models/BiRRGCN.py:236-239); the two centre cells add none -- their sum gets it once."""
        plan_f, plan_b = wb.plan
        none = np.full(wb.target.n_rows, -1, dtype=np.int64)
        return np.concatenate([self._step_time_rows(st) for st in plan_f.steps] + [none] + [self._step_time_rows(st) for st in plan_b.steps] + [none])

    def _visit_rows_on_device(self):
        # the GRU chain program gathers by its own row list (chain_rows, _build_program); the linear one reads the visit rows
        return self._linear_layer() or not self._can_chain()

    def _build_program_linear(self, wb):
        """--module BiRRGCN: the history positions of both directions, forward on weight 0 and backward on weight 1, in visit order
        [forward history | backward history] (x row = chain row); the centre position stays outside the chain (_run_batched_linear)."""
        plan_f, plan_b = wb.plan
        assert wb.target.row0 == sum(st.n_rows for st in plan_f.steps) + sum(st.n_rows for st in plan_b.steps)
        inst, hist = [], []
        for w, plan in enumerate((plan_f, plan_b)):
            last = -1
            for st in plan.steps:
                inst.append(GruInstance(st.n_rows, st.row0, w, last, st.prev_idx, st.dt, st.next_idx))
                last = len(inst) - 1
            hist.append(last)
        wb.program = GruProgram(inst)
        wb.out_inst = [-1, -1]
        wb.hist_inst = hist

    def _build_program(self, wb):
        """Chain program with ONE contiguous row range per direction: x rows are laid out
        [forward history | target | backward history | target (second copy)] and the instances follow the
        same order, so each direction's input-gate GEMM, d_x GEMM and weight-gradient GEMMs run once over
        all of its 15 positions (the copy costs one row gather; its gradient is summed by the gather's
        backward)."""
        if self._linear_layer():
            return self._build_program_linear(wb)
        plan_f, plan_b = wb.plan
        tf, tb = wb.target, wb.target_b
        nf = sum(st.n_rows for st in plan_f.steps)
        nb = sum(st.n_rows for st in plan_b.steps)
        nt = tf.n_rows
        total = nf + nb + nt
        base = wb.visit_rows_host.astype(np.int64) if wb.visit_rows_host is not None else np.arange(total, dtype=np.int64)
        assert base.shape[0] == total and tf.row0 == nf + nb
        f_rows = base[:nf]
        b_rows = base[nf:nf + nb]
        t_rows = base[tf.row0:tf.row0 + nt]
        chain = np.concatenate([f_rows, t_rows, b_rows, t_rows])
        wb.chain_rows = _lib.to_device(chain.astype(np.int32), self._device())
        wb.chain_rows_np = chain
        wb.chain_inv = TF.gather_inverse(chain, int(wb.g_all.n), self._device())
        _lib.pause_point()
        inst = []
        last = -1
        for st in plan_f.steps:
            inst.append(GruInstance(st.n_rows, st.row0, 0, last, st.prev_idx, st.dt, st.next_idx))
            last = len(inst) - 1
        inst.append(GruInstance(nt, nf, 0, last, tf.prev_idx, tf.dt))
        hist_f, out_f = last, len(inst) - 1
        last = -1
        for st in plan_b.steps:
            inst.append(GruInstance(st.n_rows, st.row0 + nt, 1, last, st.prev_idx, st.dt, st.next_idx))      # backward rows sit after the target copy
            last = len(inst) - 1
        inst.append(GruInstance(nt, nf + nt + nb, 1, last, tb.prev_idx, tb.dt))
        hist_b, out_b = last, len(inst) - 1
        wb.program = GruProgram(inst)
        wb.program.x_src = chain                  # x row i is layer-output row chain[i]: the input gates are computed once per
                                                  # distinct row of a direction (GruProgram.gi_shared)
        assert len(wb.program.groups) <= 2
        wb.out_inst = [out_f, out_b]
        wb.hist_inst = [hist_f, hist_b]

    # ---------------------------------------------------------------------------------------------
    def prepare(self, t_list, seq_len, train=True, target_edge_ids=None):
        dev = self._device()
        wb = WindowBatch()
        wb.rows = window_times(t_list, seq_len, self.total_time)
        rows_b = window_times(t_list, seq_len, self.total_time, ascending=True)
        plan_f = ChainPlan(wb.rows, self.graph_dict_train, self.num_ents, seq_len)
        _lib.pause_point()                            # (between the stages of `prepare`: a prefetch worker parks here while the loop issues a step)
        plan_b = ChainPlan(rows_b, self.graph_dict_train, self.num_ents, seq_len).flipped()
        _lib.pause_point()
        wb.plan = (plan_f, plan_b)
        if train and self.random_dropout:
            self.sample_history_graphs(plan_f)
            self.sample_history_graphs(plan_b)
        wb.graphs = [self.graph_dict_train[r[-1]] for r in wb.rows]
        tgt = self.sample_target_graphs(wb.graphs, 0.5, target_edge_ids) if train else wb.graphs
        _lib.pause_point()
        wb.target, wb.target_b = self._bi_target(plan_f, plan_b, wb.rows, tgt)
        wb.batched = self._can_batch()
        wb.steps = plan_f.steps + plan_b.steps + [wb.target]
        _lib.pause_point()
        self._upload(wb, dev, train)
        _lib.pause_point()
        if wb.program is None or self._linear_layer():      # (the centre of the linear model runs on the per-row operators)
            wb.target.tensors(dev)
            wb.target_b.tensors(dev)
        elif self.ent_encoder.use_time_embedding:
            wb.target_time = offset_tables(self._step_time_rows(wb.target), self.ent_encoder.layer_2.time_embed.shape[0], dev)
        if train:
            self._plan_loss(wb)
        return wb

    def encode(self, t_list, seq_len, train=True, target_edge_ids=None):
        wb = self.prepare(t_list, seq_len, train, target_edge_ids)
        out, hist = self.run(wb)
        return list(out.split(wb.target.sizes)), wb.plan, wb.rows, wb.graphs, hist

    def _isolated_rnns(self, hist):
        l2 = self.ent_encoder.layer_2
        (Hf, _), (Hb, _) = hist
        return [(l2.forward_rnn, Hf), (l2.backward_rnn, Hb)]

    # -- reference-default flags (both layers recurrent): all-entity pass of all windows at once -------------------
    def _fused_all_entity_ok(self, wb):
        if wb.batched:
            # --module BiRRGCN: the ReLU follows the sum of the two directions' terms, so the pair sets of the directions interact and a
            # batched pass needs the union map (_union_maps): with bi_pair_pass the parent's rule, without it the
            # all-entity pass stays per window and the loss per graph
            return (self._bi_pair(wb) or not self._linear_layer()) and super()._fused_all_entity_ok(wb)
        enc = self.ent_encoder
        # (this variant keeps ONE isolated pass per entity: not while the self-loop dropout draws -- every window then needs its own mask)
        return (self.use_batched_path and not enc.use_time_embedding and not getattr(self.args, "use_embed_for_non_active", False)
                and isinstance(enc.layer_1, BiGRRGCNLayer) and isinstance(enc.layer_2, BiGRRGCNLayer) and not self._all_rep()
                and getattr(enc.layer_2, "num_layers", 1) == 1 and not (enc.layer_1._extra() or enc.layer_2._extra()))

    def _all_maps(self, wb):
        """Batched path: per-direction maps (DynamicRGCN._all_maps), with bi_pair_pass the union map.  Reference-granular path (both
        layers recurrent): the first layer's state of a (window, entity) pair depends on BOTH directions' previous states, so the
        pairs are the union as well (_union_maps)."""
        if wb.batched and not self._bi_pair(wb):
            return super()._all_maps(wb)
        return self._union_maps(wb)

    def _union_maps(self, wb):
        """bi_pair_pass, and the reference-granular path: ONE map over the union pairs -- inactive (window, entity) pairs with a
        previous state in EITHER direction, window-major, each with its two history rows (-1: no state in that direction) and time
        gaps; every other inactive entity takes its row of the table (one row per entity; on the batched path per (window, entity)
        while the self-loop dropout draws, as in DynamicRGCN._all_maps: `ent` then indexes those rows).  asm assembles [encoder
        output ; pair rows ; table]."""
        rep = wb.batched and self._all_rep()                               # (the reference-granular pass keeps one row per entity)
        if getattr(wb, "all_maps", None) is None or getattr(wb, "all_rep", False) != rep:
            dev = self._device()
            N, B = self.num_ents, len(wb.graphs)
            plan_f, plan_b = wb.plan
            L = plan_f.seq_len
            frame = act, n_out, _, _, T = self._all_frame(wb, rep)
            _lib.pause_point()
            fin_f = [plan_f.final_all(b, L - 1) for b in range(B)]
            fin_b = [plan_b.final_all(b, L - 1) for b in range(B)]
            rf, gf = np.stack([f[0] for f in fin_f]), np.stack([f[1] for f in fin_f])
            rb, gb = np.stack([f[0] for f in fin_b]), np.stack([f[1] for f in fin_b])
            has = ~act & ((rf >= 0) | (rb >= 0))
            bb, ee = np.nonzero(has)                                       # window-major
            n_prev = int(bb.shape[0])
            asm, n_src = self._all_asm(wb, has, frame)
            ent = bb * N + ee if rep else ee                               # the pair's row of the table
            host = dict(ent=ent, idx_f=rf[bb, ee], idx_b=rb[bb, ee], asm=asm.reshape(-1),
                        dt_f=gf[bb, ee].astype(np.float32).view(np.int32), dt_b=gb[bb, ee].astype(np.float32).view(np.int32))
            _lib.pause_point()
            d = S.upload_packed(host, dev, np.int32)
            f32 = lambda t: t.view(torch.float32).view(-1, 1)
            wb.all_maps = [dict(n_prev=n_prev, ent=d["ent"], idx_f=d["idx_f"], idx_b=d["idx_b"], dt_f=f32(d["dt_f"]), dt_b=f32(d["dt_b"]),
                                idx_f_host=host["idx_f"], idx_b_host=host["idx_b"], asm=d["asm"],
                                ent_inv=TF.gather_inverse(ent, T, dev) if n_prev else None,
                                asm_inv=TF.gather_inverse(asm.reshape(-1), n_src if wb.n_inactive else n_out, dev))]
        return wb.all_maps

    def _all_embeds_batched_union(self, wb, out, hist):
        """BiRRGCNLayer.forward_isolated for all windows at once: x = pre_isolated2(conv_isolated1(E)) once per entity (per (window,
        entity) while the dropout draws); an inactive entity without a previous state in either direction gets act(x[e]), a union pair
        act(x[e] + both directions' recurrent terms) through ONE lin_step_rows2 node; the active rows come from `out`."""
        l1, l2 = self.ent_encoder.layer_1, self.ent_encoder.layer_2
        (m,) = self._all_maps(wb)
        if wb.n_inactive == 0:
            return self._all_from_rows(wb, out, m)
        (Hf, _), (Hb, _) = hist
        x = l2.pre_isolated(l1.conv_isolated(self._all_table_input(wb)))
        parts = [out]
        if m["n_prev"]:
            cache = m.setdefault("_gather_inv", {})
            parts.append(TF.lin_step_rows2(x, m["ent"], Hf, m["idx_f"], m["dt_f"], Hb, m["idx_b"], m["dt_b"], l2.inv_temperature,
                                           l2.time_weight_forward, l2.time_weight_backward, 1 if l2.relu_fused() else 0, m["ent_inv"],
                                           self._rows_inverse(cache, "f", m["idx_f_host"], Hf), self._rows_inverse(cache, "b", m["idx_b_host"], Hb)))
        parts.append(l2._finish(x))
        return self._all_assemble(wb, parts, m)

    def all_embeds_batched(self, wb, out, hist):
        if wb.batched and self._bi_pair(wb):
            return self._all_embeds_batched_union(wb, out, hist)
        if wb.batched:
            return super().all_embeds_batched(wb, out, hist)
        # both layers recurrent (models/BiRRGCN.py:242-257): zero-state rows once per entity through both layers' GRU pairs,
        # own rows for the union pairs
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        (m,) = self._all_maps(wb)
        if wb.n_inactive == 0:
            return self._all_from_rows(wb, out, m)
        (f1, f2), (b1, b2) = hist
        iso1 = l1.conv_isolated(self._all_table_input(wb))
        t1 = self._zero_state_rows(l1.forward_rnn, iso1, l1) + self._zero_state_rows(l1.backward_rnn, iso1, l1)
        x2 = l2.conv_isolated(t1)
        parts = [out]
        if m["n_prev"]:
            zero = iso1.new_zeros(1, iso1.shape[1])

            def both(layer, x, pf, pb):
                lam, dec = layer.inv_temperature, layer.decay_spec()
                none = torch.full_like(m["idx_f"], -1)
                return run_rnn(layer.forward_rnn, x, pf if pf is not None else zero, m["dt_f"], lam, dec, m["idx_f"] if pf is not None else none,
                               self._pair_inverse(m, "idx_f", pf) if pf is not None else None) + \
                    run_rnn(layer.backward_rnn, x, pb if pb is not None else zero, m["dt_b"], lam, dec, m["idx_b"] if pb is not None else none,
                            self._pair_inverse(m, "idx_b", pb) if pb is not None else None)
            h1p = both(l1, TF.gather_rows(iso1, m["ent"], m["ent_inv"]), f1, b1)
            parts.append(both(l2, l2.conv_isolated(h1p), f2, b2))
        parts.append(self._zero_state_rows(l2.forward_rnn, x2, l2) + self._zero_state_rows(l2.backward_rnn, x2, l2))
        return self._all_assemble(wb, parts, m)

    def get_all_embeds_Gt(self, convoluted_embeds, g, t, plans, b, hist):
        """models/BiDynamicRGCN.py:102-112."""
        dev = self._device()
        plan_f, plan_b = plans
        hf, hb = hist
        L = plan_f.seq_len
        if getattr(self.args, "use_embed_for_non_active", False):
            all_embeds = self.ent_embeds
        else:
            def prevs(plan, h):
                row_of, dt = plan.final_all(b, L - 1)
                idx = torch.from_numpy(row_of.astype(np.int32)).to(dev)
                p1 = self._gather_prev(h[0], idx, self.num_ents)
                p2 = p1 if h[1] is h[0] else self._gather_prev(h[1], idx, self.num_ents)
                return p1, p2, torch.from_numpy(dt).view(-1, 1).to(dev)
            f1, f2, dtf = prevs(plan_f, hf)
            b1, b2, dtb = prevs(plan_b, hb)
            all_embeds = self.ent_encoder.forward_isolated(self.ent_embeds, f1, f2, dtf, b1, b2, dtb, t)
        gid = torch.from_numpy(g.gids).to(dev)
        return all_embeds.index_copy(0, gid, convoluted_embeds)
