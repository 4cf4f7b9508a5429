"""The frequency gates and the embedding-level gated loss of the `--post-aggregation` models -- what PostDynamicRGCN /
PostBiDynamicRGCN (post_dynamic_rgcn.py, GRU encoders) and PostSelfAttentionRGCN / PostBiSelfAttentionRGCN
(post_self_attention_rgcn.py, attention encoder) share.  Nothing here knows how the two streams of target rows and their
all-entity matrices were produced (no window.ChainPlan, no history layout): a model supplies `_target_sizes(wb)`, the prepared
batch's `rows` / `graphs`, and the streams themselves."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as TF


class _FrequencyGateMixin:
    """Per-timestamp frequency features of a triple (temp_amd/frequency.py), prediction through the gates, and the stacking of
    per-window all-entity matrices for a fused loss node."""

    def all_entity_tables(self, t_list):
        raise NotImplementedError("%s scores against two all-entity tables (local, temporal) mixed by per-triple gates: predict() covers the "
                                  "single-table models only" % type(self).__name__)

    # -- prediction through the gates -----------------------------------------------------------------------------------------
    _gate_count = 0                       # weights a query carries: 1 (score-level ensemble), 2 (embedding-level gate: known, candidates)

    def all_entity_table_pairs(self, t_list):
        """What `predict_gated` selects from: yields (t, all_loc [N_ents, D], all_rec [N_ents, D]) for every timestamp of `t_list`
        -- the two all-entity matrices the family's evaluate() ranks against (evaluation_targets), assembled over the train graph
        the encoder ran on."""
        if not self._gate_count:
            raise NotImplementedError("%s has one all-entity table and no gates: predict_gated() covers the two-table post models" % type(self).__name__)
        for t, _, all_embeds in self.evaluation_targets(t_list):
            yield (t,) + tuple(all_embeds(self.graph_dict_train[t]))

    def query_features(self, t, known, rel, mode):
        """Frequency features of the KNOWN side of queries at timestamp t (global ids), all a query has -> (Q, 3) on the device.
        tail (s, r, ?): the object features [agg_sub[s], agg_rel[r], agg_sub_rel[(s, r)]]; head (?, r, o): the subject features
        [agg_obj[o], agg_rel[r], agg_obj_rel[(o, r)]] -- the rows a training triple's object / subject MLP sees."""
        sub_f, obj_f = self.frequency_tables().features(int(t), known, rel, known)
        return torch.from_numpy(obj_f if mode == "tail" else sub_f).to(self._device())

    def _query_gates(self, t, known, rel, mode):
        """-> the `_gate_count` weights [Q] of the queries from the model's own frequency MLPs."""
        raise NotImplementedError

    def predict_gated(self, queries, mode="tail", k=10, filtered=True, weights=None):
        """`predict` for the models that score against two all-entity tables: the k best answers of every query under the gated
        score.  queries, mode, k, filtered and the returned (ids [Q, k] int64, scores [Q, k] float32, rows in query order) are
        TKG_Module.predict's.  weights: None for the model's own frequency MLPs on the known side of the query -- the pairing of the
        training loss: a tail query is gated by the object MLP(s), a head query by the subject MLP(s) (see _query_gates) -- or
        injected weights, the counterpart of forward(..., ensemble_weights= / gate_weights=): a [Q] tensor for the score-level
        ensemble, a pair (w_known [Q], w_cand [Q]) for the embedding-level gate.  The scorer is evaluate()'s (the real head / tail
        mode; head_scored_as_tail is a quirk of the training loss alone).  Adds no parameters or buffers."""
        q = self.query_rows("predict_gated", queries, mode)
        dev = self._device()
        if weights is not None:
            weights = (weights,) if torch.is_tensor(weights) else tuple(weights)
            if len(weights) != self._gate_count or any(not torch.is_tensor(w) or w.numel() != q.shape[0] for w in weights):
                raise ValueError("predict_gated: weights must be %s" % ("a [Q] tensor" if self._gate_count == 1 else "a pair (w_known [Q], w_cand [Q])"))
            weights = tuple(w.detach().to(dev, torch.float32).reshape(-1) for w in weights)
        ranker = self._ranker()

        def select(t, tables, known, rel, sel):
            gates = self._query_gates(t, known, rel, mode) if weights is None else tuple(w[sel] for w in weights)
            return ranker.topk_single_graph(*tables, self.rel_embeds, known, rel, *gates, mode, t, k, filtered, **self._topk_relation_kw())
        return self.select_per_timestamp(q, k, self.all_entity_table_pairs, select)

    def _topk_relation_kw(self):
        """Keyword arguments of the ranker's topk_single_graph beyond self.rel_embeds: a second relation table where the two streams
        are two models (Aggregator)."""
        return {}

    def frequency_tables(self):
        ft = getattr(self, "_freq_tables", None)
        if ft is None:
            from .frequency import FrequencyTables
            ft = self._freq_tables = FrequencyTables(self.graph_dict_train, self.train_seq_len, "Bi" in self.args.module,
                                                     2 * self.num_rels)
        return ft

    def ensemble_features(self, triples, t, g):
        """Frequency features of the (local-id) triples of graph g at timestamp t -> (subject (n, 3), object (n, 3)) on the device."""
        tr = triples.detach().cpu().numpy() if torch.is_tensor(triples) else np.asarray(triples)
        tr = tr.reshape(-1, 3)
        sub_f, obj_f = self.frequency_tables().features(int(t), g.gids[tr[:, 0]], tr[:, 1], g.gids[tr[:, 2]])
        dev = self._device()
        return torch.from_numpy(sub_f).to(dev), torch.from_numpy(obj_f).to(dev)

    def _stacked_alls(self, alls):
        """The (B * N_ents, D) stacks of the two streams' all-entity matrices for a fused node.  alls: per window (all_loc,
        all_rec), or the pair of (B, N_ents, D) tensors of batched_all_embeds_post as they are (no per-window slices: every slice
        is a zero-filled (B, N_ents, D) gradient and an addition in the backward)."""
        if isinstance(alls, tuple):
            return alls[0].reshape(-1, self.embed_size), alls[1].reshape(-1, self.embed_size)
        return torch.cat([a for a, _ in alls], dim=0), torch.cat([a for _, a in alls], dim=0)


class _GatedLossMixin(_FrequencyGateMixin):
    """What PostDynamicRGCN and PostBiDynamicRGCN add to the impute window models (models/PostDynamicRGCN.py:146-321,
    models/PostBiDynamicRGCN.py:179-282): four frequency MLPs, the EMBEDDING-level gate of the training loss and of evaluate().

    Loss per target graph (PostDynamicRGCN.train_link_prediction, models/PostDynamicRGCN.py:261-282), loss_tail + loss_head:
      tail rows: known subject w_oqs * s_loc + (1 - w_oqs) * s_rec, candidates w_oqo * all_loc[c] + (1 - w_oqo) * all_rec[c]
      head rows: known object = the TEMPORAL row alone (the reference's o_loc = o_rec = ent_embed_rec[o], :276-277: w_sqo has no
                 effect and no gradient), candidates w_sqs * all_loc[c] + (1 - w_sqs) * all_rec[c]
    DistMult and ComplEx are linear in the candidate: their fused node (functional.batched_gated_link_prediction) mixes the two score
    matrices at the candidate columns.  TransE's L1 distance is not: its node reads both all-entity rows of every candidate and
    mixes them in registers (temp_l1_mix_ce_fwd / _bwd_q / _bwd_table).  Reference quirk kept: w_sqo comes from subject_query_SUBJECT_embed_linear and w_oqo from
    object_query_SUBJECT_embed_linear (calc_ensemble_ratio, :284-321), so the two *_object_embed_linear MLPs never get a gradient."""
    _all_entity_loss_refusal = "the model gates a local AND a temporal all-entity table per candidate; the all-entity node takes one table"
    _evaluater = "PostEvaluationFilter"

    def init_freq_mlp(self):
        """PostDynamicRGCN.init_freq_mlp, models/PostDynamicRGCN.py:152-172 (same module names => same state_dict keys)."""
        mk = lambda: nn.Sequential(nn.Linear(3, 3), nn.ReLU(), nn.Linear(3, 1))
        self.subject_query_subject_embed_linear = mk()
        self.object_query_subject_embed_linear = mk()
        self.subject_query_object_embed_linear = mk()
        self.object_query_object_embed_linear = mk()

    def calc_ensemble_ratio(self, triples, t, g, features=None):
        """models/PostDynamicRGCN.py:284-321 -> (w_sqs, w_sqo, w_oqs, w_oqo), each (n, 1); empty tensors for no triples.
        features: the (subject (n, 3), object (n, 3)) device rows of ensemble_features, when the caller has them cached."""
        if len(triples) == 0:
            e = torch.zeros(0, dtype=torch.int64, device=self._device())
            return e, e, e, e
        sub_f, obj_f = features if features is not None else self.ensemble_features(triples, t, g)
        w_sqs = torch.sigmoid(self.subject_query_subject_embed_linear(sub_f))
        w_sqo = torch.sigmoid(self.subject_query_subject_embed_linear(sub_f))     # (sic: the subject-embed MLP)
        w_oqs = torch.sigmoid(self.object_query_subject_embed_linear(obj_f))
        w_oqo = torch.sigmoid(self.object_query_subject_embed_linear(obj_f))      # (sic)
        return w_sqs, w_sqo, w_oqs, w_oqo

    _gate_count = 2

    def _query_gates(self, t, known, rel, mode):
        """(w_known, w_cand) [Q] of queries, paired as in gated_loss: a tail query's known subject takes w_oqs and its candidates
        w_oqo, a head query's known object w_sqo and its candidates w_sqs -- with calc_ensemble_ratio's quirk, both weights of a
        mode are the *_subject_embed_linear MLP on the same features, hence one tensor."""
        mlp = self.object_query_subject_embed_linear if mode == "tail" else self.subject_query_subject_embed_linear
        w = torch.sigmoid(mlp(self.query_features(t, known, rel, mode))).reshape(-1)
        return w, w

    def _agg_features(self, wb, samples):
        """Per window the frequency feature rows of the sampled triples, computed and uploaded ONCE per (prepared batch, sample set):
        a step with fixed samples then issues no host-to-device copy and can be captured as a HIP graph."""
        return self.per_sample_set(wb, "_agg_feats", samples, lambda: [
            self.ensemble_features(samples[i][0], wb.rows[i][-1], g) if samples[i][0].shape[0] > 0 else None
            for i, g in enumerate(wb.graphs)])

    def _batched_gates(self, wb, samples):
        """(w_known, w_cand) of the stacked rows of the fused node ([tail rows ; head rows] per window) from the model's own MLPs.
        w_sqs / w_sqo (and w_oqs / w_oqo) are the same MLP on the same features, so each MLP runs once over every window's rows
        and one tensor serves both roles (the gradient is the sum of the two roles', as for the reference's two graph nodes)."""
        feats = self._agg_features(wb, samples)

        def gate_rows():
            sizes = [f[0].shape[0] for f in feats if f is not None]
            tot, off, perm = int(sum(sizes)), 0, []
            for n in sizes:
                perm.append(np.arange(off, off + n))              # tail rows: the object-query weight (w_oqs / w_oqo)
                perm.append(tot + np.arange(off, off + n))        # head rows: the subject-query weight (w_sqo / w_sqs)
                off += n
            sub = torch.cat([f[0] for f in feats if f is not None])
            obj = torch.cat([f[1] for f in feats if f is not None])
            return torch.from_numpy(np.concatenate(perm)).to(self._device()), sub, obj
        perm, sub, obj = self.per_sample_set(wb, "_agg_gate_rows", samples, gate_rows)
        w_s = torch.sigmoid(self.subject_query_subject_embed_linear(sub))
        w_o = torch.sigmoid(self.object_query_subject_embed_linear(obj))
        w = torch.cat([w_o, w_s]).index_select(0, perm)
        return w, w

    def _gated_translation_ok(self):
        """TransE takes the gated L1 node: the L1 condition (translation_loss_ok) and a backend with the gated L1 kernels.  No
        condition on num_ents: nothing is a GEMM."""
        return self.translation_loss_ok(self.embed_size) and TF.gated_translation_supported()

    def _gated_fused_ok(self):
        """A fused gated node applies: the score-matrix node of the bilinear scorers, or the L1 node of TransE (whose candidate mix
        is not linear, so it is formed inside the kernels)."""
        return self.bilinear_loss_ok(self.embed_size) or self._gated_translation_ok()

    def batched_gated_loss(self, wb, locs, recs, alls, samples, gates):
        """The gated loss of ALL windows as one fused node, or None when the scorer / shapes need the per-window path.
        alls: see _stacked_alls; gates: per window (w_sqs, w_sqo, w_oqs, w_oqo), or None for the model's own MLPs."""
        if not self._gated_fused_ok():
            return None
        dev = self._device()
        inp = self.cached_loss_inputs(wb, "_agg_inputs", samples, self._target_sizes(wb), finish=TF.gated_loss_inputs)
        if inp is None:
            return torch.cat(locs).sum() * 0.0
        if gates is None:
            w_known, w_cand = self._batched_gates(wb, samples)
        else:
            live = [gw for gw, smp in zip(gates, samples) if smp[0].shape[0] > 0]
            w_known = torch.cat([torch.cat([oqs.reshape(-1, 1), sqo.reshape(-1, 1)]) for sqs, sqo, oqs, oqo in live]).to(dev)
            w_cand = torch.cat([torch.cat([oqo.reshape(-1, 1), sqs.reshape(-1, 1)]) for sqs, sqo, oqs, oqo in live]).to(dev)
        big_loc, big_rec = self._stacked_alls(alls)
        return TF.batched_gated_link_prediction(torch.cat(locs), torch.cat(recs), self.rel_embeds, big_loc, big_rec, w_known, w_cand,
                                                self.args.score_function, inp, self.candidate_route)

    def gated_loss(self, loc, rec, all_loc, all_rec, triplets, neg_tail, neg_head, w_sqs, w_sqo, w_oqs, w_oqo):
        """loss_tail + loss_head of one target graph, models/PostDynamicRGCN.py:200-202 + train_link_prediction :261-282."""
        if triplets.shape[0] > 0 and (self._gated_translation_ok() or (self._gated_fused_ok() and all_loc.shape[0] % 4 == 0)):
            return TF.gated_link_prediction(loc, rec, self.rel_embeds, all_loc, all_rec, triplets, neg_tail, neg_head,
                                            w_sqs, w_sqo, w_oqs, w_oqo, self.args.score_function, self.candidate_route)
        labels = torch.zeros(triplets.shape[0], dtype=torch.int64, device=triplets.device)
        r = self.rel_embeds[triplets[:, 1]]
        s = w_oqs * loc[triplets[:, 0]] + (1 - w_oqs) * rec[triplets[:, 0]]
        neg_o = w_oqo.unsqueeze(-1) * all_loc[neg_tail] + (1 - w_oqo).unsqueeze(-1) * all_rec[neg_tail]
        loss_tail = F.cross_entropy(self.calc_score(s, r, neg_o, mode='tail'), labels)
        o_rec = rec[triplets[:, 2]]
        o = w_sqo * o_rec + (1 - w_sqo) * o_rec                                 # (sic: o_loc = o_rec, :276-277)
        neg_s = w_sqs.unsqueeze(-1) * all_loc[neg_head] + (1 - w_sqs).unsqueeze(-1) * all_rec[neg_head]
        loss_head = F.cross_entropy(self.calc_score(neg_s, r, o, mode='head'), labels)
        return loss_tail + loss_head

    def _step_weights(self, wb, samples, gate_weights):
        return gate_weights               # the model's own gates run inside the fused node's hook (or per window, below)

    def _fused_windows_loss(self, *args):
        return self.batched_gated_loss(*args)

    def _window_losses(self, wb, locs, recs, alls, samples, gate_weights):
        dev = self._device()
        feats = self._agg_features(wb, samples) if gate_weights is None else None
        loss = 0
        for i, g in enumerate(wb.graphs):
            triplets, neg_tail, neg_head = (x.to(dev) for x in samples[i])
            if gate_weights is not None:
                gw = [x.to(dev) for x in gate_weights[i]]
            else:
                gw = self.calc_ensemble_ratio(triplets, wb.rows[i][-1], g, feats[i])
            a_loc, a_rec = alls[i]
            loss = loss + self.gated_loss(locs[i], recs[i], a_loc, a_rec, triplets, neg_tail, neg_head, *gw)
        return loss

    def _graph_metrics(self, rows, alls, index_sample, g, t):
        """Embedding-level gated ranks (PostEvaluationFilter, which mixes the known object of the head rows with its own local
        row) of the (local, temporal) all-entity matrices.  No classification loss."""
        loc, rec = rows
        w_sqs, w_sqo, w_oqs, w_oqo = self.calc_ensemble_ratio(index_sample, t, g)
        return self.evaluater.calc_metrics_single_graph(loc, rec, self.rel_embeds, alls[0], alls[1], index_sample,
                                                        w_sqs, w_sqo, w_oqs, w_oqo, g, t, **self._panel_kw()), None
