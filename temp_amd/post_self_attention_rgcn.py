"""PostSelfAttentionRGCN / PostBiSelfAttentionRGCN -- `--module SARGCN / BiSARGCN --post-aggregation` (main.py:74-79) with the
reference's interface (models/PostSelfAttentionRGCN.py): same constructor, `.forward(t_list) -> loss`, `.evaluate(t_list)`, same
parameter names (the encoder's, then the four frequency MLPs of PostDynamicRGCN).

The reference resolves these classes as PostSelfAttentionRGCN -> SelfAttentionRGCN -> PostDynamicRGCN: the attention encoder,
windows, history and masks of (Bi)SelfAttentionRGCN, and the gates, loss head (train_link_prediction with the real corrupt_tail
flags) and PostEvaluationFilter ranks of PostDynamicRGCN.  Here likewise: self_attention_rgcn.py + post_gates._GatedLossMixin.

Two streams (SARGCN.forward_post_ensemble / forward_isolated_post_ensemble, models/SARGCN.py:137-146; layer 1 is a plain RGCN
layer and never attends, there is no JK max and no layer-1 K/V table):
  target rows   loc = layer-2 RGCN output + time_embed_2[t],  rec = attention of loc over the row's layer-2 history
  all entities  y2iso = Iso2(Iso1(ent_embeds)) once;  all_loc[b, e] = y2iso[e] + time_embed_2[t_b];  all_rec[b, e] = attention of
                all_loc[b, e] over entity e's history rows of window b;  the nodes of window b's target graph take their target rows.
`--use-embed-for-non-active` is ignored, as the reference's get_all_embeds_Gt ignores it (it always takes the isolated pass).

Split all-entity pass (`split_all_entity`, default on).  The attention's current row of an inactive (window, entity) pair is a
SUM of a row that no window changes and a row that no entity changes, and the Q/K/V projection is linear.  So
  P_ent  = y2iso . [Wq | Wk | Wv]^T                    (N_ents, 3D)
  P_time = time_embed_2[t_b] . [Wq | Wk | Wv]^T        (B, 3D)
are projected once each and the kernel forms (q | k | v) = P_ent[e] + P_time[b] per row (temp_sa_attn_split_fwd / _bwd): the
product sees N_ents + B rows instead of B * N_inactive, and the (B * N_inactive, 3D) buffer is neither written nor read.
`split_all_entity = False` materialises the sum and calls the existing `attend` (A/B, tools/post_attention_probe.py).

Refused at construction: rec_only_last_layer = False (the reference cannot run it: forward_isolated_post_ensemble calls
layer_1.forward_isolated(ent_embeds, time) on a SARGCNLayer, a TypeError, models/SARGCN.py:143-146) and --EMA."""
import numpy as np

from . import _lib
from . import functional as TF
from .post_gates import _GatedLossMixin
from .self_attention_rgcn import SelfAttentionRGCN


class PostSelfAttentionRGCN(_GatedLossMixin, SelfAttentionRGCN):
    """models/PostSelfAttentionRGCN.py:14-123."""
    _post_aggregation_model = True

    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test, evaluater_type=None):
        if not getattr(args, "rec_only_last_layer", False):
            raise NotImplementedError("the post-aggregation attention models need --rec-only-last-layer: without it the reference's "
                                      "SARGCN.forward_isolated_post_ensemble calls layer_1.forward_isolated(ent_embeds, time) on a "
                                      "SARGCNLayer and raises a TypeError (models/SARGCN.py:143-146)")
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test, evaluater_type)
        self.split_all_entity = True      # the all-entity attention forms its current rows from P_ent / P_time (False: materialised)
        self.init_freq_mlp()              # after everything the base constructor registers: the order of parameters()

    # -- prepare -------------------------------------------------------------------------------------------------------------
    def _plan_loss(self, wb):
        wb.loss_plan = None               # (the gated node draws through draw_samples, like the GRU post models)

    def prepare(self, t_list, seq_len, train=True, target_edge_ids=None):
        wb = super().prepare(t_list, seq_len, train, target_edge_ids)
        dev = self._device()
        B = len(wb.graphs)
        # the split pass: inactive row i is entity inactive_ent[i] of window split_win[i]; the window's time row is row b of P_time
        win = np.repeat(np.arange(B, dtype=np.int64), [len(x) for x in wb.inactive_host])
        wb.split_win = _lib.to_device(win.astype(np.int32), dev)
        wb.split_inv_ent = TF.split_row_inverse(np.concatenate(wb.inactive_host) if B else np.zeros(0, np.int64), self.num_ents, dev)
        wb.split_inv_win = TF.split_row_inverse(win, B, dev)
        times = np.array(wb.target_times, dtype=np.int64)
        wb.win_time_rows = _lib.to_device(times.astype(np.int32), dev)
        wb.win_time_inv = TF.gather_inverse(times, len(self.total_time), dev)
        return wb

    # -- encoder -------------------------------------------------------------------------------------------------------------
    def run(self, wb):
        """-> ((loc, rec) target rows, each (sum n_b, D); layer-2 K/V table): SARGCN.forward_post_ensemble over the batch."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        R = wb.n_hist_rows
        y1 = l1.conv_table(wb.g_all, self.ent_embeds, wb.ids_all, wb.ids_inv)
        y2 = l2.conv(wb.g_all, y1)
        s = y2 + TF.gather_rows(l2.time_embed, wb.time_rows, wb.time_inv)
        s_hist, loc = s.split([R, s.shape[0] - R])
        kv2 = l2.project_kv(s_hist)
        rec = l2.attend(loc, kv2, wb.idx_tgt, wb.time_diff, wb.inv_tgt)
        return (loc, rec), kv2

    def all_embeds_post(self, wb, loc, rec, kv2):
        """get_all_embeds_Gt of every window at once (models/PostSelfAttentionRGCN.py:24-41 with
        SARGCN.forward_isolated_post_ensemble) -> (all_loc, all_rec), each (B, N_ents, D).  One isolated pass; the attention
        runs only over the entities that are inactive in their window's target graph."""
        enc = self.ent_encoder
        l1, l2 = enc.layer_1, enc.layer_2
        if wb.n_inactive == 0:
            return self._assemble_all(wb, loc, None), self._assemble_all(wb, rec, None)
        y2iso = l2.conv_isolated(l1.conv_isolated(self.ent_embeds))
        cur = TF.gather_rows(y2iso, wb.inactive_ent, wb.inactive_inv) + TF.gather_rows(l2.time_embed, wb.all_time_rows, wb.all_time_inv)
        if self.split_all_entity:
            p_ent = l2.project_qkv(y2iso)
            p_time = l2.project_qkv(TF.gather_rows(l2.time_embed, wb.win_time_rows, wb.win_time_inv))
            att = l2.attend_split(p_ent, wb.inactive_ent, p_time, wb.split_win, kv2, wb.idx_all, wb.time_diff, wb.inv_all,
                                  wb.split_inv_ent, wb.split_inv_win)
        else:
            att = l2.attend(cur, kv2, wb.idx_all, wb.time_diff, wb.inv_all)
        return self._assemble_all(wb, loc, cur), self._assemble_all(wb, rec, att)

    def encode_post(self, t_list, seq_len, train=True, target_edge_ids=None):
        """-> (per-window local embeddings, per-window temporal embeddings, prepared batch, layer-2 K/V table)."""
        wb = self.prepare(t_list, seq_len, train, target_edge_ids)
        (loc, rec), kv2 = self.run(wb)
        return list(loc.split(wb.target_sizes)), list(rec.split(wb.target_sizes)), wb, kv2

    # -- loss ----------------------------------------------------------------------------------------------------------------
    def run_loss(self, wb, samples=None, weights=None):
        """PostSelfAttentionRGCN.forward, models/PostSelfAttentionRGCN.py:72-94 (Bi: :158-187).  weights: optional per-window
        (w_sqs, w_sqo, w_oqs, w_oqo) in place of the frequency MLPs' (tests)."""
        (loc, rec), kv2 = self.run(wb)
        locs, recs = list(loc.split(wb.target_sizes)), list(rec.split(wb.target_sizes))
        if samples is None:
            samples = self.draw_samples(wb)
        both = self.all_embeds_post(wb, loc, rec, kv2)
        fused = self.batched_gated_loss(wb, locs, recs, both, samples, weights)       # all windows' losses as one node
        if fused is not None:
            return fused
        alls = [(both[0][i], both[1][i]) for i in range(len(wb.graphs))]
        return self._window_losses(wb, locs, recs, alls, samples, weights)

    def forward(self, t_list, reverse=False, target_edge_ids=None, samples=None, gate_weights=None):
        wb = self.prepare(t_list, self.train_seq_len, True, target_edge_ids)
        return self.run_loss(wb, samples, gate_weights)

    # -- evaluate ------------------------------------------------------------------------------------------------------------
    def evaluation_targets(self, t_list):
        """models/PostSelfAttentionRGCN.py:96-123 (Bi: :189-208): the encoder on the full train graphs at test_seq_len, both
        all-entity matrices of every window from the one batched pass; the embedding-level gated ranks are _graph_metrics (no
        classification loss, as in the reference)."""
        wb = self.prepare(t_list, self.test_seq_len, train=False)
        (loc, rec), kv2 = self.run(wb)
        all_loc, all_rec = self.all_embeds_post(wb, loc, rec, kv2)
        for i, rows in enumerate(zip(loc.split(wb.target_sizes), rec.split(wb.target_sizes))):
            yield wb.rows[i][-1], rows, lambda g, i=i: (all_loc[i], all_rec[i])


class PostBiSelfAttentionRGCN(PostSelfAttentionRGCN):
    """models/PostSelfAttentionRGCN.py:126-208: the history of both directions concatenated (BiSelfAttentionRGCN's windows)."""
    bidirectional = True
