"""Aggregator -- the checkpoint-ensemble head of the reference's models/aggregator.py (`--module Aggregator`): a trained StaticRGCN
(the "spatial" or local model) and a trained temporal window model are loaded and FROZEN, and two 3 -> 3 -> 1 frequency MLPs learn a
per-triple weight that mixes the two models' scores,  score = w * local + (1 - w) * temporal.

Both sub-models are whole models of this package with their own relation tables and possibly their own widths; nothing of them has
a gradient.  The training loss of all windows is therefore ONE node, functional.frozen_ensemble_link_prediction: two query folds and
one launch that scores the candidate lists straight from the two all-entity stacks and returns the loss rows together with
d loss / d w (temp_frozen_mix_ce) -- no (rows, N) score matrix, no backward launch.  Scorers or widths outside that node take the
literal per-graph route (calc_score on gathered candidates, F.cross_entropy).

Decisions where the reference does not run as it stands, or where this class departs from it:
  * both sub-models run under no_grad through their own evaluation_targets(): the full train graphs with train=False, in training
    and in evaluation alike, and they are kept in eval() whatever train() is called on the head (the reference leaves them in
    training mode, so their dropout would add noise to frozen scores);
  * the checkpoint of a run directory is the first of the SORTED glob (the reference takes an unsorted glob(...)[0]);
  * a temporal config with post_aggregation / post_ensemble / impute is refused: the reference routes it to the Post* / Impute*
    classes, whose get_all_embeds_Gt signatures do not fit Aggregator.forward's call, so it cannot run there either;
  * ranks are taken on the raw mixed score (the reference's sigmoid is monotone: ties only); no classification loss (nan).
Goldens G30 / G31 (tools/gen_golden_aggregator.py) hold the class to the reference's own: state_dict layout, features, weights, loss,
MLP gradients and ranks."""
import copy
import glob
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as TF
from .link_loss import FROZEN_KIND
from .post_gates import _FrequencyGateMixin
from .sampling import CorruptTriples
from .tkg_module import TKG_Module

FROZEN_MAX_WIDTH = 512            # include/temp_amd.h: temp_frozen_mix_ce keeps a row's query slices in registers up to this width


def _temporal_class(name):
    """The reference's module map (models/aggregator.py:26-33)."""
    from .bi_dynamic_rgcn import BiDynamicRGCN
    from .dynamic_rgcn import DynamicRGCN
    from .self_attention_rgcn import BiSelfAttentionRGCN, SelfAttentionRGCN
    table = {"GRRGCN": DynamicRGCN, "RRGCN": DynamicRGCN, "SARGCN": SelfAttentionRGCN, "BiGRRGCN": BiDynamicRGCN, "BiRRGCN": BiDynamicRGCN,
             "BiSARGCN": BiSelfAttentionRGCN}
    if name not in table:
        raise ValueError("Aggregator: temporal_module must be one of %s, got %r" % (sorted(table), name))
    return table[name]


def load_run(path, args):
    """A run directory of the reference's trainer -> (the run's args: a copy of `args` overlaid with its config.json, its state_dict).
    The directory holds config.json and checkpoints/*.ckpt; the first checkpoint in sorted order is taken."""
    ckpts = sorted(glob.glob(os.path.join(path, "checkpoints", "*.ckpt")))
    if not ckpts:
        raise FileNotFoundError("Aggregator: no checkpoints/*.ckpt under %r" % (path,))
    # weights_only=False, as the reference's plain torch.load of its day: a trainer's checkpoint carries a pickled Namespace (hparams)
    # and optimizer state next to 'state_dict', which the weights-only loader refuses; the directory is the user's own training run
    ckpt = torch.load(ckpts[0], map_location="cpu", weights_only=False)
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    run_args = copy.copy(args)
    run_args.__dict__.update(dict(cfg))
    return run_args, ckpt["state_dict"]


class Aggregator(_FrequencyGateMixin, TKG_Module):
    """models/aggregator.py:22-361.  state_dict keys, in order: temporal_model.*, spatial_model.*, subject_linear.{0,2}.*, object_linear.{0,2}.*."""
    _evaluater = "PostEnsembleEvaluationFilter"
    _gate_count = 1
    _all_entity_loss_refusal = "its loss mixes the scores of two frozen models' tables; the all-entity node takes one table"

    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test, spatial_model=None, temporal_model=None):
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test)
        graphs = (num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test)
        from .static_rgcn import StaticRGCN
        if spatial_model is None or temporal_model is None:
            if getattr(args, "debug", False):
                # the reference's debug branch (models/aggregator.py:44-53): fresh, untrained sub-models, the temporal one BiGRRGCN
                t_args = copy.copy(args)
                t_args.module = "BiGRRGCN"
                from .bi_dynamic_rgcn import BiDynamicRGCN
                spatial_model = StaticRGCN(args, *graphs) if spatial_model is None else spatial_model
                temporal_model = BiDynamicRGCN(t_args, *graphs) if temporal_model is None else temporal_model
            else:
                if temporal_model is None:
                    t_args, t_state = load_run(args.temporal_checkpoint, args)
                    cls = _temporal_class(args.temporal_module)
                    for flag in ("post_aggregation", "post_ensemble", "impute"):
                        if getattr(t_args, flag, False):
                            raise NotImplementedError(
                                "Aggregator: the temporal run was trained with --%s; the reference routes it to a Post* / Impute* class whose "
                                "get_all_embeds_Gt does not fit Aggregator.forward's call, so it cannot run there either" % flag.replace("_", "-"))
                    temporal_model = cls(t_args, *graphs)
                    temporal_model.load_state_dict(t_state)
                if spatial_model is None:
                    s_args, s_state = load_run(args.spatial_checkpoint, args)
                    spatial_model = StaticRGCN(s_args, *graphs)
                    spatial_model.load_state_dict(s_state)
        # registered in the order of the reference's checkpoint branch (models/aggregator.py:85, 98; pinned by golden G30): the
        # temporal model first -- the order of state_dict() and of parameters()
        self.temporal_model = temporal_model
        self.spatial_model = spatial_model
        t_args = temporal_model.args
        self.train_seq_len = self.test_seq_len = t_args.train_seq_len
        self.bidirectional = "Bi" in t_args.module
        for m in (self.spatial_model, self.temporal_model):
            m.requires_grad_(False)
            m.eval()
        self.subject_linear = nn.Sequential(nn.Linear(3, 3), nn.ReLU(), nn.Linear(3, 1))
        self.object_linear = nn.Sequential(nn.Linear(3, 3), nn.ReLU(), nn.Linear(3, 1))
        seed = getattr(args, "seed", None)
        self.sample_rng = np.random.default_rng(seed)
        if not hasattr(self, "corrupter"):            # (debug: TKG_Module builds none, and neither does the reference -- its forward cannot draw)
            self.corrupter = CorruptTriples(self.args, graph_dict_train)

    def build_model(self):
        pass

    def train(self, mode=True):
        """The head follows `mode`; the frozen sub-models stay in eval()."""
        super().train(mode)
        self.spatial_model.eval()
        self.temporal_model.eval()
        return self

    @property
    def rel_embeds(self):
        """The relation table of the LOCAL stream (what the mixins hand to the ranker first); the temporal one: _topk_relation_kw."""
        return self.spatial_model.rel_embeds

    def _topk_relation_kw(self):
        return dict(rel_enc_temporal=self.temporal_model.rel_embeds)

    def _device(self):
        return self.spatial_model.ent_embeds.device

    def optimizer_parameters(self):
        """What configure_clipped_optimizer() hands the optimizer: the parameters that require grad, i.e. the eight MLP tensors."""
        return [p for p in self.parameters() if p.requires_grad]

    # -- features and weights (models/aggregator.py:135-169) ------------------------------------------------------------------------
    def frequency_tables(self):
        """From the TEMPORAL model's window length and direction, as the reference builds its DropEdge from temporal_args."""
        ft = getattr(self, "_freq_tables", None)
        if ft is None:
            from .frequency import FrequencyTables
            ft = self._freq_tables = FrequencyTables(self.graph_dict_train, self.train_seq_len, self.bidirectional, 2 * self.num_rels)
        return ft

    def calc_ensemble_ratio(self, triples, t, g):
        """-> (weight_subject (n, 1) = sigmoid(subject_linear([obj, rel, obj_rel freq])), weight_object (n, 1) =
        sigmoid(object_linear([sub, rel, sub_rel freq]))); (0, 1) float tensors for no triples."""
        if len(triples) == 0:
            e = torch.zeros(0, 1, dtype=torch.float32, device=self._device())
            return e, e
        sub_f, obj_f = self.ensemble_features(triples, t, g)
        return torch.sigmoid(self.subject_linear(sub_f)), torch.sigmoid(self.object_linear(obj_f))

    def _query_gates(self, t, known, rel, mode):
        """(w,) [Q], paired as in the training loss: a tail query by the object MLP, a head query by the subject MLP (the convention
        post_dynamic_rgcn._PostEnsembleMixin documents)."""
        mlp = self.object_linear if mode == "tail" else self.subject_linear
        return (torch.sigmoid(mlp(self.query_features(t, known, rel, mode))).reshape(-1),)

    # -- the two frozen streams -----------------------------------------------------------------------------------------------------
    def evaluation_targets(self, t_list):
        """Both sub-models' own evaluation_targets() side by side, under no_grad: per timestamp ((local rows, temporal rows),
        all_embeds(g) -> (local table, temporal table))."""
        ts = [int(t) for t in t_list]
        with torch.no_grad():
            for (ta, rows_a, all_a), (tb, rows_b, all_b) in zip(self.spatial_model.evaluation_targets(ts), self.temporal_model.evaluation_targets(ts)):
                assert int(ta) == int(tb), "the sub-models disagree on the order of the target timestamps"
                yield int(ta), (rows_a, rows_b), (lambda g, all_a=all_a, all_b=all_b: (all_a(g), all_b(g)))

    def _frozen_ok(self, Da, Db):
        """All windows go through the one-launch node: a scorer it has, widths inside the kernel's and the fold's alignment."""
        name = self.args.score_function
        m = 8 if name == "complex" else 4
        return self.fused_loss and name in FROZEN_KIND and Da % m == 0 and Db % m == 0 and max(Da, Db) <= FROZEN_MAX_WIDTH

    def _scores(self, ent_embed, rel, triplets, neg, all_embeds_g, corrupt_tail):
        """models/aggregator.py:344-354."""
        r = rel[triplets[:, 1]]
        if corrupt_tail:
            return self.calc_score(ent_embed[triplets[:, 0]], r, all_embeds_g[neg], mode='tail')
        return self.calc_score(all_embeds_g[neg], r, ent_embed[triplets[:, 2]], mode='head')

    def forward(self, t_list, reverse=False, samples=None, ensemble_weights=None):
        """models/aggregator.py:171-209: sum over the target graphs of CE_tail (mixed by weight_object) + CE_head (mixed by
        weight_subject).  samples: per target graph, in DESCENDING timestamp order, (triplets, neg_tail, neg_head) as the post
        classes take them; None draws them with the host sampler (self.corrupter), as StaticRGCN.forward does.  ensemble_weights:
        per graph (weight_subject (P, 1), weight_object (P, 1)) in place of the MLPs'."""
        ts = sorted((int(t) for t in t_list), reverse=True)
        dev = self._device()
        graphs = [self.graph_dict_train[t] for t in ts]
        rows_a, rows_b, alls_a, alls_b = [], [], [], []
        for (t, (ra, rb), all_embeds), g in zip(self.evaluation_targets(ts), graphs):
            a, b = all_embeds(g)
            rows_a.append(ra); rows_b.append(rb); alls_a.append(a); alls_b.append(b)
        if samples is None:
            samples = [self.corrupter.single_graph_negative_sampling(t, g, self.num_ents)[:3] for t, g in zip(ts, graphs)]
        samples = [tuple(x.to(dev) for x in smp) for smp in samples]
        if ensemble_weights is None:
            weights = [self.calc_ensemble_ratio(smp[0], t, g) for smp, t, g in zip(samples, ts, graphs)]
        else:
            weights = [tuple(w.to(dev) for w in ws) for ws in ensemble_weights]
        rel_a, rel_b = self.spatial_model.rel_embeds, self.temporal_model.rel_embeds
        if self._frozen_ok(rows_a[0].shape[1], rows_b[0].shape[1]):
            offs = np.concatenate([[0], np.cumsum([g.n for g in graphs])])[:-1]
            inp = self.loss_inputs([int(o) for o in offs], samples, dev)
            if inp is None:
                return self.subject_linear[0].weight.sum() * 0.0
            w = torch.cat([torch.cat([wo.reshape(-1, 1), ws.reshape(-1, 1)]) for (ws, wo), smp in zip(weights, samples) if smp[0].shape[0] > 0])
            return TF.frozen_ensemble_link_prediction(torch.cat(rows_a), rel_a, torch.cat(alls_a), torch.cat(rows_b), rel_b, torch.cat(alls_b),
                                                      w, self.args.score_function, inp)
        loss = 0
        for i, (triplets, neg_tail, neg_head) in enumerate(samples):
            if triplets.shape[0] == 0:
                continue
            labels = torch.zeros(triplets.shape[0], dtype=torch.int64, device=dev)
            ws, wo = weights[i]
            for neg, tail, w in ((neg_tail, True, wo), (neg_head, False, ws)):
                local = self._scores(rows_a[i], rel_a, triplets, neg, alls_a[i], tail)
                temporal = self._scores(rows_b[i], rel_b, triplets, neg, alls_b[i], tail)
                loss = loss + F.cross_entropy(w * local + (1 - w) * temporal, labels)
        return loss

    # -- evaluation (models/aggregator.py:211-296) ----------------------------------------------------------------------------------
    def evaluate(self, t_list, val=True):
        """TKG_Module.evaluate over the timestamps in descending order (models/aggregator.py:212); no classification loss (nan)."""
        return super().evaluate(sorted((int(t) for t in t_list), reverse=True), val)

    def _graph_metrics(self, rows, alls, index_sample, g, t):
        """Score-level ensemble ranks over two relation tables.  As in the reference (models/aggregator.py:270-272) the
        object-corruption ranks use weight_subject and the subject-corruption ranks weight_object."""
        w_subject, w_object = self.calc_ensemble_ratio(index_sample, t, g)
        return self.evaluater.calc_metrics_single_graph(rows[0], rows[1], self.spatial_model.rel_embeds, alls[0], alls[1], w_subject, w_object,
                                                        index_sample, g, t, rel_enc_temporal=self.temporal_model.rel_embeds,
                                                        **self._panel_kw()), None
