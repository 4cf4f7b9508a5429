"""The embedding-only baselines of the paper's tables, with the reference's interface: `--module Static` (baselines/Static.py),
`--module DE`, the diachronic embedding (baselines/DiachronicEmbedding.py), `--module Hyte` (baselines/Hyte.py) and `--module Simple`
(baselines/Simple.py), all on baselines/TKG_Non_Recurrent.py.  No message passing: the all-entity table of timestamp t is a function of
the parameters and t alone,

    Static               ent_embeds
    DiachronicEmbedding  ent_embeds * [1 (first D // 2 columns) | sin(t * w_temp_ent_embeds + b_temp_ent_embeds)]
    Hyte                 ent_embeds - n_t (n_t . ent_embeds),  n_t = time_embeddings[t] / |time_embeddings[t]|   (rel_embeds likewise)
    SimplE               [ent_embeds | ent_embeds_inv], rows of width 2 D                      (rel_embeds | rel_embeds_inv likewise)

so a batch of B timestamps is ONE (B N, D) stack (functional.diachronic_rows / hyperplane_rows: one launch forward, a backward that
already sums over the timestamps) scored by ONE fused loss node (TKG_Module.batched_link_prediction) -- the loss, the sampler and the
filtered ranking are the ones the RGCN models use.  Hyte's relation rows depend on the timestamp too: its (B 2R, D) relation stack
is the loss node's relation operand (sampling.plan_batch_loss(rel_stride=2R)); SimplE's ONE (2R, 2D) pair table serves all windows."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import functional as TF
from .tkg_module import TKG_Module


class TKG_Non_Recurrent(TKG_Module):
    """baselines/TKG_Non_Recurrent.py:8-32.  Subclasses give `table_stack(times)`: the (B N, D) stack of the all-entity tables of the
    float32 device vector `times`; rows b N + gids of it are the target rows of graph b (get_per_graph_ent_embeds)."""

    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test):
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test)
        self.init_embeddings()
        self.use_device_sampler = True

    rel_stride = None           # rows between the windows' relation tables in relation_stack(); None: one table for all windows

    def build_model(self):
        pass

    def table_stack(self, times):
        raise NotImplementedError

    def relation_stack(self, times):
        """The (B 2R, D) stack of the timestamps' relation tables, or None when all timestamps share self.rel_embeds."""
        return None

    def stacks(self, times):
        """(table_stack, relation_stack) of one batch."""
        return self.table_stack(times), self.relation_stack(times)

    def _rel_rows(self, rel_stack, b):
        """The relation table of batch position b."""
        if rel_stack is None:
            return self.rel_embeds
        n = int(self.rel_embeds.shape[0])
        return rel_stack[b * n:(b + 1) * n]

    def _times(self, ts):
        return _lib.to_device(np.asarray(ts, dtype=np.float32), self._device())

    def _gids(self, g):
        return torch.from_numpy(g.gids).to(self._device())

    def get_all_embeds_Gt(self, t):
        return self.table_stack(self._times([int(t)]))

    def get_per_graph_ent_embeds(self, t, g):
        """The rows of the graph's entities (the reference gathers the parameters and applies the same element-wise map)."""
        return self.get_all_embeds_Gt(t)[self._gids(g)]

    # -- evaluation (models/TKG_Module.py:253-274) ---------------------------------------------------------------------------
    def evaluation_targets(self, t_list):
        """All B tables (and relation tables) from one stacks() call.  A graph's own rows are rows of its table, so what
        _graph_metrics takes from here is the batch position's relation table."""
        ts, N = [int(t) for t in t_list], self.num_ents
        stack, rel_stack = self.stacks(self._times(ts))
        for b, t in enumerate(ts):
            yield t, self._rel_rows(rel_stack, b), lambda g, b=b: stack[b * N:(b + 1) * N]

    def _graph_metrics(self, rel_embed, all_embeds_g, index_sample, g, t):
        return super()._graph_metrics(all_embeds_g[self._gids(g)], all_embeds_g, index_sample, g, t, rel=rel_embed)

    # -- the fused batch loss ------------------------------------------------------------------------------------------------
    def row_width(self):
        """The width of the rows of table_stack(): what the loss nodes take as the query width."""
        return self.embed_size

    def _fused_loss_ok(self):
        return self.use_device_sampler and self.fused_loss_ok(self.row_width())

    def _fused_plan(self, ts, g_list):
        """Host half of the fused loss of a batch, uploaded once: the times, the positives / operand indices / known-true slices
        (sampling.plan_batch_loss).  The known rows point INTO the table stack: local id i of graph b -> row b N + gids_b[i]."""
        from .sampling import plan_batch_loss
        dev, N, B = self._device(), self.num_ents, len(g_list)
        off = np.concatenate([[0], np.cumsum([g.n for g in g_list])])
        row_map = np.concatenate([b * N + g.gids.astype(np.int64) for b, g in enumerate(g_list)]) if B else np.zeros(0, np.int64)
        plan = plan_batch_loss(self.true_sets(), ts, g_list, off[:-1], self.args.num_pos_facts, self.sample_rng, B * N, int(self.rel_embeds.shape[0]), dev,
                               row_map=row_map, rel_stride=self.rel_stride)
        return dict(plan=plan, B=B, times=self._times(ts))

    def _fused_loss(self, fp, cand=None):
        """sum_b loss_tail + loss_head as one table_stack node and one batched_link_prediction node: the stack is both the
        all-entity operand and the source of the known rows, so its gradient arrives once; the negatives of all graphs come from
        one launch (`cand`: a fixed draw to reuse, else a fresh one per call)."""
        plan = fp["plan"]
        if plan is None:
            return self.ent_embeds.sum() * 0.0
        stack, rel_stack = self.stacks(fp["times"])
        cand = self.draw_candidates(plan, cand)
        self._last_plan = (plan, cand)
        return self.batched_link_prediction(stack, dict(plan, cand=cand), stack, rel=rel_stack)

    def prepare(self, t_list):
        """-> a prepared batch: graphs, times on the device and -- when a fused loss node takes the scorer -- the loss plan.  A step
        on it (run_loss) uploads nothing."""
        wb = type("NonRecurrentBatch", (), {})()
        wb.ts = [int(t) for t in t_list]
        wb.g_list = [self.graph_dict_train[t] for t in wb.ts]
        wb.fused = self._fused_plan(wb.ts, wb.g_list) if self._fused_loss_ok() else None
        return wb

    def run_loss(self, wb, cand=None):
        """Table stack + fused loss on a prepared batch (cand: fixed negatives, e.g. the draw of an earlier call: self._last_plan[1])."""
        if wb.fused is None:
            raise NotImplementedError("run_loss needs the fused loss (a scorer and a width with a fused node); use forward()")
        return self._fused_loss(wb.fused, cand)

    def forward(self, t_list, samples=None):
        """baselines/TKG_Non_Recurrent.py:21-32.  samples: per graph (triplets, neg_tail, neg_head) to use instead of a draw; they,
        or a scorer / width without a fused node, take the reference-granular loop -- over slices of the same one table stack."""
        ts, N = [int(t) for t in t_list], self.num_ents
        g_list = [self.graph_dict_train[t] for t in ts]
        if samples is None and self._fused_loss_ok():
            return self._fused_loss(self._fused_plan(ts, g_list))
        stack, rel_stack = self.stacks(self._times(ts))
        tables = [stack[b * N:(b + 1) * N] for b in range(len(ts))]
        return self.per_graph_loss(ts, g_list, samples, lambda b: tables[b][self._gids(g_list[b])], tables.__getitem__,
                                   rel=lambda b: self._rel_rows(rel_stack, b))


class Static(TKG_Non_Recurrent):
    """baselines/Static.py: one time-independent table."""

    def get_all_embeds_Gt(self, t):
        return self.ent_embeds

    def table_stack(self, times):
        """B times the same table, as an EXPANDED VIEW of ent_embeds made contiguous: both loss nodes address window b's table at
        row b N of their operand (link_loss._GemmScorer slices it, _L1Scorer adds window * N to every candidate), so neither
        takes a per-row base of 0 and the windows cannot share one copy; the view's adjoint sums the B blocks."""
        B = times.shape[0]
        return self.ent_embeds.unsqueeze(0).expand(B, self.num_ents, self.embed_size).reshape(B * self.num_ents, self.embed_size)


class DiachronicEmbedding(TKG_Non_Recurrent):
    """baselines/DiachronicEmbedding.py: the second half of every entity row is modulated by sin(t w + b)."""

    def build_model(self):
        self.static_embed_size = math.floor(0.5 * self.embed_size)
        self.temporal_embed_size = self.embed_size - self.static_embed_size
        self.w_temp_ent_embeds = nn.Parameter(torch.Tensor(self.num_ents, self.temporal_embed_size))
        self.b_temp_ent_embeds = nn.Parameter(torch.Tensor(self.num_ents, self.temporal_embed_size))
        nn.init.xavier_uniform_(self.w_temp_ent_embeds, gain=nn.init.calculate_gain('relu'))
        nn.init.xavier_uniform_(self.b_temp_ent_embeds, gain=nn.init.calculate_gain('relu'))

    def table_stack(self, times):
        return TF.diachronic_rows(self.ent_embeds, self.w_temp_ent_embeds, self.b_temp_ent_embeds, times)


class _TimeRows:
    """Hyte's `times`: the rows of time_embeddings of a batch on the device (int32 for gather_rows, int64 for plain indexing) and the
    static inverse that makes the gather's adjoint the deterministic segment sum."""

    def __init__(self, rows, n_rows, device):
        rows = np.asarray(rows, dtype=np.int32)
        self.shape = rows.shape
        self.idx = _lib.to_device(rows, device)
        self.idx64 = self.idx.long()
        self.inv = TF.gather_inverse(rows, n_rows, device)


class Hyte(TKG_Non_Recurrent):
    """baselines/Hyte.py: at timestamp t every entity row and every relation row is projected onto the hyperplane whose normal is
    time_embeddings[t]; the projected rows are scored with TransE.  The time row of timestamp t is its position among the training
    timestamps (list(graph_dict_train.keys())), which is the reference's time_embeddings[t] wherever its indexing is in range."""

    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test):
        args.score_function = 'transE'                              # baselines/Hyte.py:10
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test)

    def build_model(self):
        self.time_embeddings = nn.Parameter(torch.Tensor(len(self.graph_dict_train.keys()), self.embed_size))
        nn.init.xavier_uniform_(self.time_embeddings, gain=nn.init.calculate_gain('relu'))
        self._time_row = {int(t): i for i, t in enumerate(self.graph_dict_train.keys())}

    @property
    def rel_stride(self):
        return int(self.rel_embeds.shape[0])

    def _times(self, ts):
        try:
            rows = [self._time_row[int(t)] for t in ts]
        except KeyError as e:
            raise KeyError("Hyte: timestamp %s is not a training timestamp: it has no time row" % e.args[0])
        return _TimeRows(rows, int(self.time_embeddings.shape[0]), self._device())

    def time_rows(self, times):
        """w (B, D) = time_embeddings[rows]: the HIP row gather with its deterministic adjoint where its width limits allow."""
        D = self.embed_size
        if D % 4 == 0 and D <= 256:
            return TF.gather_rows(self.time_embeddings, times.idx, times.inv)
        return self.time_embeddings[times.idx64]

    def table_stack(self, times):
        return TF.hyperplane_rows(self.ent_embeds, self.time_rows(times))

    def relation_stack(self, times):
        return TF.hyperplane_rows(self.rel_embeds, self.time_rows(times))

    def stacks(self, times):
        """Both projections from ONE gather of the time rows: autograd adds their two d_w before the gather's adjoint."""
        w = self.time_rows(times)
        return TF.hyperplane_rows(self.ent_embeds, w), TF.hyperplane_rows(self.rel_embeds, w)

    def relation_table(self, t):
        return self.relation_stack(self._times([int(t)]))

    def get_per_graph_embeds(self, t, g):
        """baselines/Hyte.py:18-27 -> (projected rows of the graph's entities, projected relation rows)."""
        ent, rel = self.stacks(self._times([int(t)]))
        return ent[self._gids(g)], rel


class SimplE(TKG_Non_Recurrent):
    """baselines/Simple.py: every entity and every relation has a forward and an inverse row, and a triple's score is the mean of the
    two DistMult directions <s r, o_inv> and <s_inv r_inv, o> (scores.simple).  In the PAIR layout -- entity e is the row
    [ent_embeds[e] | ent_embeds_inv[e]], relation r the row [rel_embeds[r] | rel_embeds_inv[r]], both of width 2 D -- that score is
    bilinear in (folded query, candidate row) like DistMult's (scores.bilinear_query("simple"), scores.simple_pair), so the pair tables
    go through the loss nodes, the filtered rank and predict() as any other table.  The relation pair table does not depend on the
    timestamp: ONE (2R, 2D) table is the relation operand of every window (rel_stride stays None)."""

    def __init__(self, args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test):
        args.score_function = 'simple'                              # the score the reference's train_link_prediction computes
        super().__init__(args, num_ents, num_rels, graph_dict_train, graph_dict_val, graph_dict_test)
        self.ent_embeds_inv = nn.Parameter(torch.Tensor(self.num_ents, self.embed_size))           # baselines/Simple.py:70-75: after
        self.rel_embeds_inv = nn.Parameter(torch.Tensor(self.num_rels * 2, self.embed_size))       # the base tables, in this order
        nn.init.xavier_uniform_(self.ent_embeds_inv, gain=nn.init.calculate_gain('relu'))
        nn.init.xavier_uniform_(self.rel_embeds_inv, gain=nn.init.calculate_gain('relu'))

    def row_width(self):
        return 2 * self.embed_size

    def table_stack(self, times):
        return TF.pair_rows(self.ent_embeds, self.ent_embeds_inv, times.shape[0])

    def relation_stack(self, times):
        """The one (2R, 2D) relation pair table (one launch whatever the number of windows)."""
        return TF.pair_rows(self.rel_embeds, self.rel_embeds_inv, 1)

    def _rel_rows(self, rel_stack, b):
        return rel_stack                                            # shared by all windows: nothing to slice

    def relation_table(self, t):
        return self.relation_stack(None)

    def get_per_graph_ent_embeds(self, g_list):
        """baselines/Simple.py:80-85 -> (the graphs' rows of ent_embeds, the graphs' rows of ent_embeds_inv), one tensor per graph."""
        ids = torch.cat([self._gids(g) for g in g_list])
        sizes = [int(g.n) for g in g_list]
        return self.ent_embeds[ids].split(sizes), self.ent_embeds_inv[ids].split(sizes)


# main.py:42-55: the `--module` names of the embedding-only baselines
MODULES = {"Static": Static, "DE": DiachronicEmbedding, "Hyte": Hyte, "Simple": SimplE}
