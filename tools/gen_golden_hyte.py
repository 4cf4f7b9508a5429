"""Golden fixtures of the HyTE baseline (`--module Hyte`: baselines/Hyte.py on baselines/TKG_Non_Recurrent.py), recorded from the
reference run under the oracle's stand-ins.  Uses oracle/gen_golden.py and oracle/ref_harness.py as they are (read-only) and writes
under tests/golden/.

The reference's Hyte.forward and Hyte.evaluate do not run as written (a method that does not exist, the sampler and the filter with
older signatures).  What does run defines the model, composed as TKG_Non_Recurrent.forward and TKG_Module.calc_metrics compose it:
Hyte.get_per_graph_embeds (for the all-entity table: given a graph stand-in whose ndata['id'] is arange(N)), Hyte.train_link_prediction
on the all-entity table with the positives' global ids, the sampler's three-argument form, and
EvaluationFilter.calc_metrics_single_graph / link_classification_loss given the projected relation rows.

  G26_hyte
      D = 16, seeded parameters (tests/hyte_cases.py: seeded_params) with the entity / relation tables times G26_ENT_SCALE /
      G26_REL_SCALE, the three training timestamps with the fewest edges, 20 negatives.  The loss of the recorded draws, then backward(): d_time, d_rel, the non-zero rows of d_ent, the
      summed |gradient| of every parameter, 64 seeded rows of each projected entity table, all projected relation rows, the names
      and shapes of the reference's state_dict().  The L1 score is kinked: a component of q - e that two fp32 evaluation orders
      place on opposite sides of zero flips a gradient term.  `component_bar` is the largest fp32 error bar of a projected
      component over the three timestamps' tables, (2 D + 16) 2^-24 (|e_k| + |n_k| sum_j |n_j e_j|); seeds are tried from G26_SEEDS
      until no component of q - e over the recorded samples is smaller in magnitude than twice that; the seed and the margin
      (`kink_margin`: the smallest |component|) are recorded.  The expected number of components inside the band is about
      (number of components) * 4 bar / (their spread), whatever the scale of the tables -- 2 to 3 for these 1.8e5 components, so
      about one seed in ten qualifies (and none would with three of the larger graphs).
  G27_eval_hyte
      evaluate() ranks for val and test with the tie-band counts of G13 (band 1.5e-6): D = 16, seed 5, entity scale 4, relation
      scale 0.3.  The share of ranks outside every tie band is printed, recorded and asserted >= 0.75 on both splits.

    python tools/gen_golden_hyte.py [G26] [G27]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from tests.hyte_cases import U, params_checksum, seeded_params  # noqa: E402

D = 16
G26_ENT_SCALE, G26_REL_SCALE = 12.0, 3.0      # entity and relation rows both up to ~0.5: scores of order 1, one size of error bar
G26_SEEDS = tuple(range(831, 895))
G26_TIMES = (18, 0, 4)                        # the three training timestamps with the fewest edges (86, 91, 93): 1.8e5 components of q - e
G27_SEED, G27_ENT_SCALE, G27_REL_SCALE = 5, 4.0, 0.3
N_ALL_ROWS = 64
MAX_BYTES = 600 << 10


class AllEntities:
    """Graph stand-in for the all-entity table: get_per_graph_embeds reads nothing but ndata['id']."""

    def __init__(self, n):
        self.ndata = {'id': torch.arange(n)}


def _model(seed, ent_scale, rel_scale):
    from baselines.Hyte import Hyte
    num_e, num_r, tr, va, te_g = GG.graphs()
    args = rh.make_args(module="Hyte", hidden_size=D, embed_size=D, negative_rate=20, score_function="complex")
    sd = seeded_params(num_e, num_r, len(tr), D, seed, ent_scale, rel_scale)
    torch.manual_seed(0)
    m = Hyte(args, num_e, num_r, tr, va, te_g)
    assert args.score_function == "transE"
    m.load_state_dict(sd, strict=True)
    own = m.state_dict()
    shapes = np.full((len(own), 2), -1, dtype=np.int64)
    for i, v in enumerate(own.values()):
        shapes[i, :v.dim()] = list(v.shape)
    out = dict(module="Hyte", score_function="transE", D=D, seed=seed, neg=20, ent_scale=ent_scale, rel_scale=rel_scale,
               param_checksum=params_checksum(sd), times=np.array(list(tr.keys())), sd_names=np.array(list(own)), sd_shapes=shapes)
    return m, out


def _component_bar(table, n):
    """Largest forward error bar of a component of `table` projected with the unit normal n (fp64)."""
    e, n = table.detach().double(), n.detach().double().view(1, -1)
    bar = (2 * D + 16) * U * (e.abs() + n.abs() * (e.abs() * n.abs()).sum(1, keepdim=True))
    return float(bar.max())


def _g26_try(seed, t_list, all_g):
    m, out = _model(seed, G26_ENT_SCALE, G26_REL_SCALE)
    np.random.seed(seed)
    torch.manual_seed(seed)
    loss, samples, margin, bar = 0, [], float("inf"), 0.0
    for t in t_list:
        tt = torch.tensor(t)
        g = m.graph_dict_train[t]
        all_ent, rel_p = m.get_per_graph_embeds(tt, all_g)
        trip, neg_tail, neg_head, labels = m.corrupter.single_graph_negative_sampling(tt, g, m.num_ents)
        samples.append([x.clone() for x in (trip, neg_tail, neg_head)])
        gids = g.ndata['id'].view(-1)
        trip_g = torch.stack([gids[trip[:, 0]], trip[:, 1], gids[trip[:, 2]]], dim=1)
        loss = loss + m.train_link_prediction(all_ent, rel_p, trip_g, neg_tail, labels, corrupt_tail=True) \
            + m.train_link_prediction(all_ent, rel_p, trip_g, neg_head, labels, corrupt_tail=False)
        with torch.no_grad():
            n = m.time_embeddings[t] / m.time_embeddings[t].norm()
            bar = max(bar, _component_bar(m.ent_embeds, n), _component_bar(m.rel_embeds, n))
            a64, r64 = all_ent.double(), rel_p.double()[trip[:, 1]]
            q_tail = (a64[trip_g[:, 0]] + r64).unsqueeze(1) - a64[neg_tail]                  # s + r - o'
            q_head = a64[neg_head] + (r64 - a64[trip_g[:, 2]]).unsqueeze(1)                  # s' + r - o
            margin = min(margin, float(q_tail.abs().min()), float(q_head.abs().min()))
    return m, out, loss, samples, margin, bar


def gen_G26():
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    assert times == list(range(len(times))), "time_embeddings[t] of the reference is the position among the training timestamps"
    t_list = [int(times[i]) for i in G26_TIMES]
    all_g = AllEntities(num_e)
    for seed in G26_SEEDS:
        m, out, loss, samples, margin, bar = _g26_try(seed, t_list, all_g)
        print("  seed %d: smallest |component of q - e| %.3e, component bar %.3e -> %s" % (seed, margin, bar, "kept" if margin >= 2 * bar else "next"))
        if margin >= 2 * bar:
            break
    else:
        raise SystemExit("no seed of G26_SEEDS keeps every component of q - e away from zero")
    loss.backward()
    out.update(t_list=np.array(t_list), loss=loss.item(), n_samples=len(samples), kink_margin=margin, component_bar=bar)
    for i, (trip, nt, nh) in enumerate(samples):
        out['trip_%d' % i], out['negtail_%d' % i], out['neghead_%d' % i] = trip, nt, nh
    row_rng = np.random.default_rng(seed + 11)
    with torch.no_grad():
        for i, t in enumerate(t_list):
            rows = np.sort(row_rng.choice(num_e, N_ALL_ROWS, replace=False))
            all_ent, rel_p = m.get_per_graph_embeds(torch.tensor(t), all_g)
            out['all_rows_%d' % i], out['all_%d' % i], out['rel_%d' % i] = rows, all_ent[rows].clone(), rel_p.clone()
    g = m.ent_embeds.grad
    nz = torch.nonzero(g.abs().sum(1)).view(-1)
    stride = max(1, -(-(nz.numel() * g.shape[1] * 4) // MAX_BYTES))
    rows = nz[::stride]
    out['d_ent_sub'], out['d_ent_nz_rows'], out['d_ent_nz_vals'] = stride, rows, g[rows]
    out['d_rel'], out['d_time'] = m.rel_embeds.grad, m.time_embeddings.grad
    for k, v in m.named_parameters():
        out['gabs_' + k] = v.grad.double().abs().sum().item()
    print("  G26_hyte: seed %d, loss %.6f, %d non-zero d_ent rows, every %d-th kept" % (seed, out["loss"], nz.numel(), stride))
    GG.save("G26_hyte", **out)


def gen_G27():
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    m, out = _model(G27_SEED, G27_ENT_SCALE, G27_REL_SCALE)
    t_list = [int(times[i]) for i in (14, 8, 2)]
    out.update(t_list=np.array(t_list), band=GG.G13_BAND)
    all_g = AllEntities(num_e)
    ev = m.evaluater
    rec = dict(mode=None, graphs=[])
    orig_single, orig_perturb, orig_sort = ev.calc_metrics_single_graph, ev.perturb_and_get_rank, ev.sort_and_rank

    def single(*a, **k):
        rec['graphs'].append(dict(head=[], tail=[]))
        return orig_single(*a, **k)

    def perturb(*a, **k):
        rec['mode'] = k.get('mode', a[-1] if a and isinstance(a[-1], str) else 'tail')
        return orig_perturb(*a, **k)

    def sort_and_rank(score, target):
        ts = score.gather(1, target.view(-1, 1))
        d = (score - ts).abs()
        d.scatter_(1, target.view(-1, 1), float('inf'))
        rec['graphs'][-1][rec['mode']].append(((d <= GG.G13_BAND) & (score > 1e-30)).sum(1))
        return orig_sort(score, target)

    ev.calc_metrics_single_graph, ev.perturb_and_get_rank, ev.sort_and_rank = single, perturb, sort_and_rank
    with torch.no_grad():
        for split, graph_dict in (("val", va), ("test", te_g)):
            rec['graphs'] = []
            ranks, losses = [], []
            for t in t_list:                                                   # models/TKG_Module.py:253-274 with the projected relation rows
                tt, g = torch.tensor(t), graph_dict[t]
                ent_embed, rel_p = m.get_per_graph_embeds(tt, g)
                all_embeds_g, _ = m.get_per_graph_embeds(tt, all_g)
                index_sample = torch.stack([g.edges()[0], g.edata['type_s'], g.edges()[1]]).transpose(0, 1)
                if index_sample.shape[0] == 0:
                    continue
                label = torch.ones(index_sample.shape[0])
                ranks.append(ev.calc_metrics_single_graph(ent_embed, rel_p, all_embeds_g, index_sample, g, tt))
                losses.append(m.link_classification_loss(ent_embed, rel_p, index_sample, label).item())
            ranks, loss = torch.cat(ranks), float(np.mean(losses))
            nclose = torch.cat([torch.cat(g['head'] + g['tail']) for g in rec['graphs']])     # ranks = [head ranks ; tail ranks] per graph
            assert nclose.shape == ranks.shape
            share = (nclose == 0).float().mean().item()
            out["ranks_" + split], out["nclose_" + split], out["loss_" + split], out["band_free_" + split] = ranks, nclose, loss, share
            print("  G27_eval_hyte %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f" %
                  (split, ranks.numel(), 100.0 * share, ranks.float().mean().item()))
            assert share >= 0.75, (split, share)
    GG.save("G27_eval_hyte", **out)


ALL = dict(G26=gen_G26, G27=gen_G27)

if __name__ == "__main__":
    rh.activate()
    torch.set_num_threads(1)        # the reference's backward sums its scattered rows in thread order: one thread, one order
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
