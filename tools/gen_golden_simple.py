"""Golden fixtures of the SimplE baseline (`--module Simple`: baselines/Simple.py on baselines/TKG_Non_Recurrent.py), recorded from the
reference run under the oracle's stand-ins.  Uses oracle/gen_golden.py and oracle/ref_harness.py as they are (read-only) and writes
under tests/golden/.

The reference's SimplE.forward and its SimpleEvaluationFilter do not run as written (the sampler and the filter with older
signatures).  What does run defines the model, composed as TKG_Non_Recurrent.forward and TKG_Module.calc_metrics compose it: the
constructor, SimplE.train_link_prediction on the all-entity tables with the positives' global ids, the sampler's three-argument form,
and the BASE EvaluationFilter.calc_metrics_single_graph given a three-argument scorer -- here a wrapper that splits pair rows
[x | x_inv] and calls the reference's utils.scores.simple, i.e. the score the model is trained with.

  G28_simple
      D = 16, seeded parameters (tests/simple_cases.py: seeded_params) with the entity / relation tables times G28_ENT_SCALE /
      G28_REL_SCALE (scores of order 1; at the init's own size they are ~1e-4 and the loss log(1 + negatives) whatever the model
      does), the three training timestamps with the fewest edges, 20 negatives.  The loss sum_t tail + head of the recorded draws,
      then backward(): d_rel, d_rel_inv, the non-zero rows of d_ent and d_ent_inv (thinned under the file cap), the summed |gradient|
      of every parameter, the names and shapes of the reference's state_dict(), and the checksum of the parameters the reference's
      constructor draws under torch.manual_seed(0).
  G29_eval_simple
      ranks of val and test at three timestamps from the reference's base EvaluationFilter under the wrapper, the classification
      loss binary_cross_entropy_with_logits of the same score in 'single' mode, the tie-band counts of G13 (band GG.G13_BAND).  The
      reference ranks sigmoid(score) in fp32, which ties close scores: the share of ranks outside every tie band is printed,
      recorded and asserted >= 0.75 on both splits.

    python tools/gen_golden_simple.py [G28] [G29]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from tests.simple_cases import params_checksum, seeded_params  # noqa: E402

D = 16
G28_SEED, G28_ENT_SCALE, G28_REL_SCALE = 41, 24.0, 6.0
G28_TIMES = (18, 0, 4)                        # the three training timestamps with the fewest edges (86, 91, 93), as G26
G29_SEED, G29_ENT_SCALE, G29_REL_SCALE = 5, 24.0, 6.0
G29_TIMES = (14, 8, 2)
MAX_BYTES = 300 << 10                         # per sparse gradient: two of them in the file


def _model(seed, ent_scale, rel_scale):
    from baselines.Simple import SimplE
    num_e, num_r, tr, va, te_g = GG.graphs()
    args = rh.make_args(module="Simple", hidden_size=D, embed_size=D, negative_rate=20, score_function="complex")
    torch.manual_seed(0)
    m = SimplE(args, num_e, num_r, tr, va, te_g)
    init_checksum = params_checksum(m.state_dict())
    sd = seeded_params(num_e, num_r, D, seed, ent_scale, rel_scale)
    m.load_state_dict(sd, strict=True)
    own = m.state_dict()
    shapes = np.full((len(own), 2), -1, dtype=np.int64)
    for i, v in enumerate(own.values()):
        shapes[i, :v.dim()] = list(v.shape)
    out = dict(module="Simple", score_function="simple", D=D, seed=seed, neg=20, ent_scale=ent_scale, rel_scale=rel_scale,
               param_checksum=params_checksum(sd), init_checksum=init_checksum, times=np.array(list(tr.keys())),
               sd_names=np.array(list(own)), sd_shapes=shapes)
    return m, out


def _sparse(out, key, g):
    nz = torch.nonzero(g.abs().sum(1)).view(-1)
    stride = max(1, -(-(nz.numel() * g.shape[1] * 4) // MAX_BYTES))
    rows = nz[::stride]
    out[key + '_sub'], out[key + '_nz_rows'], out[key + '_nz_vals'] = stride, rows, g[rows]
    return nz.numel(), stride


def gen_G28():
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    t_list = [int(times[i]) for i in G28_TIMES]
    m, out = _model(G28_SEED, G28_ENT_SCALE, G28_REL_SCALE)
    np.random.seed(G28_SEED)
    torch.manual_seed(G28_SEED)
    loss, samples, size = 0, [], []
    for t in t_list:
        tt = torch.tensor(t)
        g = m.graph_dict_train[t]
        trip, neg_tail, neg_head, labels = m.corrupter.single_graph_negative_sampling(tt, g, m.num_ents)
        samples.append([x.clone() for x in (trip, neg_tail, neg_head)])
        gids = g.ndata['id'].view(-1)
        trip_g = torch.stack([gids[trip[:, 0]], trip[:, 1], gids[trip[:, 2]]], dim=1)
        loss = loss + m.train_link_prediction(m.ent_embeds, m.ent_embeds_inv, trip_g, neg_tail, labels, corrupt_tail=True) \
            + m.train_link_prediction(m.ent_embeds, m.ent_embeds_inv, trip_g, neg_head, labels, corrupt_tail=False)
        with torch.no_grad():
            from utils.scores import simple
            s = simple(m.ent_embeds[trip_g[:, 0]], m.ent_embeds_inv[trip_g[:, 0]], m.rel_embeds[trip_g[:, 1]], m.rel_embeds_inv[trip_g[:, 1]],
                       m.ent_embeds[neg_tail], m.ent_embeds_inv[neg_tail], mode='tail')
            size.append(float(s.abs().mean()))
    loss.backward()
    out.update(t_list=np.array(t_list), loss=loss.item(), n_samples=len(samples), score_size=float(np.mean(size)))
    for i, (trip, nt, nh) in enumerate(samples):
        out['trip_%d' % i], out['negtail_%d' % i], out['neghead_%d' % i] = trip, nt, nh
    n_nz, stride = _sparse(out, 'd_ent', m.ent_embeds.grad)
    n_nz_inv, stride_inv = _sparse(out, 'd_ent_inv', m.ent_embeds_inv.grad)
    out['d_rel'], out['d_rel_inv'] = m.rel_embeds.grad, m.rel_embeds_inv.grad
    for k, v in m.named_parameters():
        out['gabs_' + k] = v.grad.double().abs().sum().item()
    print("  G28_simple: loss %.6f (6 log(21) = %.6f), mean |score| %.3f, %d / %d non-zero d_ent / d_ent_inv rows, every %d-th / %d-th kept"
          % (out["loss"], 6 * np.log(21.0), out["score_size"], n_nz, n_nz_inv, stride, stride_inv))
    assert 0.1 <= out["score_size"] <= 10.0, "scores of order 1"
    GG.save("G28_simple", **out)


def pair_scorer(s, r, o, mode='single'):
    """The reference's SimplE score on pair rows [x | x_inv]."""
    from utils.scores import simple
    h = s.shape[-1] // 2
    return simple(s[..., :h], s[..., h:], r[..., :h], r[..., h:], o[..., :h], o[..., h:], mode=mode)


def gen_G29():
    from utils.evaluation import EvaluationFilter
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    m, out = _model(G29_SEED, G29_ENT_SCALE, G29_REL_SCALE)
    t_list = [int(times[i]) for i in G29_TIMES]
    out.update(t_list=np.array(t_list), band=GG.G13_BAND)
    ev = EvaluationFilter(m.args, pair_scorer, tr, va, te_g)
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
        ent_pair = torch.cat([m.ent_embeds, m.ent_embeds_inv], dim=1)
        rel_pair = torch.cat([m.rel_embeds, m.rel_embeds_inv], dim=1)
        for split, graph_dict in (("val", va), ("test", te_g)):
            rec['graphs'] = []
            ranks, losses = [], []
            for t in t_list:                                                   # models/TKG_Module.py:253-274 on the pair tables
                tt, g = torch.tensor(t), graph_dict[t]
                ent_embed = ent_pair[g.ndata['id'].view(-1)]
                index_sample = torch.stack([g.edges()[0], g.edata['type_s'], g.edges()[1]]).transpose(0, 1)
                if index_sample.shape[0] == 0:
                    continue
                label = torch.ones(index_sample.shape[0])
                ranks.append(ev.calc_metrics_single_graph(ent_embed, rel_pair, ent_pair, index_sample, g, tt))
                score = pair_scorer(ent_embed[index_sample[:, 0]], rel_pair[index_sample[:, 1]], ent_embed[index_sample[:, 2]], mode='single')
                losses.append(F.binary_cross_entropy_with_logits(score, label).item())
            ranks, loss = torch.cat(ranks), float(np.mean(losses))
            nclose = torch.cat([torch.cat(g['head'] + g['tail']) for g in rec['graphs']])     # ranks = [head ranks ; tail ranks] per graph
            assert nclose.shape == ranks.shape
            share = (nclose == 0).float().mean().item()
            out["ranks_" + split], out["nclose_" + split], out["loss_" + split], out["band_free_" + split] = ranks, nclose, loss, share
            print("  G29_eval_simple %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f" %
                  (split, ranks.numel(), 100.0 * share, ranks.float().mean().item()))
            assert share >= 0.75, (split, share)
    GG.save("G29_eval_simple", **out)


ALL = dict(G28=gen_G28, G29=gen_G29)

if __name__ == "__main__":
    rh.activate()
    torch.set_num_threads(1)        # the reference's backward sums its scattered rows in thread order: one thread, one order
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
