"""Golden fixtures of the post-aggregation ATTENTION models (`--module SARGCN / BiSARGCN --post-aggregation`:
PostSelfAttentionRGCN / PostBiSelfAttentionRGCN, models/PostSelfAttentionRGCN.py), recorded from the reference run under the
oracle's stand-ins.  Uses oracle/gen_golden.py and oracle/ref_harness.py as they are (read-only) and writes under tests/golden/:

  G22_post_sa_uni        PostSelfAttentionRGCN (SARGCN, --rec-only-last-layer).forward with the reference's own gates
  G22_post_sa_bi         PostBiSelfAttentionRGCN (BiSARGCN, --rec-only-last-layer)
  G22_post_sa_uni_learn  PostSelfAttentionRGCN with --learnable-lambda
      D = 32, 16 bases, L = 6, 20 negatives, ComplEx.  Recorded draws and samples, seeded weights of the four 3-3-1 MLPs, the
      feature rows the gate MLPs were fed, the loss AND its gradients (non-zero d_ent rows, d_rel, gabs_ of every parameter --
      unlike G20 the reference's backward runs here; every second non-zero d_ent row, see D_ENT_STRIDE), and per window the
      (loc, rec) target rows and 64 seeded rows of all_loc / all_rec (at least half of them entities that are inactive in the
      window's target graph).
  G23_eval_post_sa_{uni,bi}
      evaluate() ranks for val and test with the model's own gates (PostEvaluationFilter), with the tie-band counts of G21
      (band 1.5e-6).  Relation scale 18, not G13's 250: at 250 the gated scores saturate the sigmoid and only 32-57 % of the ranks
      lie outside every tie band; at 18 it is 84-89 % on all four splits (printed below; the tests' cap is 0.75).

    python tools/gen_golden_post_attention.py [G22] [G23]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from oracle import temp_oracle as O  # noqa: E402
from gen_golden_post_aggregation import seed_mlps  # noqa: E402

G23_REL_SCALE = 18.0
N_ALL_ROWS = 64
D_ENT_STRIDE = 2
DECAY = (0.25, -0.1)        # exponential_decay (weight, bias) of the --learnable-lambda fixtures, as G14's


def _model(cls, module, learn, seed, L, rel_scale=None):
    num_e, num_r, tr, va, te_g = GG.graphs()
    D, B = 32, 16
    args = rh.make_args(module=module, rec_only_last_layer=True, hidden_size=D, embed_size=D, n_bases=B, train_seq_len=L,
                        test_seq_len=L, batch_size=4, negative_rate=20, learnable_lambda=learn, EMA=False, post_aggregation=True)
    cfg = dict(module=module, n_bases=B, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=True, learnable_lambda=learn)
    model = O.init_model(cfg, num_e, num_r, len(tr), D, seed=seed)
    if learn:
        for ln in ('layer_1', 'layer_2'):
            model['ent_encoder'][ln]['exponential_decay'] = (torch.full((1, 1), DECAY[0]), torch.full((1,), DECAY[1]))
    csum = GG.checksum(model)
    if rel_scale is not None:
        model['rel_embeds'] = model['rel_embeds'] * rel_scale
    torch.manual_seed(0)
    m = cls(args, num_e, num_r, tr, va, te_g)
    missing = m.load_state_dict(GG.to_ref_state_dict(model), strict=False)
    assert not missing.unexpected_keys, missing
    assert all(('exponential_decay' in k or '_linear' in k) for k in missing.missing_keys), missing
    mlp = {}
    seed_mlps(m, seed, mlp)
    out = dict(module=module, rec_only=1, learn=int(learn), D=D, B=B, seed=seed, L=L, neg=20, te=1, post_aggregation=1,
               param_checksum=csum, times=np.array(list(tr.keys())))
    out.update(mlp)
    return m, out


def gen_G22():
    from models.PostSelfAttentionRGCN import PostBiSelfAttentionRGCN, PostSelfAttentionRGCN
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, cls, module, learn, seed, idx in (("G22_post_sa_uni", PostSelfAttentionRGCN, 'SARGCN', False, 741, [14, 9, 20]),
                                                ("G22_post_sa_bi", PostBiSelfAttentionRGCN, 'BiSARGCN', False, 742, [12, 18, 7]),
                                                ("G22_post_sa_uni_learn", PostSelfAttentionRGCN, 'SARGCN', True, 744, [14, 9, 20])):
        L = 6
        assert [int(x) for x in times] == list(range(len(times)))
        assert max(idx) + (L if module.startswith("Bi") else 0) <= len(times)      # the tables' windows stay inside the slice
        m, out = _model(cls, module, learn, seed, L)
        t_list = [int(times[i]) for i in idx]
        feats = dict(sub=[], obj=[])
        # calc_ensemble_ratio calls each of these two MLPs twice per graph on the same rows (w_sqs / w_sqo, w_oqs / w_oqo)
        m.subject_query_subject_embed_linear.register_forward_pre_hook(lambda mod, inp: feats["sub"].append(inp[0].detach().clone()))
        m.object_query_subject_embed_linear.register_forward_pre_hook(lambda mod, inp: feats["obj"].append(inp[0].detach().clone()))
        np.random.seed(seed)
        choices, samples, streams, alls = [], [], [], []
        orig_choice = np.random.choice

        def rec_choice(*a, **k):
            r = orig_choice(*a, **k)
            choices.append(np.asarray(r).copy())
            return r

        orig_neg = m.corrupter.single_graph_negative_sampling

        def rec_neg(t, g, n):
            res = orig_neg(t, g, n)
            samples.append([x.clone() for x in res[:3]])
            return res

        orig_final, orig_all = m.get_final_graph_embeds, m.get_all_embeds_Gt

        def rec_final(*a, **k):
            loc, rec = orig_final(*a, **k)
            streams.append(([x.detach().clone() for x in loc], [x.detach().clone() for x in rec]))
            return loc, rec

        row_rng = np.random.default_rng(seed + 11)

        def rec_all(loc, rec, g, t, *a, **k):
            a_loc, a_rec = orig_all(loc, rec, g, t, *a, **k)
            act = np.array(sorted(g.ids.values()), dtype=np.int64)
            inact = np.setdiff1d(np.arange(num_e, dtype=np.int64), act)
            n_in = min(len(inact), max(N_ALL_ROWS // 2, N_ALL_ROWS - len(act)))
            rows = np.sort(np.concatenate([row_rng.choice(inact, n_in, replace=False), row_rng.choice(act, N_ALL_ROWS - n_in, replace=False)]))
            alls.append((rows, int(np.isin(rows, inact).sum()), a_loc.detach()[rows].clone(), a_rec.detach()[rows].clone()))
            return a_loc, a_rec

        m.corrupter.single_graph_negative_sampling = rec_neg
        m.get_final_graph_embeds, m.get_all_embeds_Gt = rec_final, rec_all
        np.random.choice = rec_choice
        try:
            loss = m(torch.tensor(t_list))
        finally:
            np.random.choice = orig_choice
        loss.backward()
        out.update(t_list=np.array(t_list), loss=loss.item(), n_choices=len(choices), n_samples=len(samples))
        for i, c in enumerate(choices):
            out['choice_%d' % i] = c
        for i, (trip, nt, nh) in enumerate(samples):
            out['trip_%d' % i], out['negtail_%d' % i], out['neghead_%d' % i] = trip, nt, nh
        assert len(streams) == 1 and len(alls) == len(idx) == len(streams[0][0])
        for i in range(len(idx)):
            out['loc_%d' % i], out['rec_%d' % i] = streams[0][0][i], streams[0][1][i]
            rows, n_in, a_loc, a_rec = alls[i]
            assert 2 * n_in >= N_ALL_ROWS
            out['all_rows_%d' % i], out['all_loc_%d' % i], out['all_rec_%d' % i] = rows, a_loc, a_rec
        assert len(feats["sub"]) == 2 * len(idx) and len(feats["obj"]) == 2 * len(idx)
        for i in range(len(idx)):
            assert torch.equal(feats["sub"][2 * i], feats["sub"][2 * i + 1]) and torch.equal(feats["obj"][2 * i], feats["obj"][2 * i + 1])
            out["feat_sub_%d" % i], out["feat_obj_%d" % i] = feats["sub"][2 * i], feats["obj"][2 * i]
        eg = m.ent_embeds.grad
        nz = torch.nonzero(eg.abs().sum(1)).view(-1)
        # (the candidates' all-entity rows reach nearly every entity: every second non-zero row keeps the file under the size
        #  limit for a committed file; gabs_ent_embeds holds the sum over all of them)
        nz = nz[::D_ENT_STRIDE]
        out['d_ent_sub'] = D_ENT_STRIDE
        out['d_ent_nz_rows'], out['d_ent_nz_vals'], out['d_rel'] = nz, eg[nz], m.rel_embeds.grad
        n_grad = 0
        for k, v in m.named_parameters():
            if v.grad is not None:
                out['gabs_' + k] = v.grad.double().abs().sum().item()
                n_grad += 1
        trained = [k for k in out if k.startswith("gabs_") and "_embed_linear" in k]
        assert len(trained) == 8 and all("_subject_embed_linear" in k for k in trained), trained       # the two MLPs that train
        print("  %s: loss %.6f, %d parameters with a gradient, %d non-zero d_ent rows, features up to %.0f" %
              (name, out["loss"], n_grad, nz.numel(), max(float(f.max()) for f in feats["sub"] + feats["obj"])))
        GG.save(name, **out)


def gen_G23():
    from models.PostSelfAttentionRGCN import PostBiSelfAttentionRGCN, PostSelfAttentionRGCN
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, cls, module, seed, idx in (("G23_eval_post_sa_uni", PostSelfAttentionRGCN, 'SARGCN', 761, [14, 8, 2]),
                                         ("G23_eval_post_sa_bi", PostBiSelfAttentionRGCN, 'BiSARGCN', 762, [18, 12, 6])):
        L = 6
        assert max(idx) + (L if module.startswith("Bi") else 0) <= len(times)      # the gates' frequency windows stay inside the slice
        m, out = _model(cls, module, False, seed, L, rel_scale=G23_REL_SCALE)
        t_list = [int(times[i]) for i in idx]
        out.update(t_list=np.array(t_list), rel_scale=G23_REL_SCALE, band=GG.G13_BAND)
        ev = m.evaluater
        rec = dict(graphs=[])
        orig_single, orig_sort = ev.calc_metrics_single_graph, ev.sort_and_rank

        def single(*a, **k):
            rec['graphs'].append(([], int(a[5].shape[0])))
            return orig_single(*a, **k)

        def sort_and_rank(score, target):
            ts = score.gather(1, target.view(-1, 1))
            d = (score - ts).abs()
            d.scatter_(1, target.view(-1, 1), float('inf'))
            rec['graphs'][-1][0].append(((d <= GG.G13_BAND) & (score > 1e-30)).sum(1))
            return orig_sort(score, target)

        ev.calc_metrics_single_graph, ev.sort_and_rank = single, sort_and_rank
        with torch.no_grad():
            for split, val in (("val", True), ("test", False)):
                rec['graphs'] = []
                ranks, _ = m.evaluate(torch.tensor(t_list), val=val)
                # per graph the filter ranks tails first, then heads (in batches of eval_bz); ranks = [head ranks ; tail ranks]
                parts = []
                for lst, P in rec['graphs']:
                    nc = torch.cat(lst)
                    assert nc.shape[0] == 2 * P
                    parts.append(torch.cat([nc[P:], nc[:P]]))
                nclose = torch.cat(parts)
                assert nclose.shape == ranks.shape
                out["ranks_" + split], out["nclose_" + split] = ranks, nclose
                share = (nclose == 0).float().mean().item()
                print("  %s %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f" %
                      (name, split, ranks.numel(), 100.0 * share, ranks.float().mean().item()))
                assert share > 0.75, (name, split, share)
        GG.save(name, **out)


ALL = dict(G22=gen_G22, G23=gen_G23)

if __name__ == "__main__":
    rh.activate()
    torch.set_num_threads(1)        # the reference's backward sums its scattered rows in thread order: one thread, one order
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
