"""Golden fixtures of the post-aggregation models (`--post-aggregation`: PostDynamicRGCN / PostBiDynamicRGCN,
models/PostDynamicRGCN.py:146-321, models/PostBiDynamicRGCN.py:179-282), recorded from the reference run under the oracle's
stand-ins.  Uses oracle/gen_golden.py and oracle/ref_harness.py as they are (read-only) and writes under tests/golden/:

  G20_post_agg_uni       PostDynamicRGCN (GRRGCN, --rec-only-last-layer).forward with the reference's OWN calc_ensemble_ratio
  G20_post_agg_bi        PostBiDynamicRGCN (BiGRRGCN, --rec-only-last-layer)
  G20_post_agg_uni_full  PostDynamicRGCN (GRRGCN, both layers recurrent)
      seeded weights of all four 3-3-1 MLPs, the feature rows the gate MLPs were fed, the recorded draws and the forward loss
      (the reference's backward of this forward() fails under torch 2.x -- the in-place row overwrite of the all-entity matrices
      documented for G19 -- so no gradients are recorded)
  G21_eval_post_agg_{uni,bi}
      evaluate() ranks with the model's own gates (PostEvaluationFilter), with the tie bands of G13 / G18.

    python tools/gen_golden_post_aggregation.py [G20] [G21]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from oracle import temp_oracle as O  # noqa: E402

MLPS = ("subject_query_subject_embed_linear", "object_query_subject_embed_linear",
        "subject_query_object_embed_linear", "object_query_object_embed_linear")


def seed_mlps(m, seed, mlp):
    """Uniform(-0.6, 0.6) weights for the four MLPs (recorded under mlp_<state_dict key>)."""
    rng = np.random.default_rng(seed + 5)
    for nm in MLPS:
        for k, p in getattr(m, nm).named_parameters():
            v = torch.from_numpy(rng.uniform(-0.6, 0.6, tuple(p.shape)).astype(np.float32))
            p.data.copy_(v)
            mlp["mlp_%s.%s" % (nm, k)] = v.clone()


def gen_G20():
    from models.PostBiDynamicRGCN import PostBiDynamicRGCN
    from models.PostDynamicRGCN import PostDynamicRGCN
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, cls, module, rec_only, seed, idx in (("G20_post_agg_uni", PostDynamicRGCN, 'GRRGCN', True, 741, [14, 9, 20]),
                                                   ("G20_post_agg_bi", PostBiDynamicRGCN, 'BiGRRGCN', True, 742, [12, 18, 7]),
                                                   ("G20_post_agg_uni_full", PostDynamicRGCN, 'GRRGCN', False, 743, [16, 10, 21])):
        L = 6
        assert [int(x) for x in times] == list(range(len(times)))
        assert max(idx) + (L if module.startswith("Bi") else 0) <= len(times)      # the tables' windows stay inside the slice
        feats = dict(sub=[], obj=[])
        mlp = {}

        def tweak(m):
            seed_mlps(m, seed, mlp)
            # calc_ensemble_ratio calls each of these two MLPs twice per graph on the same rows (w_sqs / w_sqo, w_oqs / w_oqo)
            m.subject_query_subject_embed_linear.register_forward_pre_hook(lambda mod, inp: feats["sub"].append(inp[0].detach().clone()))
            m.object_query_subject_embed_linear.register_forward_pre_hook(lambda mod, inp: feats["obj"].append(inp[0].detach().clone()))

        out = GG._run_window(cls, module, rec_only, 32, 16, seed, [int(times[i]) for i in idx], L, 4, 20,
                             extra_args=dict(post_aggregation=True), tweak=tweak, backward=False)
        out.update(mlp)
        out["post_aggregation"] = 1
        assert len(feats["sub"]) == 2 * len(idx) and len(feats["obj"]) == 2 * len(idx)
        for i in range(len(idx)):
            assert torch.equal(feats["sub"][2 * i], feats["sub"][2 * i + 1]) and torch.equal(feats["obj"][2 * i], feats["obj"][2 * i + 1])
            out["feat_sub_%d" % i], out["feat_obj_%d" % i] = feats["sub"][2 * i], feats["obj"][2 * i]
        print("  %s: loss %.6f, features up to %.0f" % (name, out["loss"], max(float(f.max()) for f in feats["sub"] + feats["obj"])))
        GG.save(name, **out)


def gen_G21():
    from models.PostBiDynamicRGCN import PostBiDynamicRGCN
    from models.PostDynamicRGCN import PostDynamicRGCN
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, cls, module, seed, idx in (("G21_eval_post_agg_uni", PostDynamicRGCN, 'GRRGCN', 751, [14, 8, 2]),
                                         ("G21_eval_post_agg_bi", PostBiDynamicRGCN, 'BiGRRGCN', 752, [18, 12, 6])):
        D, B, L = 32, 16, 6
        assert max(idx) + (L if module.startswith("Bi") else 0) <= len(times)      # the gates' frequency windows stay inside the slice
        args = rh.make_args(module=module, rec_only_last_layer=True, hidden_size=D, embed_size=D, n_bases=B,
                            train_seq_len=L, test_seq_len=L, batch_size=4, negative_rate=20, post_aggregation=True)
        cfg = dict(module=module, n_bases=B, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=False)
        model = O.init_model(cfg, num_e, num_r, len(tr), D, seed=seed)
        csum = GG.checksum(model)
        model['rel_embeds'] = model['rel_embeds'] * GG.G13_REL_SCALE
        m = cls(args, num_e, num_r, tr, va, te_g)
        missing = m.load_state_dict(GG.to_ref_state_dict(model), strict=False)
        assert not missing.unexpected_keys and all("_linear" in k for k in missing.missing_keys), missing
        mlp = {}
        seed_mlps(m, seed, mlp)
        t_list = [int(times[i]) for i in idx]
        out = dict(module=module, rec_only=1, D=D, B=B, seed=seed, L=L, te=0, neg=20, t_list=np.array(t_list), post_aggregation=1,
                   param_checksum=csum, rel_scale=GG.G13_REL_SCALE, band=GG.G13_BAND)
        out.update(mlp)
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
                print("  %s %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f" %
                      (name, split, ranks.numel(), 100.0 * (nclose == 0).float().mean().item(), ranks.float().mean().item()))
        GG.save(name, **out)


ALL = dict(G20=gen_G20, G21=gen_G21)

if __name__ == "__main__":
    rh.activate()
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
