"""Golden fixtures of the Aggregator (`--module Aggregator`: models/aggregator.py), recorded from the reference run under the oracle's
stand-ins.  Uses oracle/gen_golden.py and oracle/ref_harness.py as they are (read-only) and writes under tests/golden/.

The reference's class is constructed the NON-debug way: a StaticRGCN and a DynamicRGCN / BiDynamicRGCN of the reference are built at
D = 16, dropout 0, with the oracle's seeded parameters (oracle.temp_oracle.init_model; the relation tables times GG.G13_REL_SCALE so
that the scores spread), saved as run directories -- config.json and checkpoints/*.ckpt with the trainer's extra keys next to
'state_dict' -- in a temporary directory, and models/aggregator.py:54-99 loads them back.  process_args() reads sys.argv, so it is
reset first.  Its DropEdge builds the frequency tables from the full ICEWS14 train.txt; the target timestamps lie far enough inside
the committed slice that every window the tables aggregate over is inside it too (as G19).

Where the reference does not run as it stands:
  * forward() asserts `t_list.tolist() == time_list` (models/aggregator.py:180), but DynamicRGCN.train_embed returns the time lists of
    ALL window positions, so the assertion fails for every window longer than one.  time_list is not used after it: the generator
    wraps train_embed, checks the last position's list against t_list itself and hands t_list on.  Everything else of forward() and
    backward() runs as written (both sub-models are frozen, so the in-place overwrite that breaks G19's backward saves nothing), and
    so does evaluate().
  * `debug` mode builds no `corrupter`, so its forward() cannot draw: it is not recorded.
The entity tables are scaled by ENT_SCALE and the first layer of the MLPs by 0.05: at the init's own size every score is ~1e-3 (a loss
of log(1 + negatives) whatever the weights are), and the features are counts up to ~200, which saturate every sigmoid.

  G30_aggregator_uni / _bi
      the seeds and checksums of the two sub-models, the names and shapes of the reference's state_dict(), the eight MLP tensors
      (drawn here, recorded), the sampler's draws per target graph in the order forward() visits them (descending timestamps), the
      feature rows the two MLPs were fed, the weights they returned, the loss and the gradients of the eight MLP tensors.
  G31_eval_aggregator_uni / _bi
      ranks of val and test at three timestamps from the reference's evaluate(), with the tie-band counts of G13 (band GG.G13_BAND).
      The reference ranks sigmoid(score) in fp32, which ties close scores: the share of ranks outside every tie band is printed,
      recorded and asserted >= 0.75 on both splits.

    python tools/gen_golden_aggregator.py [G30] [G31]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from oracle import temp_oracle as O  # noqa: E402

D, B, L, NEG = 16, 8, 4, 20
ENT_SCALE = 4.0               # the entity tables times this: at the init's own size every score is ~1e-3 and the loss log(1 + negatives)
VARIANTS = {"uni": ("GRRGCN", 801, 811, [14, 9, 19]), "bi": ("BiGRRGCN", 802, 812, [12, 17, 7])}       # module, seeds (spatial, temporal), timestamps
EVAL_TIMES = {"uni": [15, 8, 3], "bi": [16, 11, 5]}


def _write_run(path, args, state):
    os.makedirs(os.path.join(path, "checkpoints"))
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({k: v for k, v in vars(args).items() if isinstance(v, (int, float, str, bool)) or v is None}, f)
    # what the trainer writes next to the weights: the loader must not choke on it
    torch.save({"epoch": 3, "global_step": 120, "state_dict": state, "optimizer_states": [{"state": {}, "param_groups": [{"lr": 1e-3}]}],
                "hparams": {k: v for k, v in vars(args).items() if isinstance(v, (int, float, str, bool))}},
               os.path.join(path, "checkpoints", "_ckpt_epoch_3.ckpt"))


def _aggregator(which):
    from baselines.StaticRGCN import StaticRGCN
    from models.aggregator import Aggregator
    from models.BiDynamicRGCN import BiDynamicRGCN
    from models.DynamicRGCN import DynamicRGCN
    module, seed_s, seed_t, _ = VARIANTS[which]
    num_e, num_r, tr, va, te_g = GG.graphs()
    common = dict(hidden_size=D, embed_size=D, n_bases=B, negative_rate=NEG, train_seq_len=L, test_seq_len=L, batch_size=3, dropout=0.0)
    a_s = rh.make_args(module="SRGCN", **common)
    a_t = rh.make_args(module=module, rec_only_last_layer=True, **common)
    cfg_s = dict(module="SRGCN", n_bases=B, inv_temperature=0.1, rec_only_last_layer=False, use_time_embedding=False)
    cfg_t = dict(module=module, n_bases=B, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=False)
    m_s = O.init_model(cfg_s, num_e, num_r, len(tr), D, seed=seed_s, bias=True)
    m_t = O.init_model(cfg_t, num_e, num_r, len(tr), D, seed=seed_t)
    sums = GG.checksum(m_s), GG.checksum(m_t)
    for m in (m_s, m_t):
        m["rel_embeds"] = m["rel_embeds"] * GG.G13_REL_SCALE
        m["ent_embeds"] = m["ent_embeds"] * ENT_SCALE
    sp = StaticRGCN(a_s, num_e, num_r, tr, va, te_g)
    sp.load_state_dict(GG.to_ref_state_dict(m_s), strict=True)
    tm = (BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN)(a_t, num_e, num_r, tr, va, te_g)
    tm.load_state_dict(GG.to_ref_state_dict(m_t), strict=True)
    with tempfile.TemporaryDirectory() as tmp:
        _write_run(os.path.join(tmp, "spatial"), a_s, sp.state_dict())
        _write_run(os.path.join(tmp, "temporal"), a_t, tm.state_dict())
        sys.argv = sys.argv[:1]                                   # process_args() parses it
        a = rh.make_args(module="Aggregator", temporal_module=module, spatial_checkpoint=os.path.join(tmp, "spatial"),
                         temporal_checkpoint=os.path.join(tmp, "temporal"), **common)
        torch.manual_seed(0)
        m = Aggregator(a, num_e, num_r, tr, va, te_g)
    assert not a.debug and type(m.temporal_model) is (BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN)
    for k, v in sp.state_dict().items():
        assert torch.equal(v, m.state_dict()["spatial_model." + k]), k
    for k, v in tm.state_dict().items():
        assert torch.equal(v, m.state_dict()["temporal_model." + k]), k
    own = m.state_dict()
    shapes = np.full((len(own), 3), -1, dtype=np.int64)
    for i, v in enumerate(own.values()):
        shapes[i, :v.dim()] = list(v.shape)
    out = dict(module=module, D=D, B=B, L=L, neg=NEG, seed_spatial=seed_s, seed_temporal=seed_t, checksum_spatial=sums[0], checksum_temporal=sums[1],
               rel_scale=GG.G13_REL_SCALE, ent_scale=ENT_SCALE, sd_names=np.array(list(own)), sd_shapes=shapes, bidirectional=int(m.bidirectional),
               frozen=int(all(not p.requires_grad for p in list(m.spatial_model.parameters()) + list(m.temporal_model.parameters()))))
    rng = np.random.default_rng(seed_s + seed_t)
    for nm in ("subject_linear", "object_linear"):
        for k, p in getattr(m, nm).named_parameters():
            # (the features are counts up to ~100: first-layer weights of the usual size would saturate every sigmoid)
            v = torch.from_numpy(rng.uniform(-0.6, 0.6, tuple(p.shape)).astype(np.float32)) * (0.05 if k == "0.weight" else 1.0)
            p.data.copy_(v)
            out["mlp_%s.%s" % (nm, k)] = v.clone()
    return m, out


def _check_times(which, idx, n_times):
    assert max(idx) + (L if which == "bi" else 0) <= n_times and min(idx) >= L - 1      # the tables' windows stay inside the slice


def gen_G30():
    for which, (module, _, _, idx) in VARIANTS.items():
        m, out = _aggregator(which)
        times = list(m.graph_dict_train.keys())
        _check_times(which, idx, len(times))
        feats, weights, samples, visited = dict(sub=[], obj=[]), [], [], []
        m.subject_linear.register_forward_pre_hook(lambda mod, inp: feats["sub"].append(inp[0].detach().clone()))
        m.object_linear.register_forward_pre_hook(lambda mod, inp: feats["obj"].append(inp[0].detach().clone()))
        orig_ratio, orig_neg = m.calc_ensemble_ratio, m.corrupter.single_graph_negative_sampling

        def ratio(*a, **k):
            ws, wo = orig_ratio(*a, **k)
            weights.append((ws.detach().clone(), wo.detach().clone()))
            return ws, wo

        def rec_neg(t, g, n):
            res = orig_neg(t, g, n)
            samples.append([x.clone() for x in res[:3]])
            visited.append(int(t))
            return res

        orig_embed = m.temporal_model.train_embed

        def train_embed(t_list):
            # forward() asserts t_list.tolist() == time_list (models/aggregator.py:180), but train_embed returns the time lists of
            # ALL window positions, so the assertion fails for every window longer than one.  time_list is not used after it: the
            # last position's list -- the target timestamps -- is checked here and handed on in the shape the assertion expects.
            res = list(orig_embed(t_list))
            last = res[2][-1] if hasattr(res[2][-1], "__len__") else res[2]        # (the bidirectional class returns the targets alone)
            assert [int(t) for t in last] == t_list.tolist()
            res[2] = t_list.tolist()
            return tuple(res)

        m.temporal_model.train_embed = train_embed
        m.calc_ensemble_ratio, m.corrupter.single_graph_negative_sampling = ratio, rec_neg
        np.random.seed(out["seed_spatial"])
        torch.manual_seed(out["seed_spatial"])
        m.train()                                                  # (dropout 0: the sub-models' mode does not matter)
        loss = m(torch.tensor([int(times[i]) for i in idx]))
        loss.backward()
        n = len(idx)
        assert len(samples) == n and len(weights) == n and len(feats["sub"]) == n and visited == sorted(visited, reverse=True)
        assert all(p.grad is None for p in list(m.spatial_model.parameters()) + list(m.temporal_model.parameters()))
        out.update(t_list=np.array([int(times[i]) for i in idx]), visited=np.array(visited), loss=loss.item(), n_graphs=n)
        for i in range(n):
            out["trip_%d" % i], out["negtail_%d" % i], out["neghead_%d" % i] = samples[i]
            out["feat_sub_%d" % i], out["feat_obj_%d" % i] = feats["sub"][i], feats["obj"][i]
            out["w_sub_%d" % i], out["w_obj_%d" % i] = weights[i]
        for nm in ("subject_linear", "object_linear"):
            for k, p in getattr(m, nm).named_parameters():
                out["grad_%s.%s" % (nm, k)] = p.grad.clone()
        P = sum(s[0].shape[0] for s in samples)
        print("  G30_aggregator_%s: loss %.6f (2 n log(21) = %.6f over %d positives), features up to %.0f, weights %.3f - %.3f"
              % (which, out["loss"], 2 * n * np.log(21.0), P, max(float(f.max()) for f in feats["sub"] + feats["obj"]),
                 min(float(w.min()) for ws in weights for w in ws), max(float(w.max()) for ws in weights for w in ws)))
        GG.save("G30_aggregator_" + which, **out)


def gen_G31():
    for which in VARIANTS:
        m, out = _aggregator(which)
        times = list(m.graph_dict_train.keys())
        idx = EVAL_TIMES[which]
        _check_times(which, idx, len(times))
        t_list = [int(times[i]) for i in idx]
        out.update(t_list=np.array(t_list), band=GG.G13_BAND)
        rec = dict(graphs=[])
        orig_single, orig_sort = m.calc_metrics_single_graph, m.sort_and_rank

        def single(*a, **k):
            rec["graphs"].append([])
            return orig_single(*a, **k)

        def sort_and_rank(score, target):
            ts = score.gather(1, target.view(-1, 1))
            d = (score - ts).abs()
            d.scatter_(1, target.view(-1, 1), float("inf"))
            rec["graphs"][-1].append(((d <= GG.G13_BAND) & (score > 1e-30)).sum(1))
            return orig_sort(score, target)

        m.calc_metrics_single_graph, m.sort_and_rank = single, sort_and_rank
        m.eval()
        with torch.no_grad():
            for split, val in (("val", True), ("test", False)):
                rec["graphs"] = []
                ranks, _ = m.evaluate(torch.tensor(t_list), val=val)
                # per graph the class ranks the objects first, then the subjects; ranks = [subject ranks ; object ranks]
                nclose = torch.cat([torch.cat([g[1], g[0]]) for g in rec["graphs"]])
                assert nclose.shape == ranks.shape
                share = (nclose == 0).float().mean().item()
                out["ranks_" + split], out["nclose_" + split], out["band_free_" + split] = ranks, nclose, share
                print("  G31_eval_aggregator_%s %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f"
                      % (which, split, ranks.numel(), 100.0 * share, ranks.float().mean().item()))
                assert share >= 0.75, (which, split, share)
        GG.save("G31_eval_aggregator_" + which, **out)


ALL = dict(G30=gen_G30, G31=gen_G31)

if __name__ == "__main__":
    rh.activate()
    torch.set_num_threads(1)
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
