"""Golden fixtures of the embedding-only baselines (`--module Static / DE`: baselines/Static.py, baselines/DiachronicEmbedding.py on
baselines/TKG_Non_Recurrent.py), recorded from the reference run under the oracle's stand-ins.  Uses oracle/gen_golden.py and
oracle/ref_harness.py as they are (read-only) and writes under tests/golden/:

  G24_de_{complex,distmult,transe}, G24_static_complex
      D = 32, seeded parameters (tests/diachronic_cases.py: seeded_params), three timestamps, 20 negatives.  The reference model's
      forward() with its sampler's draws recorded, then backward(): the loss, d_rel, the non-zero rows of d_ent / d_w / d_b (every
      `*_sub`-th of them when the file would otherwise pass MAX_BYTES), the summed |gradient| of every parameter, 64 seeded rows of
      each get_all_embeds_Gt(t), and the names and shapes of the reference's state_dict().  The slice's times are 0 .. 23: the
      seeded w_temp_ent_embeds is scaled by W_SCALE (recorded) so that t w spans several periods of the sine, the other tables by
      P_SCALE (recorded) so that the scores are of order 1.
  G25_eval_{de,static}
      evaluate() ranks for val and test with the tie-band counts of G13 (band 1.5e-6), ComplEx.  Relation scale G25_REL_SCALE on
      top of P_SCALE: the share of ranks outside every tie band is printed below and asserted >= 0.75 on both splits (the tests'
      cap on rows left out as ambiguous is 0.25); it is 96-98 % on the four splits at scale 3
      (93-96 % at 1; at 10 the sigmoids begin to saturate: 62 % on Static's val split).

    python tools/gen_golden_diachronic.py [G24] [G25]
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as GG  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
from tests.diachronic_cases import params_checksum, seeded_params  # noqa: E402

W_SCALE = 30.0              # |w| up to ~1.3: t w reaches ~30 rad at t = 23, about five periods
P_SCALE = 12.0              # entity rows up to ~0.5, relation rows up to ~1.9: scores of order 1, a loss that depends on the model
G25_REL_SCALE = float(os.environ.get("G25_REL_SCALE", "3"))
N_ALL_ROWS = 64
MAX_BYTES = 600 << 10       # of gradient rows per file (the largest fixture so far is about 0.7 MB)


def _model(module, score_function, seed, rel_scale=None):
    from baselines.DiachronicEmbedding import DiachronicEmbedding
    from baselines.Static import Static
    num_e, num_r, tr, va, te_g = GG.graphs()
    D = 32
    args = rh.make_args(module=module, hidden_size=D, embed_size=D, negative_rate=20, score_function=score_function)
    sd = seeded_params(module, num_e, num_r, D, seed, W_SCALE, P_SCALE)
    csum = params_checksum(sd)
    if rel_scale is not None:
        sd["rel_embeds"] = sd["rel_embeds"] * rel_scale
    torch.manual_seed(0)
    m = {"DE": DiachronicEmbedding, "Static": Static}[module](args, num_e, num_r, tr, va, te_g)
    m.load_state_dict(sd, strict=True)
    own = m.state_dict()
    shapes = np.full((len(own), 2), -1, dtype=np.int64)
    for i, v in enumerate(own.values()):
        shapes[i, :v.dim()] = list(v.shape)
    out = dict(module=module, score_function=score_function, D=D, seed=seed, neg=20, w_scale=W_SCALE, p_scale=P_SCALE, param_checksum=csum,
               times=np.array(list(tr.keys())), sd_names=np.array(list(own)), sd_shapes=shapes)
    return m, out


def gen_G24():
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, module, score_function, seed, idx in (("G24_de_complex", "DE", "complex", 811, [14, 9, 20]),
                                                    ("G24_de_distmult", "DE", "distmult", 812, [3, 22, 11]),
                                                    ("G24_de_transe", "DE", "transE", 813, [17, 5, 23]),
                                                    ("G24_static_complex", "Static", "complex", 814, [14, 9, 20])):
        m, out = _model(module, score_function, seed)
        t_list = [int(times[i]) for i in idx]
        samples = []
        orig_neg = m.corrupter.single_graph_negative_sampling

        def rec_neg(t, g, n):
            res = orig_neg(t, g, n)
            samples.append([x.clone() for x in res[:3]])
            return res

        m.corrupter.single_graph_negative_sampling = rec_neg
        np.random.seed(seed)
        torch.manual_seed(seed)
        loss = m(torch.tensor(t_list))
        loss.backward()
        out.update(t_list=np.array(t_list), loss=loss.item(), n_samples=len(samples))
        for i, (trip, nt, nh) in enumerate(samples):
            out['trip_%d' % i], out['negtail_%d' % i], out['neghead_%d' % i] = trip, nt, nh
        row_rng = np.random.default_rng(seed + 11)
        with torch.no_grad():
            for i, t in enumerate(t_list):
                rows = np.sort(row_rng.choice(num_e, N_ALL_ROWS, replace=False))
                out['all_rows_%d' % i], out['all_%d' % i] = rows, m.get_all_embeds_Gt(torch.tensor(t))[rows].clone()
        grads = [("d_ent", m.ent_embeds.grad)]
        if module == "DE":
            grads += [("d_w", m.w_temp_ent_embeds.grad), ("d_b", m.b_temp_ent_embeds.grad)]
        nz = {k: torch.nonzero(g.abs().sum(1)).view(-1) for k, g in grads}
        total = sum(nz[k].numel() * g.shape[1] * 4 for k, g in grads)
        stride = max(1, -(-total // MAX_BYTES))
        for k, g in grads:
            rows = nz[k][::stride]
            out[k + '_sub'], out[k + '_nz_rows'], out[k + '_nz_vals'] = stride, rows, g[rows]
        out['d_rel'] = m.rel_embeds.grad
        for k, v in m.named_parameters():
            out['gabs_' + k] = v.grad.double().abs().sum().item()
        if module == "DE":
            arg = (torch.tensor(float(max(t_list))) * m.w_temp_ent_embeds).abs().max().item()
            print("  %s: largest |t w| = %.1f rad (%.1f periods)" % (name, arg, arg / (2 * np.pi)))
        print("  %s: loss %.6f, %d samples, non-zero rows %s, every %d-th kept" %
              (name, out["loss"], len(samples), {k: int(v.numel()) for k, v in nz.items()}, stride))
        GG.save(name, **out)


def gen_G25():
    num_e, num_r, tr, va, te_g = GG.graphs()
    times = list(tr.keys())
    for name, module, seed, idx in (("G25_eval_de", "DE", 821, [14, 8, 2]), ("G25_eval_static", "Static", 822, [21, 12, 6])):
        m, out = _model(module, "complex", seed, rel_scale=G25_REL_SCALE)
        t_list = [int(times[i]) for i in idx]
        out.update(t_list=np.array(t_list), rel_scale=G25_REL_SCALE, band=GG.G13_BAND)
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
            for split, val in (("val", True), ("test", False)):
                rec['graphs'] = []
                ranks, loss = m.evaluate(torch.tensor(t_list), val=val)
                nclose = torch.cat([torch.cat(g['head'] + g['tail']) for g in rec['graphs']])     # ranks = [head ranks ; tail ranks] per graph
                assert nclose.shape == ranks.shape
                out["ranks_" + split], out["nclose_" + split], out["loss_" + split] = ranks, nclose, float(loss)
                share = (nclose == 0).float().mean().item()
                print("  %s %s: %d ranks, %.1f%% outside every tie band, mean rank %.1f" %
                      (name, split, ranks.numel(), 100.0 * share, ranks.float().mean().item()))
                assert share >= 0.75, (name, split, share)
        GG.save(name, **out)


ALL = dict(G24=gen_G24, G25=gen_G25)

if __name__ == "__main__":
    rh.activate()
    torch.set_num_threads(1)        # the reference's backward sums its scattered rows in thread order: one thread, one order
    for w in sys.argv[1:] or list(ALL):
        print("== %s" % w)
        ALL[w]()
