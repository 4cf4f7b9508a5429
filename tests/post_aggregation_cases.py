"""Cases of the post-aggregation models (PostDynamicRGCN / PostBiDynamicRGCN, `--post-aggregation`) shared by the CPU (test
backend) and GPU (HIP) suites: goldens G20 (loss with the reference's own gates) / G21 (evaluate() ranks), the loss and every
gradient of the fused gated node against an fp64 restatement of the reference formula, and the reference's quirks."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import temp_oracle as O
from tests.golden_util import T, assert_close, load
from tests.window_cases import build_post_model, slice_snapshots, make_args, window_inputs

MLPS = ("subject_query_subject_embed_linear", "object_query_subject_embed_linear",
        "subject_query_object_embed_linear", "object_query_object_embed_linear")


def _cls(bi):
    from temp_amd.post_dynamic_rgcn import PostBiDynamicRGCN, PostDynamicRGCN
    return PostBiDynamicRGCN if bi else PostDynamicRGCN


def load_golden_model(z, device, batched):
    """The fixture's model with the reference-shaped state_dict loaded STRICTLY (encoder + all 16 MLP keys)."""
    m = build_post_model(z, device, _cls(str(z["module"]).startswith("Bi")), batched, post_aggregation=True)
    mlp = {k[len("mlp_"):]: T(z[k]) for k in z.files if k.startswith("mlp_")}
    assert len(mlp) == 16 and sorted(mlp) == sorted(k for k in m.state_dict() if "_linear." in k)
    sd = {k: v for k, v in m.state_dict().items() if "_linear." not in k}
    sd.update(mlp)
    m.load_state_dict(sd, strict=True)
    return m


def check_g20(name, device, batched=True):
    """forward() with the model's own gates: feature rows equal the reference's, loss within 3e-5 relative of G20's; the two
    *_object_embed_linear MLPs get no gradient (the reference computes w_sqo / w_oqo with the *_subject_embed_linear ones)."""
    z = load(name)
    m = load_golden_model(z, device, batched)
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    wb = m.prepare(t_list, int(z["L"]), True, edge_ids)
    for i, g in enumerate(wb.graphs):
        sub_f, obj_f = m.ensemble_features(samples[i][0], wb.rows[i][-1], g)
        assert torch.equal(sub_f.cpu(), T(z["feat_sub_%d" % i])), (name, i, "subject features")
        assert torch.equal(obj_f.cpu(), T(z["feat_obj_%d" % i])), (name, i, "object features")
    loss = m.run_loss(wb, samples)
    want = float(z["loss"])
    assert abs(loss.item() - want) < 3e-5 * abs(want), (name, loss.item(), want)
    loss.backward()
    assert m.subject_query_subject_embed_linear[0].weight.grad.abs().sum() > 0
    assert m.object_query_subject_embed_linear[2].bias.grad.abs().sum() > 0
    for nm in ("subject_query_object_embed_linear", "object_query_object_embed_linear"):
        assert all(p.grad is None for p in getattr(m, nm).parameters()), nm
    assert m.ent_embeds.grad.abs().sum() > 0
    return m


def check_g21(name, device, batched=True):
    """evaluate() with the model's own gates (PostEvaluationFilter) against the reference's ranks outside the tie band."""
    z = load(name)
    m = load_golden_model(z, device, batched)
    with torch.no_grad():
        m.rel_embeds.mul_(float(z["rel_scale"]))
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    for split, val in (("val", True), ("test", False)):
        ranks, _ = m.evaluate(t_list, val=val)
        want, nclose = T(z["ranks_" + split]).long(), T(z["nclose_" + split]).long()
        got = ranks.cpu()
        assert got.shape == want.shape
        safe = nclose == 0
        assert safe.float().mean().item() > 0.85, (name, split)
        assert torch.equal(got[safe], want[safe]), (name, split, int((got[safe] != want[safe]).sum()))
        assert bool(((got - want).abs() <= nclose).all()), (name, split)


def reference_loss64(kind, loc, rec, rel, a_loc, a_rec, trip, nt, nh, w_sqs, w_sqo, w_oqs, w_oqo):
    """models/PostDynamicRGCN.py:261-282 restated (any dtype): loss_tail + loss_head of one graph."""
    lab = torch.zeros(trip.shape[0], dtype=torch.int64, device=trip.device)
    r = rel[trip[:, 1]]
    s = w_oqs * loc[trip[:, 0]] + (1 - w_oqs) * rec[trip[:, 0]]
    neg_o = w_oqo.unsqueeze(-1) * a_loc[nt] + (1 - w_oqo).unsqueeze(-1) * a_rec[nt]
    o_rec = rec[trip[:, 2]]
    o = w_sqo * o_rec + (1 - w_sqo) * o_rec
    neg_s = w_sqs.unsqueeze(-1) * a_loc[nh] + (1 - w_sqs).unsqueeze(-1) * a_rec[nh]
    st = O.SCORERS[kind](s, r, neg_o, "tail")
    sh = O.SCORERS[kind](neg_s, r, o, "head")
    return F.cross_entropy(st, lab) + F.cross_entropy(sh, lab)


def _frob(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def check_gated_loss_definition(device, kind="complex", bi=True, windows=3, P=37, C=21, D=32, full_bar=False):
    """The fused gated node (model.batched_gated_loss over several windows, one of them empty) against the fp64 restatement of the
    reference formula: loss and the gradients of the local rows, temporal rows, both all-entity stacks, rel_embeds and all four
    gates.  full_bar: relative Frobenius <= 6e-6 only (large cases); else elementwise too."""
    s = slice_snapshots()
    args = make_args(module="BiGRRGCN" if bi else "GRRGCN", rec_only_last_layer=True, post_aggregation=True, score_function=kind,
                     embed_size=D, hidden_size=D)
    torch.manual_seed(8)
    m = _cls(bi)(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(device)
    N, R2 = s["num_e"], 2 * s["num_r"]
    gen = torch.Generator().manual_seed(3)
    sizes = [60 + 7 * b for b in range(windows)]
    Ps = [P if b != 1 else 0 for b in range(windows)]
    mk = lambda *shape: (torch.randn(*shape, generator=gen) * 0.4)
    loc, rec = mk(sum(sizes), D), mk(sum(sizes), D)
    big_loc, big_rec = mk(windows, N, D), mk(windows, N, D)
    samples, gates = [], []
    for b in range(windows):
        p = Ps[b]
        trip = torch.stack([torch.randint(0, sizes[b], (p,), generator=gen), torch.randint(0, R2, (p,), generator=gen),
                            torch.randint(0, sizes[b], (p,), generator=gen)], dim=1)
        nt, nh = torch.randint(0, N, (p, C), generator=gen), torch.randint(0, N, (p, C), generator=gen)
        nt[:, 0], nh[:, 0] = trip[:, 2], trip[:, 0]
        nt[:, 3], nh[:, 5] = nt[:, 1], nh[:, 2]                        # duplicate candidates
        samples.append((trip, nt, nh))
        gates.append(tuple(torch.sigmoid(mk(p, 1)) for _ in range(4)))
    # fp64 restatement
    leaves64 = [x.double().requires_grad_(True) for x in (loc, rec, big_loc, big_rec, m.rel_embeds.detach().cpu())]
    g64 = [[w.double().requires_grad_(True) for w in gw] for gw in gates]
    want, off = 0, 0
    for b in range(windows):
        n = sizes[b]
        if Ps[b]:
            want = want + reference_loss64(kind, leaves64[0][off:off + n], leaves64[1][off:off + n], leaves64[4], leaves64[2][b],
                                           leaves64[3][b], *samples[b], *g64[b])
        off += n
    want.backward()
    # the fused node
    dev = lambda t: t.to(device).requires_grad_(True)
    L = [dev(x) for x in (loc, rec, big_loc, big_rec)]
    gdev = [[dev(w) for w in gw] for gw in gates]
    wb = types.SimpleNamespace(target=types.SimpleNamespace(sizes=sizes))
    m.zero_grad()
    sm = [tuple(x.to(device) for x in smp) for smp in samples]
    got = m.batched_gated_loss(wb, list(L[0].split(sizes)), list(L[1].split(sizes)), (L[2], L[3]), sm, gdev)
    assert got is not None
    got.backward()
    assert abs(got.item() - want.item()) <= 3e-6 * abs(want.item()), (got.item(), want.item())
    pairs = [("d_loc", L[0].grad, leaves64[0].grad), ("d_rec", L[1].grad, leaves64[1].grad), ("d_all_loc", L[2].grad, leaves64[2].grad),
             ("d_all_rec", L[3].grad, leaves64[3].grad), ("d_rel", m.rel_embeds.grad, leaves64[4].grad)]
    for b in range(windows):
        if Ps[b]:
            for k, nm in enumerate(("w_sqs", "w_sqo", "w_oqs", "w_oqo")):
                pairs.append(("%s[%d]" % (nm, b), gdev[b][k].grad, g64[b][k].grad))
    for what, a, ref in pairs:
        assert a is not None, what
        assert _frob(a, ref) <= 6e-6, (what, _frob(a, ref))
        if not full_bar:
            assert_close(a, ref, 2e-5, 2e-6 * max(1.0, float(ref.abs().max())), "gated loss " + what)
    # quirk pins: the head rows' known-side weight has no effect (bit-identical loss) and an exactly zero gradient
    for b in range(windows):
        if Ps[b]:
            assert bool((gdev[b][1].grad == 0).all()), "w_sqo gradient"
    g2 = [[w.detach().clone() for w in gw] for gw in gdev]
    for b in range(windows):
        if Ps[b]:
            g2[b][1] = torch.rand_like(g2[b][1])
    with torch.no_grad():
        again = m.batched_gated_loss(wb, list(L[0].split(sizes)), list(L[1].split(sizes)), (L[2], L[3]), sm, g2)
    assert torch.equal(again.detach(), got.detach()), "perturbing w_sqo changed the loss"
    return m


def check_per_window_equals_batched(device, kind="complex"):
    """gated_loss (per-window node, the unbatched path) == the literal reference formula in fp32 and == the batched node."""
    s = slice_snapshots()
    args = make_args(module="GRRGCN", rec_only_last_layer=True, post_aggregation=True, score_function=kind)
    torch.manual_seed(8)
    m = _cls(False)(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(device)
    gen = torch.Generator().manual_seed(5)
    N, D, n, P, C = s["num_e"], 32, 50, 29, 11
    mk = lambda *shape: (torch.randn(*shape, generator=gen) * 0.4).to(device).requires_grad_(True)
    loc, rec, a_loc, a_rec = mk(n, D), mk(n, D), mk(N, D), mk(N, D)
    trip = torch.stack([torch.randint(0, n, (P,), generator=gen), torch.randint(0, 2 * s["num_r"], (P,), generator=gen),
                        torch.randint(0, n, (P,), generator=gen)], dim=1).to(device)
    nt, nh = torch.randint(0, N, (P, C), generator=gen).to(device), torch.randint(0, N, (P, C), generator=gen).to(device)
    ws = [torch.sigmoid(torch.randn(P, 1, generator=gen)).to(device).requires_grad_(True) for _ in range(4)]
    res = []
    for fused in (False, True):
        m.fused_loss = fused
        for x in [loc, rec, a_loc, a_rec] + ws:
            x.grad = None
        m.zero_grad()
        loss = m.gated_loss(loc, rec, a_loc, a_rec, trip, nt, nh, *ws)
        loss.backward()
        res.append([loss.detach()] + [x.grad.detach().clone() for x in [loc, rec, a_loc, a_rec, m.rel_embeds] + ws])
    names = ("loss", "d_loc", "d_rec", "d_all_loc", "d_all_rec", "d_rel", "d_w_sqs", "d_w_sqo", "d_w_oqs", "d_w_oqo")
    for a, b, what in zip(res[0], res[1], names):
        assert_close(b, a, 2e-5, 1e-6, "per-window gated loss: " + what)
