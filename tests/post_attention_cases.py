"""Cases of the post-aggregation attention models (PostSelfAttentionRGCN / PostBiSelfAttentionRGCN, `--module SARGCN / BiSARGCN
--post-aggregation`) and of the split-row history attention, shared by the CPU (test backend) and GPU (HIP) suites: goldens G22
(streams, loss, gradients with the reference's own gates) / G23 (evaluate() ranks), the split all-entity pass against the unsplit
one on the same batch, the scorers' fused nodes, construction and edge windows.  Every function runs under the backend that the
calling suite installed."""
import numpy as np
import pytest
import torch

from oracle import temp_oracle as O
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests.golden_util import T, assert_close, checksum, load
from tests.post_aggregation_cases import MLPS
from tests.window_cases import make_args, slice_snapshots, state_dict_from_oracle, window_inputs


def model_class(bi):
    from temp_amd.post_self_attention_rgcn import PostBiSelfAttentionRGCN, PostSelfAttentionRGCN
    return PostBiSelfAttentionRGCN if bi else PostSelfAttentionRGCN


class Recording:
    """A view of a backend that records (method name, shapes of the tensor arguments) of every call and passes it on."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = []

    def __getattr__(self, name):
        attr = getattr(self._inner, name)                # (AttributeError for what the inner backend lacks: hasattr() sees through)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.calls.append((name, tuple(tuple(x.shape) for x in a if torch.is_tensor(x))))
            return attr(*a, **k)
        return call

    def count(self, name):
        return sum(1 for c in self.calls if c[0] == name)

    def qkv_rows(self, D):
        """Row counts of the forward products with a (3D, D) weight: the Q/K/V projections."""
        return sorted(sh[0][0] for nm, sh in self.calls if nm == "linear" and len(sh) >= 2 and sh[1] == (3 * D, D) and sh[0][1] == D)


class recording:
    """with recording() as rec: ... -- the installed backend wrapped in a Recording for the block."""

    def __enter__(self):
        self.inner = TB.get_backend()
        rec = Recording(self.inner)
        TB.set_backend(rec)
        return rec

    def __exit__(self, *exc):
        TB.set_backend(self.inner)


# ---------------------------------------------------------------------------------------------------------------------
# models from the fixtures
# ---------------------------------------------------------------------------------------------------------------------
def build_model(z, device, **flags):
    """The fixture's model with the reference-shaped state_dict (encoder + the 16 MLP keys) loaded STRICTLY."""
    s = slice_snapshots()
    module, D, B, L, learn = str(z["module"]), int(z["D"]), int(z["B"]), int(z["L"]), bool(z["learn"])
    cfg = dict(module=module, n_bases=B, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=True, learnable_lambda=learn)
    model = O.init_model(cfg, s["num_e"], s["num_r"], len(s["times"]), D, seed=int(z["seed"]))
    if learn:
        for ln in ("layer_1", "layer_2"):
            model["ent_encoder"][ln]["exponential_decay"] = (torch.full((1, 1), 0.25), torch.full((1,), -0.1))
    assert abs(checksum(model) - float(z["param_checksum"])) < 1e-6
    if "rel_scale" in z.files:
        model["rel_embeds"] = model["rel_embeds"] * float(z["rel_scale"])
    kw = dict(module=module, rec_only_last_layer=True, embed_size=D, hidden_size=D, n_bases=B, train_seq_len=L, test_seq_len=L,
              negative_rate=int(z["neg"]), learnable_lambda=learn, EMA=False, post_aggregation=True)
    kw.update(flags)
    m = model_class(module.startswith("Bi"))(make_args(**kw), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    mlp = {k[len("mlp_"):]: T(z[k]) for k in z.files if k.startswith("mlp_")}
    own = m.state_dict()
    assert len(mlp) == 16 and sorted(mlp) == sorted(k for k in own if "_embed_linear." in k)
    assert [k.split(".")[0] for k in own][-16:] == [nm for nm in MLPS for _ in range(4)], "the MLPs are registered last, in the reference's order"
    enc = {k: v for k, v in state_dict_from_oracle(model).items() if k in own}
    left = set(own) - set(enc) - set(mlp)
    assert all("exponential_decay" in k for k in left), left
    sd = dict(own)
    sd.update(enc)
    sd.update(mlp)
    m.load_state_dict(sd, strict=True)
    return m.to(device)


def _prepared(name, device, **flags):
    z = load(name)
    m = build_model(z, device, **flags)
    edge_ids, samples = window_inputs(z)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    wb = m.prepare(t_list, int(z["L"]), True, edge_ids)
    return z, m, wb, samples


def check_gradients(name, z, m, device):
    eg = m.ent_embeds.grad
    rows = T(z["d_ent_nz_rows"]).long().to(device)
    assert_close(eg[rows], z["d_ent_nz_vals"], 1e-4, 3e-6, name + " d_ent")
    assert_close(m.rel_embeds.grad, z["d_rel"], 1e-4, 3e-6, name + " d_rel")
    want_keys = sorted(k[len("gabs_"):] for k in z.files if k.startswith("gabs_"))
    have = dict(m.named_parameters())
    # the same parameters train as in the reference (which also holds an all-zero gradient for what it computes and never uses:
    # layer 1's time embedding)
    assert set(k for k, v in have.items() if v.grad is not None) <= set(want_keys)
    for k in want_keys:
        want = float(z["gabs_" + k])
        got = have[k].grad.double().abs().sum().item() if have[k].grad is not None else 0.0
        assert have[k].grad is not None or want == 0.0, (name, k, want)
        assert abs(got - want) < 3e-4 * max(want, 1e-3), (name, k, got, want)
    for nm in ("subject_query_object_embed_linear", "object_query_object_embed_linear"):
        assert all(p.grad is None for p in getattr(m, nm).parameters()), nm
    assert sum(1 for k in want_keys if "_subject_embed_linear" in k) == 8


def check_g22(name, device):
    """prepare / run / all_embeds_post / run_loss with the model's own gates against G22: gate features equal the recorded rows;
    (loc, rec) target rows and the recorded all_loc / all_rec rows at 1e-5 / 2e-6; loss within 3e-5 relative; d_ent / d_rel at
    (1e-4, 3e-6), gabs_ of every parameter that trains within 3e-4; the *_object_embed_linear MLPs get no gradient."""
    z, m, wb, samples = _prepared(name, device)
    for i, g in enumerate(wb.graphs):
        sub_f, obj_f = m.ensemble_features(samples[i][0], wb.rows[i][-1], g)
        assert torch.equal(sub_f.cpu(), T(z["feat_sub_%d" % i])), (name, i, "subject features")
        assert torch.equal(obj_f.cpu(), T(z["feat_obj_%d" % i])), (name, i, "object features")
    with torch.no_grad():
        (loc, rec), kv2 = m.run(wb)
        all_loc, all_rec = m.all_embeds_post(wb, loc, rec, kv2)
    assert tuple(all_loc.shape) == tuple(all_rec.shape) == (len(wb.graphs), m.num_ents, m.embed_size)
    for i, (lo, re) in enumerate(zip(loc.split(wb.target_sizes), rec.split(wb.target_sizes))):
        assert_close(lo, z["loc_%d" % i], 1e-5, 2e-6, "%s loc %d" % (name, i))
        assert_close(re, z["rec_%d" % i], 1e-5, 2e-6, "%s rec %d" % (name, i))
        rows = T(z["all_rows_%d" % i]).long()
        inactive = ~np.isin(rows.numpy(), wb.graphs[i].gids)
        assert 2 * int(inactive.sum()) >= rows.numel()
        assert_close(all_loc[i][rows.to(device)], z["all_loc_%d" % i], 1e-5, 2e-6, "%s all_loc %d" % (name, i))
        assert_close(all_rec[i][rows.to(device)], z["all_rec_%d" % i], 1e-5, 2e-6, "%s all_rec %d" % (name, i))
        gid = torch.from_numpy(wb.graphs[i].gids).long().to(device)
        assert torch.equal(all_loc[i][gid], lo) and torch.equal(all_rec[i][gid], re), "active rows are the target rows"
    loss = m.run_loss(wb, samples)
    want = float(z["loss"])
    assert abs(loss.item() - want) < 3e-5 * abs(want), (name, loss.item(), want)
    loss.backward()
    check_gradients(name, z, m, device)
    return m


def check_injected_gates(name, device):
    """forward(gate_weights=...) with the gates the MLPs would give, as leaves: the same loss as G22, and the gradient of w_sqo --
    the known object's weight, which the reference applies to two copies of the same row -- is exactly zero."""
    z, m, wb, samples = _prepared(name, device)
    gates = []
    with torch.no_grad():
        for i, g in enumerate(wb.graphs):
            gates.append([w.detach().clone().requires_grad_(True) for w in m.calc_ensemble_ratio(samples[i][0].to(device), wb.rows[i][-1], g)])
    edge_ids, _ = window_inputs(z)
    loss = m(torch.tensor([int(t) for t in z["t_list"]]), target_edge_ids=edge_ids, samples=samples, gate_weights=gates)
    want = float(z["loss"])
    assert abs(loss.item() - want) < 3e-5 * abs(want), (name, loss.item(), want)
    loss.backward()
    for gw in gates:
        assert gw[1].grad is not None and bool((gw[1].grad == 0).all()), "w_sqo gradient"
        assert float(gw[0].grad.abs().sum()) > 0 and float(gw[2].grad.abs().sum()) > 0 and float(gw[3].grad.abs().sum()) > 0
    assert all(p.grad is None for nm in MLPS for p in getattr(m, nm).parameters())


def check_g23(name, device):
    """evaluate() with the model's own gates (PostEvaluationFilter) against the reference's ranks: more than 0.75 of the rows lie
    outside every tie band and match exactly; the others differ by at most their recorded band count."""
    z = load(name)
    m = build_model(z, device)
    t_list = torch.tensor([int(t) for t in z["t_list"]])
    for split, val in (("val", True), ("test", False)):
        ranks, loss = m.evaluate(t_list, val=val)
        assert np.isnan(loss)                                       # no classification loss, as in the reference
        want, nclose = T(z["ranks_" + split]).long(), T(z["nclose_" + split]).long()
        got = ranks.cpu()
        assert got.shape == want.shape
        safe = nclose == 0
        print("%s %s: %.3f of %d ranks outside every tie band" % (name, split, safe.float().mean().item(), want.numel()))
        assert safe.float().mean().item() > 0.75, (name, split)
        assert torch.equal(got[safe], want[safe]), (name, split, int((got[safe] != want[safe]).sum()))
        assert bool(((got - want).abs() <= nclose).all()), (name, split)


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def _step(m, wb, samples):
    m.zero_grad(set_to_none=True)
    loss = m.run_loss(wb, samples)
    loss.backward()
    return loss.detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None}


def compare_steps(what, got, ref):
    """Loss within 2e-5 relative, every gradient with assert_close(1e-4, 1e-5 * max|ref|) (the bars of the gated TransE suite's
    loss properties)."""
    assert abs(got[0].item() - ref[0].item()) <= 2e-5 * abs(ref[0].item()), (what, got[0].item(), ref[0].item())
    assert sorted(got[1]) == sorted(ref[1]), what
    for k, r in ref[1].items():
        assert_close(got[1][k], r, 1e-4, 1e-5 * float(r.abs().max()), "%s %s" % (what, k))


def check_split_route(name, device, **flags):
    """The split all-entity pass against the unsplit one on the same prepared batch: loss and every gradient at compare_steps'
    bars; a split step makes one split forward and one split backward call and its Q/K/V products see the target rows, then
    N_ents + B rows (the unsplit step: B * N_inactive); two split steps are bit-equal (see below for the learnable decay)."""
    z, m, wb, samples = _prepared(name, device, **flags)
    D, N, B = m.embed_size, m.num_ents, len(wb.graphs)
    n_tgt = int(sum(wb.target_sizes))
    assert 0 < wb.n_inactive and N + B < wb.n_inactive
    assert m.split_all_entity
    with recording() as rec:
        split = _step(m, wb, samples)
    assert rec.count("sa_attn_split_fwd") == 1 and rec.count("sa_attn_split_bwd") == 1, rec.calls
    assert rec.count("sa_attn_fwd") == 1 and rec.count("sa_attn_bwd") == 1                      # the target rows
    assert rec.qkv_rows(D) == sorted([n_tgt, N, B]), rec.qkv_rows(D)
    again = _step(m, wb, samples)
    # the step repeats bit for bit -- but for the learnable decay's two scalars: d_decay is T values summed over all rows with
    # atomics, in the split kernel as in the unsplit one (include/temp_amd.h), and nothing else reads it
    assert torch.equal(split[0], again[0]), "split step repeats bit for bit"
    for k in split[1]:
        if "exponential_decay" in k:
            assert_close(again[1][k], split[1][k], 1e-4, 1e-5 * float(split[1][k].abs().max()), "repeat " + k)
        else:
            assert torch.equal(split[1][k], again[1][k]), "split step repeats bit for bit: " + k
    m.split_all_entity = False
    with recording() as rec:
        unsplit = _step(m, wb, samples)
    assert rec.count("sa_attn_split_fwd") == 0 and rec.count("sa_attn_fwd") == 2
    assert rec.qkv_rows(D) == sorted([n_tgt, wb.n_inactive]), rec.qkv_rows(D)
    compare_steps(name + " split vs unsplit", split, unsplit)
    return m


def check_scorer(name, device, kind):
    """Every scorer takes its fused gated node (one batched node for all windows, no per-window node; on a backend with the gated
    kernels: one gated-query launch and one candidate-loss launch); fused_loss = False -- the reference formula per window --
    gives the same loss and gradients at compare_steps' bars."""
    z, m, wb, samples = _prepared(name, device, score_function=kind)
    seen = dict(batched=0, window=0)
    orig_b, orig_w = TF.batched_gated_link_prediction, TF.gated_link_prediction

    def batched(*a, **k):
        seen["batched"] += 1
        return orig_b(*a, **k)

    def window(*a, **k):
        seen["window"] += 1
        return orig_w(*a, **k)
    TF.batched_gated_link_prediction, TF.gated_link_prediction = batched, window
    try:
        with recording() as rec:
            m.zero_grad(set_to_none=True)
            loss = m.run_loss(wb, samples)
        assert seen == dict(batched=1, window=0), (kind, seen)
        inner = rec._inner
        if hasattr(inner, "gated_query_fwd"):
            assert rec.count("gated_query_fwd") == 1, rec.calls
        if kind == "transE":
            assert hasattr(inner, "l1_mix_ce_fwd") and rec.count("l1_mix_ce_fwd") == 1
        elif hasattr(inner, "gather_ce_mix_fwd"):
            assert rec.count("gather_ce_mix_fwd") == 1
        loss.backward()
        fused = (loss.detach().clone(), {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None})
        m.fused_loss = False
        seen.update(batched=0, window=0)
        plain = _step(m, wb, samples)
        assert seen == dict(batched=0, window=0), (kind, seen)
    finally:
        TF.batched_gated_link_prediction, TF.gated_link_prediction = orig_b, orig_w
    compare_steps("%s fused vs formula" % kind, fused, plain)


# ---------------------------------------------------------------------------------------------------------------------
# construction, edge windows
# ---------------------------------------------------------------------------------------------------------------------
def _args(bi, **over):
    kw = dict(module="BiSARGCN" if bi else "SARGCN", rec_only_last_layer=True, post_aggregation=True, EMA=False, train_seq_len=5,
              test_seq_len=5)
    kw.update(over)
    return make_args(**kw)


def fresh_model(device, bi, seed=3, **over):
    s = slice_snapshots()
    torch.manual_seed(seed)
    return model_class(bi)(_args(bi, **over), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"]).to(device)


def check_construction(device):
    s = slice_snapshots()
    for bi in (False, True):
        with pytest.raises(NotImplementedError, match=r"models/SARGCN\.py:143-146"):
            model_class(bi)(_args(bi, rec_only_last_layer=False), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
        with pytest.raises(NotImplementedError, match="EMA"):
            model_class(bi)(_args(bi, EMA=True), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
        with pytest.raises(NotImplementedError, match="post-ensemble"):
            model_class(bi)(_args(bi, post_ensemble=True), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
        a = fresh_model(device, bi, seed=3)
        b = fresh_model(device, bi, seed=4)
        keys = list(a.state_dict())
        assert [k.split(".")[0] for k in keys][-16:] == [nm for nm in MLPS for _ in range(4)]
        b.load_state_dict(a.state_dict(), strict=True)
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    # the plain attention classes still refuse the flag
    from temp_amd.self_attention_rgcn import SelfAttentionRGCN
    with pytest.raises(NotImplementedError, match="PostSelfAttentionRGCN"):
        SelfAttentionRGCN(_args(False), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])


def check_embed_for_non_active_ignored(name, device):
    """--use-embed-for-non-active changes nothing: these classes' get_all_embeds_Gt always takes the isolated pass."""
    res = []
    for flag in (False, True):
        z, m, wb, samples = _prepared(name, device, use_embed_for_non_active=flag)
        res.append(_step(m, wb, samples))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])


def check_edge_windows(device, bi):
    """A window at t = 0 (no history at all: every position masked, in the bidirectional model only the backward half is live)
    beside ordinary ones, one of them without sampled triples: finite loss and gradients, split == unsplit at compare_steps' bars;
    with every window empty the loss is exactly zero; evaluate() ranks all of them."""
    s = slice_snapshots()
    m = fresh_model(device, bi)
    t_list = torch.tensor([0, 7, 3])
    wb = m.prepare(t_list, m.train_seq_len, True)
    assert sorted(r[-1] for r in wb.rows) == [0, 3, 7]
    b0 = [r[-1] for r in wb.rows].index(0)
    if not bi:
        assert all(t is None for t in wb.hist_times[b0])
    gen = torch.Generator().manual_seed(9)
    N, R2, C = s["num_e"], 2 * s["num_r"], 11
    samples = []
    for b, g in enumerate(wb.graphs):
        P = 0 if b == 1 else 23
        trip = torch.stack([torch.randint(0, g.n, (P,), generator=gen), torch.randint(0, R2, (P,), generator=gen),
                            torch.randint(0, g.n, (P,), generator=gen)], dim=1)
        nt, nh = torch.randint(0, N, (P, C), generator=gen), torch.randint(0, N, (P, C), generator=gen)
        if P:
            nt[:, 0], nh[:, 0] = torch.from_numpy(g.gids)[trip[:, 2]], torch.from_numpy(g.gids)[trip[:, 0]]
        samples.append((trip, nt, nh))
    split = _step(m, wb, samples)
    assert bool(torch.isfinite(split[0])) and all(bool(torch.isfinite(v).all()) for v in split[1].values())
    assert float(split[1]["ent_embeds"].abs().sum()) > 0
    m.split_all_entity = False
    compare_steps("edge windows split vs unsplit", split, _step(m, wb, samples))
    m.split_all_entity = True
    # all windows empty: a zero loss that still backpropagates
    empty = [(smp[0][:0], smp[1][:0], smp[2][:0]) for smp in samples]
    loss = m.run_loss(wb, empty)
    assert loss.item() == 0.0
    ranks, _ = m.evaluate(t_list)
    assert ranks.numel() > 0 and int(ranks.min()) >= 1 and int(ranks.max()) <= N
