"""--module RRGCN with BOTH layers recurrent on two linear chains (DynamicRGCN._run_lin_stack) and the pair step of its all-entity pass
(functional.lin_step_rows; temp_lin_rows_fwd / _bwd): cases and checks shared by the CPU (test backend) and GPU (HIP) suites.

The row cases compare the node with a float64 torch restatement at the bars of tests/lin_chain_cases.py (the same product).  The model
cases run the ICEWS14 slice at D = 32, 16 bases, with the inputs of G10_uni_grrgcn (t_list, L, edge choices, samples; its recorded
numbers are the GRU model's and are not read) and parameters from O.init_model, and compare the new route, use_lin_stack = False (the
reference-granular path) and the float64 oracle at check_window_model's bars."""
import contextlib
import math

import numpy as np
import torch

from oracle import temp_oracle as O
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests.chain_route_cases import QUERIES, Launches
from tests.golden_util import assert_close, load
from tests.lin_chain_cases import GRAD_BAR, LAM, STATE_BAR, WIDTHS, ratio  # noqa: F401  (WIDTHS: the suites parametrise over it)

GOLDEN = "G10_uni_grrgcn"
ROW_NS = (1, 33, 70)             # one row; one full panel + 1; two full panels + 6
H_ROWS = 50
X_ROWS = 40
TIE_BAND = 1.5e-6                # oracle/gen_golden.py: G13_BAND, on sigmoid scores
REL_SCALE = 250.0                # ... and G13_REL_SCALE: the untrained model's scores spread instead of tying at sigmoid = 0.5
MAX_BAND_SHARE = 0.25            # share of ranked rows that may have a competitor inside the tie band


# ---- the pair step ----------------------------------------------------------------------------------------------------------
def rows_inputs(n, d, with_x_rows, seed=23):
    """x, H (50 rows), W, h_rows (about a quarter -1, rows repeated), x_rows (None, or an index with repeats), dt in 0 .. 14, and the
    upstream gradient of `out`."""
    g = torch.Generator().manual_seed(seed + 7 * n + d)
    n_x = X_ROWS if with_x_rows else n
    x, H = torch.randn(n_x, d, generator=g) * 0.5, torch.randn(H_ROWS, d, generator=g) * 0.5
    W = torch.randn(d, d, generator=g) / math.sqrt(d)
    h_rows = torch.randint(0, H_ROWS, (n,), generator=g)
    h_rows[torch.rand(n, generator=g) < 0.25] = -1
    h_rows[0] = 7                                    # (n = 1: the one row has a previous state)
    if n > 2:
        h_rows[1], h_rows[2] = -1, 7                 # a row without one, and a repeat, whatever the draw
    x_rows = torch.randint(0, n_x, (n,), generator=g) if with_x_rows else None
    if with_x_rows and n > 2:
        x_rows[2] = x_rows[0]
    dt = torch.randint(0, 15, (n,), generator=g).float()
    up = torch.randn(n, d, generator=g)
    return dict(x=x, H=H, W=W, h_rows=h_rows.int(), x_rows=None if x_rows is None else x_rows.int(), dt=dt, up=up)


@contextlib.contextmanager
def rows_kernel(on):
    old, TF.LIN_ROWS_KERNEL = TF.LIN_ROWS_KERNEL, on
    try:
        yield
    finally:
        TF.LIN_ROWS_KERNEL = old


def run_rows_node(c, act, device, kernel=True):
    """lin_step_rows forward + backward under the upstream gradient c["up"] -> dict(out, d_x, d_H, d_W) on the CPU."""
    x, H, W = (c[k].clone().to(device).requires_grad_(True) for k in ("x", "H", "W"))
    h_rows, dt = c["h_rows"].to(device), c["dt"].to(device)
    x_rows = c["x_rows"].to(device) if c["x_rows"] is not None else None
    h_inv = TF.gather_inverse(c["h_rows"].numpy(), H_ROWS, device)
    x_inv = TF.gather_inverse(c["x_rows"].numpy(), c["x"].shape[0], device) if x_rows is not None else None
    with rows_kernel(kernel):
        out = TF.lin_step_rows(x, x_rows, H, h_rows, dt.view(-1, 1), LAM, W, act, x_inv, h_inv)
    (out * c["up"].to(device)).sum().backward()
    return dict(out=out.detach().cpu(), d_x=x.grad.cpu(), d_H=H.grad.cpu(), d_W=W.grad.cpu())


def rows_reference(c, act, mask=None):
    """float64 restatement: the decay in front of the product.  mask (n, d) bool: the ReLU mask of the code under test (its own
    out > 0), so that an element within rounding of 0 cannot flip a gradient; None = the reference's own."""
    x, H, W = (c[k].double().clone().requires_grad_(True) for k in ("x", "H", "W"))
    hr = c["h_rows"].long()
    hdec = H[hr.clamp(min=0)] * (hr >= 0).double().view(-1, 1) * torch.exp(-LAM * c["dt"].double()).view(-1, 1)
    pre = (x[c["x_rows"].long()] if c["x_rows"] is not None else x) + hdec @ W
    out = pre if not act else (pre * mask.double() if mask is not None else torch.relu(pre))
    (out * c["up"].double()).sum().backward()
    return dict(out=out.detach(), hdec=hdec.detach(), d_x=x.grad, d_H=H.grad, d_W=W.grad)


def check_quantities(res, ref, what, names=("out", "d_x", "d_H", "d_W")):
    """Every named quantity inside its bar (STATE_BAR for out / hdec, GRAD_BAR for the gradients); max err / bar printed first."""
    figs = []
    for name in names:
        bar = STATE_BAR if name in ("out", "hdec") else GRAD_BAR
        r, atol = ratio(res[name], ref[name], bar)
        print("%s: %s max err / bar %.3g (max |ref| %.3g)" % (what, name, r, float(ref[name].abs().max())))
        figs.append((name, bar[0], atol, r))
    for name, rtol, atol, _ in figs:
        assert_close(res[name], ref[name], rtol, atol, what + " " + name)
    return {f[0]: f[-1] for f in figs}


def check_rows_node(n, d, act, device, kernel=True):
    """One (rows, width, activation) case of the node against the float64 restatement, with and without x_rows."""
    out = {}
    for with_x_rows in (False, True):
        c = rows_inputs(n, d, with_x_rows)
        res = run_rows_node(c, act, device, kernel)
        ref = rows_reference(c, act, res["out"] > 0 if act else None)
        what = "n = %d d = %d act = %d x_rows = %s%s" % (n, d, act, "index" if with_x_rows else "None", "" if kernel else " (composition)")
        out[with_x_rows] = check_quantities(res, ref, what)
    return out


# ---- the window model ---------------------------------------------------------------------------------------------------------
def stack_model(device, lin_stack=True, dropout=0.0, learnable_lambda=False, rec_only=False, module="RRGCN"):
    """-> (model, oracle parameters, cfg, golden inputs): --module RRGCN (or BiRRGCN) on the ICEWS14 slice, D = 32, 16 bases."""
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    from temp_amd.dynamic_rgcn import DynamicRGCN
    from tests.window_cases import make_args, slice_snapshots, state_dict_from_oracle
    s, z = slice_snapshots(), load(GOLDEN)
    cfg = dict(module=module, n_bases=16, inv_temperature=0.1, rec_only_last_layer=rec_only, use_time_embedding=False)
    model = O.init_model(cfg, s["num_e"], s["num_r"], len(s["times"]), 32, seed=3)
    args = make_args(module=module, rec_only_last_layer=rec_only, negative_rate=int(z["neg"]), train_seq_len=int(z["L"]), test_seq_len=int(z["L"]),
                     dropout=dropout, learnable_lambda=learnable_lambda)
    m = (BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN)(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    missing = m.load_state_dict(state_dict_from_oracle(model), strict=False)
    assert not missing.unexpected_keys and all("exponential_decay" in k for k in missing.missing_keys) and bool(missing.missing_keys) == learnable_lambda
    m.use_lin_stack = lin_stack
    return m.to(device), model, cfg, z


def golden_inputs(z):
    from tests.window_cases import window_inputs
    edge_ids, samples = window_inputs(z)
    return torch.tensor([int(t) for t in z["t_list"]]), int(z["L"]), edge_ids, samples


TIME_WEIGHTS = ["ent_encoder.layer_1.time_weight", "ent_encoder.layer_2.time_weight"]


def check_stack_model(device):
    """The new route against use_lin_stack = False and the float64 oracle: flags, loss, every gradient, encode(train=False)."""
    from tests.golden_util import slice_graphs
    from tests.window_cases import state_dict_from_oracle
    res, enc = {}, {}
    for key, stack in (("stack", True), ("generic", False)):
        m, model, cfg, z = stack_model(device, stack)
        t_list, L, edge_ids, samples = golden_inputs(z)
        assert not m.ent_encoder.rec_only_last_layer and m._can_batch() == stack
        wb = m.prepare(t_list, L, True, edge_ids)
        assert wb.batched == stack and (wb.program is not None) == stack and bool(m._fused_all_entity_ok(wb)) == stack
        loss = m.run_loss(wb, samples)
        loss.backward()
        res[key] = (loss.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters() if v.grad is not None})
        with torch.no_grad():
            enc[key] = [e.cpu() for e in m.encode(t_list, L, False)[0]]
    (l1, g1), (l0, g0) = res["stack"], res["generic"]
    print("RRGCN both layers: loss stack %.8f generic %.8f" % (l1.item(), l0.item()))
    assert abs(l0.item() - l1.item()) < 2e-5 * abs(l0.item()), (l0.item(), l1.item())
    assert set(g0) == set(g1) and len(g0) >= 8, sorted(g1)
    worst = 0.0
    for k in g0:
        atol = 3e-6 * max(1.0, float(g0[k].abs().max()))
        worst = max(worst, float(((g1[k] - g0[k]).abs() / (atol + 1e-4 * g0[k].abs())).max()))
        assert_close(g1[k], g0[k], 1e-4, atol, "stack vs generic: d_" + k)
    print("RRGCN both layers: gradients stack vs generic, max err / bar %.3g" % worst)
    for a, b in zip(enc["stack"], enc["generic"]):
        assert_close(a, b, 1e-5, 2e-6, "encode(train=False) stack vs generic")
    for k in TIME_WEIGHTS:
        assert float(g1[k].abs().max()) > 0, k

    _, _, times, gd = slice_graphs()
    tl = [int(t) for t in z["t_list"]]
    assert tl == sorted(tl, reverse=True)
    targets = [O.edge_subgraph(gd["train"][t], z["choice_%d" % i]) for i, t in enumerate(tl)]
    m64 = O.map_params(model, lambda t: t.double().clone().requires_grad_(True))
    assert cfg["rec_only_last_layer"] is False
    ref, _ = O.uni_forward_loss(m64, cfg, gd["train"], tl, times, int(z["L"]), targets, samples)
    ref.backward()
    print("RRGCN both layers: loss float64 oracle %.8f (stack: %.3g relative)" % (ref.item(), abs(ref.item() - l1.item()) / abs(ref.item())))
    assert abs(ref.item() - l1.item()) < 2e-5 * abs(ref.item()), (ref.item(), l1.item())
    g64 = {k: v.grad for k, v in state_dict_from_oracle(m64).items() if v.grad is not None}
    checked, worst = 0, 0.0
    for k, r in g64.items():
        if k in g1:
            atol = 3e-6 * max(1.0, float(r.abs().max()))
            worst = max(worst, float(((g1[k].double() - r).abs() / (atol + 1e-4 * r.abs())).max()))
            assert_close(g1[k], r.float(), 1e-4, atol, "d_%s vs float64 oracle" % k)
            checked += 1
    print("RRGCN both layers: gradients stack vs float64 oracle, max err / bar %.3g" % worst)
    assert checked >= 8 and all(k in g64 for k in TIME_WEIGHTS), sorted(g64)


class _BandBackend:
    """The installed backend with filtered_rank also noting, per ranked row, how many unfiltered competitors have a sigmoid score within
    TIE_BAND of the target's (oracle/gen_golden.py: gen_G13's `nclose`): two valid fp32 evaluation orders may swap such a pair."""

    def __init__(self, inner):
        self._inner, self.nclose = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def filtered_rank(self, score, target, filt_ptr=None, filt_ids=None):
        s = score.detach().double().clone()
        P, tgt = s.shape[0], target.long()
        if filt_ptr is not None and filt_ids is not None and filt_ids.numel():
            ptr, fid = filt_ptr.long(), filt_ids.long()
            rows = torch.repeat_interleave(torch.arange(P, device=s.device), ptr[1:] - ptr[:-1])
            keep = fid != tgt[rows]
            s[rows[keep], fid[keep]] = -10e6
        sig = torch.sigmoid(s)
        dd = (sig - sig.gather(1, tgt.view(-1, 1))).abs()
        dd.scatter_(1, tgt.view(-1, 1), float("inf"))
        self.nclose.append(((dd <= TIE_BAND) & (sig > 1e-30)).sum(1).cpu())
        return self._inner.filtered_rank(score, target, filt_ptr, filt_ids)


def evaluate_ranks(device, lin_stack):
    """evaluate() on the validation graphs of the golden's timestamps, relation rows scaled as in G13 -> (ranks, nclose per row)."""
    m, _, _, z = stack_model(device, lin_stack)
    with torch.no_grad():
        m.rel_embeds.mul_(REL_SCALE)
    t_list = golden_inputs(z)[0]
    inner = TB.get_backend()
    rec = _BandBackend(inner)
    TB.set_backend(rec)
    try:
        ranks, loss = m.evaluate(t_list, val=True)
    finally:
        TB.set_backend(inner)
    assert np.isfinite(loss)
    return ranks.cpu(), torch.cat(rec.nclose)


def check_evaluate(device):
    """evaluate() ranks of the two routes: equal on every row without a competitor inside the tie band, within the band population
    elsewhere; at most MAX_BAND_SHARE of the rows have such a competitor (on the generic route alone, too)."""
    r1, n1 = evaluate_ranks(device, True)
    r0, n0 = evaluate_ranks(device, False)
    assert r0.shape == r1.shape == n0.shape == n1.shape and r0.numel() > 50
    band = torch.maximum(n0, n1)
    print("evaluate: %d ranks, %.3f with a competitor inside the tie band (generic alone %.3f), %d differ" %
          (r0.numel(), (band > 0).float().mean().item(), (n0 > 0).float().mean().item(), int((r0 != r1).sum())))
    assert (n0 > 0).float().mean().item() <= MAX_BAND_SHARE and (band > 0).float().mean().item() <= MAX_BAND_SHARE
    safe = band == 0
    assert torch.equal(r1[safe], r0[safe]), int((r1[safe] != r0[safe]).sum())
    assert bool(((r1 - r0).abs() <= band).all())


def check_dropout(device):
    """While the self-loop dropout draws (the reference's default) the route is taken, with per-visit masks and one row per (window,
    entity) in the all-entity pass: two windows' inactive rows of one entity differ."""
    m, _, _, z = stack_model(device, True, dropout=0.1)
    m.train()
    t_list, L, edge_ids, _ = golden_inputs(z)
    wb = m.prepare(t_list, L, True, edge_ids)
    assert wb.batched and wb.lin_stack and wb.program is not None and wb.visit_rows is None and m._fused_all_entity_ok(wb)
    torch.manual_seed(5)
    out, hist = m.run(wb)
    big = m.all_embeds_batched(wb, out, hist)
    assert wb.all_rep and big.shape[:2] == (len(wb.graphs), m.num_ents) and bool(torch.isfinite(big).all())
    act = np.zeros((len(wb.graphs), m.num_ents), dtype=bool)
    for b, g in enumerate(wb.graphs):
        act[b, g.gids] = True
    both = np.nonzero(~act[0] & ~act[1])[0]
    assert both.size > 10
    rows = torch.from_numpy(both).to(big.device)
    assert float((big[0][rows] != big[1][rows]).float().mean()) > 0.05, "two windows' inactive rows of one entity share a dropout mask"
    big.sum().backward()
    for layer in (m.ent_encoder.layer_1, m.ent_encoder.layer_2):
        assert float(layer.time_weight.grad.abs().max()) > 0


def check_learnable_lambda(device):
    """--learnable-lambda: the linear layers never read the learned decay, so the model takes the chain routes and computes the
    bit-same loss; exponential_decay stays in the state dict and gets no gradient."""
    for rec_only in (False, True):
        losses = []
        for learn in (False, True):
            m, _, _, z = stack_model(device, True, learnable_lambda=learn, rec_only=rec_only)
            t_list, L, edge_ids, samples = golden_inputs(z)
            assert m._can_batch() and m._can_chain()
            wb = m.prepare(t_list, L, True, edge_ids)
            assert wb.batched and wb.program is not None and wb.lin_stack == (not rec_only)
            loss = m.run_loss(wb, samples)
            loss.backward()
            losses.append(loss.detach().cpu())
            decay = [(k, p) for k, p in m.named_parameters() if "exponential_decay" in k]
            assert len(decay) == (4 if learn else 0), [k for k, _ in decay]         # (weight and bias of both layers' nn.Linear(1, 1))
            assert all(p.grad is None for _, p in decay)
            assert all(k in m.state_dict() for k, _ in decay)
        assert torch.equal(losses[0], losses[1]), (rec_only, losses)


def check_bi_unchanged(device):
    """--module BiRRGCN with both layers recurrent keeps the reference-granular path."""
    m, _, _, z = stack_model(device, True, module="BiRRGCN")
    assert not m._can_batch()
    t_list, L, edge_ids, _ = golden_inputs(z)
    wb = m.prepare(t_list, L, True, edge_ids)
    assert not wb.batched and wb.program is None


def step_calls(device, lin_stack=True):
    """Names of the backend launches of one run_loss + backward (queries left out) -> (names, L, B)."""
    m, _, _, z = stack_model(device, lin_stack)
    t_list, L, edge_ids, samples = golden_inputs(z)
    wb = m.prepare(t_list, L, True, edge_ids)
    inner = TB.get_backend()
    rec = Launches(inner)
    TB.set_backend(rec)
    try:
        m.run_loss(wb, samples).backward()
    finally:
        TB.set_backend(inner)
    return [c[0] for c in rec.calls if not c[0].endswith(QUERIES)], L, len(wb.graphs)
