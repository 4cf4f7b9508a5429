"""--learnable-lambda windows on the persistent chain kernels: the previous state decays by exp(-max(w dt + b, 0)) with {w, b} read
from device memory (temp_gru_chain_*_decay), the backward also writes dL / d(w dt + b) per row and a fixed-order reduction turns
it into (d_w, d_b).

Kernels against a float64 autograd loop over the program's instances (written here), identities against the fixed-decay chain,
bit-repeatability, the fixed-decay path untouched, and the window models against their per-position path.

Measured on the MI355X against the float64 loop, want = None (absolute errors; d_w / d_b beside the absolute sum of their per-row terms):
  d = 200 nn.GRU   states 2.1e-07  d_x 6.5e-06  parameters 7.4e-05 (max |ref| 4.5e+02)  d_arg 5.7e-06 (max |ref| 25)  d_w 2.5e-05 of 1.3e+03  d_b 1.5e-05 of 4.0e+02
  d = 32  nn.GRU   states 1.3e-07  d_x 2.1e-06  parameters 1.9e-04 (max |ref| 1.4e+03)  d_arg 1.9e-06 (max |ref| 12)  d_w 2.3e-05 of 1.7e+03  d_b 3.6e-06 of 4.9e+02
  d = 16  type-1   states 6.8e-07  d_x 3.3e-05  parameters 4.4e-05 (max |ref| 3.7e+02)  d_arg 2.3e-05 (max |ref| 42)  d_w 7.6e-05 of 1.8e+03  d_b 1.9e-05 of 5.2e+02
Every case prints its figures before it asserts (pytest -s).
"""
import numpy as np
import pytest
import torch

from oracle import temp_oracle as O
from temp_amd import _lib
from temp_amd import gru_chain as GC
from temp_amd.backend import get_backend
from tests.chain_cases import make_rnns, random_program
from tests.golden_util import assert_close, load
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
WB = (0.3, -0.7)             # dt in {1, 2, 3, 4} -> w dt + b in {-0.4, -0.1, 0.2, 0.5}: two clamped, two active, none 0
SHAPES = [(200, False, dict(n_chain=2, K=6, E=90, lo=20, hi=70)),       # f16 route, fused forward, two GRUs sharing the decay
          (32, False, dict(n_chain=2, K=5, E=200, lo=50, hi=200)),      # several panels per chain
          (16, True, dict(n_chain=2, K=6, E=90, lo=20, hi=70)),         # type-1 cell
          (248, False, dict(n_chain=1, K=3, E=50, lo=10, hi=50)),       # past the chain kernels' widest d (224: LDS): gru_chain refuses the decay
          (216, False, dict(n_chain=1, K=3, E=50, lo=10, hi=50)),       # partial last tiles; past the f16 kernels: the bf16 chain kernels
          (220, False, dict(n_chain=2, K=4, E=70, lo=10, hi=70))]       # partial last tiles, d % 8 != 0: the fp32 chain kernels


def _launches():
    return _lib.load().temp_gru_chain_decay_launches()


def _params(m, type1):
    return [m.weight_ih, m.weight_hh, m.bias_ih, m.bias_hh] if type1 else [m.weight_ih_l0, m.weight_hh_l0, m.bias_ih_l0, m.bias_hh_l0]


def _x(n, d, seed=17):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * 0.5


def _want(prog, want):
    return None if want is None else tuple(i for i, it in enumerate(prog.inst) if it.next < 0 or i % 3 == 1)[:8]


def _out_insts(prog, want):
    return list(range(len(prog.inst))) if want is None else list(want)


def loss_weights(prog, want, d, seed=17):
    """One random weight matrix per handed-out instance (shared by every run that is compared)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(prog.inst[i].n, d, generator=g) * (k + 1) for k, i in enumerate(_out_insts(prog, want))]


def has_prev_rows(prog):
    """bool [n_total]: the rows that carry a previous state (the only rows with a decay)."""
    m = np.zeros(prog.n_total, dtype=bool)
    for it in prog.inst:
        if it.prev >= 0 and it.n:
            m[it.h0:it.h0 + it.n] = np.asarray(it.prev_idx) >= 0
    return m


def row_dt(prog):
    dt = np.zeros(prog.n_total, dtype=np.float64)
    for it in prog.inst:
        dt[it.h0:it.h0 + it.n] = np.asarray(it.dt, dtype=np.float64).reshape(-1)
    return dt


def loop_reference(prog, x, rnns, wb, type1, want, weights, lam=0.1):
    """float64 autograd over the per-position loop: instance by instance, previous rows through prev_idx, O.decay_hidden and
    O.gru_torch / O.gru_type1.  wb = (w, b): the decay argument w dt + b enters as a per-row LEAF (decay_hidden applies its own
    Linear to it with weight 1, bias 0), so the loop also yields dL / d arg per row; wb = None: the fixed decay exp(-dt lam).
    -> dict(outs, d_x, grads, d_arg [n_total], d_w, d_b, terms_w, terms_b (the absolute sums of the per-row terms))."""
    x64 = x.detach().double().clone().requires_grad_(True)
    P = [[p.detach().cpu().double().clone().requires_grad_(True) for p in _params(m, type1)] for m in rnns]
    d = x.shape[1]
    one, zero = torch.ones(1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    cell = O.gru_type1 if type1 else O.gru_torch
    H, args = [], []
    for it in prog.inst:
        dt = torch.from_numpy(np.asarray(it.dt, dtype=np.float64)).view(-1, 1)
        prev = torch.zeros(it.n, d, dtype=torch.float64)
        if it.prev >= 0 and prog.inst[it.prev].n > 0 and it.n > 0:
            pi = torch.from_numpy(np.asarray(it.prev_idx, dtype=np.int64))
            prev = H[it.prev][pi.clamp(min=0)] * (pi >= 0).double().view(-1, 1)
        if wb is not None:
            arg = (wb[0] * dt + wb[1]).requires_grad_(True)
            args.append(arg)
            hd = O.decay_hidden(prev, arg, lam, learnable=(one, zero))
        else:
            hd = O.decay_hidden(prev, dt, lam)
        H.append(cell(x64[it.x0:it.x0 + it.n], hd, *P[it.rnn]))
    loss = sum((H[i] * wgt.double()).sum() for i, wgt in zip(_out_insts(prog, want), weights))
    loss.backward()
    res = dict(outs=[H[i].detach() for i in _out_insts(prog, want)], d_x=x64.grad, grads=[p.grad if p.grad is not None else torch.zeros_like(p) for ps in P for p in ps])
    if wb is not None:
        d_arg = torch.cat([a.grad.view(-1) if a.grad is not None else torch.zeros(a.numel(), dtype=torch.float64) for a in args])
        dt_all = torch.from_numpy(row_dt(prog))
        keep = torch.from_numpy(has_prev_rows(prog))
        assert float(d_arg[~keep].abs().max() if (~keep).any() else 0.0) == 0.0      # rows without a previous state have no decay
        res.update(d_arg=d_arg, d_w=(d_arg * dt_all).sum(), d_b=d_arg.sum(), terms_w=(d_arg * dt_all).abs().sum(), terms_b=d_arg.abs().sum())
    return res


def run_chain(prog, x, rnns, device, type1, want, weights, decay=None, lam=0.1):
    """gru_chain on `device` -> dict(outs, d_x, grads, d_w, d_b, d_arg): d_arg is the per-row vector the chain backward hands to the
    reduction (read off the backend call), None for a fixed decay."""
    leaf = x.detach().clone().to(device).requires_grad_(True)
    mods = [m.to(device) for m in rnns]
    for m in mods:
        m.zero_grad()
    spec = None
    if decay is not None:
        spec = (torch.tensor([[decay[0]]], dtype=torch.float32, device=device).requires_grad_(True),
                torch.tensor([decay[1]], dtype=torch.float32, device=device).requires_grad_(True))
    be = get_backend()
    seen = []
    orig = getattr(be, "gru_chain_decay_reduce", None)
    if orig is not None:
        def spy(tabs, d, variant, d_arg, n_rnn):
            seen.append(d_arg.detach().cpu().clone())
            return orig(tabs, d, variant, d_arg, n_rnn)
        be.gru_chain_decay_reduce = spy
    try:
        out = GC.gru_chain(leaf, prog, mods, lam, type1, want, decay=spec)
        outs = [out[it.h0:it.h0 + it.n] for it in prog.inst] if want is None else list(out)
        loss = sum((o * wgt.to(device)).sum() for o, wgt in zip(outs, weights))
        loss.backward()
    finally:
        if orig is not None:
            del be.gru_chain_decay_reduce
    res = dict(outs=[o.detach().cpu() for o in outs], d_x=leaf.grad.detach().cpu(),
               grads=[p.grad.detach().cpu().clone() for m in mods for p in _params(m, type1)], d_arg=None, d_w=None, d_b=None)
    if spec is not None:
        assert len(seen) == 1
        assert spec[0].grad.shape == (1, 1) and spec[1].grad.shape == (1,)
        res.update(d_arg=seen[0], d_w=spec[0].grad.detach().cpu().view(()), d_b=spec[1].grad.detach().cpu().view(()))
    return res


def _err(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def check_states_and_grads(got, ref, type1, name):
    """The bars of test_chain_kernels_vs_reference_and_per_position_path."""
    rt, at = (1e-4, 2e-5) if type1 else (1e-5, 2e-6)
    print("%s: states %.2e  d_x %.2e  parameters %.2e (max |ref| %.2e)" % (
        name, max([_err(u, v) for u, v in zip(got["outs"], ref["outs"])] + [0.0]), _err(got["d_x"], ref["d_x"]),
        max(_err(u, v) for u, v in zip(got["grads"], ref["grads"])), max(float(v.abs().max()) for v in ref["grads"])))
    for u, v in zip(got["outs"], ref["outs"]):
        assert_close(u, v.float(), rt, at, "states vs " + name)
    assert_close(got["d_x"], ref["d_x"].float(), 1e-4, 2e-5 * max(1.0, float(ref["d_x"].abs().max())), "d_x vs " + name)
    for u, v in zip(got["grads"], ref["grads"]):
        assert_close(u, v.float(), 1e-4, 2e-5 * max(1.0, float(v.abs().max())), "GRU parameter gradient vs " + name)


def check_decay_grads(got, ref, prog, name):
    keep = torch.from_numpy(has_prev_rows(prog))
    print("%s: d_arg %.2e (max |ref| %.2e)  d_w %.2e of %.2e  d_b %.2e of %.2e" % (
        name, _err(got["d_arg"][keep], ref["d_arg"][keep]), float(ref["d_arg"].abs().max()), abs(float(got["d_w"]) - float(ref["d_w"])),
        float(ref["terms_w"]), abs(float(got["d_b"]) - float(ref["d_b"])), float(ref["terms_b"])))
    assert_close(got["d_arg"][keep], ref["d_arg"][keep].float(), 1e-4, 2e-5 * max(1.0, float(ref["d_arg"].abs().max())), "per-row d_arg vs " + name)
    # sums with cancellation: the error is that of the per-row terms, so the scale is their absolute sum
    for k, t in (("d_w", "terms_w"), ("d_b", "terms_b")):
        g, r = float(got[k]), float(ref[k])
        assert abs(g - r) <= 1e-4 * abs(r) + 2e-5 * float(ref[t]), (name, k, g, r, float(ref[t]))


@pytest.mark.parametrize("d,type1,kw", SHAPES)
@pytest.mark.parametrize("want", [None, "some"])
def test_chain_kernels_vs_float64_loop(d, type1, kw, want):
    prog, n_x = random_program(d + 1, **kw)
    hp = has_prev_rows(prog)
    arg = WB[0] * row_dt(prog)[hp] + WB[1]
    assert (arg > 0).any() and (arg < 0).any() and not (arg == 0).any()
    w = _want(prog, want)
    rnns = make_rnns(kw["n_chain"], d, type1, 5)
    x = _x(n_x, d)
    wts = loss_weights(prog, w, d)
    c0 = _launches()
    if d == 248:
        # The existing chain test runs this width through the per-position cell kernels (temp_gru_chain_supported(248) == 0), which
        # have no learnable decay: gru_chain must say so instead of running a fixed decay.  (The models never get here: prepare
        # keeps such a program on the run_rnn loop.)
        assert not get_backend().gru_chain_supported(d) and not GC.chain_decay_usable(d, _lib.GRU_TORCH, 1)
        with pytest.raises(_lib.TempAmdError, match="learnable decay"):
            run_chain(prog, x, rnns, DEV, type1, w, wts, decay=WB)
        assert _launches() == c0
        return
    ref = loop_reference(prog, x, rnns, WB, type1, w, wts)
    got = run_chain(prog, x, rnns, DEV, type1, w, wts, decay=WB)
    assert _launches() - c0 == 2                      # one forward, one backward launch carried the decay
    name = "float64 loop (d = %d%s%s)" % (d, ", type-1" if type1 else "", ", want" if w is not None else "")
    check_states_and_grads(got, ref, type1, name)
    check_decay_grads(got, ref, prog, name)


def _d200():
    prog, n_x = random_program(201, **SHAPES[0][2])
    return prog, make_rnns(2, 200, False, 5), _x(n_x, 200), loss_weights(prog, None, 200)


def _bit_equal(a, b, keys=("d_w", "d_b")):
    for u, v in zip(a["outs"] + [a["d_x"]] + a["grads"], b["outs"] + [b["d_x"]] + b["grads"]):
        assert torch.equal(u, v)
    for k in keys:
        assert torch.equal(a[k], b[k])


def test_all_rows_clamped_is_the_fixed_chain_without_decay():
    """(w, b) = (-0.25, -0.1): w dt + b < 0 on every row, both decay tables hold exactly 1.0 -- bit-identical to the fixed chain at
    lambda = 0, and the decay has no gradient."""
    prog, rnns, x, wts = _d200()
    a = run_chain(prog, x, rnns, DEV, False, None, wts, decay=(-0.25, -0.1))
    b = run_chain(prog, x, rnns, DEV, False, None, wts, lam=0.0)
    _bit_equal(a, b, keys=())
    assert float(a["d_w"]) == 0.0 and float(a["d_b"]) == 0.0
    keep = torch.from_numpy(has_prev_rows(prog))
    assert bool((a["d_arg"][keep] == 0).all())


def test_linear_decay_matches_the_fixed_chain():
    """(w, b) = (0.1, 0): exp(-max(0.1 dt, 0)) = exp(-dt 0.1), the fixed chain at lambda = 0.1."""
    prog, rnns, x, wts = _d200()
    a = run_chain(prog, x, rnns, DEV, False, None, wts, decay=(0.1, 0.0))
    b = run_chain(prog, x, rnns, DEV, False, None, wts, lam=0.1)
    check_states_and_grads(a, dict(outs=[o.double() for o in b["outs"]], d_x=b["d_x"].double(), grads=[g.double() for g in b["grads"]]), False,
                           "fixed chain at lambda = 0.1")


def test_bit_repeatable():
    prog, rnns, x, wts = _d200()
    a = run_chain(prog, x, rnns, DEV, False, None, wts, decay=WB)
    b = run_chain(prog, x, rnns, DEV, False, None, wts, decay=WB)
    _bit_equal(a, b)
    keep = torch.from_numpy(has_prev_rows(prog))
    assert torch.equal(a["d_arg"][keep], b["d_arg"][keep])


def test_fixed_decay_untouched_by_a_learnable_run():
    prog, rnns, x, wts = _d200()
    c0 = _launches()
    before = run_chain(prog, x, rnns, DEV, False, None, wts)
    assert _launches() == c0
    run_chain(prog, x, rnns, DEV, False, None, wts, decay=WB)
    c1 = _launches()
    assert c1 > c0
    after = run_chain(prog, x, rnns, DEV, False, None, wts)
    assert _launches() == c1
    _bit_equal(before, after, keys=())


# ---- window models ----------------------------------------------------------------------------------------------------
DECAY = (0.25, -0.6)         # clamped at dt <= 2, active from 3, never 0
# Inside the encoder's chain a state survives exactly one position, so every row that carries one has dt = 1 (the larger gaps of a
# window belong to rows that start from zero, and to the all-entity pass): DECAY leaves the chain's own decay clamped on all its rows.
# The second pair is active at dt = 1 (0.15), and never 0 either: the chain's decay gradient is not zero there.
DECAY_ACTIVE = (0.25, -0.1)


def _window_model(module, golden, chain, decay=DECAY):
    from tests.window_cases import make_args, slice_snapshots, state_dict_from_oracle
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    from temp_amd.dynamic_rgcn import DynamicRGCN
    s, z = slice_snapshots(), load(golden)
    cfg = dict(module=module, n_bases=16, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=False, learnable_lambda=True)
    model = O.init_model(cfg, s["num_e"], s["num_r"], len(s["times"]), 32, seed=3)
    for ln in ("layer_1", "layer_2"):
        model["ent_encoder"][ln]["exponential_decay"] = (torch.tensor([[decay[0]]]), torch.tensor([decay[1]]))
    args = make_args(module=module, rec_only_last_layer=True, learnable_lambda=True, negative_rate=int(z["neg"]))
    m = (BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN)(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    m.load_state_dict(state_dict_from_oracle(model), strict=True)
    m.use_gru_chain = chain
    return m.to(DEV), model, cfg, z


@pytest.mark.parametrize("decay", [DECAY, DECAY_ACTIVE])
@pytest.mark.parametrize("module,golden", [("GRRGCN", "G10_uni_grrgcn_rol"), ("BiGRRGCN", "G10_bi_grrgcn_rol")])
def test_window_models_chain_vs_per_position_path(module, golden, decay):
    from tests.window_cases import slice_snapshots, window_inputs
    res, enc = [], []
    for chain in (True, False):
        m, model, cfg, z = _window_model(module, golden, chain, decay)
        edge_ids, samples = window_inputs(z)
        t_list = torch.tensor([int(t) for t in z["t_list"]])
        assert m._can_batch() and m._can_chain() == chain
        c0 = _launches()
        wb = m.prepare(t_list, 8, True, edge_ids)
        assert (wb.program is not None) == chain
        if chain:
            gaps = np.concatenate([np.asarray(it.dt).reshape(-1) for it in wb.program.inst]).astype(np.float64)        # the window's gaps
            arg = decay[0] * gaps + decay[1]
            assert (arg > 0).any() and not (arg == 0).any() and ((arg < 0).any() or decay is DECAY_ACTIVE)
            carried = decay[0] * row_dt(wb.program)[has_prev_rows(wb.program)] + decay[1]                               # ... and those of the chain's decay
            assert carried.size and ((carried > 0).all() if decay is DECAY_ACTIVE else (carried < 0).all())
        loss = m.run_loss(wb, samples)
        loss.backward()
        assert (_launches() > c0) == chain
        res.append((loss.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters() if v.grad is not None}))
        with torch.no_grad():
            enc.append([e.cpu() for e in m.encode(t_list, 8, False)[0]])
    (l1, g1), (l0, g0) = res
    print("%s: loss chain %.8f per-position %.8f" % (module, l1.item(), l0.item()))
    assert abs(l0.item() - l1.item()) < 2e-5 * abs(l0.item()), (l0.item(), l1.item())
    assert set(g0) == set(g1) and len(g0) >= 8
    for k in ("ent_encoder.layer_2.exponential_decay.weight", "ent_encoder.layer_2.exponential_decay.bias"):
        assert k in g1 and (float(g0[k].abs().max()) > 0) == (decay is DECAY_ACTIVE)      # (DECAY: every decayed row of the step has dt = 1, clamped)
        print("%s: d_%s chain %.8e per-position %.8e" % (module, k, float(g1[k].view(-1)[0]), float(g0[k].view(-1)[0])))
    for k in g0:
        assert_close(g1[k], g0[k], 1e-4, 3e-6 * max(1.0, float(g0[k].abs().max())), module + " chain vs per-position: d_" + k)
    for a, b in zip(*enc):
        assert_close(a, b, 1e-5, 2e-6, module + " encode(train=False) chain vs per-position")

    # ... and the float64 oracle of the reference's forward with --learnable-lambda: loss and the two decay gradients
    from tests.golden_util import T, slice_graphs
    _, _, times, gd = slice_graphs()
    tl = sorted([int(t) for t in z["t_list"]], reverse=True)
    assert tl == [int(t) for t in z["t_list"]]
    targets = [O.edge_subgraph(gd["train"][t], z["choice_%d" % i]) for i, t in enumerate(tl)]
    m64 = O.map_params(model, lambda t: t.double().clone().requires_grad_(True))
    fn = O.bi_forward_loss if module.startswith("Bi") else O.uni_forward_loss
    ref, _ = fn(m64, cfg, gd["train"], tl, times, 8, targets, samples)
    ref.backward()
    print("%s: loss float64 oracle %.8f" % (module, ref.item()))
    assert abs(ref.item() - l1.item()) < 2e-5 * abs(ref.item()), (ref.item(), l1.item())
    w64, b64 = m64["ent_encoder"]["layer_2"]["exponential_decay"]
    for k, r in (("weight", w64.grad), ("bias", b64.grad)):
        assert_close(g1["ent_encoder.layer_2.exponential_decay." + k], r.float(), 1e-4, 3e-6 * max(1.0, float(r.abs().max())), module + " d_%s vs float64 oracle" % k)
