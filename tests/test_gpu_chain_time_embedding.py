"""--use-time-embedding windows on the persistent chain kernels: row rho leaves s = GRU(x, dec . s_prev) + table[index[rho]], the sum
is the state the next position decays (temp_gru_chain_fwd with TempGruChain.offset), the backward also writes the gradient reaching every row's state
(d_state) and the table's gradient is the deterministic adjoint of the row gather.

Kernels against a float64 autograd loop over the program's instances (written here), a range-stress table (states up to 14, past the
f16 split's constant scale), identities against the chain without an offset, bit-repeatability, the offset-free path untouched,
offset + learnable decay together, and the window models against their per-position path and the float64 oracle.

Measured on the MI355X against the float64 loop (absolute errors, want = None; the bars are rtol 1e-5 / atol 2e-6 . max(1, max |ref|)
for the states -- 1e-4 / 2e-5 for the type-1 cell -- and 1e-4 / 2e-5 . max(1, max |ref|) for the gradients):
  d = 200 nn.GRU (bf16 kernels forced)  states 3.5e-07 (max |ref| 2.6)  d_x 6.8e-06  parameters 5.0e-05 (max |ref| 4.6e+02)  d_table 4.8e-05 (max |ref| 2.6e+02)
  d = 32  nn.GRU (several panels)       states 2.3e-07 (max |ref| 3.1)  d_x 2.1e-06  parameters 2.7e-04 (max |ref| 1.4e+03)  d_table 3.5e-05 (max |ref| 2.7e+02)
  d = 16  type-1                        states 7.2e-07 (max |ref| 2.4)  d_x 2.4e-05  parameters 3.1e-05 (max |ref| 3.5e+02)  d_table 3.5e-05 (max |ref| 2.0e+02)
  d = 216 nn.GRU (bf16, partial tiles)  states 2.7e-07 (max |ref| 2.0)  d_x 1.4e-06  parameters 6.6e-06 (max |ref| 4.4e+01)  d_table 3.0e-06 (max |ref| 3.1e+01)
  d = 220 nn.GRU (fp32 kernels)         states 3.3e-07 (max |ref| 3.2)  d_x 4.3e-06  parameters 1.9e-05 (max |ref| 1.5e+02)  d_table 1.0e-05 (max |ref| 1.3e+02)
  d = 200, max |table| = 8              states 3.5e-06 (max |ref| 14)   d_x 1.2e-05  parameters 1.2e-04 (max |ref| 7.9e+02)  d_table 3.0e-05 (max |ref| 2.6e+02)
  d = 200, zero table vs offset-free    states 3.9e-07                  d_x 4.3e-06  parameters 6.1e-05 (max |ref| 4.5e+02)
  d = 200, offset + learnable decay     states 3.8e-07 (max |ref| 2.7)  d_x 7.6e-06  parameters 5.5e-05 (max |ref| 4.6e+02)  d_table 3.3e-05 (max |ref| 2.6e+02)
                                        d_arg 1.3e-05 (max |ref| 78)  d_w 2.2e-05 of 5.3e+03  d_b 9.9e-06 of 1.6e+03
  the `want`-subset runs are at or below these.  Window models (D = 32, ICEWS14 slice; chain against the per-position path): loss equal to
  all printed digits (GRRGCN 18.27647781, x 4: 18.39201355; BiGRRGCN 24.36687851, x 4: 24.43566132; float64 oracle within 2e-8 relative),
  largest gradient difference 9.3e-08 (d_time_embed of BiGRRGCN x 4, max |ref| 5.3e-02).
Every case prints its figures before it asserts (pytest -s).
"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import temp_oracle as O
from temp_amd import _lib
from temp_amd import gru_chain as GC
from temp_amd.backend import get_backend
from tests.chain_cases import make_rnns, random_program
from tests.golden_util import assert_close, load
from tests.test_gpu_chain_learnable_decay import (SHAPES, WB, _err, _out_insts, _params, _want, _x, check_decay_grads, has_prev_rows, loss_weights,
                                                   row_dt)
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
T_ROWS = 7                   # timestamps of the table
UNUSED = 4                   # ... of which no row uses this one: its d_table row must be exactly 0
NONE_INST = 1                # every row of this instance carries -1 (no offset)


def _launches():
    return _lib.load().temp_gru_chain_offset_launches()


def offset_table(d, seed=23, max_abs=None):
    t = torch.randn(T_ROWS, d, generator=torch.Generator().manual_seed(seed)) * 0.5
    return t if max_abs is None else t * (max_abs / float(t.abs().max()))


def offset_index(prog, seed=29):
    """int64 [n_total]: a random timestamp per row out of T_ROWS without UNUSED; -1 on every row of instance NONE_INST."""
    rng = np.random.default_rng(seed)
    used = np.array([t for t in range(T_ROWS) if t != UNUSED])
    idx = used[rng.integers(0, used.size, prog.n_total)].astype(np.int64)
    it = prog.inst[NONE_INST]
    assert it.n > 0
    idx[it.h0:it.h0 + it.n] = -1
    return idx


def loop_reference(prog, x, rnns, table, index, type1, want, weights, wb=None, lam=0.1):
    """float64 autograd over the per-position loop: instance by instance, previous rows through prev_idx, O.decay_hidden,
    O.gru_torch / O.gru_type1, plus the row's table row -- the sum is what the next instance reads.  wb = (w, b): the learnable
    decay's argument enters as a per-row leaf, as in test_gpu_chain_learnable_decay.loop_reference.
    -> dict(outs, d_x, grads, d_table [+ d_arg, d_w, d_b, terms_w, terms_b])."""
    x64 = x.detach().double().clone().requires_grad_(True)
    P = [[p.detach().cpu().double().clone().requires_grad_(True) for p in _params(m, type1)] for m in rnns]
    tab = table.detach().double().clone().requires_grad_(True)
    idx = torch.from_numpy(np.asarray(index, dtype=np.int64))
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
        k = idx[it.h0:it.h0 + it.n]
        H.append(cell(x64[it.x0:it.x0 + it.n], hd, *P[it.rnn]) + tab[k.clamp(min=0)] * (k >= 0).double().view(-1, 1))
    loss = sum((H[i] * wgt.double()).sum() for i, wgt in zip(_out_insts(prog, want), weights))
    loss.backward()
    res = dict(outs=[H[i].detach() for i in _out_insts(prog, want)], d_x=x64.grad, grads=[p.grad if p.grad is not None else torch.zeros_like(p) for ps in P for p in ps],
               d_table=tab.grad if tab.grad is not None else torch.zeros_like(tab))
    if wb is not None:
        d_arg = torch.cat([a.grad.view(-1) if a.grad is not None else torch.zeros(a.numel(), dtype=torch.float64) for a in args])
        dt_all = torch.from_numpy(row_dt(prog))
        res.update(d_arg=d_arg, d_w=(d_arg * dt_all).sum(), d_b=d_arg.sum(), terms_w=(d_arg * dt_all).abs().sum(), terms_b=d_arg.abs().sum())
    return res


@contextlib.contextmanager
def _spy(be, seen):
    """Record what the backend calls of one gru_chain run were handed: the packs' layout, the d_state buffer, the decay's d_arg."""
    names = ("gru_chain_fwd", "gru_chain_fwd_x", "gru_chain_bwd", "gru_chain_bwd_g4", "gru_chain_decay_reduce")
    orig = {n: getattr(be, n) for n in names if hasattr(be, n)}

    def wrap(name, fn):
        def call(*a, **kw):
            if name.startswith("gru_chain_fwd"):
                packs = a[5] if name == "gru_chain_fwd_x" else a[4]
                seen["layout"] = getattr(packs[0], "chain_pack_layout", None)
                seen["fwd"] = name
            elif name == "gru_chain_decay_reduce":
                seen["d_arg"] = a[3]
            else:
                seen["d_state"] = kw.get("d_state")
                seen["keys"] = kw.get("keys")
            return fn(*a, **kw)
        return call
    for n, fn in orig.items():
        setattr(be, n, wrap(n, fn))
    try:
        yield
    finally:
        for n in orig:
            delattr(be, n)


def run_chain(prog, x, rnns, device, type1, want, weights, table=None, index=None, decay=None, lam=0.1):
    """gru_chain on `device` -> dict(outs, d_x, grads, d_table, d_state, layout, ...): d_state / layout are read off the backend calls."""
    leaf = x.detach().clone().to(device).requires_grad_(True)
    mods = [m.to(device) for m in rnns]
    for m in mods:
        m.zero_grad()
    spec = offset = tab = None
    if decay is not None:
        spec = (torch.tensor([[decay[0]]], dtype=torch.float32, device=device).requires_grad_(True),
                torch.tensor([decay[1]], dtype=torch.float32, device=device).requires_grad_(True))
    if table is not None:
        tab = table.detach().clone().to(device).requires_grad_(True)
        offset = (tab,) + GC.offset_tables(index, tab.shape[0], device)
    seen = {}
    with _spy(get_backend(), seen):
        out = GC.gru_chain(leaf, prog, mods, lam, type1, want, decay=spec, offset=offset)
        outs = [out[it.h0:it.h0 + it.n] for it in prog.inst] if want is None else list(out)
        loss = sum((o * wgt.to(device)).sum() for o, wgt in zip(outs, weights))
        loss.backward()
    res = dict(outs=[o.detach().cpu() for o in outs], d_x=leaf.grad.detach().cpu(), grads=[p.grad.detach().cpu().clone() for m in mods for p in _params(m, type1)],
               layout=seen.get("layout"), fwd=seen.get("fwd"), keys=seen.get("keys"), d_table=None, d_state=None, d_arg=None, d_w=None, d_b=None)
    if tab is not None:
        assert tab.grad.shape == tab.shape and seen["d_state"] is not None
        res.update(d_table=tab.grad.detach().cpu(), d_state=seen["d_state"].detach().cpu())
    if spec is not None:
        res.update(d_arg=seen["d_arg"].detach().cpu(), d_w=spec[0].grad.detach().cpu().view(()), d_b=spec[1].grad.detach().cpu().view(()))
    return res


def check(got, ref, type1, name):
    """The bars of test_gpu_chain_learnable_decay.check_states_and_grads with the states' absolute term scaled by max(1, max |ref|) too
    (the states are no longer bounded by 1); d_table is judged like the parameter gradients.  Prints before it asserts."""
    rt, at = (1e-4, 2e-5) if type1 else (1e-5, 2e-6)
    smax = max([float(v.abs().max()) for v in ref["outs"] if v.numel()] + [0.0])
    print("%s: states %.2e (max |ref| %.2e)  d_x %.2e  parameters %.2e (max |ref| %.2e)  d_table %.2e (max |ref| %.2e)" % (
        name, max([_err(u, v) for u, v in zip(got["outs"], ref["outs"])] + [0.0]), smax, _err(got["d_x"], ref["d_x"]),
        max(_err(u, v) for u, v in zip(got["grads"], ref["grads"])), max(float(v.abs().max()) for v in ref["grads"]),
        _err(got["d_table"], ref["d_table"]), float(ref["d_table"].abs().max())))
    for t in got["outs"] + [got["d_x"], got["d_table"]] + got["grads"]:
        assert bool(torch.isfinite(t).all())
    for u, v in zip(got["outs"], ref["outs"]):
        assert_close(u, v.float(), rt, at * max(1.0, smax), "states vs " + name)
    assert_close(got["d_x"], ref["d_x"].float(), 1e-4, 2e-5 * max(1.0, float(ref["d_x"].abs().max())), "d_x vs " + name)
    for u, v in zip(got["grads"] + [got["d_table"]], ref["grads"] + [ref["d_table"]]):
        assert_close(u, v.float(), 1e-4, 2e-5 * max(1.0, float(v.abs().max())), "parameter / table gradient vs " + name)
    assert bool((got["d_table"][UNUSED] == 0).all()) and bool((ref["d_table"][UNUSED] == 0).all())


def _f64(r):
    return dict(outs=[o.double() for o in r["outs"]], d_x=r["d_x"].double(), grads=[g.double() for g in r["grads"]],
                d_table=r["d_table"].double() if r["d_table"] is not None else None)


def _case(d, type1, kw, want=None, max_abs=None):
    prog, n_x = random_program(d + 1, **kw)
    w = _want(prog, want)
    return prog, w, make_rnns(kw["n_chain"], d, type1, 5), _x(n_x, d), loss_weights(prog, w, d), offset_table(d, max_abs=max_abs), offset_index(prog)


@pytest.mark.parametrize("d,type1,kw", SHAPES)
@pytest.mark.parametrize("want", [None, "some"])
def test_chain_kernels_vs_float64_loop(d, type1, kw, want):
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw, want)
    assert (index == -1).any() and not (index == UNUSED).any() and (index >= 0).any() and int(index.max()) < T_ROWS
    c0 = _launches()
    if d == 248:
        # past the chain kernels' widest d (temp_gru_chain_supported(248) == 0; the per-position cell kernels add no offset):
        # gru_chain says so and launches nothing
        assert not get_backend().gru_chain_supported(d) and not GC.chain_offset_usable(d, _lib.GRU_TORCH, 1)
        with pytest.raises(_lib.TempAmdError, match="state offset"):
            run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
        assert _launches() == c0
        return
    ref = loop_reference(prog, x, rnns, table, index, type1, w, wts)
    got = run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
    assert _launches() - c0 == 2                      # one forward, one backward launch carried the offset
    assert got["layout"] in (_lib.CHAIN_PACK_BX, _lib.CHAIN_PACK_F32) and got["fwd"] == "gru_chain_fwd" and got["keys"] is None
    if d == 200:
        assert _lib.load().temp_gru_chain_pack_layout(d) in (_lib.CHAIN_PACK_HX, _lib.CHAIN_PACK_BX, _lib.CHAIN_PACK_F32)
        assert got["layout"] == _lib.load().temp_gru_chain_offset_layout(d)
    check(got, ref, type1, "float64 loop (d = %d%s%s)" % (d, ", type-1" if type1 else "", ", want" if w is not None else ""))


def test_range_stress_states_past_the_f16_state_scale():
    """max |table| = 8: states reach 14 (the blend carries dec . s_prev on), where the f16 layouts' constant scale 2^14 (|state| < 4) would overflow."""
    d, type1, kw = SHAPES[0]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw, max_abs=8.0)
    assert abs(float(table.abs().max()) - 8.0) < 1e-5
    ref = loop_reference(prog, x, rnns, table, index, type1, w, wts)
    assert max(float(v.abs().max()) for v in ref["outs"] if v.numel()) > 7.5
    got = run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
    assert got["layout"] in (_lib.CHAIN_PACK_BX, _lib.CHAIN_PACK_F32)
    check(got, ref, type1, "float64 loop (d = 200, max |table| = 8)")


def _bit_equal(a, b):
    for u, v in zip(a["outs"] + [a["d_x"]] + a["grads"], b["outs"] + [b["d_x"]] + b["grads"]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("shape", [4, 5])
def test_zero_table_is_the_chain_without_an_offset_bitwise(shape):
    """d = 216 (bf16 kernels) and 220 (fp32 kernels): the offset-free chain runs on the same layout, so h + 0 changes no bit."""
    d, type1, kw = SHAPES[shape]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    a = run_chain(prog, x, rnns, DEV, type1, w, wts, torch.zeros_like(table), index)
    b = run_chain(prog, x, rnns, DEV, type1, w, wts)
    assert a["layout"] == b["layout"] and b["layout"] in (_lib.CHAIN_PACK_BX, _lib.CHAIN_PACK_F32)
    _bit_equal(a, b)


def test_zero_table_matches_the_chain_without_an_offset_d200():
    """d = 200: the offset-free chain may run on the f16 kernels, the offset chain does not -- same result inside the bars."""
    d, type1, kw = SHAPES[0]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    a = run_chain(prog, x, rnns, DEV, type1, w, wts, torch.zeros_like(table), index)
    b = run_chain(prog, x, rnns, DEV, type1, w, wts)
    ref = _f64(b)
    ref["d_table"] = a["d_table"].double()            # (the offset-free run has no table; its gradient is checked against float64 above)
    check(a, ref, type1, "offset-free chain (d = 200, zero table)")


def test_bit_repeatable():
    d, type1, kw = SHAPES[0]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    a = run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
    b = run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
    _bit_equal(a, b)
    assert torch.equal(a["d_state"], b["d_state"]) and torch.equal(a["d_table"], b["d_table"])


def test_offset_free_chain_untouched_by_an_offset_run():
    d, type1, kw = SHAPES[0]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    c0 = _launches()
    before = run_chain(prog, x, rnns, DEV, type1, w, wts)
    assert _launches() == c0
    run_chain(prog, x, rnns, DEV, type1, w, wts, table, index)
    c1 = _launches()
    assert c1 == c0 + 2
    after = run_chain(prog, x, rnns, DEV, type1, w, wts)
    assert _launches() == c1
    _bit_equal(before, after)
    assert before["layout"] == after["layout"]


def test_offset_and_learnable_decay_together():
    """Both nullable arguments at once: hd = exp(-max(w dt + b, 0)) . (h_prev + offset_prev), so d_arg sees the offset too."""
    d, type1, kw = SHAPES[0]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    ref = loop_reference(prog, x, rnns, table, index, type1, w, wts, wb=WB)
    c0, e0 = _launches(), _lib.load().temp_gru_chain_decay_launches()
    got = run_chain(prog, x, rnns, DEV, type1, w, wts, table, index, decay=WB)
    assert _launches() - c0 == 2 and _lib.load().temp_gru_chain_decay_launches() - e0 == 2
    check(got, ref, type1, "float64 loop (d = 200, offset + learnable decay)")
    check_decay_grads(got, ref, prog, "float64 loop (d = 200, offset + learnable decay)")


@pytest.mark.parametrize("shape", [2, 4])
def test_multi_pack_zeroes_the_slabs_past_the_matrix(shape):
    """d = 16 and 216: 3d is no multiple of 32, so the backward kernel's slab walk (rounded up to an even count) ends one slab past
    the packed matrix.  The one-launch pack of several matrices must write that slab (zeros) as the single-matrix pack does: the
    pack buffer is uninitialised memory, here a block that held NaNs a moment ago."""
    d, type1, kw = SHAPES[shape]
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    n = _lib.load().temp_gru_chain_pack_floats(d) * kw["n_chain"]
    for with_offset in (True, False):
        poison = torch.full((n,), float("nan"), device=DEV)
        del poison                                        # back to the caching allocator: the next buffer of this size gets the block
        got = run_chain(prog, x, rnns, DEV, type1, w, wts, *((table, index) if with_offset else ()))
        assert got["layout"] == _lib.CHAIN_PACK_BX or (not with_offset and d == 16)       # (d = 16 without an offset: the f16 kernels)
        for t in got["outs"] + [got["d_x"]] + got["grads"]:
            assert bool(torch.isfinite(t).all())


def test_offset_on_an_f16_layout_is_refused():
    """The C ABI itself: an offset with packs in an f16 layout returns TEMP_E_UNSUPPORTED and launches nothing."""
    d, type1, kw = SHAPES[0]
    be = get_backend()
    prog, w, rnns, x, wts, table, index = _case(d, type1, kw)
    mods = [m.to(DEV) for m in rnns]
    tabs = prog.chain_tables(DEV, None)
    packs = be.gru_chain_pack_multi([m.weight_hh_l0.detach() for m in mods], layout=_lib.CHAIN_PACK_HX)
    N = prog.n_total
    gi = torch.zeros(N, 3 * d, device=DEV)
    H, saved = torch.full((N, d), 7.0, device=DEV), torch.zeros(5, N, d, device=DEV)
    c0 = _launches()
    with pytest.raises(_lib.TempAmdError):
        be.gru_chain_fwd(tabs, gi, 0.1, _lib.GRU_TORCH, packs, [m.bias_hh_l0.detach() for m in mods], H, saved,
                         offset=(table.to(DEV),) + GC.offset_tables(index, T_ROWS, DEV)[:1])
    torch.cuda.synchronize()
    assert _launches() == c0 and bool((H == 7.0).all())


# ---- window models ----------------------------------------------------------------------------------------------------
def window_model(module, golden, chain, scale, device=DEV):
    from tests.window_cases import make_args, slice_snapshots, state_dict_from_oracle
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    from temp_amd.dynamic_rgcn import DynamicRGCN
    s, z = slice_snapshots(), load(golden)
    cfg = dict(module=module, n_bases=16, inv_temperature=0.1, rec_only_last_layer=True, use_time_embedding=True)
    model = O.init_model(cfg, s["num_e"], s["num_r"], len(s["times"]), 32, seed=3)
    for ln in ("layer_1", "layer_2"):
        model["ent_encoder"][ln]["time_embed"] = model["ent_encoder"][ln]["time_embed"] * scale
    args = make_args(module=module, rec_only_last_layer=True, use_time_embedding=True, negative_rate=int(z["neg"]))
    m = (BiDynamicRGCN if module.startswith("Bi") else DynamicRGCN)(args, s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    m.load_state_dict(state_dict_from_oracle(model), strict=True)
    m.use_gru_chain = chain
    return m.to(device), model, cfg, z


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("module,golden", [("GRRGCN", "G10_uni_grrgcn_rol"), ("BiGRRGCN", "G10_bi_grrgcn_rol")])
def test_window_models_chain_vs_per_position_path(module, golden, scale):
    from tests.window_cases import window_inputs
    res, enc = [], []
    for chain in (True, False):
        m, model, cfg, z = window_model(module, golden, chain, scale)
        edge_ids, samples = window_inputs(z)
        t_list = torch.tensor([int(t) for t in z["t_list"]])
        assert m._can_batch() and m._can_chain() == chain
        c0 = _launches()
        wb = m.prepare(t_list, 8, True, edge_ids)
        assert (wb.program is not None) == chain and m._fused_all_entity_ok(wb)
        loss = m.run_loss(wb, samples)
        loss.backward()
        assert (_launches() > c0) == chain
        res.append((loss.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters() if v.grad is not None}))
        with torch.no_grad():
            enc.append([e.cpu() for e in m.encode(t_list, 8, False)[0]])
    (l1, g1), (l0, g0) = res
    print("%s (time_embed x %g): loss chain %.8f per-position %.8f" % (module, scale, l1.item(), l0.item()))
    assert abs(l0.item() - l1.item()) < 2e-5 * abs(l0.item()), (l0.item(), l1.item())
    assert set(g0) == set(g1) and len(g0) >= 8
    k = "ent_encoder.layer_2.time_embed"
    assert k in g1 and float(g1[k].abs().max()) > 0 and float(g0[k].abs().max()) > 0
    for k in g0:
        print("  d_%s: %.2e (max |per-position| %.2e)" % (k, _err(g1[k], g0[k]), float(g0[k].abs().max())))
    for k in g0:
        assert_close(g1[k], g0[k], 1e-4, 3e-6 * max(1.0, float(g0[k].abs().max())), module + " chain vs per-position: d_" + k)
    for a, b in zip(*enc):
        assert_close(a, b, 1e-5, 2e-6, module + " encode(train=False) chain vs per-position")

    check_against_oracle(module, model, cfg, z, samples, l1, g1)


def check_against_oracle(module, model, cfg, z, samples, loss, grads):
    """The float64 oracle of the reference's forward with --use-time-embedding: loss and every parameter gradient."""
    from tests.golden_util import slice_graphs
    from tests.window_cases import state_dict_from_oracle
    _, _, times, gd = slice_graphs()
    tl = sorted([int(t) for t in z["t_list"]], reverse=True)
    assert tl == [int(t) for t in z["t_list"]]
    targets = [O.edge_subgraph(gd["train"][t], z["choice_%d" % i]) for i, t in enumerate(tl)]
    m64 = O.map_params(model, lambda t: t.double().clone().requires_grad_(True))
    fn = O.bi_forward_loss if module.startswith("Bi") else O.uni_forward_loss
    ref, _ = fn(m64, cfg, gd["train"], tl, times, 8, targets, samples)
    ref.backward()
    print("%s: loss float64 oracle %.8f" % (module, ref.item()))
    assert abs(ref.item() - loss.item()) < 2e-5 * abs(ref.item()), (ref.item(), loss.item())
    sd64 = state_dict_from_oracle(m64)
    checked = 0
    for k, g in grads.items():
        r = sd64[k].grad
        if r is None:
            continue
        assert_close(g, r.float(), 1e-4, 3e-6 * max(1.0, float(r.abs().max())), module + " d_%s vs float64 oracle" % k)
        checked += 1
    assert checked >= 8 and sd64["ent_encoder.layer_2.time_embed"].grad is not None
