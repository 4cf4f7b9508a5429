"""gru_chain(offset=...) and the window models' choice of path for --use-time-embedding, on the CPU test backend.

The stock CpuTestBackend has no gru_chain_offset_supported: a time-embedding model keeps the per-position loop there, as before.
OffsetCpuBackend (below) adds the offset keywords in plain torch, which drives _GruChainFn's plumbing -- the (table, index) pair,
the d_state buffer, the table's gradient through the static inverse -- and the models' offset tables and batched all-entity pass
without a GPU."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import gru_chain as GC
from temp_amd.gru_chain import GruInstance, GruProgram
from tests.chain_cases import make_rnns, random_program
from tests.cpu_backend import CpuTestBackend
from tests.golden_util import assert_close
from tests.test_gpu_chain_learnable_decay import loss_weights
from tests.test_gpu_chain_time_embedding import (T_ROWS, check, check_against_oracle, loop_reference, offset_index, offset_table, run_chain,
                                                  window_model)

CPU = torch.device("cpu")
MASK = _lib.CHAIN_HAS_PREV - 1


class OffsetCpuBackend(CpuTestBackend):
    """CpuTestBackend + the state-offset keywords of the chain methods (HipBackend's contract)."""

    def __init__(self):
        self.offset_launches = 0

    def gru_chain_offset_supported(self, d, variant):
        return d % 4 == 0

    def gru_chain_offset_layout(self, d):
        return _lib.CHAIN_PACK_F32

    def gru_chain_offset_launches(self):
        return self.offset_launches

    def gru_chain_pack_multi(self, w_hhs, layout=None):
        assert layout in (None, _lib.CHAIN_PACK_F32)
        return [self.gru_chain_pack(w) for w in w_hhs]

    def gru_chain_fwd(self, tabs, gi, lam, variant, packs, b_hhs, h_out, saved_all, gi_index=None, offset=None):
        if offset is None:
            return super().gru_chain_fwd(tabs, gi, lam, variant, packs, b_hhs, h_out, saved_all, gi_index=gi_index)
        self.offset_launches += 1
        table, index = offset[0].detach(), offset[1].long()
        panel, rows, sinfo, dt = self._chain_tables(tabs)
        if gi_index is not None:
            gi = gi[gi_index.long()]
        d = saved_all.shape[2]
        for rnn, s0, ns, _ in panel.tolist():
            w_hh, b_hh = packs[rnn], b_hhs[rnn].detach()
            state = torch.zeros(_lib.CHAIN_TRACKS, d)
            for s in range(s0, s0 + ns):
                e = rows[s]
                act = e >= 0
                r = (e & MASK)[act]
                hp = (((e >> 30) & 1) == 1)[act]
                hd = state[act] * torch.exp(-dt[r] * lam).view(-1, 1) * hp.view(-1, 1).to(state.dtype)
                gh = torch.mm(hd, w_hh.t()) + b_hh
                h_r, h_z, h_n = gh.chunk(3, 1)
                g = gi[r]
                if variant == _lib.GRU_TORCH:
                    i_r, i_z, i_n = g.chunk(3, 1)
                    rg, zg = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
                else:
                    i_n = g
                    rg, zg = torch.sigmoid(h_r), torch.sigmoid(h_z)
                ng = torch.tanh(i_n + rg * h_n)
                k = index[r]
                h = (1 - zg) * ng + zg * hd + table[k.clamp(min=0)] * (k >= 0).view(-1, 1).to(table.dtype)      # the sum is the state
                for j, v in enumerate((rg, zg, ng, h_n, hd)):
                    saved_all[j, r] = v
                if sinfo[s, 0] & 2:
                    h_out[r] = h
                state = torch.zeros_like(state)
                state[act] = h

    def gru_chain_bwd(self, tabs, saved_all, ups, lam, variant, packs, b_hhs, dgi, dgh, offset=None, d_state=None):
        if offset is None:
            return super().gru_chain_bwd(tabs, saved_all, ups, lam, variant, packs, b_hhs, dgi, dgh)
        self.offset_launches += 1
        panel, rows, sinfo, dt = self._chain_tables(tabs)
        d = saved_all.shape[2]
        for rnn, s0, ns, _ in panel.tolist():
            w_hh = packs[rnn]
            dprev = torch.zeros(_lib.CHAIN_TRACKS, d)
            nxt_has = torch.zeros(_lib.CHAIN_TRACKS, dtype=torch.bool)
            for s in range(s0 + ns - 1, s0 - 1, -1):
                e = rows[s]
                act = e >= 0
                r = (e & MASK)[act]
                rg, zg, ng, hn, hd = (saved_all[k, r] for k in range(5))
                g = torch.zeros(r.shape[0], d)
                sel = int(sinfo[s, 1])
                if sel >= 0 and ups[sel] is not None:
                    g = g + ups[sel].detach()[r - int(sinfo[s, 2])]
                g = g + dprev[act] * nxt_has[act].view(-1, 1).to(g.dtype)
                if d_state is not None:
                    d_state[r] = g                                  # ds/dh = I: the gate gradients below are the offset-free ones
                dn_pre = g * (1 - zg) * (1 - ng * ng)
                dz_pre = g * (hd - ng) * zg * (1 - zg)
                dr_pre = dn_pre * hn * rg * (1 - rg)
                dgi[r] = torch.cat([dr_pre, dz_pre, dn_pre], 1) if variant == _lib.GRU_TORCH else dn_pre
                gh = torch.cat([dr_pre, dz_pre, dn_pre * rg], 1)
                dgh[r] = gh
                dp = (torch.mm(gh, w_hh) + g * zg) * torch.exp(-dt[r] * lam).view(-1, 1)
                dprev = torch.zeros_like(dprev)
                dprev[act] = dp
                nxt_has = act & (((e >> 30) & 1) == 1)

    def gru_chain_bwd_g4(self, tabs, saved_all, ups, lam, variant, packs, b_hhs, g4, keys=None, offset=None, d_state=None):
        assert keys is None
        N, d = saved_all.shape[1], saved_all.shape[2]
        dgi, dgh = torch.zeros(N, 3 * d), torch.zeros(N, 3 * d)
        self.gru_chain_bwd(tabs, saved_all, ups, lam, variant, packs, b_hhs, dgi, dgh, offset=offset, d_state=d_state)
        g4.copy_(torch.cat([dgi, dgh[:, 2 * d:]], 1))


@pytest.fixture
def offset_backend():
    be = OffsetCpuBackend()
    TB.set_backend(be)
    yield be
    TB.set_backend(None)


@pytest.fixture
def stock_backend():
    TB.set_backend(CpuTestBackend())
    yield
    TB.set_backend(None)


MODELS = [("GRRGCN", "G10_uni_grrgcn_rol"), ("BiGRRGCN", "G10_bi_grrgcn_rol")]


def _inputs(z):
    from tests.window_cases import window_inputs
    edge_ids, samples = window_inputs(z)
    return torch.tensor([int(t) for t in z["t_list"]]), edge_ids, samples


def _loss_and_grads(m, t_list, edge_ids, samples):
    wb = m.prepare(t_list, 8, True, edge_ids)
    loss = m.run_loss(wb, samples)
    loss.backward()
    return wb, loss.detach(), {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None}


@pytest.mark.parametrize("module,golden", MODELS)
def test_stock_backend_keeps_the_per_position_loop(stock_backend, module, golden):
    """A backend without gru_chain_offset_supported: _can_chain() is False under the flag, and the step is the same computation as
    with the chain switched off."""
    m, _, _, z = window_model(module, golden, True, 1.0, CPU)
    assert m._can_batch() and not m._can_chain()
    t_list, edge_ids, samples = _inputs(z)
    wb, loss, grads = _loss_and_grads(m, t_list, edge_ids, samples)
    assert wb.program is None
    m0, *_ = window_model(module, golden, False, 1.0, CPU)
    wb0, loss0, grads0 = _loss_and_grads(m0, t_list, edge_ids, samples)
    assert wb0.program is None and torch.equal(loss, loss0)
    assert set(grads) == set(grads0) and "ent_encoder.layer_2.time_embed" in grads
    for k in grads:
        assert torch.equal(grads[k], grads0[k]), k


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("module,golden", MODELS)
def test_models_chain_the_time_embedding_where_the_backend_takes_it(offset_backend, module, golden, scale):
    m, model, cfg, z = window_model(module, golden, True, scale, CPU)
    assert m._can_chain()
    t_list, edge_ids, samples = _inputs(z)
    wb, loss, grads = _loss_and_grads(m, t_list, edge_ids, samples)
    assert wb.program is not None and m._fused_all_entity_ok(wb) and offset_backend.offset_launches == 2
    index = wb.chain_offset[0]
    assert index.numel() == wb.program.n_total and int(index.max()) < len(model["ent_encoder"]["layer_2"]["time_embed"])
    rows_of = lambda i: index[wb.program.inst[i].h0:wb.program.inst[i].h0 + wb.program.inst[i].n]
    for i in (wb.hist_inst if isinstance(wb.hist_inst, list) else [wb.hist_inst]):
        assert rows_of(i).numel() and bool((rows_of(i) >= 0).all())                            # history rows: their own position's row
    for i in wb.out_inst:
        assert bool((rows_of(i) == -1).all()) == module.startswith("Bi")                      # bi: the centre cells add none, their sum gets it once
    m0, *_ = window_model(module, golden, False, scale, CPU)
    wb0, loss0, grads0 = _loss_and_grads(m0, t_list, edge_ids, samples)
    assert wb0.program is None and offset_backend.offset_launches == 2
    assert abs(loss.item() - loss0.item()) < 2e-5 * abs(loss0.item())
    assert set(grads) == set(grads0) and float(grads["ent_encoder.layer_2.time_embed"].abs().max()) > 0
    for k in grads0:
        assert_close(grads[k], grads0[k], 1e-4, 3e-6 * max(1.0, float(grads0[k].abs().max())), module + " chain vs per-position: d_" + k)
    check_against_oracle(module, model, cfg, z, samples, loss, grads)
    with torch.no_grad():
        for a, b in zip(m.encode(t_list, 8, False)[0], m0.encode(t_list, 8, False)[0]):
            assert_close(a, b, 1e-5, 2e-6, module + " encode(train=False) chain vs per-position")


@pytest.mark.parametrize("rep", [False, True])
@pytest.mark.parametrize("module,golden", MODELS)
def test_all_embeds_batched_equals_the_per_window_pass(offset_backend, module, golden, rep):
    """all_embeds_batched under the flag (pair rows and zero-state rows + time_embed_2[t_b] once per window, active rows from the
    encoder) against get_all_embeds_Gt window by window; also in the (window, entity) layout the dropout draws take."""
    m, _, _, z = window_model(module, golden, True, 4.0, CPU)
    m._force_all_rep = rep
    t_list, edge_ids, _ = _inputs(z)
    wb = m.prepare(t_list, 8, True, edge_ids)
    assert m._fused_all_entity_ok(wb)
    out, hist = m.run(wb)
    big = m.all_embeds_batched(wb, out, hist)
    assert bool(getattr(wb, "all_rep", False)) == rep and wb.n_inactive > 0
    w = torch.randn(big.shape, generator=torch.Generator().manual_seed(5))
    (big * w).sum().backward()
    got = {k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None}
    m.zero_grad()
    out, hist = m.run(wb)
    per = list(out.split(wb.target.sizes))
    rows = [m.get_all_embeds_Gt(per[b], g, wb.rows[b][-1], wb.plan, b, hist) for b, g in enumerate(wb.graphs)]
    for b, r in enumerate(rows):
        assert_close(big[b], r, 1e-5, 2e-6, "%s all-entity rows of window %d" % (module, b))
    (torch.stack(rows) * w).sum().backward()
    assert "ent_encoder.layer_2.time_embed" in got
    for k, v in m.named_parameters():
        if v.grad is not None:
            assert_close(got[k], v.grad, 1e-4, 3e-6 * max(1.0, float(v.grad.abs().max())), "all-entity pass: d_" + k)


def test_refused_program_stays_on_the_loop_at_prepare_time(offset_backend, monkeypatch):
    """Chain tables the kernels refuse (here: a step limit below the window length): decided in prepare, the run takes the loop."""
    m, _, _, z = window_model("BiGRRGCN", "G10_bi_grrgcn_rol", True, 1.0, CPU)
    t_list, edge_ids, samples = _inputs(z)
    ref = _loss_and_grads(m, t_list, edge_ids, samples)
    assert ref[0].program is not None
    monkeypatch.setattr(_lib, "CHAIN_MAX_STEPS", 4)
    m1, *_ = window_model("BiGRRGCN", "G10_bi_grrgcn_rol", True, 1.0, CPU)
    assert m1._can_chain()
    wb, loss, grads = _loss_and_grads(m1, t_list, edge_ids, samples)
    assert wb.program is None
    assert abs(loss.item() - ref[1].item()) < 2e-5 * abs(loss.item())
    for k in ref[2]:
        assert_close(grads[k], ref[2][k], 1e-4, 3e-6 * max(1.0, float(ref[2][k].abs().max())), "loop vs chain: d_" + k)


def test_other_models_and_layouts_still_refuse_the_flag(offset_backend):
    """Unchanged under --use-time-embedding: both layers recurrent (rec_stack), the Impute* / Post* classes, several GRU layers."""
    from temp_amd.dynamic_rgcn import DynamicRGCN
    from temp_amd.post_dynamic_rgcn import ImputeDynamicRGCN, PostEnsembleBiDynamicRGCN
    from tests.window_cases import make_args, slice_snapshots
    s = slice_snapshots()
    mk = lambda cls, **kw: cls(make_args(use_time_embedding=True, **kw), s["num_e"], s["num_r"], s["tr"], s["va"], s["te"])
    m = mk(DynamicRGCN, module="GRRGCN", rec_only_last_layer=False)
    assert not m._can_batch() and not m._can_stack() and not m._can_chain()
    m = mk(DynamicRGCN, module="GRRGCN", rec_only_last_layer=True, num_layers=2)
    assert not m._can_chain()
    for cls, kw in ((ImputeDynamicRGCN, dict(module="GRRGCN", impute=True)), (PostEnsembleBiDynamicRGCN, dict(module="BiGRRGCN", post_ensemble=True))):
        m = mk(cls, rec_only_last_layer=True, **kw)
        assert not m._can_chain()
        wb = m.prepare(torch.tensor([20, 15]), 8, True)
        assert wb.program is None and not m._fused_all_entity_ok(wb)
        assert not type(m)._window_base._fused_all_entity_ok(m, wb)


@pytest.mark.parametrize("want", [None, "some"])
def test_gru_chain_offset_gradients_equal_autograd_of_the_loop(offset_backend, want):
    """Two GRUs sharing the table (a bi chain): states, d_x, GRU parameters and d_table against the float64 loop; d_state is the
    gradient of every row's state, so its rows grouped by table row add up to d_table."""
    prog, n_x = random_program(33, n_chain=2, K=6, E=90, lo=20, hi=70)
    w = None if want is None else tuple(i for i, it in enumerate(prog.inst) if it.next < 0 or i % 3 == 1)[:8]
    d = 32
    rnns = make_rnns(2, d, False, 5)
    x = torch.randn(n_x, d, generator=torch.Generator().manual_seed(17)) * 0.5
    wts = loss_weights(prog, w, d)
    table, index = offset_table(d), offset_index(prog)
    ref = loop_reference(prog, x, rnns, table, index, False, w, wts)
    got = run_chain(prog, x, rnns, CPU, False, w, wts, table, index)
    assert offset_backend.offset_launches == 2
    check(got, ref, False, "float64 loop")
    sums = torch.zeros(T_ROWS, d).index_add_(0, torch.from_numpy(index[index >= 0]), got["d_state"][torch.from_numpy(index >= 0)])
    assert_close(sums, got["d_table"], 1e-5, 1e-5, "d_table = d_state summed by table row")


def test_index_without_a_prepared_inverse(offset_backend):
    """offset=(table, index): the inverse is built from a host copy of the index."""
    prog, n_x = random_program(33, n_chain=1, K=4, E=60, lo=20, hi=50)
    rnns = make_rnns(1, 32, False, 5)
    x = torch.randn(n_x, 32, generator=torch.Generator().manual_seed(17)) * 0.5
    table, index = offset_table(32).requires_grad_(True), offset_index(prog)
    out = GC.gru_chain(x, prog, rnns, 0.1, False, None, offset=(table, torch.from_numpy(index.astype(np.int32))))
    out.sum().backward()
    counts = torch.from_numpy(np.bincount(index[index >= 0], minlength=T_ROWS))
    assert table.grad.shape == table.shape and bool((table.grad[counts == 0] == 0).all()) and bool((table.grad[counts > 0] != 0).any())


def test_offset_free_call_passes_no_offset_keywords(stock_backend):
    """gru_chain(offset=None) calls the backend exactly as before (the stock test backend has no offset keywords)."""
    prog, n_x = random_program(33, n_chain=2, K=6, E=90, lo=20, hi=70)
    rnns = make_rnns(2, 32, False, 5)
    x = torch.randn(n_x, 32, generator=torch.Generator().manual_seed(17)) * 0.5
    wts = loss_weights(prog, None, 32)
    got = run_chain(prog, x, rnns, CPU, False, None, wts)
    ref = loop_reference(prog, x, rnns, torch.zeros(T_ROWS, 32), offset_index(prog), False, None, wts)
    for u, v in zip(got["outs"], ref["outs"]):
        assert_close(u, v.float(), 1e-5, 2e-6, "states")


def test_gru_chain_refuses_an_offset_it_cannot_run(offset_backend):
    """A program without chain tables (two GRUs in one chain): a clear error instead of states without the offset."""
    n = 12
    idx = np.arange(n, dtype=np.int64)
    inst = [GruInstance(n, 0, 0, -1, np.full(n, -1, dtype=np.int64), np.ones(n, dtype=np.float32)),
            GruInstance(n, n, 1, 0, idx, np.full(n, 3, dtype=np.float32))]
    prog = GruProgram(inst)
    assert prog.chain_plan() is None
    rnns = make_rnns(2, 32, False, 5)
    x = torch.randn(2 * n, 32)
    table = offset_table(32).requires_grad_(True)
    off = (table,) + GC.offset_tables(np.zeros(2 * n, dtype=np.int64), T_ROWS, CPU)
    with pytest.raises(_lib.TempAmdError, match="state offset"):
        GC.gru_chain(x, prog, rnns, 0.1, False, None, offset=off)
    GC.gru_chain(x, prog, rnns, 0.1, False, None)              # without an offset the per-position cells still run it
    # ... and so does a backend without the offset methods, whatever the program
    TB.set_backend(CpuTestBackend())
    prog2, n_x = random_program(33, n_chain=2, K=6, E=90, lo=20, hi=70)
    off2 = (table,) + GC.offset_tables(offset_index(prog2), T_ROWS, CPU)
    with pytest.raises(_lib.TempAmdError, match="state offset"):
        GC.gru_chain(torch.randn(n_x, 32), prog2, rnns, 0.1, False, None, offset=off2)


# recorded on the commit before _GruChainFn was split into one function per route (tests/chain_route_cases.py), never on the code under test
OFFSET_LAUNCHES = [('gru_input_gates_multi', (), ()),
                   ('gru_chain_pack_multi', (), ('layout',)),
                   ('gru_chain_fwd', ((553, 96), (553, 32), (5, 553, 32)), ('offset',)),
                   ('gru_chain_bwd_g4', ((5, 553, 32), (553, 128)), ('d_state', 'offset')),
                   ('gru_grads_g4', (), ()),
                   ('segment_sum_rows', ((553, 32), (8,), (491,)), ())]


def test_offset_route_launches(offset_backend):
    from tests.chain_route_cases import OFFSET_CASE, run_route
    assert run_route(OFFSET_CASE, CPU)[0] == OFFSET_LAUNCHES
