"""What tests/test_gpu_gru_cell_routes.py rests on, without a GPU: the fp64 restatement of the GRU cell in
tests/gru_cell_route_cases.py agrees with oracle.temp_oracle (gru_torch, gru_type1, decay_hidden and torch autograd) in float64,
the case table reaches every route the restated dispatch predicates can name, and the data recipes are deterministic."""
import pytest
import torch

from oracle import temp_oracle as O
from tests import gru_cell_route_cases as RC

RTOL = 1e-12


def _close(got, want, what):
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert torch.isfinite(got).all() and err <= RTOL * max(scale, 1e-300), "%s: error %.3e, max |want| %.3e" % (what, err, scale)


@pytest.mark.parametrize("learnable", [False, True], ids=["fixed", "learnable"])
@pytest.mark.parametrize("variant", [RC.TORCH, RC.TYPE1], ids=["torch", "type1"])
def test_restatement_matches_the_oracle(variant, learnable):
    n, d, n_prev = 13, 12, 17
    g = torch.Generator().manual_seed(5 + variant)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, prev = rnd(n, d) * 0.5, rnd(n_prev, d) * 0.5
    w_ih, w_hh, b_ih, b_hh = [p.double() for p in RC.gru_weights(d, variant, 3)]
    prev_idx = RC.index_rows(n, n_prev, 7)
    assert (prev_idx < 0).any() and (prev_idx >= 0).any()
    dt = RC.dt_rows(n, 9)
    wb = RC.WB if learnable else None
    if learnable:
        arg = wb[0] * dt + wb[1]
        assert (arg > 0).any() and (arg < 0).any()
    up = rnd(n, d)

    # the oracle, by autograd
    leaves = [t.clone().requires_grad_(True) for t in (x, w_ih, w_hh, b_ih, b_hh)]
    w_leaf = torch.tensor([[wb[0] if learnable else 0.0]], dtype=torch.float64, requires_grad=True)
    b_leaf = torch.tensor([wb[1] if learnable else 0.0], dtype=torch.float64, requires_grad=True)
    idx = prev_idx.long()
    rows = (prev[idx.clamp(min=0)] * (idx >= 0).double().view(-1, 1)).requires_grad_(True)
    hd = O.decay_hidden(rows, dt.double().view(-1, 1), RC.LAM, learnable=(w_leaf, b_leaf) if learnable else None)
    h = (O.gru_torch if variant == RC.TORCH else O.gru_type1)(leaves[0], hd, *leaves[1:])
    (h * up).sum().backward()

    # the restatement, stage by stage
    out = RC.forward64(variant, x, None, prev, prev_idx, dt, RC.LAM, wb, w_ih, w_hh, b_ih, b_hh)
    _close(out[0], h.detach(), "h")
    _close(out[5], hd.detach(), "hdec")
    gi = x @ w_ih.t() + b_ih
    hoisted = RC.forward64(variant, None, gi, prev, prev_idx, dt, RC.LAM, wb, None, w_hh, None, b_hh)
    for a, b in zip(out, hoisted):
        _close(a, b, "hoisted input gates")
    assert float(out[5][idx < 0].abs().max()) == 0.0
    saved = torch.stack(out[1:])
    dgi, dgh, dec, gz = RC.gates64(variant, saved, up, None, None, dt, RC.LAM, wb)
    d_prev = RC.d_prev64(dgh, w_hh, gz, dec)
    _close(d_prev, rows.grad, "d_prev")
    d_x, d_w_ih, d_w_hh, d_b_ih, d_b_hh = RC.weight_grads64(x, out[5], dgi, dgh, w_ih)
    for got, leaf, what in zip((d_x, d_w_ih, d_w_hh, d_b_ih, d_b_hh), leaves, ("d_x", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")):
        _close(got, leaf.grad, what)
    if learnable:
        d_w, d_b, t_w, t_b = RC.decay_wb_grads64(d_prev, prev, prev_idx, dt, wb)
        _close(d_w.view(1), w_leaf.grad.view(1), "d_decay_w")
        _close(d_b.view(1), b_leaf.grad.view(1), "d_decay_b")
        assert float(t_w) >= abs(float(d_w)) and float(t_b) >= abs(float(d_b)) > 0

    # the gradient gathered from the next position adds to the upstream one; the zero state is prev_idx = -1 everywhere
    nxt_tab, nxt = rnd(9, d), RC.index_rows(n, 9, 11)
    a = RC.gates64(variant, saved, up, nxt_tab, nxt, dt, RC.LAM, wb)
    nl = nxt.long()
    b = RC.gates64(variant, saved, up + nxt_tab[nl.clamp(min=0)] * (nl >= 0).double().view(-1, 1), None, None, dt, RC.LAM, wb)
    for u, v in zip(a, b):
        _close(u, v, "next_idx")
    only_next = RC.gates64(variant, saved, None, nxt_tab, nxt, dt, RC.LAM, wb)
    assert float(only_next[1][nl < 0].abs().max()) == 0.0
    zero = RC.forward64(variant, None, gi, None, None, dt, RC.LAM, wb, None, w_hh, None, b_hh)
    none = RC.forward64(variant, None, gi, prev, torch.full((n,), -1, dtype=torch.int32), dt, RC.LAM, wb, None, w_hh, None, b_hh)
    for u, v in zip(zero, none):
        assert torch.equal(u, v)
    # the absolute forms bound the plain ones
    for u, v in zip(RC.gates64(variant, saved, up, nxt_tab, nxt, dt, RC.LAM, wb, absolute=True)[:2], a[:2]):
        assert bool((u >= v.abs()).all())
    assert bool((RC.d_prev64(dgh, w_hh, gz, dec, absolute=True) >= d_prev.abs()).all())


def test_case_table_covers_the_route_set():
    hit = set()
    for c in RC.ALL:
        assert c.routes and c.routes <= RC.ROUTE_SET, (c.id, sorted(c.routes - RC.ROUTE_SET))
        hit |= c.routes
    assert hit == set(RC.ROUTE_SET), "routes without a case: %s" % sorted(RC.ROUTE_SET - hit)
    # every name the predicates can produce is in the set (a new route there must be added to ROUTE_SET, and then needs a case)
    for d in range(4, 400, 4):
        for v in RC.VNAME.values():
            for hoisted in (False, True):
                assert RC.fwd_route(d, hoisted) + "/" + v in RC.ROUTE_SET
        for n in (1, 4096 * 256 // RC.gates_lpr(d), 4096 * 256 // RC.gates_lpr(d) + 1):
            assert RC.gates_routes(d, n) <= RC.ROUTE_SET
        for hn in (False, True):
            assert RC.wgrad_routes(d, hn, not hn) <= RC.ROUTE_SET


def test_case_table_shapes_reach_their_edges():
    """The facts the issue's shapes rest on, from the restated predicates."""
    assert [RC.fwd_route(d, True) for d in (8, 36, 40, 100, 136, 200, 208, 260)] == ["wres", "stream_hoisted", "wres", "stream_hoisted",
                                                                                      "wres", "wres", "stream_hoisted", "stream_hoisted"]
    assert RC.fwd_route(4, True) == "stream_hoisted" and RC.fwd_route(204, True) == "stream_hoisted"
    assert [RC.gates_lpr(d) for d in (4, 32, 36, 64, 68, 128, 132, 200, 260)] == [8, 8, 16, 16, 32, 32, 64, 64, 64]
    for d, n in ((4, 131080), (36, 65540), (68, 32770), (132, 16389)):
        lpr = RC.gates_lpr(d)
        assert RC.gates_routes(d, n) == {"gates_lpr%d/stride" % lpr} and RC.gates_routes(d, n - 8) == {"gates_lpr%d/once" % lpr}
    assert RC.gates_routes(260, 37) == {"gates_lpr64/once", "gates/two_pass"} and RC.gates_routes(256, 37) == {"gates_lpr64/once"}
    assert 65540 * 36 // 4 > 2048 * 256 >= 5 * 8 // 4                      # the zero cell's grid-stride loop
    assert RC.multi_taken((20000, 17003), 200, RC.TORCH)
    assert not RC.multi_taken((900, 700), 200, RC.TORCH) and not RC.multi_taken((20000, 20000), 128, RC.TORCH)
    assert not RC.multi_taken((20000, 17003), 200, RC.TYPE1)
    # the dense-product planners at the shapes of the cases
    assert RC.panel_launches((37,), 200, 600) == {("panel", 1): 1} and RC.panel_launches((4100,), 200, 600) == {("wres", 1): 1}
    assert RC.panel_launches((131080,), 4, 12) == {("wres", 1): 1} and RC.panel_launches((65540,), 36, 108) == {("wres", 2): 1}
    assert RC.panel_launches((20000,), 200, 600) == {("hxp", 3): 1}        # tests/gemm_route_cases.py: the GRU d_x shape
    assert RC.tn_launches(300, 200, 200) == {("tn_split", 7): 1} and RC.tn_launches(300, 256, 100) == {("tn_w8", 4): 1}
    assert RC.tn_launches(300, 200, 328) == {("tn_w7", 7): 1} and RC.tn_launches(4100, 600, 200) == {}
    # integer data: every partial sum is an integer below 2^24
    assert max(c.d for c in RC.ALL) * 3 * 64 + 8 < 2 ** 24 and 4100 * 64 < 2 ** 24


def test_generators_are_deterministic():
    for fn, args in ((RC.standard, ((7, 12), 3)), (RC.wide, ((7, 12), 3)), (RC.wide_rows, ((7, 12), 3)), (RC.dt_rows, (9, 3)),
                     (RC.index_rows, (9, 12, 3)), (RC.pattern, (7, 12, 3, 5, 1)), (RC.gru_weights, (12, RC.TORCH, 3))):
        a, b = fn(*args), fn(*args)
        for u, v in zip(a, b) if isinstance(a, tuple) else ((a, b),):
            assert torch.equal(u, v), fn.__name__
    sat = RC.saturate(RC.standard((40, 60), 1), 2)
    assert torch.equal(sat, RC.saturate(RC.standard((40, 60), 1), 2))
    share = float((sat.abs() == 40.0).float().mean())
    assert 0.28 < share < 0.39 and bool((sat == 40.0).any()) and bool((sat == -40.0).any())
    case = next(c for c in RC.FORWARD if c.entry == "cell_fwd_multi" and any(c.zero) and not all(c.zero))
    fused = next(c for c in RC.FORWARD if c.entry == "gru_fwd" and c.ns[0] > 1)
    for c in (case, fused):
        for data in RC.DATA:
            for cell in range(len(c.ns)):
                a, b = RC.forward_operands(c, cell, data), RC.forward_operands(c, cell, data)
                assert a.keys() == b.keys()
                for k in a:
                    assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (c.id, data, k)
                assert (a["prev"] is None) == c.zero[cell]
                if data == "integer":
                    assert float(a["dt"].abs().max()) == 0.0 and bool((a["w_hh"] == a["w_hh"].round()).all())
