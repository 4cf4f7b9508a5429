"""Every route of the per-position GRU cell kernels (temp_amd/csrc/gru_kernels.hip behind temp_gru_fwd / temp_gru_bwd,
temp_gru_cell_fwd / _bwd and their _multi forms, temp_gru_weight_grads / _multi, k_decay_grad) on the MI355X, each against the
fp64 restatement of tests/gru_cell_route_cases.py, which also holds the cases and the routes they must take.

Every case goes through the HipBackend method the product uses, into NaN-filled outputs with 64 guard rows where the method lets
the caller allocate, and checks
  * the route: temp_gru_route_launches and temp_gemm_route_launches moved by exactly the case's entries, and the kernel trace
    (temp_trace_begin / temp_trace_end) holds exactly the case's kernel names;
  * guard rows keep their NaN bits, a second call gives the same bits;
  * all elements against fp64 (bars in the helpers' docstrings); nothing is sampled, nothing excluded.
Every case prints its figures before it asserts (pytest -s)."""
import ctypes
import functools

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import gru_chain as GCH
from tests import gemm_route_cases as GC
from tests import gru_cell_route_cases as RC
from tests.chain_cases import make_rnns, random_program
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
NAN = float("nan")
NAN_BITS = 0x7FC00000          # what torch.full(..., nan) writes
GUARD = 64
LAM = RC.f32(RC.LAM)
EPS = 2.0 ** -24
FIGURES = {}                   # "route quantity" -> largest error seen, as a fraction of its bar


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be
    TB.set_backend(None)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _all_nan_bits(t):
    return t.numel() == 0 or bool((_bits(t) == NAN_BITS).all())


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev(t):
    return None if t is None else t.to(DEV)


def _gemm_table(lib):
    return [[lib.temp_gemm_route_launches(r, w) for w in range(GC.WIDTHS)] for r in range(len(GC.ROUTES))]


def _gru_table(lib):
    return [lib.temp_gru_route_launches(r) for r in range(len(RC.GRU_ROUTES))]


class Routes:
    """with Routes() as r: ...  -> r.gemm {(route, width): launches}, r.gru {route: launches} of the block"""

    def __enter__(self):
        self.lib = _lib.load()
        self.g0, self.r0 = _gemm_table(self.lib), _gru_table(self.lib)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        g1, r1 = _gemm_table(self.lib), _gru_table(self.lib)
        self.gemm = {(GC.ROUTES[r], w): g1[r][w] - self.g0[r][w] for r in range(len(GC.ROUTES)) for w in range(GC.WIDTHS) if g1[r][w] != self.g0[r][w]}
        self.gru = {RC.GRU_ROUTES[r]: r1[r] - self.r0[r] for r in range(len(RC.GRU_ROUTES)) if r1[r] != self.r0[r]}
        return False


def _traced(fn, cap=64):
    """fn() between temp_trace_begin / temp_trace_end -> (result, names of the launches the library recorded)."""
    lib = _lib.load()
    ids, ms, cnt = (ctypes.c_int32 * cap)(), (ctypes.c_float * cap)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(cap), "temp_trace_begin")
    try:
        out = fn()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, cap, ctypes.byref(cnt)), "temp_trace_end")
    assert cnt.value < cap
    return out, [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)]


def _note(route, what, value):
    """keep the largest figure per (route, quantity); a new maximum is printed, so the last line of a key is the route's figure"""
    key = "%s %s" % (route, what)
    if float(value) > FIGURES.get(key, -1.0):
        FIGURES[key] = float(value)
        print("  figure  %-70s %.3e" % (key, float(value)))


def _ratio(err, bar):
    """largest err / bar over the elements (0 / 0 counts as 0, x / 0 and NaN as infinite)"""
    if err.numel() == 0:
        return 0.0
    inf = torch.full_like(err, float("inf"))
    q = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(torch.where(torch.isnan(q), inf, q).max())


def _within(got, want, bar, what):
    """every element of got is finite and within bar (a tensor) of want; -> the largest error as a fraction of its bar"""
    g = got.double()
    err = (g - want).abs()
    worst = _ratio(err, bar.expand_as(err) if bar.shape != err.shape else bar)
    bad = ~(torch.isfinite(g) & (err <= bar))
    if bool(bad.any()):
        i = [int(v) for v in torch.nonzero(bad)[0]]
        raise AssertionError("%s: %d/%d elements out of their bar (%d not finite), worst %.3g of the bar; first at %s: got %r, want %r, bar %.3e" % (
            what, int(bad.sum()), g.numel(), int((~torch.isfinite(g)).sum()), worst, i, float(g[tuple(i)]), float(want[tuple(i)]),
            float(bar.expand_as(err)[tuple(i)])))
    return worst


def _exact(got, want, what):
    g = got.double()
    bad = ~(g == want)
    if bool(bad.any()):
        i = [int(v) for v in torch.nonzero(bad)[0]]
        raise AssertionError("%s: %d/%d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), g.numel(), i, float(g[tuple(i)]), float(want[tuple(i)])))


# =====================================================================================================================
# forward
# =====================================================================================================================
def _wb(case):
    return None if case.decay is None else (RC.f32(case.decay[0]), RC.f32(case.decay[1]))


def _forward_call(be, case, ops):
    """One call of the case's method -> per cell (h buffer, n), saved_all [5, N, d], per cell row0."""
    d, v = case.d, case.variant
    if case.entry == "gru_fwd":
        o = ops[0]
        wb = None if case.decay is None else torch.tensor(case.decay, dtype=torch.float32, device=DEV)
        h, saved = be.gru_fwd(o["x"], o["prev"], o["prev_idx"], o["dt"], LAM, wb, o["w_ih"], o["w_hh"], o["b_ih"], o["b_hh"], v)
        assert h.shape == (case.ns[0], d) and saved.shape == (5, case.ns[0], d)
        return [h], saved, [0]
    row0, at = [], GUARD
    for n in case.ns:
        row0.append(at)
        at += n + GUARD
    saved_all = _nan(5, at, d)
    hbufs = [_nan(n + GUARD, d) for n in case.ns]
    if case.entry == "cell_fwd":
        o, n = ops[0], case.ns[0]
        be.gru_cell_fwd(o["gi"], o["prev"], o["prev_idx"], o["dt"], LAM, o["w_hh"], o["b_hh"], v, hbufs[0][:n], saved_all, row0[0])
    else:
        cells = [dict(gi=o["gi"], prev=o["prev"], prev_idx=o["prev_idx"], dt=o["dt"], w_hh=o["w_hh"], b_hh=o["b_hh"], h_out=hb[:n], row0=r0)
                 for o, hb, n, r0 in zip(ops, hbufs, case.ns, row0)]
        be.gru_cell_fwd_multi(cells, LAM, v, saved_all)
    torch.cuda.synchronize()
    return hbufs, saved_all, row0


def _forward_expect(case):
    """-> (gru routes, gemm routes, trace names) of one call"""
    gru, gemm, names = {}, {}, []
    live = [(n, z) for n, z in zip(case.ns, case.zero) if n > 0]
    if any(z for _, z in live):
        gru["fwd_zero"] = 1
        names.append("k_gru_fwd")
    if any(not z for _, z in live):
        route = RC.fwd_route(case.d, case.entry != "gru_fwd")
        gru["fwd_" + route] = 1
        names.append("k_gru_fwd")
        if route == "wres":
            gemm[("wres_split", 3)] = 1
    return gru, gemm, names


def check_forward_cell(case, cell, data, o, h, saved):
    """One cell's h [n, d] and saved planes [5, n, d] against forward64 of the same operands.

    Bars.  hdec = saved[4]: 1e-6 relative (the bar of test_decay_rows_vs_fp64: half an ulp of the argument, expf, the product),
    exactly 0 without a previous row.  hn = saved[3]: 1e-6 (sum |hdec||W_hn| + |b_hn|), the fp32-kernel bar of
    tests/test_gpu_gemm_routes.py.  r, z, n, h on standard data: rtol 1e-5 / atol 2e-6 (nn.GRU layout), 1e-4 / 2e-5 (type-1).
    On wide, saturated and integer data the product error is no longer below those: with S_g the sum of the absolute terms of the
    pre-activation of gate g (forward64(absolute=True)) and E_g = 1e-6 S_g its error,
        |dr| <= E_r / 4, |dz| <= E_z / 4                      (sigmoid' <= 1/4)
        |dn| <= E_n + |hn| |dr| + |r| |dhn|,  E_n = 1e-6 (S_n + |r hn|)      (tanh' <= 1; n = tanh(i_n + r hn))
        |dh| <= |1 - z| |dn| + |hdec - n| |dz| + |z| 1e-6 |hdec|            (h = (1 - z) n + z hdec, both variants)
    (first order: the products of two errors are below 1e-12 S^2) -- each added to the standard bar of its plane."""
    v, d = case.variant, case.d
    n = h.shape[0]
    if n == 0:
        return
    route = next(iter(r for r in case.routes if r.startswith("zero") == (o["prev"] is None)))
    wb = _wb(case)
    args = (v, o.get("x"), o.get("gi"), o["prev"], o["prev_idx"], o["dt"], LAM, wb, o["w_ih"], o["w_hh"], o["b_ih"], o["b_hh"])
    ref = RC.forward64(*args)
    s_r, s_z, s_n, s_hn = RC.forward64(*args, absolute=True)
    h64, r64, z64, n64, hn64, hd64 = ref
    got = [h] + [saved[k] for k in range(5)]
    for t in got:
        assert bool(torch.isfinite(t).all()), "%s %s cell %d: non-finite outputs" % (case.id, data, cell)
    assert bool(((saved[0] >= 0) & (saved[0] <= 1) & (saved[1] >= 0) & (saved[1] <= 1) & (saved[2].abs() <= 1)).all()), "gates out of range"
    what = "%s %s cell %d " % (case.id, data, cell)
    _note(route, "hdec / 1e-6 |hdec|", _within(saved[4], hd64, 1e-6 * hd64.abs(), what + "hdec"))
    if o["prev"] is None:
        assert bool((saved[4] == 0).all()), what + "hdec of a zero-state cell is not 0"
    elif o["prev_idx"] is not None:
        assert bool((saved[4][o["prev_idx"] < 0] == 0).all()), what + "hdec is not 0 where there is no previous row"
    _note(route, "hn / 1e-6 sum|a||b|", _within(saved[3], hn64, 1e-6 * s_hn, what + "hn"))
    if data == "integer":
        _exact(saved[3], hn64, what + "hn on integer operands")
        rows = torch.zeros(n, d, device=DEV, dtype=torch.float64) if o["prev"] is None else RC.gather64(o["prev"], o["prev_idx"], n)[0]
        _exact(saved[4], rows, what + "hdec at dt = 0")
    rt, at = (1e-5, 2e-6) if v == RC.TORCH else (1e-4, 2e-5)
    std = lambda w: at + rt * w.abs()
    if data == "standard":
        for name, g, w in (("r", saved[0], r64), ("z", saved[1], z64), ("n", saved[2], n64), ("h", h, h64)):
            _note(route, "%s / standard bar" % name, _within(g, w, std(w), what + name))
        return
    d_r, d_z, d_hn = 0.25e-6 * s_r, 0.25e-6 * s_z, 1e-6 * s_hn
    d_n = 1e-6 * (s_n + (r64 * hn64).abs()) + hn64.abs() * d_r + r64.abs() * d_hn
    d_h = (1 - z64).abs() * (std(n64) + d_n) + (hd64 - n64).abs() * (std(z64) + d_z) + z64.abs() * 1e-6 * hd64.abs()
    for name, g, w, extra in (("r", saved[0], r64, d_r), ("z", saved[1], z64, d_z), ("n", saved[2], n64, d_n), ("h", h, h64, d_h)):
        _note(route, "%s / propagated bar" % name, _within(g, w, std(w) + extra, what + name))


@pytest.mark.parametrize("case", RC.FORWARD, ids=[c.id for c in RC.FORWARD])
def test_forward_route(case, hip_backend):
    be = hip_backend
    want_gru, want_gemm, want_names = _forward_expect(case)
    for data in RC.DATA:
        ops = [{k: _dev(t) for k, t in RC.forward_operands(case, cell, data).items()} for cell in range(len(case.ns))]
        with Routes() as rt:
            hbufs, saved_all, row0 = _forward_call(be, case, ops)
        (hb2, sa2, _), names = _traced(lambda: _forward_call(be, case, ops))
        print("%s %s: gru %s gemm %s trace %s" % (case.id, data, sorted(rt.gru.items()), sorted(rt.gemm.items()), names))
        assert rt.gru == want_gru and rt.gemm == want_gemm, "launched %s %s, the case pins %s %s" % (rt.gru, rt.gemm, want_gru, want_gemm)
        assert names == want_names, (names, want_names)
        assert _same_bits(saved_all, sa2) and all(_same_bits(a, b) for a, b in zip(hbufs, hb2)), "two calls gave different bits"
        if case.entry != "gru_fwd":
            written = torch.zeros(saved_all.shape[1], dtype=torch.bool, device=DEV)
            for n, r0, hb in zip(case.ns, row0, hbufs):
                written[r0:r0 + n] = True
                assert _all_nan_bits(hb[n:]), "h_out: guard rows were written"
            assert _all_nan_bits(saved_all[:, ~written]), "saved_all: rows outside the cells were written"
        for cell, (n, r0, hb) in enumerate(zip(case.ns, row0, hbufs)):
            check_forward_cell(case, cell, data, ops[cell], hb[:n], saved_all[:, r0:r0 + n])


# =====================================================================================================================
# gate gradients and d_prev
# =====================================================================================================================
@functools.lru_cache(maxsize=4)
def _saved_planes(variant, d, ns, no_prev):
    """The forward of every cell (standard data, hoisted gates, the case's zero-state cells from prev = NULL) through
    temp_gru_cell_fwd_multi -> (saved_all, row0s, per cell operands): the GPU's own saved planes feed the backward."""
    fc = RC.fwd_case("cell_fwd_multi", variant, d, ns, prev_idx=True, zero=no_prev)
    ops = [{k: _dev(t) for k, t in RC.forward_operands(fc, cell, "standard").items()} for cell in range(len(ns))]
    _, saved_all, row0 = _forward_call(TB.get_backend(), fc, ops)
    return saved_all, row0, ops


def _bwd_operands(case, cell):
    n, d = case.ns[cell], case.d
    seed = 7000 + 100 * cell + d
    n_next = n // 2 + 3
    up = _dev(RC.standard((n, d), seed, 1.0)) if case.dh_up[cell] else None
    nxt = _dev(RC.index_rows(n, n_next, seed + 1)) if case.next_idx[cell] else None
    tab = _dev(RC.standard((n_next, d), seed + 2, 1.0)) if case.next_idx[cell] else None
    return up, tab, nxt


def _bwd_call(be, case, saved_all, row0, ops, grads):
    d, v = case.d, case.variant
    gw = 3 * d if v == RC.TORCH else d
    outs = [dict(dgi=_nan(n + GUARD, gw), dgh=_nan(n + GUARD, 3 * d), decv=_nan(n + GUARD), d_prev=_nan(n + GUARD, d)) for n in case.ns]
    if case.entry == "cell_bwd":
        n, (up, tab, nxt), o = case.ns[0], grads[0], outs[0]
        be.gru_cell_bwd(saved_all, row0[0], n, up, tab, nxt, ops[0]["dt"], LAM, ops[0]["w_hh"], v, o["dgi"][:n], o["dgh"][:n], o["decv"][:n], o["d_prev"][:n])
    else:
        cells = [dict(row0=r0, n=n, dh_up=up, d_prev_next=tab, next_idx=nxt, dt=op["dt"], w_hh=op["w_hh"], dgi=o["dgi"][:n], dgh=o["dgh"][:n],
                      decv=o["decv"][:n], d_prev=o["d_prev"][:n], no_prev=np_)
                 for r0, n, (up, tab, nxt), op, o, np_ in zip(row0, case.ns, grads, ops, outs, case.no_prev)]
        be.gru_cell_bwd_multi(cells, LAM, v, saved_all)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("case", RC.GATES, ids=[c.id for c in RC.GATES])
def test_gate_gradient_route(case, hip_backend):
    """dgi, dgh: every element within 16 * 2^-24 of the same formula on absolute values (gates64(absolute=True)): the longest
    expression, dr_pre, takes 8 roundings in k_gru_bwd_gates, doubled for contraction; the saved planes are the GPU's own, cast to
    fp64, so only this kernel's arithmetic is judged.  decv: the bar of hdec.  d_prev: 1e-6 (sum |dgh||W_hh| + |g z|) around
    ((dgh as the GPU wrote it) . W_hh + g z) dec.  A no_prev cell: d_prev holds the gate kernel's seed g z (include/temp_amd.h:
    TempGruCellBwd.no_prev) -- one sum and one product in fp32: 4 * 2^-24 |g||z|."""
    be = hip_backend
    d, v = case.d, case.variant
    saved_all, row0, ops = _saved_planes(v, d, case.ns, case.no_prev)
    grads = [_bwd_operands(case, cell) for cell in range(len(case.ns))]
    lpr = RC.gates_lpr(d)
    Ms = [0 if np_ else n for n, np_ in zip(case.ns, case.no_prev)]
    want_gemm = RC.panel_launches(Ms, d, 3 * d, distinct_b=True)
    want_names = ["k_gru_bwd_gates"] + ["k_gemm_panel<gru_dprev>"] * sum(want_gemm.values())
    before = saved_all.clone()
    with Routes() as rt:
        outs = _bwd_call(be, case, saved_all, row0, ops, grads)
    outs2, names = _traced(lambda: _bwd_call(be, case, saved_all, row0, ops, grads))
    print("%s: gru %s gemm %s trace %s" % (case.id, sorted(rt.gru.items()), sorted(rt.gemm.items()), names))
    assert rt.gru == {"gates_lpr%d" % lpr: 1} and rt.gemm == want_gemm, "launched %s %s, the case pins lpr %d, %s" % (rt.gru, rt.gemm, lpr, want_gemm)
    assert names == want_names, (names, want_names)
    assert _same_bits(before, saved_all), "the backward wrote into the saved planes"
    gate_route = next(r for r in case.routes if r.startswith("gates_lpr"))
    for cell, (n, r0, o, o2, (up, tab, nxt), op) in enumerate(zip(case.ns, row0, outs, outs2, grads, ops)):
        what = "%s cell %d " % (case.id, cell)
        for k in o:
            assert _same_bits(o[k], o2[k]), what + k + ": two calls gave different bits"
            assert _all_nan_bits(o[k][n:]), what + k + ": guard rows were written"
        if n == 0:
            continue
        saved = saved_all[:, r0:r0 + n]
        dgi, dgh, dec, gz = RC.gates64(v, saved, up, tab, nxt, op["dt"], LAM, None)
        a_dgi, a_dgh, _, a_gz = RC.gates64(v, saved, up, tab, nxt, op["dt"], LAM, None, absolute=True)
        _note(gate_route, "dgi / 16 eps |formula|", _within(o["dgi"][:n], dgi, 16 * EPS * a_dgi, what + "dgi"))
        _note(gate_route, "dgh / 16 eps |formula|", _within(o["dgh"][:n], dgh, 16 * EPS * a_dgh, what + "dgh"))
        _note(gate_route, "decv / 1e-6", _within(o["decv"][:n], dec, 1e-6 * dec, what + "decv"))
        if case.no_prev[cell]:
            _note("no_prev", "d_prev / 4 eps |g||z|", _within(o["d_prev"][:n], gz, 4 * EPS * a_gz, what + "d_prev of a no_prev cell (the seed g z)"))
            continue
        want = RC.d_prev64(o["dgh"][:n], op["w_hh"], gz, dec)
        bar = 1e-6 * RC.d_prev64(o["dgh"][:n], op["w_hh"], gz, dec, absolute=True)
        _note("d_prev %s" % (sorted(want_gemm) or [("none", 0)])[0][0], "/ 1e-6 (sum|dgh||W| + |gz|)", _within(o["d_prev"][:n], want, bar, what + "d_prev"))


# =====================================================================================================================
# weight gradients
# =====================================================================================================================
def _wgrad_operands(d, n, variant, data, seed, hdec_null=False):
    gw = 3 * d if variant == RC.TORCH else d
    if data == "integer":
        x, hdec = RC.pattern(n, d, 7, 11, seed % 5), RC.pattern(n, d, 11, 7, 3)
        dgi, dgh, w_ih = RC.pattern(n, gw, 3, 5, 1), RC.pattern(n, 3 * d, 5, 3, 2), RC.pattern(gw, d, 3, 7, 4)
    else:
        x, hdec = RC.wide((n, d), seed + 1, 0.5), RC.wide((n, d), seed + 2, 0.5)
        dgi, dgh = RC.wide_rows((n, gw), seed + 3), RC.wide_rows((n, 3 * d), seed + 4)
        w_ih = RC.gru_weights(d, variant, seed + 5)[0]
    return _dev(x), None if hdec_null else _dev(hdec), _dev(dgi), _dev(dgh), _dev(w_ih)


def _tn_names(M, Ka, Nb):
    if RC.tn_bx(M, Ka, Nb):
        return ["k_gemm_tn_bx8" if Ka > 256 else "k_gemm_tn_bx", "k_reduce_slices"]
    return ["k_gemm_tn", "k_reduce_slices"]


def _wgrad_expect(n, d, variant, hdec_null, dx_null):
    """-> (gemm routes, trace names, bars per output (d_x, d_w_ih, d_w_hh, d_b_ih, d_b_hh)) of one temp_gru_weight_grads"""
    gw = 3 * d if variant == RC.TORCH else d
    dx = {} if dx_null else RC.panel_launches((n,), d, gw)
    gemm = RC.merge(dx, RC.tn_launches(n, gw, d), {} if hdec_null else RC.tn_launches(n, 3 * d, d))
    names = ["k_gemm_panel<gru_dx>"] * sum(dx.values()) + _tn_names(n, gw, d)
    names += ["k_colsum_part", "k_reduce_slices"] if hdec_null else _tn_names(n, 3 * d, d)
    fuse = d % 32 != 0
    if not fuse:
        names += ["k_colsum_part", "k_reduce_slices"] * (1 if hdec_null else 2)
    fp32 = lambda route: route in ("panel", "wres", "wres_split")
    b_dx = 1e-6 if all(fp32(r) for r, _ in dx) else 2e-6
    b_ih = 2e-6 if RC.tn_bx(n, gw, d) else 1e-6
    b_hh = 2e-6 if (not hdec_null and RC.tn_bx(n, 3 * d, d)) else 1e-6
    return gemm, names, (b_dx, b_ih, b_hh, b_ih if fuse else 1e-6, b_hh if fuse else 1e-6)


def _check_wgrad(what, route, got, ops, bars, data, hdec_null):
    x, hdec, dgi, dgh, w_ih = ops
    want = RC.weight_grads64(x, hdec, dgi, dgh, w_ih)
    scale = RC.weight_grads64(x, hdec, dgi, dgh, w_ih, absolute=True)
    for name, g, w, s, bar in zip(("d_x", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh"), got, want, scale, bars):
        if g is None:
            continue
        if data == "integer":
            assert float(w.abs().max()) < 2 ** 24
            _exact(g, w, "%s %s on integer operands" % (what, name))
        else:
            _note(route, "%s / %g sum|a||b|" % (name, bar), _within(g, w, bar * s, "%s %s" % (what, name)))
    if hdec_null:
        assert bool((got[2] == 0).all()), what + " d_w_hh is not exactly 0 without hdec"


@pytest.mark.parametrize("case", RC.WGRAD, ids=[c.id for c in RC.WGRAD])
def test_weight_gradient_route(case, hip_backend):
    """Every product within 1e-6 of sum |a||b| where the counters show the fp32 kernels, 2e-6 where the split-operand kernels ran
    (the bars of tests/test_gpu_gemm_routes.py and tests/test_gpu_gate_grads.py); a bias gradient that rides along as the ones
    column of its product takes that product's bar, one that k_colsum_part sums the fp32 bar.  Exact on integer operands."""
    be = hip_backend
    n, d, v = case.ns[0], case.d, case.variant
    want_gemm, want_names, bars = _wgrad_expect(n, d, v, case.hdec_null, case.dx_null)
    route = "+".join(sorted(case.routes)) + (" n=%d" % n)
    for data in ("wide", "integer"):
        ops = _wgrad_operands(d, n, v, data, 100 + d, case.hdec_null)
        x, hdec, dgi, dgh, w_ih = ops

        def call():
            dxb = None if case.dx_null else _nan(n + GUARD, d)
            res = be.gru_weight_grads(x, hdec, dgi, dgh, w_ih, v, None if dxb is None else dxb[:n])
            torch.cuda.synchronize()
            return dxb, res
        with Routes() as rt:
            dxb, res = call()
        (dxb2, res2), names = _traced(call)
        print("%s %s: gemm %s trace %s" % (case.id, data, sorted(rt.gemm.items()), names))
        assert rt.gru == {} and rt.gemm == want_gemm, "launched %s %s, the case pins %s" % (rt.gru, rt.gemm, want_gemm)
        assert names == want_names, (names, want_names)
        assert all(_same_bits(a, b) for a, b in zip(res, res2)), "two calls gave different bits"
        if dxb is not None:
            assert _same_bits(dxb, dxb2) and _all_nan_bits(dxb[n:]), "d_x: different bits, or guard rows written"
        _check_wgrad(case.id + " " + data, route, (None if dxb is None else dxb[:n],) + tuple(res), ops, bars, data, case.hdec_null)


@pytest.mark.parametrize("case", RC.WGRAD_MULTI, ids=[c.id for c in RC.WGRAD_MULTI])
def test_weight_gradient_multi_route(case, hip_backend):
    """temp_gru_weight_grads_multi: taken exactly where the library's workspace query says so (and the case table agrees); the
    gradients within the split-operand bar of fp64, d_x bit-identical to the per-GRU call where both pick the same kernel
    (tests/test_gpu_parity_r2.py: test_gru_weight_grads_multi_gpu); refused: None, nothing launched."""
    be, lib = hip_backend, _lib.load()
    d, ns, k = case.d, case.ns, len(case.ns)
    taken = "multi_taken" in case.routes
    assert (lib.temp_gru_weight_grads_multi_workspace(k, (ctypes.c_int * k)(*ns), d, _lib.GRU_TORCH) != 0) == taken
    ops = [_wgrad_operands(d, n, RC.TORCH, "wide", 300 + 10 * i + d) for i, n in enumerate(ns)]

    def call():
        dxs = [_nan(n + GUARD, d) for n in ns]
        res = be.gru_weight_grads_multi([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops], [o[3] for o in ops], [o[4] for o in ops],
                                        _lib.GRU_TORCH, [b[:n] for b, n in zip(dxs, ns)])
        torch.cuda.synchronize()
        return dxs, res
    with Routes() as rt:
        dxs, res = call()
    (dxs2, res2), names = _traced(call)
    print("%s: gemm %s trace %s" % (case.id, sorted(rt.gemm.items()), names))
    if not taken:
        assert res is None and res2 is None and rt.gemm == {} and rt.gru == {} and names == []
        assert all(_all_nan_bits(b) for b in dxs)
        return
    want_gemm = RC.panel_launches(ns, d, 3 * d, distinct_b=True)
    assert rt.gru == {} and rt.gemm == want_gemm, "launched %s, the case pins %s" % (rt.gemm, want_gemm)
    # one weight-gradient launch, one reduction; the d_x launch of 37 003 rows with K = 600 takes its own key pass and weight pack
    assert names == ["k_gemm_tn_bx8", "k_reduce_slices", "k_absmax_keys", "k_bx_pack", "k_gemm_panel<gru_dx>"], names
    same_kernel = min(ns) >= 16384 or sum(ns) < 16384
    for i, (n, o) in enumerate(zip(ns, ops)):
        assert _all_nan_bits(dxs[i][n:]) and _same_bits(dxs[i], dxs2[i]) and all(_same_bits(a, b) for a, b in zip(res[i], res2[i]))
        _check_wgrad("%s GRU %d" % (case.id, i), "multi_taken", (dxs[i][:n],) + tuple(res[i]), o, (2e-6,) * 5, "wide", False)
        dx1 = _nan(n, d)
        one = be.gru_weight_grads(o[0], o[1], o[2], o[3], o[4], _lib.GRU_TORCH, dx1)
        torch.cuda.synchronize()
        if same_kernel:
            assert torch.equal(dx1, dxs[i][:n]), "d_x: the same kernel on the same rows"
        _check_wgrad("%s GRU %d, per-GRU call" % (case.id, i), "per-GRU n=%d" % n, (dx1,) + tuple(one), o, (2e-6,) * 5, "wide", False)


# =====================================================================================================================
# the learnable decay's gradient (temp_gru_bwd with decay_wb)
# =====================================================================================================================
@pytest.mark.parametrize("case", RC.DECAY, ids=[c.id for c in RC.DECAY])
def test_decay_gradient_route(case, hip_backend):
    """d_decay_wb of temp_gru_bwd against the fp64 cell (forward64 -> gates64 -> d_prev64 -> decay_wb_grads64) at the bars of
    check_decay_grads in tests/test_gpu_chain_learnable_decay.py: 1e-4 |want| + 2e-5 (the absolute sum of the per-row terms).
    Every row clamped: both gradients are exactly 0."""
    be = hip_backend
    n, d, v = case.ns[0], case.d, case.variant
    fc = RC.fwd_case("gru_fwd", v, d, n, prev_idx=True, decay=case.decay)
    o = {k: _dev(t) for k, t in RC.forward_operands(fc, 0, "standard").items()}
    wb = _wb(case)
    wb_dev = torch.tensor(case.decay, dtype=torch.float32, device=DEV)
    arg = wb[0] * o["dt"].double() + wb[1]
    clamped = case.decay == RC.WB_CLAMPED
    assert bool((arg < 0).all()) if clamped else bool((arg > 0).any() and (arg < 0).any() and not (arg == 0).any())
    d_h = _dev(RC.standard((n, d), 77 + d, 1.0))
    h, saved = be.gru_fwd(o["x"], o["prev"], o["prev_idx"], o["dt"], LAM, wb_dev, o["w_ih"], o["w_hh"], o["b_ih"], o["b_hh"], v)

    def call():
        res = be.gru_bwd(o["x"], o["prev"], o["prev_idx"], o["dt"], LAM, wb_dev, o["w_ih"], o["w_hh"], saved, d_h, v)
        torch.cuda.synchronize()
        return res
    with Routes() as rt:
        res = call()
    res2, names = _traced(call)
    dprev_gemm = RC.panel_launches((n,), d, 3 * d)
    wg_gemm, wg_names, _ = _wgrad_expect(n, d, v, False, False)
    want_names = ["k_gru_bwd_gates"] + ["k_gemm_panel<gru_dprev>"] * sum(dprev_gemm.values()) + wg_names + ["k_decay_grad"]
    print("%s: gru %s gemm %s trace %s" % (case.id, sorted(rt.gru.items()), sorted(rt.gemm.items()), names))
    assert rt.gru == {"gates_lpr%d" % RC.gates_lpr(d): 1} and rt.gemm == RC.merge(dprev_gemm, wg_gemm)
    assert names == want_names, (names, want_names)
    assert all(_same_bits(a, b) for a, b in zip(res, res2)), "two calls gave different bits"
    ref = RC.forward64(v, o["x"], None, o["prev"], o["prev_idx"], o["dt"], LAM, wb, o["w_ih"], o["w_hh"], o["b_ih"], o["b_hh"])
    dgi, dgh, dec, gz = RC.gates64(v, torch.stack(ref[1:]), d_h, None, None, o["dt"], LAM, wb)
    d_prev = RC.d_prev64(dgh, o["w_hh"], gz, dec)
    d_w, d_b, t_w, t_b = [float(t) for t in RC.decay_wb_grads64(d_prev, o["prev"], o["prev_idx"], o["dt"], wb)]
    got_w, got_b = float(res[6][0]), float(res[6][1])
    print("%s: d_w %.8e (fp64 %.8e, error %.2e of %.2e)  d_b %.8e (fp64 %.8e, error %.2e of %.2e)" % (
        case.id, got_w, d_w, abs(got_w - d_w), t_w, got_b, d_b, abs(got_b - d_b), t_b))
    if clamped:
        assert got_w == 0.0 and got_b == 0.0 and d_w == 0.0 and d_b == 0.0
        return
    assert t_w > 0 and t_b > 0
    route = next(iter(case.routes))
    _note(route, "d_w error / absolute sum of the row terms", abs(got_w - d_w) / t_w)
    _note(route, "d_b error / absolute sum of the row terms", abs(got_b - d_b) / t_b)
    assert abs(got_w - d_w) <= 1e-4 * abs(d_w) + 2e-5 * t_w and abs(got_b - d_b) <= 1e-4 * abs(d_b) + 2e-5 * t_b


# =====================================================================================================================
# end to end: gru_chain on the per-position kernels
# =====================================================================================================================
@pytest.mark.parametrize("d", [36, 208, 260])
def test_per_position_chain_vs_float64_loop(d):
    """gru_chain with CHAIN_KERNELS = False (forward and backward on the kernels above) against the float64 loop of
    tests/test_gpu_chain_learnable_decay.py, at its bars.  d = 36: the d % 8 == 4 routes; 208: the hoisted streaming kernel and
    64 lanes per row; 260: two passes of the gate-gradient lanes.  No chain kernel may run."""
    from tests.test_gpu_chain_learnable_decay import _x, check_states_and_grads, loop_reference, loss_weights, run_chain
    prog, n_x = random_program(d + 1)
    assert any(it.n == 0 for it in prog.inst) and any(it.prev >= 0 and it.n and (it.prev_idx < 0).any() for it in prog.inst)
    rnns = make_rnns(2, d, False, 5)
    x = _x(n_x, d)
    wts = loss_weights(prog, None, d)
    ref = loop_reference(prog, x, rnns, None, False, None, wts)
    old = GCH.CHAIN_KERNELS
    GCH.CHAIN_KERNELS = False
    try:
        with Routes() as rt:
            got, names = _traced(lambda: run_chain(prog, x, rnns, DEV, False, None, wts), cap=4096)
    finally:
        GCH.CHAIN_KERNELS = old
    print("d = %d: gru %s gemm %s" % (d, sorted(rt.gru.items()), sorted(rt.gemm.items())))
    assert not [nm for nm in names if nm.startswith("k_gru_chain")], sorted(set(names))
    assert {"k_gru_fwd", "k_gru_bwd_gates", "k_gemm_panel<gru_dprev>"} <= set(names), sorted(set(names))
    assert rt.gru.get("fwd_stream_hoisted", 0) > 0 and rt.gru.get("fwd_zero", 0) > 0 and rt.gru.get("gates_lpr%d" % RC.gates_lpr(d), 0) > 0
    assert set(rt.gru) == {"fwd_stream_hoisted", "fwd_zero", "gates_lpr%d" % RC.gates_lpr(d)}, rt.gru
    check_states_and_grads(got, ref, False, "float64 loop, per-position kernels (d = %d)" % d)
