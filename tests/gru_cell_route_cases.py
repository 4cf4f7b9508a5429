"""Cases that pin every route of the per-position GRU cell kernels (temp_amd/csrc/gru_kernels.hip: launch_gru_fwd_batch,
temp_gru_cell_fwd_multi, launch_gru_gates_batch, gru_weight_grads, temp_gru_weight_grads_multi, k_decay_grad), an fp64 restatement
of the cell stage by stage, and the data recipes -- shared by tests/test_gru_cell_route_cases_cpu.py (the restatement against
oracle.temp_oracle, the coverage of the route set) and tests/test_gpu_gru_cell_routes.py (the kernels against fp64).  Importable
without a GPU: plain torch, every function works on the device of its operands.

A case names its entry point (the HipBackend method), the cell variant, d, the rows of every cell of the call, which optional
operands are NULL, and `routes`: the routes it must take, from a restatement of the dispatch predicates (fwd_route, gates_routes,
wgrad_routes, multi_taken below; k_decay_grad's single block strides from 256 rows).  What the dense-product counters (temp_gemm_route_launches) must then show is
restated from the planners as well: panel_launches, tn_launches.

RESULTS (MI355X), the largest error per route against the fp64 reference, every data recipe, all elements:
Forward, per route and variant (hdec as a relative error; hn as a fraction of sum |hdec||W_hn| + |b_hn|; r, z, n, h as a
fraction of their bar: standard data at rtol / atol 1e-5 / 2e-6 (nn.GRU) and 1e-4 / 2e-5 (type-1), the other recipes with the
propagated product error added):
    route                  hdec      hn        r / z / n / h standard      r / z / n / h wide, saturated, integer
    wres/torch             1.07e-07  3.12e-07  0.021 / 0.029 / 0.093 / 0.073      0.037 / 0.032 / 0.072 / 0.047
    wres/type1             1.07e-07  3.76e-07  0.003 / 0.002 / 0.009 / 0.007      0.005 / 0.004 / 0.021 / 0.006
    stream_hoisted/torch   1.06e-07  3.03e-07  0.033 / 0.026 / 0.129 / 0.093      0.043 / 0.038 / 0.088 / 0.043
    stream_hoisted/type1   1.06e-07  3.13e-07  0.003 / 0.003 / 0.011 / 0.009      0.005 / 0.005 / 0.023 / 0.007
    stream_fused/torch     1.06e-07  3.00e-07  0.050 / 0.052 / 0.166 / 0.142      0.066 / 0.067 / 0.090 / 0.057
    stream_fused/type1     1.06e-07  3.13e-07  0.003 / 0.003 / 0.016 / 0.013      0.005 / 0.005 / 0.026 / 0.009
    zero/torch             0.00e+00  0.00e+00  0.010 / 0.010 / 0.036 / 0.032      0.011 / 0.010 / 0.034 / 0.015
    zero/type1             0.00e+00  0.00e+00  0.001 / 0.001 / 0.004 / 0.003      0.001 / 0.001 / 0.004 / 0.002
Gate gradients (dgi, dgh as a multiple of 2^-24 times the formula on absolute values, bar 16; decv relative):
    gates_lpr8/once        dgi 1.50  dgh 1.39  decv 4.73e-08
    gates_lpr8/stride      dgi 2.28  dgh 2.28  decv 4.73e-08
    gates_lpr16/once       dgi 1.44  dgh 1.44  decv 4.73e-08
    gates_lpr16/stride     dgi 2.14  dgh 2.14  decv 4.73e-08
    gates_lpr32/once       dgi 1.71  dgh 1.71  decv 4.73e-08
    gates_lpr32/stride     dgi 1.97  dgh 1.97  decv 4.73e-08
    gates_lpr64/once       dgi 1.88  dgh 1.88  decv 4.73e-08
    gates_lpr64/stride     dgi 2.06  dgh 2.06  decv 4.73e-08
    (gates/two_pass, d = 260, is part of gates_lpr64/once)
    d_prev as a fraction of sum |dgh||W_hh| + |g z|: panel 2.07e-07, wres 2.20e-07; a no_prev cell's seed g z: 0.97 x 2^-24 |g||z|
Weight gradients, wide data, as a fraction of sum |a||b| (integer data: exact everywhere):
    bias_fused  n = 37     d_x 2.29e-07  d_w_ih 3.14e-07  d_w_hh 4.19e-07  d_b_ih 1.60e-07  d_b_hh 2.29e-07
    bias_fused  n = 4100   d_x 3.33e-07  d_w_ih 2.16e-07  d_w_hh 1.97e-07  d_b_ih 3.87e-08  d_b_hh 4.87e-08
    bias_colsum n = 37     d_x 1.54e-07  d_w_ih 3.67e-07  d_w_hh 4.22e-07  d_b_ih 1.17e-07  d_b_hh 1.05e-07
    bias_colsum n = 4100   d_x 3.65e-07  d_w_ih 2.11e-07  d_w_hh 4.64e-07  d_b_ih 6.17e-08  d_b_hh 8.65e-08
    multi_taken            d_x 2.14e-07  d_w_ih 2.98e-07  d_w_hh 1.86e-07  d_b_ih 2.79e-08  d_b_hh 2.89e-08
    per-GRU n = 20000      d_x 1.81e-07  d_w_ih 1.13e-07  d_w_hh 9.29e-08  d_b_ih 1.81e-08  d_b_hh 2.28e-08
    (hdec_null: d_w_hh exactly 0; dx_null: no d_x; the n = 4100 rows of bias_fused at d = 200 run the split-operand kernels)
Decay gradient, error as a fraction of the absolute sum of the per-row terms (bar 2e-5 plus 1e-4 relative): below 256 rows
    d_w 1.0e-08  d_b 1.7e-08; above  d_w 9.6e-11  d_b 5.3e-09; every row clamped: exactly 0.
gru_chain with CHAIN_KERNELS = False against the float64 loop (absolute): d = 36 states 1.4e-07 d_x 3.3e-06 parameters 3.5e-05;
    d = 208 states 3.4e-07 d_x 7.1e-06 parameters 6.3e-05; d = 260 states 3.4e-07 d_x 6.9e-06 parameters 4.2e-05.
"""
import collections
import math

import torch

TORCH, TYPE1 = 0, 1                      # temp_amd._lib.GRU_TORCH / GRU_TYPE1
LAM = 0.1
WB = (0.3, -0.7)                         # dt in 0..8: w dt + b <= 0 for dt <= 2, active above, never 0
WB_CLAMPED = (-0.25, -0.1)               # w dt + b < 0 on every row
VNAME = {TORCH: "torch", TYPE1: "type1"}

# include/temp_amd.h: TEMP_GRU_*
GRU_ROUTES = ("fwd_wres", "fwd_stream_hoisted", "fwd_stream_fused", "fwd_zero", "gates_lpr8", "gates_lpr16", "gates_lpr32", "gates_lpr64")


def f32(x):
    """the value as the kernel receives it: rounded to fp32"""
    return float(torch.tensor(x, dtype=torch.float32))


# =====================================================================================================================
# fp64 restatement of the cell: same operands as the C ABI (include/temp_amd.h), one function per stage
# =====================================================================================================================
def decay64(dt, lam, wb):
    """[n] decay factors: exp(-dt lam), or exp(-max(0, w dt + b)) with wb = (w, b)"""
    dt = dt.double().view(-1)
    if wb is not None:
        return torch.exp(-torch.clamp(wb[0] * dt + wb[1], min=0.0))
    return torch.exp(-dt * lam)


def gather64(prev, prev_idx, n):
    """[n, d] previous rows (prev_idx None: rows in order, -1: the zero vector, prev None: all zero) and bool [n]: has a row"""
    if prev is None:
        raise ValueError("a zero-state cell has no previous rows: pass d")
    if prev_idx is None:
        return prev[:n].double(), torch.ones(n, dtype=torch.bool, device=prev.device)
    idx = prev_idx.long()
    has = idx >= 0
    return prev.double()[idx.clamp(min=0)] * has.view(-1, 1).double(), has


def forward64(variant, x, gi, prev, prev_idx, dt, lam, wb, w_ih, w_hh, b_ih, b_hh, absolute=False):
    """One cell -> (h, r, z, n, hn, hdec), the kernel's h_out and its five saved planes.  Either x (the input gates are computed
    here, temp_gru_fwd) or gi = x . W_ih^T + b_ih (hoisted, temp_gru_cell_fwd*); prev None: the zero state.
    absolute=True -> (S_r, S_z, S_n, S_hn): the sum of the absolute terms of every pre-activation (S_n without the r * hn term)."""
    n = (x if gi is None else gi).shape[0]
    d = w_hh.shape[1]
    w_hh, b_hh = w_hh.double(), b_hh.double()
    if prev is None:
        hdec = torch.zeros(n, d, dtype=torch.float64, device=w_hh.device)
    else:
        rows, _ = gather64(prev, prev_idx, n)
        hdec = rows * decay64(dt, lam, wb).view(-1, 1)
    if gi is None:
        gi = x.double() @ w_ih.double().t() + b_ih.double()
        gi_abs = x.double().abs() @ w_ih.double().abs().t() + b_ih.double().abs()
    else:
        gi = gi.double()
        gi_abs = gi.abs()
    gh = hdec @ w_hh.t() + b_hh
    gh_abs = hdec.abs() @ w_hh.abs().t() + b_hh.abs()
    hr, hz, hn = gh[:, :d], gh[:, d:2 * d], gh[:, 2 * d:]
    if variant == TORCH:
        r, z, i_n = torch.sigmoid(gi[:, :d] + hr), torch.sigmoid(gi[:, d:2 * d] + hz), gi[:, 2 * d:]
        s = (gi_abs[:, :d] + gh_abs[:, :d], gi_abs[:, d:2 * d] + gh_abs[:, d:2 * d], gi_abs[:, 2 * d:], gh_abs[:, 2 * d:])
    else:
        r, z, i_n = torch.sigmoid(hr), torch.sigmoid(hz), gi
        s = (gh_abs[:, :d], gh_abs[:, d:2 * d], gi_abs, gh_abs[:, 2 * d:])
    if absolute:
        return s
    nn_ = torch.tanh(i_n + r * hn)
    h = (1 - z) * nn_ + z * hdec if variant == TORCH else nn_ + z * (hdec - nn_)
    return h, r, z, nn_, hn, hdec


def gates64(variant, saved, dh_up, d_prev_next, next_idx, dt, lam, wb, absolute=False):
    """Gate gradients from GIVEN saved planes (r, z, n, hn, hdec: [5, n, d]) -> (dgi, dgh, decv, g z).
    g = dh_up (None: 0) + d_prev_next[next_idx] (None or -1: 0).  absolute=True: the same formulas with every operand replaced by
    its absolute value and every difference by a sum -- the scale of the rounding error of each output element."""
    r, z, nn_, hn, hd = [p.double() for p in saved]
    if absolute:
        r, z, nn_, hn, hd = r.abs(), z.abs(), nn_.abs(), hn.abs(), hd.abs()
    sub = (lambda a, b: a + b) if absolute else (lambda a, b: a - b)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    g = torch.zeros_like(r)
    if dh_up is not None:
        g = g + ab(dh_up.double())
    if next_idx is not None:
        idx = next_idx.long()
        g = g + ab(d_prev_next.double())[idx.clamp(min=0)] * (idx >= 0).view(-1, 1).double()
    dn = g * sub(1.0, z)
    dz = g * sub(hd, nn_)
    dn_pre = dn * sub(1.0, nn_ * nn_)
    dr_pre = dn_pre * hn * r * sub(1.0, r)
    dz_pre = dz * z * sub(1.0, z)
    dhn = dn_pre * r
    dgi = torch.cat([dr_pre, dz_pre, dn_pre], 1) if variant == TORCH else dn_pre
    dgh = torch.cat([dr_pre, dz_pre, dhn], 1)
    return dgi, dgh, decay64(dt, lam, wb), g * z


def d_prev64(dgh, w_hh, gz, dec, absolute=False):
    """d_prev = (dgh . W_hh + g z) * dec  (absolute=True: sum |dgh||W_hh| + |g z|, without the decay)"""
    if absolute:
        return dgh.double().abs() @ w_hh.double().abs() + gz.double().abs()
    return (dgh.double() @ w_hh.double() + gz.double()) * dec.double().view(-1, 1)


def weight_grads64(x, hdec, dgi, dgh, w_ih, absolute=False):
    """-> (d_x, d_W_ih, d_W_hh, d_b_ih, d_b_hh) from given gate gradients; hdec None: every row started from the zero state."""
    ab = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    d = x.shape[1]
    d_w_hh = ab(dgh).t() @ ab(hdec) if hdec is not None else torch.zeros(3 * d, d, dtype=torch.float64, device=x.device)
    return ab(dgi) @ ab(w_ih), ab(dgi).t() @ ab(x), d_w_hh, ab(dgi).sum(0), ab(dgh).sum(0)


def decay_wb_grads64(d_prev, prev, prev_idx, dt, wb):
    """Learnable decay exp(-max(0, w dt + b)): -> (d_w, d_b, the absolute sums of their per-row terms).  A row contributes
    -<d_prev[row], prev[prev_idx[row]]> (times dt for d_w) when it has a previous row and w dt + b > 0."""
    rows, has = gather64(prev, prev_idx, d_prev.shape[0])
    dt = dt.double().view(-1)
    on = has & (wb[0] * dt + wb[1] > 0)
    s = -(d_prev.double() * rows).sum(1) * on.double()
    return (s * dt).sum(), s.sum(), (s * dt).abs().sum(), s.abs().sum()


# =====================================================================================================================
# dispatch predicates, restated (csrc/gru_kernels.hip, gemm_wres.hpp, gemm_panel.hpp, gemm_bx.hpp, gemm_hx.hpp, gemm_kernels.hip)
# =====================================================================================================================
def ceil_div(a, b):
    return -(-a // b)


def fwd_route(d, hoisted, zero=False):
    """launch_gru_fwd_batch / temp_gru_cell_fwd_multi (TEMP_OPT_GRU_STREAM = 0)"""
    if zero:
        return "zero"
    if not hoisted:
        return "stream_fused"
    ldk = ceil_div(d, 40) * 40 + 4
    if d % 8 == 0 and d >= 8 and 96 * ldk * 4 <= 80 * 1024:
        return "wres"
    return "stream_hoisted"


def gates_lpr(d):
    d4 = d // 4
    return 8 if d4 <= 8 else 16 if d4 <= 16 else 32 if d4 <= 32 else 64


def gates_routes(d, max_n):
    """launch_gru_gates_batch: lanes per row by d, the row loop strides once the grid is capped at 4096 blocks, a lane makes a
    second pass beyond 4 * 64 columns"""
    lpr = gates_lpr(d)
    out = {"gates_lpr%d/%s" % (lpr, "stride" if ceil_div(max_n, 256 // lpr) > 4096 else "once")}
    if d // 4 > 64:
        out.add("gates/two_pass")
    return out


def wgrad_routes(d, hdec_null, dx_null):
    out = {"bias_fused" if d % 32 else "bias_colsum"}
    if hdec_null:
        out.add("hdec_null")
    if dx_null:
        out.add("dx_null")
    return out


def tn_cfg(M, Ka, Nb):
    """gemm_kernels.hip: tn_cfg (TEMP_OPT_TN_SPLIT = 1) -> (wpb, split, kab, nt, nbb)"""
    kt = ceil_div(Ka, 32)
    wpb = 7 if ceil_div(kt, 7) * 7 - kt <= ceil_div(kt, 8) * 8 - kt else 8
    split = 1
    ntn = ceil_div(Nb, 32)
    if 5 <= ntn <= 7:
        wpb, split = 8, 2
    kab = ceil_div(Ka, (wpb // split) * 32)
    nt = 7 if ntn >= 5 else 4 if ntn >= 3 else 2 if ntn == 2 else 1
    return wpb, split, kab, nt, ceil_div(ntn, nt)


def tn_bx(M, Ka, Nb):
    """gemm_tn takes the split-operand weight-gradient kernels (not counted by temp_gemm_route_launches; traced as k_gemm_tn_bx8 for
    Ka > 256, else k_gemm_tn_bx)"""
    _, split, _, _, nbb = tn_cfg(M, Ka, Nb)
    return split == 2 and nbb == 1 and M >= 4096


def tn_launches(M, Ka, Nb):
    """{(route, width): 1} of one gemm_tn"""
    if tn_bx(M, Ka, Nb):
        return {}
    wpb, split, _, nt, _ = tn_cfg(M, Ka, Nb)
    if split == 2:
        return {("tn_split", 7): 1}
    return {("tn_w7" if wpb == 7 else "tn_w8", nt): 1}


def multi_taken(ns, d, variant):
    """temp_gru_weight_grads_multi_workspace != 0  (gemm_tn_multi_bias_supported of 2 count products [max_n, 3d]^T [max_n, d])"""
    if not 1 <= len(ns) <= 4 or variant != TORCH or min(ns) <= 0 or d % 4:
        return False
    _, split, _, _, nbb = tn_cfg(max(ns), 3 * d, d)
    kab8 = ceil_div(3 * d, 256)
    per = 32 // kab8
    units = 0 if kab8 > 32 else 8 * per + (8 * (32 - per * kab8)) // kab8
    return (split == 2 and nbb == 1 and max(ns) >= 4096 and 3 * d > 256 and d % 32 != 0 and 5 <= ceil_div(d, 32) <= 7 and units >= 2 * len(ns))


def wres_tps(N, K, rows):
    """gemm_wres.hpp: wres_plan -> tiles per slice, None when the shape streams"""
    if K % 4 or N % 4 or K < 8:
        return None
    ldk = ceil_div(K, 40) * 40 + 4
    nt = ceil_div(N, 32)
    tmax = 3
    while tmax > 1 and tmax * 32 * ldk * 4 > 80 * 1024:
        tmax -= 1
    if tmax * 32 * ldk * 4 > 80 * 1024:
        return None
    tmax = min(tmax, nt)
    best, best_cost = 1, 1e30
    for t in range(1, tmax + 1):
        ns = ceil_div(nt, t)
        cost = ns * t + 0.25 * ns
        if cost <= best_cost:
            best, best_cost = t, cost
    if ceil_div(nt, best) > 16 or rows < 4096:
        return None
    return best


def bx_group(N, max_m, rows):
    """gemm_bx.hpp: bx_plan -> G, tiles per column group"""
    nt = ceil_div(N, 32)
    row_tiles = ceil_div(max_m, 128)
    best, best_cost = 1, 1e30
    for w in range(1, min(nt, 7) + 1):
        blocks = max(ceil_div(rows, 128), row_tiles) * ceil_div(nt, w)
        rounds = 1.0 if blocks <= 512 else blocks / 512.0 + 0.5
        cost = rounds * (w + 0.5)
        if cost < best_cost * 0.999 or (cost <= best_cost * 1.001 and w > best):
            best, best_cost = w, cost
    return best


def panel_launches(Ms, N, K, distinct_b=False):
    """{(route, width): launches} of one launch_gemm_panel_multi with a plain epilogue, no row keys, default options"""
    rows = sum(m for m in Ms if m > 0)
    if rows <= 0:
        return {}
    if rows >= 16384 and K >= 16 and K % 4 == 0:
        keyless_ok = ceil_div(N, 32) >= 16 or K >= 400           # hx_supported without caller keys
        if K % 8 == 0:
            resident = 72 <= K <= 208 and N <= 1024
            if resident:
                return {("hxr" if keyless_ok else "bxr", 0): 1}
            return {("hxp" if keyless_ok else "bxp", bx_group(N, max(Ms), rows)): 1}
        if keyless_ok:
            return {("hxp", bx_group(N, max(Ms), rows)): 1}
    tps = wres_tps(N, K, rows)
    if tps is not None:
        split = distinct_b and len(Ms) > 1 and ceil_div(ceil_div(N, 32), tps) * len(Ms) <= 64
        return {("wres_split" if split else "wres", tps): 1}
    nt_all = ceil_div(N, 32)
    blocks = sum(ceil_div(max(m, 0), 128) for m in Ms)
    nt = 4
    while nt > 1 and blocks * ceil_div(nt_all, nt) < 384:
        nt >>= 1
    out = collections.Counter()
    full, rem = nt_all // nt, nt_all % nt
    if full:
        out[("panel", nt)] += 1
    if rem:
        out[("panel", rem)] += 1
    return dict(out)


def merge(*dicts):
    out = collections.Counter()
    for dct in dicts:
        out.update(dct)
    return dict(out)


# =====================================================================================================================
# data recipes: deterministic, CPU generators, fp32
# =====================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def standard(shape, seed, scale=0.5):
    return torch.randn(shape, generator=_gen(seed)) * scale


def gru_weights(d, variant, seed):
    """(w_ih, w_hh, b_ih, b_hh), uniform in +-1/sqrt(d) as nn.GRU initialises them"""
    g, k = _gen(seed), 1.0 / math.sqrt(d)
    u = lambda *s: (torch.rand(s, generator=g) * 2 - 1) * k
    gw = 3 * d if variant == TORCH else d
    return u(gw, d), u(3 * d, d), u(gw), u(3 * d)


def wide(shape, seed, scale=1.0):
    """the `_wide` recipe of tests/test_gpu_gemm_routes.py: magnitudes spread over e^+-1.5 per element"""
    g = _gen(seed)
    return torch.randn(shape, generator=g) * torch.exp(3.0 * torch.rand(shape, generator=g) - 1.5) * scale


def wide_rows(shape, seed, scale=0.1):
    """a dynamic range across ROWS, as the gate gradients of tests/test_gpu_gate_grads.py: test_gru_grads_g4_vs_fp64_gpu"""
    g = _gen(seed)
    return torch.randn(shape, generator=g) * scale * torch.exp(torch.randn(shape[0], 1, generator=g) * 1.5)


def saturate(t, seed, reach=40.0):
    """a third of the elements moved to +-reach (the rest untouched): pre-activations deep in both tails"""
    g = _gen(seed)
    pick = torch.rand(t.shape, generator=g) < (1.0 / 3.0)
    sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(pick, sign * reach, t)


def pattern(rows, cols, mr, mc, shift):
    """x[r][c] = ((mr r + mc c + shift) % 17) - 8: integers in [-8, 8] (`_pattern` of tests/test_gpu_gemm_routes.py)"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    c = torch.arange(cols, dtype=torch.int64)[None, :]
    return (((mr * r + mc * c + shift) % 17) - 8).float()


def dt_rows(n, seed):
    return torch.randint(0, 9, (n,), generator=_gen(seed)).float()


def index_rows(n, n_src, seed, none_share=0.3):
    """int32 [n]: rows of an n_src-row table, about `none_share` of them -1; the first entry -1 and the last the table's last row"""
    g = _gen(seed)
    idx = torch.randint(0, max(n_src, 1), (n,), generator=g)
    idx = torch.where(torch.rand(n, generator=g) < none_share, torch.full_like(idx, -1), idx)
    if n > 1:
        idx[0], idx[-1] = -1, n_src - 1
    return idx.int()


DATA = ("standard", "wide", "saturated", "integer")


def forward_operands(case, cell, data):
    """The operands of cell `cell` of a forward case -> dict(x | gi, prev, prev_idx, dt, w_ih, w_hh, b_ih, b_hh) on the CPU.
    prev has n + 7 rows when prev_idx is given (longer than the cell), n otherwise; None for a zero-state cell."""
    d, n, v = case.d, case.ns[cell], case.variant
    seed = 1000 * cell + d
    gw = 3 * d if v == TORCH else d
    hoisted = case.entry != "gru_fwd"
    has_idx = case.prev_idx[cell]
    n_prev = n + 7 if has_idx else n
    op = dict(prev_idx=index_rows(n, n_prev, seed + 1) if has_idx else None)
    if data == "integer":
        w_ih, w_hh = pattern(gw, d, 3, 5, cell), pattern(3 * d, d, 5, 3, 2 + cell)
        b_ih, b_hh = pattern(1, gw, 0, 7, 1)[0], pattern(1, 3 * d, 0, 11, 4)[0]
        x = pattern(n, d, 7, 11, 3 * cell)
        prev = pattern(n_prev, d, 11, 7, 5 + cell)
        op["dt"] = torch.zeros(n)                                   # the decay is exactly 1
    else:
        w_ih, w_hh, b_ih, b_hh = gru_weights(d, v, seed + 2)
        if data == "standard":
            x, prev = standard((n, d), seed + 3), standard((n_prev, d), seed + 4)
        else:
            x, prev = wide((n, d), seed + 3, 0.5), wide((n_prev, d), seed + 4, 0.5)
        op["dt"] = dt_rows(n, seed + 5)
    if data == "saturated":                                         # +-40 on a third of b_hh and of gi (of b_ih where gi is computed inside)
        b_hh = saturate(b_hh, seed + 6)
        if not hoisted:
            b_ih = saturate(b_ih, seed + 7)
    if hoisted:
        gi = (x.double() @ w_ih.double().t() + b_ih.double()).float()
        op["gi"] = saturate(gi, seed + 8) if data == "saturated" else gi
    else:
        op["x"] = x
    op.update(prev=None if case.zero[cell] else prev, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh)
    if case.zero[cell]:
        op["prev_idx"] = None
    return op


# =====================================================================================================================
# the case table
# =====================================================================================================================
Case = collections.namedtuple("Case", "entry variant d ns prev_idx zero decay dh_up next_idx no_prev hdec_null dx_null routes tag")
Case.id = property(lambda c: "%s-%s-d%d-n%s%s" % (c.entry, VNAME[c.variant], c.d, "_".join(str(n) for n in c.ns), c.tag))


def _tup(v, k):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * k


def fwd_case(entry, variant, d, ns, prev_idx=True, zero=False, decay=None):
    ns = _tup(ns, 1)
    k = len(ns)
    prev_idx, zero = _tup(prev_idx, k), _tup(zero, k)
    hoisted = entry != "gru_fwd"
    routes = set()
    if any(n > 0 and z for n, z in zip(ns, zero)):
        routes.add("zero/" + VNAME[variant])
    if any(n > 0 and not z for n, z in zip(ns, zero)):
        routes.add(fwd_route(d, hoisted) + "/" + VNAME[variant])
    tag = ("-idx" + "".join("01"[p] for p in prev_idx)) + ("-zero" + "".join("01"[z] for z in zero) if any(zero) else "") + ("-learnable" if decay else "")
    return Case(entry, variant, d, ns, prev_idx, zero, decay, None, None, None, None, None, frozenset(routes), tag)


def bwd_case(entry, variant, d, ns, dh_up=True, next_idx=True, no_prev=False):
    ns = _tup(ns, 1)
    k = len(ns)
    dh_up, next_idx, no_prev = _tup(dh_up, k), _tup(next_idx, k), _tup(no_prev, k)
    routes = gates_routes(d, max(ns))
    tag = "-up%s-next%s" % ("".join("01"[u] for u in dh_up), "".join("01"[u] for u in next_idx)) + ("-noprev" + "".join("01"[u] for u in no_prev) if any(no_prev) else "")
    return Case(entry, variant, d, ns, None, None, None, dh_up, next_idx, no_prev, None, None, frozenset(routes), tag)


def wgrad_case(variant, d, n, hdec_null=False, dx_null=False):
    tag = ("-hdec0" if hdec_null else "") + ("-dx0" if dx_null else "")
    return Case("weight_grads", variant, d, (n,), None, None, None, None, None, None, hdec_null, dx_null, frozenset(wgrad_routes(d, hdec_null, dx_null)), tag)


def multi_case(d, ns):
    taken = multi_taken(ns, d, TORCH)
    return Case("weight_grads_multi", TORCH, d, tuple(ns), None, None, None, None, None, None, False, False,
                frozenset({"multi_taken" if taken else "multi_refused"}), "")


def decay_case(d, n, wb):
    routes = {"decay_grad/%s" % ("above256" if n > 256 else "below256")}
    return Case("gru_bwd", TORCH, d, (n,), (True,), (False,), wb, None, None, None, None, None, frozenset(routes), "-clamped" if wb == WB_CLAMPED else "")


FORWARD = []
for _v in (TORCH, TYPE1):
    # hoisted gates: the resident kernel (d % 8 == 0 up to 200), the streaming kernel (d % 8 == 4, and from 208)
    for _d in (8, 36, 40, 100, 136, 200, 208, 260):
        FORWARD.append(fwd_case("cell_fwd_multi", _v, _d, (300, 0, 129, 1), prev_idx=(True, True, False, True)))
    for _d, _n, _p in ((8, 1, False), (200, 33, True), (36, 33, True), (260, 1, False), (136, 129, False)):
        FORWARD.append(fwd_case("cell_fwd", _v, _d, _n, prev_idx=_p))
    # batches that mix zero-state and carried cells
    FORWARD.append(fwd_case("cell_fwd_multi", _v, 40, (129, 33, 300, 5), prev_idx=(True, False, False, False), zero=(False, True, False, True)))
    FORWARD.append(fwd_case("cell_fwd_multi", _v, 36, (129, 33), prev_idx=(True, False), zero=(False, True)))
    # zero-state cells alone: past the grid cap (n d / 4 > 2048 * 256), and the smallest
    FORWARD.append(fwd_case("cell_fwd_multi", _v, 36, (65540,), prev_idx=False, zero=True))
    FORWARD.append(fwd_case("cell_fwd_multi", _v, 8, (5, 0), prev_idx=False, zero=True))
    # the input gates computed inside: d % 8 == 4, a partial last column tile together with a partial 40-wide K chunk
    for _d, _n, _p, _w in ((12, 1, False, None), (12, 300, True, WB), (36, 33, True, None), (36, 129, False, WB), (72, 129, True, None),
                           (72, 300, True, WB), (260, 33, True, WB), (260, 300, True, None)):
        FORWARD.append(fwd_case("gru_fwd", _v, _d, _n, prev_idx=_p, decay=_w))
FORWARD = tuple(FORWARD)

GATES = (
    # the row loop strides: more rows than 4096 blocks of 256 / LPR
    bwd_case("cell_bwd", TORCH, 4, 131080, dh_up=False),
    bwd_case("cell_bwd", TORCH, 36, 65540, dh_up=False),
    bwd_case("cell_bwd", TORCH, 68, 32770, dh_up=False),
    bwd_case("cell_bwd", TYPE1, 68, 32770, dh_up=False),
    bwd_case("cell_bwd", TORCH, 132, 16389, dh_up=False),
    # two passes of a lane
    bwd_case("cell_bwd", TORCH, 260, 37),
    bwd_case("cell_bwd", TYPE1, 260, 37),
) + tuple(
    bwd_case("cell_bwd", (TORCH, TYPE1)[(_i + _u + _x) % 2], _d, 70, dh_up=bool(_u), next_idx=bool(_x))
    for _i, _d in enumerate((32, 64, 128, 200)) for _u in (0, 1) for _x in (0, 1)
) + (
    bwd_case("cell_bwd_multi", TORCH, 32, (70, 0, 33, 5), dh_up=(True, True, False, True), next_idx=(True, False, True, False), no_prev=(False, False, True, False)),
    bwd_case("cell_bwd_multi", TYPE1, 64, (70, 33), dh_up=(False, True), next_idx=(True, True), no_prev=(True, False)),
    bwd_case("cell_bwd_multi", TORCH, 200, (300, 0, 129, 1), dh_up=(True, False, True, True), next_idx=(True, True, True, False), no_prev=(False, False, False, True)),
)

WGRAD = tuple(wgrad_case(TORCH, _d, _n) for _d in (36, 64, 128, 200, 260) for _n in (37, 4100)) + (
    wgrad_case(TYPE1, 36, 37), wgrad_case(TYPE1, 64, 4100), wgrad_case(TYPE1, 200, 4100),
    wgrad_case(TORCH, 200, 37, hdec_null=True), wgrad_case(TORCH, 64, 4100, hdec_null=True),
    wgrad_case(TORCH, 36, 4100, dx_null=True), wgrad_case(TORCH, 128, 37, dx_null=True),
)
WGRAD_MULTI = (multi_case(200, (20000, 17003)), multi_case(200, (900, 700)), multi_case(128, (20000, 20000)))
DECAY = (decay_case(36, 200, WB), decay_case(200, 700, WB), decay_case(36, 200, WB_CLAMPED))

ALL = FORWARD + GATES + WGRAD + WGRAD_MULTI + DECAY
assert len({c.id for c in ALL}) == len(ALL), "case ids must be unique"

# every route name the restated predicates can produce: a new name here without a case fails tests/test_gru_cell_route_cases_cpu.py
ROUTE_SET = frozenset(
    {"%s/%s" % (r, v) for r in ("wres", "stream_hoisted", "stream_fused", "zero") for v in VNAME.values()}
    | {"gates_lpr%d/%s" % (l, s) for l in (8, 16, 32, 64) for s in ("once", "stride")} | {"gates/two_pass"}
    | {"bias_fused", "bias_colsum", "hdec_null", "dx_null", "multi_taken", "multi_refused"}
    | {"decay_grad/below256", "decay_grad/above256"})
