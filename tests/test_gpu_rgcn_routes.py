"""Every route of the RGCN edge-kernel dispatcher (temp_amd/csrc/rgcn_kernels.hip: run_agg / launch_agg / run_dw / launch_fixup,
rgcn_tile.hpp) on the MI355X, each against the fp64 sum over the plain edge list.  The cases and what each must launch are in
tests/rgcn_route_cases.py; tests/test_rgcn_route_cases_cpu.py checks the host-side facts they rest on.

A case calls the C ABI directly.  loop_w = 0, no bias and no activation make the layer's output the edge kernels' result alone
(the epilogue adds +0): forward through temp_rgcn_fwd, d/dh through temp_rgcn_bwd_dh, d/dweight through temp_rgcn_bwd_weights.
Outputs are NaN-filled with 64 guard rows and the workspace holds NaN bit patterns before every call, so a partial slot that is
read without having been written, or a row that is left alone, shows.  Checked:
  * the launches the library counted (temp_rgcn_route_launches) are exactly the case's, "no fix-up launch" included;
  * guard rows keep their bits; rows without in-edges (forward) / out-edges (d/dh) and relation rows without edges are exactly 0;
  * exact data -- nnorm = 2^-(node % 3), patterned integers in [-4, 4] and [-2, 2], every partial sum below 2^24 sixteenths -- the
    result equals the fp64 value bit for bit, whatever the summation order;
  * wide data -- reals over three decades, the graph's own 1 / in-degree -- every element is finite, within 1e-6 of sum |t| and
    within k 2^-24 sum |t| (rgcn_route_cases.chain_k);
  * a second call gives the same bits; with h_ids into a table of 3 n rows (NaN in the rows nobody reads) the forward gives the bits
    of the gathered rows; for d <= 256 temp_rgcn_table_bwd's d_weight equals temp_rgcn_bwd_weights on the gathered rows bit for bit;
  * a quarter of the cases: the whole temp_rgcn_bwd with random loop weights, bias and ReLU against the fp64 layer."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import rgcn_route_cases as RC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
NAN = float("nan")
NAN_BITS = 0x7FC00000          # what torch.full(..., nan) writes
GUARD = 64
DEFAULTS = {"tile": 1, "scalar": 1, "debug": 0}


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be
    TB.set_backend(None)


@functools.lru_cache(maxsize=2)
def _graph(family, seed, members, R2, exact):
    case = RC.Case("", family, seed, members, 0, 0, 0, R2, {}, {}, {}, {}, (), False, False)
    snap = RC.build(case, exact)
    return snap, snap.device_graph(DEV, R2)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(rows, cols):
    return torch.full((rows + GUARD, cols), NAN, device=DEV)


def _poisoned(nbytes):
    """a workspace of at least nbytes whose every word is a NaN bit pattern"""
    return torch.full((int(nbytes) // 4 + 64,), NAN, device=DEV)


def _bits(t):
    return t.view(torch.int32)


def _guard_ok(buf, rows):
    return bool((_bits(buf[rows:]) == NAN_BITS).all())


def _table(lib):
    return [[lib.temp_rgcn_route_launches(r, s) for s in range(RC.S_CELLS)] for r in range(len(RC.ROUTES))]


def _delta(lib, before):
    after = _table(lib)
    return {(RC.ROUTES[r], s): after[r][s] - before[r][s] for r in range(len(RC.ROUTES)) for s in range(RC.S_CELLS) if after[r][s] != before[r][s]}


class Calls:
    """the three isolated entry points (and the whole backward) of one case on one device graph"""

    def __init__(self, lib, case, dg):
        self.lib, self.c, self.dg = lib, case, dg
        self.n = dg.n_nodes
        self.wrow = RC.shapes(case)[2]
        self.zero_lw = torch.zeros(case.d_in, case.d_out, device=DEV)

    def fwd(self, h, w, h_ids=None, lw=None, bias=None, act=_lib.ACT_NONE):
        c, g = self.c, self.dg.ref()
        out = _nan(self.n, c.d_out)
        ws = _poisoned(self.lib.temp_rgcn_fwd_workspace(g, c.d_out))
        rc = self.lib.temp_rgcn_fwd(g, _p(h), _p(h_ids), c.d_in, c.d_out, c.B, c.R2, _p(w), _p(self.zero_lw if lw is None else lw), _p(bias), act,
                                    _p(out), _p(ws), ws.numel() * 4, None, _stream())
        _lib.check(rc, "temp_rgcn_fwd")
        torch.cuda.synchronize()
        return out

    def _bwd_ws(self):
        c = self.c
        return _poisoned(self.lib.temp_rgcn_bwd_workspace(self.dg.ref(), c.d_in, c.d_out, c.B, c.R2))

    def dx(self, dz, w):
        c = self.c
        d_h, ws = _nan(self.n, c.d_in), self._bwd_ws()
        rc = self.lib.temp_rgcn_bwd_dh(self.dg.ref(), None, _p(dz), c.d_in, c.d_out, c.B, c.R2, _p(w), _p(self.zero_lw), _lib.ACT_NONE, _p(d_h), None, None,
                                       _p(ws), ws.numel() * 4, None, _stream())
        _lib.check(rc, "temp_rgcn_bwd_dh")
        torch.cuda.synchronize()
        return d_h

    def dw(self, h, dz):
        c = self.c
        d_w, d_loop, ws = _nan(c.R2, self.wrow), torch.empty(c.d_in, c.d_out, device=DEV), self._bwd_ws()
        rc = self.lib.temp_rgcn_bwd_weights(self.dg.ref(), _p(h), _p(dz), None, c.d_in, c.d_out, c.B, c.R2, 0, _p(d_w), _p(d_loop), None, _p(ws),
                                            ws.numel() * 4, _stream())
        _lib.check(rc, "temp_rgcn_bwd_weights")
        torch.cuda.synchronize()
        return d_w

    def table_dw(self, table, ids, dz, w):
        """d_weight of temp_rgcn_table_bwd: the weight-gradient kernels reading their x rows through x_ids"""
        c, g = self.c, self.dg.ref()
        n_table = table.shape[0]
        inv_ptr, inv_order = TF.gather_inverse(ids.cpu().numpy().astype(np.int64), n_table, DEV)
        d_table, d_w, d_loop = torch.empty(n_table, c.d_in, device=DEV), _nan(c.R2, self.wrow), torch.empty(c.d_in, c.d_out, device=DEV)
        ws = _poisoned(self.lib.temp_rgcn_table_bwd_workspace(g, n_table, c.d_in, c.d_out, c.B))
        rc = self.lib.temp_rgcn_table_bwd(g, _p(table), _p(ids), _p(inv_ptr), _p(inv_order), n_table, None, _p(dz), c.d_in, c.d_out, c.B, c.R2, _p(w),
                                          _p(self.zero_lw), 0, _lib.ACT_NONE, _p(d_table), _p(d_w), _p(d_loop), None, _p(ws), ws.numel() * 4, None, _stream())
        _lib.check(rc, "temp_rgcn_table_bwd")
        torch.cuda.synchronize()
        return d_w

    def whole_bwd(self, h, out, gy, w, lw):
        c = self.c
        d_h, d_w, d_loop, d_bias, ws = _nan(self.n, c.d_in), _nan(c.R2, self.wrow), _nan(c.d_in, c.d_out), _nan(1, c.d_out), self._bwd_ws()
        rc = self.lib.temp_rgcn_bwd(self.dg.ref(), _p(h), _p(out), _p(gy), c.d_in, c.d_out, c.B, c.R2, _p(w), _p(lw), 1, _lib.ACT_RELU, _p(d_h), _p(d_w),
                                    _p(d_loop), _p(d_bias), _p(ws), ws.numel() * 4, None, _stream())
        _lib.check(rc, "temp_rgcn_bwd")
        torch.cuda.synchronize()
        return d_h, d_w, d_loop, d_bias


def _bar1(got, ref, sabs):
    """(finite, worst |got - ref| / (1e-6 sum |t|))"""
    g = got.double()
    err = (g - ref).abs()
    r = torch.where(err <= 0, torch.zeros_like(err), err / (RC.BAR1 * sabs))
    return bool(torch.isfinite(g).all()), float(r.nan_to_num(nan=float("inf"), posinf=float("inf")).max())


def measure(case):
    """Run the case; -> report dict.  Nothing is asserted here (a script can print the figures of every case)."""
    lib = _lib.load()
    rep = {"problems": []}
    bad = rep["problems"].append
    prev = {k: lib.temp_set_option(RC.OPT[k], {**DEFAULTS, **case.opts}[k]) for k in DEFAULTS}
    try:
        # ---- wide data on the graph's own norms: counters, bars, repeatability, gathers
        snap, dg = _graph(case.family, case.seed, case.members, case.R2, False)
        n = snap.n
        run = Calls(lib, case, dg)
        h, dz, w = RC.operands(case, n, "wide", DEV)
        ref = RC.reference(case, snap, h, dz, w, DEV)
        got, launched = {}, {}
        for phase, call in (("fwd", lambda: run.fwd(h, w)), ("dx", lambda: run.dx(dz, w)), ("dw", lambda: run.dw(h, dz))):
            before = _table(lib)
            got[phase] = call()
            launched[phase] = _delta(lib, before)
            again = call()
            if not torch.equal(_bits(got[phase]), _bits(again)):
                bad("%s: two calls gave different bits" % phase)
        rep["launched"] = launched
        rows = {"fwd": n, "dx": n, "dw": case.R2}
        rep["ratios"] = {}
        for phase in ("fwd", "dx", "dw"):
            val, sabs, cnt = ref[phase]
            buf = got[phase]
            if not _guard_ok(buf, rows[phase]):
                bad("%s: guard rows were written" % phase)
            res = buf[:rows[phase]]
            if not bool((res[cnt == 0] == 0).all()):
                bad("%s: a row without edges is not exactly zero" % phase)
            finite, r1, r2 = RC.compare(case, phase, res, val, sabs, cnt)
            rep["ratios"][phase] = (r1, r2)
            if not finite:
                bad("%s: non-finite elements" % phase)
        ids = torch.randperm(3 * n, generator=torch.Generator().manual_seed(5))[:n].to(DEV).int()
        table = torch.full((3 * n, case.d_in), NAN, device=DEV)
        table[ids.long()] = h
        if not torch.equal(_bits(run.fwd(table, w, h_ids=ids)), _bits(got["fwd"])):
            bad("forward through h_ids differs from the forward on the gathered rows")
        if case.d_in <= 256 and case.d_out <= 256:
            if not torch.equal(_bits(run.table_dw(table, ids, dz, w)), _bits(got["dw"])):
                bad("d_weight of temp_rgcn_table_bwd differs from temp_rgcn_bwd_weights on the gathered rows")
        if case.whole:
            lw = RC._wide(torch, (case.d_in, case.d_out), 34, 0.1).to(DEV)
            bias = RC._wide(torch, (case.d_out,), 35, 0.5).to(DEV)
            out = run.fwd(h, w, lw=lw, bias=bias, act=_lib.ACT_RELU)
            h64, lw64 = h.double(), lw.double()
            pre = ref["fwd"][0] + h64 @ lw64 + bias.double()
            pre_abs = ref["fwd"][1] + h64.abs() @ lw64.abs() + bias.double().abs()
            w_rep = {"out": _bar1(out[:n], torch.relu(pre), pre_abs)}
            # (an element whose pre-activation is within its error of zero may land on either side of the ReLU: not counted)
            unsure = (pre.abs() <= RC.BAR1 * pre_abs) & ((out[:n].double() - torch.relu(pre)).abs() <= RC.BAR1 * pre_abs)
            gy = dz
            dzm = torch.where(out[:n] > 0, gy, torch.zeros_like(gy))
            r2 = RC.reference(case, snap, h, dzm, w, DEV)
            d_h, d_w, d_loop, d_bias = run.whole_bwd(h, out[:n].contiguous(), gy, w, lw)
            dzm64 = dzm.double()
            w_rep["d_h"] = _bar1(d_h[:n], r2["dx"][0] + dzm64 @ lw64.t(), r2["dx"][1] + dzm64.abs() @ lw64.abs().t())
            w_rep["d_weight"] = _bar1(d_w[:case.R2], r2["dw"][0], r2["dw"][1])
            w_rep["d_loop_w"] = _bar1(d_loop[:case.d_in], h64.t() @ dzm64, h64.abs().t() @ dzm64.abs())
            w_rep["d_bias"] = _bar1(d_bias[:1], dzm64.sum(0, keepdim=True), dzm64.abs().sum(0, keepdim=True))
            rep["whole"] = w_rep
            rep["whole_unsure"] = int(unsure.sum())
            for name, buf, r in (("d_h", d_h, n), ("d_weight", d_w, case.R2), ("d_loop_w", d_loop, case.d_in), ("d_bias", d_bias, 1)):
                if not _guard_ok(buf, r):
                    bad("whole backward: guard rows of %s were written" % name)
        del got, ref
        # ---- exact data: the fp64 value bit for bit
        snap, dg = _graph(case.family, case.seed, case.members, case.R2, True)
        run = Calls(lib, case, dg)
        h, dz, w = RC.operands(case, n, "exact", DEV)
        ref = RC.reference(case, snap, h, dz, w, DEV)
        rep["exact"] = {}
        for phase, buf in (("fwd", run.fwd(h, w)), ("dx", run.dx(dz, w)), ("dw", run.dw(h, dz))):
            val, sabs, _ = ref[phase]
            assert float(sabs.max()) * 16 < 2 ** 24, "the exact operands are not exact in fp32 here"
            rep["exact"][phase] = RC.first_difference(buf[:rows[phase]], val)
            if not _guard_ok(buf, rows[phase]):
                bad("%s (exact data): guard rows were written" % phase)
    finally:
        for k, v in prev.items():
            lib.temp_set_option(RC.OPT[k], v)
    return rep


def check(case, rep):
    for phase, want in (("fwd", case.fwd), ("dx", case.dx), ("dw", case.dw)):
        r1, r2 = rep["ratios"][phase]
        main = [r for r, _ in want if not r.startswith("fix")][0]
        print("rgcn-route %s %s %s: %.3f of the first bar, %.3f of the second; launched %s" % (case.id, phase, main, r1, r2, sorted(rep["launched"][phase].items())))
    if "whole" in rep:
        print("rgcn-route %s whole backward: %s (%d elements at the ReLU's edge)" % (case.id, {k: "%.3f" % v[1] for k, v in rep["whole"].items()}, rep["whole_unsure"]))
    for phase, want in (("fwd", case.fwd), ("dx", case.dx), ("dw", case.dw)):
        assert rep["launched"][phase] == want, "%s launched %s, the case pins %s" % (phase, sorted(rep["launched"][phase].items()), sorted(want.items()))
    assert not rep["problems"], "; ".join(rep["problems"])
    for phase in ("fwd", "dx", "dw"):
        assert rep["exact"][phase] is None, "%s, integer operands: %s" % (phase, rep["exact"][phase])
    for phase in ("fwd", "dx", "dw"):
        r1, r2 = rep["ratios"][phase]
        assert r1 <= 1.0, "%s: worst error %.3f of 1e-6 sum|t|" % (phase, r1)
        assert r2 <= 1.0, "%s: worst error %.3f of k 2^-24 sum|t|" % (phase, r2)
    for name, (finite, r1) in rep.get("whole", {}).items():
        assert finite and r1 <= 1.0, "whole backward, %s: worst error %.3f of 1e-6 sum|t| (finite: %s)" % (name, r1, finite)


@pytest.mark.parametrize("case", RC.ALL, ids=[c.id for c in RC.ALL])
def test_rgcn_route(case):
    check(case, measure(case))


def test_route_counter_bounds():
    lib = _lib.load()
    assert lib.temp_rgcn_route_launches(len(RC.ROUTES), 0) == -1 and lib.temp_rgcn_route_launches(0, RC.S_CELLS) == -1
    assert lib.temp_rgcn_route_launches(-1, 0) == -1 and lib.temp_rgcn_route_launches(0, -1) == -1
    assert lib.temp_rgcn_route_launches(0, 0) >= 0 and lib.temp_rgcn_route_launches(len(RC.ROUTES) - 1, RC.S_CELLS - 1) >= 0
