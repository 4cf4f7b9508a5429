"""Every route and template width of the dense-product dispatcher (temp_amd/csrc/gemm_wres.hpp: launch_gemm_panel_multi, behind
temp_linear / temp_linear_keys / temp_linear_t / temp_linear_multi) and of the fp32 weight-gradient kernel (temp_linear_tn) on the
MI355X, each against the full fp64 product.  The cases and what each must launch are in tests/gemm_route_cases.py.

Every case runs through the C ABI into NaN-filled outputs with a padded leading dimension and 64 guard rows, and checks
  * the launches the library counted (temp_gemm_route_launches) are exactly the case's, and temp_scratch_refused did not move;
  * padding columns and guard rows keep their bits; operands with padded leading dimensions carry NaN in the padding;
  * every element is finite and within 1e-6 of sum |a||b| of the fp64 product (all elements, nothing sampled);
  * a second call gives the same bits;
  * on integer operands in [-8, 8] (K <= 608: every partial sum below 2^24, and the bf16 / f16 pieces hold such values exactly
    because the f16 scales are powers of two) the result equals the integer product exactly.  The integer reference is the fp64
    product, which is itself exact here: all its partial sums are integers far below 2^53."""
import ctypes
import functools

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import gemm_route_cases as GC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
NAN = float("nan")
NAN_BITS = 0x7FC00000          # what torch.full(..., nan) writes
GUARD = 64
BAR = 1e-6


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be
    TB.set_backend(None)


@functools.lru_cache(maxsize=16)
def _wide_host(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp(3.0 * torch.rand(shape, generator=g) - 1.5) * scale


def _wide(shape, seed, scale):
    return _wide_host(tuple(shape), seed, scale).to(DEV)


def _pattern(rows, cols, mr, mc, shift):
    """x[r][c] = ((mr r + mc c + shift) % 17) - 8: integers in [-8, 8], so that a wrong element names its row, column and k-chunk."""
    r = torch.arange(rows, device=DEV, dtype=torch.int64)[:, None]
    c = torch.arange(cols, device=DEV, dtype=torch.int64)[None, :]
    return (((mr * r + mc * c + shift) % 17) - 8).float()


def _operands(case, data):
    """-> (a_list, b_list): the logical fp32 operands, a_i [M_i, K] and b_j [K, N] (for `tn`: a [M, Ka], b [M, Nb])."""
    if case.entry == "tn":
        M = case.Ms[0]
        if data == "wide":
            return [_wide((M, case.K), 21, 1.0)], [_wide((M, case.N), 22, 1.0)]
        return [_pattern(M, case.K, 7, 11, 0)], [_pattern(M, case.N, 3, 5, 0)]
    nb = max(case.bpat) + 1
    if data == "wide":
        return ([_wide((m, case.K), 11 + 7 * i, 1.0) for i, m in enumerate(case.Ms)],
                [_wide((case.K, case.N), 12 + 7 * j, 0.2) for j in range(nb)])
    return ([_pattern(m, case.K, 7, 11, 3 * i) for i, m in enumerate(case.Ms)],
            [_pattern(case.K, case.N, 3, 5, 2 * j) for j in range(nb)])


def _buf(x, ld):
    """x [r, c] stored with leading dimension ld >= c (at least one row, so that an empty operand still has an address); the padding
    holds NaN: a kernel that multiplies by it cannot pass."""
    r, c = x.shape
    if ld == c and r > 0:
        return x.contiguous()
    b = torch.full((max(r, 1), ld), NAN, device=DEV)
    b[:r, :c] = x
    return b


def _out(rows, cols, ld):
    return torch.full((rows + GUARD, ld), NAN, device=DEV)


def _bits(t):
    return t.view(torch.int32)


def _table(lib):
    return [[lib.temp_gemm_route_launches(r, w) for w in range(GC.WIDTHS)] for r in range(len(GC.ROUTES))]


def _delta(lib, before):
    after = _table(lib)
    return {(GC.ROUTES[r], w): after[r][w] - before[r][w] for r in range(len(GC.ROUTES)) for w in range(GC.WIDTHS) if after[r][w] != before[r][w]}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _row_keys(lib, a_buf, M, K, lda):
    """the magnitude keys of A's rows: temp_absmax_keys where it takes the width, else the same definition by torch"""
    if K <= 256:
        rk = torch.empty(M, dtype=torch.int32, device=DEV)
        _lib.check(lib.temp_absmax_keys(M, K, a_buf.data_ptr(), lda, rk.data_ptr(), None, _stream()), "temp_absmax_keys")
        return rk
    mx = a_buf[:M, :K].abs().max(dim=1).values.contiguous()
    return (mx.view(torch.int32) & 0x7FFFFFFF).contiguous()


def _call(lib, case, a_list, b_list):
    """One call of the case's entry point into fresh NaN-filled outputs -> per problem (buffer, (rows, cols) of the region the
    call may write, the product as a view [M or Ka, N or Nb] of that region)."""
    K, N, tb = case.K, case.N, int(case.trans_b)
    if case.entry == "tn":
        M, Ka, Nb = case.Ms[0], K, N
        lda, ldb, ldo = Ka + (4 if case.pad else 0), Nb + (4 if case.pad else 0), Nb + 4
        a, b, out = _buf(a_list[0], lda), _buf(b_list[0], ldb), _out(Ka, Nb, ldo)
        nb = lib.temp_linear_tn_workspace(M, Ka, Nb)
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        rc = lib.temp_linear_tn(M, Ka, Nb, a.data_ptr(), lda, b.data_ptr(), ldb, out.data_ptr(), ldo, ws.data_ptr(), nb, _stream())
        _lib.check(rc, "temp_linear_tn")
        res = [(out, (Ka, Nb), out[:Ka, :Nb])]
    else:
        width = K if tb else N
        lda, ldb, ldc = K + (4 if case.pad else 0), width + (8 if case.pad else 0), N + 4
        a_bufs = [_buf(a, lda) for a in a_list]
        b_bufs = [_buf(b.t() if tb else b, ldb) for b in b_list]
        outs = [_out(m, N, ldc) for m in case.Ms]
        res = [(o, (m, N), o[:m, :N]) for o, m in zip(outs, case.Ms)]
        M = case.Ms[0]
        if case.entry == "linear_t":
            ldct = M + 3
            out = _out(N, M, ldct)
            rc = lib.temp_linear_t(M, N, K, a_bufs[0].data_ptr(), lda, b_bufs[0].data_ptr(), ldb, tb, out.data_ptr(), ldct, _stream())
            _lib.check(rc, "temp_linear_t")
            res = [(out, (N, M), out[:N, :M].t())]
        elif case.entry == "linear" and case.keys:
            rk = _row_keys(lib, a_bufs[0], M, K, lda)
            rc = lib.temp_linear_keys(M, N, K, a_bufs[0].data_ptr(), lda, rk.data_ptr(), b_bufs[0].data_ptr(), ldb, tb, outs[0].data_ptr(), ldc, _stream())
            _lib.check(rc, "temp_linear_keys")
        elif case.entry == "linear":
            rc = lib.temp_linear(M, N, K, a_bufs[0].data_ptr(), lda, b_bufs[0].data_ptr(), ldb, tb, outs[0].data_ptr(), ldc, _stream())
            _lib.check(rc, "temp_linear")
        else:
            assert case.entry == "multi" and not case.keys
            arr = (_lib.TempLinearProblem * len(case.Ms))()
            for i, m in enumerate(case.Ms):
                arr[i].M, arr[i].A, arr[i].B, arr[i].C = m, a_bufs[i].data_ptr(), b_bufs[case.bpat[i]].data_ptr(), outs[i].data_ptr()
            _lib.check(lib.temp_linear_multi(len(case.Ms), arr, N, K, lda, ldb, tb, ldc, _stream()), "temp_linear_multi")
    torch.cuda.synchronize()           # (the operand buffers live until the launch has run)
    return res


def _untouched(buf, region):
    """every element of `buf` outside its first region = (rows, cols) still holds the NaN it was filled with, bit for bit"""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[:region[0], :region[1]] = False
    return bool((_bits(buf)[mask] == NAN_BITS).all())


def _references(case, a_list, b_list):
    refs = []
    for i in range(len(case.Ms)):
        a = a_list[i].double()
        if case.entry == "tn":
            a, b = a.t(), b_list[0].double()
        else:
            b = b_list[case.bpat[i]].double()
        refs.append((a @ b, a.abs() @ b.abs()))
    return refs


def measure(case):
    """Run the case; -> report dict.  Nothing is asserted here (a script can print the figures of every case)."""
    lib = _lib.load()
    rep = {}
    prev = {k: lib.temp_set_option(GC.OPT[k], v) for k, v in case.opts.items()}
    try:
        a_list, b_list = _operands(case, "wide")
        refused0 = lib.temp_scratch_refused()
        before = _table(lib)
        first = _call(lib, case, a_list, b_list)
        rep["launched"] = _delta(lib, before)
        second = _call(lib, case, a_list, b_list)
        torch.cuda.synchronize()
        rep["refused"] = lib.temp_scratch_refused() - refused0
        rep["repeatable"] = all(torch.equal(_bits(x[0]), _bits(y[0])) for x, y in zip(first, second))
        rep["untouched"] = all(_untouched(buf, region) for buf, region, _ in first)
        worst, ok, finite = 0.0, True, True
        for (ref, sabs), (_, _, got) in zip(_references(case, a_list, b_list), first):
            if got.numel() == 0:
                continue
            g = got.double()
            err = (g - ref).abs()
            finite = finite and bool(torch.isfinite(g).all())
            ok = ok and bool((err <= BAR * sabs).all())
            rel = torch.where(err <= 0, torch.zeros_like(err), err / sabs)       # (a NaN error stays NaN: counted as infinite)
            worst = max(worst, float(rel.nan_to_num(nan=float("inf"), posinf=float("inf")).max()))
        rep["finite"], rep["within_bar"], rep["worst"] = finite, ok, worst
        del first, second
        a_list, b_list = _operands(case, "exact")
        exact = _call(lib, case, a_list, b_list)
        torch.cuda.synchronize()
        rep["exact_untouched"] = all(_untouched(buf, region) for buf, region, _ in exact)
        rep["exact_bad"] = None
        for i, ((ref, _), (_, _, got)) in enumerate(zip(_references(case, a_list, b_list), exact)):
            assert float(ref.abs().max()) < 2 ** 24 if ref.numel() else True
            g = got.double()
            if not torch.equal(g, ref):
                bad = ~(g == ref)
                r, c = [int(v) for v in torch.nonzero(bad)[0]]
                rep["exact_bad"] = "problem %d: %d/%d elements differ, first at row %d column %d: got %r, want %r" % (
                    i, int(bad.sum()), g.numel(), r, c, float(g[r, c]), float(ref[r, c]))
                break
    finally:
        for k, v in prev.items():
            lib.temp_set_option(GC.OPT[k], v)
    return rep


def check(case, rep):
    print("%s: launched %s, worst error %.3e of sum|a||b|" % (case.id, sorted(rep["launched"].items()), rep["worst"]))
    assert rep["launched"] == case.expect, "launched %s, the case pins %s" % (sorted(rep["launched"].items()), sorted(case.expect.items()))
    assert rep["refused"] == 0, "a scratch slot was refused"
    assert rep["untouched"] and rep["exact_untouched"], "padding columns or guard rows were written"
    assert rep["finite"], "non-finite elements in the product"
    assert rep["within_bar"], "worst error %.3e of sum|a||b| (bar %g)" % (rep["worst"], BAR)
    assert rep["repeatable"], "two calls gave different bits"
    assert rep["exact_bad"] is None, "integer operands: " + str(rep["exact_bad"])


@pytest.mark.parametrize("case", GC.ALL, ids=[c.id for c in GC.ALL])
def test_dense_product_route(case):
    check(case, measure(case))


def test_linear_t_refuses_ragged_quad():
    """temp_linear_t with N % 4 != 0 (n_valid ragged inside a column quad) below the weights-resident rows: the row-panel route
    refuses it -- TEMP_E_UNSUPPORTED, no launch counted, nothing written."""
    lib = _lib.load()
    M, K, N = GC.LINEAR_T_REFUSED
    a, b = _wide((M, K), 11, 1.0), _wide((K, N + 2), 12, 0.2)       # (ldb = N + 2: a multiple of 4)
    out = _out(N, M, M + 3)
    before = _table(lib)
    rc = lib.temp_linear_t(M, N, K, a.data_ptr(), K, b.data_ptr(), N + 2, 0, out.data_ptr(), M + 3, _stream())
    torch.cuda.synchronize()
    assert rc == 2, "temp_linear_t returned %d, TEMP_E_UNSUPPORTED expected" % rc
    assert _delta(lib, before) == {}
    assert bool((_bits(out) == NAN_BITS).all())


def test_route_table_covers_every_route_and_width():
    """The cases together reach every kernel family and every width the planners can produce at these shapes."""
    lib = _lib.load()
    hit = set()
    for c in GC.ALL:
        hit |= set(c.expect)
    want = {("panel", w) for w in (1, 2, 3, 4)} | {("wres", w) for w in (1, 2, 3)} | {("wres_split", 1)}
    want |= {("hxr", 0), ("bxr", 0)} | {("tn_w7", w) for w in (1, 2, 4, 7)} | {("tn_w8", 4), ("tn_w8", 7), ("tn_split", 7)}
    assert want <= hit, sorted(want - hit)
    slab = {w for (r, w) in hit if r in ("hxp", "bxp", "bx", "bx_t")}
    assert {1, 7} <= slab and {"hxp", "bxp", "bx", "bx_t"} <= {r for (r, _) in hit}
    assert lib.temp_gemm_route_launches(len(GC.ROUTES), 0) == -1 and lib.temp_gemm_route_launches(0, GC.WIDTHS) == -1
    assert lib.temp_gemm_route_launches(-1, 0) == -1 and lib.temp_gemm_route_launches(0, 0) >= 0
