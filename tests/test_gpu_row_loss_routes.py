"""Every route of the row kernels (rows_kernels.hip) and of the candidate-loss kernels (loss_kernels.hip, gated_loss.hip) on the
MI355X, each against a plain high-precision restatement of the same operation.

Segment sums: integer-valued sources, so every sum is exact in fp32 whatever the order, compared with torch.equal against an int64
index_add_; the route is pinned by the workspace the library asks for and by the number of launches it records.  Candidate
cross-entropy: fp64 logsumexp with autograd at every threshold between two kernels and at the LDS ceiling of the backward.  Raw
ctypes calls write into NaN-filled outputs, and the comparisons here fail on any non-finite element."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import row_loss_route_cases as RC
from tests.cpu_backend import CpuTestBackend
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
NAN = float("nan")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


# ---------------------------------------------------------------------------------------------------------------------
# NaN-strict comparisons
# ---------------------------------------------------------------------------------------------------------------------
def assert_close_strict(got, want, rtol, atol, what):
    """|got - want| <= atol + rtol |want| element by element; a shape mismatch or a non-finite element of `got` fails."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    assert g.shape == w.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(w.shape))
    assert bool(torch.isfinite(w).all()), "%s: the reference itself is not finite" % what
    if g.numel() == 0:
        return
    finite = torch.isfinite(g)
    assert bool(finite.all()), "%s: %d/%d elements are not finite" % (what, int((~finite).sum()), g.numel())
    err, tol = (g - w).abs(), atol + rtol * w.abs()
    i = int(torch.argmax(err - tol))
    print("%s: max |err| %.3e, max |err| / bar %.3g (max|want| %.3e)" % (what, float(err.max()), float((err / tol.clamp(min=1e-300)).max()), float(w.abs().max())))
    bad = ~(err <= tol)
    assert not bool(bad.any()), "%s: %d/%d elements out of tolerance (rtol=%g atol=%g); worst |err|=%.3e at flat %d (got %.8g, want %.8g)" % (
        what, int(bad.sum()), g.numel(), rtol, atol, float(err.view(-1)[i]), i, float(g.view(-1)[i]), float(w.view(-1)[i]))


def assert_exact(got, want, what):
    """Bit-for-bit the reference (integer-valued data): torch.equal, which an unwritten (NaN) element cannot pass."""
    g, w = got.detach().cpu(), want.to(got.dtype)
    assert g.shape == w.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(w.shape))
    if not torch.equal(g, w):
        bad = ~(g == w)
        i = int(torch.nonzero(bad.view(-1))[0])
        raise AssertionError("%s: %d/%d elements differ (%d not finite); first at flat %d of shape %s: got %r, want %r" % (
            what, int(bad.sum()), g.numel(), int((~torch.isfinite(g.double())).sum()), i, tuple(g.shape), float(g.view(-1)[i]), float(w.view(-1)[i])))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _traced(fn):
    """fn() between temp_trace_begin / temp_trace_end -> (result, names of the launches the library recorded)."""
    lib = _lib.load()
    ids, ms, cnt = (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(64), "temp_trace_begin")
    try:
        out = fn()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 64, ctypes.byref(cnt)), "temp_trace_end")
    return out, [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)]


# ---------------------------------------------------------------------------------------------------------------------
# segment sums
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segmentation(name):
    """-> (ids int64 [n] host, seg_ptr, order on the device, n_seg, n_rows) of a case of tests/row_loss_route_cases.py."""
    n_seg, n_rows = RC.check_shape(name)
    ids = RC.gather_ids(name)
    seg_ptr, order = TF.gather_inverse(ids, n_seg, DEV)
    assert order.shape[0] == n_rows and seg_ptr.shape[0] == n_seg + 1 and 0 < int((ids < 0).sum()) <= len(ids) // 40
    assert np.array_equal(np.diff(seg_ptr.cpu().numpy()), RC.lengths(name))
    return torch.from_numpy(ids.astype(np.int64)), seg_ptr, order, n_seg, n_rows


@functools.lru_cache(maxsize=4)
def _int_problem(name, d):
    """Integer-valued sources in [-8, 8] (|any sum| < 2^24: exact in fp32 in any order), a non-negative table with exact zeros
    for the folded ReLU, and the int64 sums.  Computed once per (case, width) and left unchanged."""
    ids, _, _, n_seg, _ = _segmentation(name)
    rng = np.random.default_rng(1000 + d)
    src = torch.from_numpy(rng.integers(-8, 9, size=(len(ids), d)))
    table = torch.from_numpy(rng.integers(0, 3, size=(n_seg, d)).astype(np.float32))
    keep = ids >= 0
    want = torch.zeros(n_seg, d, dtype=torch.int64).index_add_(0, ids[keep], src[keep])
    assert int(want.abs().max()) < 2 ** 24 and bool((table == 0).any()) and bool((want != 0).any())
    return src.float(), table, want


def _want(name, d, relu):
    _, table, want = _int_problem(name, d)
    return want * (table > 0) if relu else want


def _raw_segment_sum(name, d, src, relu_of, with_workspace):
    """temp_segment_sum_rows[_relu] through ctypes into a NaN-filled `out` (workspace NULL unless with_workspace)."""
    lib = _lib.load()
    _, seg_ptr, order, n_seg, n_rows = _segmentation(name)
    out = torch.full((n_seg, d), NAN, dtype=torch.float32, device=DEV)
    nb = lib.temp_segment_sum_rows_workspace(n_seg, n_rows, d) if with_workspace else 0
    ws = torch.full((max(nb, 4) // 4,), NAN, dtype=torch.float32, device=DEV) if nb else None
    if relu_of is None:
        rc = lib.temp_segment_sum_rows(n_seg, n_rows, d, _p(seg_ptr), _p(order), _p(src), _p(out), _p(ws), nb, TB._stream())
    else:
        rc = lib.temp_segment_sum_rows_relu(n_seg, n_rows, d, _p(seg_ptr), _p(order), _p(src), _p(relu_of), _p(out), _p(ws), nb, TB._stream())
    _lib.check(rc, "temp_segment_sum_rows")
    return out


def _check_repeatable(name, d, table, be):
    _, seg_ptr, order, n_seg, _ = _segmentation(name)
    g = torch.Generator().manual_seed(d)
    src = torch.randn(_segmentation(name)[0].shape[0], d, generator=g).to(DEV)
    a = be.segment_sum_rows(src, seg_ptr, order, n_seg, relu_of=table)
    b = be.segment_sum_rows(src, seg_ptr, order, n_seg, relu_of=table)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b), "float source: two runs differ"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name,d", RC.NARROW)
def test_segment_sum_every_route_exact(name, d, relu, hip_backend):
    """short (LPR 8 .. 64, tail guard), pieces (hub over 19 pieces, aligned starts and ends, empty runs, partial last piece),
    blk<4> (skew; grid-stride), blk<16>, split (parts and segments that are empty): the workspace names the route, the trace counts
    its launches (2 for split and pieces, else 1), the sums equal int64 index_add_ exactly, with and without the folded ReLU."""
    lib = _lib.load()
    _, seg_ptr, order, n_seg, n_rows = _segmentation(name)
    src, table, _ = _int_problem(name, d)
    assert lib.temp_segment_sum_rows_workspace(n_seg, n_rows, d) == RC.workspace_bytes(name, d)
    src, table = src.to(DEV), (table.to(DEV) if relu else None)
    got, names = _traced(lambda: hip_backend.segment_sum_rows(src, seg_ptr, order, n_seg, relu_of=table))
    assert names == ["k_segment_sum_rows"] * RC.launches(name, d), names
    assert_exact(got, _want(name, d, relu), "segment sum %s d=%d" % (name, d))
    _check_repeatable(name, d, table, hip_backend)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name,d", RC.NULL_WS_CASES)
def test_segment_sum_null_workspace_falls_back(name, d, relu):
    """workspace = NULL: the promised fallback, one wave per segment (k_segment_sum_rows<8 / 16 / 32 / 64> on the pieces shape)
    or one block per segment (blk<16> on the split shape) -- one launch, every element written."""
    src, table, _ = _int_problem(name, d)
    src, table = src.to(DEV), (table.to(DEV) if relu else None)
    got, names = _traced(lambda: _raw_segment_sum(name, d, src, table, with_workspace=False))
    assert names == ["k_segment_sum_rows"], names
    assert_exact(got, _want(name, d, relu), "segment sum %s d=%d, NULL workspace" % (name, d))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name,d", RC.WIDE)
def test_segment_sum_wider_than_256(name, d, relu, hip_backend):
    """d > 256: more float4 columns than a wave has lanes.  Every column of every segment is written and exact, through the backend
    and through a raw call into a NaN-filled buffer, on the short, pieces, blk<16> and split segmentations."""
    lib = _lib.load()
    _, seg_ptr, order, n_seg, n_rows = _segmentation(name)
    src, table, _ = _int_problem(name, d)
    assert lib.temp_segment_sum_rows_workspace(n_seg, n_rows, d) == 0
    src, table = src.to(DEV), (table.to(DEV) if relu else None)
    got, names = _traced(lambda: hip_backend.segment_sum_rows(src, seg_ptr, order, n_seg, relu_of=table))
    assert names == ["k_segment_sum_rows"], names
    assert_exact(got, _want(name, d, relu), "segment sum %s d=%d" % (name, d))
    raw = _raw_segment_sum(name, d, src, table, with_workspace=True)
    assert_exact(raw, _want(name, d, relu), "segment sum %s d=%d, raw call" % (name, d))
    _check_repeatable(name, d, table, hip_backend)


def test_segment_sum_rejects_unaligned_width():
    """d % 4 != 0 -> TEMP_E_UNSUPPORTED before anything is launched (the kernels move float4 columns)."""
    lib = _lib.load()
    _, seg_ptr, order, n_seg, n_rows = _segmentation("blk16")
    src = torch.ones(_segmentation("blk16")[0].shape[0], 6, device=DEV)
    out = torch.full((n_seg, 6), 7.0, device=DEV)
    rc = lib.temp_segment_sum_rows(n_seg, n_rows, 6, _p(seg_ptr), _p(order), _p(src), _p(out), None, 0, TB._stream())
    assert rc == 2
    rc = lib.temp_segment_sum_rows_relu(n_seg, n_rows, 6, _p(seg_ptr), _p(order), _p(src), _p(out), _p(out), None, 0, TB._stream())
    assert rc == 2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# candidate cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def _candidates(P, C, N, g):
    cand = torch.randint(0, N, (P, C), generator=g).int()
    if C > 2:
        cand[:, 2] = cand[:, 1]                                             # duplicate candidates
        cand[::3, 1] = cand[::3, 0]                                         # the truth listed twice
    return cand


def _ce_bars(mag):
    # those of test_gather_ce_mix_kernels_vs_fp64: at magnitude 1e3 the fp32 score resolves s - lse to ~1e-4 only
    return (2e-5, 2e-6) if mag == 1.0 else (3e-4, 1e-4)


CE_SHAPES = [(9, 1100, 2052),       # forward: counters in LDS, a workgroup per row
             (6, 512, 1024),        # upper edge of the wave kernels: all 16 registers per lane live
             (6, 513, 1028),        # just past it
             (33, 500, 1000),       # N % 64 != 0, P % 4 != 0
             (5, 8192, 16384),      # 64 KB of counters in both directions
             (5, 8200, 16388),      # plain forward with the C > 1024 loop; backward past 64 KB
             (7, 1024, 4000),       # plain forward: candidates in registers, at the edge
             (7, 1025, 4000),       # plain forward: the loop, at the edge
             (3, 600, 40704),       # backward at its LDS ceiling (159 KB)
             (4, 1, 8)]             # one candidate: loss rows and d_scores are 0 up to the rounding of lse - s


@pytest.mark.parametrize("mag", [1.0, 1e3])
@pytest.mark.parametrize("row_scale", [False, True])
@pytest.mark.parametrize("P,C,N", CE_SHAPES)
def test_gather_ce_kernels_vs_fp64(P, C, N, row_scale, mag, hip_backend):
    """temp_gather_ce_fwd / _bwd at every threshold of their dispatch against fp64 logsumexp with autograd: duplicate candidates,
    the truth listed twice, row_scale null and set, an upstream scale of 0.7, gradients exactly 0 off the candidate columns.
    Bars of test_gather_ce_mix_kernels_vs_fp64."""
    g = torch.Generator().manual_seed(P * 131 + C * 13 + N)
    s = torch.randn(P, N, generator=g) * mag
    cand = _candidates(P, C, N, g)
    rs = torch.rand(P, generator=g) if row_scale else None
    s64 = s.double().requires_grad_(True)
    logits = s64.gather(1, cand.long())
    lse64 = torch.logsumexp(logits, dim=1)
    loss64 = lse64 - logits[:, 0]
    scale64 = rs.double() if row_scale else torch.full((P,), 1.0 / P, dtype=torch.float64)
    (0.7 * (loss64 * scale64).sum()).backward()
    dev = lambda t: t.to(DEV)
    loss, lse = hip_backend.gather_ce_fwd(dev(s), dev(cand))
    d = hip_backend.gather_ce_bwd(dev(s), dev(cand), lse, dev(torch.tensor([0.7])), 1.0 / P, dev(rs) if row_scale else None)
    rt, at = _ce_bars(mag)
    assert_close_strict(loss, loss64, 2e-5, 2e-6 * mag, "loss rows")
    assert_close_strict(lse, lse64, 2e-5, 2e-6 * mag, "lse")
    assert_close_strict(d, s64.grad, rt, at, "d scores")
    off = torch.ones(P, N, dtype=torch.bool).scatter_(1, cand.long(), False)
    assert bool((d.cpu()[off] == 0).all())


def test_gather_ce_bwd_refuses_rows_past_its_lds():
    """N = 40708: four bytes past the backward's 159 KB of counters -> TempAmdError, nothing launched; the forward (no such
    limit: candidates gathered in registers) still answers."""
    be = TB.get_backend()
    P, C, N = 3, 600, 40708
    g = torch.Generator().manual_seed(5)
    s = torch.randn(P, N, generator=g)
    cand = _candidates(P, C, N, g)
    logits = s.double().gather(1, cand.long())
    lse64 = torch.logsumexp(logits, dim=1)
    loss, lse = be.gather_ce_fwd(s.to(DEV), cand.to(DEV))
    assert_close_strict(loss, lse64 - logits[:, 0], 2e-5, 2e-6, "loss rows")
    assert_close_strict(lse, lse64, 2e-5, 2e-6, "lse")
    with pytest.raises(_lib.TempAmdError):
        be.gather_ce_bwd(s.to(DEV), cand.to(DEV), lse, torch.tensor([0.7], device=DEV), 1.0 / P)


@pytest.mark.parametrize("mag", [1.0, 1e3])
@pytest.mark.parametrize("row_scale", [False, True])
@pytest.mark.parametrize("N", [16388, 40704])
def test_gather_ce_mix_long_rows_vs_fp64(N, row_scale, mag, hip_backend):
    """temp_gather_ce_mix_fwd / _bwd with more than 64 KB of counters, and at the 159 KB ceiling, against fp64 (formulas and bars of
    test_gather_ce_mix_kernels_vs_fp64)."""
    P, C = 3, 21
    g = torch.Generator().manual_seed(N + 7)
    s_a, s_b = torch.randn(P, N, generator=g) * mag, torch.randn(P, N, generator=g) * mag
    w = torch.tensor([0.0, 1.0, 0.37])
    cand = _candidates(P, C, N, g)
    rs = torch.rand(P, generator=g) if row_scale else None
    a64, b64, w64 = (x.double().requires_grad_(True) for x in (s_a, s_b, w))
    m = w64.view(-1, 1) * a64.gather(1, cand.long()) + (1 - w64.view(-1, 1)) * b64.gather(1, cand.long())
    lse64 = torch.logsumexp(m, dim=1)
    loss64 = lse64 - m[:, 0]
    scale64 = rs.double() if row_scale else torch.full((P,), 1.0 / P, dtype=torch.float64)
    (0.7 * (loss64 * scale64).sum()).backward()
    dev = lambda t: t.to(DEV)
    loss, lse = hip_backend.gather_ce_mix_fwd(dev(s_a), dev(s_b), dev(w), dev(cand))
    d_a, d_b, d_w = hip_backend.gather_ce_mix_bwd(dev(s_a), dev(s_b), dev(w), dev(cand), lse, dev(torch.tensor([0.7])), 1.0 / P,
                                                  dev(rs) if row_scale else None)
    rt, at = _ce_bars(mag)
    assert_close_strict(loss, loss64, 2e-5, 2e-6 * mag, "loss rows")
    assert_close_strict(lse, lse64, 2e-5, 2e-6 * mag, "lse")
    assert_close_strict(d_a, a64.grad, rt, at, "d s_a")
    assert_close_strict(d_b, b64.grad, rt, at, "d s_b")
    assert_close_strict(d_w, w64.grad, rt, 2e-6 if mag == 1.0 else at * float((s_a - s_b).abs().max()), "d w")
    off = torch.ones(P, N, dtype=torch.bool).scatter_(1, cand.long(), False)
    assert bool((d_a.cpu()[off] == 0).all()) and bool((d_b.cpu()[off] == 0).all())


def test_gather_ce_mix_bwd_refuses_rows_past_its_lds():
    be = TB.get_backend()
    P, C, N = 3, 21, 40708
    g = torch.Generator().manual_seed(6)
    s_a, s_b, w = torch.randn(P, N, generator=g), torch.randn(P, N, generator=g), torch.rand(P, generator=g)
    cand = _candidates(P, C, N, g)
    m = w.double().view(-1, 1) * s_a.double().gather(1, cand.long()) + (1 - w.double().view(-1, 1)) * s_b.double().gather(1, cand.long())
    loss, lse = be.gather_ce_mix_fwd(s_a.to(DEV), s_b.to(DEV), w.to(DEV), cand.to(DEV))
    assert_close_strict(lse, torch.logsumexp(m, dim=1), 2e-5, 2e-6, "lse")
    assert_close_strict(loss, torch.logsumexp(m, dim=1) - m[:, 0], 2e-5, 2e-6, "loss rows")
    with pytest.raises(_lib.TempAmdError):
        be.gather_ce_mix_bwd(s_a.to(DEV), s_b.to(DEV), w.to(DEV), cand.to(DEV), lse, torch.tensor([0.7], device=DEV), 1.0 / P)


# ---------------------------------------------------------------------------------------------------------------------
# decay, gather, scatter, filtered rank
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 4), (37, 32), (1000, 64), (513, 128), (300, 200), (70, 260), (16500, 260), (131100, 8), (0, 16)])
def test_decay_rows_vs_fp64(n, d, hip_backend):
    """temp_decay_rows against fp64 x exp(-dt lambda), dt in [0, 50], lambda = 0.1 (as the kernel receives it: rounded to fp32).
    Every lanes-per-row variant, the column loop (d > 256), both grid caps (16 500 rows at 4 per block, 131 100 at 32), no rows.
    rtol 1e-6: half an ulp of the argument (|arg| <= 5: 2.4e-7 relative in the result), expf, and the product."""
    g = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, d, generator=g)
    dt = torch.rand(n, generator=g) * 50.0
    if n > 1:
        dt[0], dt[-1] = 0.0, 50.0
    lam = float(np.float32(0.1))
    got = hip_backend.decay_rows(x.to(DEV), dt.to(DEV), lam)
    want = x.double() * torch.exp(-dt.double().view(-1, 1) * lam)
    assert_close_strict(got, want, 1e-6, 0.0, "decay rows")


@pytest.mark.parametrize("n,d,rows", [(30000, 200, 700), (17, 4, 5), (50, 260, 9)])
def test_gather_rows_exact(n, d, rows, hip_backend):
    """temp_gather_rows past its grid cap (30 000 x 50 float4 > 4096 x 256 threads), at one float4 per row and wider than 256;
    idx < 0 gives a zero row."""
    rng = np.random.default_rng(n + d)
    table = torch.from_numpy(rng.integers(-8, 9, size=(rows, d)).astype(np.float32))
    idx = rng.integers(-1, rows, size=n).astype(np.int64)
    idx[0], idx[-1] = -1, rows - 1
    got = hip_backend.gather_rows(table.to(DEV), torch.from_numpy(idx.astype(np.int32)).to(DEV))
    want = table[torch.from_numpy(idx).clamp(min=0)] * torch.from_numpy(idx >= 0).float().view(-1, 1)
    assert_exact(got, want, "gather rows")


@pytest.mark.parametrize("n,d,rows", [(5000, 6, 300), (5000, 260, 300)])
def test_scatter_add_rows_exact(n, d, rows, hip_backend):
    """temp_scatter_add_rows at a width that is no multiple of 4 and past its grid cap (5000 x 260 > 4096 x 256): integer data,
    so the atomic sums are exact in any order."""
    rng = np.random.default_rng(n + d)
    src = torch.from_numpy(rng.integers(-8, 9, size=(n, d)))
    base = torch.from_numpy(rng.integers(-8, 9, size=(rows, d)))
    idx = torch.from_numpy(rng.integers(-1, rows, size=n))
    keep = idx >= 0
    want = base.clone().index_add_(0, idx[keep], src[keep])
    got = hip_backend.scatter_add_rows(src.float().to(DEV), idx.int().to(DEV), base.float().to(DEV))
    assert_exact(got, want, "scatter add rows")


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("N", [3, 7, 1030])
def test_filtered_rank_padded_rows_raw(N, filtered):
    """temp_filtered_rank with ld > N and N % 4 != 0 (the C ABI takes both, the Python wrapper neither): padding columns of +inf
    must not be read; ranks equal the test backend's on [:, :N].  Scores on a grid of 0.5 in [-4, 4]: many exact ties (the
    tie-break by entity id), and distinct scores keep distinct sigmoids in any rounding."""
    lib = _lib.load()
    P, ld = 37, 4 * ((N + 3) // 4) + 4
    g = torch.Generator().manual_seed(N)
    scores = torch.full((P, ld), float("inf"))
    scores[:, :N] = torch.randint(-8, 9, (P, N), generator=g).float() * 0.5
    target = torch.randint(0, N, (P,), generator=g).int()
    filt_ptr = filt_ids = None
    if filtered:
        lists = [torch.unique(torch.cat([torch.randint(0, N, (min(N, 1 + p % 5),), generator=g), target[p:p + 1].long()])) for p in range(P)]
        filt_ptr = torch.tensor([0] + [len(x) for x in lists]).cumsum(0).int()
        filt_ids = torch.cat(lists).int()
    want = CpuTestBackend().filtered_rank(scores[:, :N].contiguous(), target, filt_ptr, filt_ids)
    dev = lambda t: None if t is None else t.to(DEV)
    s_d, t_d, fp_d, fi_d = dev(scores), dev(target), dev(filt_ptr), dev(filt_ids)
    ranks = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    rc = lib.temp_filtered_rank(P, N, ld, _p(s_d), _p(t_d), _p(fp_d), _p(fi_d), _p(ranks), TB._stream())
    _lib.check(rc, "temp_filtered_rank")
    assert torch.equal(ranks.cpu().long(), want), (ranks.cpu().tolist(), want.tolist())
    assert len(set(want.tolist())) > 1
