"""temp_filtered_topk on the GPU (tests/topk_cases.py): the kernel against temp_amd.evaluation.topk_composite bit for bit on tie-rich
scores -- every filter variant, keep, padding, carried panels in any order, repeatability, refused arguments; topk_single_graph
and predict() through the kernel; TransE answers inside the fp64 band."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd.evaluation import topk_composite
from tests import topk_cases as KC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def dv(t):
    return None if t is None else t.to(DEV)


def same(got, want, what):
    assert torch.equal(got[1].cpu(), want[1]), what + ": ids"
    assert torch.equal(got[0].cpu(), want[0]), what + ": values"


@pytest.mark.parametrize("N", KC.N_VALUES)
@pytest.mark.parametrize("k", KC.K_VALUES)
def test_kernel_equals_composite_bit_exact(k, N):
    """Five rows (ld > N, +inf behind column N; a row with -inf inside N; a row with a +inf score) under every filter variant with
    and without keep: ids and values equal topk_composite's, twice."""
    P = 5
    s = KC.tie_scores(P, N)
    s_d = dv(s)
    be = TB.get_backend()
    for kind in KC.FILTERS:
        for with_keep in (False, True):
            ptr, ids, keep = KC.filter_lists(kind, s, N, with_keep)
            want = topk_composite(s, k, ptr, ids, keep, n=N)
            what = "k=%d N=%d %s keep=%s" % (k, N, kind, with_keep)
            got = be.filtered_topk(s_d, k, dv(ptr), dv(ids), dv(keep), n=N)
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
            same(got, want, what)
            again = be.filtered_topk(s_d, k, dv(ptr), dv(ids), dv(keep), n=N)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), what + ": not bit-repeatable"
            if kind == "all" and not with_keep:
                assert bool((got[1] == -1).all()) and bool((got[0] == KC.NINF).all())


@pytest.mark.parametrize("k", [10, 256])
def test_ascending_and_descending_rows(k):
    """A strictly ascending row (every column survives the compare with the current k-th entry) and a strictly descending one (none
    after the first chunk does) at N = 4096, and the two beyond one chunk at N = 4100."""
    be = TB.get_backend()
    for N in (4096, 4100):
        up = torch.arange(N, dtype=torch.float32) / 8.0
        s = torch.stack([up, up.flip(0), torch.zeros(N)])
        same(be.filtered_topk(dv(s), k), topk_composite(s, k), "N=%d k=%d" % (N, k))


@pytest.mark.parametrize("order", ["asc", "desc", "shuffled"])
@pytest.mark.parametrize("width", [64, 1000])
def test_carried_panels_equal_one_call(width, order):
    """The same matrix in one call and in column panels -- pointer slices with the wide ld and matching col0 -- in ascending,
    descending and shuffled order: all equal, bit for bit."""
    P, N = 5, 4100
    s = KC.tie_scores(P, N)
    s_d = dv(s)
    be = TB.get_backend()
    for k in (10, 256):
        ptr, ids, keep = KC.filter_lists("top", s, N, True)
        want = topk_composite(s, k, ptr, ids, keep, n=N)
        same(be.filtered_topk(s_d, k, dv(ptr), dv(ids), dv(keep), n=N), want, "one call k=%d" % k)
        carry = None
        for c0, c1 in KC.panels(N, width, order):
            carry = be.filtered_topk(s_d[:, c0:], k, dv(ptr), dv(ids), dv(keep), col0=c0, n=c1 - c0, carry=carry)
        same(carry, want, "panels of %d, %s, k=%d" % (width, order, k))


def test_arguments():
    """k = 0, k = 257, ld % 4 != 0 and a misaligned slice are refused by the wrapper and by the C entry point; P = 0 succeeds."""
    be = TB.get_backend()
    s = torch.zeros(3, 8, device=DEV)
    for k in (0, _lib.TOPK_MAX + 1):
        with pytest.raises(ValueError):
            be.filtered_topk(s, k)
    with pytest.raises(ValueError):
        be.filtered_topk(torch.zeros(3, 6, device=DEV), 2)
    with pytest.raises(ValueError):
        be.filtered_topk(s[:, 1:], 2, n=4)
    val, idx = be.filtered_topk(torch.zeros(0, 8, device=DEV), 4)
    assert tuple(val.shape) == tuple(idx.shape) == (0, 4)
    lib = _lib.load()
    tv, ti = torch.empty(3, 4, device=DEV), torch.empty(3, 4, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def call(P, N, ld, k, col0=0, off=0):
        return lib.temp_filtered_topk(P, N, ld, k, col0, p(s, off), None, None, None, 0, p(tv), p(ti), TB._stream())

    assert call(3, 8, 8, 4) == 0
    for bad in (call(3, 8, 8, 0), call(3, 8, 8, _lib.TOPK_MAX + 1), call(3, 6, 6, 4), call(3, 4, 8, 4, off=4), call(3, 8, 4, 4),
                call(3, 8, 8, 4, col0=-1), call(-1, 8, 8, 4)):
        assert bad != 0
    assert lib.temp_filtered_topk(0, 8, 8, 4, 0, None, None, None, None, 0, None, None, TB._stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,k,filtered", KC.BAND_CASES)
def test_transe_answers_inside_fp64_band(case, k, filtered):
    """temp_filtered_topk over temp_l1_scores against fp64: everything above b + 2 tol returned, nothing below b - 2 tol, values
    within tol of the returned id's fp64 score, the contract's order; at most 25 % of the rows ambiguous (an input condition,
    checked without a GPU in tests/test_topk_cpu.py)."""
    c, ptr, ids = KC.band_inputs(case, filtered)
    be = TB.get_backend()
    N = c["s64"].shape[1]
    val, idx = be.filtered_topk(be.l1_scores(dv(c["q"]), dv(c["table"])), k, dv(ptr), dv(ids), n=N)
    amb = KC.band_check(c["s64"], c["tol"], k, val, idx, ptr, ids, "case %d k=%d filtered=%s" % (case, k, filtered))
    print("case %d k=%d filtered=%s: %.2f of the rows ambiguous" % (case, k, filtered, amb))
    assert amb <= 0.25


@pytest.mark.parametrize("panel", [None, 64])
@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("mode", ["tail", "head"])
@pytest.mark.parametrize("N,d", [(204, 8), (203, 8), (204, 200)])
@pytest.mark.parametrize("name", ["distmult", "complex", "transE"])
def test_evaluater_exact_on_integer_tables(name, N, d, mode, filtered, panel):
    KC.check_evaluater(DEV, name, N, d, mode, filtered, panel)


@pytest.mark.parametrize("panel", [None, 64])
def test_evaluater_selection_on_real_scores(panel):
    """Real-valued tables: the device score matrix (the same temp_linear calls, panel by panel), copied to the host and put through
    topk_composite, equals topk_single_graph's answer -- the selection pinned independently of how the scores round."""
    from temp_amd import scores as SC
    import types
    N, d, k = 204, 32, 10
    g = torch.Generator().manual_seed(3)
    table, rel_rows = torch.randn(N, d, generator=g).to(DEV), torch.randn(6, d, generator=g).to(DEV)
    splits = KC.synthetic_splits(N)
    ev = KC.EvaluationFilter(types.SimpleNamespace(score_function="distmult"), SC.distmult, *splits)
    known, rel = KC.queries_at(splits, 0, 5)
    ptr, ids = KC.sets_to_csr(KC.true_sets(splits, 0, known, rel, "tail"))
    q = SC.bilinear_query("distmult", table[torch.as_tensor(known, device=DEV)], rel_rows[torch.as_tensor(rel, device=DEV)], "tail").contiguous()
    width = N if panel is None else panel
    score = torch.cat([TB.get_backend().linear(q, table[c0:c0 + width].contiguous(), True) for c0 in range(0, N, width)], dim=1).cpu()
    want_val, want_idx = topk_composite(score, k, ptr, ids)
    got_idx, got_val = ev.topk_single_graph(table, rel_rows, known, rel, "tail", 0, k, panel=panel)
    assert torch.equal(got_idx.cpu(), want_idx) and torch.equal(got_val.cpu(), want_val)


@pytest.mark.parametrize("module", KC.MODELS)
def test_predict_against_fp64_tables(module):
    KC.check_predict(module, DEV)


def test_predict_distmult_and_known_true():
    KC.check_predict("Static", DEV, "distmult")
    KC.check_unfiltered_can_return_known(DEV)


def test_k_above_the_kernel_limit():
    KC.check_large_k(DEV)


def test_post_models_raise_and_state_dict():
    KC.check_post_models_raise(DEV)
    KC.check_state_dict_round_trip(DEV)


def test_launch_is_traced_under_its_name():
    """The launch goes through the trace macros: one k_filtered_topk record per call."""
    lib = _lib.load()
    be = TB.get_backend()
    s = dv(KC.tie_scores(5, 1024))
    be.filtered_topk(s, 10, n=1024)
    torch.cuda.synchronize()
    ids, ms, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(16), "temp_trace_begin")
    try:
        be.filtered_topk(s, 10, n=1024)
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 16, ctypes.byref(cnt)), "temp_trace_end")
    assert [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)] == ["k_filtered_topk"]
