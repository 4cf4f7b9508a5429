"""The all-entity ("1-vs-all") loss on the MI355X: temp_filtered_ce_fwd / _bwd against the torch composite in fp64 on the same fp32
scores (bars of tests/test_gpu_row_loss_routes.py), at every shape the dispatch distinguishes and every kind of filter list; the
carry over panels; the autograd node and its launches; the option through the models."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import all_entity_cases as AC
from tests.chain_route_cases import Launches
from tests.test_gpu_row_loss_routes import _ce_bars, _traced, assert_close_strict
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def dev(t):
    return None if t is None else t.to(DEV)


def run_kernels(be, c, lists=True, row_scale=True, col0=0):
    lo, hi, ids = (dev(c["lo"]), dev(c["hi"]), dev(c["ids"])) if lists else (None, None, None)
    s, truth = dev(c["s"]), dev(c["truth"])
    loss, lse, state = be.filtered_ce_fwd(s, truth, lo, hi, ids, col0=col0, n=c["N"])
    out = torch.full_like(s, float("nan"))
    d = be.filtered_ce_bwd(s, truth, lo, hi, ids, lse, dev(torch.tensor([0.7])), 1.0, dev(c["rs"]) if row_scale else None, col0=col0, n=c["N"], out=out)
    return loss, lse, d, state


def check_case(be, c):
    loss, lse, d, _ = run_kernels(be, c)
    rt, at = _ce_bars(c["mag"])
    assert_close_strict(loss, c["loss64"], 2e-5, 2e-6 * c["mag"], "loss rows")
    assert_close_strict(lse, c["lse64"], 2e-5, 2e-6 * c["mag"], "lse")
    assert_close_strict(d, c["d64"], rt, at, "d scores")
    dc = d.cpu()
    assert bool((dc[AC.filtered_mask(c)] == 0).all()), "filtered and pad columns are exactly 0"
    if c["P"] > 1:
        assert bool((dc[c["P"] // 2] == 0).all()), "a row scale of 0 gives an exactly zero row"
    again = run_kernels(be, c)
    for a, b in zip((loss, lse, d), again):
        assert torch.equal(a, b), "two identical calls differ"
    return dc


# (1, 8) .. (7, 4001 | 4004): the shapes every suite covers; 1024 | 1028: the two sides of the wave / workgroup threshold; 1280: the
# workgroup route with one step for wave 0 alone and a partial one for wave 1; 40708: past the LDS ceiling of temp_gather_ce_bwd
SHAPES = [(1, 8, 8), (5, 64, 64), (33, 1000, 1000), (7, 4001, 4004), (6, 1024, 1024), (6, 1028, 1028), (9, 1280, 1280), (3, 40708, 40708)]


@pytest.mark.parametrize("mag", [1.0, 1e3])
@pytest.mark.parametrize("P,N,ld", SHAPES)
def test_kernels_vs_fp64(P, N, ld, mag, hip_backend):
    """Row p takes list kind p % 7: empty, the truth alone, the truth plus others, entities 0 and N - 1, 70 entries, 1 500 entries,
    every entity but the truth (loss and gradient 0 up to the rounding of lse - s); truths at 0 and N - 1; one row scale 0."""
    long_row = N == 40708                                  # 3 rows: the long lists and the all-but-truth row on the long row too
    c = AC.kernel_case(P, N, ld, mag, kinds=("long1500", "all-but-truth", "long70") if long_row else AC.LIST_KINDS)
    d = check_case(hip_backend, c)
    if long_row:
        assert float(d[1].abs().max()) <= _ce_bars(mag)[1]
    elif P >= len(AC.LIST_KINDS):
        p = AC.LIST_KINDS.index("all-but-truth")
        assert float(d[p].abs().max()) <= _ce_bars(mag)[1]


@pytest.mark.parametrize("N", [600, 2000])
@pytest.mark.parametrize("kind", AC.LIST_KINDS)
def test_every_list_kind_on_every_row(kind, N, hip_backend):
    """One kind of list on all 9 rows, on the wave route (600) and the workgroup route (2000)."""
    check_case(hip_backend, AC.kernel_case(9, N, N, 1.0, kinds=(kind,), seed=3))


@pytest.mark.parametrize("N", [600, 2000])
def test_no_lists(N, hip_backend):
    """lo == NULL: nothing is filtered."""
    c = AC.kernel_case(9, N, N, 1.0, seed=5)
    c["rows"] = [np.zeros(0, dtype=np.int64)] * 9
    c.update(AC.reference(c, c["rs"], lists=False))
    loss, lse, d, _ = run_kernels(hip_backend, c, lists=False)
    assert_close_strict(loss, c["loss64"], 2e-5, 2e-6, "loss rows")
    assert_close_strict(lse, c["lse64"], 2e-5, 2e-6, "lse")
    assert_close_strict(d, c["d64"], *_ce_bars(1.0), "d scores")


@pytest.mark.parametrize("N", [600, 2000])
def test_cancellation_filtered_entity_holds_the_maximum(N, hip_backend):
    """One FILTERED entity scores +80 beside N(0, 1) admissible scores: exp(80) is 5.5e34 and a sum-then-subtract kernel loses every
    admissible term; the same bars hold here."""
    c = AC.kernel_case(9, N, N, 1.0, seed=9, spike=80.0)
    assert float(c["lse64"].max()) < 20.0
    check_case(hip_backend, c)


@pytest.mark.parametrize("N,panel", [(1000, 4), (1000, 64), (1000, 44), (4000, 64), (4000, 44)])
def test_panels_carry(panel, N, hip_backend):
    """The carried result over panels (44: an odd multiple of 4 that does not divide N) against a single call and fp64; the truth of
    one row in the last panel with EVERY earlier panel entirely filtered for it: its state stays (-inf, 0) bit for bit, no NaN."""
    c = AC.kernel_case(33, N, N, 1.0, seed=11)
    p_all = AC.LIST_KINDS.index("all-but-truth")
    c["truth"][p_all] = N - 1
    c["rows"][p_all] = np.arange(N - 1)
    c["rows"][0] = np.array([panel - 1, panel, c["truth"][0].item()])       # both sides of a panel edge
    c["rows"][0].sort()
    c["rows"][0] = np.unique(c["rows"][0])
    c["lo"], c["hi"], c["ids"] = AC.pack_lists(c["rows"])
    c.update(AC.reference(c, c["rs"]))
    be = hip_backend
    s, truth, lo, hi, ids = (dev(c[k]) for k in ("s", "truth", "lo", "hi", "ids"))
    state = None
    for c0 in range(0, N, panel):
        loss, lse, state = be.filtered_ce_fwd(s[:, c0:min(N, c0 + panel)].contiguous(), truth, lo, hi, ids, col0=c0, carry=state)
        if c0 == 0:
            first = state.clone()
    assert float(first[0, p_all]) == float("-inf") and float(first[1, p_all]) == 0.0 and not bool(torch.isnan(first).any())
    one_loss, one_lse, _ = be.filtered_ce_fwd(s, truth, lo, hi, ids)
    for got, want, what in ((loss, c["loss64"], "carried loss"), (lse, c["lse64"], "carried lse"), (one_loss, c["loss64"], "loss"), (one_lse, c["lse64"], "lse")):
        assert_close_strict(got, want, 2e-5, 2e-6, what)
    assert_close_strict(loss, one_loss, 2e-5, 2e-6, "carried against single")
    scale, rs = dev(torch.tensor([0.7])), dev(c["rs"])
    d = torch.cat([be.filtered_ce_bwd(s[:, c0:min(N, c0 + panel)].contiguous(), truth, lo, hi, ids, lse, scale, 1.0, rs, col0=c0)
                   for c0 in range(0, N, panel)], dim=1)
    assert_close_strict(d, c["d64"], *_ce_bars(1.0), "d scores over panels")
    assert bool((d.cpu()[AC.filtered_mask(c)] == 0).all())


@pytest.mark.parametrize("P,N,ld", [(33, 1000, 1000), (7, 4001, 4004)])
def test_gradient_rows_sum_to_zero(P, N, ld, hip_backend):
    """scale 0.7 and unit row scale: softmax minus one-hot sums to 0 over a row, within atol * N."""
    c = AC.kernel_case(P, N, ld, 1.0, seed=13)
    c["rs"] = torch.ones(P)
    _, _, d, _ = run_kernels(hip_backend, c)
    assert bool(torch.isfinite(d).all()) and float(d.sum(dim=1).abs().max()) <= _ce_bars(1.0)[1] * N


def test_entry_point_conditions(hip_backend):
    """P == 0 succeeds without a launch; a row stride off a multiple of 4 and a misaligned matrix are TEMP_E_UNSUPPORTED; one kernel
    name per entry point in the trace."""
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    st = TB._stream()
    fwd = lambda P, N, ld, s: lib.temp_filtered_ce_fwd(P, N, ld, 0, s, p(zi), None, None, None, 0, p(z), p(z), p(z), p(z), p(z), st)
    _, names = _traced(lambda: fwd(0, 8, 8, p(z)))
    assert names == [] and fwd(0, 8, 8, p(z)) == 0
    assert lib.temp_filtered_ce_bwd(0, 8, 8, 0, p(z), p(zi), None, None, None, p(z), p(z), 1.0, None, p(z), st) == 0
    assert fwd(2, 6, 6, p(z)) == 2 and fwd(2, 8, 8, ctypes.c_void_p(z.data_ptr() + 4)) == 2              # TEMP_E_UNSUPPORTED
    assert fwd(2, 8, 4, p(z)) == 1 and fwd(2, 0, 8, p(z)) == 1                                            # TEMP_E_BADARG
    c = AC.kernel_case(5, 64, 64, 1.0)
    _, names = _traced(lambda: run_kernels(hip_backend, c))
    assert names == ["k_filtered_ce_bwd", "k_filtered_ce_fwd"] or names == ["k_filtered_ce_fwd", "k_filtered_ce_bwd"], names


@pytest.mark.parametrize("panel", [None, 16])
@pytest.mark.parametrize("kind", AC.NODE_KINDS)
def test_node_against_literal_fp64(kind, panel, hip_backend):
    AC.check_node(kind, DEV, panel)


def test_node_launches(hip_backend):
    """The node draws nothing and gathers nothing: no corrupt_sample, no gather_ce_*; one pass = one launch of each stage."""
    rec = Launches(hip_backend)
    TB.set_backend(rec)
    try:
        AC.run_node("complex", DEV, None)
    finally:
        TB.set_backend(None)
    names = [c[0] for c in rec.calls]
    assert names == ["bilinear_query_fwd", "linear_multi", "filtered_ce_fwd", "filtered_ce_bwd", "linear_multi", "linear_tn_multi", "bilinear_query_bwd",
                     "segment_sum_rows", "segment_sum_rows"], names


def test_window_model_fused_equals_literal(hip_backend):
    rec = Launches(hip_backend)
    TB.set_backend(rec)
    try:
        AC.check_window_model(DEV)
    finally:
        TB.set_backend(None)
    names = [c[0] for c in rec.calls]
    assert names.count("corrupt_sample") == 1 and names.index("corrupt_sample") > names.index("filtered_ce_bwd"), "only the option-off step draws"
    assert names.count("filtered_ce_fwd") == 2 and names.count("filtered_ce_bwd") == 1 and names.count("gather_ce_fwd") == 1


def test_static_and_simple_models_fused_equal_literal(hip_backend):
    AC.check_static_model(DEV)
    AC.check_simple_model(DEV)
