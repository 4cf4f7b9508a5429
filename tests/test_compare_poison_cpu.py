"""The two helpers every GPU test leans on, checked without a GPU: `golden_util.assert_close` must fail on anything
non-finite that the reference does not have at the same place, and `poison.poisoned_allocations` must put its
pattern into every buffer `torch.empty`, `torch.empty_like` and `Tensor.new_empty` hand out and leave no trace."""
import math
import struct

import numpy as np
import pytest
import torch

from tests import poison
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations, poisoned_allocations_fixture  # noqa: F401  (the second registers the fixture)

NAN, INF = float("nan"), float("inf")


def _t(*v):
    return torch.tensor(v, dtype=torch.float32)


def _one_nan_among_many():
    want = torch.linspace(-3.0, 3.0, 10 ** 4)
    got = want.clone()
    got[7321] = NAN
    return got, want


MUST_FAIL = {
    "nan_vs_finite": lambda: (_t(1.0, NAN, 3.0), _t(1.0, 2.0, 3.0)),
    "finite_vs_nan_reference": lambda: (_t(1.0, 2.0, 3.0), _t(1.0, NAN, 3.0)),
    "nan_vs_nan_reference": lambda: (_t(1.0, NAN), _t(1.0, NAN)),
    "inf_vs_finite": lambda: (_t(INF, 2.0), _t(1.0, 2.0)),
    "neg_inf_vs_finite": lambda: (_t(-INF, 2.0), _t(1.0, 2.0)),
    "finite_vs_inf": lambda: (_t(1.0, 2.0), _t(INF, 2.0)),
    "inf_vs_neg_inf": lambda: (_t(INF, 2.0), _t(-INF, 2.0)),
    "nan_vs_inf": lambda: (_t(NAN, 2.0), _t(INF, 2.0)),
    "one_nan_among_1e4": _one_nan_among_many,
    "shape_mismatch": lambda: (torch.zeros(2, 3), torch.zeros(3, 2)),
    "plain_error": lambda: (_t(1.0, 2.1), _t(1.0, 2.0)),
}


@pytest.mark.parametrize("name", sorted(MUST_FAIL))
def test_assert_close_fails(name):
    got, want = MUST_FAIL[name]()
    with pytest.raises(AssertionError):
        assert_close(got, want, 1e-5, 1e-6, name)
    with pytest.raises(AssertionError):                      # numpy inputs go the same way
        assert_close(got.numpy(), want.numpy(), 1e-5, 1e-6, name)


def test_assert_close_huge_tolerance_does_not_excuse_non_finite():
    """atol = inf makes every finite error pass; a NaN or a wrong infinity must still fail."""
    assert_close(_t(1.0, 2.0), _t(5.0, -7.0), 0.0, INF, "finite")
    for got, want in ((_t(NAN, 2.0), _t(1.0, 2.0)), (_t(INF, 2.0), _t(1.0, 2.0)), (_t(INF, 2.0), _t(-INF, 2.0))):
        with pytest.raises(AssertionError):
            assert_close(got, want, 0.0, INF, "non-finite")


def _at_the_bar():
    # in float64, where the comparison is made, 0.5 + 0.125 and 1.0 * 0.125 are exact: the error equals the bar
    want = torch.tensor([1.0, -1.0], dtype=torch.float64)
    return want + torch.tensor([0.625, -0.625], dtype=torch.float64), want, 0.125, 0.5


MUST_PASS = {
    "equal_infinities": lambda: (_t(INF, 1.0, -INF, 2.0), _t(INF, 1.0, -INF, 2.0), 1e-5, 1e-6),
    "empty": lambda: (torch.empty(0, 4), torch.empty(0, 4), 1e-5, 1e-6),
    "empty_with_nan_tolerance_irrelevant": lambda: (torch.empty(0), torch.empty(0), 0.0, 0.0),
    "error_exactly_at_the_bar": _at_the_bar,
    "exact": lambda: (_t(1.0, 2.0), _t(1.0, 2.0), 0.0, 0.0),
}


@pytest.mark.parametrize("name", sorted(MUST_PASS))
def test_assert_close_passes(name):
    got, want, rtol, atol = MUST_PASS[name]()
    assert_close(got, want, rtol, atol, name)


def test_assert_close_just_past_the_bar_fails():
    got, want, rtol, atol = _at_the_bar()
    got = got.clone()
    got[0] = math.nextafter(float(got[0]), INF)
    with pytest.raises(AssertionError):
        assert_close(got, want, rtol, atol, "past the bar")


def test_assert_close_message_names_non_finite_count_and_a_sane_worst_element():
    got, want = _one_nan_among_many()
    got[11] = INF
    got[12] += 0.5                                            # the largest FINITE error; must not be what is reported
    with pytest.raises(AssertionError) as e:
        assert_close(got, want, 1e-5, 1e-6, "msg")
    msg = str(e.value)
    assert msg.startswith("msg: 3/10000 elements out of tolerance (rtol=1e-05 atol=1e-06)")
    assert "2 non-finite in got" in msg
    assert "at flat 11 " in msg or "at flat 7321 " in msg     # a non-finite element is the worst one
    # finite failures only: the pick is the largest excess, and the count is zero
    got, want = _t(1.0, 2.5, 3.1), _t(1.0, 2.0, 3.0)
    with pytest.raises(AssertionError) as e:
        assert_close(got, want, 1e-5, 1e-6, "msg")
    assert "2/3 elements" in str(e.value) and "at flat 1 " in str(e.value) and "0 non-finite in got" in str(e.value)


def test_assert_close_message_for_nan_reference():
    with pytest.raises(AssertionError, match=r"the reference itself is not finite \(NaN\)"):
        assert_close(_t(1.0, 2.0), _t(1.0, NAN), 1e-5, 1e-6, "ref")


# ------------------------------------------------------------------------------------------------ poisoned_allocations

FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
INTS = (torch.int32, torch.int64)


@pytest.mark.parametrize("dtype", FLOATS + INTS + (torch.bool,), ids=str)
def test_poison_pattern_by_dtype(dtype):
    with poisoned_allocations():
        ts = [torch.empty(3, 5, dtype=dtype), torch.empty((7,), dtype=dtype), torch.empty_like(torch.zeros(2, 2, dtype=dtype)),
              torch.zeros(1, dtype=dtype).new_empty(4, 3), torch.zeros(1).new_empty((6,), dtype=dtype)]
    for t in ts:
        assert t.dtype == dtype
        if dtype in FLOATS:
            assert torch.isnan(t).all()
        elif dtype in INTS:
            assert (t == -2).all()
        else:
            assert t.all()


@pytest.mark.parametrize("nbytes", [1, 3, 4, 7, 64, 1027])
def test_poison_uint8_workspace_reads_as_nan_and_minus_two(nbytes):
    with poisoned_allocations():
        ws = torch.empty(nbytes, dtype=torch.uint8)
    n4 = nbytes - nbytes % 4
    raw = bytes(ws.tolist())
    assert raw == struct.pack("<I", 0xFFFFFFFE) * (n4 // 4) + b"\xff" * (nbytes % 4)
    if n4:
        assert torch.isnan(ws[:n4].view(torch.float32)).all()
        assert (ws[:n4].view(torch.int32) == -2).all()
        assert torch.isnan(ws[:n4].view(torch.float16)).all()
    if n4 >= 8:
        n8 = nbytes - nbytes % 8
        assert torch.isnan(ws[:n8].view(torch.float64)).all()
    assert (ws[n4:] == 0xFF).all()


def test_poison_uint8_other_layouts():
    base = torch.zeros(6, 10, dtype=torch.uint8).t()          # non-contiguous, dense
    with poisoned_allocations():
        like = torch.empty_like(base)
        two_d = torch.empty(5, 8, dtype=torch.uint8)
    assert like.stride() == base.stride() and not like.is_contiguous()
    assert bytes(like.reshape(-1).tolist()) == struct.pack("<I", 0xFFFFFFFE) * 15
    assert (two_d.view(torch.int32) == -2).all()


def test_poison_empty_like_of_non_contiguous():
    base = torch.zeros(8, 6)[:, ::2].t()                      # strides (2, 6): neither contiguous nor dense
    dense_t = torch.zeros(4, 9).t()
    with poisoned_allocations():
        a, b = torch.empty_like(base), torch.empty_like(dense_t)
        c = torch.empty_like(base, dtype=torch.int32)
    assert a.shape == base.shape and torch.isnan(a).all()
    assert b.stride() == dense_t.stride() and torch.isnan(b).all()
    assert torch.isnan(torch.as_strided(b, (36,), (1,))).all()          # every element of the storage, not only a view of it
    assert (c == -2).all()


def test_poison_new_empty_follows_the_source_tensor():
    src = torch.zeros(3, dtype=torch.float64)
    par = torch.nn.Parameter(torch.zeros(2))
    with poisoned_allocations():
        a = src.new_empty(2, 5)
        b = src.new_empty((4,), dtype=torch.int64)
        c = par.new_empty(3)
        d = src.new_empty(size=(2, 2))
    assert a.dtype == torch.float64 and a.shape == (2, 5) and torch.isnan(a).all()
    assert b.dtype == torch.int64 and (b == -2).all()
    assert torch.isnan(c).all() and not c.requires_grad
    assert torch.isnan(d).all()


def test_poison_keyword_forms_and_requires_grad():
    with poisoned_allocations():
        a = torch.empty(size=(2, 3), dtype=torch.float32)
        b = torch.empty(4, requires_grad=True)
        out = torch.zeros(5)
        c = torch.empty(5, out=out)
    assert torch.isnan(a).all()
    assert b.requires_grad and b.is_leaf and torch.isnan(b).all()
    assert c is out and torch.isnan(out).all()


def test_poison_zero_size_untouched():
    with poisoned_allocations():
        for t in (torch.empty(0), torch.empty(0, 7, dtype=torch.int32), torch.empty(3, 0, dtype=torch.uint8),
                  torch.empty_like(torch.zeros(0, 2)), torch.zeros(2).new_empty(0)):
            assert t.numel() == 0


def _patched():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__)


def test_poison_restores_originals():
    before = _patched()
    with poisoned_allocations():
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
    assert _patched() == before
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned_allocations():
            torch.empty(3)
            raise RuntimeError("boom")
    assert _patched() == before
    assert torch.zeros(2).new_empty(3).shape == (3,)          # the inherited method is back and works


def test_poison_nests():
    before = _patched()
    with poisoned_allocations():
        outer = _patched()
        with poisoned_allocations():
            assert torch.isnan(torch.empty(3)).all() and (torch.zeros(1).new_empty(2, dtype=torch.int32) == -2).all()
        assert _patched() == outer
        assert torch.isnan(torch.empty(3)).all()              # the outer one is still active
        assert torch.isnan(torch.zeros(1).new_empty(2)).all()
    assert _patched() == before


def test_poison_leaves_other_constructors_alone():
    with poisoned_allocations():
        z, o, f = torch.zeros(4, 3), torch.ones(5, dtype=torch.int32), torch.full((3,), 2.5)
        r = torch.randn(1000, generator=torch.Generator().manual_seed(0))
        a = torch.arange(6)
        n = torch.from_numpy(np.zeros(3, dtype=np.float32))
        zl = torch.zeros_like(r)
    assert (z == 0).all() and (o == 1).all() and (f == 2.5).all() and (zl == 0).all() and (n == 0).all()
    assert torch.isfinite(r).all() and torch.equal(r, torch.randn(1000, generator=torch.Generator().manual_seed(0)))
    assert torch.equal(a, torch.tensor([0, 1, 2, 3, 4, 5]))


@pytest.mark.usefixtures("poisoned_allocations")
def test_poison_fixture_poisons_its_test():
    assert torch.empty.__module__ == poison.__name__ and torch.isnan(torch.empty(2)).all()


def test_poison_fixture_is_undone_after_its_test():
    assert torch.empty.__module__ != poison.__name__ and "new_empty" not in torch.Tensor.__dict__


# ------------------------------------------------------------------------------------- end to end, on the CPU backend

def _stub_gather_rows(table, index, skip_row=None):
    """A kernel wrapper as temp_amd/backend.py writes them: allocate with torch.empty, let the 'kernel' fill it."""
    out = torch.empty(index.numel(), table.shape[1], dtype=table.dtype)
    for i, j in enumerate(index.tolist()):
        if i != skip_row:
            out[i] = table[j]
    return out


def test_unwritten_row_is_caught_under_poison_with_the_strict_compare():
    rng = np.random.default_rng(5)
    table = torch.from_numpy(rng.standard_normal((9, 7)).astype(np.float32))
    index = torch.from_numpy(rng.integers(0, 9, 13))
    want = table.double()[index]
    with poisoned_allocations():
        assert_close(_stub_gather_rows(table, index), want, 0.0, 0.0, "all rows written")
        got = _stub_gather_rows(table, index, skip_row=12)
    assert torch.isnan(got[12]).all() and torch.isfinite(got[:12]).all()
    with pytest.raises(AssertionError, match="7 non-finite in got"):
        assert_close(got, want, 1e-5, 1e-6, "last row skipped")
