"""temp_frozen_mix_ce (the one-launch loss of two frozen streams, csrc/gated_loss.hip) through the C ABI against an fp64 evaluation
of its formula on the same fp32 inputs: the logsumexp, and autograd for d_w.

Error bars.  Loss rows: (rtol 2e-5, atol 2e-6), the bars of test_gather_ce_mix_kernels_vs_fp64 at magnitude 1.  d_w:
|err| <= 2e-5 |want| + 2e-6 (1 + max_c |a_c - b_c|), every value compared NaN-strictly.  A CPU simulation of the kernel's arithmetic (a
sequential fp32 dot, an fp32 online logsumexp; D up to 256, C up to 1 025, |score| up to ~10) used at most 0.1 of either bar; the inputs
here are scaled so that |score| = O(1)."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
DOT, L1 = 0, 1
KIND_NAME = {DOT: "dot", L1: "l1"}

# (P, C, Da, Db, rows)
SHAPES = {
    "smallest": (9, 7, 8, 12, 40),            # P % 4 != 0, unequal widths, rows narrower than a lane group
    "project": (33, 101, 200, 128, 500),      # the project's widths; C is no multiple of the four groups
    "long_list": (6, 1030, 64, 64, 3000),     # more than one 64-candidate chunk per wave, a ragged last one
    "single": (5, 1, 16, 16, 8),              # one candidate: loss 0 within the bar, d_w exactly 0
    "widest": (4, 5, 512, 512, 64),           # the upper width edge
}


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _call(P, C, Da, Db, kind, q_a, T_a, q_b, T_b, w, cand, row_scale, inv_rows, loss, d_w):
    rc = _lib.load().temp_frozen_mix_ce(P, C, Da, Db, kind, _ptr(q_a), _ptr(T_a), _ptr(q_b), _ptr(T_b), _ptr(w), _ptr(cand), _ptr(row_scale),
                                        float(inv_rows), _ptr(loss), _ptr(d_w), None)
    torch.cuda.synchronize()
    return rc


def _traced(fn):
    lib = _lib.load()
    ids, ms, cnt = (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)(), ctypes.c_int32(0)
    _lib.check(lib.temp_trace_begin(64), "temp_trace_begin")
    try:
        out = fn()
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 64, ctypes.byref(cnt)), "temp_trace_end")
    return out, [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)]


def _candidates(P, C, rows, g):
    """As _candidates of tests/test_gpu_row_loss_routes.py (duplicates, the truth listed twice), over a table that is a stack of two
    windows of rows // 2 entities: odd rows take their candidates from the second window."""
    n = rows // 2
    cand = torch.randint(0, n, (P, C), generator=g).int()
    if C > 2:
        cand[:, 2] = cand[:, 1]
        cand[::3, 1] = cand[::3, 0]
    cand[1::2] += n
    return cand


def _inputs(shape, kind, seed=0):
    P, C, Da, Db, rows = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    def mk(n, d):
        # dot: <q, t> ~ N(0, 1); l1: |q - t|_1 = O(1)
        s = d ** -0.25 if kind == DOT else 1.0 / d
        return torch.randn(n, d, generator=g) * s
    q_a, T_a, q_b, T_b = mk(P, Da), mk(rows, Da), mk(P, Db), mk(rows, Db)
    w = torch.sigmoid(torch.randn(P, generator=g))
    row_scale = torch.rand(P, generator=g) + 0.1
    return dict(q_a=q_a, T_a=T_a, q_b=q_b, T_b=T_b, w=w, cand=_candidates(P, C, rows, g), row_scale=row_scale)


def _scores64(q, T, cand, kind):
    rows = T.double()[cand.long()]
    qs = q.double().unsqueeze(1)
    return (qs * rows).sum(-1) if kind == DOT else -(qs - rows).abs().sum(-1)


def _reference(x, kind, scale):
    """fp64 on the fp32 inputs -> (loss_rows, d_w, max_c |a_c - b_c| per row)."""
    w = x["w"].double().requires_grad_(True)
    loss = TF.frozen_mix_ce_rows(x["q_a"].double(), x["T_a"].double(), x["q_b"].double(), x["T_b"].double(), w, x["cand"], KIND_NAME[kind])
    d_w, = torch.autograd.grad((loss * scale.double()).sum(), w)
    spread = (_scores64(x["q_a"], x["T_a"], x["cand"], kind) - _scores64(x["q_b"], x["T_b"], x["cand"], kind)).abs().max(dim=1).values
    return loss.detach(), d_w, spread


def _run(shape, kind, x, row_scale, inv_rows=0.0):
    P, C, Da, Db, _ = SHAPES[shape]
    d = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in x.items()}
    loss = torch.full((P,), float("nan"), device=DEV)
    d_w = torch.full((P,), float("nan"), device=DEV)
    rc = _call(P, C, Da, Db, kind, d["q_a"], d["T_a"], d["q_b"], d["T_b"], d["w"], d["cand"], d["row_scale"] if row_scale else None, inv_rows,
               loss, d_w)
    assert rc == 0
    return loss.cpu(), d_w.cpu()


def _check(got, want, tol, what):
    """|got - want| <= tol element by element, NaN-strict: a non-finite element on either side fails."""
    g, w = got.double(), want.double()
    assert g.shape == w.shape, what
    assert bool(torch.isfinite(w).all()), "%s: the reference is not finite" % what
    assert bool(torch.isfinite(g).all()), "%s: %d non-finite elements" % (what, int((~torch.isfinite(g)).sum()))
    err = (g - w).abs()
    bad = err > tol
    print("%s: max err / bar = %.3g" % (what, float((err / tol).max()) if g.numel() else 0.0))
    assert not bool(bad.any()), "%s: %d elements outside the bar, worst err %.3e at bar %.3e" % (
        what, int(bad.sum()), float(err[bad].max()), float(tol[bad][err[bad].argmax()]))


def _check_pair(loss, d_w, ref, what):
    want_loss, want_dw, spread = ref
    _check(loss, want_loss, 2e-6 + 2e-5 * want_loss.abs(), what + " loss rows")
    _check(d_w, want_dw, 2e-5 * want_dw.abs() + 2e-6 * (1 + spread), what + " d_w")


@pytest.mark.parametrize("scaled", [False, True], ids=["inv_rows", "row_scale"])
@pytest.mark.parametrize("kind", [DOT, L1], ids=["dot", "l1"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frozen_mix_ce_vs_fp64(shape, kind, scaled):
    P = SHAPES[shape][0]
    x = _inputs(shape, kind)
    inv_rows = 1.0 / 7
    scale = x["row_scale"] if scaled else torch.full((P,), inv_rows)
    (loss, d_w), names = _traced(lambda: _run(shape, kind, x, scaled, inv_rows))
    assert names == ["k_frozen_mix_ce"]
    _check_pair(loss, d_w, _reference(x, kind, scale), "%s/%s" % (shape, KIND_NAME[kind]))
    if shape == "single":
        assert bool((d_w == 0).all()), "one candidate: d_w must be exactly 0"
    again = _run(shape, kind, x, scaled, inv_rows)
    assert torch.equal(loss, again[0]) and torch.equal(d_w, again[1]), "two launches must give bit-identical outputs"


@pytest.mark.parametrize("kind", [DOT, L1], ids=["dot", "l1"])
@pytest.mark.parametrize("w_val", [0.0, 1.0])
def test_weight_at_the_ends_is_the_single_table_ce(kind, w_val):
    """w exactly 0 / 1: no NaN, and the loss rows are the CE of the one table that is left, within the bars."""
    shape = "project"
    x = _inputs(shape, kind, seed=3)
    x["w"] = torch.full_like(x["w"], w_val)
    loss, d_w = _run(shape, kind, x, True)
    _check_pair(loss, d_w, _reference(x, kind, x["row_scale"]), "w=%g/%s" % (w_val, KIND_NAME[kind]))
    s = _scores64(x["q_a"], x["T_a"], x["cand"], kind) if w_val == 1.0 else _scores64(x["q_b"], x["T_b"], x["cand"], kind)
    single = torch.logsumexp(s, dim=1) - s[:, 0]
    _check(loss, single, 2e-6 + 2e-5 * single.abs(), "w=%g single-table CE" % w_val)


@pytest.mark.parametrize("Da,Db", [(6, 8), (8, 516)])
def test_unsupported_widths_touch_nothing(Da, Db):
    P, C, rows = 3, 4, 10
    q_a, T_a, q_b, T_b = (torch.zeros(n, d, device=DEV) for n, d in ((P, Da), (rows, Da), (P, Db), (rows, Db)))
    w = torch.full((P,), 0.5, device=DEV)
    cand = torch.zeros(P, C, dtype=torch.int32, device=DEV)
    loss, d_w = torch.full((P,), 7.0, device=DEV), torch.full((P,), -3.0, device=DEV)
    rc, names = _traced(lambda: _call(P, C, Da, Db, DOT, q_a, T_a, q_b, T_b, w, cand, None, 1.0, loss, d_w))
    assert rc == 2 and names == []
    assert bool((loss == 7.0).all()) and bool((d_w == -3.0).all())


def test_no_rows_no_launch():
    e = torch.zeros(0, 8, device=DEV)
    T = torch.zeros(4, 8, device=DEV)
    z = torch.zeros(0, device=DEV)
    rc, names = _traced(lambda: _call(0, 3, 8, 8, DOT, e, T, e, T, z, torch.zeros(0, 3, dtype=torch.int32, device=DEV), None, 1.0, z, z))
    assert rc == 0 and names == []


def test_backend_call_matches_the_abi(hip_backend):
    x = _inputs("smallest", DOT)
    want = _run("smallest", DOT, x, True)
    d = {k: v.to(DEV) for k, v in x.items()}
    got = hip_backend.frozen_mix_ce(d["q_a"], d["T_a"], d["q_b"], d["T_b"], d["w"], d["cand"], d["row_scale"], None, "dot")
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    with pytest.raises(ValueError):
        hip_backend.frozen_mix_ce(d["q_a"], d["T_a"], d["q_b"], d["T_b"], d["w"][:-1], d["cand"], None, None, "dot")
