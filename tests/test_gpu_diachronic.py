"""The diachronic table kernels (temp_diachronic_rows_fwd / _bwd) and the embedding-only baselines on the MI355X: both routes of
the kernels against fp64 taken of the fp32 two-rounding argument (t = 4016 included: a contracted t w + b fails the forward bar
by 5x and more), overwrite / canary / repeatability, the argument checks; then the model cases of tests/diachronic_cases.py
(goldens G24 / G25, fused against per-graph route, prepared batches, edge batches) on the HIP path."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import diachronic_cases as DC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG = 1

# (B, N, d): one element; the scalar route with ds = 3; d % 4 == 0 but ds = 18 (scalar route); the vector route with ds = 100 and
# several blocks per timestamp; 1030 entities at the shipped width 128; d = 8 (one float4 per half)
CASES = [(1, 1, 2), (3, 37, 6), (3, 37, 36), (8, 300, 200), (2, 1030, 128), (5, 65, 8)]
# times per case: 0, 1 and 4016 (ICEWS05-15's last timestamp) on one case of each route -- (3, 37, 6) scalar, (8, 300, 200) vector
TIMES = {(1, 1, 2): [7.0], (3, 37, 6): [0.0, 1.0, 4016.0], (3, 37, 36): [2.0, 364.0, 11.0],
         (8, 300, 200): [0.0, 1.0, 4016.0, 23.0, 2008.0, 364.0, 4015.0, 3.0], (2, 1030, 128): [4016.0, 12.0], (5, 65, 8): [5.0, 0.0, 100.0, 1.0, 77.0]}


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


_INPUTS = {}


def _inputs(B, N, d):
    """Host inputs and their fp64 expectations, computed once per shape: |w| up to 1 (the argument reaches ~4e3), b in [-pi, pi]."""
    key = (B, N, d)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * B + 10 * N + d)
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        u = lambda lo, hi, *s: torch.from_numpy(rng.uniform(lo, hi, s).astype(np.float32))
        ent, w, b = f(N, d), u(-1.0, 1.0, N, d - d // 2), u(-np.pi, np.pi, N, d - d // 2)
        t = torch.tensor(TIMES[key], dtype=torch.float32)
        d_out = f(B * N, d)
        assert t.shape[0] == B
        _INPUTS[key] = (ent, w, b, t, d_out, DC.table_fp64(ent, w, b, t), DC.adjoint_fp64(ent, w, b, t, d_out))
    return _INPUTS[key]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_times_cover_both_routes():
    for key in ((3, 37, 6), (8, 300, 200)):
        assert {0.0, 1.0, 4016.0} <= set(TIMES[key])
    assert (6 // 2) % 4 != 0 and 200 % 4 == 0 and (200 // 2) % 4 == 0 and 36 % 4 == 0 and (36 // 2) % 4 != 0


@pytest.mark.parametrize("B,N,d", CASES)
def test_forward_vs_fp64(B, N, d, hip_backend):
    """Every element within 2e-6 |ent| of fp64 (the device sine's few ulp of 1 and one product rounding), the static half an exact
    copy; the B N d canary floats behind `out` stay untouched."""
    ent, w, b, t, _, want, _ = _inputs(B, N, d)
    e, wd, bd, td = ent.to(DEV), w.to(DEV), b.to(DEV), t.to(DEV)
    buf = torch.full((2 * B * N, d), -77.0, dtype=torch.float32, device=DEV)
    rc = hip_backend.lib.temp_diachronic_rows_fwd(B, N, d, _p(e), _p(wd), _p(bd), _p(td), _p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    out = buf[:B * N].cpu()
    assert bool((buf[B * N:] == -77.0).all()), "canary"
    ds = d // 2
    assert torch.equal(out[:, :ds], ent.repeat(B, 1)[:, :ds]), "the static half is a copy"
    err = (out.double() - want).abs()
    bar = 2e-6 * ent.abs().double().repeat(B, 1)
    print("fwd (%d, %d, %d): max err / |ent| = %.3g" % (B, N, d, float((err / ent.abs().double().repeat(B, 1).clamp(min=1e-30)).max())))
    assert bool((err <= bar).all())
    assert torch.equal(hip_backend.diachronic_rows_fwd(e, wd, bd, td).cpu(), out), "the backend method is the same launch"


@pytest.mark.parametrize("B,N,d", CASES)
def test_backward_vs_fp64(B, N, d, hip_backend):
    """d_w / d_b within 2e-6 of sum_b |d_out ent| max(1, t_b), d_ent within 2e-6 of sum_b |d_out|; buffers pre-filled with NaN are
    fully overwritten; a second call is bit-equal."""
    ent, w, b, t, d_out, _, ((w_ent, w_w, w_b), (mag_ent, mag_wb)) = _inputs(B, N, d)
    e, wd, bd, td, gd = ent.to(DEV), w.to(DEV), b.to(DEV), t.to(DEV), d_out.to(DEV)
    runs = []
    for _ in range(2):
        d_ent, d_w, d_b = [torch.full_like(x, float("nan")) for x in (e, wd, bd)]
        rc = hip_backend.lib.temp_diachronic_rows_bwd(B, N, d, _p(e), _p(wd), _p(bd), _p(td), _p(gd), _p(d_ent), _p(d_w), _p(d_b), None)
        torch.cuda.synchronize()
        assert rc == 0
        runs.append([x.cpu() for x in (d_ent, d_w, d_b)])
    for a, c in zip(*runs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, c)
    for got, want, mag, what in zip(runs[0], (w_ent, w_w, w_b), (mag_ent, mag_wb, mag_wb), ("d_ent", "d_w", "d_b")):
        err = (got.double() - want).abs()
        print("bwd (%d, %d, %d) %s: max err / magnitude = %.3g" % (B, N, d, what, float((err / mag.clamp(min=1e-30)).max())))
        assert bool((err <= 2e-6 * mag).all()), what
    for a, c in zip(hip_backend.diachronic_rows_bwd(e, wd, bd, td, gd), runs[0]):
        assert torch.equal(a.cpu(), c)


def test_bad_arguments_launch_nothing(hip_backend):
    lib = hip_backend.lib
    x = torch.zeros(64, device=DEV)
    out = torch.full((64,), 5.0, device=DEV)
    for B, N, d in ((0, 4, 4), (2, 0, 4), (2, 4, 1), (-1, 4, 4)):
        assert lib.temp_diachronic_rows_fwd(B, N, d, _p(x), _p(x), _p(x), _p(x), _p(out), None) == E_BADARG
        assert lib.temp_diachronic_rows_bwd(B, N, d, _p(x), _p(x), _p(x), _p(x), _p(x), _p(out), _p(out), _p(out), None) == E_BADARG
    assert lib.temp_diachronic_rows_fwd(2, 4, 4, _p(x), None, _p(x), _p(x), _p(out), None) == E_BADARG
    assert lib.temp_diachronic_rows_bwd(2, 4, 4, _p(x), _p(x), _p(x), _p(x), _p(x), _p(out), None, _p(out), None) == E_BADARG
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    with pytest.raises(_lib.TempAmdError):
        hip_backend.diachronic_rows_fwd(x.view(16, 4), x[:16].view(16, 1), x[:16].view(16, 1), x[:2])


def test_kernels_are_traced_by_name(hip_backend):
    lib = hip_backend.lib
    ent, w, b, t, d_out, _, _ = _inputs(3, 37, 6)
    e, wd, bd, td, gd = ent.to(DEV), w.to(DEV), b.to(DEV), t.to(DEV), d_out.to(DEV)
    ids, ms, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)(), ctypes.c_int32()
    _lib.check(lib.temp_trace_begin(16), "temp_trace_begin")
    try:
        hip_backend.diachronic_rows_bwd(e, wd, bd, td, gd)
        hip_backend.diachronic_rows_fwd(e, wd, bd, td)
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 16, ctypes.byref(cnt)), "temp_trace_end")
    assert [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)] == ["k_diachronic_bwd", "k_diachronic_fwd"]


def test_node_equals_torch_composition():
    DC.check_node(DEV)


@pytest.mark.parametrize("name", DC.G24)
def test_g24_tables_loss_gradients(name):
    DC.check_g24(name, DEV)


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_state_dict_is_the_references(name):
    DC.check_state_dict(name, DEV)


@pytest.mark.parametrize("name", DC.G25)
def test_g25_evaluate(name):
    DC.check_g25(name, DEV)


@pytest.mark.parametrize("name,kind", [("G24_de_complex", "complex"), ("G24_de_complex", "distmult"), ("G24_de_complex", "transE"),
                                       ("G24_static_complex", "complex")])
def test_fused_route_equals_per_graph(name, kind):
    n_fwd, n_bwd = DC.check_fused_equals_per_graph(name, DEV, kind)
    assert (n_fwd, n_bwd) == ((1, 1) if "de" in name else (0, 0)), "one table launch each way for the whole batch"


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_prepared_batch_is_repeatable(name):
    DC.check_prepared_repeatable(name, DEV)


@pytest.mark.parametrize("name", ["G24_de_complex", "G24_static_complex"])
def test_edge_batches(name):
    DC.check_edge_batches(name, DEV)
