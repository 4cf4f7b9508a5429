"""The hyperplane projection kernels (temp_hyperplane_rows_fwd / _bwd) and the HyTE baseline on the MI355X: every route of the
kernels against fp64 with derived error bars, overwrite / canary / repeatability, the argument and workspace checks, exact cases;
then the node and model cases of tests/hyte_cases.py (goldens G26 / G27, fused against per-graph route, prepared batches, edge
batches, per-window relation rows, predict()) on the HIP path.

Error bars (u = 2^-24).  A row dot of d products is a chain of at most d roundings (4 fused multiply-adds per lane, a butterfly over
the lanes) and n = w / |w| carries a few more from the sum of squares, the square root, the division and the product:
  forward   (2 d + 16) u (|e_ik| + |n_k| sum_j |n_j e_ij|)
  backward  (2 d + 16 + L) u (sum of the absolute terms of the exact expression, hyte_cases.adjoint_fp64), L = hyte_cases.chain_length(N)
            = TEMP_HYPERPLANE_TILE_ROWS + number of tiles: the additions a d_w element goes through in the tile and in the finishing
            kernel (d_table's chain, the B timestamps, is shorter for every shape here)."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from tests import hyte_cases as HC
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG = 1

# (B, N, d).  Routes: d % 4 == 0 -> float4 columns, else one float per lane; 16 / 32 / 64 lanes per row by the row's width in such
# columns; more than 64 columns -> the column-loop kernels.
CASES = [(1, 1, 1),                       # one element (scalar, 16 lanes)
         (3, 37, 6),                      # scalar route, two tiles with a ragged second
         (3, 37, 36),                     # float4, 9 columns -> 16 lanes
         (5, 65, 8),                      # three tiles, the last with one row
         (8, 300, 200),                   # float4, 50 columns -> 64 lanes; a full chunk of normals
         (2, 1030, 128),                  # float4, 32 columns -> 32 lanes; 33 tiles: more than one block
         (HC.CHUNK + 1, 40, 8),           # one normal more than a chunk: d_table goes through memory between the chunks
         (2, 3 * HC.TILE_ROWS + 1, 12),   # three full tiles + 1 row: the finishing kernel adds four partials
         (2, 33, 18), (2, 33, 50),        # scalar route on 32 and on 64 lanes
         (HC.CHUNK + 1, 35, 260),         # float4 column loop (65 columns), two chunks, two tiles
         (2, 5, 67)]                      # scalar column loop


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


_INPUTS = {}


def _inputs(B, N, d):
    """Host inputs and their fp64 expectations, computed once per shape."""
    key = (B, N, d)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * B + 10 * N + d)
        f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        table, w, d_out = f(N, d), HC.scaled_normals(rng, B, d), f(B * N, d)
        _INPUTS[key] = (table, w, d_out, HC.table_fp64(table, w), HC.adjoint_fp64(table, w, d_out))
    return _INPUTS[key]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _ws(lib, B, N, d):
    nb = lib.temp_hyperplane_rows_bwd_workspace(B, N, d)
    assert nb == -(-N // HC.TILE_ROWS) * B * d * 4, "the documented formula"
    return torch.full((nb // 4,), float("nan"), dtype=torch.float32, device=DEV), nb


def test_norms_span_the_range():
    _, w, _, _, _ = _inputs(8, 300, 200)
    norms = w.norm(dim=1)
    assert abs(float(norms.min()) - 0.05) < 1e-3 and abs(float(norms.max()) - 20.0) < 1e-2


@pytest.mark.parametrize("B,N,d", CASES)
def test_forward_vs_fp64(B, N, d, hip_backend):
    """Every element within its bar of fp64; the B N d canary floats behind `out` stay untouched."""
    table, w, _, (want, bar), _ = _inputs(B, N, d)
    e, wd = table.to(DEV), w.to(DEV)
    buf = torch.full((2 * B * N, d), -77.0, dtype=torch.float32, device=DEV)
    rc = hip_backend.lib.temp_hyperplane_rows_fwd(B, N, d, _p(e), _p(wd), _p(buf), None)
    torch.cuda.synchronize()
    assert rc == 0
    out = buf[:B * N].cpu()
    assert bool((buf[B * N:] == -77.0).all()), "canary"
    err = (out.double() - want).abs()
    print("fwd (%d, %d, %d): max err / bar = %.3g" % (B, N, d, float((err / bar.clamp(min=1e-300)).max())))
    assert bool((err <= bar).all())
    assert torch.equal(hip_backend.hyperplane_rows_fwd(e, wd).cpu(), out), "the backend method is the same launch"


@pytest.mark.parametrize("B,N,d", CASES)
def test_backward_vs_fp64(B, N, d, hip_backend):
    """d_table and d_w within (2 d + 16 + L) u of their sums of absolute terms; NaN-prefilled outputs (and workspace) are fully
    overwritten; a second call is bit-equal."""
    table, w, d_out, _, ((w_table, w_w), (mag_table, mag_w)) = _inputs(B, N, d)
    e, wd, gd = table.to(DEV), w.to(DEV), d_out.to(DEV)
    lib = hip_backend.lib
    runs = []
    for _ in range(2):
        d_table, d_w = torch.full_like(e, float("nan")), torch.full_like(wd, float("nan"))
        ws, nb = _ws(lib, B, N, d)
        rc = lib.temp_hyperplane_rows_bwd(B, N, d, _p(e), _p(wd), _p(gd), _p(d_table), _p(d_w), _p(ws), nb, None)
        torch.cuda.synchronize()
        assert rc == 0
        assert not bool(torch.isnan(ws).any()), "every tile partial is written"
        runs.append([x.cpu() for x in (d_table, d_w)])
    for a, c in zip(*runs):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, c)
    k = (2 * d + 16 + HC.chain_length(N)) * HC.U
    for got, want, mag, what in zip(runs[0], (w_table, w_w), (mag_table, mag_w), ("d_table", "d_w")):
        err = (got.double() - want).abs()
        print("bwd (%d, %d, %d) %s: max err / bar = %.3g" % (B, N, d, what, float((err / (k * mag).clamp(min=1e-300)).max())))
        assert bool((err <= k * mag).all()), what
    for a, c in zip(hip_backend.hyperplane_rows_bwd(e, wd, gd), runs[0]):
        assert torch.equal(a.cpu(), c)


@pytest.mark.parametrize("d", [8, 6])
def test_exact_rows(d, hip_backend):
    """A table row that is 2^3 times w_b projects to (nearly) nothing under b: |out| within the bar.  A row whose support is disjoint
    from w_b's is orthogonal to it in exact arithmetic -- every product of the dot is an exact zero -- and comes back bit-equal."""
    rng = np.random.default_rng(d)
    w = HC.scaled_normals(rng, 2, d)
    w[1, :d // 2] = 0.0                                            # w_1 lives on the second half of the columns
    table = torch.from_numpy(rng.standard_normal((4, d)).astype(np.float32))
    table[0] = 8.0 * w[0]
    table[1, d // 2:] = 0.0                                        # row 1 lives on the first half
    out = hip_backend.hyperplane_rows_fwd(table.to(DEV), w.to(DEV)).cpu()
    _, bar = HC.table_fp64(table, w)
    assert bool((out[0].abs().double() <= bar[0]).all()), "the multiple of w_0 under normal 0"
    assert torch.equal(out[4 + 1], table[1]), "the row orthogonal to w_1 under normal 1"


def test_bad_arguments_launch_nothing(hip_backend):
    lib = hip_backend.lib
    x = torch.zeros(256, device=DEV)
    out = torch.full((256,), 5.0, device=DEV)
    big = 1 << 20
    for B, N, d in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4)):
        assert lib.temp_hyperplane_rows_bwd_workspace(B, N, d) == 0
        assert lib.temp_hyperplane_rows_fwd(B, N, d, _p(x), _p(x), _p(out), None) == E_BADARG
        assert lib.temp_hyperplane_rows_bwd(B, N, d, _p(x), _p(x), _p(x), _p(out), _p(out), _p(out), big, None) == E_BADARG
    assert lib.temp_hyperplane_rows_fwd(2, 4, 4, _p(x), None, _p(out), None) == E_BADARG
    assert lib.temp_hyperplane_rows_bwd(2, 4, 4, _p(x), _p(x), _p(x), _p(out), None, _p(out), big, None) == E_BADARG
    need = lib.temp_hyperplane_rows_bwd_workspace(2, 40, 4)
    assert need == 2 * 2 * 4 * 4
    assert lib.temp_hyperplane_rows_bwd(2, 40, 4, _p(x), _p(x), _p(x), _p(out), _p(out), _p(out), need - 1, None) == E_BADARG, "short workspace"
    assert lib.temp_hyperplane_rows_bwd(2, 40, 4, _p(x), _p(x), _p(x), _p(out), _p(out), None, need, None) == E_BADARG, "no workspace"
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    with pytest.raises(_lib.TempAmdError):
        hip_backend.hyperplane_rows_fwd(x[:64].view(16, 4), x[:10].view(2, 5))


def test_kernels_are_traced_by_name(hip_backend):
    lib = hip_backend.lib
    table, w, d_out, _, _ = _inputs(3, 37, 6)
    e, wd, gd = table.to(DEV), w.to(DEV), d_out.to(DEV)
    ids, ms, cnt = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)(), ctypes.c_int32()
    _lib.check(lib.temp_trace_begin(16), "temp_trace_begin")
    try:
        hip_backend.hyperplane_rows_bwd(e, wd, gd)
        hip_backend.hyperplane_rows_fwd(e, wd)
    finally:
        _lib.check(lib.temp_trace_end(ids, ms, 16, ctypes.byref(cnt)), "temp_trace_end")
    assert [lib.temp_trace_kernel_name(ids[i]).decode() for i in range(cnt.value)] == \
        ["k_hyperplane_bwd", "k_hyperplane_bwd_finish", "k_hyperplane_fwd"]


def test_node_equals_torch_composition():
    HC.check_node(DEV)


def test_repeated_timestamp_sums_its_rows():
    HC.check_repeated_timestamp(DEV)


def test_plan_rel_stride():
    HC.check_plan_rel_stride(DEV)


def test_state_dict_is_the_references():
    HC.check_state_dict(DEV)


def test_g26_tables_loss_gradients():
    HC.check_g26(DEV)


def test_g27_evaluate():
    HC.check_g27(DEV)


@pytest.mark.parametrize("n_times", [3, 1])
def test_fused_route_equals_per_graph(n_times):
    z = HC.load("G26_hyte")
    t_list = torch.tensor([int(t) for t in z["t_list"]][:n_times])
    assert HC.check_fused_equals_per_graph(DEV, t_list) == (2, 2), "two projection launches each way, whatever B is"


def test_prepared_batch_is_repeatable():
    HC.check_prepared_repeatable(DEV)


def test_edge_batches():
    HC.check_edge_batches(DEV)


def test_query_uses_window_relation_rows():
    HC.check_query_uses_window_relation_rows(DEV)


def test_predict():
    HC.check_predict(DEV)
