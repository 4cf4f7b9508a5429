"""Split-row history attention (temp_sa_attn_split_fwd / _bwd) and the post-aggregation attention models on the MI355X: the split
kernels bit for bit against temp_sa_attn_fwd / _bwd fed the fp32 sum of the two rows, and independently against the dense softmax
formulation; the sums into the two tables' gradients against fp64; the argument checks; then the model cases of
tests/post_attention_cases.py (goldens G22 / G23, split against unsplit route, scorers, edge windows) on the HIP path."""
import ctypes

import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import post_attention_cases as PC
from tests.cpu_backend import CpuTestBackend
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG, E_UNSUPPORTED = 1, 2

# (n, R, T, D, rows of pa, rows of pb, decay): d_k = 1 .. 64 (every per-lane column count), ragged d_k = 25, T = 1, n no multiple
# of the 4 rows of a block, one block and several, repeated ia
CASES = [(1, 1, 1, 8, 1, 1, False), (37, 50, 6, 32, 11, 3, True), (65, 10, 4, 64, 65, 1, True), (301, 700, 29, 200, 97, 4, True),
         (33, 9, 3, 512, 5, 2, False)]


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    yield TB.get_backend()
    TB.set_backend(None)


def _inputs(n, R, T, D, na, nb, decay):
    rng = np.random.default_rng(n * 7 + T)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    pa, pb, kvh, d_out = f(na, 3 * D), f(nb, 3 * D), f(R, 2 * D), f(n, D)
    ia = torch.from_numpy(rng.integers(0, na, n).astype(np.int32))
    ib = torch.from_numpy(rng.integers(0, nb, n).astype(np.int32))
    if na >= n:
        ia = torch.from_numpy(rng.permutation(na)[:n].astype(np.int32))          # (65 rows of pa for 65 query rows: each once)
    idx = rng.integers(0, R, (n, T - 1)).astype(np.int32)
    idx[rng.random((n, T - 1)) < 0.6] = -1
    if n > 2 and T > 1:
        idx[0] = -1                                # all history masked: only the current position is alive
        idx[1] = 0                                 # every position reads history row 0
    dec = torch.from_numpy(-rng.random(T).astype(np.float32)) if decay else None
    return pa, ia, pb, ib, kvh, torch.from_numpy(idx), dec, d_out


@pytest.mark.parametrize("n,R,T,D,na,nb,decay", CASES)
def test_split_attention_kernels(n, R, T, D, na, nb, decay, hip_backend):
    be = hip_backend
    host = _inputs(n, R, T, D, na, nb, decay)
    pa, ia, pb, ib, kvh, idx, dec, d_out = [t.to(DEV) if t is not None else None for t in host]
    qkv = pa[ia.long()] + pb[ib.long()]                        # the fp32 sum, rounded once per element
    # forward: bit-equal to the unsplit kernel on the sum (the split kernel forms the same fp32 row, then identical arithmetic)
    out, score, lse = be.sa_attn_split_fwd(pa, ia, pb, ib, kvh, idx, dec)
    w_out, w_score, w_lse = be.sa_attn_fwd(qkv, kvh, idx, dec)
    assert torch.equal(out, w_out) and torch.equal(lse, w_lse)
    assert torch.equal(score.view(torch.int32), w_score.view(torch.int32))          # (bit patterns: -inf where masked)
    # ... and against the dense formulation, at the bars of test_history_attention_kernel_vs_dense
    cpu = CpuTestBackend()
    h_qkv = host[0][host[1].long()] + host[2][host[3].long()]
    c_out, c_score, c_lse = cpu.sa_attn_fwd(h_qkv, host[4], host[5], host[6])
    assert_close(out, c_out, 1e-5, 2e-6, "split attn out")
    assert_close(lse, c_lse, 1e-5, 2e-6, "split attn lse")
    live = torch.isfinite(c_score)
    assert torch.equal(torch.isfinite(score).cpu(), live)
    assert_close(torch.where(live, score.cpu(), torch.zeros(())), torch.where(live, c_score, torch.zeros(())), 1e-5, 2e-6, "split attn score")
    # backward, atomic form: the per-row gradient of the summed current row is bit-equal
    g = be.sa_attn_split_bwd(pa, ia, pb, ib, kvh, idx, dec, out, score, lse, d_out)
    w = be.sa_attn_bwd(qkv, kvh, idx, dec, out, score, lse, d_out)
    c = cpu.sa_attn_bwd(h_qkv, host[4], host[5], host[6], c_out, c_score, c_lse, host[7])
    assert tuple(g[0].shape) == (n, 3 * D) and torch.equal(g[0], w[0])
    assert_close(g[0], c[0], 2e-5, 3e-6, "split d_qkv")
    assert_close(g[1], c[1], 2e-5, 3e-6, "split d_kv_hist (atomics)")
    if decay:
        assert_close(g[2], c[2], 5e-5, 2e-5, "split d_decay")
    else:
        assert g[2] is None
    if T > 1:                                                  # table-pass form: the history gradient is bit-equal too
        inv = TF.attention_inverse(host[5].numpy(), R, DEV)
        g1 = be.sa_attn_split_bwd(pa, ia, pb, ib, kvh, idx, dec, out, score, lse, d_out, inv)
        w1 = be.sa_attn_bwd(qkv, kvh, idx, dec, out, score, lse, d_out, inv)
        assert torch.equal(g1[0], w1[0]) and torch.equal(g1[1], w1[1])
        assert_close(g1[1], c[1], 2e-5, 3e-6, "split d_kv_hist (table pass)")
    else:
        inv = None
    # the autograd node: d_pa / d_pb = the per-row gradient summed over ia / ib, against fp64; output, d_pa, d_pb and the history
    # gradient repeat bit for bit
    inv_a, inv_b = TF.split_row_inverse(host[1].numpy(), na, DEV), TF.split_row_inverse(host[3].numpy(), nb, DEV)
    runs = []
    for _ in range(2):
        leaves = [pa.clone().requires_grad_(True), pb.clone().requires_grad_(True), kvh.clone().requires_grad_(True)]
        dl = dec.clone().requires_grad_(True) if decay else None
        o = TF.split_history_attention(leaves[0], ia, leaves[1], ib, leaves[2], idx, dl, inv, inv_a, inv_b)
        o.backward(d_out)
        runs.append([o.detach()] + [x.grad for x in leaves])       # (not d_decay: T values summed with atomics, as in the unsplit kernel)
    assert torch.equal(runs[0][0], out)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "not repeatable"
    rows64 = (g1[0] if T > 1 else g[0]).double().cpu()
    for got, index, n_tab, what in ((runs[0][1], host[1], na, "d_pa"), (runs[0][2], host[3], nb, "d_pb")):
        want = torch.zeros(n_tab, 3 * D, dtype=torch.float64).index_add_(0, index.long(), rows64)
        mag = torch.zeros(n_tab, 3 * D, dtype=torch.float64).index_add_(0, index.long(), rows64.abs())
        m = torch.bincount(index.long(), minlength=n_tab).double().view(-1, 1)
        err = (got.double().cpu() - want).abs()
        assert bool((err <= m * 2.0 ** -24 * mag).all()), (what, float((err - m * 2.0 ** -24 * mag).max()))
    if T > 1:
        assert torch.equal(runs[0][3], g1[1])


def _desc(n, D, T, heads=8):
    a = _lib.TempAttn()
    a.n, a.D, a.heads, a.T = n, D, heads, T
    return a


def test_split_attention_arguments(hip_backend):
    lib = hip_backend.lib
    D, n, T = 32, 5, 3
    t = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    pa, pb, kvh = t(4, 3 * D), t(2, 3 * D), t(6, 2 * D)
    ia = torch.zeros(n, dtype=torch.int32, device=DEV)
    idx = torch.full((n, T - 1), -1, dtype=torch.int32, device=DEV)
    out, score, lse = t(n, D), t(n, 8, T), t(n, 8)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())

    def split(with_ia=True):
        s = _lib.TempAttnSplit()
        s.pa, s.lda, s.pb, s.ldb = pa.data_ptr(), 3 * D, pb.data_ptr(), 3 * D
        s.ia = ia.data_ptr() if with_ia else None
        s.ib = ia.data_ptr() if with_ia else None
        return s

    def fwd(a, s):
        a.kh, a.vh, a.ldh, a.idx = kvh.data_ptr(), kvh.data_ptr() + 4 * D, 2 * D, idx.data_ptr()
        return lib.temp_sa_attn_split_fwd(ctypes.byref(a), ctypes.byref(s) if s is not None else None, vp(out), vp(score), vp(lse), None)

    assert fwd(_desc(n, D, T), split()) == 0                                 # q / kc / vc NULL: not read
    assert fwd(_desc(0, D, T), split(False)) == 0                            # n = 0 succeeds
    assert fwd(_desc(n, D, T, heads=4), split()) == E_UNSUPPORTED
    assert fwd(_desc(n, 36, T), split()) == E_UNSUPPORTED                    # D % 8 != 0
    assert fwd(_desc(n, D, 65), split()) == E_UNSUPPORTED                    # T > 64
    assert fwd(_desc(n, D, T), split(False)) == E_BADARG                     # NULL ia / ib with n > 0
    assert fwd(_desc(n, D, T), None) == E_BADARG
    a = _desc(n, D, T)
    a.kh, a.vh, a.ldh, a.idx = kvh.data_ptr(), kvh.data_ptr() + 4 * D, 2 * D, idx.data_ptr()
    d_qkv, d_hist = t(n, 3 * D), t(6, 2 * D)
    bwd = lambda a, s, n_: lib.temp_sa_attn_split_bwd(ctypes.byref(a), ctypes.byref(s), vp(out), vp(score), vp(lse), vp(out), vp(d_qkv), n_,
                                                      vp(d_hist), ctypes.c_void_p(d_hist.data_ptr() + 4 * D), 2 * D, None, 6, None, None, None, None)
    assert bwd(a, split(False), 3 * D) == E_BADARG
    assert bwd(a, split(), 3 * D - 4) == E_BADARG                            # the gradient rows hold (d_q | d_k | d_v)
    a0 = _desc(0, D, T)
    assert bwd(a0, split(False), 3 * D) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
G22 = ("G22_post_sa_uni", "G22_post_sa_bi", "G22_post_sa_uni_learn")


@pytest.mark.parametrize("name", G22)
def test_g22_streams_loss_gradients_gpu(name):
    PC.check_g22(name, DEV)


def test_injected_gates_gpu():
    PC.check_injected_gates("G22_post_sa_bi", DEV)


@pytest.mark.parametrize("name", ["G23_eval_post_sa_uni", "G23_eval_post_sa_bi"])
def test_g23_evaluate_gpu(name):
    PC.check_g23(name, DEV)


@pytest.mark.parametrize("name", G22)
def test_split_route_equals_unsplit_gpu(name):
    PC.check_split_route(name, DEV)


@pytest.mark.parametrize("kind", ["distmult", "complex", "transE"])
def test_scorers_take_their_fused_nodes_gpu(kind, hip_backend):
    assert hasattr(hip_backend, "gated_query_fwd") and hasattr(hip_backend, "gather_ce_mix_fwd") and hasattr(hip_backend, "l1_mix_ce_fwd")
    PC.check_scorer("G22_post_sa_bi", DEV, kind)


def test_construction_gpu():
    PC.check_construction(DEV)


def test_use_embed_for_non_active_is_ignored_gpu():
    PC.check_embed_for_non_active_ignored("G22_post_sa_uni", DEV)


@pytest.mark.parametrize("bi", [False, True])
def test_edge_windows_gpu(bi):
    PC.check_edge_windows(DEV, bi)
