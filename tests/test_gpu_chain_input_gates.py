"""The chain forward with the input gates computed inside (temp_gru_chain_fwd's x route): x rows in, no gi, no gate GEMM.

Against the gi route it replaces (the gate GEMM + temp_gru_chain_fwd, forced with gru_chain.FUSED_INPUT_GATES = False or TEMP_DEBUG
bit 22) and against the CPU panel reference of the test backend."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import gru_chain as GC
from temp_amd.gru_chain import GruInstance, GruProgram
from tests.chain_cases import make_rnns, random_program
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
FWD_X_OFF = 1 << 22          # TEMP_DEBUG bit: callers take the gi route


def _launches():
    return _lib.load().temp_gru_chain_fwd_x_launches()


def _run(prog, x, rnns, device, want=None, fused=True, seed=17, between=None):
    """-> (outputs of the wanted instances, d_x, [grads of every GRU parameter]) of gru_chain on the given x rows.
    between: called after the forward, before the backward."""
    g = torch.Generator().manual_seed(seed)
    leaf = x.detach().clone().to(device).requires_grad_(True)
    mods = [m.to(device) for m in rnns]
    for m in mods:
        m.zero_grad()
    old = GC.FUSED_INPUT_GATES
    GC.FUSED_INPUT_GATES = fused
    try:
        out = GC.gru_chain(leaf, prog, mods, 0.1, False, want)
        outs = [out[it.h0:it.h0 + it.n] for it in prog.inst] if want is None else list(out)
        loss = 0
        for k, o in enumerate(outs):
            loss = loss + (o * torch.randn(o.shape, generator=g).to(device)).sum() * (k + 1)
        if between is not None:
            between()
        loss.backward()
    finally:
        GC.FUSED_INPUT_GATES = old
    return [o.detach().cpu() for o in outs], leaf.grad.detach().cpu(), [p.grad.detach().cpu().clone() for m in mods for p in m.parameters()]


def _cpu(prog, x, rnns, want):
    from tests.cpu_backend import CpuTestBackend
    TB.set_backend(CpuTestBackend())
    try:
        prog.__dict__.pop("_chain_tabs", None)
        prog.dev = None
        return _run(prog, x, [m.cpu() for m in rnns], torch.device("cpu"), want)
    finally:
        TB.set_backend(None)
        prog.__dict__.pop("_chain_tabs", None)
        prog.dev = None


def _close(a, b, name):
    for u, v in zip(a[0], b[0]):
        assert_close(u, v, 1e-5, 2e-6, "states vs " + name)
    assert_close(a[1], b[1], 1e-4, 2e-5 * max(1.0, float(b[1].abs().max())), "d_x vs " + name)
    for u, v in zip(a[2], b[2]):
        assert_close(u, v, 1e-4, 2e-5 * max(1.0, float(v.abs().max())), "GRU parameter gradient vs " + name)


def _x(n, d, seed=17):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * 0.5


def _permuted_program(seed):
    """random_program with the x rows of every instance moved to another block of a larger x (x row != chain row)."""
    prog, n_x = random_program(seed, n_chain=2, K=5, E=120, lo=30, hi=120)
    order = np.random.default_rng(seed).permutation(len(prog.inst))
    inst, x0 = [], 7
    starts = {}
    for i in order:
        starts[i] = x0
        x0 += prog.inst[i].n + 3
    for i, it in enumerate(prog.inst):
        inst.append(GruInstance(it.n, starts[i], it.rnn, it.prev, it.prev_idx, it.dt))
    return GruProgram(inst), x0


@pytest.mark.parametrize("d,kw", [(200, dict(n_chain=2, K=6, E=90, lo=20, hi=70)), (128, dict(n_chain=2, K=5, E=64, lo=1, hi=64)),
                                  (248, dict(n_chain=2, K=4, E=50, lo=10, hi=50)), (32, dict(n_chain=2, K=5, E=200, lo=50, hi=200))])
@pytest.mark.parametrize("want", [None, "some"])
def test_fused_route_vs_gi_route_and_cpu_reference(d, kw, want):
    """Random chain programs of two GRUs (idle tracks, tracks that start mid-chain, an empty position): the fused route against
    the gi route and the CPU reference.  d = 248 is past the f16 chain kernels: it keeps the gi route (no fused launch)."""
    prog, n_x = random_program(d + 1, **kw)
    w = None if want is None else tuple(i for i, it in enumerate(prog.inst) if it.next < 0 or i % 3 == 1)[:8]
    rnns = make_rnns(2, d, False, 5)
    x = _x(n_x, d)
    c0 = _launches()
    fused = _run(prog, x, rnns, DEV, w, fused=True)
    ran = _launches() - c0
    assert ran == (0 if d == 248 else 1), ran
    gi = _run(prog, x, rnns, DEV, w, fused=False)
    assert _launches() - c0 == ran
    _close(fused, gi, "gi route")
    _close(fused, _cpu(prog, x, rnns, w), "CPU reference")


def test_fused_route_x_rows_apart_from_chain_rows():
    """x rows in another order than the chain rows, with rows no instance reads (the x_index table)."""
    prog, n_x = _permuted_program(11)
    rnns = make_rnns(2, 200, False, 6)
    x = _x(n_x, 200, 3)
    c0 = _launches()
    fused = _run(prog, x, rnns, DEV)
    assert _launches() - c0 == 1
    _close(fused, _run(prog, x, rnns, DEV, fused=False), "gi route")
    _close(fused, _cpu(prog, x, rnns, None), "CPU reference")


def test_fused_route_row_scales():
    """x rows whose magnitudes span 2^-20 .. 2^10 (the per-row keys of the x planes).  Pre-activations of several hundred make
    fp32 itself the limit (an ulp of 500 is 3e-5), so the bar is the gi route's own distance from the CPU reference (measured:
    9.4e-5 against 4.2e-5 -- a few more fp32 roundings of the same magnitude: gi + gh in the accumulator, then the unscale)."""
    prog, n_x = random_program(5, n_chain=2, K=5, E=80, lo=20, hi=80)
    rnns = make_rnns(2, 200, False, 7)
    rng = np.random.default_rng(9)
    x = _x(n_x, 200, 4) * torch.from_numpy(np.exp2(rng.integers(-20, 11, n_x)).astype(np.float32))[:, None]
    fused = _run(prog, x, rnns, DEV)
    gi = _run(prog, x, rnns, DEV, fused=False)
    cpu = _cpu(prog, x, rnns, None)
    for u, v, c in zip(fused[0], gi[0], cpu[0]):
        if c.numel() == 0:
            continue
        e_f, e_g = float((u - c).abs().max()), float((v - c).abs().max())
        assert e_f <= 4 * e_g + 2e-6, (e_f, e_g)
    x1 = _x(n_x, 200, 4) * torch.from_numpy(np.exp2(rng.integers(-20, 1, n_x)).astype(np.float32))[:, None]
    _close(_run(prog, x1, rnns, DEV), _cpu(prog, x1, rnns, None), "CPU reference (rows 2^-20 .. 1)")


def test_fused_route_bit_repeatable_and_switch():
    """Two fused runs are bit-identical; TEMP_DEBUG bit 22 sends the same call down the gi route."""
    prog, n_x = random_program(8, n_chain=2, K=6, E=90, lo=20, hi=70)
    rnns = make_rnns(2, 200, False, 8)
    x = _x(n_x, 200, 8)
    a = _run(prog, x, rnns, DEV)
    c0 = _launches()
    b = _run(prog, x, rnns, DEV)
    assert _launches() - c0 == 1
    for u, v in zip(a[0] + [a[1]] + a[2], b[0] + [b[1]] + b[2]):
        assert torch.equal(u, v)
    lib = _lib.load()
    prev = lib.temp_set_option(_lib.OPT_DEBUG, FWD_X_OFF)
    try:
        c0 = _launches()
        off = _run(prog, x, rnns, DEV)
        assert _launches() == c0
    finally:
        lib.temp_set_option(_lib.OPT_DEBUG, prev)
    _close(a, off, "TEMP_DEBUG gi route")


def test_fused_route_with_and_without_x_src():
    """The route does not depend on the x_src labels: a labelled and an unlabelled run take the fused kernel, bit-identically."""
    prog, n_x = random_program(23, n_chain=2, K=7, E=300, lo=100, hi=300)
    labels = np.random.default_rng(3).integers(0, n_x // 3, n_x)
    rnns = make_rnns(2, 200, False, 5)
    x = _x(int(labels.max()) + 1, 200)[torch.from_numpy(labels).long()]
    c0 = _launches()
    prog.x_src = labels
    try:
        lab = _run(prog, x, rnns, DEV)
    finally:
        prog.__dict__.pop("x_src", None)
        prog.__dict__.pop("_gi_shared", None)
    unl = _run(prog, x, rnns, DEV)
    assert _launches() - c0 == 2
    for u, v in zip(lab[0], unl[0]):
        assert torch.equal(u, v)


def test_long_panels_keep_the_gi_route():
    """At d = 200 the fused kernel's LDS holds panels of up to 19 positions; a program with longer panels takes the gi route."""
    prog, n_x = random_program(31, n_chain=2, K=24, E=40, lo=34, hi=40)
    tabs = prog.chain_tables(DEV, None)
    assert tabs["max_steps"] > 19
    rnns = make_rnns(2, 200, False, 9)
    x = _x(n_x, 200, 5)
    c0 = _launches()
    got = _run(prog, x, rnns, DEV)
    assert _launches() == c0
    _close(got, _cpu(prog, x, rnns, None), "CPU reference")


def test_large_w_ih_columns():
    """W_hh's forward planes share their column scales with W_ih's: W_ih 2^8 times larger than W_hh (x 2^8 smaller, so the
    pre-activations stay moderate) costs W_hh no precision beyond the usual bar."""
    prog, n_x = random_program(12, n_chain=2, K=6, E=90, lo=20, hi=70)
    rnns = make_rnns(2, 200, False, 10)
    with torch.no_grad():
        for m in rnns:
            m.weight_ih_l0.mul_(256.0)
    x = _x(n_x, 200, 6) / 256.0
    c0 = _launches()
    got = _run(prog, x, rnns, DEV)
    assert _launches() - c0 == 1
    _close(got, _cpu(prog, x, rnns, None), "CPU reference")


@pytest.mark.parametrize("fused", [True, False])
def test_options_toggled_between_forward_and_backward(fused):
    """The chain kernels follow the layout the packs were written in (TempGruChain.pack_layout), not the options at launch
    time: switching the f16 arithmetic off between the forward and the backward still gives the right gradients."""
    prog, n_x = random_program(14, n_chain=2, K=6, E=90, lo=20, hi=70)
    rnns = make_rnns(2, 200, False, 11)
    x = _x(n_x, 200, 7)
    lib = _lib.load()
    prev = [lib.temp_get_option(_lib.OPT_MFMA_F16X2)]

    def toggle():
        lib.temp_set_option(_lib.OPT_MFMA_F16X2, 0)

    try:
        got = _run(prog, x, rnns, DEV, fused=fused, between=toggle)
    finally:
        lib.temp_set_option(_lib.OPT_MFMA_F16X2, prev[0])
    _close(got, _cpu(prog, x, rnns, None), "CPU reference")
