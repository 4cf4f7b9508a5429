"""The chain forward with the input gates inside (k_gru_chain_fwd_x) at the edges of its x prefetch and of its store count.

The memory role of the kernel loads the x rows of position s + 2 behind barrier A of position s and stores five or six planes per
active track and pass; how many loads and stores a wave has in flight at each of its waits therefore depends on where the panel
ends (s + 1 < ns, s + 2 < ns), on which tracks are idle in which pass, and on which positions are wanted (the H store).  The
programs below put each of these at its edges; the fused route is compared with the gi route it replaces and with the CPU panel
reference of the test backend, at the bars of tests/test_gpu_chain_input_gates.py, and run five times for bit-equal results."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd.gru_chain import GruInstance, GruProgram
from tests.chain_cases import make_rnns, random_program
from tests.test_gpu_chain_input_gates import DEV, _close, _cpu, _launches, _run, _x
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]

# (d, random_program arguments, panel lengths the program must contain).  lo = 1 (5 for the longest panel): positions of a single row
# up to full ones, so whole waves of a pass are idle and tracks start mid-chain; with K >= 4 the second chain has a position with no
# rows.  A panel covers its tracks' life time, so one program holds panels of several lengths.
CASES = [
    (200, dict(n_chain=2, K=2, E=40, lo=1, hi=40), (1, 2)),          # ns = 1: no x split and no prefetch inside the loop; ns = 2: one x split
    (200, dict(n_chain=2, K=3, E=40, lo=1, hi=40), (1, 2, 3)),       # ns = 3: one prefetch inside the loop
    (200, dict(n_chain=2, K=19, E=40, lo=5, hi=40), (19,)),          # a panel of 19 positions: the longest the fused route takes at d = 200
    (200, dict(n_chain=2, K=7, E=64, lo=1, hi=5), (6, 7)),           # at most 5 of 32 tracks active: idle waves in every pass
    (200, dict(n_chain=2, K=6, E=70, lo=1, hi=70), (1, 3, 5, 6)),    # several panels per position, an empty position
    (128, dict(n_chain=2, K=2, E=40, lo=1, hi=40), (1, 2)),
    (128, dict(n_chain=2, K=3, E=70, lo=1, hi=70), (2, 3)),
    (128, dict(n_chain=2, K=6, E=70, lo=1, hi=70), (2, 3, 5, 6)),
    (32, dict(n_chain=2, K=2, E=40, lo=1, hi=40), (1, 2)),
    (32, dict(n_chain=2, K=3, E=40, lo=1, hi=40), (1, 3)),
    (32, dict(n_chain=2, K=5, E=70, lo=1, hi=70), (1, 2, 3, 4, 5)),
]


def _plan_properties(prog):
    """What the plan of a program really holds: (a step whose four passes each have an idle track -- slot = pass * 8 + wave, so a wave
    idles in every pass; a row without a previous state behind its panel's first step; an instance with no rows)."""
    plan = prog.chain_plan()
    rows = plan["rows"]
    idle = any(all((rows[s, 8 * ps:8 * ps + 8] < 0).any() for ps in range(4)) for s in range(rows.shape[0]))
    mid = False
    for _, s0, ns, _ in plan["panel"].tolist():
        later = rows[s0 + 1:s0 + ns]
        mid = mid or bool(((later >= 0) & ((later & _lib.CHAIN_HAS_PREV) == 0)).any())
    return idle, mid, any(it.n == 0 for it in prog.inst)


def _permuted(prog, seed):
    """The program with the x rows of every instance moved to another block of a larger x (x row != chain row), gaps between."""
    order = np.random.default_rng(seed).permutation(len(prog.inst))
    starts, x0 = {}, 5
    for i in order:
        starts[int(i)] = x0
        x0 += prog.inst[int(i)].n + 2
    return GruProgram([GruInstance(it.n, starts[i], it.rnn, it.prev, it.prev_idx, it.dt) for i, it in enumerate(prog.inst)]), x0


def _want(prog, want):
    return None if want is None else tuple(i for i, it in enumerate(prog.inst) if it.next < 0 or i % 3 == 1)[:8]


@pytest.mark.parametrize("d,kw,ns", CASES, ids=["d%d-K%d-E%d-hi%d" % (d, kw["K"], kw["E"], kw["hi"]) for d, kw, _ in CASES])
@pytest.mark.parametrize("want", [None, "some"])
def test_fused_route_at_the_edges_of_prefetch_and_store_count(d, kw, ns, want):
    """want = None: every position's states are stored (flags & 2 everywhere); "some": only the wanted instances', so the number
    of plane stores differs from position to position."""
    prog, n_x = random_program(1000 * d + kw["K"], **kw)
    lengths = set(int(n) for n in prog.chain_plan()["panel"][:, 2])
    assert set(ns) <= lengths and max(lengths) <= 19, lengths
    idle, mid, empty = _plan_properties(prog)
    assert idle and mid, (idle, mid)
    assert empty == (kw["K"] >= 4)
    w = _want(prog, want)
    rnns = make_rnns(2, d, False, 5)
    x = _x(n_x, d)
    c0 = _launches()
    fused = _run(prog, x, rnns, DEV, w, fused=True)
    assert _launches() - c0 == 1, "the fused kernel did not run"
    gi = _run(prog, x, rnns, DEV, w, fused=False)
    assert _launches() - c0 == 1
    _close(fused, gi, "gi route")
    _close(fused, _cpu(prog, x, rnns, w), "CPU reference")


@pytest.mark.parametrize("want", [None, "some"])
def test_fused_route_five_runs_bit_equal(want):
    """The same program five times, both GRUs: every output and gradient bit-equal (a wait that leaves one access too many in
    flight reads a register or an LDS row early on some runs)."""
    prog, n_x = random_program(77, n_chain=2, K=9, E=70, lo=1, hi=70)
    w = _want(prog, want)
    rnns = make_rnns(2, 200, False, 12)
    x = _x(n_x, 200, 9)
    c0 = _launches()
    runs = [_run(prog, x, rnns, DEV, w) for _ in range(5)]
    assert _launches() - c0 == 5
    first = runs[0][0] + [runs[0][1]] + runs[0][2]
    for r in runs[1:]:
        for u, v in zip(first, r[0] + [r[1]] + r[2]):
            assert torch.equal(u, v)


@pytest.mark.parametrize("d,K", [(200, 2), (200, 3), (32, 3)])
def test_fused_route_short_panels_x_rows_apart_from_chain_rows(d, K):
    """Panels of 1, 2 and 3 positions with x rows that are NOT the chain rows: the indices read one position ahead of their row
    loads must be those of the right position (a stale or shifted index reads another instance's rows)."""
    base, _ = random_program(1000 * d + K, n_chain=2, K=K, E=40, lo=1, hi=40)
    prog, n_x = _permuted(base, 3)
    assert {1, K} <= set(int(n) for n in prog.chain_plan()["panel"][:, 2])
    rnns = make_rnns(2, d, False, 6)
    x = _x(n_x, d, 3)
    c0 = _launches()
    fused = _run(prog, x, rnns, DEV)
    assert _launches() - c0 == 1
    _close(fused, _run(prog, x, rnns, DEV, fused=False), "gi route")
    _close(fused, _cpu(prog, x, rnns, None), "CPU reference")


@pytest.mark.parametrize("d", [200, 128, 32])
def test_development_instantiation_computes_the_same(d):
    """TEMP_DEBUG bit 14 (a.dbg bit 6: every block starts its slab walk at slab 0) sends the launch to the DEV = 1 instantiation of
    its width; the walk's order changes the fp32 sums only within the usual bars."""
    prog, n_x = random_program(1000 * d + 6, n_chain=2, K=6, E=70, lo=1, hi=70)
    rnns = make_rnns(2, d, False, 5)
    x = _x(n_x, d)
    ref = _run(prog, x, rnns, DEV)
    lib = _lib.load()
    prev = lib.temp_set_option(_lib.OPT_DEBUG, 64 << 8)
    try:
        c0 = _launches()
        dev = _run(prog, x, rnns, DEV)
        assert _launches() - c0 == 1
    finally:
        lib.temp_set_option(_lib.OPT_DEBUG, prev)
    _close(dev, ref, "production instantiation")
    _close(dev, _cpu(prog, x, rnns, None), "CPU reference")
