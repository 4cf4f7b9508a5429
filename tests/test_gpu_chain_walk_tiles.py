"""The weight walks of the f16 window-chain kernels (k_gru_chain_bwd_hx, k_gru_chain_fwd_x) at the edges of their tile split.

A matrix wave of these kernels streams the weight planes of its tiles (tiles wave, wave + NMW, ... of ceil(d / 32) in the
backward, of ceil(3 d / 32) in the forward) through a ring of registers that is refilled while the products run, across the end
of a position's walk into the first slabs of the next position's.  How many tiles a wave really holds depends on the width: the
backward loads the clamped last tile for a tile it does not own and never stores its products, a wave with no tile at all skips
the walk and only keeps the position's barriers, and the forward is compiled once per number of valid tiles.  The programs below
put each of these at its edges -- widths whose waves hold 0, 1, 2 (3 in the forward) tiles, panels of 1, 2 and 3 positions (the
ring wraps into the next position; a panel's last reloads are never used), positions whose walk is skipped while the reloads are
in flight, idle tracks, many panels -- and compare with the CPU panel reference of the test backend at the bars of
tests/test_gpu_chain_input_gates.py, five runs each for bit-equal results."""
import pytest
import torch

from temp_amd import _lib
from tests.chain_cases import make_rnns, random_program
from tests.test_gpu_chain_fwd_waits import _plan_properties, _want
from tests.test_gpu_chain_input_gates import DEV, _close, _cpu, _launches, _run, _x
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]

# d -> (tiles per matrix wave of the backward: 4 waves over ceil(d / 32) tiles; of the forward: 8 waves over ceil(3 d / 32)).
# d = 256 is past the f16 chain kernels (they end at 20 forward tiles, d = 208): it runs the bf16 kernels through the same entry
# points, so the widths on both sides of that edge are checked.
TILES = {32: ({0, 1}, {0, 1}), 72: ({0, 1}, {0, 1}), 136: ({1, 2}, {1, 2}), 200: ({1, 2}, {2, 3}), 256: ({2}, {3})}
# (d, K) -> panel lengths the program must contain; per width the two programs hold panels of 1, 2 and 3 positions
SHORT = {(32, 2): (1, 2), (32, 3): (1, 3), (72, 2): (1, 2), (72, 3): (3,), (136, 2): (2,), (136, 3): (1, 3),
         (200, 2): (1, 2), (200, 3): (1, 2, 3), (256, 2): (1, 2), (256, 3): (3,)}


def _tiles_per_wave(n_tiles, n_waves):
    return {len(range(w, n_tiles, n_waves)) for w in range(n_waves)}


def _f16(d):
    return bool(_lib.load().temp_gru_chain_keys_supported(d))


def _five_runs(prog, x, rnns, want, d):
    """Five runs of the chain (fused forward where the width has it), bit-equal; -> the first."""
    c0 = _launches()
    runs = [_run(prog, x, rnns, DEV, want) for _ in range(5)]
    assert _launches() - c0 == (5 if _f16(d) else 0), "the fused forward kernel did not run"
    first = runs[0][0] + [runs[0][1]] + runs[0][2]
    for r in runs[1:]:
        for u, v in zip(first, r[0] + [r[1]] + r[2]):
            assert torch.equal(u, v)
    return runs[0]


def test_the_widths_cover_every_tile_count():
    for d, (bwd, fwd) in TILES.items():
        assert _tiles_per_wave((d + 31) // 32, 4) == bwd and _tiles_per_wave((3 * d + 31) // 32, 8) == fwd, d
        assert _f16(d) == (d <= 208), d
    assert set().union(*(b for b, _ in TILES.values())) == {0, 1, 2}
    assert set().union(*(f for _, f in TILES.values())) == {0, 1, 2, 3}
    for d in TILES:
        assert set(SHORT[d, 2]) | set(SHORT[d, 3]) == {1, 2, 3}


@pytest.mark.parametrize("d,K", sorted(SHORT), ids=["d%d-K%d" % k for k in sorted(SHORT)])
def test_short_panels_at_every_tile_count(d, K):
    """Panels of 1, 2 and 3 positions with idle tracks and tracks that start mid-panel, all states wanted."""
    prog, n_x = random_program(1000 * d + K, n_chain=2, K=K, E=40, lo=1, hi=40)
    plan = prog.chain_plan()
    lengths = set(int(n) for n in plan["panel"][:, 2])
    assert set(SHORT[d, K]) <= lengths and max(lengths) <= 3, lengths
    idle, mid, _ = _plan_properties(prog)
    assert idle and mid, (idle, mid)
    assert not any(bool(plan["any_prev"][s0]) for _, s0, _, _ in plan["panel"].tolist())       # no walk at a panel's first position
    rnns = make_rnns(2, d, False, 5)
    x = _x(n_x, d)
    _close(_five_runs(prog, x, rnns, None, d), _cpu(prog, x, rnns, None), "CPU reference")


@pytest.mark.parametrize("d", [72, 136, 200])
def test_positions_without_a_walk_inside_a_panel(d):
    """A chain with an empty position: its panels hold positions BEHIND their first at which no track carries a state, so the walk
    is skipped while the ring's reloads of the walk before are in flight; only some instances' states are wanted."""
    prog, n_x = random_program(1000 * d + 6, n_chain=2, K=6, E=70, lo=1, hi=70)
    plan = prog.chain_plan()
    idle, mid, empty = _plan_properties(prog)
    assert idle and mid and empty, (idle, mid, empty)
    inner = [bool(plan["any_prev"][s]) for _, s0, ns, _ in plan["panel"].tolist() for s in range(s0 + 1, s0 + ns)]
    assert inner and any(inner) and not all(inner)
    w = _want(prog, "some")
    rnns = make_rnns(2, d, False, 6)
    x = _x(n_x, d, 2)
    _close(_five_runs(prog, x, rnns, w, d), _cpu(prog, x, rnns, w), "CPU reference")


def test_more_panels_than_compute_units():
    """288 panels at d = 32.  The launchers start one workgroup per panel, so a workgroup's panel loop runs once and no program
    reaches its second turn (which primes the ring again); what a program can reach is more workgroups than the device runs at
    once, each priming a ring whose last reloads nobody uses."""
    d = 32
    prog, n_x = random_program(32007, n_chain=2, K=3, E=4600, lo=4400, hi=4600)
    n_panels = int(prog.chain_plan()["panel"].shape[0])
    assert n_panels > torch.cuda.get_device_properties(DEV).multi_processor_count, n_panels
    rnns = make_rnns(2, d, False, 7)
    x = _x(n_x, d, 4)
    _close(_five_runs(prog, x, rnns, None, d), _cpu(prog, x, rnns, None), "CPU reference")
