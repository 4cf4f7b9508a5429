"""The GRU chain reading its input rows where they lie (gru_chain(table=...), temp_gru_grads_g4_rows) against the copy into chain
order it replaces (functional.gather_rows(keys=True) + today's gru_chain; models/BiRRGCN.py:202-225 feeds layer 2's output rows to
the GRU step of models/RRGCN.py:84).  Nothing numeric changes on the route -- the same rows reach the same kernels' arithmetic in the
same order -- so every comparison with the copy is bit for bit; the weight-gradient kernel is also held to the fp64 bars of
tests/test_gpu_f16_split.py::test_gru_grads_g4_keys_vs_fp64_gpu."""
import numpy as np
import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from temp_amd import gru_chain as GC
from tests.chain_cases import make_rnns
from tests.chain_route_cases import GPU_CASES, QUERIES, recorded
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be
    TB.set_backend(None)


def _key(x):
    return (x.contiguous().view(torch.int32).to(torch.int64)) & 0x7FFFFFFF


def run_rows(n, table_rows, rng, reserved):
    """A row list of n entries made of runs of 5, 21 and 500 consecutive table rows (the last run cut to fit), every third run in
    DESCENDING order, none reading the `reserved` rows at the table's end; then one table row is written to two far-apart places."""
    out, k = [], 0
    while len(out) < n:
        ln = (5, 21, 500)[k % 3]
        r0 = int(rng.integers(0, table_rows - reserved - ln))
        run = np.arange(r0, r0 + ln)
        out.extend(run[::-1] if k % 3 == 2 else run)
        k += 1
    rows = np.asarray(out[:n], dtype=np.int32)
    if n >= 30:
        rows[3] = rows[n - 7]
    return rows


# group row counts that are no multiple of the 16-row slab, two of them far shorter than a row slice (most of their slices are empty);
# the third carries the launch over the 16 384 rows below which the library leaves these shapes to the fp32 kernels.
# d = 40: one mixed workgroup per slice; d = 56: two single-operand left-over workgroups; d = 200 (the flagship width): full
# workgroups that share the left-over tiles as tails
@pytest.mark.parametrize("d", [40, 56, 200])
def test_gru_grads_g4_rows_equals_copy_and_fp64_gpu(d, hip_backend):
    be = hip_backend
    rows = (37, 250, 16405)
    T, reserved = 20000, 1000
    gen = torch.Generator(device="cpu").manual_seed(5 + d)
    rng = np.random.default_rng(d)
    mk = lambda n, w, s=1.0: (torch.randn(n, w, generator=gen) * s)
    table = mk(T, d)
    table[T - reserved:] = float("nan")                              # rows no chain reads: reading one would show
    x_rows = [run_rows(n, T, rng, reserved) for n in rows]
    assert all(int(r.max()) < T - reserved for r in x_rows) and len(set(x_rows[2].tolist())) < rows[2]
    hd = [(torch.rand(n, d, generator=gen) * 2 - 1) for n in rows]                        # decayed GRU states, |.| <= 1
    g4 = [mk(n, 4 * d, 0.1) * torch.exp(mk(n, 1) * 1.5) for n in rows]
    ws = [((torch.rand(3 * d, d, generator=gen) - 0.5) * 0.3).to(DEV) for _ in rows]
    table, hd, g4 = table.to(DEV), [t.to(DEV) for t in hd], [t.to(DEV).contiguous() for t in g4]
    x_rows = [torch.from_numpy(r).to(DEV) for r in x_rows]
    xs = [table[r.long()].contiguous() for r in x_rows]                                   # the copy the route does without
    assert all(torch.isfinite(x).all() for x in xs)
    assert be.gru_grads_g4_supported(list(rows), d, _lib.GRU_TORCH) and be.gru_grads_g4_rows_supported(list(rows), d, _lib.GRU_TORCH, T)
    row_keys = [_key(t[:, :3 * d].abs().max(dim=1).values).to(torch.int32) for t in g4]
    col_keys = [_key(t.abs().max(dim=0).values).to(torch.int32).contiguous() for t in g4]
    x_col = [_key(torch.cat(xs).abs().max(dim=0).values).to(torch.int32).contiguous()] * len(rows)   # one bound over all rows read
    dx = [torch.full((n, d), float("nan"), device=DEV) for n in rows]
    dx2 = [torch.full_like(t, float("nan")) for t in dx]
    got = be.gru_grads_g4_rows(table, x_rows, hd, g4, ws, dx, row_keys, col_keys, x_col)
    ref = be.gru_grads_g4(xs, hd, g4, ws, dx2, row_keys=row_keys, col_keys=col_keys, x_col_keys=x_col)
    torch.cuda.synchronize()
    for k, n in enumerate(rows):
        G = g4[k].double()
        dgi, dgh = G[:, :3 * d], torch.cat([G[:, :2 * d], G[:, 3 * d:]], 1)
        want = (dgi.t() @ xs[k].double(), dgh.t() @ hd[k].double(), dgi.sum(0), dgh.sum(0))
        scale = (dgi.abs().t() @ xs[k].abs().double(), dgh.abs().t() @ hd[k].abs().double(), dgi.abs().sum(0), dgh.abs().sum(0))
        for a, b, w, sc in zip(got[k], ref[k], want, scale):
            assert a.shape == w.shape and torch.isfinite(a).all()
            err = float(((a.double() - w).abs() / sc.clamp_min(1e-300)).max())
            print("d=%d group %d %s: max error / sum|a||b| = %.3g, equal to the copy route: %s" % (d, k, tuple(a.shape), err, torch.equal(a, b)))
            assert torch.equal(a, b), "rows in place and the gathered copy must give the same bits"
            assert err < 2e-6
        assert torch.equal(dx[k], dx2[k])
        wantx, scx = dgi @ ws[k].double(), dgi.abs() @ ws[k].abs().double()
        assert float(((dx[k].double() - wantx).abs() / scx.clamp_min(1e-300)).max()) < 2e-6


def test_gru_grads_g4_rows_refuses_gpu(hip_backend):
    be = hip_backend
    assert not be.gru_grads_g4_rows_supported([900, 700], 200, _lib.GRU_TORCH, 5000)           # what gru_grads_g4 leaves to the fp32 kernels
    assert not be.gru_grads_g4_rows_supported([30000], 200, _lib.GRU_TORCH, 2 ** 32 // 800 + 1)    # table byte offsets need 33 bits
    assert be.gru_grads_g4_rows_supported([30000], 200, _lib.GRU_TORCH, 2 ** 32 // 800)
    assert not be.gru_grads_g4_rows_supported([2000000], 200, _lib.GRU_TORCH, 5000)            # a slice's row list does not fit LDS


def _route(c, fold, in_place):
    """One forward + backward of route case `c` with x = table[chain_rows]: through gru_chain(table=...) (`in_place`) or through the
    keyed gather and today's gru_chain.  Every table row is a chain row (as in the models' batches: the column keys of the table are
    then those of the copy), a quarter of the x rows repeat one.  -> (launches, tensors, whether the in-place route was usable)."""
    prog, n_x = c["prog"]()
    d = c["d"]
    rnns = [m.to(DEV) for m in make_rnns(max(it.rnn for it in prog.inst) + 1, d, False, 5)]
    g = torch.Generator().manual_seed(17)
    rng = np.random.default_rng(3)
    T = n_x - n_x // 4
    chain = np.concatenate([rng.permutation(T), rng.integers(0, T, n_x - T)])[rng.permutation(n_x)]
    table = torch.randn(T, d, generator=g) * 0.5
    leaf = (torch.relu(table) if fold else table).to(DEV).requires_grad_(True)
    rows_dev, inv = _lib.to_device(chain.astype(np.int32), DEV), TF.gather_inverse(chain, T, DEV)
    prog.x_rows(DEV, chain)
    want = tuple(i for i, it in enumerate(prog.inst) if it.next < 0) if c["want"] else None
    usable = GC.rows_in_place_usable(prog, leaf, inv, len(rnns), False, want)
    with recorded(c["flags"]) as rec:
        if in_place:
            out = GC.gru_chain(None, prog, rnns, 0.1, False, want, table=(leaf, rows_dev, inv, fold))
        else:
            x, keys = TF.gather_rows(leaf, rows_dev, inv, relu_table=fold, keys=True)
            out = GC.gru_chain(x, prog, rnns, 0.1, False, want, x_keys=keys)
        outs = [out] if want is None else list(out)
        loss = sum((o * torch.randn(o.shape, generator=g).to(DEV)).sum() * (k + 1) for k, o in enumerate(outs))
        loss.backward()
    tensors = [o.detach() for o in outs] + [leaf.grad] + [p.grad for m in rnns for p in m.parameters()]
    return [call for call in rec.calls if not call[0].endswith(QUERIES)], [t.cpu() for t in tensors], usable


# The launches of the in-place route, recorded from this route's first passing run (there is no earlier commit that has it): the
# column keys of the table, ONE pack, the x-route forward over the table, the keyed chain backward, the weight gradients with the
# rows in place, the table's gradient -- no gather_rows_keys, no second pack.
IN_PLACE_LAUNCHES = {
    "large-d200": [('absmax_keys', ((14175, 200),), ('rows',)),
                   ('gru_chain_pack_x_multi', (), ()),
                   ('gru_chain_fwd_x', ((14175, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                   ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                   ('gru_grads_g4_rows', ((14175, 200),), ('col_keys', 'row_keys', 'x_col_keys')),
                   ('segment_sum_rows', ((18899, 200), (14176,), (18899,)), ('relu_of',))],
    "large-want-d200": [('absmax_keys', ((14175, 200),), ('rows',)),
                        ('gru_chain_pack_x_multi', (), ()),
                        ('gru_chain_fwd_x', ((14175, 200), (18899,), (18899, 200), (5, 18899, 200)), ()),
                        ('gru_chain_bwd_g4', ((5, 18899, 200), (18899, 800)), ('keys',)),
                        ('gru_grads_g4_rows', ((14175, 200),), ('col_keys', 'row_keys', 'x_col_keys')),
                        ('segment_sum_rows', ((18899, 200), (14176,), (18899,)), ())],
}


@pytest.mark.parametrize("name,fold", [("large-d200", True), ("large-want-d200", False), ("shared-centre", False)])
def test_route_in_place_equals_gather_gpu(name, fold, hip_backend):
    """Outputs, d_table and every GRU gradient of gru_chain(table=...) are those of the gather + today's gru_chain, bit for bit.  The
    large programs take the in-place route; `shared-centre` (two groups over the same x rows: its weight gradients go group by group,
    not through the one keyed launch) does not meet the route's condition and must come out as the gather route it falls back to."""
    c = GPU_CASES[name]
    launches, got, usable = _route(c, fold, True)
    _, ref, _ = _route(c, fold, False)
    print(name, launches)
    assert len(got) == len(ref)
    for k, (u, v) in enumerate(zip(got, ref)):
        assert torch.isfinite(u).all() and torch.equal(u, v), "tensor %d differs from the gather route" % k
    names = [call[0] for call in launches]
    if name == "shared-centre":
        assert not usable and names[0] == "gather_rows_keys" and "gru_grads_g4_rows" not in names
        return
    assert usable and "gather_rows_keys" not in names and "gather_rows" not in names
    assert sum(1 for n in names if "pack" in n) == 1 and names.count("gru_grads_g4_rows") == 1
    assert launches == IN_PLACE_LAUNCHES[name]
    old = GC.ROWS_IN_PLACE
    GC.ROWS_IN_PLACE = False
    try:
        off_launches, off, _ = _route(c, fold, True)
    finally:
        GC.ROWS_IN_PLACE = old
    assert off_launches[0][0] == "gather_rows_keys" and all(torch.equal(u, v) for u, v in zip(off, ref))


def test_model_step_switch_on_equals_off_gpu(hip_backend):
    """S-tiny BiGRRGCN, prepare + forward + backward with ROWS_IN_PLACE on and off: every array bit for bit."""
    import bench
    from temp_amd import synthetic
    w = synthetic.workload("S-tiny", seed=0)
    targets = synthetic.default_targets(w["num_times"], w["L"], w["bsz"], 0)
    res, old = [], GC.ROWS_IN_PLACE
    try:
        for flag in (True, False):
            GC.ROWS_IN_PLACE = flag
            torch.manual_seed(11)                                    # (the same initial weights and dropout draws in both runs)
            model = bench.build_model(w, DEV)
            model.sample_rng = np.random.default_rng(2)
            wb = model.prepare(targets, w["L"], train=True)
            out = model.run(wb)[0]
            (out * out).sum().backward()
            res.append((out.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in model.named_parameters() if v.grad is not None}))
    finally:
        GC.ROWS_IN_PLACE = old
    (o1, g1), (o0, g0) = res
    assert torch.isfinite(o1).all() and torch.equal(o1, o0)
    assert set(g0) == set(g1) and len(g0) >= 8
    for k in g0:
        assert torch.equal(g1[k], g0[k]), "d_" + k


@pytest.fixture(scope="module")
def gdelt():
    from temp_amd import synthetic
    return synthetic.workload("S-gdelt", seed=0)


@pytest.mark.parametrize("module,n_windows", [("BiGRRGCN", 4), ("GRRGCN", 8)])
def test_headline_step_takes_the_route_and_equals_the_gather_gpu(module, n_windows, gdelt, hip_backend):
    """The S-tiny step above is too small for the route (fewer than 16 384 chain rows: it checks that the switch changes nothing there).
    Here the models take it: an S-gdelt encoder step of the bi-directional model and of the uni-directional one (shared visits) makes
    exactly one gru_grads_g4_rows call and no keyed gather with the switch on, the reverse with it off, and output and every
    gradient are the same bits."""
    import bench
    from temp_amd import synthetic
    from tests.chain_route_cases import recorded
    w = dict(gdelt, module=module)
    targets = synthetic.default_targets(w["num_times"], w["L"], n_windows, 0)
    res = []
    for flag in (True, False):
        model = bench.build_model(w, DEV)
        model.sample_rng = np.random.default_rng(2)
        with recorded(dict(ROWS_IN_PLACE=flag)) as rec:
            wb = model.prepare(targets, w["L"], train=True)
            out = model.run(wb)[0]
            (out * out).sum().backward()
        names = [c[0] for c in rec.calls]
        assert names.count("gru_grads_g4_rows") == (1 if flag else 0) and names.count("gru_grads_g4") == (0 if flag else 1)
        assert ("gather_rows_keys" not in names) if flag else True
        assert (wb.last_x is None) == flag
        res.append((out.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in model.named_parameters() if v.grad is not None}))
    (o1, g1), (o0, g0) = res
    assert torch.isfinite(o1).all() and torch.equal(o1, o0)
    assert set(g0) == set(g1) and len(g0) >= 8
    for k in g0:
        assert torch.equal(g1[k], g0[k]), "d_" + k
