"""The host-side facts the cases of tests/attention_route_cases.py rest on, without a GPU: the widths reach every per-lane column
count of the dispatch at both edges of its band; every index recipe has the rows it promises; the inverse maps group what the table
pass walks; on real and stress data the fp32 dense formulation sits within a quarter of every bar against fp64 (a CONDITION on the
cases: one that breaks it gets less stress, never a wider bar); every tensor a case declares exact is exact -- the fp32 dense
formulation in two further summation orders equals the fp64 value with `==`; the fp64 reference's history gradient agrees with the
sum written out from p, ds and the index matrix."""
import numpy as np
import pytest
import torch

from temp_amd import functional as TF
from tests import attention_route_cases as AC

CPU = torch.device("cpu")
REALS = [c for c in AC.ALL if c.regime in ("real", "stress")]
UNIFORM = [c for c in AC.ALL if c.regime == "uniform"]
ONEHOT = [c for c in AC.ALL if c.regime == "onehot"]
BANDS = {1: (1, 8), 2: (9, 16), 4: (17, 32), 8: (33, 64)}             # MAXC: lowest and highest d_k


def _ids(cases):
    return [c.id for c in cases]


def _dispatch(D):
    """TEMP_ATTN_LAUNCH written out: a.dk = D / 8; mc = (a.dk + 7) / 8; mc <= 1 -> K<1>, <= 2 -> K<2>, <= 4 -> K<4>, else K<8>"""
    dk = D // 8
    mc = (dk + 7) // 8
    if mc <= 1:
        return dk, mc, 1
    if mc <= 2:
        return dk, mc, 2
    if mc <= 4:
        return dk, mc, 4
    return dk, mc, 8


def test_width_table():
    for D, dk, mc, maxc in AC.WIDTHS:
        assert D % 8 == 0 and _dispatch(D) == (dk, mc, maxc) == AC.mc_maxc(D)
    assert {w[3] for w in AC.WIDTHS} == {1, 2, 4, 8}
    for group in (REALS, UNIFORM + ONEHOT):
        assert {_dispatch(c.D)[2] for c in group} == {1, 2, 4, 8}, "every MAXC in real and in exact data"
    have = {c.D // 8 for c in REALS}
    for maxc, (lo, hi) in BANDS.items():
        assert _dispatch(8 * lo)[2] == _dispatch(8 * hi)[2] == maxc and (lo == 1 or _dispatch(8 * (lo - 1))[2] < maxc)
        assert lo in have and hi in have, "band MAXC = %d without a real case at an edge" % maxc
    assert {c.D for c in REALS} >= {w[0] for w in AC.WIDTHS}
    assert {9, 16} <= {c.D // 8 for c in UNIFORM}, "both edges of the MAXC = 2 band on uniform data"
    assert {c.D for c in ONEHOT} == {8, 32, 128, 512} and all(AC.is_pow4(c.D // 8) for c in ONEHOT)


def test_case_table():
    shapes = {(c.D, c.T) for c in REALS}
    assert {(D, T) for D in (72, 128) for T in (1, 2, 9, 64)} | {(200, 64), (136, 2)} <= shapes
    assert {c.n for c in REALS} >= {1, 3, 4, 5, 37}
    assert all(c.n <= 37 for c in AC.ALL if c.id != "hub") and all(c.T <= 64 and c.D <= 512 for c in AC.ALL)
    hub = AC.BY_ID["hub"]
    assert (hub.n, hub.T, hub.D, hub.R, hub.regime) == (301, 64, 128, 5, "real")
    assert {c.decay for c in REALS} == {None, "rand", "deep"} and {c.decay for c in UNIFORM} == {None, "half"}
    assert any((c.na, c.nb) == (1, 1) for c in REALS) and any(c.na >= c.n > 1 for c in REALS) and any(c.na * 3 <= c.n for c in REALS)
    assert {AC.mc_maxc(c.D)[2] for c in AC.ALL if c.packed} == {1, 2, 4, 8}, "one case per MAXC with the packed strides"
    assert any(c.regime == "stress" for c in REALS) and all(1 < c.scale <= 3 for c in REALS if c.regime == "stress")
    assert any(c.T == 64 for c in UNIFORM) and any(c.recipe == "hub" for c in UNIFORM)
    a = AC.BY_ID[AC.AUTOGRAD_CASE]
    assert (a.D, a.T, AC.mc_maxc(a.D)[2]) == (128, 9, 2)
    for c in AC.ALL:
        inp = AC.inputs(c)
        assert inp.idx.shape == (c.n, c.T - 1) and inp.idx.dtype == torch.int32 and inp.qkv.shape == (c.n, 3 * c.D)
        assert inp.kvh.shape == (inp.R, 2 * c.D) and (inp.decay is None or inp.decay.shape == (c.T,))
        assert torch.equal(inp.qkv, inp.pa[inp.ia.long()] + inp.pb[inp.ib.long()])
        if c.T == 1:
            assert inp.R == 0 and inp.idx.numel() == 0
        if c.decay == "deep":
            assert int((inp.decay == -30).sum()) >= c.T // 3 and float(inp.decay.max()) <= 0
        if c.decay == "rand":
            assert -1 <= float(inp.decay.min()) and float(inp.decay.max()) <= 0
        ia, ib = inp.ia.numpy(), inp.ib.numpy()
        assert ia.min() >= 0 and ia.max() < c.na and ib.min() >= 0 and ib.max() < c.nb
        if c.na >= c.n:
            assert np.unique(ia).shape[0] == c.n, "more rows than n: each used once"
        else:
            assert np.unique(ia).shape[0] == c.na, "few rows: every one used"


@pytest.mark.parametrize("case", [c for c in AC.ALL if c.T > 1], ids=_ids([c for c in AC.ALL if c.T > 1]))
def test_index_recipes(case):
    f = AC.index_facts(case)
    idx, live, R, Th = f["idx"], f["live"], f["R"], case.T - 1
    assert R % 4 != 0 and R >= 5, "R no multiple of the 4 rows of a workgroup"
    assert f["used"].max() < R - 3 and (f["cnt"][R - 3:] == 0).all(), "the last three table rows are referenced by nobody"
    assert idx.min() >= -1
    if case.n >= 3:
        assert not live[0].any(), "row 0 entirely masked"
        assert (idx[2] == idx[2, 0]).all() and idx[2, 0] >= 0, "row 2: every position on the same table row"
        if case.recipe != "hub":
            assert live[1].all() and np.unique(idx[1]).shape[0] == Th, "row 1 entirely live on distinct table rows"
    if case.n >= 4:
        assert live[case.n - 1].all(), "the last row entirely live"
    if case.n >= 5 and case.T >= 5 and case.regime != "uniform":
        assert 0.3 <= f["share"] <= 0.8, "about half the slots masked"
    if case.recipe == "hub":
        assert set(f["used"]) == {0, 1} and R == 5
    if case.id == "hub":
        print("hub: cnt %s" % f["cnt"])
        assert f["cnt"].max() >= 2000
    if case.regime == "uniform":
        m = live.sum(1) + 1
        assert ((m & (m - 1)) == 0).all() and m.max() <= 64, "live counts (current position included) are powers of two"
    if case.regime == "onehot":
        rest = np.delete(idx, 2, axis=0) if case.n >= 3 else idx
        r = rest[rest >= 0]
        assert np.unique(r).shape[0] == r.shape[0] and (case.n < 3 or idx[2, 0] not in r), "every table row referenced once, row 2's apart"


def test_uniform_facts():
    assert any(int((AC.index_facts(c)["live"].sum(1) + 1).max()) == 64 for c in UNIFORM), "T = 64 with all 64 live"
    seen = set()
    for c in UNIFORM:
        inp = AC.inputs(c)
        assert bool((inp.qkv[:, :c.D] == 0).all()) and not bool((inp.pa[:, :c.D] == 0).all())
        for t in (inp.qkv, inp.kvh, inp.d_out):
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= 4
        seen |= set((AC.index_facts(c)["live"].sum(1) + 1).tolist())
        s = AC.reference(c)["score"]
        fin = torch.isfinite(s)
        assert bool((torch.where(fin, s, s[:, :, -1:]) == s[:, :, -1:]).all()), "every live score of a row is equal"
    assert seen >= {1, 2, 4, 8, 16, 32, 64}
    hub = AC.BY_ID["uni_hub"]
    assert AC.index_facts(hub)["cnt"].max() >= 100


@pytest.mark.parametrize("case", ONEHOT, ids=_ids(ONEHOT))
def test_onehot_facts(case):
    inp, ref = AC.inputs(case), AC.reference(case)
    n, T, D = case.n, case.T, case.D
    dk = D // 8
    q = inp.qkv[:, :D].reshape(n, 8, dk)
    assert bool(((q != 0).sum(-1) == 1).all()) and bool((q.abs().sum(-1) == 64 * dk ** 0.5).all())
    for t in (inp.qkv, inp.kvh, inp.d_out, inp.pa, inp.pb):
        assert bool((t == t.round()).all())
    s = ref["score"]
    hot = torch.from_numpy(inp.hot)
    assert bool((s.gather(2, hot.unsqueeze(-1)) == 128).all())
    rest = s.scatter(2, hot.unsqueeze(-1), float("-inf"))
    assert float(rest.max()) <= 0, "every other live position scores <= 0"
    assert float(ref["p"].scatter(2, hot.unsqueeze(-1), 0.0).max()) <= np.exp(-128.0)
    cur, first, last = hot == T - 1, torch.zeros_like(hot, dtype=torch.bool), torch.zeros_like(hot, dtype=torch.bool)
    live = inp.idx >= 0
    for i in range(n):
        pos = torch.nonzero(live[i]).view(-1)
        if pos.numel():
            first[i], last[i] = hot[i] == int(pos[0]), hot[i] == int(pos[-1])
    assert bool(cur.any()) and bool(first.any()) and bool(last.any()), "hot: the current position, the first live, the last live"
    if n >= 4:
        assert any(len(set(inp.hot[i].tolist())) > 1 for i in range(n)), "the hot position differs between heads"
    assert len({tuple(r) for r in inp.hot.tolist()}) > 1, "... and between rows"


def test_inverse_maps():
    for c in AC.ALL:
        inp = AC.inputs(c)
        if c.T > 1:
            idx = inp.idx.numpy()
            ptr, ref = (t.numpy() for t in TF.attention_inverse(idx, inp.R, CPU))
            flat = idx.reshape(-1)
            assert ptr.shape[0] == inp.R + 1 and ptr[0] == 0 and ptr[-1] == ref.shape[0] == int((flat >= 0).sum())
            assert np.array_equal(np.sort(ref), np.nonzero(flat >= 0)[0]), "exactly the live pairs"
            for r in range(inp.R):
                assert (flat[ref[ptr[r]:ptr[r + 1]]] == r).all()
            assert np.array_equal(np.diff(ptr), AC.reference(c)["cnt"].numpy().astype(np.int64))
        for rows, n_tab in ((inp.ia, c.na), (inp.ib, c.nb)):
            ptr, order = (t.numpy() for t in TF.split_row_inverse(rows.numpy(), n_tab, CPU))
            assert ptr.shape[0] == 3 * n_tab + 1 and np.array_equal(np.sort(order), np.arange(3 * c.n)), "a partition of the 3 n thirds"
            for seg in range(3 * n_tab):
                th = order[ptr[seg]:ptr[seg + 1]]
                assert (rows.numpy()[th // 3] == seg // 3).all() and (th % 3 == seg % 3).all()


NAMES = ("out", "lse", "score", "d_q", "d_k", "d_v", "d_kh", "d_vh", "d_decay")


@pytest.mark.parametrize("case", REALS, ids=_ids(REALS))
def test_fp32_dense_formulation_within_a_quarter_of_the_bars(case):
    ref, f32 = AC.reference(case), AC.dense(AC.inputs(case), torch.float32)
    ratios = {k: AC.ratio(k, f32[k], ref[k], ref) for k in NAMES if ref[k] is not None}
    print("attention condition %s: fp32 dense / bar %s" % (case.id, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert all(torch.isfinite(ref[k]).all() for k in NAMES if ref[k] is not None and k != "score")
    assert max(ratios.values()) <= AC.CONDITION, ratios


@pytest.mark.parametrize("case", REALS + UNIFORM, ids=_ids(REALS + UNIFORM))
def test_history_gradient_written_out(case):
    """autograd's history gradient = the sum over the index matrix written out (the same sum whose absolute values are `mag`)"""
    ref = AC.reference(case)
    for half in ("kh", "vh"):
        err = (ref["x_" + half] - ref["d_" + half]).abs()
        assert bool((err <= 1e-12 * ref["mag_" + half] + 1e-300).all()), half
        assert bool((ref["mag_" + half] >= ref["d_" + half].abs() * (1 - 1e-12)).all())
    assert bool((ref["cnt"][-3:] == 0).all()) or case.T == 1


@pytest.mark.parametrize("case", UNIFORM + ONEHOT, ids=_ids(UNIFORM + ONEHOT))
def test_declared_tensors_are_exact(case):
    inp, ref = AC.inputs(case), AC.reference(case)
    names = AC.exact_tensors(case)
    assert {"out", "d_k", "d_v"} <= set(names)
    runs = [AC.dense(inp, torch.float32, order) for order in ("hist_reversed", "backwards")]
    for k in names:
        want = AC.exact_want(ref[k])
        gap = float((want - ref[k]).abs().max()) if want.numel() else 0.0
        assert gap == 0 if case.regime == "uniform" else gap <= 1e-50, (k, gap)           # (onehot: the exp(-128) weights)
        for run in runs:
            assert torch.equal(run[k].double(), want), "%s: %s is not exact" % (case.id, k)
    # what the declarations say in words
    assert bool((ref["d_k"].float() == 0).all()) and bool((ref["d_kh"].float() == 0).all())
    if case.regime == "onehot":
        n, D, dk = case.n, case.D, case.D // 8
        assert bool((ref["lse"] == 128).all()) and bool((ref["d_q"].float() == 0).all())
        assert ref["d_decay"] is None or bool((ref["d_decay"].float() == 0).all())
        hot = torch.from_numpy(inp.hot)
        v_hot = torch.zeros(n, 8, dk, dtype=torch.float64)
        want_vh = torch.zeros(inp.R, D, dtype=torch.float64)
        want_vc = torch.zeros(n, D, dtype=torch.float64)
        dov = inp.d_out.double().view(n, dk, 8).transpose(1, 2)                            # the head-transposed layout
        for i in range(n):
            for h in range(8):
                t = int(hot[i, h])
                sl = slice(h * dk, (h + 1) * dk)
                if t == case.T - 1:
                    v_hot[i, h], want_vc[i, sl] = inp.qkv[i, 2 * D:][sl].double(), dov[i, h]
                else:
                    v_hot[i, h], want_vh[int(inp.idx[i, t]), sl] = inp.kvh[int(inp.idx[i, t]), D:][sl].double(), dov[i, h]
        assert torch.equal(AC.exact_want(ref["out"]), v_hot.transpose(1, 2).reshape(n, D)), "out = the hot position's v"
        assert torch.equal(AC.exact_want(ref["d_v"]), want_vc) and torch.equal(AC.exact_want(ref["d_vh"]), want_vh), "the hot row receives d_out"
    else:
        # any order of the accumulated sums is exact: sum |terms| stays below 2^24 quanta (weights are multiples of 1/64, ds of 1/4096)
        assert float(ref["mag_vh"].max()) * 64 < 2 ** 24
        assert float(ref["ds"].abs().sum((0, 1)).max()) * 4096 < 2 ** 24
