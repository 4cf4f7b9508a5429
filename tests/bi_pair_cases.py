"""--module BiRRGCN's union pair pass (BiDynamicRGCN.bi_pair_pass) and its row operator (functional.lin_step_rows2; temp_lin_rows2_fwd /
_bwd): cases and checks shared by the CPU (test backend) and GPU (HIP) suites.

The row cases compare the node with a float64 autograd loop over the two directions at the bars of tests/lin_chain_cases.py (the same
product, twice the depth).  The model cases run lin_chain_cases.window_model("BiRRGCN", "G10_bi_grrgcn_rol") -- the ICEWS14 slice at
D = 32 -- with the attribute on against the same model with it off on the same draws, and against the float64 oracle's loss that
tests/test_lin_chain_cpu.py records."""
import contextlib
import math

import numpy as np
import torch

from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import lin_chain_cases as LC
from tests.chain_route_cases import QUERIES, Launches
from tests.golden_util import assert_close
from tests.lin_chain_cases import GRAD_BAR, LAM, STATE_BAR, ratio

MODULE, GOLDEN = "BiRRGCN", "G10_bi_grrgcn_rol"
WIDTHS = (20, 32, 200, 256)      # one partial column tile; exact; the headline width (six tiles + 8); the widest the kernels take
ROW_NS = (1, 31, 33, 97)         # below, across and over the 32-row tile; three tiles + 1
HF_ROWS, HB_ROWS, X_ROWS = 50, 45, 40
ORACLE_LOSS = 24.35783386        # tests/test_lin_chain_cpu.py: the float64 oracle's loss of this model on these draws
LOSS_BAR = 1e-6                  # relative
MODEL_GRAD_BAR = (1e-4, 3e-6)    # tests/test_gpu_lin_stack.py's: rtol, atol . max(1, max |ref|)
GRADS = ("d_x", "d_Hf", "d_Hb", "d_Wf", "d_Wb")


# ---- the row operator -------------------------------------------------------------------------------------------------------
def rows2_inputs(n, d, with_x_rows, seed=29):
    """x, Hf (50 rows), Hb (45 rows), Wf, Wb, rows_f / rows_b (about 40 % -1 each and, from four rows on, rows 0 .. 3 forward only,
    backward only, both, neither, whatever the draw; history rows repeat), x_rows (None, or an index with a -1 and a repeat), dt in
    0 .. 14 per direction and the upstream gradient of `out`."""
    g = torch.Generator().manual_seed(seed + 7 * n + d)
    n_x = X_ROWS if with_x_rows else n
    x, Hf, Hb = (torch.randn(r, d, generator=g) * 0.5 for r in (n_x, HF_ROWS, HB_ROWS))
    Wf, Wb = (torch.randn(d, d, generator=g) / math.sqrt(d) for _ in range(2))
    rows = []
    for r in (HF_ROWS, HB_ROWS):
        h = torch.randint(0, r, (n,), generator=g)
        h[torch.rand(n, generator=g) < 0.4] = -1
        rows.append(h)
    rows_f, rows_b = rows
    rows_f[0], rows_b[0] = 7, (-1 if n >= 4 else 9)     # (n = 1: the one row has both)
    if n >= 4:
        rows_f[1], rows_b[1] = -1, 9
        rows_f[2], rows_b[2] = 7, 9                      # (repeats of rows 0 / 1)
        rows_f[3], rows_b[3] = -1, -1
    x_rows = torch.randint(0, n_x, (n,), generator=g) if with_x_rows else None
    if with_x_rows and n >= 4:
        x_rows[1], x_rows[2] = -1, x_rows[0]
    dt_f, dt_b = (torch.randint(0, 15, (n,), generator=g).float() for _ in range(2))
    up = torch.randn(n, d, generator=g)
    return dict(x=x, Hf=Hf, Hb=Hb, Wf=Wf, Wb=Wb, rows_f=rows_f.int(), rows_b=rows_b.int(), x_rows=None if x_rows is None else x_rows.int(),
                dt_f=dt_f, dt_b=dt_b, up=up)


def kinds(rows_f, rows_b):
    """-> (forward only, backward only, both, neither) row counts."""
    f, b = np.asarray(rows_f) >= 0, np.asarray(rows_b) >= 0
    return int((f & ~b).sum()), int((~f & b).sum()), int((f & b).sum()), int((~f & ~b).sum())


@contextlib.contextmanager
def rows_kernel(on):
    old, TF.LIN_ROWS_KERNEL = TF.LIN_ROWS_KERNEL, on
    try:
        yield
    finally:
        TF.LIN_ROWS_KERNEL = old


def run_rows2_node(c, act, device, kernel=True, absent=None):
    """lin_step_rows2 forward + backward under the upstream gradient c["up"] -> dict(out, d_x, d_Hf, d_Hb, d_Wf, d_Wb) on the CPU.
    absent "f" / "b": that direction's H is None (its d_H is left out; its d_W is None or zero)."""
    leaf = {k: c[k].clone().to(device).requires_grad_(True) for k in ("x", "Hf", "Hb", "Wf", "Wb")}
    t = {k: c[k].to(device) for k in ("rows_f", "rows_b", "dt_f", "dt_b")}
    x_rows = c["x_rows"].to(device) if c["x_rows"] is not None else None
    x_inv = TF.gather_inverse(c["x_rows"].numpy(), c["x"].shape[0], device) if x_rows is not None else None
    f_inv = TF.gather_inverse(c["rows_f"].numpy(), HF_ROWS, device)
    b_inv = TF.gather_inverse(c["rows_b"].numpy(), HB_ROWS, device)
    Hf, Hb = (None if absent == "f" else leaf["Hf"]), (None if absent == "b" else leaf["Hb"])
    with rows_kernel(kernel):
        out = TF.lin_step_rows2(leaf["x"], x_rows, Hf, t["rows_f"], t["dt_f"].view(-1, 1), Hb, t["rows_b"], t["dt_b"].view(-1, 1), LAM,
                                leaf["Wf"], leaf["Wb"], act, x_inv, f_inv, b_inv)
    (out * c["up"].to(device)).sum().backward()
    res = dict(out=out.detach().cpu())
    for k, v in leaf.items():
        if absent is not None and k in ("H" + absent, "W" + absent):
            assert v.grad is None or not bool(v.grad.any()), "a direction without history handed out a gradient: " + k
            continue
        res["d_" + k] = v.grad.cpu()
    return res


def rows2_reference(c, act, mask=None, absent=None):
    """float64 loop over the directions: the decay in front of the product.  mask (n, d) bool: the ReLU mask of the code under test (its
    own out > 0), so that an element within rounding of 0 cannot flip a gradient; None = the reference's own."""
    leaf = {k: c[k].double().clone().requires_grad_(True) for k in ("x", "Hf", "Hb", "Wf", "Wb")}
    x = leaf["x"]
    if c["x_rows"] is not None:
        xr = c["x_rows"].long()
        pre = x[xr.clamp(min=0)] * (xr >= 0).double().view(-1, 1)
    else:
        pre = x
    for s in ("f", "b"):
        if s == absent:
            continue
        r = c["rows_" + s].long()
        hdec = leaf["H" + s][r.clamp(min=0)] * (r >= 0).double().view(-1, 1) * torch.exp(-LAM * c["dt_" + s].double()).view(-1, 1)
        pre = pre + hdec @ leaf["W" + s]
    out = pre if not act else (pre * mask.double() if mask is not None else torch.relu(pre))
    (out * c["up"].double()).sum().backward()
    res = dict(out=out.detach())
    for k, v in leaf.items():
        if absent is None or k not in ("H" + absent, "W" + absent):
            res["d_" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return res


def check_quantities(res, ref, what):
    """out inside STATE_BAR, every gradient inside GRAD_BAR; max err / bar printed first -> {name: ratio}."""
    figs = []
    assert set(res) == set(ref), (sorted(res), sorted(ref))
    for name in sorted(ref):
        bar = STATE_BAR if name == "out" else GRAD_BAR
        r, atol = ratio(res[name], ref[name], bar)
        print("%s: %s max err / bar %.3g (max |ref| %.3g)" % (what, name, r, float(ref[name].abs().max())))
        figs.append((name, bar[0], atol, r))
    for name, rtol, atol, _ in figs:
        assert_close(res[name], ref[name], rtol, atol, what + " " + name)
    return {f[0]: f[-1] for f in figs}


def check_rows2_node(n, d, act, device, kernel=True):
    """One (rows, width, activation) case of the node against the float64 loop, with and without x_rows."""
    for with_x_rows in (False, True):
        c = rows2_inputs(n, d, with_x_rows)
        if n >= 4:
            assert min(kinds(c["rows_f"], c["rows_b"])) >= 1
        res = run_rows2_node(c, act, device, kernel)
        ref = rows2_reference(c, act, res["out"] > 0 if act else None)
        check_quantities(res, ref, "n = %d d = %d act = %d x_rows = %s%s" % (n, d, act, "index" if with_x_rows else "None", "" if kernel else " (composition)"))


def check_absent_direction(d, device, kernel=True):
    """One direction's H is None (windows of length 1): as if every row index of it were -1."""
    for absent in ("f", "b"):
        c = rows2_inputs(33, d, True)
        res = run_rows2_node(c, 1, device, kernel, absent)
        ref = rows2_reference(c, 1, res["out"] > 0, absent)
        check_quantities(res, ref, "d = %d H%s = None%s" % (d, absent, "" if kernel else " (composition)"))


ONE_SOURCE_N, ONE_SOURCE_WIDTHS = 33, (20, 200)     # two workgroups, the second with one live row; one padded tile, seven tiles (waves
                                                    # 0 .. 2 use their second accumulator, wave 3 does not)


def one_source_inputs(d):
    """rows2_inputs(33, d, x_rows given) with the forward row list redrawn: about a quarter -1; row 0 has a history row, row 1 none, row
    32 (the second workgroup's one live row) repeats row 0's."""
    c = rows2_inputs(ONE_SOURCE_N, d, True)
    g = torch.Generator().manual_seed(53 + d)
    h = torch.randint(0, HF_ROWS, (ONE_SOURCE_N,), generator=g)
    h[torch.rand(ONE_SOURCE_N, generator=g) < 0.25] = -1
    h[0], h[1], h[ONE_SOURCE_N - 1] = 7, -1, 7
    assert 4 <= int((h < 0).sum()) <= 13
    c["rows_f"] = h.int()
    return c


def run_one_source(c, device, two):
    """The forward direction alone, ReLU on, under the upstream gradient c["up"]: lin_step_rows (two False) or lin_step_rows2 with
    Hb = None (two True) -> dict(out, d_x, d_Hf, d_Wf) on the CPU."""
    leaf = {k: c[k].clone().to(device).requires_grad_(True) for k in ("x", "Hf", "Wf", "Wb")}
    x_rows, rows_f, dt_f = c["x_rows"].to(device), c["rows_f"].to(device), c["dt_f"].to(device).view(-1, 1)
    x_inv = TF.gather_inverse(c["x_rows"].numpy(), c["x"].shape[0], device)
    f_inv = TF.gather_inverse(c["rows_f"].numpy(), HF_ROWS, device)
    if two:
        out = TF.lin_step_rows2(leaf["x"], x_rows, leaf["Hf"], rows_f, dt_f, None, None, None, LAM, leaf["Wf"], leaf["Wb"], 1, x_inv, f_inv, None)
    else:
        out = TF.lin_step_rows(leaf["x"], x_rows, leaf["Hf"], rows_f, dt_f, LAM, leaf["Wf"], 1, x_inv, f_inv)
    (out * c["up"].to(device)).sum().backward()
    assert leaf["Wb"].grad is None or not bool(leaf["Wb"].grad.any())
    return dict(out=out.detach().cpu(), d_x=leaf["x"].grad.cpu(), d_Hf=leaf["Hf"].grad.cpu(), d_Wf=leaf["Wf"].grad.cpu())


def check_one_source(d, device, exact):
    """lin_step_rows2 with the backward direction absent against lin_step_rows on the same inputs.  exact (the kernel route): equal to
    the bit -- both kernels decay in front of the product and walk source 0 first, and the absent source adds products with exact
    zeros, which change no finite accumulator value.  Not exact (the two torch compositions round in different orders: the decay
    behind the product against in front of it): out inside STATE_BAR, the gradients inside GRAD_BAR."""
    c = one_source_inputs(d)
    one, two = run_one_source(c, device, False), run_one_source(c, device, True)
    assert float(one["out"].abs().max()) > 0 and bool((one["out"] == 0).any()), "the ReLU cuts some elements and not all"
    if not exact:
        return check_quantities(two, one, "d = %d, one source: lin_step_rows2(Hb = None) against lin_step_rows" % d)
    for k in sorted(one):
        diff = float((two[k] - one[k]).abs().max())
        print("d = %d, one source: %s max |lin_step_rows2(Hb = None) - lin_step_rows| = %.3g" % (d, k, diff))
    for k in sorted(one):
        assert torch.equal(two[k], one[k]), k


# ---- the window model ---------------------------------------------------------------------------------------------------------
def bi_model(device, on, dropout=0.0):
    m, _, _, z = LC.window_model(MODULE, GOLDEN, device, dropout=dropout)
    m.bi_pair_pass = on
    return m, z


def golden_inputs(z):
    from tests.window_cases import window_inputs
    edge_ids, samples = window_inputs(z)
    return torch.tensor([int(t) for t in z["t_list"]]), int(z["L"]), edge_ids, samples


def loss_and_grads(device, on, L=None):
    m, z = bi_model(device, on)
    t_list, L0, edge_ids, samples = golden_inputs(z)
    wb = m.prepare(t_list, L if L is not None else L0, True, edge_ids)
    assert wb.batched and bool(m._fused_all_entity_ok(wb)) == on
    loss = m.run_loss(wb, samples)
    loss.backward()
    return loss.detach().cpu(), {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters() if v.grad is not None}


def check_on_vs_off(device, L=None, oracle=True):
    """Loss and every parameter gradient with the attribute on against the attribute off on the same draws (L: another window length
    than the golden's); the loss also against the float64 oracle's recorded figure."""
    (l1, g1), (l0, g0) = loss_and_grads(device, True, L), loss_and_grads(device, False, L)
    rel = abs(l1.item() - l0.item()) / abs(l0.item())
    print("BiRRGCN L = %s: loss on %.8f off %.8f (%.3g relative)" % (L, l1.item(), l0.item(), rel))
    worst = 0.0
    for k in g0:
        if k in g1:
            worst = max(worst, ratio(g1[k], g0[k], MODEL_GRAD_BAR)[0])
    print("BiRRGCN L = %s: gradients on vs off, max err / bar %.3g" % (L, worst))
    if oracle:
        print("BiRRGCN: loss on against the float64 oracle's %.8f: %.3g relative" % (ORACLE_LOSS, abs(l1.item() - ORACLE_LOSS) / ORACLE_LOSS))
    assert rel < LOSS_BAR, (l1.item(), l0.item())
    # (windows of length 1: the off arm multiplies zero states into the time weights and hands them a zero gradient, the on arm none)
    assert set(g1) <= set(g0) and len(g1) >= 6 and all(not bool(g0[k].any()) for k in set(g0) - set(g1)), (sorted(g0), sorted(g1))
    assert L == 1 or set(g0) == set(g1)
    for k in g1:
        assert_close(g1[k], g0[k], MODEL_GRAD_BAR[0], MODEL_GRAD_BAR[1] * max(1.0, float(g0[k].abs().max())), "on vs off: d_" + k)
    if oracle:
        assert abs(l1.item() - ORACLE_LOSS) < LOSS_BAR * ORACLE_LOSS, (l1.item(), ORACLE_LOSS)
        for k in LC.time_weight_names(MODULE):
            assert float(g1[k].abs().max()) > 0, k


def union_kinds(m, wb):
    (mp,) = m._all_maps(wb)
    return kinds(mp["idx_f_host"], mp["idx_b_host"])


def check_all_embeds(device, force_rep):
    """all_embeds_batched against the stack of get_all_embeds_Gt over the windows, on a batch whose union map holds pairs of every
    kind (forward only, backward only, both)."""
    m, z = bi_model(device, True)
    m._force_all_rep = force_rep
    t_list, L, edge_ids, _ = golden_inputs(z)
    wb = m.prepare(t_list, L, True, edge_ids)
    nf, nb, nboth, none = union_kinds(m, wb)
    print("union pairs: %d forward only, %d backward only, %d both" % (nf, nb, nboth))
    assert nf > 0 and nb > 0 and nboth > 0 and none == 0, (nf, nb, nboth, none)
    with torch.no_grad():
        out, hist = m.run(wb)
        big = m.all_embeds_batched(wb, out, hist)
        assert bool(wb.all_rep) == force_rep
        per = list(out.split(wb.target.sizes))
        ref = torch.stack([m.get_all_embeds_Gt(per[b], g, wb.rows[b][-1], wb.plan, b, hist) for b, g in enumerate(wb.graphs)])
    r, atol = ratio(big.cpu(), ref.cpu(), STATE_BAR)
    print("all_embeds_batched (rep = %s) vs get_all_embeds_Gt: max err / bar %.3g" % (force_rep, r))
    assert_close(big.cpu(), ref.cpu(), STATE_BAR[0], atol, "all_embeds_batched vs get_all_embeds_Gt")


def check_dropout(device):
    """While the self-loop dropout draws the pass keeps one row per (window, entity): two windows' inactive rows of one entity differ
    (each window its own mask), and two runs on one seed are bit-equal."""
    m, z = bi_model(device, True, dropout=0.1)
    m.train()
    t_list, L, edge_ids, _ = golden_inputs(z)
    wb = m.prepare(t_list, L, True, edge_ids)
    assert wb.batched and m._fused_all_entity_ok(wb)
    bigs = []
    for _ in range(2):
        torch.manual_seed(5)
        out, hist = m.run(wb)
        bigs.append(m.all_embeds_batched(wb, out, hist))
    big = bigs[0]
    assert torch.equal(bigs[0], bigs[1])
    assert wb.all_rep and big.shape[:2] == (len(wb.graphs), m.num_ents) and bool(torch.isfinite(big).all())
    act = np.zeros((len(wb.graphs), m.num_ents), dtype=bool)
    for b, g in enumerate(wb.graphs):
        act[b, g.gids] = True
    both = np.nonzero(~act[0] & ~act[1])[0]
    assert both.size > 10
    rows = torch.from_numpy(both).to(big.device)
    assert float((big[0][rows] != big[1][rows]).float().mean()) > 0.05, "two windows' inactive rows of one entity share a dropout mask"
    big.sum().backward()
    l2 = m.ent_encoder.layer_2
    assert float(l2.time_weight_forward.grad.abs().max()) > 0 and float(l2.time_weight_backward.grad.abs().max()) > 0


def step_calls(device, setting):
    """Names of the backend launches of one run_loss + backward (queries left out) -> (names, L, B).  setting True / False: the
    attribute set on the model; "deleted": the class attribute removed for the run (the model as it was before the attribute)."""
    from temp_amd.bi_dynamic_rgcn import BiDynamicRGCN
    m, z = bi_model(device, bool(setting) if setting != "deleted" else False)
    saved = BiDynamicRGCN.bi_pair_pass
    if setting == "deleted":
        del m.bi_pair_pass
        del BiDynamicRGCN.bi_pair_pass
    inner = TB.get_backend()
    rec = Launches(inner)
    try:
        t_list, L, edge_ids, samples = golden_inputs(z)
        wb = m.prepare(t_list, L, True, edge_ids)
        TB.set_backend(rec)
        m.run_loss(wb, samples).backward()
    finally:
        TB.set_backend(inner)
        BiDynamicRGCN.bi_pair_pass = saved
    return [c[0] for c in rec.calls if not c[0].endswith(QUERIES)], L, len(wb.graphs)
