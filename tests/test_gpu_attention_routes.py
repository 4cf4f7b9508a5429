"""The history attention kernels (temp_amd/csrc/attn_kernels.hip) on the MI355X: every case of tests/attention_route_cases.py through
all four routes -- temp_sa_attn_fwd / _bwd and temp_sa_attn_split_fwd / _bwd, each with the atomic and the table-pass backward --
against the fp64 dense formulation (tests/test_attention_route_cases_cpu.py checks the host-side facts the cases rest on).

A case calls the C ABI directly, with leading dimensions the wrappers of temp_amd/backend.py cannot express: q, kc and vc are three
allocations with ldq = D + 8 != ldc = D + 12, ldh = 2D + 4, ld_dq = D + 12, ld_dc = D + 20, ld_dh = 2D + 8, lda = 3D + 4,
ldb = 3D + 16, ld_dqkv = 3D + 8; one case per MAXC also runs with the packed strides of backend.py.  Every input's pad columns hold
NaN; every output is NaN-filled, pad columns and 64 guard rows included -- but the [R, D] payloads of d_kh / d_vh on the atomic
route and d_decay [T], which the caller zeroes.  Checked per case, layout and route:
  * every payload element finite (score: -inf exactly where the reference masks) and within the bars of the cases module against
    fp64; on exact data every declared tensor equal with `==`;
  * every pad column and guard row still holds the NaN bit pattern;
  * table rows nobody attends are exactly 0 in d_kh / d_vh on both backward routes;
  * the split routes bit-equal to the plain routes fed the fp32 sum: out, lse, the score bit patterns, d_q / d_k / d_v and the
    table-pass history gradient;
  * two runs of the table-pass backward bit-equal in every tensor but d_decay (atomics in both forms);
  * launches: forward [k_sa_attn_fwd], atomic backward [k_sa_attn_bwd], table-pass backward twice k_sa_attn_bwd (the trace's name
    of both of its kernels); T = 1 with inverse maps given takes the atomic form; n = 0 and every refused call launch nothing.

Measured on the MI355X, worst |got - ref| / bar over all cases, layouts and routes of a regime (pytest -s prints each):
  regime   out    lse    score  d_q    d_k    d_v    d_kh   d_vh   d_decay
  real     0.085  0.109  0.131  0.210  0.079  0.019  0.199  0.059  0.043      (d_q: d200_t64; d_kh: d72_t64; out, score: hub)
  stress   0.074  0.097  0.090  0.137  0.012  0.014  0.108  0.081  0.014      (d_q, d_kh: stress_d200_t33)
  uniform  0      0      0      0.437  0      0      0      0      0          (d_q where d_k is no power of four: uni_hub)
  onehot   0      0      0      0      0      0      0      0      0
  autograd nodes (d128_t9): out 0.056, d_q 0.103, d_kh 0.092, d_decay 0.019, d_pa 0.054, d_pb 0.007
The MAXC = 2 band (D = 72, 128) at unit scale stays below 0.20 at T = 64 and below 0.13 at T = 9.  The whole module runs 2 s.

What these cases found: with the forward's running sums rounded to fp32 at every position, stress_d72_t64 (q x2, T = 64, no decay) had
d_kh at 1.287 of its bar and d_q at 0.650 on all four routes, the fp32 dense formulation being at 0.123 / 0.063.  Row 2 of the recipe
puts 63 positions on ONE table row: their scores are equal, dp - delta is 0.014 where dp and delta are 4.45, and delta = <d_out, out>
carried the several ulps that `out` had gathered over 64 accumulation steps -- the same error in all 63 score gradients, summed
into one row of d_kh.  An fp32 model of the kernel's arithmetic on the host gave 1.284 with the plain sums and 0.068 with compensated
ones; k_sa_attn_fwd now keeps its sums in two floats (scale_add2), and the case measures 0.065 (d_q 0.049)."""
import ctypes

import pytest
import torch

from temp_amd import _lib
from temp_amd import backend as TB
from temp_amd import functional as TF
from tests import attention_route_cases as AC
from tests.golden_util import assert_close
from tests.poison import poisoned_allocations_fixture  # noqa: F401  (registers the fixture)
from tests.test_gpu_row_loss_routes import _traced

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_allocations")]
DEV = torch.device("cuda:0")
E_BADARG, E_UNSUPPORTED = 1, 2                               # include/temp_amd.h
NAN = float("nan")
FWD, BWD, BWD_TABLE = ["k_sa_attn_fwd"], ["k_sa_attn_bwd"], ["k_sa_attn_bwd", "k_sa_attn_bwd"]
FWD_NAMES = ("out", "lse", "score")
ROW_GRADS = ("d_q", "d_k", "d_v")
HIST_GRADS = ("d_kh", "d_vh")


@pytest.fixture(autouse=True)
def hip_backend():
    TB.set_backend(None)
    be = TB.get_backend()
    assert be.name == "hip"
    yield be
    TB.set_backend(None)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(rows, ld):
    """a NaN-filled output of `rows` rows of `ld` floats with GUARD guard rows behind"""
    return torch.full((rows + AC.GUARD, ld), NAN, device=DEV)


def _pad(t, ld):
    """the rows of host tensor t on the device at leading dimension ld, NaN in the pad columns"""
    buf = torch.full((t.shape[0], ld), NAN, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(buf, rows, cols):
    """the guard rows and pad columns of an output still hold the NaN bit pattern"""
    b = buf.view(torch.int32)
    return bool((b[rows:] == AC.NAN_BITS).all()) and bool((b[:rows, cols:] == AC.NAN_BITS).all())


def strides(D, packed):
    if packed:
        return dict(ldq=3 * D, ldc=3 * D, ldh=2 * D, ld_dq=3 * D, ld_dc=3 * D, ld_dh=2 * D, lda=3 * D, ldb=3 * D, ld_dqkv=3 * D)
    return dict(ldq=D + 8, ldc=D + 12, ldh=2 * D + 4, ld_dq=D + 12, ld_dc=D + 20, ld_dh=2 * D + 8, lda=3 * D + 4, ldb=3 * D + 16, ld_dqkv=3 * D + 8)


class Calls:
    """the raw entry points of one case in one layout; every call allocates its outputs afresh"""

    def __init__(self, lib, case, packed):
        inp = AC.inputs(case)
        self.lib, self.c, self.inp, self.packed = lib, case, inp, packed
        self.n, self.D, self.T, self.R = case.n, case.D, case.T, inp.R
        n, D = self.n, self.D
        self.L = L = strides(D, packed)
        if packed:
            self.qkv = inp.qkv.to(DEV)
            base = self.qkv.data_ptr()
            self.cur = (base, base + 4 * D, base + 8 * D)
        else:
            self.q, self.kc, self.vc = _pad(inp.qkv[:, :D], L["ldq"]), _pad(inp.qkv[:, D:2 * D], L["ldc"]), _pad(inp.qkv[:, 2 * D:], L["ldc"])
            self.cur = (self.q.data_ptr(), self.kc.data_ptr(), self.vc.data_ptr())
        self.kvh = _pad(inp.kvh, L["ldh"]) if self.T > 1 else None
        self.pa, self.pb = _pad(inp.pa, L["lda"]), _pad(inp.pb, L["ldb"])
        self.ia, self.ib, self.idx = inp.ia.to(DEV), inp.ib.to(DEV), inp.idx.contiguous().to(DEV)
        self.decay = inp.decay.to(DEV) if inp.decay is not None else None
        self.d_out = inp.d_out.to(DEV)
        self.inv = TF.attention_inverse(inp.idx.numpy(), self.R, DEV) if self.T > 1 else (torch.zeros(1, dtype=torch.int32, device=DEV), None)

    def desc(self, split):
        a = _lib.TempAttn()
        a.n, a.D, a.heads, a.T = self.n, self.D, 8, self.T
        if not split:                                        # (split: q / kc / vc are not read and stay NULL)
            a.q, a.kc, a.vc = self.cur
            a.ldq, a.ldc = self.L["ldq"], self.L["ldc"]
        if self.T > 1:
            a.kh, a.vh, a.ldh, a.idx = self.kvh.data_ptr(), self.kvh.data_ptr() + 4 * self.D, self.L["ldh"], self.idx.data_ptr()
        a.decay = self.decay.data_ptr() if self.decay is not None else None
        return a

    def split_desc(self):
        s = _lib.TempAttnSplit()
        s.pa, s.ia, s.lda = self.pa.data_ptr(), self.ia.data_ptr(), self.L["lda"]
        s.pb, s.ib, s.ldb = self.pb.data_ptr(), self.ib.data_ptr(), self.L["ldb"]
        return s

    def fwd(self, split):
        """-> (rc, {name: payload}, everything outside the payloads untouched)"""
        n, D, T = self.n, self.D, self.T
        a = self.desc(split)
        out, score, lse = _nan(n, D), _nan(n, 8 * T), _nan(n, 8)
        if split:
            rc = self.lib.temp_sa_attn_split_fwd(ctypes.byref(a), ctypes.byref(self.split_desc()), _p(out), _p(score), _p(lse), _stream())
        else:
            rc = self.lib.temp_sa_attn_fwd(ctypes.byref(a), _p(out), _p(score), _p(lse), _stream())
        torch.cuda.synchronize()
        clean = _untouched(out, n, D) and _untouched(score, n, 8 * T) and _untouched(lse, n, 8)
        return rc, {"out": out[:n], "score": score[:n].view(n, 8, T), "lse": lse[:n]}, clean

    def bwd(self, split, table, f):
        """f: the payloads of this route's forward -> (rc, {name: payload}, everything outside the payloads untouched)"""
        n, D, T, R, L = self.n, self.D, self.T, self.R, self.L
        a = self.desc(split)
        d_h = d_kh = d_vh = None
        if T > 1:
            d_h = _nan(R, L["ld_dh"])
            if not table:
                d_h[:R, :2 * D] = 0                          # the atomic form accumulates: exactly the [R, D] payloads are zeroed
            d_kh, d_vh = ctypes.c_void_p(d_h.data_ptr()), ctypes.c_void_p(d_h.data_ptr() + 4 * D)
        d_decay = None
        if self.decay is not None:
            d_decay = _nan(T, 1)
            d_decay[:T] = 0
        inv_ptr, inv_ref = self.inv if table else (None, None)
        ds_ws = torch.full((n * 8 * T + 64,), NAN, device=DEV) if table and T > 1 else None
        fixed = (_p(f["out"]), _p(f["score"]), _p(f["lse"]), _p(self.d_out))
        tail = (_p(d_decay), R, _p(inv_ptr), _p(inv_ref), _p(ds_ws), _stream())
        if split:
            d_qkv = _nan(n, L["ld_dqkv"])
            rc = self.lib.temp_sa_attn_split_bwd(ctypes.byref(a), ctypes.byref(self.split_desc()), *fixed, _p(d_qkv), L["ld_dqkv"], d_kh, d_vh, L["ld_dh"], *tail)
            g = {"d_q": d_qkv[:n, :D], "d_k": d_qkv[:n, D:2 * D], "d_v": d_qkv[:n, 2 * D:3 * D]}
            bufs = [(d_qkv, n, 3 * D)]
        elif self.packed:
            d_qkv = _nan(n, 3 * D)
            b = d_qkv.data_ptr()
            vp = ctypes.c_void_p
            rc = self.lib.temp_sa_attn_bwd(ctypes.byref(a), *fixed, vp(b), 3 * D, d_kh, d_vh, L["ld_dh"], vp(b + 4 * D), vp(b + 8 * D), 3 * D, *tail)
            g = {"d_q": d_qkv[:n, :D], "d_k": d_qkv[:n, D:2 * D], "d_v": d_qkv[:n, 2 * D:]}
            bufs = [(d_qkv, n, 3 * D)]
        else:
            d_q, d_kc, d_vc = _nan(n, L["ld_dq"]), _nan(n, L["ld_dc"]), _nan(n, L["ld_dc"])
            rc = self.lib.temp_sa_attn_bwd(ctypes.byref(a), *fixed, _p(d_q), L["ld_dq"], d_kh, d_vh, L["ld_dh"], _p(d_kc), _p(d_vc), L["ld_dc"], *tail)
            g = {"d_q": d_q[:n, :D], "d_k": d_kc[:n, :D], "d_v": d_vc[:n, :D]}
            bufs = [(d_q, n, D), (d_kc, n, D), (d_vc, n, D)]
        torch.cuda.synchronize()
        if T > 1:
            g["d_kh"], g["d_vh"] = d_h[:R, :D], d_h[:R, D:2 * D]
            bufs.append((d_h, R, 2 * D))
        if d_decay is not None:
            g["d_decay"] = d_decay[:T, 0]
            bufs.append((d_decay, T, 1))
        return rc, g, all(_untouched(*b) for b in bufs)


def _compare(tag, got, ref, names, exact, bad, ratios):
    """the payloads `names` of one call against fp64 -> ratios[name] = worst err / bar; problems go to bad()"""
    for k in names:
        if k not in got:
            continue
        r = AC.ratio(k, got[k], ref[k], ref)
        ratios[k] = max(ratios.get(k, 0.0), r)
        if k in exact:
            if not torch.equal(got[k].cpu().double(), AC.exact_want(ref[k])):
                bad("%s: %s is not exact (err / bar %.3g)" % (tag, k, r))
        elif k in HIST_GRADS or k == "score":
            if not r <= 1.0:
                bad("%s: %s at %.3g of its bar" % (tag, k, r))
        else:
            try:
                assert_close(got[k], ref[k], *AC.BARS[k], what="%s: %s" % (tag, k))
            except AssertionError as e:
                bad(str(e))


def measure(case, packed=False):
    """every route of a case in one layout -> ({route: {tensor: worst err / bar}}, problems).  Nothing is asserted here."""
    lib = _lib.load()
    calls, ref = Calls(lib, case, packed), AC.reference(case)
    exact = AC.exact_tensors(case)
    problems, report, kept = [], {}, {}
    bad = problems.append
    unref = (ref["cnt"] == 0).to(DEV)
    for split in (False, True):
        route = "split" if split else "plain"
        (rc, f, clean), names = _traced(lambda: calls.fwd(split))
        _lib.check(rc, "%s %s forward" % (case.id, route))
        if names != FWD:
            bad("%s forward launched %s" % (route, names))
        if not clean:
            bad("%s forward wrote outside its payloads" % route)
        ratios = {}
        _compare(route, f, ref, FWD_NAMES, exact, bad, ratios)
        kept[(route, "fwd")] = f
        for table in (False, True):
            form = "table" if table else "atomic"
            tag = "%s %s" % (route, form)
            (rc, g, clean), names = _traced(lambda: calls.bwd(split, table, f))
            _lib.check(rc, "%s %s backward" % (case.id, tag))
            if names != (BWD_TABLE if table and case.T > 1 else BWD):
                bad("%s backward launched %s" % (tag, names))
            if not clean:
                bad("%s backward wrote outside its payloads" % tag)
            r = dict(ratios)
            _compare(tag, g, ref, ROW_GRADS + HIST_GRADS + ("d_decay",), exact, bad, r)
            if case.T > 1 and not (bool((g["d_kh"][unref] == 0).all()) and bool((g["d_vh"][unref] == 0).all())):
                bad("%s: table rows nobody attends are not exactly zero" % tag)
            report[tag] = r
            kept[(route, form)] = g
        rc, g2, _ = calls.bwd(split, True, f)
        _lib.check(rc, "%s %s second table-pass backward" % (case.id, route))
        g1 = kept[(route, "table")]
        for k in g1:
            if k != "d_decay" and not torch.equal(_bits(g1[k]), _bits(g2[k])):
                bad("%s table-pass backward: two runs differ in %s" % (route, k))
    # the header's contract: the split routes are the plain routes fed the fp32 sum, bit for bit
    for k in FWD_NAMES:
        if not torch.equal(_bits(kept[("split", "fwd")][k]), _bits(kept[("plain", "fwd")][k])):
            bad("split forward differs from the plain forward in the bits of %s" % k)
    for form in ("atomic", "table"):
        for k in ROW_GRADS + (HIST_GRADS if form == "table" and case.T > 1 else ()):
            if not torch.equal(_bits(kept[("split", form)][k]), _bits(kept[("plain", form)][k])):
                bad("split %s backward differs from the plain one in the bits of %s" % (form, k))
    for tag, r in report.items():
        print("attention %s%s %s: max err/bar %s" % (case.id, " packed" if packed else "", tag, " ".join("%s %.3f" % kv for kv in r.items())))
    return report, problems


RUNS = [(c, False) for c in AC.ALL] + [(c, True) for c in AC.ALL if c.packed]


@pytest.mark.parametrize("case,packed", RUNS, ids=[c.id + ("-packed" if p else "") for c, p in RUNS])
def test_attention_routes(case, packed):
    report, problems = measure(case, packed)
    assert not problems, "; ".join(problems)


def _desc(n, D, T, heads=8):
    a = _lib.TempAttn()
    a.n, a.D, a.heads, a.T = n, D, heads, T
    return a


def test_plain_attention_arguments(hip_backend):
    """the return contract of temp_sa_attn_fwd / _bwd (the split pair's: tests/test_gpu_post_attention.py); nothing is launched on
    any error or for n = 0"""
    lib = hip_backend.lib
    D, n, T, R = 32, 5, 3, 6
    t = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    qkv, kvh, d_out = t(n, 3 * D), t(R, 2 * D), t(n, D)
    idx = torch.full((n, T - 1), -1, dtype=torch.int32, device=DEV)
    out, score, lse = t(n, D), t(n, 8, T), t(n, 8)
    d_qkv, d_hist, ds_ws = t(n, 3 * D), t(R, 2 * D), t(n * 8 * T)
    inv_ptr, inv_ref = torch.zeros(R + 1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    vp = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + 4 * off) if x is not None else None

    def desc(n_=n, D_=D, T_=T, heads=8, drop=()):
        a = _desc(n_, D_, T_, heads)
        a.q, a.kc, a.vc, a.ldq, a.ldc = qkv.data_ptr(), qkv.data_ptr() + 4 * D, qkv.data_ptr() + 8 * D, 3 * D, 3 * D
        a.kh, a.vh, a.ldh, a.idx = kvh.data_ptr(), kvh.data_ptr() + 4 * D, 2 * D, idx.data_ptr()
        for name in drop:
            setattr(a, name, None)
        return a

    def fwd(a, o=out, s=score, l=lse):
        rc, names = _traced(lambda: lib.temp_sa_attn_fwd(ctypes.byref(a), vp(o), vp(s), vp(l), None))
        torch.cuda.synchronize()
        return rc, names

    def bwd(a, d_kh=d_hist, n_table=R, ptr=None, ref=None, ws=None, d_q=d_qkv):
        rc, names = _traced(lambda: lib.temp_sa_attn_bwd(ctypes.byref(a), vp(out), vp(score), vp(lse), vp(d_out), vp(d_q), 3 * D, vp(d_kh),
                                                         vp(d_kh, D), 2 * D, vp(d_q, D), vp(d_q, 2 * D), 3 * D, None, n_table, vp(ptr), vp(ref), vp(ws), None))
        torch.cuda.synchronize()
        return rc, names

    assert fwd(desc()) == (0, FWD) and bwd(desc()) == (0, BWD)
    assert bwd(desc(), ptr=inv_ptr, ref=inv_ref, ws=ds_ws) == (0, BWD_TABLE)
    # n = 0 succeeds with NULL buffers
    a0 = _desc(0, D, T)
    assert _traced(lambda: lib.temp_sa_attn_fwd(ctypes.byref(a0), None, None, None, None)) == (0, [])
    assert _traced(lambda: lib.temp_sa_attn_bwd(ctypes.byref(a0), None, None, None, None, None, 0, None, None, 0, None, None, 0, None, 0, None, None, None,
                                                None)) == (0, [])
    for a in (desc(heads=4), desc(D_=36), desc(D_=520), desc(T_=65)):
        assert fwd(a) == (E_UNSUPPORTED, []) and bwd(a) == (E_UNSUPPORTED, [])
    refused = [desc(T_=0)] + [desc(drop=(k,)) for k in ("q", "kc", "vc", "idx", "kh", "vh")]
    for a in refused:
        assert fwd(a) == (E_BADARG, []) and bwd(a) == (E_BADARG, [])
    assert fwd(desc(), None) == (E_BADARG, []) and fwd(desc(), out, None) == (E_BADARG, []) and fwd(desc(), out, score, None) == (E_BADARG, [])
    assert bwd(desc(), None) == (E_BADARG, [])                                           # NULL d_kh at T > 1
    assert bwd(desc(), ptr=inv_ptr, ref=inv_ref, ws=None) == (E_BADARG, [])              # the table form needs its scratch,
    assert bwd(desc(), ptr=inv_ptr, ref=None, ws=ds_ws) == (E_BADARG, [])                # its reference list
    for n_table in (0, -1):
        assert bwd(desc(), n_table=n_table, ptr=inv_ptr, ref=inv_ref, ws=ds_ws) == (E_BADARG, [])      # and a table
    # T = 1: the inverse maps are ignored (the atomic form), no history buffer is needed
    a1 = desc(T_=1, drop=("idx", "kh", "vh"))
    score1 = t(n, 8, 1)
    assert fwd(a1, out, score1, lse) == (0, FWD)
    runs = []
    for ptr in (None, inv_ptr):
        g = torch.full((n, 3 * D), NAN, device=DEV)
        rc, names = _traced(lambda: lib.temp_sa_attn_bwd(ctypes.byref(a1), vp(out), vp(score1), vp(lse), vp(d_out), vp(g), 3 * D, None, None, 0, vp(g, D),
                                                         vp(g, 2 * D), 3 * D, None, 0, vp(ptr), None, None, None))
        torch.cuda.synchronize()
        assert (rc, names) == (0, BWD)
        runs.append(g)
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and bool(torch.isfinite(runs[0]).all())


def test_autograd_nodes(hip_backend):
    """TF.history_attention and TF.split_history_attention with inverse maps on the MAXC = 2 case D = 128, T = 9: out and every leaf
    gradient against fp64 at the bars.  d_pa / d_pb are sums of rows of d_qkv over ia / ib: each summed element may miss by its own
    bar, and summing m fp32 terms in any order adds at most m 2^-24 sum |term| (the form of test_split_attention_kernels)."""
    case = AC.BY_ID[AC.AUTOGRAD_CASE]
    inp, ref = AC.inputs(case), AC.reference(case)
    n, D = case.n, case.D
    dev = lambda x: x.to(DEV) if x is not None else None
    pa, ia, pb, ib, qkv, kvh, idx, dec, d_out = (dev(x) for x in inp[:9])
    inv = TF.attention_inverse(inp.idx.numpy(), inp.R, DEV)
    inv_a, inv_b = TF.split_row_inverse(inp.ia.numpy(), case.na, DEV), TF.split_row_inverse(inp.ib.numpy(), case.nb, DEV)
    leaf = lambda x: x.clone().requires_grad_(True)

    def plain():
        a, b, c = leaf(qkv), leaf(kvh), leaf(dec)
        o = TF.history_attention(a, b, idx, c, inv)
        o.backward(d_out)
        return {"out": o.detach(), "d_qkv": a.grad, "d_hist": b.grad, "d_decay": c.grad}

    def split():
        a, a2, b, c = leaf(pa), leaf(pb), leaf(kvh), leaf(dec)
        o = TF.split_history_attention(a, ia, a2, ib, b, idx, c, inv, inv_a, inv_b)
        o.backward(d_out)
        return {"out": o.detach(), "d_pa": a.grad, "d_pb": a2.grad, "d_hist": b.grad, "d_decay": c.grad}

    ref_qkv = torch.cat([ref["d_q"], ref["d_k"], ref["d_v"]], dim=1)
    bar_qkv = torch.cat([AC.bar(k, ref[k]) for k in ROW_GRADS], dim=1)
    problems = []
    for name, node in (("history_attention", plain), ("split_history_attention", split)):
        r1, r2 = node(), node()
        for k in r1:
            if k != "d_decay" and not torch.equal(_bits(r1[k]), _bits(r2[k])):
                problems.append("%s: two runs differ in %s" % (name, k))
        got = {"out": r1["out"], "d_kh": r1["d_hist"][:, :D], "d_vh": r1["d_hist"][:, D:], "d_decay": r1["d_decay"]}
        if "d_qkv" in r1:
            got.update(d_q=r1["d_qkv"][:, :D], d_k=r1["d_qkv"][:, D:2 * D], d_v=r1["d_qkv"][:, 2 * D:])
        ratios = {}
        _compare(name, got, ref, ("out",) + ROW_GRADS + HIST_GRADS + ("d_decay",), (), problems.append, ratios)
        for k, index, n_tab in (("d_pa", inp.ia, case.na), ("d_pb", inp.ib, case.nb)):
            if k not in r1:
                continue
            z = lambda: torch.zeros(n_tab, 3 * D, dtype=torch.float64)
            want, mag = z().index_add_(0, index.long(), ref_qkv), z().index_add_(0, index.long(), ref_qkv.abs())
            m = torch.bincount(index.long(), minlength=n_tab).double().view(-1, 1)
            tol = z().index_add_(0, index.long(), bar_qkv) + m * 2.0 ** -24 * mag
            g = r1[k].double().cpu()
            ratios[k] = float(((g - want).abs() / tol).nan_to_num(nan=float("inf")).max())
            if not (bool(torch.isfinite(g).all()) and ratios[k] <= 1.0):
                problems.append("%s: %s at %.3g of its bar" % (name, k, ratios[k]))
        print("attention %s %s: max err/bar %s" % (case.id, name, " ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not problems, "; ".join(problems)
