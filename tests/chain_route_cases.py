"""Which backend calls gru_chain makes on each of its routes: the cases and the runner shared by the CPU (test backend) and GPU
(HIP) suites.  A case is one gru_chain forward + backward under a Recording of the installed backend; what the suites compare is the
ordered list of (method name, shapes of the tensor arguments, keywords given) without the query methods.  The expected lists are literals in the
test files, recorded by run_route on the commit BEFORE _GruChainFn was split by route (never on the code under test): the kernel
tests compare numbers, so a route that silently falls back to a slower one passes them -- these do not."""
import contextlib

import numpy as np
import torch

from temp_amd import backend as TB
from temp_amd import gru_chain as GC
from temp_amd.gru_chain import GruInstance, GruProgram
from tests.chain_cases import make_rnns, random_program
from tests.post_attention_cases import Recording

QUERIES = ("_supported", "_layout", "_launches")       # a name ending in one of these asks the backend something: not a launch
DECAY = (0.3, -0.7)          # dt in {1, 2, 3, 4} -> w dt + b in {-0.4, -0.1, 0.2, 0.5}: two clamped, two active
T_ROWS = 7                   # rows of the offset table


def shared_centre_program():
    """Two chains of three dense positions whose LAST instances read the same x rows (the centre of a bi-directional window):
    the groups' x rows overlap, so the weight gradients go group by group and the second writer of d_x accumulates."""
    n, idx = 12, np.arange(12, dtype=np.int64)
    mk = lambda x0, rnn, prev: GruInstance(n, x0, rnn, prev, idx if prev >= 0 else np.full(n, -1, dtype=np.int64), np.full(n, 2, dtype=np.float32))
    return GruProgram([mk(0, 0, -1), mk(12, 0, 0), mk(24, 0, 1), mk(36, 1, -1), mk(48, 1, 3), mk(24, 1, 4)]), 60


def long_panel_program():
    """Panels of more positions than the fused forward's LDS holds at d = 200 (19): the chain keeps the gi route."""
    return random_program(31, n_chain=2, K=24, E=40, lo=34, hi=40)


def large_program():
    """Enough rows (16384 or more in all) for the library's one-launch weight-gradient paths."""
    return random_program(23, n_chain=2, K=6, E=2000, lo=1500, hi=2000)


def case(d=32, type1=False, prog=lambda: random_program(33), want=False, labels=False, decay=False, offset=False, **flags):
    return dict(d=d, type1=type1, prog=prog, want=want, labels=labels, decay=decay, offset=offset, flags=flags)


# the standard program: two chains, six positions, at most 70 rows each, one empty position
CASES = {
    "chain": case(),
    "chain-d200": case(d=200),
    "want": case(want=True),
    "labels": case(labels=True),
    "type1": case(d=40, type1=True),
    "two-gate-matrices": case(GATE_GRADS_ONCE=False),
    "per-gru-weight-grads": case(WEIGHT_GRADS_MULTI=False),
    "per-position": case(CHAIN_KERNELS=False),
    "one-chain": case(prog=lambda: random_program(33, n_chain=1)),
    "zero-state": case(prog=lambda: (GC.zero_state_program(17), 17)),
    "shared-centre": case(prog=shared_centre_program),
}
DECAY_CASE = case(decay=True)
OFFSET_CASE = case(offset=True)
# what only the library has.  The fused x route of the forward takes the standard program; the one-launch weight-gradient paths (the
# keyed g4 above all) take 16384 rows or more, hence the large program (about 10 000 rows per GRU), at the flagship width
GPU_CASES = dict(CASES, **{
    "decay": DECAY_CASE,
    "offset": OFFSET_CASE,
    "long-panels-d200": case(d=200, prog=long_panel_program),
    "large-d200": case(d=200, prog=large_program),
    "large-want-d200": case(d=200, prog=large_program, want=True),
    "large-gi-route-d200": case(d=200, prog=large_program, FUSED_INPUT_GATES=False),
    "large-gi-route-labels-d200": case(d=200, prog=large_program, labels=True, FUSED_INPUT_GATES=False),
    "large-unkeyed-d200": case(d=200, prog=large_program, KEYED_GRADS=False),
    "large-two-gate-matrices-d200": case(d=200, prog=large_program, GATE_GRADS_ONCE=False),
    "large-decay-d200": case(d=200, prog=large_program, decay=True),
    "large-offset-d200": case(d=200, prog=large_program, offset=True),
})


class Launches(Recording):
    """Recording that also notes which keyword arguments a call was given (not None): the keys, the decay and the offset travel as
    keywords, and whether they were passed is part of the route.  calls: [(method name, shapes of the tensor arguments, keywords)]."""

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if not callable(fn):
            return fn

        def call(*a, **k):
            at = len(self.calls)
            try:
                return fn(*a, **k)
            finally:
                self.calls[at] += (tuple(sorted(n for n, v in k.items() if v is not None)),)
        return call


@contextlib.contextmanager
def recorded(flags):
    """The installed backend wrapped in a Launches, and gru_chain's A/B switches set to `flags`, for the block."""
    inner, old = TB.get_backend(), {k: getattr(GC, k) for k in flags}
    rec = Launches(inner)
    TB.set_backend(rec)
    for k, v in flags.items():
        setattr(GC, k, v)
    try:
        yield rec
    finally:
        TB.set_backend(inner)
        for k, v in old.items():
            setattr(GC, k, v)


def run_route(c, device):
    """One gru_chain forward + backward of case `c` under the installed backend.
    -> (launches: [(method name, shapes of its tensor arguments, keywords given)], tensors: outputs, d_x, every GRU parameter's gradient and the
    decay's / offset table's, on the CPU; None where autograd left none)."""
    prog, n_x = c["prog"]()
    d, type1 = c["d"], c["type1"]
    rnns = [m.to(device) for m in make_rnns(max(it.rnn for it in prog.inst) + 1, d, type1, 5)]
    g = torch.Generator().manual_seed(17)
    rng = np.random.default_rng(3)
    if c["labels"]:                                    # equal labels = equal x rows: one row in three distinct
        prog.x_src = rng.integers(0, n_x // 3, n_x)
        leaf = (torch.randn(int(prog.x_src.max()) + 1, d, generator=g) * 0.5).to(device).requires_grad_(True)
        x = leaf[torch.from_numpy(prog.x_src).long().to(device)]
    else:
        leaf = x = (torch.randn(n_x, d, generator=g) * 0.5).to(device).requires_grad_(True)
    want = tuple(i for i, it in enumerate(prog.inst) if it.next < 0) if c["want"] else None
    kw, extra = {}, []
    if c["decay"]:
        extra += [torch.tensor([[DECAY[0]]], device=device).requires_grad_(True), torch.tensor([DECAY[1]], device=device).requires_grad_(True)]
        kw["decay"] = tuple(extra)
    if c["offset"]:
        extra.append((torch.randn(T_ROWS, d, generator=g) * 0.5).to(device).requires_grad_(True))
        kw["offset"] = (extra[-1],) + GC.offset_tables(rng.integers(-1, T_ROWS, prog.n_total), T_ROWS, device)
    with recorded(c["flags"]) as rec:
        out = GC.gru_chain(x, prog, rnns, 0.1, type1, want, **kw)
        outs = [out] if want is None else list(out)
        loss = sum((o * torch.randn(o.shape, generator=g).to(device)).sum() * (k + 1) for k, o in enumerate(outs))
        loss.backward()
    tensors = [o.detach() for o in outs] + [leaf.grad] + [p.grad for m in rnns for p in m.parameters()] + [t.grad for t in extra]
    return [call for call in rec.calls if not call[0].endswith(QUERIES)], [None if t is None else t.cpu() for t in tensors]
