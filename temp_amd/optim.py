"""ClippedAdam -- the reference trainer's optimizer step as one object: clip_grad_norm_(parameters, max_norm) followed by
Adam(lr, weight_decay) (main.py:128-129 builds Trainer(gradient_clip_val=...), models/TKG_Module.py:154-160 the optimizer).

The contract (include/temp_amd.h: temp_grad_norm_clip / temp_adam_clip_step), over every parameter that HAS a gradient -- one
whose grad is None gets no state and its step count does not advance:
  1. norm = sqrt(sum g^2) over all such parameters of all groups, accumulated in fp64
  2. r = max_norm / (norm + 1e-6); coef = r if (r < 1 or r != r) else 1          (max_norm None: no norm pass, coef = 1)
  3. g' = coef g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g' g';  p -= lr / (1 - b1^t) . m / (sqrt(v) / sqrt(1 - b2^t) + eps)
     with the per-parameter scalars computed on the host in double from the parameter's own step count t.
Non-finite gradients get no special case (an inf element: coef = 0, that element NaN, a decay-only step everywhere else; a NaN
element: NaN everywhere) -- which is what torch's pair gives.

Route: when every parameter and gradient is a contiguous float32 tensor on one GPU and the backend has the kernels, a step is a
table upload and at most three launches, without a host synchronisation; otherwise (the CPU test backend, other dtypes, strided
gradients, `use_kernel = False`) the same contract in plain torch.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import backend as TB

_ROW = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("inv_bias2_sqrt", "<f4"),
                 ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"), ("eps", "<f4"), ("weight_decay", "<f4"),
                 ("first_chunk", "<i4")])
assert _ROW.itemsize == ctypes.sizeof(_lib.TempAdamTensor) == 72
_RING_MIN, _RING_MAX = 4, 64   # pinned staging buffers of the table (a few KB each)


def step_scalars(group, t):
    """(step_size, 1 / sqrt(bias correction 2), 1 - b1, b2, 1 - b2, eps, weight decay) of step t, in double."""
    b1, b2 = group["betas"]
    return (group["lr"] / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), 1.0 - b1, b2, 1.0 - b2, group["eps"], group["weight_decay"])


class _Staging:
    """Ring of pinned host buffers for the table.  The upload is a stream-ordered copy, so the buffer it reads must stay as it is
    until the copy has run: every slot carries the event recorded behind its last copy.  When the next slot's copy is still in
    flight -- the host runs several steps ahead of a device that needs longer per step -- the ring grows by a slot instead of
    waiting, up to _RING_MAX; only then does the host wait (for a copy issued _RING_MAX steps ago)."""

    def __init__(self):
        self.slots = []
        self.next = 0

    @staticmethod
    def _new(n_rows):
        buf = torch.empty(max(n_rows, 64) * _ROW.itemsize, dtype=torch.uint8, pin_memory=True)
        return [buf, buf.numpy().view(_ROW), torch.cuda.Event()]

    def take(self, n_rows):
        i = self.next
        if len(self.slots) < _RING_MIN or (len(self.slots) < _RING_MAX and not self.slots[i][2].query()):
            self.slots.insert(i, self._new(n_rows))
        else:
            self.slots[i][2].synchronize()
            if self.slots[i][1].shape[0] < n_rows:
                self.slots[i] = self._new(n_rows)
        self.next = (i + 1) % len(self.slots)
        return self.slots[i]


class ClippedAdam(torch.optim.Optimizer):
    """Adam(lr, betas, eps, weight_decay) -- torch's L2 form, the decay added to the gradient -- behind a global gradient-norm clip
    at `max_norm` (None: no clip).  State per parameter is named as torch.optim.Adam's (`step`, `exp_avg`, `exp_avg_sq`; `step` is
    a host integer), so either optimizer loads the other's state_dict.  `last_grad_norm` / `last_clip_coef`: float32 scalars of the
    last step on the parameters' device (reading them is the caller's synchronisation), None without a clip."""

    use_kernel = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_norm=None):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError("max_norm must be positive or None (no clipping), got %r" % (max_norm,))
        self.max_norm = None if max_norm is None else float(max_norm)
        self.last_grad_norm = None
        self.last_clip_coef = None
        self._staging = {}
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    # -- state ------------------------------------------------------------------------------------------------------------------
    def __setstate__(self, state):
        super().__setstate__(state)
        for k, v in (("_staging", {}), ("max_norm", None), ("last_grad_norm", None), ("last_clip_coef", None)):
            self.__dict__.setdefault(k, v)              # (an unpickled optimizer carries defaults, state and groups only)
        for st in self.state.values():
            if "step" in st and torch.is_tensor(st["step"]):               # torch.optim.Adam keeps a tensor (on the device when fused)
                st["step"] = int(round(float(st["step"].item())))

    def load_state_dict(self, state_dict):
        for group in state_dict["param_groups"]:
            for flag in ("amsgrad", "maximize", "decoupled_weight_decay"):
                if group.get(flag):
                    raise ValueError("ClippedAdam cannot continue a run with %s=True: it implements plain Adam with L2 weight decay" % flag)
        super().load_state_dict(state_dict)

    # -- the step ---------------------------------------------------------------------------------------------------------------
    def _collect(self):
        items = []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("ClippedAdam does not support sparse gradients, please consider SparseAdam instead")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                items.append((p, g, st, group))
        return items

    def _kernel_device(self, items):
        """The GPU all of the step's tensors live on when the kernels take it, else None."""
        dev = items[0][0].device
        if not self.use_kernel or dev.type != "cuda" or not hasattr(TB.get_backend(), "adam_clip_step"):
            return None
        f32 = torch.float32
        for p, g, st, _ in items:
            for t in (p, g, st["exp_avg"], st["exp_avg_sq"]):
                if t.device != dev or t.dtype != f32 or not t.is_contiguous():
                    return None
            if g.shape != p.shape or st["exp_avg"].shape != p.shape or st["exp_avg_sq"].shape != p.shape:
                return None
        return dev

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items = self._collect()
        self.last_grad_norm = self.last_clip_coef = None
        if not items:
            return loss
        dev = self._kernel_device(items)
        if dev is not None:
            self._step_kernel(items, dev)
        else:
            self._step_composite(items)
        return loss

    def _step_kernel(self, items, dev):
        be = TB.get_backend()
        C = _lib.ADAM_CHUNK
        cache = {}
        ptrs, scal = [], []
        for p, g, st, group in items:
            t = st["step"] + 1
            st["step"] = t
            n = p.numel()
            if n == 0:
                continue
            key = (t, id(group))
            s = cache.get(key)
            if s is None:
                s = cache[key] = step_scalars(group, t)
            ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), n))
            scal.append(s)
        n_rows = len(ptrs)
        if n_rows == 0:
            return
        staging = self._staging.get(dev)
        if staging is None:
            staging = self._staging[dev] = _Staging()
        with torch.cuda.device(dev):
            pinned, rows, event = staging.take(n_rows)
            r = rows[:n_rows]
            pa = np.array(ptrs, dtype=np.uint64)
            r["p"], r["g"], r["m"], r["v"] = pa[:, 0], pa[:, 1], pa[:, 2], pa[:, 3]
            counts = pa[:, 4].astype(np.int64)
            r["n"] = counts
            sa = np.array(scal, dtype=np.float64)
            for j, name in enumerate(("step_size", "inv_bias2_sqrt", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "weight_decay")):
                r[name] = sa[:, j]                                          # (one rounding, double -> float)
            chunks = (counts + (C - 1)) // C
            ends = np.cumsum(chunks)
            n_chunks = int(ends[-1])
            if n_chunks >= 2 ** 31:
                raise _lib.TempAmdError("ClippedAdam: %d chunks exceed the table's int32 chunk numbers" % n_chunks)
            r["first_chunk"] = ends - chunks
            nbytes = n_rows * _ROW.itemsize
            table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            table.copy_(pinned[:nbytes], non_blocking=True)
            event.record()
            norm_coef = None
            if self.max_norm is not None:
                norm_coef = torch.empty(2, dtype=torch.float32, device=dev)
                ws = torch.empty(be.grad_norm_workspace(n_chunks), dtype=torch.uint8, device=dev)
                be.grad_norm_clip(table, n_rows, n_chunks, self.max_norm, ws, norm_coef)
                self.last_grad_norm, self.last_clip_coef = norm_coef[0], norm_coef[1]
            be.adam_clip_step(table, n_rows, n_chunks, norm_coef)

    def _step_composite(self, items):
        coef = None
        if self.max_norm is not None:
            dev = items[0][0].device
            norms = [torch.linalg.vector_norm(g, 2, dtype=torch.float64).to(dev) for _, g, _, _ in items]
            norm = torch.linalg.vector_norm(torch.stack(norms), 2)
            r = self.max_norm / (norm + 1e-6)
            coef = torch.where((r < 1.0) | (r != r), r, torch.ones_like(r))
            self.last_grad_norm, self.last_clip_coef = norm.to(torch.float32), coef.to(torch.float32)
        for p, g, st, group in items:
            t = st["step"] + 1
            st["step"] = t
            step_size, inv_bc2, omb1, b2, omb2, eps, wd = step_scalars(group, t)
            m, v = st["exp_avg"], st["exp_avg_sq"]
            gp = g * coef.to(device=p.device, dtype=p.dtype) if coef is not None else g
            gp = gp.add(p, alpha=wd)
            m.add_(gp - m, alpha=omb1)
            v.mul_(b2).addcmul_(gp, gp, value=omb2)
            denom = v.sqrt().mul_(inv_bc2).add_(eps)
            p.addcdiv_(m, denom, value=-step_size)
