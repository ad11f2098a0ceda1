"""``FlatAdam``: ``clip_grad_norm_`` + ``torch.optim.Adam`` (main.py:63-66) on the packed gradient buffer, one library call per step.

``parallel.FlatGradBucket`` already keeps every gradient in one contiguous buffer (``bucket.flat``); this optimizer keeps Adam's two
moments in flat buffers of the same layout and runs the clip and the update as ``stage_flat_adam_step`` (csrc/flat_adam.hip): two
kernel launches, no device read-back, no float atomics.  The parameters stay where they are -- the kernels reach them through a
device-resident table of their addresses -- so everything keyed on the Parameter objects (weight-image caches, ``groups.gate``)
keeps working.

    bucket = parallel.FlatGradBucket(model.parameters())
    optimizer = FlatAdam(bucket, lr=1e-3, weight_decay=3e-7, max_grad_norm=10.0)
    ...
    loss.backward(); bucket.all_reduce(); optimizer.step()          # no separate clip_grad_norm_ call

The kernels write the parameters behind autograd's back (no version-counter bump, as a write through ``p.data``): nothing in this
package trusts the counter across steps (``ops.new_step``), and no graph is alive when an optimizer steps.

Semantics are torch's ``Adam`` (L2 weight decay, a step count per parameter, a parameter whose ``grad is None`` is not stepped) and
its ``state_dict`` format, in both directions.

Several ranks need nothing extra: ``step()`` runs after ``bucket.all_reduce()``, every rank then holds the same gradient buffer, and
the kernels add in a fixed order, so the replicas stay bit-identical.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import StageHipError

CHUNK = 1024     # csrc/flat_adam.hip: FA_CHUNK


def build_chunk_table(numels: Sequence[int], chunk: int = CHUNK) -> np.ndarray:
    """(segment, offset inside the segment, length) per chunk as an (n, 3) int32 array: every segment cut into consecutive chunks of
    at most ``chunk`` elements, in order; no chunk crosses a segment boundary (segments of 0 elements have none)."""
    if chunk < 1:
        raise ValueError("build_chunk_table: chunk must be positive")
    rows = []
    for s, n in enumerate(numels):
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise ValueError("build_chunk_table: segment %d has %d elements (0 .. 2^31 - 1 supported)" % (s, n))
        off = np.arange(0, n, chunk, dtype=np.int64)
        rows.append(np.stack([np.full_like(off, s), off, np.minimum(chunk, n - off)], axis=1))
    out = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), np.int64)
    return np.ascontiguousarray(out.astype(np.int32))


class FlatAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` over ``bucket.params`` with the gradient clip inside (``max_grad_norm``; None: the caller keeps calling
    ``bucket.clip_grad_norm_``).  One param group; ``param_groups[0]["lr"]`` (and betas / eps / weight_decay) are read at every step,
    so ``ReduceLROnPlateau`` (main.py:213) works unchanged.  ``last_grad_norm``: 0-dim device tensor, the total gradient norm the
    last step found in ``bucket.flat`` (before its clip: what ``clip_grad_norm_`` returns).  ``flag_uploads`` counts the host-to-device
    copies of the active flags (one per CHANGE of the set of parameters that carry a gradient; none in a steady-state step).
    Where it differs from torch: ``max_grad_norm`` must be positive; ``zero_grad`` only drops gradients (``set_to_none=True``); a
    step in which NO parameter has a gradient does nothing and sets ``last_grad_norm`` to 0."""

    def __init__(self, bucket, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None, amsgrad: bool = False, maximize: bool = False):
        if amsgrad or maximize:
            raise ValueError("FlatAdam: amsgrad / maximize are not supported")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FlatAdam: lr must be a Python number")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay:
            raise ValueError("FlatAdam: lr, eps and weight_decay must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FlatAdam: betas must lie in [0, 1)")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            # (torch's clip_grad_norm_(0) zeroes the gradients; the library reads max_norm <= 0 as "no clip": refuse the ambiguity)
            raise ValueError("FlatAdam: max_grad_norm must be positive (None: no clip inside the step)")
        params = list(bucket.params)
        if not params:
            raise ValueError("FlatAdam: the bucket holds no parameter")
        dev = bucket.flat.device
        for p in params:
            if not p.is_cuda:
                raise StageHipError("FlatAdam: parameters must live on the GPU (no CPU / eager fallback exists)")
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError("FlatAdam: parameters must be contiguous float32 tensors on the bucket's device")
        if bucket.flat.dtype != torch.float32:
            raise ValueError("FlatAdam: the bucket's buffer must be float32")
        # the group carries torch.optim.Adam's keys, so that state_dict() loads into one as it is: `fused` names the layout of the
        # state (float32 step counts on the parameters' device, what Adam(fused=True) keeps), the rest are Adam's defaults
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, decoupled_weight_decay=False,
                                      fused=True))
        self.bucket = bucket
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._lib = _lib.load()
        self._params: List[torch.nn.Parameter] = params
        numels = [p.numel() for p in params]
        total, S = sum(numels), len(params)
        if total != bucket.flat.numel() or total <= 0:
            raise ValueError("FlatAdam: the bucket's buffer does not match its parameters")
        self._total = total
        self._starts = np.concatenate([[0], np.cumsum(numels)[:-1]]).astype(np.int64)
        self._numels = np.asarray(numels, dtype=np.int64)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._steps = torch.zeros(S, dtype=torch.float32, device=dev)
        self._active = torch.zeros(S, dtype=torch.uint8, device=dev)
        self._active_pin = torch.zeros(S, dtype=torch.uint8).pin_memory()
        self._active_event = None
        self._active_host: Optional[List[bool]] = [False] * S
        self.flag_uploads = 0
        chunks = build_chunk_table(numels)
        self._n_chunk = int(chunks.shape[0])
        self._chunks = torch.from_numpy(chunks).to(dev)
        self._ptrs: List[int] = []
        self._segs = torch.zeros((S, 3), dtype=torch.int64, device=dev)
        self._upload_segments()
        self._ws_bytes = int(self._lib.stage_flat_adam_ws_bytes(total))
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)
        self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._betas = (ctypes.c_double * 2)(*betas)
        self._has_state = [False] * S

    # ---- tables --------------------------------------------------------------------------------------------------------------
    def _upload_segments(self) -> None:
        """Address, start and numel of every parameter (at construction, and again if a parameter's storage moved: ``model.to``,
        ``load_state_dict(assign=True)``) -- the kernels write through these addresses, so they are compared at every step."""
        self._ptrs = [p.data_ptr() for p in self._params]
        tab = np.stack([np.asarray(self._ptrs, dtype=np.int64), self._starts, self._numels], axis=1)
        self._segs.copy_(torch.from_numpy(np.ascontiguousarray(tab)))

    def _set_active(self, active: List[bool]) -> None:
        if self._active_event is not None:
            self._active_event.synchronize()       # the previous upload has read the pinned bytes (long ago)
        self._active_pin.copy_(torch.tensor(active, dtype=torch.uint8))
        self._active.copy_(self._active_pin, non_blocking=True)
        self._active_event = torch.cuda.Event()
        self._active_event.record(torch.cuda.current_stream(self._active.device))
        self._active_host = list(active)
        self.flag_uploads += 1
        for i, a in enumerate(active):
            if a and not self._has_state[i]:
                self._make_state(i)

    def _make_state(self, i: int) -> None:
        p, lo, n = self._params[i], int(self._starts[i]), int(self._numels[i])
        self.state[p] = dict(step=self._steps[i], exp_avg=self.exp_avg[lo: lo + n].view_as(p),
                             exp_avg_sq=self.exp_avg_sq[lo: lo + n].view_as(p))
        self._has_state[i] = True

    # ---- torch.optim.Optimizer -----------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True) -> None:
        if not set_to_none:
            raise ValueError("FlatAdam.zero_grad: only set_to_none=True (FlatGradBucket.zero drops the gradients)")
        self.bucket.zero()

    def add_param_group(self, param_group) -> None:
        if self.param_groups:
            raise ValueError("FlatAdam: one param group (the bucket's parameters)")
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None) -> None:
        if closure is not None:
            raise ValueError("FlatAdam.step takes no closure")
        bucket, params = self.bucket, self._params
        # the same precondition as FlatGradBucket.clip_grad_norm_: every gradient is a view of bucket.flat (pointer comparisons only)
        # (the active set is taken BEFORE packing: pack() hands every parameter a view of the buffer -- zeros for one without a
        # gradient, which bucket.all_reduce() drops again -- and torch's Adam does not step a parameter whose grad is None)
        active = [p.grad is not None for p in params]
        if not any(active):
            # nothing to step, as in torch; the buffer holds an earlier step's gradients, so the norm is that of "no gradients"
            self.last_grad_norm.zero_()
            return
        if any(p.grad is not None and p.grad.data_ptr() != v.data_ptr() for v, p in zip(bucket.views, params)):
            bucket.pack()
            for p, a in zip(params, active):
                if not a:
                    p.grad = None
        dev = self._steps.device
        with torch.cuda.device(dev):
            if active != self._active_host:
                self._set_active(active)
            if any(p.data_ptr() != a for p, a in zip(params, self._ptrs)):
                for p in params:
                    if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                        raise StageHipError("FlatAdam: a parameter left the optimizer's device / dtype / layout")
                self._upload_segments()
            group = self.param_groups[0]
            self._betas[0], self._betas[1] = group["betas"]
            rc = self._lib.stage_flat_adam_step(
                bucket.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self._segs.data_ptr(), len(params),
                self._chunks.data_ptr(), self._n_chunk, self._steps.data_ptr(), self._active.data_ptr(), self._total,
                group["lr"], ctypes.addressof(self._betas), group["eps"], group["weight_decay"],
                self.max_grad_norm if self.max_grad_norm is not None else 0.0, self._ws.data_ptr(), self._ws_bytes,
                self.last_grad_norm.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            _lib.check(rc, "stage_flat_adam_step")

    def load_state_dict(self, state_dict) -> None:
        """A ``torch.optim.Adam`` (default, foreach or fused) or ``FlatAdam`` state dict: the values are copied INTO the flat buffers,
        ``state[p]`` keeps aliasing them; the group's lr / betas / eps / weight_decay are taken over."""
        state_dict = dict(state_dict)
        for pre_hook in self._optimizer_load_state_dict_pre_hooks.values():
            hooked = pre_hook(self, state_dict)
            if hooked is not None:
                state_dict = hooked
        if "param_groups" not in state_dict or "state" not in state_dict:
            raise ValueError("FlatAdam.load_state_dict: expected the keys 'state' and 'param_groups'")
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatAdam.load_state_dict: expected one param group of %d parameters" % len(self._params))
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FlatAdam: amsgrad / maximize are not supported")
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError("FlatAdam: lr must be a Python number")
        for i, key in enumerate(g["params"]):
            st = state_dict["state"].get(key)
            if st and not all(k in st for k in ("step", "exp_avg", "exp_avg_sq")):
                raise ValueError("FlatAdam.load_state_dict: state of parameter %d lacks step / exp_avg / exp_avg_sq" % i)
            if st and not (tuple(st["exp_avg"].shape) == tuple(st["exp_avg_sq"].shape) == tuple(self._params[i].shape)):
                raise ValueError("FlatAdam.load_state_dict: state of parameter %d has another shape" % i)
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in g:
                self.param_groups[0][k] = tuple(g[k]) if k == "betas" else g[k]
        with torch.no_grad():
            # (copies first: the dictionary may be this optimizer's own state_dict(), whose tensors ARE the flat buffers)
            dev, loaded = self._steps.device, []
            for i, key in enumerate(g["params"]):
                st = state_dict["state"].get(key)
                if st:
                    step = st["step"]
                    loaded.append((i, st["exp_avg"].to(device=dev, dtype=torch.float32, copy=True),
                                   st["exp_avg_sq"].to(device=dev, dtype=torch.float32, copy=True),
                                   float(step.item()) if torch.is_tensor(step) else float(step)))
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self._steps.zero_()
            self.state.clear()
            self._has_state = [False] * len(self._params)
            for i, m, v, step in loaded:
                self._make_state(i)
                mine = self.state[self._params[i]]
                mine["exp_avg"].copy_(m)
                mine["exp_avg_sq"].copy_(v)
                mine["step"].fill_(step)
        self._active_host = None         # the next step uploads its flags and creates the state of newly active parameters
        for post_hook in self._optimizer_load_state_dict_post_hooks.values():
            post_hook(self)
