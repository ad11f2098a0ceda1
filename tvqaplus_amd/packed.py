"""Packed context features: one context stream (``sub_bert`` or ``vid``) as the rows that exist.

The reference's collate (tvqa_dataset.py:515-553 ``pad_collate``) zero-fills a padded ``(N, Li, L, K)`` tensor, copies the rows of every
frame into it in a Python loop and builds pure prefix masks from the lengths: everything behind a frame's length is zero by
construction, so the padded tensor says nothing that ``(rows, lengths)`` does not -- and at the full configuration more than half of
what goes over the host link is that padding (docs/measurement.md).  ``PackedFeatures`` is the stream without it:

* ``data`` ``(P + 1, K)`` fp32 / fp16 / bf16, contiguous: frame-major, frame ``f = n * Li + i`` owns rows ``start[f] .. start[f] + len[f] - 1``
  (``start`` = exclusive prefix sum of ``len``); **row P is all zeros**, the source of every padded position;
* ``lens`` ``(N, Li)`` int32 numpy, on the host (the loader knows it), ``0 <= len <= L``; ``L`` = the padded row length the model sees.

A batch carries it IN PLACE of the feature tensor (the masks of that stream may then be absent: STAGE builds them on the device).  The
ragged context layout points its source-row table into ``data`` (tvqaplus_amd/ragged.py: CtxLayout, csrc/packed.hip:
stage_pack_ctx_rows) and the existing kernels read the same numbers from less than half the bytes; every other path builds the padded
image on the device (stage_pack_unpack).  ``unpad_host`` is the specification of both, for the tests -- never on the product path.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


class PackedFeatures:
    def __init__(self, data: torch.Tensor, lens, L: int):
        L = int(L)
        lens = self._check_lens(lens, L)
        P = int(lens.sum(dtype=np.int64))
        if not torch.is_tensor(data) or data.dim() != 2 or data.shape[0] != P + 1 or data.dtype not in _DTYPES or not data.is_contiguous():
            raise ValueError("data must be a contiguous (P + 1 = %d, K) fp32 / fp16 / bf16 tensor" % (P + 1))
        self.data, self.lens, self.L, self.P = data, lens, L, P
        self.N, self.Li = (int(v) for v in lens.shape)
        self.K = int(data.shape[1])

    @staticmethod
    def _check_lens(lens, L: int) -> np.ndarray:
        lens = np.ascontiguousarray(lens)
        if lens.ndim != 2 or not np.issubdtype(lens.dtype, np.integer):
            raise ValueError("lens must be an (N, Li) integer array, got %r %s" % (lens.shape, lens.dtype))
        if L < 1 or (lens.size and (int(lens.min()) < 0 or int(lens.max()) > L)):
            raise ValueError("every len must be in [0, L = %d]" % L)
        return lens.astype(np.int32)

    # ---- what stage.py reads from a feature tensor ------------------------------------------------------------------------------
    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.N, self.Li, self.L, self.K))

    @property
    def dtype(self) -> torch.dtype:
        return self.data.dtype

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def is_cuda(self) -> bool:
        return self.data.is_cuda

    @property
    def nbytes(self) -> int:
        return (self.P + 1) * self.K * self.data.element_size()

    def is_contiguous(self) -> bool:
        return True

    def dim(self) -> int:
        return 4

    def to(self, *args, **kw) -> "PackedFeatures":
        """``.to(device, non_blocking=...)`` / ``.to(dtype)``: ``lens`` stays on the host; rounding keeps row P zero (0 rounds to 0)."""
        data = self.data.to(*args, **kw)
        if data.dtype not in _DTYPES:
            raise ValueError("packed features are fp32, fp16 or bf16")
        return self if data is self.data else PackedFeatures(data.contiguous(), self.lens, self.L)

    def float(self) -> "PackedFeatures":
        return self.to(torch.float32)

    def half(self) -> "PackedFeatures":
        return self.to(torch.float16)

    def record_stream(self, stream) -> None:
        if self.data.is_cuda:
            self.data.record_stream(stream)

    # ---- tables -----------------------------------------------------------------------------------------------------------------
    def starts(self) -> np.ndarray:
        """(N * Li,) int64: first packed row of every frame."""
        lv = self.lens.reshape(-1).astype(np.int64)
        return np.concatenate([[0], np.cumsum(lv)[:-1]]).astype(np.int64) if lv.size else np.zeros(0, np.int64)

    def ptab(self) -> np.ndarray:
        """(frames, 2) int32 (first packed row, len): what the kernels of csrc/packed.hip take."""
        return np.stack([self.starts(), self.lens.reshape(-1).astype(np.int64)], axis=1).astype(np.int32)

    def _valid(self) -> torch.Tensor:
        return torch.arange(self.L).view(1, 1, self.L) < torch.from_numpy(self.lens.astype(np.int64)).unsqueeze(-1)

    # ---- construction -----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_padded(cls, x: torch.Tensor, lens, check: bool = False) -> "PackedFeatures":
        """Rows ``[0, len)`` of every frame of the padded ``(N, Li, L, K)`` tensor, verbatim (holes inside a prefix stay).
        ``check``: assert that everything behind ``len`` is zero."""
        N, Li, L, K = x.shape
        lens = cls._check_lens(lens, int(L))
        self = cls(torch.zeros(int(lens.sum(dtype=np.int64)) + 1, K, dtype=x.dtype, device=x.device), lens, L)
        if self.lens.shape != (N, Li):
            raise ValueError("lens %r does not match the tensor's (N, Li) = %r" % (self.lens.shape, (N, Li)))
        valid = self._valid().to(x.device)
        if check:
            assert not bool((x[~valid] != 0).any()), "from_padded: a non-zero value behind a frame's length"
        if self.P:
            self.data[:self.P] = x[valid]
        return self

    @classmethod
    def from_sequences(cls, seqs: Sequence[Sequence[torch.Tensor]], L: int, Li: Optional[int] = None,
                       out: Optional[torch.Tensor] = None) -> "PackedFeatures":
        """The collate: ``seqs[n][i]`` is the ``(len, K)`` tensor of frame i of example n (examples may have fewer than ``Li`` frames:
        the missing ones have length 0).  The rows are concatenated straight into ``out`` (a pinned ``(>= P + 1, K)`` buffer, when
        given); the padded tensor is never built."""
        N = len(seqs)
        Li = max([len(s) for s in seqs] + [1]) if Li is None else int(Li)
        lens = np.zeros((N, Li), dtype=np.int64)
        flat = []
        for n, s in enumerate(seqs):
            if len(s) > Li:
                raise ValueError("example %d has %d frames, Li = %d" % (n, len(s), Li))
            for i, t in enumerate(s):
                lens[n, i] = t.shape[0]
                flat.append(t)
        if not flat:
            raise ValueError("from_sequences needs at least one frame (the feature width comes from it)")
        if int(lens.max()) > int(L):
            raise ValueError("every len must be in [0, L = %d]" % int(L))
        K, dt, P = int(flat[0].shape[1]), flat[0].dtype, int(lens.sum())
        if out is None:
            data = torch.empty(P + 1, K, dtype=dt)
        else:
            if out.dim() != 2 or out.shape[0] < P + 1 or out.shape[1] != K or out.dtype != dt or not out.is_contiguous():
                raise ValueError("out must be a contiguous (>= %d, %d) %s buffer" % (P + 1, K, dt))
            data = out[:P + 1]
        rows = [t for t in flat if t.shape[0]]
        if rows:
            torch.cat(rows, dim=0, out=data[:P])
        data[P].zero_()
        return cls(data, lens, L)

    # ---- the specification (tests) ----------------------------------------------------------------------------------------------
    def unpad_host(self):
        """-> (padded ``(N, Li, L, K)`` tensor, ``(N, Li, L)`` fp32 prefix mask) on the CPU: what stage_pack_unpack writes."""
        valid = self._valid()
        dense = torch.zeros(self.N, self.Li, self.L, self.K, dtype=self.dtype)
        if self.P:
            dense[valid] = self.data[:self.P].cpu()
        return dense, valid.float()

    def slice_examples(self, lo: int, hi: int) -> "PackedFeatures":
        """The examples ``[lo, hi)`` as a packed stream of their own: only their rows are copied, plus the zero row."""
        lo, hi, _ = slice(lo, hi).indices(self.N)
        hi = max(lo, hi)
        st = np.concatenate([self.starts(), [self.P]])
        r0, r1 = int(st[lo * self.Li]), int(st[hi * self.Li])
        data = torch.cat([self.data[r0:r1], self.data[self.P:self.P + 1]], dim=0)
        return PackedFeatures(data, self.lens[lo:hi], self.L)

    def __repr__(self) -> str:
        return "PackedFeatures(shape=%r, rows=%d, dtype=%s, device=%s)" % (tuple(self.shape), self.P, self.dtype, self.device)


def pack_batch(batch, check: bool = False):
    """The batch with ``sub_bert`` / ``vid`` packed (lengths: ``batch.mask_host``'s, or the last non-zero mask position + 1) and the masks
    of the packed streams dropped -- for batches that were collated padded (tvqaplus_amd.synth.make_batch(packed=True), tools)."""
    from .ragged import mask_lens
    out = type(batch)(batch)
    mh = dict(batch.get("mask_host") or {})
    for feat, mask, key in (("sub_bert", "sub_mask", "sub_len"), ("vid", "vid_mask", "vid_len")):
        x = batch.get(feat)
        if not torch.is_tensor(x):
            continue
        lens = mh.get(key)
        if lens is None:
            lens = mask_lens(batch[mask].cpu().numpy())
        out[feat] = PackedFeatures.from_padded(x, lens, check=check)
        mh[key] = out[feat].lens
        out.pop(mask, None)
    out["mask_host"] = mh
    return out
