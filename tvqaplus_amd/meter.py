"""Run meter: the statistics of the caller's training / validation loop, kept on the device.

The reference's loop reads five values back per training step (main.py:69-74: ``loss.data.item()``, ``float(att_loss)``,
``float(temporal_loss)``, ``cls_loss.item()``, ``pred_ids.eq(targets.data).tolist()``) and two more per validation batch
(:173-176); each one drains the queue the step depends on.  ``RunMeter`` owns one device buffer (include/stage_hip.h "Run meter",
csrc/meter.hip) that the same numbers are accumulated into by ONE stream-ordered launch per step:

    meter = RunMeter(device)
    loss = reference_loss(outputs, targets, att_loss, t_loss, len(qids), att_w, ts_w, meter=meter)   # the loss line AND main.py:69-74
    ...
    meter.update_grad_norm(optimizer.last_grad_norm)
    if step % log_freq == 0:
        s = meter.read()            # the only synchronising call: one device-to-host copy
        print(s.train_summary(), s.nonfinite_steps)
        meter.reset()

``update`` is the stand-alone form (validation: main.py:173-176), ``update_spans`` adds the temporal metrics of
eval/eval_tvqa_plus.py:14-69 for a validation batch and returns the decoded rows a ``PredictionWriter`` would compute.  A meter
belongs to one stream.  ``host_update`` / ``host_spans`` restate the two kernels in numpy on a host-side ``MeterState``: reference
semantics; tests only; never on the product path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

N_F, N_I = 8, 24                               # include/stage_hip.h: double f[8], long long i[24], then the ring
HEAD_BYTES = (N_F + N_I) * 8
F_NAMES = ("loss_sum", "cls_sum", "att_sum", "ts_sum", "grad_norm_sum", "grad_norm_max", "iou_sum")
I_NAMES = ("steps", "rows", "correct", "nonfinite_steps", "ring_cursor", "ring_dropped", "span_rows", "span_right", "asa")
I_RECALL = 9                                   # i[9 .. 17]: IoU >= 0.1 .. 0.9
I_GNORM_STEPS = 18
THD = np.arange(0.1, 1, 0.1)                   # evaluation.compute_temporal_metrics' thresholds, bit for bit (0.30000000000000004, ...)
_F_MAX = F_NAMES.index("grad_norm_max")


class MeterState:
    """A meter on the host: ``f`` (8 float64), ``i`` (24 int64), ``ring`` (uint16 per row written: bits 0-14 the predicted index,
    bit 15 the correct flag), ``qids`` / ``span_qids`` (host lists in arrival order).  The named fields (``loss_sum``, ``rows``,
    ``correct``, ``nonfinite_steps``, ...) read ``f`` / ``i``."""

    def __init__(self, f=None, i=None, ring=None, qids=None, span_qids=None, ring_cap: int = 0):
        self.f = np.zeros(N_F, dtype=np.float64) if f is None else np.array(f, dtype=np.float64)
        self.i = np.zeros(N_I, dtype=np.int64) if i is None else np.array(i, dtype=np.int64)
        self.ring = np.zeros(0, dtype=np.uint16) if ring is None else np.array(ring, dtype=np.uint16)
        self.qids: List[int] = list(qids or [])
        self.span_qids: List[int] = list(span_qids or [])
        self.ring_cap = int(ring_cap)

    def __getattr__(self, name):
        if name in F_NAMES:
            return float(self.f[F_NAMES.index(name)])
        if name in I_NAMES:
            return int(self.i[I_NAMES.index(name)])
        if name == "grad_norm_steps":
            return int(self.i[I_GNORM_STEPS])
        raise AttributeError(name)

    @property
    def recall_bins(self) -> List[int]:
        return [int(v) for v in self.i[I_RECALL:I_RECALL + 9]]

    @property
    def predictions(self) -> np.ndarray:
        return (self.ring & 0x7FFF).astype(np.int64)

    @property
    def corrects(self) -> np.ndarray:
        return (self.ring >> 15).astype(np.int64)

    def train_summary(self) -> Dict[str, float]:
        """main.py:90-94: accuracy and the four loss sums, each divided by the number of classified rows."""
        n = float(self.rows)
        return dict(acc=self.correct / n, loss=self.loss_sum / n, loss_att=self.att_sum / n, loss_cls=self.cls_sum / n,
                    loss_ts=self.ts_sum / n)

    def valid_summary(self) -> Tuple[float, float, List[str]]:
        """main.py:180-182: (accuracy, loss / rows, the "qid\\tcorrect" strings of the rows the ring holds)."""
        n = float(self.rows)
        return self.correct / n, self.loss_sum / n, ["%d\t%d" % (a, b) for a, b in zip(self.qids, self.corrects.tolist())]

    def temporal_metrics(self) -> Dict[str, float]:
        """The keys of ``evaluation.compute_temporal_metrics`` from the span counters."""
        n = self.span_rows
        res = {}
        for k, thd in enumerate(THD):
            res["R@{:.2f}".format(thd)] = 1.0 * self.recall_bins[k] / n
        res["miou"] = 1.0 * self.iou_sum / n
        res["ans_span_joint_acc@.5"] = 1.0 * self.asa / n
        res["qa_acc"] = 1.0 * self.span_right / n
        return res

    def __add__(self, other: "MeterState") -> "MeterState":
        """Merge two meters after reading (ranks, or consecutive intervals): sums add, the maximum is the larger one, the rings and
        the qid lists are concatenated."""
        if not isinstance(other, MeterState):
            return NotImplemented
        f = self.f + other.f
        f[_F_MAX] = max(self.f[_F_MAX], other.f[_F_MAX])
        return MeterState(f, self.i + other.i, np.concatenate([self.ring, other.ring]), self.qids + other.qids,
                          self.span_qids + other.span_qids, self.ring_cap + other.ring_cap)


def _f32(v) -> np.float32:
    return np.float32(v.item() if torch.is_tensor(v) else v)


def host_update(state: MeterState, outputs=None, targets=None, loss=None, cls_loss=None, att_loss=None, ts_loss=None,
                att_weight: float = 1.0, ts_weight: float = 1.0, grad_norm=None, qids: Optional[Sequence[int]] = None) -> MeterState:
    """Reference semantics; tests only; never on the product path.  What ``stage_meter_update`` does, in numpy, on a host state
    (``state.ring_cap`` bounds its ring): same prediction rule, same fp32 products, one float64 addition per value."""
    if outputs is not None and targets is not None and len(outputs) > 0:
        x = np.asarray(outputs, dtype=np.float32)
        t = np.asarray(targets, dtype=np.int64)
        words = []
        for row, tgt in zip(x, t):
            nan = np.flatnonzero(np.isnan(row))
            pred = int(nan[0]) if nan.size else int(np.flatnonzero(row == row.max())[0])
            ok = int(tgt) == pred
            state.i[2] += int(ok)
            words.append(pred | (0x8000 if ok else 0))
        room = max(0, state.ring_cap - int(state.i[4]))
        kept = words[:room]
        state.ring = np.concatenate([state.ring, np.asarray(kept, dtype=np.uint16)])
        state.i[1] += len(words)
        state.i[4] += len(kept)
        state.i[5] += len(words) - len(kept)
        if qids is not None:
            state.qids += [int(q) for q in qids]
    given = [v is not None for v in (loss, cls_loss, att_loss, ts_loss)]
    if loss is not None:
        v = _f32(loss)
        state.f[0] = state.f[0] + np.float64(v)
        state.i[3] += 0 if np.isfinite(v) else 1
    if cls_loss is not None:
        state.f[1] = state.f[1] + np.float64(_f32(cls_loss))
    if att_loss is not None:
        state.f[2] = state.f[2] + np.float64(np.float32(att_weight) * _f32(att_loss))
    if ts_loss is not None:
        state.f[3] = state.f[3] + np.float64(np.float32(ts_weight) * _f32(ts_loss))
    if any(given):
        state.i[0] += 1
    if grad_norm is not None:
        g = np.float64(_f32(grad_norm))
        state.f[4] = state.f[4] + g
        if g > state.f[5]:
            state.f[5] = g
        state.i[I_GNORM_STEPS] += 1
    return state


def host_spans(state: MeterState, answer, t_prob, targets, gt_ts, image_indices, qids: Optional[Sequence[int]] = None) -> np.ndarray:
    """Reference semantics; tests only; never on the product path.  What ``stage_meter_spans`` does, on the host: the sweep of
    ``evaluation.find_max_pair`` on the fp32 probabilities of the predicted answer, ``PredictionWriter``'s time mapping,
    ``evaluation.temporal_iou``.  Returns the (N, 3) [st, ed, answer] rows."""
    from .evaluation import find_max_pair, temporal_iou
    answer = np.asarray(answer, dtype=np.float32)
    t_prob = np.asarray(t_prob, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.int64)
    rows = np.zeros((len(answer), 3), dtype=np.int32)
    for n in range(len(answer)):
        pred = int(np.flatnonzero(answer[n] == answer[n].max())[0])
        (st, ed), _ = find_max_pair(t_prob[n, pred, :, 0], t_prob[n, pred, :, 1])      # numpy float32 scalars: fp32 products
        rows[n] = (st, ed, pred)
        offset = (image_indices[n][0] % 6) / 3
        iou = temporal_iou([int(st) * 2 + offset, (int(ed) + 1) * 2 + offset], [float(gt_ts[n][0]), float(gt_ts[n][1])])
        right = int(targets[n]) == pred
        state.i[6] += 1
        state.i[7] += int(right)
        state.i[8] += int(right and iou >= 0.5)
        for k, thd in enumerate(THD):
            state.i[I_RECALL + k] += int(iou >= thd)
        state.f[6] = state.f[6] + np.float64(iou)
    if qids is not None:
        state.span_qids += [int(q) for q in qids]
    return rows


def _scalar_ptr(v, name: str):
    """Address of a 0-d / one-element fp32 device tensor; anything that is not a tensor (None, the Python 0 of a disabled loss) is absent."""
    if not torch.is_tensor(v):
        return None
    if not v.is_cuda:
        raise _lib.StageHipError("tvqaplus_amd.meter: %s is a %s tensor; the meter takes device tensors (there is no CPU fallback)"
                                 % (name, v.device))
    if v.dtype != torch.float32 or v.numel() != 1:
        raise TypeError("%s: expected one float32 value, got %s of %d elements" % (name, v.dtype, v.numel()))
    return v.data_ptr()


class RunMeter:
    """One meter buffer on ``device`` (a CUDA / HIP device).  ``ring_rows`` > 0 keeps (prediction, correct) of that many rows in
    arrival order for ``valid_summary``; a call that would not fit raises ``ValueError`` before it launches anything.  Every method
    but ``read`` is asynchronous on the current stream; use one stream per meter."""

    def __init__(self, device, ring_rows: int = 0):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.StageHipError("tvqaplus_amd.meter: RunMeter needs a GPU device, got %s (there is no CPU fallback)" % device)
        if ring_rows < 0:
            raise ValueError("ring_rows must be >= 0")
        from .att_host import PinnedStage
        self.device = device
        self.ring_cap = int(ring_rows)
        self._lib = _lib.load()
        self.nbytes = int(self._lib.stage_meter_bytes(self.ring_cap))
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self._stage = PinnedStage()
        self._thd = (ctypes.c_double * 9)(*[float(t) for t in THD])
        self._cursor = 0
        self.qids: List[int] = []
        self.span_qids: List[int] = []

    def _stream(self):
        from .ops import _stream
        return _stream()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self._lib.stage_meter_reset(self.buf.data_ptr(), self.ring_cap, self._stream()), "stage_meter_reset")
        self._cursor = 0
        self.qids, self.span_qids = [], []

    def claim(self, rows: int, qids: Optional[Sequence[int]] = None) -> None:
        """Host mirror of the ring cursor for a call that is about to add ``rows`` rows (``update`` and the fused loss call it)."""
        if self.ring_cap:
            if self._cursor + rows > self.ring_cap:
                raise ValueError("RunMeter: %d more rows do not fit the ring (%d of %d used); read() and reset() first, or size ring_rows "
                                 "for the pass" % (rows, self._cursor, self.ring_cap))
            self._cursor += rows
        if qids is not None:
            self.qids += [int(q) for q in qids]

    def update(self, outputs, targets, loss=None, cls_loss=None, att_loss=None, ts_loss=None, att_weight: float = 1.0,
               ts_weight: float = 1.0, qids: Optional[Sequence[int]] = None) -> None:
        """main.py:69-74 / :173-176 as one launch: outputs (P, C) fp32 logits, targets (P) int64, the losses 0-d device tensors
        (``att_loss`` / ``ts_loss`` UNWEIGHTED: the kernel multiplies by the weights in fp32 as main.py:55-56 does)."""
        from .ops import _chk
        x = _chk(outputs.detach(), "outputs")
        t = _chk(targets, "targets", torch.int64)
        if x.dim() != 2 or t.numel() != x.shape[0] or t.device != x.device or x.device != self.device:
            raise ValueError("RunMeter.update: outputs (P, C) and targets (P) on the meter's device")
        P, C = x.shape
        ptrs = [_scalar_ptr(v, n) for v, n in ((loss, "loss"), (cls_loss, "cls_loss"), (att_loss, "att_loss"), (ts_loss, "ts_loss"))]
        self.claim(P, qids)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.stage_meter_update(self.buf.data_ptr(), self.ring_cap, x.data_ptr(), t.data_ptr(), P, C, ptrs[0], ptrs[1],
                                                    ptrs[2], ptrs[3], float(att_weight), float(ts_weight), None, self._stream()),
                       "stage_meter_update")

    def update_grad_norm(self, t) -> None:
        """t: 0-d device tensor -- ``FlatAdam.last_grad_norm`` or what ``FlatGradBucket.clip_grad_norm_`` returns."""
        p = _scalar_ptr(t, "grad norm")
        if p is None:
            raise TypeError("update_grad_norm: a 0-d device tensor is required")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.stage_meter_update(self.buf.data_ptr(), self.ring_cap, None, None, 0, 0, None, None, None, None, 1.0, 1.0,
                                                    p, self._stream()), "stage_meter_update")

    def update_spans(self, answer, t_prob, targets, gt_ts, image_indices, qids: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Temporal metrics of a validation batch (inference-mode outputs ``answer`` (N, NA), ``t_scores`` (N, NA, Li, 2) softmaxed):
        ``gt_ts`` N ground-truth (start, end) in seconds, ``image_indices`` as ``PredictionWriter.add_batch`` takes them.  The (N, 3)
        double table [start, end, offset] is built on the host and sent through pinned staging, non-blocking.  Returns the (N, 3)
        int32 rows [st, ed, answer] on the device: what ``groups.answer_spans`` returns."""
        from .ops import _chk
        a, tp = _chk(answer.detach(), "answer"), _chk(t_prob.detach(), "t_prob")
        t = _chk(targets, "targets", torch.int64)
        N, NA = a.shape
        Li = tp.shape[2] if tp.dim() == 4 else -1
        if tuple(tp.shape) != (N, NA, Li, 2) or t.numel() != N or len(gt_ts) != N or len(image_indices) != N:
            raise ValueError("update_spans: answer (N, NA), t_prob (N, NA, Li, 2), N targets, N ground-truth spans, N image index lists")
        if a.device != self.device or tp.device != self.device or t.device != self.device:
            raise ValueError("update_spans: tensors on the meter's device")
        table = np.empty((N, 3), dtype=np.float64)
        table[:, :2] = np.asarray(gt_ts, dtype=np.float64).reshape(N, 2)
        table[:, 2] = [(img[0] % 6) / 3 for img in image_indices]
        gt = self._stage.upload(table, self.device)
        rows = torch.empty(N, 3, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.stage_meter_spans(self.buf.data_ptr(), a.data_ptr(), tp.data_ptr(), t.data_ptr(), gt.data_ptr(),
                                             ctypes.addressof(self._thd), N, NA, Li, rows.data_ptr(), self._stream())
        if rc == _lib.STAGE_ERR_SHAPE:
            raise ValueError("stage_meter_spans does not take N = %d, NA = %d, Li = %d (NA <= 64, Li <= 2048)" % (N, NA, Li))
        _lib.check(rc, "stage_meter_spans")
        if qids is not None:
            self.span_qids += [int(q) for q in qids]
        return rows

    def read(self) -> MeterState:
        """The only synchronising call: ONE device-to-host copy of the buffer."""
        raw = self.buf.cpu().numpy()
        f = raw[:N_F * 8].view(np.float64)
        i = raw[N_F * 8:HEAD_BYTES].view(np.int64)
        written = min(int(i[4]), self.ring_cap)
        ring = raw[HEAD_BYTES:HEAD_BYTES + 2 * written].view(np.uint16)
        return MeterState(f, i, ring, self.qids, self.span_qids, self.ring_cap)
