"""Grounding meter: the box mAP of a validation pass, kept on the device.

``RunMeter`` keeps QA accuracy, temporal mIoU and ASA of a validation pass on the device; the fourth headline number, grounding mAP,
otherwise exists only at the end of the file route: the model in ``inference_mode``, ``att_host.get_att_prediction`` (K * (2 Lr + 1)
words back per batch, every accepted slot a Python dict), ``PredictionWriter`` + ``json.dump``, ``evaluation.load_predictions`` (which
drops everything but the ground-truth answer's annotated words) and ``evaluation.detection_map``'s Python loops.  ``GroundingMeter``
owns one device buffer (include/stage_hip.h "Grounding meter", csrc/grounding.hip) that the detection records -- (class, score,
matched or not), all AP needs -- are appended to by ONE stream-ordered launch per validation batch, next to the attention map:

    g = GroundingMeter(device, gt_entries, w2i, capacity=1 << 16)
    g.reset()
    for batch in loader:                                     # model.eval()
        out, att_loss, _, ts_loss, t_prob, other = model.forward_main(batch)
        g.update(other["vid_raw_s"], batch)                  # tables up in one pinned transfer, one launch, no read-back
    m = g.read().metrics()                                   # the only synchronising call; detection_map's keys

The result equals ``detection_map(load_predictions(<PredictionWriter file>, gt, w2i)["bbox"], load_annotation(gt)["bbox"], w2i)`` for
the questions fed, where the scores of a class are distinct (the reference orders equal scores by an unstable sort).
``host_grounding`` restates the kernel in numpy on a host-side ``GroundingState``: reference semantics; tests only; never on the
product path.
"""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .evaluation import _pairwise_iou, average_precision, clean_label

N_COUNTERS = 8                                 # include/stage_hip.h: unsigned long long c[8], then the records
HEAD_BYTES = N_COUNTERS * 8
C_NAMES = ("cursor", "dropped", "tasks", "detections", "overflow", "bad")
TASK_WORDS = 8                                 # word_off, score_off, label, box_first, n_boxes, gt_first, n_gt, spare
MAX_L, MAX_WORDS, MAX_GT = 64, 8, 32           # csrc/grounding.hip: GROUND_MAX_L / _WORDS / _GT
MATCH_BIT = np.uint32(0x80000000)


class GroundingState:
    """A grounding meter on the host: ``c`` (8 int64 counters; ``cursor``, ``dropped``, ``tasks``, ``detections``, ``overflow``,
    ``bad`` read them), the records written (``words`` uint32: bits 0-30 the label, bit 31 the match; ``scores`` float32),
    ``n_positives`` {label id: ground-truth boxes of the questions seen} and ``idx2word`` for the names of ``metrics``."""

    def __init__(self, c=None, words=None, scores=None, n_positives: Optional[Mapping[int, int]] = None,
                 idx2word: Optional[Mapping[int, str]] = None, capacity: int = 0):
        self.c = np.zeros(N_COUNTERS, dtype=np.int64) if c is None else np.array(c, dtype=np.int64)
        self.words = np.zeros(0, dtype=np.uint32) if words is None else np.array(words, dtype=np.uint32)
        self.scores = np.zeros(0, dtype=np.float32) if scores is None else np.array(scores, dtype=np.float32)
        self.n_positives: Dict[int, int] = dict(n_positives or {})
        self.idx2word = idx2word if idx2word is not None else {}
        self.capacity = int(capacity)

    def __getattr__(self, name):
        if name in C_NAMES:
            return int(self.c[C_NAMES.index(name)])
        raise AttributeError(name)

    @property
    def labels(self) -> np.ndarray:
        return (self.words & ~MATCH_BIT).astype(np.int64)

    @property
    def matches(self) -> np.ndarray:
        return (self.words >> np.uint32(31)).astype(np.int64)

    def sorted_records(self) -> List[Tuple[int, int, int]]:
        """The multiset of records as a sorted list of (label, score bits, match): record order across tasks is unspecified."""
        return sorted(zip(self.labels.tolist(), self.scores.view(np.uint32).tolist(), self.matches.tolist()))

    def metrics(self) -> Dict[str, object]:
        """``evaluation.detection_map``'s result from the records: per class the shared AP tail over its (score, match) records and
        ``n_positives``; ``overall_map`` their nanmean.  Raises when records are missing (``dropped``, ``overflow``, ``bad``)."""
        wrong = [n for n in ("dropped", "overflow", "bad") if getattr(self, n) != 0]
        if wrong:
            raise ValueError("GroundingState.metrics: the records are incomplete -- " +
                             ", ".join("%s = %d" % (n, getattr(self, n)) for n in wrong))
        labels, matches = self.labels, self.matches
        per_class, aps = {}, []
        for l in sorted(k for k, v in self.n_positives.items() if v > 0):
            sel = labels == l
            entry = average_precision(self.scores[sel], matches[sel], self.n_positives[l])
            aps.append(entry["ap"])
            name = self.idx2word[l]
            entry.update(class_id=int(l), label=name)
            per_class[name] = entry
        return {"metrics_per_class": per_class, "overall_map": float(np.nanmean(aps)) if aps else float("nan")}

    def __add__(self, other: "GroundingState") -> "GroundingState":
        """Merge two meters after reading (ranks, or consecutive intervals): counters and ``n_positives`` add, records concatenate."""
        if not isinstance(other, GroundingState):
            return NotImplemented
        pos = dict(self.n_positives)
        for k, v in other.n_positives.items():
            pos[k] = pos.get(k, 0) + v
        return GroundingState(self.c + other.c, np.concatenate([self.words, other.words]), np.concatenate([self.scores, other.scores]),
                              pos, self.idx2word or other.idx2word, self.capacity + other.capacity)


class GroundingIndex:
    """The annotation (``tvqa_plus_*.json`` entries, as ``evaluation.load_annotation`` takes them) by qid: the answer index, and per
    annotated frame the ground-truth boxes grouped by label id (``w2i.get(clean_label(label), unk)``, ``<unk>`` left out), float32
    xyxy as ``load_annotation`` + ``detection_map`` form them.  ``tables`` turns a batch into the kernel's three tables."""

    def __init__(self, gt_data: Sequence[Mapping], w2i: Mapping[str, int]):
        self.unk = int(w2i["<unk>"])
        self.idx2word = {int(i): w for w, i in w2i.items()}
        self.by_qid: Dict[int, Tuple[int, Dict[int, List[Tuple[int, np.ndarray]]], Dict[int, int], bool]] = {}
        for e in gt_data:
            frames, n_pos, has_zero = {}, {}, False
            for frame, items in e["bbox"].items():
                by_label: Dict[int, list] = {}
                for b in items:
                    l = int(w2i.get(clean_label(b["label"]), self.unk))
                    if l == self.unk:
                        continue
                    has_zero = has_zero or l == 0
                    by_label.setdefault(l, []).append([b["left"], b["top"], b["left"] + b["width"], b["top"] + b["height"]])
                    n_pos[l] = n_pos.get(l, 0) + 1
                frames[int(frame)] = [(l, np.asarray(v, dtype=np.float32)) for l, v in by_label.items()]
            self.by_qid[int(e["qid"])] = (int(e["answer_idx"]), frames, n_pos, has_zero)

    def tables(self, batch, shape, n_positives: Optional[Dict[int, int]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(tasks (T, 8) int64, region_boxes (R, 4) float32, gt_boxes (G, 4) float32) of a batch whose map has ``shape``
        (N, NA, Li, Lqa, Lr); ``n_positives``, if given, receives the ground-truth box counts of the batch's questions.  A qid that
        is not annotated raises ``KeyError``, a ground-truth label with word id 0 ``ValueError`` (``detection_map`` gives class 0 to
        the dummy detection of an image without prediction; that rule is not restated)."""
        N, NA, Li, Lqa, Lr = (int(v) for v in shape)
        entries = [self.by_qid[int(q)] for q in batch.qid]              # KeyError before anything else happens
        if len(entries) != N:
            raise ValueError("GroundingIndex.tables: %d qids for a map of %d examples" % (len(entries), N))
        for q, e in zip(batch.qid, entries):
            if e[3]:
                raise ValueError("question %s has a ground-truth label whose word id is 0 (the class of detection_map's dummy "
                                 "detection)" % q)
        vocab = set(int(w) for w in batch.eval_object_word_ids)
        tasks, rboxes, gboxes = [], [], []
        n_r = n_g = 0
        for b, (answer, frames, n_pos, _) in enumerate(entries):
            if n_positives is not None:
                for l, n in n_pos.items():
                    n_positives[l] = n_positives.get(l, 0) + n
            if not 0 <= answer < NA:
                raise ValueError("question %s: answer_idx %d outside the map's %d candidates" % (batch.qid[b], answer, NA))
            start = int(batch.anno_st_idx[b])
            word_off = (b * NA + answer) * Lqa
            for local, img_boxes in enumerate(batch.boxes[b]):
                g = start + local
                labelled = [(l, gt) for l, gt in frames.get(int(batch.image_indices[b][g]), ()) if l in vocab]
                if not labelled:
                    continue
                if not 0 <= g < Li:
                    raise IndexError("annotated image %d of question %s lies outside the map's %d frames" % (g, batch.qid[b], Li))
                rb = np.asarray(img_boxes, dtype=np.float32).reshape(-1, 4)
                score_off = ((b * NA + answer) * Li + g) * Lqa * Lr
                for l, gt in labelled:
                    tasks.append((word_off, score_off, l, n_r, rb.shape[0], n_g, gt.shape[0], 0))
                    gboxes.append(gt)
                    n_g += gt.shape[0]
                rboxes.append(rb)
                n_r += rb.shape[0]
        cat = lambda parts: np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=np.float32)
        return np.asarray(tasks, dtype=np.int64).reshape(-1, TASK_WORDS), cat(rboxes), cat(gboxes)


def host_grounding_tables(state: GroundingState, scores, words, tasks, region_boxes, gt_boxes, Lqa: int, Lr: int,
                          score_thd: float = 0.2, iou_thd: float = 0.5) -> GroundingState:
    """Reference semantics; tests only; never on the product path.  What ``stage_grounding_update`` does with its three tables, in
    numpy, on a host state (``state.capacity`` bounds its records): the same bounds in the same order, ``_pairwise_iou`` itself, a
    stable sort for the rank order."""
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    wd = np.asarray(words, dtype=np.int64).reshape(-1)
    rbox = np.asarray(region_boxes, dtype=np.float32).reshape(-1, 4)
    gbox = np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4)
    thd, iou_thd = np.float32(score_thd), np.float32(iou_thd)

    def inside(first, n, size):
        return first >= 0 and n >= 0 and first <= size and n <= size - first

    for word_off, score_off, label, box_first, n_boxes, gt_first, n_gt, _ in np.asarray(tasks, dtype=np.int64).reshape(-1, 8).tolist():
        state.c[2] += 1
        if not (0 <= label <= 0x7FFFFFFF and inside(word_off, Lqa, wd.size) and inside(score_off, Lr, sc.size)
                and inside(box_first, n_boxes, rbox.shape[0]) and n_gt >= 1 and inside(gt_first, n_gt, gbox.shape[0])):
            state.c[5] += 1
            continue
        pos = np.flatnonzero(wd[word_off:word_off + Lqa] == label)
        if pos.size > MAX_WORDS or n_gt > MAX_GT:
            state.c[4] += 1
            continue
        det_s, det_r, ok = [], [], True
        for w in pos.tolist():
            off = score_off + w * Lr
            if not inside(off, Lr, sc.size):
                ok = False
                break
            row = sc[off:off + Lr]
            keep = np.flatnonzero(row >= thd)                     # fp32 compare; a NaN is never kept
            if keep.size and int(keep.max()) >= n_boxes:
                ok = False
                break
            det_s += row[keep].tolist()
            det_r += keep.tolist()
        if not ok:
            state.c[5] += 1
            continue
        if not det_s:
            continue
        s = np.asarray(det_s, dtype=np.float32)
        order = np.argsort(-s, kind="stable")                     # descending; equal scores: lower (position, region) first
        pb = rbox[box_first + np.asarray(det_r, dtype=np.int64)][order].copy()
        gb = gbox[gt_first:gt_first + n_gt].copy()
        pb[:, 2:] += 1
        gb[:, 2:] += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = _pairwise_iou(pb, gb)
        who = iou.argmax(axis=1)
        who[iou.max(axis=1) < iou_thd] = -1
        taken = np.zeros(n_gt, dtype=bool)
        match = []
        for j in who:
            match.append(int(j >= 0 and not taken[j]))
            if j >= 0:
                taken[j] = True
        room = min(max(0, state.capacity - int(state.c[0])), len(match))
        rec = np.uint32(label) | (np.asarray(match, dtype=np.uint32) << np.uint32(31))
        state.words = np.concatenate([state.words, rec[:room]])
        state.scores = np.concatenate([state.scores, s[order][:room]])
        state.c[0] += len(match)
        state.c[1] += len(match) - room
        state.c[3] += len(match)
    return state


def host_grounding(state: GroundingState, scores, batch, index: GroundingIndex, score_thd: float = 0.2,
                   iou_thd: float = 0.5) -> GroundingState:
    """Reference semantics; tests only; never on the product path.  ``GroundingMeter.update`` on a host ``GroundingState``: the
    tables of ``index`` for the batch, then ``host_grounding_tables`` on host copies of the map and the word ids."""
    sc = scores.detach().cpu().numpy() if torch.is_tensor(scores) else np.asarray(scores, dtype=np.float32)
    qas = batch.qas.detach().cpu().numpy() if torch.is_tensor(batch.qas) else np.asarray(batch.qas)
    tasks, rbox, gbox = index.tables(batch, sc.shape, state.n_positives)
    if not state.idx2word:
        state.idx2word = index.idx2word
    return host_grounding_tables(state, sc, qas, tasks, rbox, gbox, sc.shape[3], sc.shape[4], score_thd, iou_thd)


class GroundingMeter:
    """One record buffer of ``capacity`` detections on ``device`` (a CUDA / HIP device) for the questions of ``gt_data`` (the
    annotation entries, as ``evaluation.load_annotation`` takes them).  ``update`` and ``reset`` are asynchronous on the current
    stream; ``read`` is the only synchronising call.  Use one stream per meter."""

    def __init__(self, device, gt_data: Sequence[Mapping], w2i: Mapping[str, int], capacity: int, score_thd: float = 0.2,
                 iou_thd: float = 0.5):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.StageHipError("tvqaplus_amd.grounding: GroundingMeter needs a GPU device, got %s (there is no CPU fallback)"
                                     % device)
        if capacity < 0:
            raise ValueError("capacity must be >= 0")
        from .att_host import PinnedStage
        self.device = device
        self.capacity = int(capacity)
        self.score_thd, self.iou_thd = float(score_thd), float(iou_thd)
        self.index = GroundingIndex(gt_data, w2i)
        self._lib = _lib.load()
        self.nbytes = int(self._lib.stage_grounding_bytes(self.capacity))
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self._stage = PinnedStage()
        self.n_positives: Dict[int, int] = {}

    def _stream(self):
        from .ops import _stream
        return _stream()

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(self._lib.stage_grounding_reset(self.buf.data_ptr(), self.capacity, self._stream()), "stage_grounding_reset")
        self.n_positives = {}

    def _check(self, scores, words):
        from .ops import _chk
        s = _chk(scores.detach(), "scores")
        w = _chk(words, "words", torch.int64)
        if s.dim() != 5 or s.device != self.device or w.device != self.device:
            raise ValueError("GroundingMeter: scores (N, NA, Li, Lqa, Lr) fp32 and the word ids int64, both on the meter's device")
        Lqa, Lr = int(s.shape[3]), int(s.shape[4])
        if not self._lib.stage_grounding_supported(Lqa, Lr):
            raise ValueError("the grounding meter does not take Lqa = %d, Lr = %d (1 <= Lqa <= %d, 1 <= Lr <= %d)" % (Lqa, Lr, MAX_L, MAX_L))
        return s, w, Lqa, Lr

    def update_tables(self, scores, words, tasks: np.ndarray, region_boxes: np.ndarray, gt_boxes: np.ndarray) -> None:
        """The launch of ``update`` on explicit tables (include/stage_hip.h "Grounding meter"): ONE pinned upload of the three
        tables, ONE library call on the current stream."""
        s, w, Lqa, Lr = self._check(scores, words)
        tasks = np.ascontiguousarray(tasks, dtype=np.int64).reshape(-1, TASK_WORDS)
        rb = np.ascontiguousarray(region_boxes, dtype=np.float32).reshape(-1, 4)
        gb = np.ascontiguousarray(gt_boxes, dtype=np.float32).reshape(-1, 4)
        if not (np.isfinite(rb).all() and np.isfinite(gb).all()):
            raise ValueError("GroundingMeter: a box coordinate is not finite")
        T = tasks.shape[0]
        if T == 0:
            return
        n_t, n_r = T * TASK_WORDS, 2 * rb.shape[0]              # sizes in 8-byte words: a box is two of them
        packed = np.empty(n_t + n_r + 2 * gb.shape[0], dtype=np.int64)
        packed[:n_t] = tasks.reshape(-1)
        packed[n_t:n_t + n_r].view(np.float32)[:] = rb.reshape(-1)
        packed[n_t + n_r:].view(np.float32)[:] = gb.reshape(-1)
        dev = self._stage.upload(packed, self.device)
        base = dev.data_ptr()
        with torch.cuda.device(self.device):
            rc = self._lib.stage_grounding_update(self.buf.data_ptr(), self.capacity, s.data_ptr(), s.numel(), w.data_ptr(), w.numel(),
                                                  base, T, base + 8 * n_t, rb.shape[0], base + 8 * (n_t + n_r), gb.shape[0], Lqa, Lr,
                                                  self.score_thd, self.iou_thd, self._stream())
        _lib.check(rc, "stage_grounding_update")

    def update(self, scores, batch) -> None:
        """One validation batch: ``scores`` = ``vid_raw_s`` (N, NA, Li, Lqa, Lr), contiguous fp32 on the meter's device (in ``eval()``
        mode ``model.forward_main(batch)[-1]["vid_raw_s"]``).  Reads ``batch.qid``, ``qas`` (device int64; compared on the device),
        ``image_indices``, ``anno_st_idx``, ``boxes`` and ``eval_object_word_ids``; nothing of ``batch.target``.  No device-to-host
        copy; a qid that is not annotated raises ``KeyError`` before anything is launched."""
        s, w, _, _ = self._check(scores, batch.qas)
        if tuple(w.shape) != tuple(s.shape[:2]) + (s.shape[3],):
            raise ValueError("GroundingMeter.update: batch.qas %s does not belong to a map of shape %s" % (tuple(w.shape), tuple(s.shape)))
        pos: Dict[int, int] = {}
        tasks, rb, gb = self.index.tables(batch, s.shape, pos)
        self.update_tables(s, w, tasks, rb, gb)
        for l, n in pos.items():
            self.n_positives[l] = self.n_positives.get(l, 0) + n

    def read(self) -> GroundingState:
        """The only synchronising call: ONE device-to-host copy of the buffer."""
        raw = self.buf.cpu().numpy()
        c = raw[:HEAD_BYTES].view(np.int64)
        written = min(int(c[0]), self.capacity)
        rec = raw[HEAD_BYTES:HEAD_BYTES + 8 * written].view(np.uint32).reshape(-1, 2)
        return GroundingState(c, rec[:, 0], rec[:, 1].copy().view(np.float32), self.n_positives, self.index.idx2word, self.capacity)
