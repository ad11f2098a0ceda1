"""Host-side consumers of the attention map ``vid_raw_s``.

* ``get_att_loss``  -- supervised ranking loss over (positive region, sampled negative region) pairs of the
  ground-truth answer (model/stage.py:557-746).  Index lists are built on the host once per batch; the loss itself is
  one gather + one fused elementwise reduction on the device tensor, so autograd sends a sparse gradient into
  ``raw_s`` (the ``dS_raw_ext`` input of ``stage_str_attn_bwd``).
* ``get_att_prediction`` -- box predictions for inference (model/stage.py:748-806): per (question, answer, annotated
  image, object word) the regions whose cosine score >= 0.2, ascending by score.

Neither needs the scores on the host when they are a contiguous fp32 device tensor with at most 64 regions per row: the rows
are ranked next to the tensor (csrc/score_rows.hip, ``groups.att_predict`` / ``groups.att_hard_negatives``).  Hard-negative
sampling becomes a score-free plan (``build_hard_plan``) resolved on the device (``AttHardPairs``); box prediction uploads the
offsets of the rows it reads (``build_predict_rows``) and brings back K * (2 Lr + 1) * 4 bytes in one copy.  Every other case
keeps the host code below, unchanged.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch


def _draw(high: int, n: int) -> np.ndarray:
    """One ``torch.randint(0, high, (n,))`` on the default CPU generator: the reference's ``sample_negatives`` draws with
    exactly this call per (image, word) pair, so issuing the same calls in the same order reproduces its negatives."""
    return torch.randint(0, high, (n,)).numpy()


def _sample_negatives_np(row: Optional[np.ndarray], pr: np.ndarray, nr: np.ndarray, num_negatives: int, hard: bool,
                         pool: int, num_hard: int, drop_topk: int) -> Tuple[np.ndarray, np.ndarray]:
    """model/stage.py:557-611 for ONE (image, word) pair.  pr / nr: positive / negative region indices; ``row``: the
    predicted scores of the word's regions (hard mode only).  Returns the region indices of (P*num_negatives) pairs."""
    n_pos = pr.shape[0]
    pos_rep = pr if num_negatives == 1 else np.concatenate((pr,) * num_negatives)      # == pos.repeat(num_negatives, 1)
    if not hard:
        return pos_rep, nr[torch.randint(0, nr.shape[0], (pos_rep.shape[0],)).numpy()]
    # descending by predicted score (torch.sort(descending=True) at :577; scores are distinct floats in practice)
    order = nr[np.argsort(-row[nr], kind="stable")]
    if pool > num_negatives:
        hard_pool = order[drop_topk:drop_topk + pool]
        n_hard = num_negatives
        easy_part = None
        if num_hard < num_negatives:
            easy_pool = order[drop_topk + pool:]
            n_hard = num_hard
            easy_part = easy_pool[_draw(easy_pool.shape[0], (num_negatives - n_hard) * n_pos)]
        hard_part = hard_pool[_draw(hard_pool.shape[0], n_hard * n_pos)]
        return pos_rep, (hard_part if easy_part is None else np.concatenate([hard_part, easy_part]))
    return pos_rep, order[drop_topk:drop_topk + pos_rep.shape[0]]


def _labels_to_host(att_labels) -> List[List[np.ndarray]]:
    """att_labels: per item a list (per annotated image) of (num_words, num_regions) 0/1 tensors.  They are built on the
    host by the data set; if a caller moved them to the device they come back in ONE copy per item."""
    out = []
    for per in att_labels:
        if len(per) and torch.is_tensor(per[0]) and per[0].is_cuda:
            per = list(torch.stack(list(per)).cpu())
        out.append([(l.detach().numpy() if torch.is_tensor(l) else np.asarray(l)) for l in per])
    return out


def targets_on_device_ok(model, batch, n_local_candidates: Optional[int]) -> bool:
    """True when the pair lists can be built WITHOUT knowing the answer indices on the host: the batch carries no host copy of them
    (``target_list``: a batch straight from the reference's prepare_inputs, tvqa_dataset.py:631-688, has only the device tensor), every
    candidate is local (the answer index then only selects a slice of the score tensor, it filters nothing) and the negatives are drawn at
    random (hard negatives read the scores of the answer's rows).  ``AttPairs(..., target_dev=batch.target)`` then adds the answer's
    offset on the device -- instead of ``batch.target.tolist()``, which drains the whole queue (11-16 ms per step, DESIGN finding 18)."""
    if bool(getattr(batch, "use_hard_negatives", False)):
        return False
    return device_only_targets(model, batch, n_local_candidates)


def device_only_targets(model, batch, n_local_candidates: Optional[int]) -> bool:
    """``targets_on_device_ok`` without its condition on the sampling mode (the hard-negative plan, ``build_hard_plan``, needs no
    scores on the host either)."""
    if getattr(batch, "target_list", None) is not None:
        return False
    if int(getattr(batch, "cand_offset", 0) or 0) != 0:
        return False
    t = getattr(batch, "target", None)
    if not (torch.is_tensor(t) and t.is_cuda):
        return False
    return n_local_candidates is None or int(n_local_candidates) == int(getattr(model, "num_a", n_local_candidates))


def _labelled_rows(batch, n_local_candidates: Optional[int], placeholder_targets: bool):
    """The labelled (image, word) rows of the batch in the reference's visiting order (model/stage.py:612-660): per row its
    (b, ca_local, img, word) head and the positive / negative region indices."""
    # host copy of the answer indices when the input pipeline kept one (`.tolist()` of a device tensor waits for the whole
    # queue: measured 11-16 ms inside the step -- a full host/device serialisation per batch, which the reference also pays)
    targets = getattr(batch, "target_list", None)
    if placeholder_targets:      # ``targets_on_device_ok``: candidate column 0 everywhere, the device adds the answer's offset
        targets = [0] * len(batch.att_labels)
    elif targets is None:
        targets = batch.target.tolist()
    targets = list(targets)
    k0 = int(getattr(batch, "cand_offset", 0) or 0)      # candidate-sharded batches: only locally held ground truths contribute
    labels = _labels_to_host(batch.att_labels)
    heads, prs, nrs = [], [], []                           # per (image, word) entry: (b, ca_local, img, word), pos / neg regions
    for b, ca in enumerate(targets):
        ca -= k0
        if n_local_candidates is not None and (ca < 0 or ca >= n_local_candidates):
            continue
        start = int(batch.anno_st_idx[b])
        for local, lab in enumerate(labels[b]):
            nz = lab != 0
            rows = np.flatnonzero(nz.any(axis=1))
            if rows.size == 0:
                continue
            sub = nz[rows]                                  # (#labelled words, Lr): one nonzero each way for the image
            pw, pr_all = np.nonzero(sub)
            nw, nr_all = np.nonzero(~sub)
            pcut = np.searchsorted(pw, np.arange(rows.size + 1)).tolist()
            ncut = np.searchsorted(nw, np.arange(rows.size + 1)).tolist()
            img = start + local
            for j, w in enumerate(rows.tolist()):
                prs.append(pr_all[pcut[j]:pcut[j + 1]])
                nrs.append(nr_all[ncut[j]:ncut[j + 1]])
                heads.append((b, ca, img, w))
    return heads, prs, nrs


def build_att_pairs(model, batch, scores: Optional[torch.Tensor] = None, n_local_candidates: Optional[int] = None,
                    placeholder_targets: bool = False):
    """Host half of ``get_att_loss`` (model/stage.py:612-694): the (positive, sampled negative) index pairs of the batch as
    two (M, 5) int64 arrays of (batch, answer, image, word, region) rows, in the reference's order and with the reference's
    random draws.  Random-negative mode needs no scores (it can run ahead of the device, e.g. in the data loader);
    hard-negative mode reads the predicted scores of the labelled words -- ONE gather + ONE device-to-host copy per
    batch instead of the reference's sort + ``.cpu()`` per word."""
    hard = bool(getattr(batch, "use_hard_negatives", False))
    heads, prs, nrs = _labelled_rows(batch, n_local_candidates, placeholder_targets)
    if not heads:
        return None, None
    pred_rows = None
    if hard:
        if scores is None:
            raise ValueError("hard-negative sampling ranks the negatives by their predicted scores: pass `scores`")
        idx = torch.tensor(heads, dtype=torch.long).to(scores.device, non_blocking=True)
        pred_rows = scores.detach()[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]].cpu().numpy()    # (K, Lr): the one sync
    sps, sns = [], []
    for k in range(len(heads)):
        sp, sn = _sample_negatives_np(None if pred_rows is None else pred_rows[k], prs[k], nrs[k], model.num_negatives,
                                      hard, model.negative_pool_size, model.num_hard, model.drop_topk)
        sps.append(sp)
        sns.append(sn)
    counts = np.fromiter((a.shape[0] for a in sps), dtype=np.int64, count=len(sps))
    head_rows = np.repeat(np.asarray(heads, dtype=np.int64), counts, axis=0)
    pos = np.concatenate([head_rows, np.concatenate(sps).astype(np.int64)[:, None]], axis=1)
    neg = np.concatenate([head_rows, np.concatenate(sns).astype(np.int64)[:, None]], axis=1)
    return pos, neg


class HardPlan:
    """Everything hard-negative sampling needs EXCEPT the scores (``build_hard_plan``).  K labelled rows, M pairs:
    ``heads`` (K, 4) int64 (b, ca_local, img, word); ``negbits`` (K) uint64, bit r = region r is a labelled negative; ``slot_begin``
    (K + 1) int32: pairs [slot_begin[k], slot_begin[k + 1]) belong to row k; ``slot_q`` (M) int32: the position of each pair's
    negative in the descending score order of its row's negatives; ``pos_row`` / ``pos_region`` (M): the positive of each pair."""

    def __init__(self, heads, negbits, slot_begin, slot_q, pos_region):
        self.heads, self.negbits, self.slot_begin, self.slot_q, self.pos_region = heads, negbits, slot_begin, slot_q, pos_region
        self.pos_row = np.repeat(np.arange(heads.shape[0], dtype=np.int64), np.diff(slot_begin))
        self.k, self.m = int(heads.shape[0]), int(slot_q.shape[0])


def build_hard_plan(model, batch, n_local_candidates: Optional[int] = None, placeholder_targets: bool = False) -> Optional[HardPlan]:
    """Hard-negative mode of ``build_att_pairs`` without the scores (model/stage.py:557-611).  Which negative a pair gets depends
    on the scores only through the rank order of its row's negatives; the positions inside that order, the number of pairs and
    the reference's ``torch.randint`` calls (their bounds are lengths of slices of the order) follow from the labels alone.  So
    the draws are issued here, in the reference's order, before the scores exist, and ``AttHardPairs.resolve`` turns positions
    into regions next to the score tensor (csrc/score_rows.hip) -- no gather, no ``.cpu()``, no host sort inside the step.

    ``None`` (nothing drawn; the caller keeps ``build_att_pairs`` and its errors) when the plan cannot be exact: no labelled
    row, labels wider than 64 regions, a row with fewer negatives than ``drop_topk + num_negatives * P`` in top-k mode (the
    reference's slice comes out short there), an empty hard or easy pool (the reference raises inside ``randint``)."""
    heads, prs, nrs = _labelled_rows(batch, n_local_candidates, placeholder_targets)
    if not heads:
        return None
    nn, pool, drop = int(model.num_negatives), int(model.negative_pool_size), int(model.drop_topk)
    n_hard = min(int(model.num_hard), nn) if pool > nn else nn
    if nn < 1 or drop < 0 or n_hard < 0:
        return None
    n_pos = np.fromiter((a.shape[0] for a in prs), dtype=np.int64, count=len(prs))
    n_neg = np.fromiter((a.shape[0] for a in nrs), dtype=np.int64, count=len(nrs))
    if int((n_pos + n_neg).max()) > 64:
        return None
    if pool > nn:
        n_h = np.clip(n_neg - drop, 0, pool)              # len(order[drop:drop + pool])
        n_e = np.clip(n_neg - drop - pool, 0, None)       # len(order[drop + pool:])
        if (n_h < 1).any() or (n_hard < nn and (n_e < 1).any()):
            return None
    elif (n_neg < drop + nn * n_pos).any():
        return None
    qs, bits = [], []
    for k in range(len(heads)):
        P = int(n_pos[k])
        if pool > nn:
            easy = _draw(int(n_e[k]), (nn - n_hard) * P) + (drop + pool) if n_hard < nn else None      # the easy draw comes first
            q = _draw(int(n_h[k]), n_hard * P) + drop
            if easy is not None:
                q = np.concatenate([q, easy])
        else:
            q = np.arange(drop, drop + nn * P)
        qs.append(q)
        bits.append(int(np.bitwise_or.reduce(np.uint64(1) << nrs[k].astype(np.uint64))) if nrs[k].size else 0)
    slot_begin = np.zeros(len(heads) + 1, dtype=np.int32)
    np.cumsum(nn * n_pos, out=slot_begin[1:])
    pos_region = np.concatenate([pr if nn == 1 else np.concatenate((pr,) * nn) for pr in prs]).astype(np.int64)
    return HardPlan(np.asarray(heads, dtype=np.int64), np.asarray(bits, dtype=np.uint64), slot_begin,
                    np.concatenate(qs).astype(np.int32), pos_region)


class PinnedStage:
    """Two pinned host buffers for the per-step index upload, each guarded by the event of the copy that last read it: the host
    may only rewrite a buffer once the asynchronous host-to-device copy issued from it has run (a single unguarded buffer was a
    race whenever nothing else synchronised the step -- add_local off, or a loop with no per-step host read)."""

    def __init__(self):
        self.bufs = [None, None]
        self.events = [None, None]
        self.turn = 0

    def upload(self, t, device) -> torch.Tensor:
        """t: a host tensor or a numpy array (staged with numpy: a torch CPU copy of more than 32 K elements goes through the intra-op
        thread pool, and waking that pool inside the training step cost 50-130 ms every few steps on a 256-thread host)."""
        i = self.turn
        self.turn ^= 1
        if self.events[i] is not None:
            self.events[i].synchronize()           # the copy that read this buffer two steps ago has finished
        is_np = isinstance(t, np.ndarray)
        n = int(t.size) if is_np else t.numel()
        dt = torch.from_numpy(t[:0]).dtype if is_np else t.dtype
        if self.bufs[i] is None or self.bufs[i].numel() < n or self.bufs[i].dtype != dt:
            self.bufs[i] = torch.empty(max(2 * n, 4096), dtype=dt, pin_memory=True)
        if is_np:
            np.copyto(self.bufs[i].numpy()[:n], t.reshape(-1))
        else:
            self.bufs[i][:n].copy_(t)
        with torch.cuda.device(device):
            dev = self.bufs[i][:n].to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
        self.events[i] = ev
        return dev


class AttPairs:
    """Flat indices into a contiguous (N, NA, Li, Lqa, Lr) score tensor for the M positive rows followed by the M negative
    rows, resident on the device.  ``stage`` = a ``PinnedStage`` reused across steps (``pin_memory()`` per call registers
    a fresh page-locked allocation every time: ~0.5 ms of host time on the launch path)."""

    def __init__(self, pos: np.ndarray, neg: np.ndarray, shape, device, stage: Optional[PinnedStage] = None,
                 target_dev: Optional[torch.Tensor] = None):
        """``target_dev`` (N,) int64 on the device: the pairs were built with candidate 0 as a placeholder
        (``build_att_pairs(placeholder_targets=True)``); the answer's slice offset is added here, on the device, without a host read."""
        both = np.concatenate([pos, neg], axis=0)
        _, NA, Li, Lqa, Lr = shape
        if both.size and ((both < 0).any() or (both >= np.asarray([shape[0], NA, Li, Lqa, Lr])).any()):
            raise IndexError("attention-loss pair outside the (N, NA, Li, Lqa, Lr) score tensor")    # (the kernels gather / scatter unchecked)
        flat = (((both[:, 0] * NA + both[:, 1]) * Li + both[:, 2]) * Lqa + both[:, 3]) * Lr + both[:, 4]
        self.m = pos.shape[0]
        self.shape = tuple(shape)
        if target_dev is not None:
            flat = np.concatenate([flat, both[:, 0]])            # the example of every pair rides in the same upload
        t = torch.from_numpy(flat)
        if torch.device(device).type == "cuda":
            if stage is None:
                stage = PinnedStage()
            self.flat = stage.upload(t, device)
        else:
            self.flat = t
        if target_dev is not None:
            n2 = 2 * self.m
            tdev = target_dev.to(self.flat.device)
            ca = tdev.clamp(0, NA - 1).index_select(0, self.flat[n2:])     # (the kernels gather unchecked: the clamp is for memory safety)
            self.flat = self.flat[:n2] + ca * (Li * Lqa * Lr)
            # an answer index outside [0, NA) is an ERROR in the reference (scores[batch_idx, ca_idx] raises, model/stage.py:645) and on
            # the host path above; here nothing can raise without a read-back, so the loss is poisoned instead: get_att_loss multiplies
            # by this factor (1.0, or NaN when any target was out of range) -- the step fails loudly, not silently on the wrong candidate
            self.poison = torch.where(((tdev < 0) | (tdev >= NA)).any(), float("nan"), 1.0).to(torch.float32)
        else:
            self.poison = None
        self.stage = stage


class AttHardPairs:
    """``AttPairs`` for a ``HardPlan``: the same ``flat`` / ``m`` / ``shape`` / ``poison`` that ``get_att_loss`` consumes, with the
    negative half of ``flat`` written on the device by ``resolve(scores)`` once the scores exist.  Everything the kernel needs
    travels in ONE ``PinnedStage`` transfer; ``target_dev``: as for ``AttPairs`` (the plan was built with candidate 0, the answer's
    slice offset is added to the row offsets and the positives on the device)."""

    def __init__(self, plan: HardPlan, shape, device, stage: Optional[PinnedStage] = None,
                 target_dev: Optional[torch.Tensor] = None):
        if torch.device(device).type != "cuda":
            raise ValueError("AttHardPairs resolves its negatives on the device: scores on the host keep build_att_pairs")
        _, NA, Li, Lqa, Lr = shape
        h, K, M = plan.heads, plan.k, plan.m
        n_neg = np.asarray([bin(int(b)).count("1") for b in plan.negbits], dtype=np.int64)
        if ((h < 0).any() or (h >= np.asarray([shape[0], NA, Li, Lqa])).any() or (plan.pos_region < 0).any()
                or (plan.pos_region >= Lr).any() or (Lr < 64 and (plan.negbits >> np.uint64(Lr)).any())
                or (plan.slot_q < 0).any() or (plan.slot_q >= np.repeat(n_neg, np.diff(plan.slot_begin))).any()):
            raise IndexError("attention-loss pair outside the (N, NA, Li, Lqa, Lr) score tensor")    # (first line; the kernel checks again)
        row_off = (((h[:, 0] * NA + h[:, 1]) * Li + h[:, 2]) * Lqa + h[:, 3]) * Lr
        parts = [row_off[plan.pos_row] + plan.pos_region, row_off, plan.negbits.view(np.int64)]
        if target_dev is not None:
            parts += [h[:, 0], h[plan.pos_row, 0]]                  # the example of every row and of every pair
        words = np.concatenate([plan.slot_begin, plan.slot_q, np.zeros((K + 1 + M) & 1, dtype=np.int32)])
        parts.append(words.view(np.int64))
        if stage is None:
            stage = PinnedStage()
        dev = stage.upload(np.concatenate(parts), device)
        cut = np.cumsum([0] + [a.shape[0] for a in parts]).tolist()
        pos, self.row_off, self.negbits = dev[cut[0]:cut[1]], dev[cut[1]:cut[2]], dev[cut[2]:cut[3]]
        w32 = dev[cut[-2]:cut[-1]].view(torch.int32)
        self.slot_begin, self.slot_q = w32[:K + 1], w32[K + 1:K + 1 + M]
        self.flat = torch.empty(2 * M, dtype=torch.int64, device=dev.device)
        if target_dev is not None:
            tdev = target_dev.to(dev.device)
            step = tdev.clamp(0, NA - 1) * (Li * Lqa * Lr)          # (the kernels gather unchecked: the clamp is for memory safety)
            self.row_off = self.row_off + step.index_select(0, dev[cut[3]:cut[4]])
            torch.add(pos, step.index_select(0, dev[cut[4]:cut[5]]), out=self.flat[:M])
            self.poison = torch.where(((tdev < 0) | (tdev >= NA)).any(), float("nan"), 1.0).to(torch.float32)    # see AttPairs
        else:
            self.flat[:M].copy_(pos)
            self.poison = None
        self.m = M
        self.shape = tuple(shape)
        self.stage = stage

    def resolve(self, scores: torch.Tensor) -> "AttHardPairs":
        """One launch: the negative half of ``flat`` from the rank order of every row's negatives under ``scores``."""
        from . import groups
        groups.att_hard_negatives(scores, self.row_off, self.negbits, self.slot_begin, self.slot_q, self.flat[self.m:])
        return self


def _score_rows_ok(scores: torch.Tensor) -> bool:
    """The device route of the two row consumers: a contiguous fp32 (N, NA, Li, Lqa, Lr) tensor on the GPU with Lr <= 64."""
    if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 5 and scores.is_contiguous()):
        return False
    from . import groups
    return groups.score_rows_supported(scores.shape[-1])


def get_att_loss(model, scores: torch.Tensor, batch, pairs=None):
    """scores (N,5,Li,Lqa,Lr) raw cosine scores; batch.att_labels: per item a list (per annotated image) of
    (num_words, num_regions) 0/1 tensors; batch.anno_st_idx: index of the first annotated image.
    ``pairs``: an ``AttPairs`` prepared ahead (random-negative mode: STAGE.forward_main builds it before the first launch of
    the step, hard-negative mode an ``AttHardPairs`` whose negatives are resolved here, next to the scores) or a
    ``build_att_pairs`` result; built here otherwise."""
    if pairs is None:
        pairs = getattr(batch, "att_pairs", None)
    if pairs is None and bool(getattr(batch, "use_hard_negatives", False)) and _score_rows_ok(scores):
        on_dev = device_only_targets(model, batch, scores.shape[1])
        plan = build_hard_plan(model, batch, n_local_candidates=scores.shape[1], placeholder_targets=on_dev)
        if plan is not None:
            pairs = AttHardPairs(plan, scores.shape, scores.device, target_dev=batch.target if on_dev else None)
    if isinstance(pairs, AttHardPairs):
        pairs.resolve(scores if scores.is_contiguous() else scores.contiguous())      # the negatives under THESE scores: one launch
    elif pairs is None:
        pairs = build_att_pairs(model, batch, scores, n_local_candidates=scores.shape[1])
    if not isinstance(pairs, (AttPairs, AttHardPairs)):
        pos, neg = pairs
        if pos is None:
            return scores.sum() * 0.0, None
        pairs = AttPairs(pos, neg, scores.shape, scores.device)
    assert pairs.shape == tuple(scores.shape), (pairs.shape, tuple(scores.shape))
    grouped = getattr(model, "_grouped", None)
    if grouped is not None and grouped() and scores.is_cuda and scores.dtype == torch.float32 and pairs.m > 0:
        # gather + loss + per-pair gradient coefficients in one kernel; the backward zero-fills and scatters (csrc/groups.hip)
        from . import groups
        try:
            loss = groups.att_loss(scores.contiguous(), pairs.flat, pairs.m, model.att_loss_type, model.alpha, model.margin)
            return (loss if pairs.poison is None else loss * pairs.poison), None
        except groups.Unsupported:
            pass      # the plain gather below
    # ONE flat gather: the gradient reaches raw_s as a sparse scatter
    vals = scores.contiguous().reshape(-1).index_select(0, pairs.flat)
    s_pos, s_neg = vals[: pairs.m], vals[pairs.m:]
    if model.att_loss_type == "hinge":
        loss = torch.clamp(model.margin + s_neg - s_pos, min=0).sum()
    elif model.att_loss_type == "lse":
        loss = torch.log1p(torch.exp(model.alpha * (s_neg - s_pos))).sum()
    else:
        raise NotImplementedError("Only support hinge and lse")
    if pairs.poison is not None:
        loss = loss * pairs.poison
    return loss, None  # att_predictions are only produced outside training in the reference (:702)


def build_predict_rows(words, object_vocab, boxes, start_indices, shape) -> np.ndarray:
    """The rows of the (N, NA, Li, Lqa, Lr) attention map that ``get_att_prediction`` reads, as a (K, 4) int64 table of
    (b, a, image, word) in the reference's visiting order (example, candidate, annotated image, word; model/stage.py:760-790):
    the words of ``words`` (N, NA, Lqa) that are in the object vocabulary, once per annotated image of their example."""
    wd = words.detach().cpu().numpy() if torch.is_tensor(words) else np.asarray(words)
    N, NA = int(shape[0]), int(shape[1])
    hit = np.isin(wd, np.fromiter((int(w) for w in object_vocab), dtype=np.int64))
    out = []
    for b in range(N):
        n_img = len(boxes[b])
        if n_img == 0:
            continue
        imgs = np.arange(n_img, dtype=np.int64) + int(start_indices[b])
        for a in range(NA):
            w = np.flatnonzero(hit[b, a])
            if w.size == 0:
                continue
            blk = np.empty((n_img * w.size, 4), dtype=np.int64)
            blk[:, 0], blk[:, 1] = b, a
            blk[:, 2] = np.repeat(imgs, w.size)
            blk[:, 3] = np.tile(w, n_img)
            out.append(blk)
    return np.concatenate(out, axis=0) if out else np.zeros((0, 4), dtype=np.int64)


_predict_stage = None      # PinnedStage of the row-offset upload, reused across calls


def _fetch(dev: torch.Tensor) -> np.ndarray:
    """The ONE device-to-host copy of the device route of ``get_att_prediction``: K * (2 Lr + 1) * 4 bytes."""
    return dev.cpu().numpy()


def _predict_on_device(scores, rows: np.ndarray, wd: np.ndarray, boxes, start_indices, vid_names, qids, img_indices, thd) -> list:
    from . import groups
    global _predict_stage
    N, NA, Li, Lqa, Lr = scores.shape
    K = rows.shape[0]
    if K:
        if _predict_stage is None:
            _predict_stage = PinnedStage()
        off = (((rows[:, 0] * NA + rows[:, 1]) * Li + rows[:, 2]) * Lqa + rows[:, 3]) * Lr
        buf = torch.empty(K * (2 * Lr + 1), dtype=torch.int32, device=scores.device)
        groups.att_predict(scores, _predict_stage.upload(off, scores.device), thd, out=buf)
        host = _fetch(buf)
        cnt = host[:K]
        if (cnt < 0).any():
            raise IndexError("attention-map row outside the (N, NA, Li, Lqa, Lr) score tensor")
        # only the accepted slots become Python objects, as two flat lists cut per row: K x Lr nested lists (mostly fill) made
        # the collector walk tens of thousands of short-lived containers -- 5x the time of everything else in this function
        keep = np.arange(Lr, dtype=np.int32)[None, :] < cnt[:, None]
        val = host[K:K + K * Lr].view(np.float32).reshape(K, Lr)[keep].tolist()
        idx = host[K + K * Lr:].reshape(K, Lr)[keep].tolist()
        cut = np.concatenate([[0], np.cumsum(cnt)]).tolist()
        word = wd[rows[:, 0], rows[:, 1], rows[:, 3]].tolist()
    rows_l = rows.tolist()
    out = [{a: [] for a in range(NA)} for _ in range(N)]
    for k in range(K):
        b, a, g, _ = rows_l[k]
        s, e = cut[k], cut[k + 1]
        img_boxes = boxes[b][g - int(start_indices[b])]
        out[b][a].append({"pred": val[s:e], "bbox": [img_boxes[i] for i in idx[s:e]], "word": int(word[k]),
                          "qid": int(qids[b]), "vid_name": vid_names[b], "img_idx": img_indices[b][g]})
    return out


def get_att_prediction(scores: torch.Tensor, object_vocab, words: torch.Tensor, vid_names, qids, img_indices, boxes,
                       start_indices, score_thd: float = 0.2) -> Optional[list]:
    """model/stage.py:748-806.  A contiguous fp32 map on the GPU with Lr <= 64 is ranked there (csrc/score_rows.hip): the offsets of
    the rows that are read go up, K * (2 Lr + 1) * 4 bytes come back in one copy -- not the whole map.  Anything else (a host
    tensor, another dtype, Lr > 64, a row outside the map) takes the reference's host loop below."""
    if _score_rows_ok(scores):
        wd = words.detach().cpu().numpy()
        rows = build_predict_rows(wd, object_vocab, boxes, start_indices, scores.shape)
        if not rows.size or ((rows >= 0).all() and (rows < np.asarray(scores.shape[:4])).all()):
            from . import groups
            try:
                return _predict_on_device(scores.detach(), rows, wd, boxes, start_indices, vid_names, qids, img_indices, score_thd)
            except groups.Unsupported:
                pass
    vocab = set(int(w) for w in object_vocab)
    sc = scores.detach().cpu().numpy()
    wd = words.detach().cpu().numpy()
    out = []
    for b in range(sc.shape[0]):
        start = int(start_indices[b])
        per_q = {}
        for a in range(sc.shape[1]):
            dets = []
            for local, img_boxes in enumerate(boxes[b]):
                g = local + start
                for w_idx, w in enumerate(wd[b, a].tolist()):
                    if w not in vocab:
                        continue
                    row = sc[b, a, g, w_idx]
                    keep = np.nonzero(row >= score_thd)[0]
                    order = np.argsort(row[keep])
                    dets.append({"pred": [float(row[keep[i]]) for i in order],
                                 "bbox": [img_boxes[int(keep[i])] for i in order],
                                 "word": int(w), "qid": int(qids[b]), "vid_name": vid_names[b],
                                 "img_idx": img_indices[b][g]})
            per_q[a] = dets
        out.append(per_q)
    return out
