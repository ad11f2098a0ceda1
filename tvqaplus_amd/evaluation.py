"""Inference decoding, the prediction file and the TVQA+ metrics, Python 3.

The reference splits this over ``inference.py`` (span decoding ``find_max_pair`` :13-35, the prediction dictionary
:42-72, written with ``save_json`` :98) and ``eval/eval_tvqa_plus.py`` + ``eval/maskrcnn_voc`` (Python 2 only:
``dict.keys()[0]``, implicit relative imports, ``np.nanmean(dict.values())``).  Here:

* ``find_max_pair_batch``   -- the span decoder for a whole batch ON THE DEVICE (no ``.cpu()`` per question); the
                               host version ``find_max_pair`` is kept as the specification it is tested against
* ``find_max_triples_batch`` -- the n best spans of a row (model/model_utils.py:92-123 for a batch), on the device in O(L) memory
* ``PredictionWriter``      -- accumulates ``{"ts_answer": {qid: [[st, ed], answer]}, "raw_bbox": [...]}`` from the
                               model's ``inference_mode`` outputs with the reference's time mapping, and saves it
* ``compute_temporal_metrics``, ``detection_map`` (PASCAL-VOC AP as maskrcnn-benchmark's voc evaluation, numpy),
  ``load_annotation``, ``load_predictions``, ``evaluate_files`` / ``python -m tvqaplus_amd.evaluation`` -- QA Acc.,
  Grd. mAP, Temp. mIoU, ASA (eval/eval_sample.sh:5-9 lists the values of the reference's sample prediction file, which is
  not part of the public tree; tests/golden/eval_*.npz pin these functions against the reference's own code instead).
"""
from __future__ import annotations

import json
from collections import defaultdict
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

NUM_ANSWERS = 5
IMAGE_SIZE = (640, 360)       # eval/eval_tvqa_plus.py:118 (unused by the arithmetic: boxes are absolute pixels)


# ---------------------------------------------------------------------------------------------------------------
# span decoding (inference.py:13-35)
# ---------------------------------------------------------------------------------------------------------------
def find_max_pair(p1: Sequence[float], p2: Sequence[float]) -> Tuple[Tuple[int, int], float]:
    """(k1, k2), k1 <= k2, maximising p1[k1] * p2[k2]: one left-to-right sweep that carries the first arg-max of p1 so
    far; a later end position only wins with a strictly larger product; (0, 1) with value 0 when nothing is positive."""
    best, best_val, lead = (0, 1), 0.0, 0
    for i in range(len(p1)):
        if p1[lead] < p1[i]:
            lead = i
        prod = p1[lead] * p2[i]
        if prod > best_val:
            best, best_val = (lead, i), prod
    return best, float(best_val)


def find_max_pair_batch(p_st: torch.Tensor, p_ed: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The same decoder for R rows at once, wherever the tensors live.  p_st, p_ed: (R, L) -> (st (R,), ed (R,), value (R,)).
    Tie rules of the sweep: the start carried to position i is the FIRST arg-max of p_st[:i+1]; the end is the FIRST
    position reaching the best product; rows whose best product is not positive return (0, 1, 0)."""
    R, L = p_st.shape
    run_max, _ = torch.cummax(p_st, dim=1)
    pos = torch.arange(L, device=p_st.device).expand(R, L)
    # position i starts a new strict maximum <=> p_st[i] > max(p_st[:i]); its index is carried forward
    prev = torch.cat([torch.full((R, 1), float("-inf"), device=p_st.device, dtype=p_st.dtype), run_max[:, :-1]], dim=1)
    lead = torch.cummax(torch.where(p_st > prev, pos, torch.zeros_like(pos)), dim=1)[0]
    prod = run_max * p_ed
    val, ed = prod.max(dim=1)                      # first maximal position (torch.max documents first-occurrence)
    ed = torch.argmax((prod == val.unsqueeze(1)).to(torch.int8), dim=1)   # explicit: the FIRST position equal to the maximum
    st = lead.gather(1, ed.unsqueeze(1)).squeeze(1)
    none = val <= 0
    st = torch.where(none, torch.zeros_like(st), st)
    ed = torch.where(none, torch.ones_like(ed), ed)
    val = torch.where(none, torch.zeros_like(val), val)
    return st, ed, val


def _find_max_triples_host(p_st: torch.Tensor, p_ed: torch.Tensor, top_n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The specification of the top-K span search, as plain torch: every pair (st <= ed) valued p_st[st] * p_ed[ed] (one
    multiplication in the tensors' type), sorted by value descending with equal values in ascending st * L + ed (a stable sort of the
    row-major product), the first top_n taken; ranks past the L (L + 1) / 2 pairs are (-1, -1) with value 0."""
    R, L = p_st.shape
    span = torch.full((R, top_n, 2), -1, dtype=torch.int64, device=p_st.device)
    conf = torch.zeros((R, top_n), dtype=p_st.dtype, device=p_st.device)
    upper = torch.ones(L, L, dtype=torch.bool, device=p_st.device).triu().view(-1)
    n = min(top_n, L * (L + 1) // 2)
    for r in range(R):                                   # one (L, L) product at a time
        prod = (p_st[r].unsqueeze(1) * p_ed[r].unsqueeze(0)).reshape(-1)
        val, flat = torch.sort(prod[upper], descending=True, stable=True)
        flat = torch.nonzero(upper).view(-1)[flat[:n]]
        span[r, :n, 0], span[r, :n, 1] = flat // L, flat % L
        conf[r, :n] = val[:n]
    return span, conf


def find_max_triples_batch(p_st: torch.Tensor, p_ed: torch.Tensor, top_n: int, prob_thd: Optional[float] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """model/model_utils.py:92-123 (find_max_triples) for R rows, wherever the tensors live: the top_n pairs (st <= ed) with the
    largest p_st[st] * p_ed[ed].  p_st, p_ed: (R, L) probabilities -> (span (R, top_n, 2) int64 [st, ed], conf (R, top_n)).
    Order: value descending, equal values by ascending st * L + ed (``STAGE._best_span``'s rule; the reference's argsort leaves
    ties to numpy's unstable sort).  Ranks without a pair -- where the reference lists a zero of the lower triangle -- and, with
    ``prob_thd``, ranks whose value is below it (a suffix of the list) are (-1, -1) with value 0.
    fp32 rows on the GPU go through one kernel (``groups.topk_spans``, O(L) memory per row); anything else, and shapes the kernel
    declines (L > 2048, top_n > 8), through ``_find_max_triples_host``, which is also the kernel's specification."""
    if p_st.dim() != 2 or p_st.shape != p_ed.shape or top_n < 1:
        raise ValueError("find_max_triples_batch: p_st, p_ed must be (R, L) and top_n >= 1")
    span = conf = None
    if p_st.is_cuda and p_ed.is_cuda and p_st.dtype == torch.float32 and p_ed.dtype == torch.float32 and p_st.shape[0] >= 1:
        from . import groups
        if groups.topk_spans_supported(p_st.shape[1], top_n):
            span, conf = groups.topk_spans(torch.stack([p_st.detach(), p_ed.detach()], dim=2), top_n, is_prob=True)
            span = span.long()
    if span is None:
        span, conf = _find_max_triples_host(p_st.detach(), p_ed.detach(), top_n)
    if prob_thd is not None:
        drop = (conf < prob_thd) | (span[:, :, 0] < 0)
        span = torch.where(drop.unsqueeze(2), torch.full_like(span, -1), span)
        conf = torch.where(drop, torch.zeros_like(conf), conf)
    return span, conf


def _device_rows(answer: torch.Tensor, t_scores: torch.Tensor) -> Optional[torch.Tensor]:
    """(N, 3) [st, ed, answer] from ONE kernel (``groups.answer_spans``: the decoder above, same tie rules) when both tensors are
    fp32 on the GPU and the kernel takes the shape; None otherwise (the torch composition of ``find_max_pair_batch`` then runs)."""
    if not (answer.is_cuda and t_scores.is_cuda and answer.dtype == torch.float32 and t_scores.dtype == torch.float32
            and answer.dim() == 2 and t_scores.dim() == 4 and 1 <= t_scores.shape[2] <= 2048 and answer.shape[0] >= 1):
        return None
    from . import groups
    try:
        return groups.answer_spans(answer, t_scores)
    except groups.Unsupported:
        return None


class PredictionWriter:
    """inference.py:42-72: per batch, the predicted answer, the (st, ed) span of the PREDICTED answer decoded from the
    softmaxed temporal scores and mapped to seconds (frames are sampled at 0.5 fps: ``st * 2 + offset``,
    ``(ed + 1) * 2 + offset`` with ``offset = (image_indices[0] % 6) / 3``), plus the raw box predictions."""

    def __init__(self, n_best: int = 1):
        """``n_best`` > 1: the file gains ``"ts_nbest": {qid: [[st_sec, ed_sec, conf], ...]}``, the n_best spans of the predicted
        answer by ``find_max_triples_batch`` (best first, same time mapping, fewer entries when the row has fewer pairs).  The
        ``ts_answer`` records keep their layout, so the evaluation reads such a file unchanged; n_best = 1 writes today's file."""
        if int(n_best) < 1:
            raise ValueError("PredictionWriter: n_best must be >= 1")
        self.n_best = int(n_best)
        self.predictions: Dict[str, object] = dict(ts_answer={}, raw_bbox=[])
        if self.n_best > 1:
            self.predictions["ts_nbest"] = {}

    def add_batch(self, outputs: Mapping[str, object], qids: Sequence[int], image_indices: Sequence[Sequence[int]]) -> None:
        answer, t_scores = outputs["answer"], outputs["t_scores"]             # (N, 5), (N, 5, Li, 2) softmaxed over Li
        rows = _device_rows(answer, t_scores)
        if rows is None:
            pred = answer.detach().max(1)[1]                                   # (N,)
            N, _, Li, _ = t_scores.shape
            picked = t_scores.detach().gather(1, pred.view(N, 1, 1, 1).expand(N, 1, Li, 2)).squeeze(1)    # (N, Li, 2)
            st, ed, _ = find_max_pair_batch(picked[:, :, 0], picked[:, :, 1])
            rows = torch.stack([st, ed, pred], dim=1)
        nbest = None
        if self.n_best > 1:
            N, _, Li, _ = t_scores.shape
            picked = t_scores.detach().gather(1, rows[:, 2].long().view(N, 1, 1, 1).expand(N, 1, Li, 2)).squeeze(1)      # (N, Li, 2)
            span, conf = find_max_triples_batch(picked[:, :, 0], picked[:, :, 1], self.n_best)
            nbest = torch.cat([span.double(), conf.double().unsqueeze(2)], dim=2).cpu().tolist()    # one more copy per batch
        rows = rows.cpu().tolist()                                             # ONE copy per batch
        if outputs.get("att_predictions"):
            self.predictions["raw_bbox"] += outputs["att_predictions"]
        for qid, (s, e, a), img in zip(qids, rows, image_indices):
            offset = (img[0] % 6) / 3
            self.predictions["ts_answer"][str(qid)] = [[s * 2 + offset, (e + 1) * 2 + offset], int(a)]
        if nbest is not None:
            for qid, ranks, img in zip(qids, nbest, image_indices):
                offset = (img[0] % 6) / 3
                self.predictions["ts_nbest"][str(qid)] = [[int(s) * 2 + offset, (int(e) + 1) * 2 + offset, c]
                                                          for (s, e, c) in ranks if s >= 0]

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.predictions, f)


# ---------------------------------------------------------------------------------------------------------------
# temporal metrics (eval/eval_tvqa_plus.py:14-69)
# ---------------------------------------------------------------------------------------------------------------
def temporal_iou(pred: Sequence[float], gt: Sequence[float]) -> float:
    inter = max(0, min(pred[1], gt[1]) - max(pred[0], gt[0]))
    hull = max(pred[1], gt[1]) - min(pred[0], gt[0])          # the reference divides by the hull, not the true union
    return 0 if hull == 0 else 1.0 * inter / hull


def compute_temporal_metrics(pred: Mapping, gt: Mapping) -> Dict[str, float]:
    """pred / gt: {qid: [[st, ed], answer_idx]} (key types may differ: json gives str, the annotation int)."""
    keys = sorted(pred.keys())
    cast = type(next(iter(gt.keys())))
    iou = np.array([temporal_iou(pred[k][0], gt[cast(k)][0]) for k in keys])
    right = np.array([pred[k][1] for k in keys]) == np.array([gt[cast(k)][1] for k in keys])
    res = {}
    for thd in np.arange(0.1, 1, 0.1):
        res["R@{:.2f}".format(thd)] = 1.0 * np.sum(iou >= thd) / len(iou)
    res["miou"] = 1.0 * np.sum(iou) / len(iou)
    res["ans_span_joint_acc@.5"] = 1.0 * np.sum(right * (iou >= 0.5)) / len(right)
    res["qa_acc"] = 1.0 * np.sum(right) / len(right)
    return res


# ---------------------------------------------------------------------------------------------------------------
# grounding mAP (eval/maskrcnn_voc/voc_eval.py + boxlist_ops.py, re-stated on plain arrays)
# ---------------------------------------------------------------------------------------------------------------
def _pairwise_iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(N,4) x (M,4) float32 xyxy, inclusive pixel convention (+1 on widths / heights)."""
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    lt = np.maximum(a[:, None, :2], b[:, :2])
    rb = np.minimum(a[:, None, 2:], b[:, 2:])
    wh = np.clip(rb - lt + 1, 0, None)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area_a[:, None] + area_b - inter)


def _image_table(boxes_by_image: Mapping[str, list], w2i: Mapping[str, int]) -> Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """{image: [[label, score, xyxy], ...]} -> {image: (labels, scores, boxes float32)} without the <unk> labels; images
    that keep no box are dropped (eval_tvqa_plus.py:94-125)."""
    unk = w2i["<unk>"]
    out = {}
    for name, items in boxes_by_image.items():
        lab = np.array([w2i.get(e[0], unk) for e in items])
        keep = [i for i, l in enumerate(lab) if int(l) != unk]
        if not keep:
            continue
        out[name] = (lab[keep], np.array([items[i][1] for i in keep]),
                     np.array([items[i][2] for i in keep], dtype=np.float32))
    return out


def detection_map(pred_by_image: Mapping[str, list], gt_by_image: Mapping[str, list], w2i: Mapping[str, int],
                  iou_thresh: float = 0.5) -> Dict[str, object]:
    """PASCAL-VOC detection AP per object word and their mean (the reference's ``compute_att_metrics_using_maskrcnn_voc``:
    area under the monotone precision envelope, no 'difficult' boxes, +1 on the far box edges before matching, every
    ground-truth box matched at most once, detections of an image without prediction = one dummy box of class 0)."""
    preds = _image_table(pred_by_image, w2i)
    gts = _image_table(gt_by_image, w2i)
    dummy = (np.array([0]), np.array([0]), np.array([[0, 0, 0, 0]], dtype=np.float32))
    scores, matches = defaultdict(list), defaultdict(list)
    all_gt_labels = []
    for name, (g_lab, _g_sc, g_box) in gts.items():
        p_lab, p_sc, p_box = preds.get(name, dummy)
        all_gt_labels.append(g_lab)
        for l in np.unique(np.concatenate((p_lab, g_lab)).astype(int)):
            sel = p_lab == l
            order = p_sc[sel].argsort()[::-1]
            pb, ps = p_box[sel][order], p_sc[sel][order]
            gb = g_box[g_lab == l]
            scores[l].extend(ps)
            if len(pb) == 0:
                continue
            if len(gb) == 0:
                matches[l].extend((0,) * pb.shape[0])
                continue
            pb, gb = pb.copy(), gb.copy()
            pb[:, 2:] += 1
            gb[:, 2:] += 1
            iou = _pairwise_iou(pb, gb)
            who = iou.argmax(axis=1)
            who[iou.max(axis=1) < iou_thresh] = -1
            taken = np.zeros(gb.shape[0], dtype=bool)
            for j in who:
                if j >= 0:
                    matches[l].append(0 if taken[j] else 1)
                    taken[j] = True
                else:
                    matches[l].append(0)
    gt_all = np.concatenate(all_gt_labels)
    per_class, aps = {}, []
    idx2word = {i: w for w, i in w2i.items()}
    for l in np.unique(gt_all.astype(int)):
        n_pos = int(np.sum(gt_all.astype(int) == l))
        entry = average_precision(scores[l], matches[l], n_pos)
        aps.append(entry["ap"])
        entry.update(class_id=int(l), label=idx2word[int(l)])
        per_class[idx2word[int(l)]] = entry
    return {"metrics_per_class": per_class, "overall_map": float(np.nanmean(aps)) if aps else float("nan")}


def average_precision(scores: Sequence[float], matches: Sequence[int], n_pos: int) -> Dict[str, object]:
    """The per-class tail of ``detection_map`` (and of ``grounding.GroundingState.metrics``): the detections of one class -- their
    scores and 0 / 1 matches, in any order -- and its number of ground-truth boxes -> ``ap`` (area under the monotone precision
    envelope), ``precisions``, ``recalls``, ``n_tp``, ``n_fp``, ``n_positives``."""
    sc, mt = np.array(scores, dtype=np.float64), np.array(matches, dtype=np.int8)
    mt = mt[sc.argsort()[::-1]]
    tp, fp = np.cumsum(mt == 1), np.cumsum(mt == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = tp / (fp + tp)
    rec = tp / n_pos
    mpre = np.concatenate(([0], np.nan_to_num(prec), [0]))
    mrec = np.concatenate(([0], rec, [1]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    step = np.where(mrec[1:] != mrec[:-1])[0]
    ap = float(np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1]))
    return {"ap": ap, "precisions": prec.tolist(), "recalls": rec.tolist(), "n_tp": int(np.sum(mt == 1)), "n_fp": int(np.sum(mt == 0)),
            "n_positives": int(n_pos)}


# ---------------------------------------------------------------------------------------------------------------
# files (eval/eval_tvqa_plus.py:148-210)
# ---------------------------------------------------------------------------------------------------------------
def clean_label(label: str) -> str:
    return label.replace(u"’", "'").replace(u"‘", "'").lower()


def _image_key(vid_name: str, qid, frame) -> str:
    return "{}_{}_{:05d}".format(vid_name, int(qid), int(frame))


def load_annotation(raw: Sequence[Mapping]) -> Dict[str, Mapping]:
    """tvqa_plus_{val,...}.json entries -> {"ts_answer": {qid: [ts, answer_idx]}, "bbox": {image: [[label, 1, xyxy]]}}."""
    boxes, spans = defaultdict(list), {}
    for e in raw:
        spans[e["qid"]] = [e["ts"], int(e["answer_idx"])]
        for frame, items in e["bbox"].items():
            key = _image_key(e["vid_name"], e["qid"], frame)
            for b in items:
                boxes[key].append([clean_label(b["label"]), 1,
                                   [b["left"], b["top"], b["left"] + b["width"], b["top"] + b["height"]]])
    return dict(ts_answer=spans, bbox=boxes)


def load_predictions(raw_preds: Mapping, gt_data: Sequence[Mapping], w2i: Mapping[str, int]) -> Dict[str, Mapping]:
    """A ``PredictionWriter`` file -> the evaluation layout: only the boxes predicted for the GROUND-TRUTH answer count, and
    of those only words that are annotated in that frame."""
    idx2word = {i: w for w, i in w2i.items()}
    answer = {int(e["qid"]): int(e["answer_idx"]) for e in gt_data}
    gt_boxes = {int(e["qid"]): e["bbox"] for e in gt_data}
    unk = w2i["<unk>"]
    out: Dict[str, list] = {}
    for per_q in raw_preds["raw_bbox"]:
        qid = None
        for a in range(NUM_ANSWERS):
            if len(per_q[str(a)]) > 0:
                qid = per_q[str(a)][0]["qid"]
        assert qid is not None
        for p in per_q[str(answer[int(qid)])]:
            annotated = [w2i.get(clean_label(b["label"]), unk) for b in gt_boxes[int(qid)][str(p["img_idx"])]]
            key = _image_key(p["vid_name"], qid, p["img_idx"])
            rows = out.setdefault(key, [])
            if p["word"] in annotated:
                rows.extend([idx2word[p["word"]], float(p["pred"][i]), b] for i, b in enumerate(p["bbox"]))
    return dict(ts_answer=raw_preds["ts_answer"], bbox=out)


def evaluate(prediction: Mapping, groundtruth: Mapping, w2i: Mapping[str, int]) -> Dict[str, object]:
    res = dict(detection_map(prediction["bbox"], groundtruth["bbox"], w2i))
    res.update(compute_temporal_metrics(prediction["ts_answer"], groundtruth["ts_answer"]))
    return res


def evaluate_files(pred_path: str, gt_path: str, w2i_path: str, preprocessed: bool = False) -> Dict[str, object]:
    with open(gt_path) as f:
        gt_raw = json.load(f)
    with open(w2i_path) as f:
        w2i = json.load(f)
    with open(pred_path) as f:
        raw = json.load(f)
    prediction = raw if preprocessed else load_predictions(raw, gt_raw, w2i)
    return evaluate(prediction, load_annotation(gt_raw), w2i)


def main(argv: Optional[List[str]] = None) -> None:
    import argparse
    ap = argparse.ArgumentParser(description="TVQA+ metrics: QA Acc., Grd. mAP, Temp. mIoU, ASA")
    ap.add_argument("--gt_path", default="data/tvqa_plus_val.json")
    ap.add_argument("--pred_path", required=True)
    ap.add_argument("--word2idx_path", default="data/word2idx.json")
    ap.add_argument("--output_path")
    ap.add_argument("--no_preproc_pred", action="store_true")
    args = ap.parse_args(argv)
    m = evaluate_files(args.pred_path, args.gt_path, args.word2idx_path, args.no_preproc_pred)
    print("QA Acc. {}\nGrd. mAP {}\nTemp. mIoU{}\nASA {}".format(m["qa_acc"], m["overall_map"], m["miou"],
                                                               m["ans_span_joint_acc@.5"]))
    if args.output_path:
        with open(args.output_path, "w") as f:
            f.write(json.dumps(m, indent=4, sort_keys=True))


if __name__ == "__main__":
    main()
