"""CPU: the grounding meter's specification (tvqaplus_amd/grounding.py: ``host_grounding`` + ``GroundingState.metrics``, what
tests/test_hip_grounding.py holds the kernel against) IS the file route's grounding mAP: the predictions of
``att_host.get_att_prediction``'s host loop in a ``PredictionWriter``-shaped dict, through ``evaluation.load_predictions`` and
``evaluation.detection_map`` -- which tests/test_evaluation.py pins to the reference's own evaluation code -- on the same synthetic
inputs, and directly on the reference-generated fixture tests/golden/eval_metrics.json.

Bounds: ``overall_map`` and every ``ap`` to rel = 1e-12 (the bound of tests/test_evaluation.py; both sides run the same
``evaluation.average_precision`` on the same multiset of (score, match) pairs, so the values are in fact equal); ``n_tp``, ``n_fp``,
``n_positives`` and the set of classes are equal."""
import json
import os

import numpy as np
import pytest
import torch

from tvqaplus_amd import evaluation as E
from tvqaplus_amd import grounding as G
from tvqaplus_amd.synth import Batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

W2I = {"<pad>": 0, "<unk>": 1, "sheldon": 2, "leonard": 3, "penny": 4, "cup": 5, "laptop": 6, "door": 7, "phone": 8, "couch": 9,
       "the": 10, "is": 11}
OBJECT_WORDS = list(range(2, 10))
N, NA, LI = 3, 5, 6
THD = np.float32(0.2)


def _box(b):
    return {"label": b[0], "left": b[1], "top": b[2], "width": b[3] - b[1], "height": b[4] - b[2]}


def grounding_case(Lr, Lqa=12, seed=0):
    """scores (N, NA, Li, Lqa, Lr) float32, the batch fields the meter reads, the annotation entries and the word table.

    Example 0 (qid 100, answer 2, images at dense frames 1, 2 = frame numbers 9, 15): the statement holds `sheldon` at positions 0 and
    2 (a label whose word occurs twice), `cup` at 1, `door` at 3 (an object word that is not annotated in frame 9); frame 9 has TWO
    sheldon boxes, and regions 2 and 3 both lie over the first one (the second detection of it is a false positive), one cup box whose
    row holds a score of exactly float32(0.2) and one a single ulp below, a `phone` box (a label whose word does not occur) and an
    <unk> label; frame 15 has the cup box [0, 0, 9, 10] with region 0 = [0, 0, 9, 4] (IoU exactly 0.5) and region 1 = [0, 0, 9, 3]
    (0.4167).  Frame 40 is annotated but not in the batch (it counts in n_positives only).
    Example 1 (qid 101): no annotated images in the batch.
    Example 2 (qid 102, answer 0, one image): `Leonard` (cleaned to lower case) with a box, `couch` whose row has nothing >= 0.2."""
    assert Lr >= 5 and Lqa >= 4
    rng = np.random.default_rng(1000 * Lr + 10 * Lqa + seed)
    scores = rng.uniform(-0.6, 1.0, size=(N, NA, LI, Lqa, Lr)).astype(np.float32)
    scores[..., Lr - 1] = -np.abs(scores[..., Lr - 1])         # a region below the threshold in every row
    qas = rng.integers(10, 12, size=(N, NA, Lqa)).astype(np.int64)        # filler words outside the object vocabulary
    qas[0, 2, :4] = [2, 5, 2, 7]
    qas[2, 0, :4] = [10, 3, 11, 9]
    if Lqa >= 12:
        qas[0, 2, 5] = 6                                       # laptop: in the vocabulary, annotated nowhere
    qas[0, 1, :2] = [4, 8]                                     # a wrong answer that names annotated objects: never read

    def rand_boxes(n):
        xy = rng.integers(0, 300, size=(n, 2))
        wh = rng.integers(20, 200, size=(n, 2))
        return np.concatenate([xy, xy + wh], axis=1).tolist()

    boxes = [[rand_boxes(Lr), rand_boxes(Lr)], [], [rand_boxes(Lr)]]
    # example 0, frame 9 (dense frame 1)
    boxes[0][0][2] = [12, 12, 108, 112]
    boxes[0][0][3] = [10, 10, 110, 110]
    scores[0, 2, 1, 0, :] = rng.uniform(-0.6, 0.19, size=Lr).astype(np.float32)      # the first sheldon row keeps regions 2 and 3 only,
    scores[0, 2, 1, 2, :] = np.minimum(scores[0, 2, 1, 2, :], np.float32(0.8))        # and they lead the second one
    scores[0, 2, 1, 2, :] -= np.linspace(0, 0.01, Lr, dtype=np.float32)               # (the clipped ones stay distinct)
    scores[0, 2, 1, 0, 2], scores[0, 2, 1, 0, 3] = 0.83, 0.91
    scores[0, 2, 1, 1, 0] = THD
    scores[0, 2, 1, 1, 1] = np.nextafter(THD, np.float32(0))
    # example 0, frame 15 (dense frame 2)
    boxes[0][1][0] = [0, 0, 9, 4]
    boxes[0][1][1] = [0, 0, 9, 3]
    scores[0, 2, 2, 1, :2] = [0.77, 0.66]
    scores[0, 2, 2, 1, 2:] = -0.25
    # example 2: couch (position 3) keeps nothing
    scores[2, 0, 0, 3, :] = rng.uniform(-0.5, 0.19, size=Lr).astype(np.float32)
    near = lambda b, d: [b[0] + d, b[1] - d, b[2] + 2 * d, b[3] + d]
    gt = [
        {"qid": 100, "vid_name": "s01e01_seg01_clip_00", "answer_idx": "2", "ts": [1.0, 5.0], "bbox": {
            "9": [_box(["Sheldon", 10, 10, 110, 110]), _box(["sheldon", 300, 50, 400, 200]), _box(["cup"] + near(boxes[0][0][0], 3)),
                  _box(["phone"] + boxes[0][0][1]), _box(["unknownthing", 5, 5, 50, 50])],
            "15": [_box(["cup", 0, 0, 9, 10]), _box(["sheldon"] + near(boxes[0][1][2], 5))],
            "40": [_box(["penny", 1, 2, 30, 40]), _box(["sheldon", 3, 4, 50, 60])]}},
        {"qid": 101, "vid_name": "s01e01_seg01_clip_01", "answer_idx": "4", "ts": [0.0, 2.0], "bbox": {
            "50": [_box(["leonard", 20, 20, 90, 140])]}},
        {"qid": 102, "vid_name": "s01e01_seg01_clip_02", "answer_idx": "0", "ts": [3.0, 4.0], "bbox": {
            "7": [_box(["Leonard"] + near(boxes[2][0][1], 2)), _box(["couch"] + boxes[2][0][0]), _box(["leonard", 400, 200, 500, 300])]}},
    ]
    batch = Batch(qid=[100, 101, 102], vid_name=[e["vid_name"] for e in gt], qas=torch.from_numpy(qas), anno_st_idx=[1, 0, 0],
                  image_indices=[[3, 9, 15, 21, 27, 33], [50, 56, 62, 68, 74, 80], [7, 13, 19, 25, 31, 37]], boxes=boxes,
                  eval_object_word_ids=OBJECT_WORDS)
    return scores, batch, gt, W2I


def file_route(scores, batch, gt, w2i):
    """The grounding mAP as the file route computes it: ``get_att_prediction``'s host loop on a host tensor, a ``PredictionWriter``-
    shaped dict through JSON, ``load_predictions``, ``detection_map``.  (A question without annotated images has no entry under any
    answer; ``load_predictions`` cannot name the question of such an entry, so it is left out of ``raw_bbox``: it predicts nothing.)"""
    from tvqaplus_amd.att_host import get_att_prediction
    sc = scores if torch.is_tensor(scores) else torch.from_numpy(np.asarray(scores))
    per_q = get_att_prediction(sc.cpu(), batch.eval_object_word_ids, batch.qas.cpu(), batch.vid_name, batch.qid, batch.image_indices,
                               batch.boxes, batch.anno_st_idx)
    raw = dict(ts_answer={}, raw_bbox=[q for q in per_q if any(len(v) for v in q.values())])
    raw = json.loads(json.dumps(raw))
    pred = E.load_predictions(raw, gt, w2i)
    return E.detection_map(pred["bbox"], E.load_annotation(gt)["bbox"], w2i)


def same_metrics(got, ref):
    assert got["overall_map"] == pytest.approx(ref["overall_map"], rel=1e-12, abs=0)
    assert set(got["metrics_per_class"]) == set(ref["metrics_per_class"])
    for k, r in ref["metrics_per_class"].items():
        g = got["metrics_per_class"][k]
        assert g["ap"] == pytest.approx(r["ap"], rel=1e-12, abs=0), k
        assert (g["n_tp"], g["n_fp"], g["n_positives"]) == (r["n_tp"], r["n_fp"], r["n_positives"]), k


def host_state(scores, batch, gt, w2i, capacity=1 << 16, state=None):
    state = G.GroundingState(capacity=capacity) if state is None else state
    return G.host_grounding(state, scores, batch, G.GroundingIndex(gt, w2i))


def check_inputs(state, scores, batch, gt, w2i):
    """The conditions the comparison rests on: the scores of a class are distinct (the reference orders equal scores by an unstable
    sort), and every labelled image has a region below the threshold in the rows that are read (a threshold ignored would show)."""
    for l in set(state.labels.tolist()):
        s = state.scores[state.labels == l]
        assert len(set(s.view(np.uint32).tolist())) == s.size, l
    tasks, _, _ = G.GroundingIndex(gt, w2i).tables(batch, scores.shape)
    qas = batch.qas.numpy().reshape(-1)
    flat = np.asarray(scores).reshape(-1)
    Lqa, Lr = scores.shape[3], scores.shape[4]
    assert tasks.shape[0] >= 6
    for word_off, score_off, label, *_ in tasks.tolist():
        for w in np.flatnonzero(qas[word_off:word_off + Lqa] == label).tolist():
            assert (flat[score_off + w * Lr:score_off + (w + 1) * Lr] < THD).any()


@pytest.mark.parametrize("Lr", [5, 25, 64])
def test_host_grounding_is_the_file_routes_detection_map(Lr):
    scores, batch, gt, w2i = grounding_case(Lr)
    st = host_state(scores, batch, gt, w2i)
    check_inputs(st, scores, batch, gt, w2i)
    assert (st.dropped, st.overflow, st.bad) == (0, 0, 0) and st.cursor == st.detections == st.scores.size > 0
    ref = file_route(scores, batch, gt, w2i)
    got = st.metrics()
    same_metrics(got, ref)
    assert set(got["metrics_per_class"]) == {"sheldon", "leonard", "penny", "cup", "phone", "couch"}
    assert got["metrics_per_class"]["sheldon"]["n_positives"] == 4 and got["metrics_per_class"]["penny"]["n_tp"] == 0
    assert st.n_positives == {2: 4, 5: 2, 8: 1, 4: 1, 3: 3, 9: 1}
    # the constructed cases, read off the records
    rec = {(l, np.uint32(b).view(np.float32).item()): m for l, b, m in st.sorted_records()}
    assert rec[(5, float(THD))] in (0, 1) and (5, float(np.nextafter(THD, np.float32(0)))) not in rec      # 0.2 kept, one ulp below not
    assert rec[(5, float(np.float32(0.77)))] == 1 and rec[(5, float(np.float32(0.66)))] == 0               # IoU 0.5 matches, 0.4167 does not
    assert rec[(2, float(np.float32(0.91)))] == 1 and rec[(2, float(np.float32(0.83)))] == 0               # the second one over a taken box
    assert not any(l in (6, 7, 8, 9) for l, _, _ in st.sorted_records())      # no record without an annotated, occurring, kept word


def test_pairwise_iou_of_the_threshold_boxes():
    gt = np.array([[0, 0, 9, 10]], dtype=np.float32)
    det = np.array([[0, 0, 9, 4], [0, 0, 9, 3]], dtype=np.float32)
    gt[:, 2:] += 1
    det[:, 2:] += 1
    iou = E._pairwise_iou(det, gt)[:, 0]
    assert iou[0] == np.float32(0.5) and abs(float(iou[1]) - 0.4167) < 1e-4 and iou.dtype == np.float32


def test_states_add_limits_and_refusals():
    from tvqaplus_amd._lib import StageHipError
    scores, batch, gt, w2i = grounding_case(25)
    a = host_state(scores, batch, gt, w2i)
    scores2, batch2, _, _ = grounding_case(25, seed=1)
    b = host_state(scores2, batch2, gt, w2i)
    c = a + b
    assert c.c.tolist() == (a.c + b.c).tolist() and c.sorted_records() == sorted(a.sorted_records() + b.sorted_records())
    assert c.n_positives == {k: 2 * v for k, v in a.n_positives.items()} and c.capacity == a.capacity + b.capacity
    assert set(c.metrics()["metrics_per_class"]) == set(a.metrics()["metrics_per_class"])
    # capacity: what does not fit is counted, and metrics() names it
    small = host_state(scores, batch, gt, w2i, capacity=3)
    assert small.scores.size == 3 and small.cursor == a.cursor and small.dropped == a.cursor - 3
    with pytest.raises(ValueError, match="dropped"):
        small.metrics()
    # a qid that is not annotated; a ground-truth label with word id 0
    other = Batch(batch)
    other.qid = [100, 101, 999]
    with pytest.raises(KeyError):
        host_state(scores, other, gt, w2i)
    w2i_zero = dict(w2i, **{"<pad>": 12, "cup": 0})
    with pytest.raises(ValueError, match="word id is 0"):
        host_state(scores, batch, gt, w2i_zero)
    with pytest.raises(StageHipError):
        G.GroundingMeter("cpu", gt, w2i, capacity=16)
    # the limits of the table form: 9 positions / 33 boxes book `overflow`, a row or a box outside its table books `bad`
    Lqa, Lr = 12, 5
    sc = np.full((1, 1, 1, Lqa, Lr), 0.5, dtype=np.float32)
    rb = np.tile(np.array([[0, 0, 9, 9]], dtype=np.float32), (Lr, 1))
    gb = np.tile(np.array([[0, 0, 9, 9]], dtype=np.float32), (40, 1))
    words = np.full(Lqa, 7, dtype=np.int64)
    words[9:] = 3
    ok = [0, 0, 3, 0, Lr, 0, 1, 0]
    tasks = [ok, [0, 0, 7, 0, Lr, 0, 1, 0], [0, 0, 3, 0, Lr, 0, 33, 0], [0, 0, 3, 0, Lr - 1, 0, 1, 0], [0, 1, 3, 0, Lr, 0, 1, 0],
             [0, 0, 3, 1, Lr, 0, 1, 0], [0, 0, 3, 0, Lr, 40, 1, 0], [1, 0, 3, 0, Lr, 0, 1, 0], [0, 0, -1, 0, Lr, 0, 1, 0], [0, 0, 3, 0, Lr, 0, 0, 0]]
    st = G.host_grounding_tables(G.GroundingState(capacity=100), sc, words, np.asarray(tasks), rb, gb, Lqa, Lr)
    assert (st.tasks, st.overflow, st.bad, st.detections, st.dropped) == (10, 2, 7, 3 * Lr, 0)
    assert st.matches.sum() == 1 and set(st.labels.tolist()) == {3}


@pytest.mark.parametrize("case", range(3))
def test_records_rebuilt_from_the_reference_fixture_reproduce_its_numbers(case):
    """tests/golden/eval_metrics.json (the reference's own evaluation code on a prediction file): for every entry of the ground-truth
    answer the `pred` values are placed in a score row, its `bbox` list becomes (a part of) the image's region boxes, its `word` goes
    into a made-up statement; the new path on these inputs gives the fixture's `expected` per-class numbers."""
    c = json.load(open(os.path.join(GOLDEN, "eval_metrics.json")))[case]
    gt, raw, w2i, exp = c["gt"], c["pred"], c["w2i"], c["expected"]
    by_qid = {}
    for per_q in raw["raw_bbox"]:
        for a, entries in per_q.items():
            for p in entries:
                by_qid.setdefault(int(p["qid"]), {}).setdefault(int(a), []).append(p)
    plans = []                                                 # per question: (answer, frames, statement, [(frame k, position, first region, entry)])
    for e in gt:
        answer = int(e["answer_idx"])
        frames, statement, rows, used = [], [], [], {}
        for p in by_qid.get(int(e["qid"]), {}).get(answer, []):
            if p["img_idx"] not in frames:
                frames.append(p["img_idx"])
            k = frames.index(p["img_idx"])
            if p["word"] not in statement:
                statement.append(p["word"])
            rows.append((k, statement.index(p["word"]), used.get(k, 0), p))
            used[k] = used.get(k, 0) + len(p["bbox"])
        plans.append((answer, frames, statement, rows, used))
    n = len(gt)
    Li = max(1, max(len(p[1]) for p in plans))
    Lqa = max(1, max(len(p[2]) for p in plans))
    Lr = max(1, max(max(p[4].values(), default=0) for p in plans))
    assert Lr <= 64 and Lqa <= 64
    scores = np.full((n, 5, Li, Lqa, Lr), -1.0, dtype=np.float32)
    pad = max(w2i.values()) + 1
    qas = np.full((n, 5, Lqa), pad, dtype=np.int64)
    boxes, image_indices = [], []
    for b, (answer, frames, statement, rows, used) in enumerate(plans):
        qas[b, answer, :len(statement)] = statement
        per_image = [[[0, 0, 0, 0] for _ in range(used.get(k, 0))] for k in range(len(frames))]
        for k, w, first, p in rows:
            assert min(p["pred"], default=1.0) >= 0.2
            scores[b, answer, k, w, first:first + len(p["pred"])] = p["pred"]
            per_image[k][first:first + len(p["bbox"])] = p["bbox"]
        boxes.append(per_image)
        image_indices.append(frames + [10_000 + i for i in range(Li - len(frames))])
    batch = Batch(qid=[e["qid"] for e in gt], vid_name=[e["vid_name"] for e in gt], qas=torch.from_numpy(qas), anno_st_idx=[0] * n,
                  image_indices=image_indices, boxes=boxes, eval_object_word_ids=[i for i in w2i.values() if i != w2i["<unk>"]])
    st = host_state(scores, batch, gt, w2i)
    got = st.metrics()
    assert got["overall_map"] == pytest.approx(exp["overall_map"], rel=1e-12, abs=1e-15)
    assert sorted(got["metrics_per_class"]) == sorted(exp["per_class"])
    for k, e in exp["per_class"].items():
        g = got["metrics_per_class"][k]
        assert g["ap"] == pytest.approx(e["ap"], rel=1e-12, abs=1e-15), k
        assert (g["n_tp"], g["n_fp"], g["n_positives"]) == (e["n_tp"], e["n_fp"], e["n_positives"]), k
