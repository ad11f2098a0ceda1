"""-m gpu: the grounding meter on the device (csrc/grounding.hip; tvqaplus_amd.grounding.GroundingMeter) against its host restatement
``host_grounding`` -- which tests/test_grounding_host.py holds against the file route's ``detection_map`` -- and, end to end, against
that route itself on a model's own attention map.

Tolerances: the records are compared as sorted multisets of (label, score bits, match) and the counters as integers: exact (the kernel
copies the scores, and its IoU is ``_pairwise_iou``'s fp32 operations one by one).  ``metrics()`` against ``detection_map``: the
bounds of tests/test_grounding_host.py (rel = 1e-12 on ``overall_map`` and every ``ap``, counts equal)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tvqaplus_amd import grounding as G
from tvqaplus_amd.synth import Batch
from test_grounding_host import check_inputs, file_route, grounding_case, host_state, same_metrics
from test_hip_meter import _count_calls

pytestmark = pytest.mark.gpu


def _on(batch, device):
    out = Batch(batch)
    out.qas = batch.qas.to(device)
    return out


def _same_state(got, host):
    assert got.c.tolist() == host.c.tolist(), (got.c, host.c)
    assert got.sorted_records() == host.sorted_records()
    assert got.n_positives == host.n_positives


# ---- 1. the kernel equals its restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lqa", [4, 12, 40])
@pytest.mark.parametrize("Lr", [5, 25, 64])
def test_update_equals_host_grounding_over_three_calls(hip_device, Lr, Lqa):
    cases = [grounding_case(Lr, Lqa, seed) for seed in (0, 1, 0)]
    _, _, gt, w2i = cases[0]
    m = G.GroundingMeter(hip_device, gt, w2i, capacity=1 << 14)
    m.reset()
    host = G.GroundingState(capacity=1 << 14)
    for scores, batch, _, _ in cases:
        m.update(torch.from_numpy(scores).to(hip_device), _on(batch, hip_device))
        host_state(scores, batch, gt, w2i, state=host)
    got = m.read()
    _same_state(got, host)
    assert got.detections == got.cursor > 0 and (got.dropped, got.overflow, got.bad) == (0, 0, 0) and got.tasks >= 18
    # against detection_map: the first two calls are two batches of distinct scores; as one pass they need distinct image keys, so each
    # is held to its own file-route result
    for scores, batch, _, _ in cases[:2]:
        one = G.GroundingMeter(hip_device, gt, w2i, capacity=1 << 12)
        one.reset()
        one.update(torch.from_numpy(scores).to(hip_device), _on(batch, hip_device))
        st = one.read()
        check_inputs(st, scores, batch, gt, w2i)
        same_metrics(st.metrics(), file_route(scores, batch, gt, w2i))


# ---- 2. capacity -----------------------------------------------------------------------------------------------------------------
def test_capacity_drops_and_guard_bytes(hip_device):
    import tvqaplus_amd._lib as L
    lib = L.load()
    scores, batch, gt, w2i = grounding_case(25)
    full = host_state(scores, batch, gt, w2i)
    cap = 10
    assert full.detections > 2 * cap
    m = G.GroundingMeter(hip_device, gt, w2i, capacity=cap)
    m.reset()
    sd, bd = torch.from_numpy(scores).to(hip_device), _on(batch, hip_device)
    m.update(sd, bd)
    got = m.read()
    assert got.scores.size == cap and got.cursor == got.detections == full.detections and got.dropped == full.detections - cap
    assert got.tasks == full.tasks and (got.overflow, got.bad) == (0, 0)
    expected = full.sorted_records()
    for r in got.sorted_records():
        assert r in expected
        expected.remove(r)                                    # a sub-multiset
    with pytest.raises(ValueError, match="dropped"):
        got.metrics()
    # ABI level: capacity = 10 on a buffer allocated for 64 records; everything behind the 10-record meter is guard
    small, big = int(lib.stage_grounding_bytes(cap)), int(lib.stage_grounding_bytes(64))
    buf = torch.full((big,), 0xAB, dtype=torch.uint8, device=hip_device)
    m.buf = buf                                               # the meter's tables and launch on the caller's buffer
    m.reset()
    m.update(sd, bd)
    m.update(sd, bd)
    raw = buf.cpu().numpy()
    assert (raw[small:] == 0xAB).all()
    c = raw[:G.HEAD_BYTES].view(np.int64)
    assert (int(c[0]), int(c[1]), int(c[2])) == (2 * full.detections, 2 * full.detections - cap, 2 * full.tasks)


# ---- 3. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_book_overflow_and_bad_and_wide_rows_are_refused(hip_device):
    """All memory in range; only table VALUES are out of range, which the kernel checks before it reads."""
    Lqa, Lr = 12, 5
    g = np.random.default_rng(3)
    sc = g.uniform(0.25, 1.0, size=(1, 2, 1, Lqa, Lr)).astype(np.float32)
    sc[..., 4] = -0.5                                          # region 4 is never kept
    rb = np.concatenate([np.array([[0, 0, 9, 9]] * Lr, dtype=np.float32), g.uniform(0, 50, size=(3, 4)).astype(np.float32)])
    gb = np.tile(np.array([[0, 0, 9, 9]], dtype=np.float32), (40, 1))
    words = np.full((1, 2, Lqa), 7, dtype=np.int64)
    words[0, 0, 8:] = 3                                        # statement 0: label 7 eight times, label 3 four times
    words[0, 1, 9:] = 3                                        # statement 1: label 7 nine times
    n_sc, row1 = sc.size, Lqa * Lr
    tasks = np.asarray([
        [0, 0, 7, 0, Lr, 0, 2, 0],                            # eight positions: exact
        [0, 0, 3, 0, 4, 0, 1, 0],                             # four boxes for kept regions 0..3: exact
        [Lqa, row1, 7, 0, Lr, 0, 1, 0],                       # nine positions: overflow
        [0, 0, 3, 0, Lr, 0, 33, 0],                           # 33 ground-truth boxes: overflow
        [0, 0, 3, 0, 3, 0, 1, 0],                             # kept region 3 >= 3 boxes: bad
        [0, n_sc - Lr + 1, 3, 0, Lr, 0, 1, 0],                # first row outside n_scores: bad
        [0, n_sc - 9 * Lr, 3, 0, Lr, 0, 1, 0],                # position 8's row is the map's last, position 9's outside n_scores: bad
        [0, -1, 3, 0, Lr, 0, 1, 0], [2 * Lqa - 1, 0, 3, 0, Lr, 0, 1, 0], [0, 0, 3, 4, Lr, 0, 1, 0], [0, 0, 3, 0, Lr, 40, 1, 0],
        [0, 0, 3, 0, Lr, 0, 0, 0], [0, 0, 1 << 31, 0, Lr, 0, 1, 0], [0, 0, 3, 0, -1, 0, 1, 0], [0, 0, 3, 0, Lr, 0, 41, 0],
    ], dtype=np.int64)
    host = G.host_grounding_tables(G.GroundingState(capacity=4096), sc, words, tasks, rb, gb, Lqa, Lr)
    assert (host.tasks, host.overflow, host.bad, host.detections, host.dropped) == (15, 2, 11, 8 * 4 + 4 * 4, 0)
    m = G.GroundingMeter(hip_device, [], {"<unk>": 0}, capacity=4096)
    m.reset()
    sd, wd = torch.from_numpy(sc).to(hip_device), torch.from_numpy(words).to(hip_device)
    m.update_tables(sd, wd, tasks, rb, gb)
    got = m.read()
    assert got.c.tolist() == host.c.tolist() and got.sorted_records() == host.sorted_records()
    with pytest.raises(ValueError, match="overflow = 2, bad = 11"):
        got.metrics()
    # nine positions book overflow and nothing else
    m.reset()
    m.update_tables(sd, wd, tasks[2:3], rb, gb)
    assert m.read().c.tolist() == [0, 0, 1, 0, 1, 0, 0, 0]
    # Lr = 65 / Lqa = 65: refused before any launch
    wide = torch.zeros(1, 1, 1, 4, 65, device=hip_device)
    with _count_calls() as seen:
        with pytest.raises(ValueError, match="Lr = 65"):
            m.update_tables(wide, torch.zeros(1, 1, 4, dtype=torch.int64, device=hip_device), tasks[:1], rb, gb)
        with pytest.raises(ValueError, match="Lqa = 65"):
            m.update_tables(wide.view(1, 1, 1, 65, 4), torch.zeros(1, 1, 65, dtype=torch.int64, device=hip_device), tasks[:1], rb, gb)
        scores, batch, gt, w2i = grounding_case(5)
        known = G.GroundingMeter(hip_device, gt[:2], w2i, capacity=16)
        with pytest.raises(KeyError):
            known.update(torch.from_numpy(scores).to(hip_device), _on(batch, hip_device))
    assert not seen
    assert m.read().c.tolist() == [0, 0, 1, 0, 1, 0, 0, 0]


def test_the_largest_task_and_equal_scores(hip_device):
    """Eight positions of 64 regions with 32 ground-truth boxes: every list at its limit (more than one candidate per lane), scores
    rounded to two decimals so that equal scores meet (the kernel's order among them is the restatement's: position, then region)."""
    Lqa, Lr = 12, 64
    g = np.random.default_rng(4)
    sc = np.round(g.uniform(0.0, 1.0, size=(1, 1, 2, Lqa, Lr)), 2).astype(np.float32)
    words = np.full((1, 1, Lqa), 9, dtype=np.int64)
    words[0, 0, [1, 4, 10, 11]] = 2
    xy = g.integers(0, 60, size=(2 * Lr + 32, 2))
    wh = g.integers(10, 40, size=(2 * Lr + 32, 2))
    all_boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    rb, gb = all_boxes[:2 * Lr], all_boxes[2 * Lr:]
    tasks = np.asarray([[0, 0, 9, 0, Lr, 0, 32, 0], [0, Lqa * Lr, 9, Lr, Lr, 0, 32, 0], [0, 0, 2, 0, Lr, 3, 7, 0]], dtype=np.int64)
    host = G.host_grounding_tables(G.GroundingState(capacity=4096), sc, words, tasks, rb, gb, Lqa, Lr)
    assert host.detections > 2 * 6 * 64 and (host.overflow, host.bad) == (0, 0) and 0 < host.matches.sum() <= 32 + 32 + 7
    m = G.GroundingMeter(hip_device, [], {"<unk>": 0}, capacity=4096)
    m.reset()
    m.update_tables(torch.from_numpy(sc).to(hip_device), torch.from_numpy(words).to(hip_device), tasks, rb, gb)
    got = m.read()
    assert got.c.tolist() == host.c.tolist() and got.sorted_records() == host.sorted_records()


# ---- 4. call discipline ----------------------------------------------------------------------------------------------------------
def test_one_upload_one_library_call_no_allocation_no_synchronisation(hip_device):
    scores, batch, gt, w2i = grounding_case(25)
    sd, bd = torch.from_numpy(scores).to(hip_device), _on(batch, hip_device)
    m = G.GroundingMeter(hip_device, gt, w2i, capacity=1 << 14)
    m.reset()
    for _ in range(3):                                        # first calls: both pinned buffers and anything lazily set up
        m.update(sd, bd)
    torch.cuda.synchronize()
    uploads, real = [], m._stage.upload

    def counted(t, device):
        uploads.append(int(t.size))
        return real(t, device)

    m._stage.upload = counted
    try:
        with _count_calls() as seen:
            m.update(sd, bd)
        assert seen == {"stage_grounding_update": 1} and len(uploads) == 1, (seen, uploads)
        before = torch.cuda.memory_allocated()
        for _ in range(10):
            m.update(sd, bd)
            assert torch.cuda.memory_allocated() == before
        assert len(uploads) == 11
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(10):
                m.update(sd, bd)
            with pytest.raises(RuntimeError):
                m.read()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        m._stage.upload = real
    one = host_state(scores, batch, gt, w2i)
    s = m.read()
    assert s.tasks == 24 * one.tasks and s.detections == 24 * one.detections and (s.dropped, s.overflow, s.bad) == (0, 0, 0)


# ---- 5. repeatability ------------------------------------------------------------------------------------------------------------
def test_two_identical_sequences_give_identical_records_and_metrics(hip_device):
    out = []
    for _ in range(2):
        _, _, gt, w2i = grounding_case(25)
        m = G.GroundingMeter(hip_device, gt, w2i, capacity=1 << 14)
        m.reset()
        for k in range(3):
            scores, batch, _, _ = grounding_case(25, 12, seed=5 * k)
            m.update(torch.from_numpy(scores).to(hip_device), _on(batch, hip_device))
        out.append(m.read())
    a, b = out
    assert a.c.tolist() == b.c.tolist() and a.sorted_records() == b.sorted_records() and a.detections > 0
    assert a.metrics() == b.metrics()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def test_eval_pass_against_the_inference_mode_file_route(hip_device, tmp_path):
    """A random small model on a synthetic batch with word ids, region boxes and annotated images filled in: ``eval()`` +
    ``forward_main`` + ``GroundingMeter`` against the same model in ``inference_mode`` through ``PredictionWriter``, a file, and
    ``evaluation.evaluate_files``' grounding half -- both on the map's own values."""
    import json
    from tvqaplus_amd import evaluation as E
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    from test_grounding_host import OBJECT_WORDS, W2I
    N, Li, Lr, Lqa = 4, 6, 12, 10
    torch.manual_seed(7)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(hsz=16, embedding_size=64, vfeat_size=300)).to(hip_device).eval()
    batch = make_batch(N=N, Li=Li, Lr=Lr, Lw=8, Lqa=Lqa, wd_size=64, seed=11, ragged=True)
    rng = np.random.default_rng(12)
    batch.qas = torch.from_numpy(rng.integers(2, 12, size=(N, 5, Lqa)).astype(np.int64))
    batch.eval_object_word_ids = OBJECT_WORDS
    batch.anno_st_idx = [1, 0, 2, 1]
    batch.image_indices = [[100 * b + 6 * i + 3 for i in range(Li)] for b in range(N)]
    idx2word = {i: w for w, i in W2I.items()}
    gt, boxes = [], []
    for b in range(N):
        per_image, frames = [], {}
        for local in range(2):
            xy = rng.integers(0, 300, size=(Lr, 2))
            wh = rng.integers(20, 200, size=(Lr, 2))
            regions = np.concatenate([xy, xy + wh], axis=1)
            per_image.append(regions.tolist())
            items = []
            for r in rng.permutation(Lr)[:5].tolist():         # five labelled boxes next to region boxes (labels repeat within a frame)
                x1, y1, x2, y2 = (regions[r] + rng.integers(-6, 7, size=4)).tolist()
                items.append({"label": idx2word[int(rng.integers(2, 10))].capitalize(), "left": x1, "top": y1, "width": x2 - x1,
                              "height": y2 - y1})
            frames[str(batch.image_indices[b][batch.anno_st_idx[b] + local])] = items
        boxes.append(per_image)
        gt.append({"qid": 500 + b, "vid_name": "clip_%d" % b, "answer_idx": str(int(rng.integers(0, 5))), "ts": [0.0, 4.0], "bbox": frames})
    batch.boxes, batch.qid, batch.vid_name = boxes, [e["qid"] for e in gt], [e["vid_name"] for e in gt]
    batch = batch.to(hip_device)
    # (a) the file route
    model.inference_mode = True
    with torch.no_grad():
        out = model(batch)
    model.inference_mode = False
    writer = E.PredictionWriter()
    writer.add_batch(out, batch.qid, batch.image_indices)
    paths = {k: str(tmp_path / (k + ".json")) for k in ("pred", "gt", "w2i")}
    writer.save(paths["pred"])
    for k, v in (("gt", gt), ("w2i", W2I)):
        with open(paths[k], "w") as f:
            json.dump(v, f)
    ref = E.evaluate_files(paths["pred"], paths["gt"], paths["w2i"])
    # (b) the meter
    m = G.GroundingMeter(hip_device, gt, W2I, capacity=1 << 14)
    m.reset()
    with torch.no_grad():
        scores = model.forward_main(batch)[-1]["vid_raw_s"]
    m.update(scores, batch)
    st = m.read()
    assert st.detections > 0 and st.matches.sum() > 0 and (st.dropped, st.overflow, st.bad) == (0, 0, 0)
    for l in set(st.labels.tolist()):                          # the condition of the equality claim
        s = st.scores[st.labels == l]
        assert len(set(s.view(np.uint32).tolist())) == s.size, l
    same_metrics(st.metrics(), ref)
    _same_state(st, host_state(scores, batch, gt, W2I))
