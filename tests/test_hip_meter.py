"""-m gpu: the run meter on the device (csrc/meter.hip; tvqaplus_amd.meter.RunMeter, stage.reference_loss(meter=...)) against its host
restatement ``host_update`` / ``host_spans`` -- which tests/test_meter_abi.py holds against the reference's own bookkeeping -- and, in
the whole-loop test, against that bookkeeping directly (main.py:69-74, 90-94, 173-183; PredictionWriter + compute_temporal_metrics).

Tolerances: integer fields, ring bytes and the double sums of ``update`` are exact (one IEEE addition of a widened fp32 per call).
``iou_sum``: 1e-12 relative (the kernel's tree against sequential addition of at most 34 values in [0, 1]).  The cls / att / ts parts
of the fused loss against the eager lines: 1e-6 * (1 + |value|), the tolerance of
tests/test_hip_groups.py::test_reference_loss_matches_the_eager_lines (the order of the row sums differs)."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import Fixture

from tvqaplus_amd import meter as M
from test_meter_abi import span_case

pytestmark = pytest.mark.gpu

ATT_W, TS_W = 0.1, 0.5


@contextlib.contextmanager
def _count_calls():
    """Every launching C-ABI call the Python thread makes, by name (the wrapping of tests/test_hip_flat_adam.py)."""
    import tvqaplus_amd._lib as L
    from tvqaplus_amd import ops
    lib = L.load()
    names = [k for k in L.SIGNATURES if not k.endswith("_bytes") and "supported" not in k and "recomputes" not in k
             and k not in ("stage_hip_abi_version", "stage_hip_error_string")]
    real, seen = {k: getattr(lib, k) for k in names}, {}
    for k in names:
        def wrap(*a, _f=real[k], _k=k):
            seen[_k] = seen.get(_k, 0) + 1
            return _f(*a)
        setattr(lib, k, wrap)
    ops._FN.clear()
    try:
        yield seen
    finally:
        for k in names:
            setattr(lib, k, real[k])
        ops._FN.clear()


def _rows(P, C, first_row, g):
    """P rows of logits and targets; the row kind cycles with the GLOBAL row number, so that P = 1 meets every kind over seven calls:
    exact ties (half-integer values), an all-equal row, +inf (twice: a tie of infinities), a NaN next to +inf, all -inf; targets of
    -100 and >= C."""
    x = torch.randn(P, C, generator=g).mul(3).round().div(2)
    t = torch.randint(0, C, (P,), generator=g)
    for r in range(P):
        kind = (first_row + r) % 8
        if kind == 4:
            x[r] = 0.75
        elif kind == 5:
            x[r, C // 2] = float("inf")
            x[r, C - 1] = float("inf")
        elif kind == 6:
            x[r, C - 1] = float("inf")
            x[r, (2 * C) // 3] = float("nan")
            x[r, 0] = float("-inf")
        elif kind == 7:
            x[r] = float("-inf")
        if (first_row + r) % 5 == 3:
            t[r] = -100
        if (first_row + r) % 7 == 2:
            t[r] = C + (first_row + r) % 3
    return x, t


def _same_state(dev_state, host_state):
    assert dev_state.i.tolist() == host_state.i.tolist()
    assert dev_state.ring.tobytes() == host_state.ring.tobytes()
    assert dev_state.f.tobytes() == host_state.f.tobytes(), (dev_state.f, host_state.f)


# ---- 1. update against host_update ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 5, 64])
@pytest.mark.parametrize("P", [1, 5, 255, 256, 257, 600])
def test_update_equals_host_update_over_seven_calls(hip_device, P, C):
    g = torch.Generator().manual_seed(1000 * P + C)
    m = M.RunMeter(hip_device, ring_rows=7 * P)
    m.reset()
    host = M.MeterState(ring_cap=7 * P)
    for k in range(7):
        x, t = _rows(P, C, k * P, g)
        loss, cls, att, ts, gn = (torch.randn((), generator=g) * s for s in (9.0, 5.0, 3.0, 7.0, 20.0))
        gn = gn.abs()
        qids = [10_000 * k + r for r in range(P)]
        on = lambda v: v.to(hip_device)
        if k == 3:                                            # a call without the side losses
            m.update(on(x), on(t), loss=on(loss), qids=qids)
            M.host_update(host, x.numpy(), t.numpy(), loss=loss, qids=qids)
        else:
            m.update(on(x), on(t), on(loss), on(cls), on(att), on(ts), ATT_W, TS_W, qids=qids)
            M.host_update(host, x.numpy(), t.numpy(), loss, cls, att, ts, ATT_W, TS_W, qids=qids)
        m.update_grad_norm(on(gn))
        M.host_update(host, grad_norm=gn)
        if k == 6:
            got = m.read()
            clean = ~torch.isnan(x).any(dim=1)                # the NaN-free rows of the last call: CPU torch's own arg max
            assert got.predictions[6 * P:][clean.numpy()].tolist() == x[clean].max(1)[1].tolist()
    _same_state(got, host)
    assert got.rows == 7 * P and got.steps == 7 and got.grad_norm_steps == 7 and got.ring_dropped == 0 and got.qids == host.qids
    assert got.valid_summary() == host.valid_summary()


# ---- 2. the fused loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 31, 32, 257])
def test_fused_loss_equals_reference_loss_and_books_the_step(hip_device, P):
    from tvqaplus_amd.stage import reference_loss
    C, n_examples = 5, 16
    g = torch.Generator().manual_seed(77 + P)
    total, per_step = M.RunMeter(hip_device, ring_rows=3 * P), M.RunMeter(hip_device)
    total.reset()
    host = M.MeterState(ring_cap=3 * P)
    loss_sum = 0.0
    for k in range(3):
        logits = (3.0 * torch.randn(P, C, generator=g)).to(hip_device)
        targets = torch.randint(0, C, (P,), generator=g)
        if P > 4:
            targets[torch.randperm(P, generator=g)[:2]] = -100
        targets = targets.to(hip_device)
        att = (torch.rand((), generator=g) * 4).to(hip_device)
        ts = (torch.rand((), generator=g) * 9).to(hip_device)
        with_att = k != 1                                     # the middle step has no attention loss (a Python 0, as without sup att)
        res = []
        for meter in (None, total, per_step):
            x = logits.clone().requires_grad_()
            a = att.clone().requires_grad_() if with_att else 0
            t = ts.clone().requires_grad_()
            if meter is per_step:
                meter.reset()
            loss = reference_loss(x, targets, a, t, n_examples, ATT_W, TS_W, meter=meter)
            (loss * 1.7).backward()
            res.append((loss.detach(), x.grad, a.grad if with_att else None, t.grad))
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]) and torch.equal(res[0][1], other[1])
            assert torch.equal(res[0][3], other[3]) and (not with_att or torch.equal(res[0][2], other[2]))
        loss_sum = loss_sum + float(res[0][0])
        # the parts against the eager lines main.py:55-59
        sc = float(n_examples) / P
        cls_ref = float(F.cross_entropy(logits, targets, reduction="sum") * sc)
        att_ref, ts_ref = float(ATT_W * att) if with_att else 0.0, float(TS_W * ts)
        s = per_step.read()
        assert s.steps == 1 and s.rows == P and s.loss_sum == float(res[0][0])
        for got, ref in ((s.cls_sum, cls_ref), (s.att_sum, att_ref), (s.ts_sum, ts_ref)):
            assert abs(got - ref) <= 1e-6 * (1 + abs(ref)), (got, ref)
        M.host_update(host, logits.cpu().numpy(), targets.cpu().numpy())
    s = total.read()
    assert s.loss_sum == loss_sum and s.steps == 3 and s.rows == 3 * P and s.nonfinite_steps == 0
    assert s.correct == host.correct and s.ring.tobytes() == host.ring.tobytes() and s.ring_cursor == 3 * P


# ---- 3. spans ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Li", [1, 2, 65, 300])
@pytest.mark.parametrize("N", [1, 3, 17])
def test_spans_equal_host_spans_and_the_decoder(hip_device, N, Li):
    from tvqaplus_amd import groups
    m = M.RunMeter(hip_device)
    m.reset()
    host = M.MeterState()
    for rep in range(2):                                      # two calls: the counters accumulate
        answer, t_prob, targets, gt, img = span_case(N, Li, 100 * N + Li + rep)
        a, tp = answer.to(hip_device), t_prob.to(hip_device)
        rows = m.update_spans(a, tp, targets.to(hip_device), gt, img, qids=list(range(N)))
        assert rows.dtype == torch.int32 and torch.equal(rows, groups.answer_spans(a, tp))
        ref_rows = M.host_spans(host, answer.numpy(), t_prob.numpy(), targets.numpy(), gt, img, qids=list(range(N)))
        assert rows.cpu().tolist() == ref_rows.tolist()
    got = m.read()
    assert got.i.tolist() == host.i.tolist() and got.span_rows == 2 * N and got.span_qids == host.span_qids
    assert abs(got.iou_sum - host.iou_sum) <= 1e-12 * abs(host.iou_sum)
    assert np.array_equal(got.f[:6], np.zeros(6))
    if Li >= 5:
        assert got.recall_bins[4] >= 2                        # the IoU == 0.5 row of each call is in the 0.5 bin
    assert set(got.temporal_metrics()) == {"R@0.%d0" % k for k in range(1, 10)} | {"miou", "ans_span_joint_acc@.5", "qa_acc"}


# ---- 4. the ring ---------------------------------------------------------------------------------------------------------------
def test_ring_order_overflow_and_guard_bytes(hip_device):
    import tvqaplus_amd._lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(4)
    m = M.RunMeter(hip_device, ring_rows=20)
    m.reset()
    host = M.MeterState(ring_cap=20)
    for k, P in enumerate((7, 1, 12)):
        x, t = _rows(P, 5, 3 * k, g)
        m.update(x.to(hip_device), t.to(hip_device), qids=[100 * k + r for r in range(P)])
        M.host_update(host, x.numpy(), t.numpy(), qids=[100 * k + r for r in range(P)])
    x, t = _rows(1, 5, 0, g)
    with _count_calls() as seen:
        with pytest.raises(ValueError):
            m.update(x.to(hip_device), t.to(hip_device))      # 20 of 20 used: refused on the host
    assert not seen
    got = m.read()
    assert got.ring.tobytes() == host.ring.tobytes() and got.qids == host.qids and got.ring_cursor == 20 and got.steps == 0
    assert got.valid_summary()[2] == host.valid_summary()[2]
    # ABI level: ring_cap = 10 on a buffer allocated for 64 rows; everything behind the 10-row meter is guard
    small, big = int(lib.stage_meter_bytes(10)), int(lib.stage_meter_bytes(64))
    buf = torch.full((big,), 0xAB, dtype=torch.uint8, device=hip_device)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.stage_meter_reset(buf.data_ptr(), 10, st) == 0
    host = M.MeterState(ring_cap=10)
    for P in (16, 5):
        x, t = _rows(P, 5, 0, g)
        xd, td = x.to(hip_device), t.to(hip_device)
        assert lib.stage_meter_update(buf.data_ptr(), 10, xd.data_ptr(), td.data_ptr(), P, 5, None, None, None, None, 1.0, 1.0, None, st) == 0
        M.host_update(host, x.numpy(), t.numpy())
    raw = buf.cpu().numpy()
    assert (raw[small:] == 0xAB).all() and not raw[M.HEAD_BYTES + 20:small].any()
    i = raw[64:256].view(np.int64)
    assert i.tolist() == host.i.tolist() and (int(i[1]), int(i[4]), int(i[5])) == (21, 10, 11)
    assert raw[M.HEAD_BYTES:M.HEAD_BYTES + 20].tobytes() == host.ring.tobytes()


# ---- 5. steady state -----------------------------------------------------------------------------------------------------------
def test_one_library_call_no_allocation_no_synchronisation(hip_device):
    from tvqaplus_amd.stage import reference_loss
    g = torch.Generator().manual_seed(5)
    P, C = 24, 5
    x, t = _rows(P, C, 0, g)
    x, t = x.to(hip_device), t.to(hip_device)
    logits = torch.randn(P, C, generator=g).to(hip_device).requires_grad_()
    vals = [torch.rand((), generator=g).to(hip_device) for _ in range(5)]
    m = M.RunMeter(hip_device)
    m.reset()

    def fused():
        reference_loss(logits, t.clamp(0, C - 1), vals[2], vals[3], 16, ATT_W, TS_W, meter=m)

    m.update(x, t, vals[0], vals[1], vals[2], vals[3], ATT_W, TS_W)           # first calls: anything lazily set up happens here
    m.update_grad_norm(vals[4])
    tc = t.clamp(0, C - 1)
    fused()
    torch.cuda.synchronize()
    with _count_calls() as seen:
        m.update(x, t, vals[0], vals[1], vals[2], vals[3], ATT_W, TS_W)
    assert seen == {"stage_meter_update": 1}, seen
    with _count_calls() as seen:
        m.update_grad_norm(vals[4])
    assert seen == {"stage_meter_update": 1}, seen
    with _count_calls() as seen:
        reference_loss(logits, tc, vals[2], vals[3], 16, ATT_W, TS_W, meter=m)
    assert seen == {"stage_train_loss_meter": 1}, seen
    before = torch.cuda.memory_allocated()
    for _ in range(10):
        m.update(x, t, vals[0], vals[1], vals[2], vals[3], ATT_W, TS_W)
        m.update_grad_norm(vals[4])
        assert torch.cuda.memory_allocated() == before
    reference_loss(logits, tc, vals[2], vals[3], 16, ATT_W, TS_W, meter=m)    # its loss and gradient are freed when it returns
    assert torch.cuda.memory_allocated() == before
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            m.update(x, t, vals[0], vals[1], vals[2], vals[3], ATT_W, TS_W)
            m.update_grad_norm(vals[4])
            reference_loss(logits, tc, vals[2], vals[3], 16, ATT_W, TS_W, meter=m)
        with pytest.raises(RuntimeError):
            m.read()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s = m.read()
    assert s.steps == 22 + 13 and s.grad_norm_steps == 22 and s.rows == 35 * P       # 22 updates, 13 fused losses


# ---- 6. bit repeatability ------------------------------------------------------------------------------------------------------
def test_two_identical_sequences_give_identical_buffers(hip_device):
    from tvqaplus_amd.stage import reference_loss
    bufs = []
    for _ in range(2):
        g = torch.Generator().manual_seed(6)
        m = M.RunMeter(hip_device, ring_rows=2000)
        m.reset()
        for k in range(3):
            x, t = _rows(300, 7, 300 * k, g)
            vals = [torch.randn((), generator=g).to(hip_device) for _ in range(5)]
            m.update(x.to(hip_device), t.to(hip_device), vals[0], vals[1], vals[2], vals[3], ATT_W, TS_W)
            m.update_grad_norm(vals[4].abs())
            reference_loss(torch.randn(33, 5, generator=g).to(hip_device), torch.randint(0, 5, (33,), generator=g).to(hip_device),
                           vals[2], vals[3], 16, ATT_W, TS_W, meter=m)
            answer, t_prob, targets, gt, img = span_case(17, 65, k)
            m.update_spans(answer.to(hip_device), t_prob.to(hip_device), targets.to(hip_device), gt, img)
        torch.cuda.synchronize()
        bufs.append(m.buf.clone())
    assert torch.equal(bufs[0], bufs[1]) and int(bufs[0].count_nonzero()) > 0


# ---- 7. the whole loop ---------------------------------------------------------------------------------------------------------
def _model_from(fx, device):
    from tvqaplus_amd.stage import STAGE
    model = STAGE(fx.opt)
    model.load_state_dict(fx.group("param"), strict=True)
    model.mha_dropout_override = 0.0
    return model.to(device)


def test_training_loop_against_the_item_bookkeeping(hip_device):
    """Three steps on the tiny_train_local fixture with reference_loss(meter=m) + update_grad_norm; beside it main.py:69-74, 90-94
    literally, on the same outputs.  The meter is read and reset after every step and the states are added (what a logging loop
    does per interval): counts exact, loss exact (the same fp32 value widened), the cls / att / ts parts to the eager tolerance."""
    from tvqaplus_amd import parallel
    from tvqaplus_amd.stage import reference_loss
    fx = Fixture("tiny_train_local")
    model = _model_from(fx, hip_device).train()
    batch = fx.batch().to(hip_device)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3)
    criterion = torch.nn.CrossEntropyLoss(reduction="sum")
    m = M.RunMeter(hip_device, ring_rows=64)
    m.reset()
    train_loss, train_loss_att, train_loss_ts, train_loss_cls, train_corrects, norms = [], [], [], [], [], []
    total = M.MeterState()
    qids = batch.qid
    for step in range(3):
        bucket.zero()
        (outputs, targets), att_loss, _, temporal_loss, _ = model(batch)
        loss = reference_loss(outputs, targets, att_loss, temporal_loss, len(qids), ATT_W, TS_W, meter=m)
        loss.backward()
        bucket.all_reduce()
        norm = bucket.clip_grad_norm_(10.0)
        m.update_grad_norm(norm)
        optimizer.step()
        # the reference's lines, beside it
        att_w = ATT_W * att_loss
        ts_w = TS_W * temporal_loss
        cls_loss = criterion(outputs, targets) * (1.0 * len(qids) / len(targets))
        train_loss.append(loss.data.item())
        train_loss_att.append(float(att_w))
        train_loss_ts.append(float(ts_w))
        train_loss_cls.append(cls_loss.item())
        pred_ids = outputs.data.max(1)[1]
        train_corrects += pred_ids.eq(targets.data).tolist()
        norms.append(float(norm))
        s = m.read()
        m.reset()
        assert (s.steps, s.rows, s.nonfinite_steps, s.grad_norm_steps) == (1, len(targets), 0, 1)
        assert s.corrects.tolist() == [int(c) for c in pred_ids.eq(targets.data).tolist()]
        assert s.loss_sum == train_loss[-1] and s.grad_norm_sum == norms[-1] == s.grad_norm_max
        for got, ref in ((s.cls_sum, train_loss_cls[-1]), (s.att_sum, train_loss_att[-1]), (s.ts_sum, train_loss_ts[-1])):
            assert abs(got - ref) <= 1e-6 * (1 + abs(ref)), (got, ref)
        total = total + s
    n = float(len(train_corrects))
    summary = total.train_summary()
    assert total.rows == len(train_corrects) and total.steps == 3 and summary["acc"] == sum(train_corrects) / n
    assert total.grad_norm_max == max(norms)
    ref = dict(loss=train_loss, loss_att=train_loss_att, loss_cls=train_loss_cls, loss_ts=train_loss_ts)
    for key, values in ref.items():
        bound = sum(1e-6 * (1 + abs(v)) for v in values) / n  # every step's value was held to its own bound above
        assert abs(summary[key] - sum(values) / n) <= bound, key
    # a step fed a NaN loss is counted, exactly once
    (outputs, targets), att_loss, _, temporal_loss, _ = model(batch)
    reference_loss(outputs, targets, att_loss, temporal_loss, len(qids), ATT_W, TS_W, meter=m)
    reference_loss(outputs, targets, torch.full((), float("nan"), device=hip_device), temporal_loss, len(qids), ATT_W, TS_W, meter=m)
    reference_loss(outputs, targets, att_loss, temporal_loss, len(qids), ATT_W, TS_W, meter=m)
    s = m.read()
    assert s.nonfinite_steps == 1 and s.steps == 3 and np.isnan(s.loss_sum)


def test_validation_pass_against_validate_and_the_temporal_metrics(hip_device):
    """One eval pass on tiny_eval (the batch twice, as two batches with their own qids): ``update`` against main.py:173-183,
    ``update_spans`` against PredictionWriter + compute_temporal_metrics."""
    from tvqaplus_amd.evaluation import PredictionWriter, compute_temporal_metrics
    fx = Fixture("tiny_eval")
    model = _model_from(fx, hip_device).eval()
    batch = fx.batch().to(hip_device)
    criterion = torch.nn.CrossEntropyLoss(reduction="sum")
    N = len(batch.qid)
    g = torch.Generator().manual_seed(8)
    m = M.RunMeter(hip_device, ring_rows=4 * N)
    m.reset()
    valid_qids, valid_loss, valid_corrects = [], [], []
    writer, gt_all = PredictionWriter(), {}
    for k in range(2):
        qids = [1000 * k + q for q in batch.qid]
        image_indices = [[int(torch.randint(0, 900, (1,), generator=g))] + list(img[1:]) for img in batch.image_indices]
        gt_ts = [[float(v), float(v) + float(torch.rand((), generator=g) * 6)] for v in torch.rand(N, generator=g) * 4]
        with torch.no_grad():
            outputs, att_loss, _, temporal_loss, t_prob = model(batch)
        targets = batch.target
        loss = criterion(outputs, targets) + ATT_W * att_loss + TS_W * temporal_loss
        m.update(outputs, targets, loss=loss, qids=qids)
        rows = m.update_spans(outputs, t_prob, targets, gt_ts, image_indices, qids=qids)
        # main.py:173-176
        valid_qids += [int(x) for x in qids]
        valid_loss.append(loss.data.item())
        pred_ids = outputs.data.max(1)[1]
        valid_corrects += pred_ids.eq(targets.data).tolist()
        writer.add_batch(dict(answer=outputs, t_scores=t_prob), qids, image_indices)
        gt_all.update({q: [gt_ts[n], int(targets[n])] for n, q in enumerate(qids)})
        assert rows[:, 2].tolist() == pred_ids.tolist()
    s = m.read()
    acc = 0.0
    for v in valid_loss:
        acc = acc + v
    valid_acc = sum(valid_corrects) / float(len(valid_corrects))
    qid_corrects = ["%d\t%d" % (a, b) for a, b in zip(valid_qids, valid_corrects)]
    assert s.valid_summary() == (valid_acc, acc / float(len(valid_corrects)), qid_corrects)
    ref = compute_temporal_metrics(writer.predictions["ts_answer"], gt_all)
    got = s.temporal_metrics()
    assert set(got) == set(ref) and s.span_rows == 2 * N and s.span_qids == valid_qids
    for key in ref:
        if key == "miou":
            assert abs(got[key] - ref[key]) <= 1e-12 * abs(ref[key]), (got[key], ref[key])
        else:
            assert got[key] == ref[key], (key, got[key], ref[key])
