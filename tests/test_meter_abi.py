"""CPU-side checks of the run meter (include/stage_hip.h "Run meter", csrc/meter.hip, tvqaplus_amd/meter.py): the five symbols are
exported and bound under the unchanged ABI version, the size query answers without a GPU, the argument checks answer before any
launch, and the host restatement of the two kernels (``host_update`` / ``host_spans``: what tests/test_hip_meter.py holds the kernels
against) IS the reference's bookkeeping -- a literal transcription of main.py:69-74, 90-94, 173-183 and ``PredictionWriter`` +
``compute_temporal_metrics``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

from tvqaplus_amd import meter as M

SYMBOLS = ["stage_meter_bytes", "stage_meter_reset", "stage_meter_update", "stage_train_loss_meter", "stage_meter_spans"]


@pytest.fixture(scope="module")
def lib():
    from tvqaplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", ROOT, "-j8"], stdout=subprocess.DEVNULL)
    return _lib.load()


def test_symbols_exported_and_bound_under_abi_5(lib):
    from tvqaplus_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0], name
    assert lib.stage_hip_abi_version() == 7 == _lib.ABI_VERSION


def test_size_query_needs_no_gpu(lib):
    prev = 0
    for cap in [0, 1, 2, 3, 4, 5, 255, 256, 257, 4096, 100_001, 1 << 20, (1 << 31) + 3]:
        b = lib.stage_meter_bytes(cap)
        assert b >= 8 * 8 + 24 * 8 + 2 * cap, cap
        assert b >= prev and b % 8 == 0, cap
        prev = b
    assert lib.stage_meter_bytes(0) == M.HEAD_BYTES == 256
    assert lib.stage_meter_bytes(-1) == 0


def test_calls_reject_null_meter_and_bad_shapes(lib):
    """The argument checks answer before anything touches the device: the library's shape error, no launch.  As in
    tests/test_flat_adam_abi.py, the per-argument part (ONE bad argument, every other one plausible) runs where no GPU is visible --
    there a call that slipped through a regressed check fails in the launch and this test fails; with a GPU in sight it would launch
    on made-up addresses, so there every call carries a NULL meter AND a bad size (refused by two independent checks)."""
    from tvqaplus_amd import _lib
    E = _lib.STAGE_ERR_SHAPE
    thd = (ctypes.c_double * 9)(*M.THD)
    p = 4096      # never dereferenced: every call below is refused by the checks in front of the launches
    upd = [p, 8, p, p, 4, 5, p, p, p, p, 0.1, 0.5, p, None]
    fused = [p, p, p, p, None, 1.0, 0.1, 0.5, p, p, 4, 5, None, p, 8]
    spans = [p, p, p, p, p, ctypes.addressof(thd), 3, 5, 7, p, None]

    def with_(args, **kw):
        out = list(args)
        for i, v in kw.items():
            out[int(i[1:])] = v
        return out

    if torch.cuda.is_available():
        assert lib.stage_meter_reset(None, -1, None) == E
        assert lib.stage_meter_update(*with_(upd, _0=None, _4=-1)) == E
        assert lib.stage_train_loss_meter(*with_(fused, _13=None, _10=0)) == E
        assert lib.stage_meter_spans(*with_(spans, _0=None, _7=65)) == E
        return
    assert lib.stage_meter_reset(None, 8, None) == E
    assert lib.stage_meter_reset(p, -1, None) == E
    assert lib.stage_meter_reset(p + 4, 8, None) == E                        # not 8-byte aligned
    for bad in (dict(_0=None), dict(_0=p + 2), dict(_1=-1), dict(_4=-1), dict(_5=0), dict(_5=4097)):
        assert lib.stage_meter_update(*with_(upd, **bad)) == E, bad
    assert lib.stage_meter_update(p, 0, None, None, 0, 0, None, None, None, None, 1.0, 1.0, None, None) == 0     # nothing to add: no launch
    for bad in (dict(_13=None), dict(_13=p + 1), dict(_14=-1), dict(_10=0), dict(_10=-3), dict(_11=0), dict(_11=4097), dict(_0=None),
                dict(_1=None), dict(_8=None), dict(_9=None)):
        assert lib.stage_train_loss_meter(*with_(fused, **bad)) == E, bad
    for bad in (dict(_0=None), dict(_1=None), dict(_2=None), dict(_3=None), dict(_4=None), dict(_5=None), dict(_6=-1), dict(_7=0),
                dict(_7=65), dict(_8=0), dict(_8=2049), dict(_2=p + 4)):
        assert lib.stage_meter_spans(*with_(spans, **bad)) == E, bad
    assert lib.stage_meter_spans(*with_(spans, _6=0)) == 0                   # no example: no launch


def _steps(seed, n_steps=7):
    """Random host data of a loop: logits with exact ties, +-inf, an all-equal row, a NaN row, targets of -100 and >= C."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n_steps):
        P, C = int(torch.randint(1, 40, (1,), generator=g)), 5
        x = torch.randn(P, C, generator=g).mul(3).round().div(2)            # half-integers: many exact ties
        t = torch.randint(0, C, (P,), generator=g)
        if P > 6:
            x[1] = 1.25
            x[2, 3] = float("inf")
            x[3, :] = float("-inf")
            x[4, 2] = float("nan")
            x[4, 4] = float("inf")
            t[5] = -100
            t[6] = C + 2
        att, ts = torch.rand((), generator=g) * 3, torch.rand((), generator=g) * 7
        cls = torch.rand((), generator=g) * 11
        out.append((x, t, cls, att, ts, [1000 * k + r for r in range(P)]))
    return out


def test_host_update_is_the_training_loops_bookkeeping():
    """main.py:55-60, 69-74, 90-94, transcribed: counts exact, sums bit-equal to sequential float64 addition."""
    att_weight, ts_weight = 0.1, 0.5
    train_loss, train_loss_att, train_loss_ts, train_loss_cls, train_corrects = [], [], [], [], []
    st = M.MeterState(ring_cap=10_000)
    for outputs, targets, cls_loss, att_raw, ts_raw, _ in _steps(11):
        att_loss = att_weight * att_raw
        temporal_loss = ts_weight * ts_raw
        loss = cls_loss + att_loss + temporal_loss
        train_loss.append(loss.data.item())
        train_loss_att.append(float(att_loss))
        train_loss_ts.append(float(temporal_loss))
        train_loss_cls.append(cls_loss.item())
        pred_ids = outputs.data.max(1)[1]
        train_corrects += pred_ids.eq(targets.data).tolist()
        M.host_update(st, outputs.numpy(), targets.numpy(), loss, cls_loss, att_raw, ts_raw, att_weight, ts_weight)

    def seq(values):          # sequential float64 addition (np.sum is pairwise, CPython 3.12's sum() compensated)
        acc = 0.0
        for v in values:
            acc = acc + v
        return acc

    n = float(len(train_corrects))
    assert st.steps == 7 and st.rows == len(train_corrects) and st.correct == int(seq(train_corrects))
    assert st.corrects.tolist() == [int(c) for c in train_corrects] and st.ring_dropped == 0 and st.ring_cursor == st.rows
    assert st.loss_sum == seq(train_loss) and st.att_sum == seq(train_loss_att)
    assert st.ts_sum == seq(train_loss_ts) and st.cls_sum == seq(train_loss_cls)
    assert st.nonfinite_steps == 0
    s = st.train_summary()
    assert s == dict(acc=int(seq(train_corrects)) / n, loss=seq(train_loss) / n, loss_att=seq(train_loss_att) / n,
                     loss_cls=seq(train_loss_cls) / n, loss_ts=seq(train_loss_ts) / n)
    M.host_update(st, loss=torch.tensor(float("nan")))
    M.host_update(st, loss=torch.tensor(float("inf")))
    assert st.nonfinite_steps == 2 and st.steps == 9 and st.rows == len(train_corrects)
    M.host_update(st, grad_norm=torch.tensor(3.5))
    M.host_update(st, grad_norm=torch.tensor(1.5))
    assert (st.grad_norm_sum, st.grad_norm_max, st.grad_norm_steps, st.steps) == (5.0, 3.5, 2, 9)


def test_host_update_is_validates_bookkeeping_and_the_ring_drops_what_does_not_fit():
    """main.py:173-183, transcribed."""
    valid_qids, valid_loss, valid_corrects = [], [], []
    st, small = M.MeterState(ring_cap=10_000), M.MeterState(ring_cap=10)
    for outputs, targets, loss, _, _, qids in _steps(12):
        valid_qids += [int(x) for x in qids]
        valid_loss.append(loss.data.item())
        pred_ids = outputs.data.max(1)[1]
        valid_corrects += pred_ids.eq(targets.data).tolist()
        M.host_update(st, outputs.numpy(), targets.numpy(), loss=loss, qids=qids)
        M.host_update(small, outputs.numpy(), targets.numpy(), loss=loss, qids=qids)
    acc = 0.0
    for v in valid_loss:
        acc = acc + v
    valid_acc = sum(int(c) for c in valid_corrects) / float(len(valid_corrects))
    qid_corrects = ["%d\t%d" % (a, b) for a, b in zip(valid_qids, valid_corrects)]
    assert st.valid_summary() == (valid_acc, acc / float(len(valid_corrects)), qid_corrects)
    assert small.rows == st.rows and small.correct == st.correct and small.ring_cursor == 10
    assert small.ring_dropped == st.rows - 10 and small.ring.tolist() == st.ring[:10].tolist()


def span_case(N, Li, seed):
    """answer (N, 5), softmaxed t_prob (N, 5, Li, 2), targets, ground-truth spans, image indices: random rows, and rows built for
    the edges -- no overlap, containment, IoU exactly 0.5 (prediction [0, 10] s against [0, 5] s), non-zero offsets
    (image_indices[0] % 6 in {0, 3, 5}), an all-zero t_prob row (the (0, 1) default)."""
    g = torch.Generator().manual_seed(seed)
    NA = 5
    answer = torch.randn(N, NA, generator=g)
    t_prob = torch.softmax(torch.randn(N, NA, Li, 2, generator=g) * 2, dim=2)
    targets = torch.randint(0, NA, (N,), generator=g)
    pred = answer.max(1)[1]
    targets[::2] = pred[::2]                                   # half the rows right
    gt = [[float(2 * torch.rand((), generator=g) * Li), 0.0] for _ in range(N)]
    for r in gt:
        r[1] = r[0] + float(torch.rand((), generator=g) * Li)
    img = [[int(torch.randint(0, 600, (1,), generator=g))] + [7] * 3 for _ in range(N)]

    def one_hot(n, s, e):
        t_prob[n, pred[n]] = 0.0
        t_prob[n, pred[n], s, 0] = 1.0
        t_prob[n, pred[n], e, 1] = 1.0

    if N >= 1 and Li >= 5:
        one_hot(0, 0, 4)
        gt[0], img[0][0] = [0.0, 5.0], 12                      # prediction [0, 10], ground truth [0, 5]: IoU exactly 0.5
    if N >= 3:
        t_prob[1, pred[1]] = 0.0                               # nothing positive: (0, 1) -> [0 + off, 4 + off]
        gt[1], img[1][0] = [100.0, 101.5], 3                   # offset 1.0; no overlap
        gt[2], img[2][0] = [-5.0, 5000.0], 5                   # offset 5 / 3; the prediction is contained
    if N >= 17 and Li >= 65:
        one_hot(3, 10, 64)
        gt[3], img[3][0] = [40.0, 60.0], 6                     # ground truth contained in the prediction [20, 130]
        one_hot(4, 2, 2)
        gt[4], img[4][0] = [4.0, 6.0], 0                       # identical: IoU 1
    return answer, t_prob, targets, gt, img


@pytest.mark.parametrize("N,Li", [(1, 1), (3, 2), (3, 65), (17, 65), (17, 300)])
def test_host_spans_is_the_writer_and_the_temporal_metrics(N, Li):
    from tvqaplus_amd.evaluation import PredictionWriter, compute_temporal_metrics
    answer, t_prob, targets, gt, img = span_case(N, Li, 100 * N + Li)
    qids = [50 + n for n in range(N)]
    w = PredictionWriter()
    w.add_batch(dict(answer=answer, t_scores=t_prob), qids, img)
    ref = compute_temporal_metrics(w.predictions["ts_answer"], {q: [gt[n], int(targets[n])] for n, q in enumerate(qids)})
    st = M.MeterState()
    rows = M.host_spans(st, answer.numpy(), t_prob.numpy(), targets.numpy(), gt, img, qids)
    assert [[list(v[0]), v[1]] for v in w.predictions["ts_answer"].values()] == \
        [[[int(s) * 2 + (i[0] % 6) / 3, (int(e) + 1) * 2 + (i[0] % 6) / 3], int(a)] for (s, e, a), i in zip(rows, img)]
    got = st.temporal_metrics()
    assert set(got) == set(ref) and st.span_rows == N and st.span_qids == qids
    for k in ref:
        if k == "miou":
            assert abs(got[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])
    if Li >= 5:
        assert st.recall_bins[4] >= 1                          # the IoU == 0.5 row sits in the 0.5 bin


def test_states_add_and_run_meter_refuses_the_host():
    from tvqaplus_amd._lib import StageHipError
    a, b = M.MeterState(ring_cap=1000), M.MeterState(ring_cap=1000)
    steps = _steps(13)
    for k, (x, t, cls, att, ts, qids) in enumerate(steps):
        M.host_update(a if k < 4 else b, x.numpy(), t.numpy(), cls, cls, att, ts, 0.1, 0.5, grad_norm=att, qids=qids)
    c = a + b
    assert c.i.tolist() == (a.i + b.i).tolist() and c.rows == sum(len(s[1]) for s in steps)
    assert c.loss_sum == a.loss_sum + b.loss_sum and c.grad_norm_max == max(a.grad_norm_max, b.grad_norm_max)
    assert c.ring.tolist() == a.ring.tolist() + b.ring.tolist() and c.qids == a.qids + b.qids
    assert len(c.valid_summary()[2]) == c.rows == c.ring_cursor and c.ring_cap == 2000
    with pytest.raises(StageHipError):
        M.RunMeter("cpu")
    with pytest.raises(StageHipError):
        M.RunMeter(torch.device("cpu"), ring_rows=4)
