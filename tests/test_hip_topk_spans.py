"""-m gpu: the multi-proposal head (max_num_proposal > 1).  The top-K span kernel (csrc/topk_spans.hip) against an fp64 brute-force
ranking, its ties, its agreement with the arg-max kernels; the pooling + classifier head with more than two proposals per example
against an fp64 autograd restatement built from the oracle's functions; the whole model; the loss with P = 4 N rows; the n-best
prediction file."""
import contextlib
import io
import json

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

NEG = -1e10
# 511 / 512 / 513: the edge where a thread gets a second pair of rows (it takes row i with row Li - 1 - i, i = tid, tid + 256, ...)
LIS = [1, 2, 3, 7, 64, 65, 255, 256, 257, 300, 511, 512, 513, 2048]
KS = [1, 2, 5, 8]
GAP = 1e-5          # a row enters the order comparison when the fp64 values of its ranks 0 .. K are separated by more than this
_REF = {}


def _scores(Li):
    """16 rows (3 at Li = 2048) of 3 * randn scores, seed 1234 + Li.  Row 0: trailing frames at -1e10 as mask_logits leaves them
    (Li >= 7); row 1: the maximum planted at (Li - 1, Li - 1); row 2: at (0, Li - 1); the rest as drawn."""
    R = 3 if Li == 2048 else 16
    g = torch.Generator().manual_seed(1234 + Li)
    x = torch.randn(R, Li, 2, generator=g) * 3
    if Li >= 7:
        x[0, Li - Li // 3:] = NEG
    x[1, Li - 1, :] = 25.0
    x[2, 0, 0] = 25.0
    x[2, Li - 1, 1] = 25.0
    return x


def _reference(Li, is_prob):
    """(input (R, Li, 2) fp32, fp64 ranking): the full Li x Li product on the host from the same fp32 numbers, the 9 best pairs of
    the upper triangle by (value descending, st * Li + ed ascending).  Computed once per (Li, is_prob)."""
    key = (Li, is_prob)
    if key not in _REF:
        x = _scores(Li)
        if is_prob:
            x = torch.softmax(x, dim=1)                  # fp32 probabilities: the kernel uses them as given
            p = x.double()
        else:
            p = torch.softmax(x.double(), dim=1)
        lower = torch.ones(Li, Li, dtype=torch.bool).tril(-1).view(-1)
        n = min(9, Li * (Li + 1) // 2)
        vals, idxs = [], []
        for r in range(x.shape[0]):
            prod = (p[r, :, 0].unsqueeze(1) * p[r, :, 1].unsqueeze(0)).reshape(-1)
            prod[lower] = -1.0
            v, i = torch.sort(prod, descending=True, stable=True)
            vals.append(v[:n].clone())
            idxs.append(i[:n].clone())
        _REF[key] = (x, torch.stack(vals), torch.stack(idxs))
    return _REF[key]


def _comparable(val, K):
    """rows whose fp64 values of ranks 0 .. K (as far as they exist) are pairwise separated by a relative gap above GAP"""
    v = val[:, :K + 1]
    if v.shape[1] < 2:
        return torch.ones(v.shape[0], dtype=torch.bool)
    return ((v[:, :-1] - v[:, 1:]) > GAP * v[:, :-1]).all(dim=1)


# ---- 1. the kernel against the fp64 ranking ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Li", LIS)
def test_topk_equals_fp64_brute_force(hip_device, Li):
    from tvqaplus_amd import groups
    for is_prob in (False, True):
        x, val, idx = _reference(Li, is_prob)
        pairs = Li * (Li + 1) // 2
        xd = x.to(hip_device)
        for K in KS:
            span, conf = groups.topk_spans(xd, K, is_prob=is_prob)
            span, conf = span.cpu().long(), conf.cpu()
            n = min(K, pairs)
            keep = _comparable(val, K)
            err = rel_err(conf[:, :n], val[:, :n].float())
            print("Li %d K %d is_prob %d: conf rel_err %.2e, rows left out %d, smallest gap %.2e" % (
                Li, K, is_prob, err, int((~keep).sum()),
                float(((val[:, :-1] - val[:, 1:]) / val[:, :-1])[:, :K].min()) if val.shape[1] > 1 else float("nan")))
            assert err <= 2e-4, (Li, K, is_prob, err)
            assert int((~keep).sum()) == 0, (Li, K, is_prob)              # the committed seeds leave no row out
            want = torch.stack([idx[:, :n] // Li, idx[:, :n] % Li], dim=2)
            assert torch.equal(span[:, :n][keep], want[keep]), (Li, K, is_prob)
            # ranks no pair fills: st = ed = -1, confidence 0
            assert bool((span[:, n:] == -1).all()) and bool((conf[:, n:] == 0).all()), (Li, K, is_prob)
            assert bool((span[:, :n, 0] <= span[:, :n, 1]).all()) and bool((span[:, :n] >= 0).all()) and bool((span[:, :n] < Li).all())
    # the planted maxima
    span, _ = groups.topk_spans(_scores(Li).to(hip_device), 1)
    assert span[1, 0].tolist() == [Li - 1, Li - 1] and span[2, 0].tolist() == [0, Li - 1]


# ---- 2. exact ties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Li", [3, 64, 257])
def test_exact_ties_come_in_ascending_flat_index(hip_device, Li):
    """Equal scores give bit-equal probabilities inside one kernel: every product ties, the order is ascending st * Li + ed --
    whichever threads hold the pairs (Li = 257: thread 0 holds rows 0 and 256, thread 1 rows 1 and 255)."""
    from tvqaplus_amd import groups
    x = torch.full((2, Li, 2), 0.5, device=hip_device)
    pairs = [(i, j) for i in range(Li) for j in range(i, Li)][:8]
    pairs += [(-1, -1)] * (8 - len(pairs))
    a = groups.topk_spans(x, 8)
    b = groups.topk_spans(x, 8)
    assert a[0][0].tolist() == [list(p) for p in pairs] and a[0][1].tolist() == a[0][0].tolist()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c = groups.topk_spans(torch.full((2, Li, 2), 1.0 / Li, device=hip_device), 8, is_prob=True)
    assert torch.equal(c[0], a[0])


# ---- 3. rank 0 is the arg-max kernels' span ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Li", [5, 300])
def test_rank_0_has_the_bits_of_the_arg_max_kernels(hip_device, Li):
    from tvqaplus_amd import groups
    g = torch.Generator().manual_seed(77 + Li)
    N, NA, D = 6, 5, 32
    t = (torch.randn(N, NA, Li, 2, generator=g) * 3)
    t[1, :, Li - 2:] = NEG
    t = t.to(hip_device)
    target = torch.randint(0, NA, (N,), generator=g).to(hip_device)
    target[2] = 7                                                            # out of range: clamped as stage_gt_spans does
    st = torch.randint(0, Li, (N,), generator=g).to(hip_device)
    ed = torch.randint(0, Li, (N,), generator=g).to(hip_device)
    one = groups.gt_spans(t, target, st, ed)
    k1 = groups.gt_spans_topk(t, target, st, ed, 1)
    k5 = groups.gt_spans_topk(t, target, st, ed, 5)
    assert one.shape == k1.shape == (6, N) and k5.shape == (18, N)
    assert torch.equal(one.view(torch.int32), k1.view(torch.int32))
    assert torch.equal(one[:3].view(torch.int32), k5[:3].view(torch.int32)) and torch.equal(one[3:].view(torch.int32), k5[15:].view(torch.int32))
    # ... and of the evaluation head's span search on every candidate row
    first = torch.randn(N * NA, Li, D, generator=g).to(hip_device)
    mask = torch.ones(N * NA, Li, device=hip_device)
    params = [torch.ones(2 * D, device=hip_device), torch.zeros(2 * D, device=hip_device), torch.randn(1, 2 * D, generator=g).to(hip_device),
              torch.zeros(1, device=hip_device)]
    _, span, conf = groups.eval_head(first, mask, t.view(N * NA, Li, 2), 3, True, params)
    span3, conf3 = groups.topk_spans(t.view(N * NA, Li, 2), 3)
    assert torch.equal(span3[:, 0], span) and torch.equal(conf3[:, 0].view(torch.int32), conf.view(torch.int32))


# ---- 4. the head in isolation -----------------------------------------------------------------------------------------------------
def _head_inputs():
    """N = 4, NA = 5, Li = 12, D = 128.  The ground-truth candidate's scores are log-probabilities peaked so that (prob_thd 0.01,
    IoU 0.5, k = 3): example 0 keeps none of its predicted spans (they lie away from the label), example 1 one (ranks 1, 2 fall below the
    threshold), example 2 all three, example 3 is random with two masked trailing frames."""
    g = torch.Generator().manual_seed(31)
    N, NA, Li, D = 4, 5, 12, 128
    t = torch.randn(N, NA, Li, 2, generator=g) * 2
    targets = torch.tensor([1, 4, 0, 2])
    lab_st, lab_ed = torch.tensor([8, 4, 3, 2]), torch.tensor([10, 7, 8, 6])

    def peaked(main):                       # {frame: probability}, the rest shared out, then a jitter that breaks every tie
        p = torch.full((Li,), (1.0 - sum(main.values())) / (Li - len(main)))
        for i, v in main.items():
            p[i] = v
        return torch.log(p) + 0.01 * torch.randn(Li, generator=g)
    t[0, 1, :, 0], t[0, 1, :, 1] = peaked({1: 0.9}), peaked({2: 0.6, 3: 0.3})
    t[1, 4, :, 0], t[1, 4, :, 1] = peaked({4: 0.97}), peaked({7: 0.97})
    t[2, 0, :, 0], t[2, 0, :, 1] = peaked({3: 0.5, 4: 0.3}), peaked({8: 0.6, 7: 0.3})
    frame_mask = torch.ones(N, Li)
    frame_mask[3, Li - 2:] = 0
    t = t * frame_mask.view(N, 1, Li, 1) + (1 - frame_mask.view(N, 1, Li, 1)) * NEG
    first = torch.randn(N, NA, Li, D, generator=g)
    mx_mask = frame_mask.view(N, 1, Li, 1).expand(N, NA, Li, 1).clone()
    return first, mx_mask, t, targets, dict(st=lab_st, ed=lab_ed)


def _head_reference(first, mx_mask, t, targets, ts, params, k, extra):
    """fp64 autograd restatement from the oracle's functions (model/stage.py:408-438, 526-536)."""
    from oracle import stage_oracle as O
    N, NA, Li, D = first.shape
    ca = torch.softmax(t[torch.arange(N), targets].double(), dim=1)
    pred = O.best_spans(ca[:, :, 0], ca[:, :, 1], top_n=k, prob_thd=0.01)
    masked = O.mask_logits(first, mx_mask.double())
    loc, glo, tgt, counts = [], [], [], []
    for n in range(N):
        gt = (int(ts["st"][n]), int(ts["ed"][n]) + 1)
        spans = [gt] + [(s, e + 1) for (s, e, _c) in pred[n] if O.temporal_iou((s, e + 1), gt) >= 0.5]
        counts.append(len(spans))
        for sp in spans:
            s, e = O.expand_span(sp, extra)
            loc.append(masked[n, :, s:e].max(dim=1)[0])
            glo.append(masked[n].max(dim=1)[0])
            tgt.append(int(targets[n]))
    pooled = torch.cat([torch.stack(loc), torch.stack(glo)], dim=-1)
    y = F.layer_norm(pooled, (2 * D,), params[0], params[1], 1e-5)
    return F.linear(y, params[2], params[3]).squeeze(2), tgt, counts


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("route", ["grouped", "per-op", "per-op sharded"])
def test_head_proposals_against_fp64(hip_device, route, k):
    """``per-op sharded``: the span table from ``gt_scores_fn``'s rows (candidate-sharded batches, parallel.CandidateLayout.gt_scores)."""
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    extra = 3
    gt_scores_fn = (lambda t, tg: t[torch.arange(len(tg), device=tg.device), tg]) if route == "per-op sharded" else None
    torch.manual_seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(hsz=128, add_local=True, dropout=0.0, max_num_proposal=k)).to(hip_device).train()
    cl = model.classifier
    with torch.no_grad():
        for p in cl.parameters():
            p.add_(0.1 * torch.randn_like(p))
    plist = [cl.conv[0].weight, cl.conv[0].bias, cl.conv[2].weight, cl.conv[2].bias]
    first, mx_mask, t, targets, ts = _head_inputs()
    f64 = first.double().requires_grad_()
    p64 = [p.detach().cpu().double().requires_grad_() for p in plist]
    ref, ref_tgt, counts = _head_reference(f64, mx_mask, t, targets, ts, p64, k, extra)
    if k == 3:
        assert counts[:3] == [1, 2, 4] and max(counts) >= 3    # a stride-2 inverse table would lose rows of example 2
    else:
        assert counts == [1, 2, 2, 1]                          # one example with a single row, two with a kept proposal
    w = torch.randn(ref.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (ref * w).sum().backward()

    dev = lambda v: v.to(hip_device)
    tsd = {a: dev(b) for a, b in ts.items()}
    runs = []
    for _ in range(2):
        for p in plist:
            p.grad = None
        fd = dev(first).requires_grad_()
        if route == "grouped":
            logits, tg = model._proposals_grouped(fd, dev(mx_mask), dev(t), dev(targets), tsd, extra)
        else:
            pooled, tg = model.get_proposals(fd, dev(mx_mask), dev(t), dev(targets), tsd, extra_span_length=extra,
                                             gt_scores_fn=gt_scores_fn)
            logits, _ = model._linear_wrapper(pooled.reshape(-1, pooled.shape[-1]), cl)
        logits = logits.view(-1, 5)
        (logits * dev(w).float()).sum().backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), tg.clone(), fd.grad.clone(), [p.grad.clone() for p in plist]))
    a, b = runs
    assert a[1].tolist() == ref_tgt                                        # targets and row order
    errs = dict(logits=rel_err(a[0], ref.detach()), d_first=rel_err(a[2], f64.grad))
    for name, got, want in zip(("ln.w", "ln.b", "fc.w", "fc.b"), a[3], p64):
        errs[name] = rel_err(got, want.grad)
    print("head k = %d (%s): %s" % (k, route, ", ".join("%s %.2e" % kv for kv in errs.items())))
    for name, e in errs.items():
        assert e <= 2e-4, (name, e)
    # two identical steps are bit-equal (the per-op path sums an example's proposals in slot order, not by atomics)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)


# ---- 5. the whole model -----------------------------------------------------------------------------------------------------------
SMALL = (dict(hsz=32, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.2), dict(N=2, Li=5, Lr=7, Lw=9, Lqa=6, wd_size=48, vfeat_size=40))


def _build(kw, seed=3):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(**kw))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model.use_ragged = False
    return model


def _step(model, batch, use_groups):
    model.use_groups = use_groups
    model._seed_state = 12345
    torch.manual_seed(11)
    for p in model.parameters():
        p.grad = None
    (out, targets), _, _, t_loss, t_scores, _ = model.forward_main(batch)
    loss = F.cross_entropy(out, targets, reduction="sum") * (len(batch.qid) / len(targets)) + 0.5 * t_loss
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return out.detach().clone(), targets.clone(), t_scores.detach().clone(), loss.detach().clone(), grads


def test_model_with_three_proposals(hip_device, monkeypatch):
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import proposal_rows
    from tvqaplus_amd.synth import make_batch
    monkeypatch.setenv("STAGE_NO_CAT3_FUSED", "1")        # same kernels on both paths, as tests/test_hip_groups.py compares them
    kw, shape = SMALL
    batch = make_batch(seed=5, **shape).to(hip_device)
    base = _step(_build(kw).to(hip_device).train(), batch, True)
    model = _build(dict(kw, max_num_proposal=3)).to(hip_device).train()
    o1, tg1, t1, l1, g1 = _step(model, batch, False)
    o2, tg2, t2, l2, g2 = _step(model, batch, True)
    # the row count is the host loop's P on the spans of these very scores
    host = groups.gt_spans_topk(t2, batch.target, batch.ts_label["st"], batch.ts_label["ed"], 3).cpu().tolist()
    src, _, _, tgt = proposal_rows(host, shape["N"], 3, 0.5, 0.01, model.extra_span_length)
    assert o2.shape == (len(src), 5) and tg2.tolist() == tgt and o1.shape == o2.shape and tg1.tolist() == tgt
    assert len(src) >= base[0].shape[0]
    print("proposals at k = 1 / k = 3: %d / %d" % (base[0].shape[0], len(src)))
    # grouped against per-op at the tolerances of tests/test_hip_groups.py::test_group_path_equals_per_op_path
    assert torch.equal(o1, o2) and torch.equal(t1, t2), (float((o1 - o2).abs().max()), float((t1 - t2).abs().max()))
    assert abs(float(l1) - float(l2)) <= 2e-6 * (1 + abs(float(l1)))
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None) == (base[4][k] is None), k
        if g1[k] is None:
            continue
        assert bool(torch.isfinite(g1[k]).all()) and bool(torch.isfinite(g2[k]).all()), k
        scale = float(g1[k].abs().max()) + 1e-12
        assert float((g1[k] - g2[k]).abs().max()) <= 2e-5 * scale + 1e-7, (k, float((g1[k] - g2[k]).abs().max()), scale)


@pytest.mark.parametrize("use_groups", [True, False])
def test_max_num_proposal_1_is_the_model_without_the_option(hip_device, use_groups):
    from tvqaplus_amd.synth import make_batch
    kw, shape = SMALL
    batch = make_batch(seed=5, **shape).to(hip_device)
    a = _step(_build(kw).to(hip_device).train(), batch, use_groups)
    b = _step(_build(dict(kw, max_num_proposal=1)).to(hip_device).train(), batch, use_groups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for k in a[4]:
        assert (a[4][k] is None) == (b[4][k] is None) and (a[4][k] is None or torch.equal(a[4][k], b[4][k])), k


# ---- 6. the loss with more than two rows per example ------------------------------------------------------------------------------
def test_loss_with_four_rows_per_example(hip_device):
    from tvqaplus_amd import meter as M
    from tvqaplus_amd.stage import reference_loss
    N, C = 16, 5
    P = 4 * N
    g = torch.Generator().manual_seed(3)
    logits = (3.0 * torch.randn(P, C, generator=g)).to(hip_device)
    targets = torch.randint(0, C, (P,), generator=g).to(hip_device)
    att, ts = (torch.rand((), generator=g) * 4).to(hip_device), (torch.rand((), generator=g) * 9).to(hip_device)
    m = M.RunMeter(hip_device, ring_rows=P)
    m.reset()
    x0 = logits.clone().requires_grad_()
    eager = F.cross_entropy(x0, targets, reduction="sum") * (N / P) + 0.1 * att + 0.5 * ts
    eager.backward()
    for meter in (None, m):
        x = logits.clone().requires_grad_()
        loss = reference_loss(x, targets, att, ts, N, 0.1, 0.5, meter=meter)
        loss.backward()
        assert abs(float(loss) - float(eager)) <= 1e-6 * (1 + abs(float(eager))), (float(loss), float(eager))
        assert float((x.grad - x0.grad).abs().max()) <= 1e-6 * (1 + float(x0.grad.abs().max()))
    s = m.read()
    assert s.steps == 1 and s.rows == P and s.ring_dropped == 0
    assert s.correct == int((logits.max(1)[1] == targets).sum())
    assert abs(s.cls_sum - float(F.cross_entropy(logits, targets, reduction="sum") * (N / P))) <= 1e-6 * (1 + abs(s.cls_sum))


# ---- 7. the n-best prediction file ------------------------------------------------------------------------------------------------
def test_prediction_writer_n_best_on_device_outputs(hip_device, tmp_path):
    from tvqaplus_amd.evaluation import PredictionWriter, find_max_triples_batch
    g = torch.Generator().manual_seed(8)
    N, NA, Li = 6, 5, 40
    answer = torch.randn(N, NA, generator=g)
    t_prob = torch.softmax(torch.randn(N, NA, Li, 2, generator=g) * 2, dim=2)
    qids, img = list(range(100, 100 + N)), [[n + 2, n + 8] for n in range(N)]
    out_dev = dict(answer=answer.to(hip_device), t_scores=t_prob.to(hip_device))
    blobs = []
    for i, w in enumerate((PredictionWriter(), PredictionWriter(n_best=1), PredictionWriter(n_best=3))):
        w.add_batch(out_dev, qids, img)
        w.save(str(tmp_path / ("p%d.json" % i)))
        blobs.append(open(str(tmp_path / ("p%d.json" % i)), "rb").read())
    assert blobs[0] == blobs[1]                                            # n_best = 1 writes today's bytes
    rec = json.loads(blobs[2])
    assert rec["ts_answer"] == json.loads(blobs[0])["ts_answer"]
    pred = answer.max(1)[1]
    span, conf = find_max_triples_batch(t_prob[torch.arange(N), pred][:, :, 0], t_prob[torch.arange(N), pred][:, :, 1], 3)   # host copy
    for n, qid in enumerate(qids):
        nb = rec["ts_nbest"][str(qid)]
        off = (img[n][0] % 6) / 3
        assert nb[0][:2] == rec["ts_answer"][str(qid)][0]
        assert [v[:2] for v in nb] == [[s * 2 + off, (e + 1) * 2 + off] for s, e in span[n].tolist()]
        assert max(abs(v[2] - c) for v, c in zip(nb, conf[n].tolist())) <= 1e-6
