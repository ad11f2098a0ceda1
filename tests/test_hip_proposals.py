"""-m gpu: span proposals chosen on the device (opt.device_proposals).  The decision kernel (csrc/proposals.hip) against its
specification ``stage.proposal_meta_host`` byte by byte on constructed span tables; the pooling + classifier head at the fixed
capacity against the read-back path and against an fp64 autograd restatement built from the oracle's functions; the whole model
with the option against the model without it, and that the step never reaches the read-back."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from test_hip_topk_spans import _build, _head_inputs, _head_reference

pytestmark = pytest.mark.gpu

LO = np.float32(0.01)                        # below the double 0.01: rejected
HI = np.nextafter(LO, np.float32(1))         # the next float up: kept


# ---- 1. the kernel against the specification ---------------------------------------------------------------------------------------
def _table(N, k, variant, Li=24, seed=0):
    """(3k + 3, N) float32, built on the host.  Example n: label [gs, ge] of 1 .. 5 frames; its ranks by n % 4 ("mixed": 0 none kept,
    1 the even ranks, 2 all k, 3 drawn), all kept ("full": P == Pmax) or none ("none": P == N).  A kept rank covers the label's span
    (+ one frame for odd ranks: IoU L / (L + 1) >= 0.5); a rejected one by turns has a low confidence, lies behind the label's span
    (IoU 0) or is the empty rank (-1, -1, 0) of the top-K kernel."""
    rng = np.random.RandomState(1000 * N + 10 * k + seed)
    t = np.zeros((3 * k + 3, N), dtype=np.float32)
    for n in range(N):
        gs = (7 * n) % (Li - 6)
        ge = gs + n % 5
        t[3 * k:, n] = gs, ge, n % 5
        mode = {"full": 2, "none": 0}.get(variant, n % 4)
        for j in range(k):
            keep = (mode == 2) or (mode == 1 and j % 2 == 0) or (mode == 3 and rng.rand() < 0.5)
            if keep:
                t[3 * j:3 * j + 3, n] = gs, ge + j % 2, 0.5 / (j + 1)
            else:
                t[3 * j:3 * j + 3, n] = [(gs, ge, 0.005), (ge + 2, ge + 3, 0.4), (-1, -1, 0)][(n + j) % 3]
    return t


def _against_spec(table, k, iou, thd, extra, dev):
    """device (meta, count, scale) of ``table`` equal the specification's bytes; returns (meta on the host, P)"""
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import proposal_meta_host
    N = table.shape[1]
    want, P = proposal_meta_host(table.tolist(), N, k, iou, thd, extra)
    meta, count, scale = groups.proposal_meta(torch.from_numpy(table).to(dev), k, iou, thd, extra)
    assert meta.dtype == torch.int32 and count.dtype == torch.int32 and scale.dtype == torch.float32
    assert count.dim() == 0 and scale.dim() == 0 and meta.is_cuda and count.is_cuda and scale.is_cuda
    got = meta.cpu()
    assert torch.equal(got, torch.from_numpy(want)), (N, k, (got != torch.from_numpy(want)).nonzero().view(-1)[:8].tolist())
    assert torch.equal(count.cpu(), torch.tensor(P, dtype=torch.int32))
    want_scale = torch.from_numpy(np.array(np.float32(float(N) / P)))
    assert torch.equal(scale.cpu().view(torch.int32), want_scale.view(torch.int32)), (float(scale), float(want_scale))
    return want, P


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 3, 255, 256, 257, 600])
def test_kernel_equals_the_specification(hip_device, N, k):
    slots = k + 1
    for variant in ("mixed", "full", "none"):
        table = _table(N, k, variant)
        meta, P = _against_spec(table, k, 0.5, 0.01, 3, hip_device)
        counts = (meta[3 * slots * N:4 * slots * N].reshape(N, slots) >= 0).sum(1)
        if variant == "full":
            assert P == slots * N                                           # every slot full: no padding row
        elif variant == "none":
            assert P == N
        elif N >= 3:
            assert counts[0] == 1 and counts[2] == slots and N < P < slots * N
            if k >= 2:
                assert 1 < counts[1] < slots
    # other thresholds and no extra frames on the same mixed table
    _against_spec(_table(N, k, "mixed", seed=1), k, 0.7, 0.1, 0, hip_device)


def test_planted_decisions(hip_device):
    k, Li = 2, 12
    #        ex 0            1              2              3               4                5
    cols = [
        # conf = np.float32(0.01) rejected, its next float up kept (same span as the label)
        dict(r0=(4, 5, LO), r1=(4, 5, HI), lab=(4, 5), kept=1),
        # IoU exactly 0.5: inter 1 / union 2, kept; one unit below (inter 1 / union 3): rejected
        dict(r0=(4, 4, 0.5), r1=(4, 4, 0.5), lab=(4, 5), kept=2),
        dict(r0=(4, 4, 0.5), r1=(5, 6, 0.5), lab=(4, 6), kept=1),          # 1 / 3 rejected, 2 / 3 kept
        # the top-K kernel's empty rank, and a start of -1 under a high confidence: skipped
        dict(r0=(-1, -1, 0.0), r1=(-1, 3, 0.9), lab=(2, 3), kept=0),
        # label windows at both ends: st = 0; ed = Li - 1 with extra = 3 (the upper end stays unclamped: Li + 3)
        dict(r0=(0, 0, 0.5), r1=(0, 1, 0.5), lab=(0, 0), kept=2),
        dict(r0=(Li - 1, Li - 1, 0.5), r1=(0, 0, 0.5), lab=(Li - 1, Li - 1), kept=1),
    ]
    N = len(cols)
    t = np.zeros((3 * k + 3, N), dtype=np.float32)
    for n, c in enumerate(cols):
        t[0:3, n], t[3:6, n], t[6:9, n] = c["r0"], c["r1"], c["lab"] + (n % 5,)
    meta, P = _against_spec(t, k, 0.5, 0.01, 3, hip_device)
    Pmax = 3 * N
    counts = (meta[3 * Pmax:4 * Pmax].reshape(N, 3) >= 0).sum(1)
    assert counts.tolist() == [1 + c["kept"] for c in cols]
    win = meta[Pmax:3 * Pmax].reshape(Pmax, 2)
    inv = meta[3 * Pmax:4 * Pmax].reshape(N, 3)
    assert win[inv[4, 0]].tolist() == [0, 4] and win[inv[5, 0]].tolist() == [Li - 4, Li + 3]
    # IoU exactly at 0.3: inter 3 / union 10 kept, inter 2 / union 10 rejected
    t = np.array([[0, 0], [2, 1], [0.5, 0.5], [0, 0], [9, 9], [1, 2]], dtype=np.float32)
    meta, P = _against_spec(t, 1, 0.3, 0.01, 3, hip_device)
    assert P == 3 and meta[3 * 4:4 * 4].tolist() == [0, 1, 2, -1]


def test_nan_confidence_and_nan_start_make_the_rank_absent(hip_device):
    """No value of the table becomes an index: the call returns 0 (groups.proposal_meta raises otherwise), the NaN ranks are absent
    and the others decided as ever."""
    k = 2
    t = _table(5, k, "full")
    t[2, 1] = np.nan              # rank 0 of example 1: NaN confidence
    t[3, 2] = np.nan              # rank 1 of example 2: NaN start
    meta, P = _against_spec(t, k, 0.5, 0.01, 3, hip_device)
    Pmax = 3 * 5
    assert (meta[3 * Pmax:4 * Pmax].reshape(5, 3) >= 0).sum(1).tolist() == [3, 2, 2, 3, 3] and P == 13
    torch.cuda.synchronize()


def test_from_real_scores(hip_device):
    """The table of gt_spans_topk itself, used as it is: the device rows equal proposal_rows on the read-back of that table."""
    from tvqaplus_amd import groups
    from tvqaplus_amd.stage import proposal_rows
    _, _, t, targets, ts = _head_inputs()
    dev = lambda v: v.to(hip_device)
    N, k = 4, 3
    spans = groups.gt_spans_topk(dev(t), dev(targets), dev(ts["st"]), dev(ts["ed"]), k)
    meta, count, scale = groups.proposal_meta(spans, k, 0.5, 0.01, 3)
    src, wins, inv, tgt = proposal_rows(spans.cpu().tolist(), N, k, 0.5, 0.01, 3)
    P, Pmax = len(src), (k + 1) * N
    m = meta.cpu().tolist()
    assert int(count) == P and m[:P] == src and m[Pmax:Pmax + 2 * P] == wins and m[3 * Pmax:4 * Pmax] == inv and m[4 * Pmax:4 * Pmax + P] == tgt
    counts = [sum(1 for v in inv[(k + 1) * n:(k + 1) * (n + 1)] if v >= 0) for n in range(N)]
    assert counts[:3] == [1, 2, 4]
    # the top-K kernel's empty ranks (Li (Li + 1) / 2 < k): skipped, never an index
    for Li, kk in ((1, 2), (2, 8)):
        g = torch.Generator().manual_seed(Li)
        tt = dev(torch.randn(3, 5, Li, 2, generator=g))
        tg, st, ed = dev(torch.tensor([0, 3, 4])), dev(torch.zeros(3, dtype=torch.long)), dev(torch.full((3,), Li - 1))
        sp = groups.gt_spans_topk(tt, tg, st, ed, kk)
        host = sp.cpu()
        assert bool((host[3 * (Li * (Li + 1) // 2)] == -1).all())         # the first rank no pair fills
        meta, count, _ = groups.proposal_meta(sp, kk, 0.5, 0.01, 3)
        src, wins, inv, tgt = proposal_rows(host.tolist(), 3, kk, 0.5, 0.01, 3)
        P, Pmax = len(src), (kk + 1) * 3
        m = meta.cpu().tolist()
        assert int(count) == P and m[:P] == src and m[Pmax:Pmax + 2 * P] == wins and m[3 * Pmax:4 * Pmax] == inv


# ---- 2. the head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("k", [3, 1])
def test_head_on_device_against_read_back_and_fp64(hip_device, k, p_drop):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    extra = 3
    torch.manual_seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(hsz=128, add_local=True, dropout=p_drop, max_num_proposal=k)).to(hip_device).train()
    cl = model.classifier
    with torch.no_grad():
        for p in cl.parameters():
            p.add_(0.1 * torch.randn_like(p))
    plist = [cl.conv[0].weight, cl.conv[0].bias, cl.conv[2].weight, cl.conv[2].bias]
    first, mx_mask, t, targets, ts = _head_inputs()
    N = first.shape[0]
    dev = lambda v: v.to(hip_device)
    tsd = {a: dev(b) for a, b in ts.items()}
    wgen = torch.Generator().manual_seed(4)
    w_all = torch.randn((k + 1) * N, 5, generator=wgen, dtype=torch.float64)

    def run(fn):
        model._seed_state = 777
        for p in plist:
            p.grad = None
        fd = dev(first).requires_grad_()
        logits, tg = fn(fd, dev(mx_mask), dev(t), dev(targets), tsd, extra)
        logits = logits.view(-1, 5)
        P = int((tg >= 0).sum())
        (logits[:P] * dev(w_all[:P]).float()).sum().backward()             # rows past P: no gradient, as under the loss
        torch.cuda.synchronize()
        return logits.detach().clone(), tg.clone(), fd.grad.clone(), [p.grad.clone() for p in plist], P

    rb = run(model._proposals_grouped)
    d1 = run(model._proposals_on_device)
    d2 = run(model._proposals_on_device)
    P, Pmax = rb[4], (k + 1) * N
    info = model.last_proposals
    assert rb[0].shape == (P, 5) and d1[0].shape == (Pmax, 5) and d1[1].shape == (Pmax,) and d1[1].dtype == torch.int64
    assert info.on_device and info.capacity == Pmax and int(info.count) == P == d1[4]
    assert torch.equal(info.scale.cpu().view(torch.int32), torch.from_numpy(np.array(np.float32(float(N) / P))).view(torch.int32))
    # rows [0, P): the read-back path's rows at the same indices, under the same dropout words
    assert torch.equal(d1[1][:P], rb[1]) and bool((d1[1][P:] == -100).all())
    assert torch.equal(d1[0][:P], rb[0]), float((d1[0][:P] - rb[0]).abs().max())
    assert bool(torch.isfinite(d1[0]).all())
    # gradients against the read-back path: the same arithmetic, possibly another summation order over the rows
    names = ("d_first", "ln.w", "ln.b", "fc.w", "fc.b")
    for name, a, b in zip(names, [d1[2]] + d1[3], [rb[2]] + rb[3]):
        assert bool(torch.isfinite(a).all()), name
        scale = float(b.abs().max()) + 1e-12
        diff = float((a - b).abs().max())
        print("k = %d p = %.1f %s: |device - read-back| %.2e (scale %.2e)" % (k, p_drop, name, diff, scale))
        assert diff <= 2e-5 * scale + 1e-7, (name, diff, scale)
    # two identical device-path steps are bit-equal
    assert torch.equal(d1[0], d2[0]) and torch.equal(d1[1], d2[1]) and torch.equal(d1[2], d2[2])
    for a, b in zip(d1[3], d2[3]):
        assert torch.equal(a, b)
    if p_drop == 0.0:
        f64 = first.double().requires_grad_()
        p64 = [p.detach().cpu().double().requires_grad_() for p in plist]
        ref, ref_tgt, _ = _head_reference(f64, mx_mask, t, targets, ts, p64, k, extra)
        assert ref.shape[0] == P and d1[1][:P].tolist() == ref_tgt
        (ref * w_all[:P]).sum().backward()
        errs = dict(logits=rel_err(d1[0][:P], ref.detach()), d_first=rel_err(d1[2], f64.grad))
        for name, got, want in zip(names[1:], d1[3], p64):
            errs[name] = rel_err(got, want.grad)
        print("device head k = %d against fp64: %s" % (k, ", ".join("%s %.2e" % kv for kv in errs.items())))
        for name, e in errs.items():
            assert e <= 2e-4, (name, e)


# ---- 3. the whole model -----------------------------------------------------------------------------------------------------------
SMALL = (dict(hsz=32, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.2), dict(N=2, Li=5, Lr=7, Lw=9, Lqa=6, wd_size=48, vfeat_size=40))


def _step(model, batch, use_groups=True, backward=True):
    """one training step with the loss line of INTEGRATION.md section 2: reference_loss(..., scale=model.last_proposals.scale)"""
    from tvqaplus_amd.stage import reference_loss
    model.use_groups = use_groups
    model._seed_state = 12345
    torch.manual_seed(11)
    for p in model.parameters():
        p.grad = None
    (out, targets), att_loss, _, t_loss, t_scores, _ = model.forward_main(batch)
    loss = reference_loss(out, targets, att_loss, t_loss, len(batch.qid), scale=model.last_proposals.scale)
    if backward:
        loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return out.detach().clone(), targets.clone(), t_scores.detach().clone(), loss.detach().clone(), grads


@pytest.mark.parametrize("k", [1, 3])
def test_model_step_with_device_proposals(hip_device, monkeypatch, k):
    from tvqaplus_amd import stage as S
    from tvqaplus_amd.stage import reference_loss
    from tvqaplus_amd.synth import make_batch
    kw, shape = SMALL
    N = shape["N"]
    batch = make_batch(seed=5, **shape).to(hip_device)
    base_model = _build(dict(kw, max_num_proposal=k)).to(hip_device).train()
    o1, tg1, t1, l1, g1 = _step(base_model, batch)
    P = o1.shape[0]
    assert not base_model.last_proposals.on_device and base_model.last_proposals.capacity == P
    assert int(base_model.last_proposals.count) == P

    model = _build(dict(kw, max_num_proposal=k, device_proposals=True)).to(hip_device).train()
    assert model.device_proposals

    def never(*a, **kws):
        raise AssertionError("the device path reached the read-back")
    monkeypatch.setattr(S.STAGE, "_read_spans", never)
    monkeypatch.setattr(S, "proposal_rows", never)
    o2, tg2, t2, l2, g2 = _step(model, batch)
    monkeypatch.undo()
    info = model.last_proposals
    Pmax = (k + 1) * N
    assert o2.shape == (Pmax, 5) and tg2.shape == (Pmax,) and info.on_device and info.capacity == Pmax
    assert int(info.count) == P
    assert torch.equal(info.scale.cpu().view(torch.int32), torch.from_numpy(np.array(np.float32(N / P))).view(torch.int32))
    assert torch.equal(o2[:P], o1) and torch.equal(t1, t2), float((o2[:P] - o1).abs().max())
    assert torch.equal(tg2[:P], tg1) and bool((tg2[P:] == -100).all()) and bool(torch.isfinite(o2).all())
    print("k = %d: P = %d of %d, loss %.6f / %.6f" % (k, P, Pmax, float(l1), float(l2)))
    assert abs(float(l1) - float(l2)) <= 2e-6 * (1 + abs(float(l1)))
    for name in g1:
        assert (g1[name] is None) == (g2[name] is None), name
        if g1[name] is None:
            continue
        assert bool(torch.isfinite(g2[name]).all()), name
        scale = float(g1[name].abs().max()) + 1e-12
        diff = float((g1[name] - g2[name]).abs().max())
        assert diff <= 2e-5 * scale + 1e-7, (name, diff, scale)
    # the eager line with the default ignore_index is the same loss
    x = o2.clone()
    eager = F.cross_entropy(x, tg2, reduction="sum") * info.scale
    fused = reference_loss(x, tg2, 0, 0, N, scale=info.scale)
    assert abs(float(eager) - float(fused)) <= 2e-6 * abs(float(fused)), (float(eager), float(fused))


def test_output_shape_does_not_depend_on_the_proposal_count(hip_device):
    """Two batches whose proposal counts differ (labels on the predicted spans: every slot full; labels away from them: none kept)
    return the same (slots * N, 5)."""
    from tvqaplus_amd import groups
    from tvqaplus_amd.synth import make_batch
    kw, shape = SMALL
    N, Li = shape["N"], shape["Li"]
    batch = make_batch(seed=5, **shape).to(hip_device)
    model = _build(dict(kw, device_proposals=True)).to(hip_device).train()
    _, _, t_scores, _, _ = _step(model, batch, backward=False)
    pred = groups.gt_spans(t_scores, batch.target, batch.ts_label["st"], batch.ts_label["ed"]).cpu()
    st, ed = pred[0].long(), pred[1].long()
    far = [(Li - 1, Li - 1) if e < Li - 1 else (0, 0) for s, e in zip(st.tolist(), ed.tolist())]     # IoU < 0.5 with [s, e]
    counts = []
    for lab_st, lab_ed in ((st, ed), (torch.tensor([f[0] for f in far]), torch.tensor([f[1] for f in far]))):
        batch.ts_label = dict(st=lab_st.to(hip_device), ed=lab_ed.to(hip_device))
        out, tg, t2, _, _ = _step(model, batch, backward=False)
        assert torch.equal(t2, t_scores)                                    # the labels do not enter the scores
        assert out.shape == (2 * N, 5) and tg.shape == (2 * N,)
        counts.append(int(model.last_proposals.count))
        assert int((tg >= 0).sum()) == counts[-1]
    assert counts == [2 * N, N]


@pytest.mark.parametrize("use_groups", [True, False])
def test_option_off_is_the_model_without_the_attribute(hip_device, use_groups):
    from tvqaplus_amd.synth import make_batch
    kw, shape = SMALL
    batch = make_batch(seed=5, **shape).to(hip_device)
    a = _step(_build(kw).to(hip_device).train(), batch, use_groups)
    b = _step(_build(dict(kw, device_proposals=False)).to(hip_device).train(), batch, use_groups)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    for name in a[4]:
        assert (a[4][name] is None) == (b[4][name] is None) and (a[4][name] is None or torch.equal(a[4][name], b[4][name])), name


def test_per_op_path_keeps_the_read_back(hip_device):
    """use_groups = False with the option on: compact rows, and last_proposals filled from the host's numbers."""
    from tvqaplus_amd.synth import make_batch
    kw, shape = SMALL
    N = shape["N"]
    batch = make_batch(seed=5, **shape).to(hip_device)
    a = _step(_build(kw).to(hip_device).train(), batch, False)
    model = _build(dict(kw, device_proposals=True)).to(hip_device).train()
    b = _step(model, batch, False)
    info = model.last_proposals
    P = a[0].shape[0]
    assert b[0].shape == (P, 5) and bool((b[1] >= 0).all()) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert info.on_device is False and info.capacity == P and int(info.count) == P and info.count.is_cuda and info.scale.is_cuda
    assert torch.equal(info.scale.cpu().view(torch.int32), torch.from_numpy(np.array(np.float32(N / P))).view(torch.int32))
    assert abs(float(a[3]) - float(b[3])) <= 2e-6 * (1 + abs(float(a[3])))
