"""-m gpu: the row kernels of csrc/score_rows.hip (box prediction, rank order of a row's negatives) against numpy's stable sorts,
and the two consumers built on them (att_host.get_att_prediction, hard-negative get_att_loss) against the host routes they
replace: integer / bit equality throughout, the reference fixtures of tests/golden/att_*.npz, and the whole model."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import Fixture, rel_err
from test_hip_stage import TOL
from tvqaplus_amd import att_host, groups

pytestmark = pytest.mark.gpu
THD = 0.2
HARD_CASES = ["att_hinge_hard", "att_lse_pool_mix", "att_hinge_pool"]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _counted(monkeypatch, module, name):
    """Replace module.name by a wrapper that counts its calls and keeps its results."""
    fn = getattr(module, name)
    log = SimpleNamespace(calls=0, results=[])

    def wrapper(*a, **kw):
        log.calls += 1
        out = fn(*a, **kw)
        log.results.append(out)
        return out
    monkeypatch.setattr(module, name, wrapper)
    return log


def _quantised(rng, shape, plant=True):
    """fp32 multiples of 0.05 in [0, 0.35]; in three rows of four two regions are set to the threshold itself (4 * 0.05f == 0.2f
    exactly), so ties and scores equal to the threshold are the rule, not the exception."""
    s = (rng.integers(0, 8, size=shape) * np.float32(0.05)).astype(np.float32)
    if plant and shape[-1] >= 2:
        flat = s.reshape(-1, shape[-1])
        for i in range(flat.shape[0]):
            if i % 4 != 3:
                flat[i, rng.choice(shape[-1], 2, replace=False)] = np.float32(THD)
    return s


def _predict_ref(row, thd):
    keep = np.flatnonzero(row >= np.float32(thd))
    return keep[np.argsort(row[keep], kind="stable")]


def _desc_order(row, bits, Lr):
    nr = np.asarray([r for r in range(Lr) if (int(bits) >> r) & 1], dtype=np.int64)
    return nr[np.argsort(-row[nr], kind="stable")]


def _hard_inputs(rng, flat_scores, off, Lr):
    """Random negative sets; every rank position of every row is asked for once, in shuffled order."""
    K = off.shape[0]
    bits = rng.integers(0, 2 ** 63, size=K, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=K, dtype=np.uint64)
    if Lr < 64:
        bits &= np.uint64((1 << Lr) - 1)
    n_neg = np.asarray([bin(int(b)).count("1") for b in bits], dtype=np.int64)
    slot_begin = np.zeros(K + 1, dtype=np.int32)
    np.cumsum(n_neg, out=slot_begin[1:])
    slot_q = np.concatenate([rng.permutation(int(n)) for n in n_neg] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    exp = np.zeros(slot_q.shape[0], dtype=np.int64)
    for k in range(K):
        order = _desc_order(flat_scores[off[k]:off[k] + Lr], bits[k], Lr)
        sl = slice(int(slot_begin[k]), int(slot_begin[k + 1]))
        exp[sl] = off[k] + order[slot_q[sl]]
    return bits, slot_begin, slot_q, exp


def _dev(a, device):
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _load(name, device):
    fx = Fixture(name)
    cfg = json.loads(str(fx["cfg"]))
    labels = [[torch.from_numpy(l) for l in per] for per in fx["labels"]]
    N = fx["scores"].shape[0]
    batch = SimpleNamespace(target=torch.from_numpy(fx["target"]), att_labels=labels, anno_st_idx=[cfg["start"]] * N,
                            use_hard_negatives=cfg["hard"])
    model = SimpleNamespace(num_negatives=cfg["num_negatives"], negative_pool_size=cfg["pool"], num_hard=cfg["num_hard"],
                            drop_topk=cfg["drop_topk"], att_loss_type=cfg["loss_type"], margin=0.1, alpha=20.0, num_a=5,
                            _grouped=lambda: True)       # the K-group loss kernel (att_loss_kernel), as STAGE runs it
    return fx, cfg, torch.from_numpy(fx["scores"]).to(device), batch, model


def _existing_route(model, batch, scores, seed):
    """build_att_pairs (gather + .cpu() + numpy sort) -> AttPairs -> the loss kernel: the route hard-negative mode had."""
    torch.manual_seed(seed)
    pos, neg = att_host.build_att_pairs(model, batch, scores.detach(), n_local_candidates=scores.shape[1])
    pairs = att_host.AttPairs(pos, neg, scores.shape, scores.device)
    s = scores.detach().clone().requires_grad_()
    loss, _ = att_host.get_att_loss(model, s, batch, pairs=pairs)
    loss.backward()
    return pairs, loss.detach(), s.grad


def _new_route(model, batch, scores, seed, target_dev=None):
    torch.manual_seed(seed)
    plan = att_host.build_hard_plan(model, batch, n_local_candidates=scores.shape[1], placeholder_targets=target_dev is not None)
    assert plan is not None
    pairs = att_host.AttHardPairs(plan, scores.shape, scores.device, target_dev=target_dev)
    s = scores.detach().clone().requires_grad_()
    loss, _ = att_host.get_att_loss(model, s, batch, pairs=pairs)
    loss.backward()
    return pairs, loss.detach(), s.grad


def _same_grad(model, a, b):
    if model.att_loss_type == "hinge":       # coefficients 0 / 1: the scatter's atomic adds are exact in any order
        assert torch.equal(a, b)
    else:                                    # lse: a positive receives num_negatives atomic adds in no fixed order
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=1e-6)


# ---- 5. kernels against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 1000])
@pytest.mark.parametrize("Lr", [1, 7, 16, 20, 33, 64])
def test_row_kernels_match_stable_numpy_sorts(hip_device, Lr, K):
    rng = np.random.default_rng(1000 * Lr + K)
    R = 4 * K + 3
    sc = _quantised(rng, (R, Lr))
    flat = sc.reshape(-1)
    off = np.concatenate([rng.permutation(R)[:K - K // 3] * Lr,                       # whole rows of the tensor
                          rng.integers(0, flat.shape[0] - Lr + 1, size=K // 3)]).astype(np.int64)      # and any Lr consecutive scores
    rows = np.stack([flat[o:o + Lr] for o in off])
    if Lr >= 7:
        ties = sum(np.unique(r).size < Lr for r in rows)
        at_thd = sum(bool((r == np.float32(THD)).any()) for r in rows)
        assert 2 * ties > K and 2 * at_thd > K, (ties, at_thd, K)
    d_scores = torch.from_numpy(sc).to(hip_device)
    cnt, val, idx = groups.att_predict(d_scores, _dev(off, hip_device), THD)
    cnt, val, idx = cnt.cpu().numpy(), val.cpu().numpy(), idx.cpu().numpy()
    exp_cnt, exp_val, exp_idx = np.zeros(K, np.int32), np.zeros((K, Lr), np.float32), np.full((K, Lr), -1, np.int32)
    for k in range(K):
        keep = _predict_ref(rows[k], THD)
        exp_cnt[k] = keep.size
        exp_idx[k, :keep.size] = keep
        exp_val[k, :keep.size] = rows[k][keep]
    assert np.array_equal(cnt, exp_cnt) and np.array_equal(idx, exp_idx) and np.array_equal(val.view(np.int32), exp_val.view(np.int32))

    bits, slot_begin, slot_q, exp = _hard_inputs(rng, flat, off, Lr)
    out = torch.full((slot_q.shape[0],), -7, dtype=torch.int64, device=hip_device)
    groups.att_hard_negatives(d_scores, _dev(off, hip_device), _dev(bits, hip_device), _dev(slot_begin, hip_device),
                              _dev(slot_q, hip_device), out)
    assert np.array_equal(out.cpu().numpy(), exp)


def test_out_of_range_rows_and_positions_give_sentinels(hip_device):
    Lr, R = 20, 16
    rng = np.random.default_rng(7)
    sc = _quantised(rng, (R, Lr))
    flat, n = sc.reshape(-1), R * Lr
    off = np.asarray([3 * Lr, -1, n - Lr + 1, 5 * Lr + 2, n, 1 << 40, n - Lr, -(1 << 40)], dtype=np.int64)
    good = [0, 3, 6]
    K = off.shape[0]
    d_scores = torch.from_numpy(sc).to(hip_device)
    cnt, val, idx = (t.cpu().numpy() for t in groups.att_predict(d_scores, _dev(off, hip_device), THD))
    for k in range(K):
        if k in good:
            keep = _predict_ref(flat[off[k]:off[k] + Lr], THD)
            assert cnt[k] == keep.size and np.array_equal(idx[k, :keep.size], keep)
            assert np.array_equal(val[k, :keep.size], flat[off[k]:off[k] + Lr][keep])
            assert (idx[k, keep.size:] == -1).all() and (val[k, keep.size:] == 0).all()
        else:
            assert cnt[k] == -1 and (idx[k] == -1).all() and (val[k] == 0).all()

    bits = np.full(K, (1 << Lr) - 1 - 0b1001, dtype=np.uint64)          # 18 negatives per row
    per = 4
    slot_begin = (np.arange(K + 1) * per).astype(np.int32)
    slot_q = np.tile(np.asarray([0, 17, 18, -1], dtype=np.int32), K)     # first, last, one past the last, negative
    out = torch.full((K * per,), -7, dtype=torch.int64, device=hip_device)
    groups.att_hard_negatives(d_scores, _dev(off, hip_device), _dev(bits, hip_device), _dev(slot_begin, hip_device),
                              _dev(slot_q, hip_device), out)
    out = out.cpu().numpy().reshape(K, per)
    for k in range(K):
        if k in good:
            order = _desc_order(flat[off[k]:off[k] + Lr], bits[k], Lr)
            assert out[k].tolist() == [off[k] + order[0], off[k] + order[17], -1, -1]
        else:
            assert (out[k] == -1).all()


def test_shapes_outside_one_wavefront_are_declined(hip_device):
    s = torch.zeros(2, 65, device=hip_device)
    off = torch.zeros(1, dtype=torch.int64, device=hip_device)
    with pytest.raises(groups.Unsupported):
        groups.att_predict(s, off, THD)
    with pytest.raises(groups.Unsupported):
        groups.att_hard_negatives(s, off, off, torch.zeros(2, dtype=torch.int32, device=hip_device),
                                  torch.zeros(0, dtype=torch.int32, device=hip_device),
                                  torch.zeros(0, dtype=torch.int64, device=hip_device))


# ---- 6. box prediction ----------------------------------------------------------------------------------------------------------
def _pred_args(fx, cfg, N):
    return dict(object_vocab=fx["vocab"].tolist(), words=torch.from_numpy(fx["words"]), vid_names=["v%d" % b for b in range(N)],
                qids=list(range(N)), img_indices=[list(range(100, 100 + cfg["Li"]))] * N, boxes=fx["boxes"].tolist(),
                start_indices=[cfg["start"]] * N)


def _assert_preds_equal(got, exp, keys=str):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert sorted(g.keys()) == sorted(int(k) for k in e.keys())
        for a in g:
            ge, ee = g[a], e[keys(a)]
            assert len(ge) == len(ee)
            for dg, de in zip(ge, ee):
                assert dg["word"] == de["word"] and dg["qid"] == de["qid"] and dg["vid_name"] == de["vid_name"]
                assert dg["img_idx"] == de["img_idx"] and dg["bbox"] == de["bbox"]
                np.testing.assert_allclose(dg["pred"], de["pred"], rtol=0, atol=0)


@pytest.mark.parametrize("name", ["att_lse_random", "att_hinge_hard"])
def test_att_prediction_on_the_device_matches_reference(hip_device, monkeypatch, name):
    fx, cfg, scores, batch, model = _load(name, hip_device)
    N = scores.shape[0]
    log = _counted(monkeypatch, groups, "att_predict")
    got = att_host.get_att_prediction(scores, **_pred_args(fx, cfg, N))
    assert log.calls == 1                                        # the device route ran
    _assert_preds_equal(got, json.loads(str(fx["preds"])))
    host = att_host.get_att_prediction(scores.cpu(), **_pred_args(fx, cfg, N))
    assert log.calls == 1                                        # a host tensor keeps the host loop
    assert got == host


def test_att_prediction_wider_than_a_wavefront_takes_the_host_route(hip_device, monkeypatch):
    g = torch.Generator().manual_seed(3)
    N, NA, Li, Lqa, Lr = 2, 5, 3, 4, 65
    scores = (torch.rand(N, NA, Li, Lqa, Lr, generator=g) * 0.4)
    args = dict(object_vocab=[1, 3], words=torch.randint(0, 5, (N, NA, Lqa), generator=g), vid_names=["a", "b"], qids=[4, 5],
                img_indices=[list(range(Li))] * N, boxes=[[[[i, r] for r in range(Lr)] for i in range(2)]] * N, start_indices=[1, 0])
    log = _counted(monkeypatch, groups, "att_predict")
    got = att_host.get_att_prediction(scores.to(hip_device), **args)
    assert log.calls == 0
    assert got == att_host.get_att_prediction(scores, **args) and any(d["pred"] for q in got for a in q for d in q[a])


# ---- 7 - 9. hard negatives ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HARD_CASES)
def test_hard_negatives_on_the_device_match_the_host_route(hip_device, monkeypatch, name):
    fx, cfg, scores, batch, model = _load(name, hip_device)
    old_pairs, old_loss, old_grad = _existing_route(model, batch, scores, cfg["seed"])
    new_pairs, new_loss, new_grad = _new_route(model, batch, scores, cfg["seed"])
    assert new_pairs.m == old_pairs.m and torch.equal(new_pairs.flat, old_pairs.flat)
    assert torch.equal(new_loss, old_loss)                       # same kernel, same indices, fixed summation order
    _same_grad(model, new_grad, old_grad)
    assert rel_err(new_loss, torch.tensor(float(fx["loss"]))) < TOL
    # get_att_loss takes the new route by itself
    log = _counted(monkeypatch, groups, "att_hard_negatives")
    torch.manual_seed(cfg["seed"])
    loss, _ = att_host.get_att_loss(model, scores, batch)
    assert log.calls == 1 and torch.equal(loss, old_loss)


@pytest.mark.parametrize("name", HARD_CASES)
def test_hard_negatives_with_tied_scores(hip_device, name):
    fx, cfg, scores, batch, model = _load(name, hip_device)
    rng = np.random.default_rng(5)
    q = _quantised(rng, tuple(scores.shape), plant=False)
    q[..., -5:] = 0.0                                            # zero-padded regions: five equal scores at the end of every row
    scores = torch.from_numpy(q).to(hip_device)
    old_pairs, old_loss, old_grad = _existing_route(model, batch, scores, cfg["seed"])
    new_pairs, new_loss, new_grad = _new_route(model, batch, scores, cfg["seed"])
    assert torch.equal(new_pairs.flat, old_pairs.flat) and torch.equal(new_loss, old_loss)
    _same_grad(model, new_grad, old_grad)


@pytest.mark.parametrize("name", HARD_CASES)
def test_hard_negatives_withdevice_only_targets(hip_device, monkeypatch, name):
    fx, cfg, scores, batch, model = _load(name, hip_device)
    old_pairs, old_loss, old_grad = _existing_route(model, batch, scores, cfg["seed"])
    batch.target = batch.target.to(hip_device)                   # no target_list: the answers exist on the device only
    assert att_host.device_only_targets(model, batch, scores.shape[1])
    new_pairs, new_loss, new_grad = _new_route(model, batch, scores, cfg["seed"], target_dev=batch.target)
    assert torch.equal(new_pairs.flat, old_pairs.flat) and torch.equal(new_loss, old_loss)
    _same_grad(model, new_grad, old_grad)
    log = _counted(monkeypatch, att_host, "build_hard_plan")
    torch.manual_seed(cfg["seed"])
    loss, _ = att_host.get_att_loss(model, scores, batch)
    assert log.calls == 1 and (log.results[0].heads[:, 1] == 0).all() and torch.equal(loss, old_loss)
    bad = batch.target.clone()
    bad[0] = 7                                                   # outside [0, NA): the reference raises; here the loss is poisoned
    batch.target = bad
    torch.manual_seed(cfg["seed"])
    loss, _ = att_host.get_att_loss(model, scores, batch)
    assert bool(torch.isnan(loss))


# ---- 10. no read-back -----------------------------------------------------------------------------------------------------------
class _NoReadBack:
    """Inside: ``torch.cuda.set_sync_debug_mode("error")`` and, independently of whether this torch build traps there,
    ``Tensor.cpu / tolist / item / numpy`` of a DEVICE tensor are counted (``device_reads``)."""

    def __init__(self):
        self.device_reads = []

    def __enter__(self):
        self.mp = pytest.MonkeyPatch()
        for name in ("cpu", "tolist", "item", "numpy"):
            orig = getattr(torch.Tensor, name)

            def patched(t, *a, _orig=orig, _name=name, **kw):
                if t.is_cuda:
                    self.device_reads.append(_name)
                return _orig(t, *a, **kw)
            self.mp.setattr(torch.Tensor, name, patched)
        self.mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        self.mp.undo()
        return False


def _sync_mode_traps(device) -> bool:
    t = torch.ones(1, device=device)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(mode)


@pytest.mark.parametrize("device_targets", [False, True])
def test_hard_negative_loss_reads_nothing_back(hip_device, monkeypatch, device_targets):
    fx, cfg, scores, batch, model = _load("att_lse_pool_mix", hip_device)
    _, old_loss, _ = _existing_route(model, batch, scores, cfg["seed"])
    if device_targets:
        batch.target = batch.target.to(hip_device)
    else:
        batch.target_list = batch.target.tolist()
        batch.target = batch.target.to(hip_device)
    s = scores.clone().requires_grad_()
    print("sync debug mode traps on this build:", _sync_mode_traps(hip_device))
    torch.manual_seed(cfg["seed"])
    torch.cuda.synchronize()
    with _NoReadBack() as guard:
        loss, _ = att_host.get_att_loss(model, s, batch)
        loss.backward()
    assert guard.device_reads == []
    assert torch.equal(loss.detach(), old_loss)


def test_att_prediction_reads_back_one_small_copy(hip_device, monkeypatch):
    fx, cfg, scores, batch, model = _load("att_lse_random", hip_device)
    N, Lr = scores.shape[0], scores.shape[-1]
    fetch = att_host._fetch
    copies = []
    guard = _NoReadBack()

    def one_copy(dev):                                           # the single result copy: the only place that may wait for the device
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("default")
        seen = len(guard.device_reads)
        try:
            out = fetch(dev)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        del guard.device_reads[seen:]
        copies.append(dev.numel() * dev.element_size())
        return out
    args = _pred_args(fx, cfg, N)
    torch.cuda.synchronize()
    with guard:
        monkeypatch.setattr(att_host, "_fetch", one_copy)
        got = att_host.get_att_prediction(scores, **args)
    assert guard.device_reads == []
    assert copies == [108 * (2 * Lr + 1) * 4]                    # K (2 Lr + 1) 4 bytes, K = 108 rows -- not the 100 800-byte map
    _assert_preds_equal(got, json.loads(str(fx["preds"])))


# ---- 11. whole model ------------------------------------------------------------------------------------------------------------
def _small_model_and_batch(device, seed, **opt_kw):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    torch.manual_seed(11)
    model = STAGE(make_opt(hsz=128, embedding_size=96, vfeat_size=64, dropout=0.1, use_sup_att=True, **opt_kw)).to(device)
    N, Li, Lr, Lqa = 3, 6, 16, 7
    batch = make_batch(N=N, Li=Li, Lr=Lr, Lw=5, Lqa=Lqa, wd_size=96, vfeat_size=64, seed=seed, att_imgs=3, att_words=2)
    batch.qas = torch.randint(0, 12, (N, 5, Lqa), generator=torch.Generator().manual_seed(seed))
    batch.eval_object_word_ids = [1, 4, 7, 10]
    batch.boxes = [[[[n, i, r, r + 1] for r in range(Lr)] for i in range(3)] for n in range(N)]
    return model, batch.to(device)


def test_inference_boxes_from_the_hip_forward(hip_device, monkeypatch):
    model, batch = _small_model_and_batch(hip_device, 2018)
    model.eval()
    log = _counted(monkeypatch, groups, "att_predict")
    model.inference_mode = True
    with torch.no_grad():
        res = model(batch)
    assert log.calls == 1
    model.inference_mode = False
    with torch.no_grad():
        other = model.forward_main(batch)[-1]
    host = att_host.get_att_prediction(other["vid_raw_s"].cpu(), batch.eval_object_word_ids, batch.qas.cpu(), batch.vid_name, batch.qid,
                                       batch.image_indices, batch.boxes, batch.anno_st_idx)
    assert log.calls == 1
    got = res["att_predictions"]
    assert got == host
    dets = [d for q in got for a in q for d in q[a]]
    assert dets and any(d["pred"] for d in dets)                 # boxes predicted from scores the HIP forward produced


@pytest.mark.parametrize("seed", [2018, 9])
@pytest.mark.parametrize("mode", ["topk", "pool_mix"])
def test_hard_negative_training_step_equals_the_host_route(hip_device, monkeypatch, mode, seed):
    kw = dict(num_negatives=3, drop_topk=1) if mode == "topk" else dict(num_negatives=3, negative_pool_size=4, num_hard=2)
    model, batch = _small_model_and_batch(hip_device, seed, **kw)
    model.train()
    batch.use_hard_negatives = True

    def step():
        model._seed_state = None
        torch.manual_seed(5)
        (out, targets), att_loss, _, t_loss, t_scores, other = model.forward_main(batch)
        return att_loss.detach().clone(), out.detach().clone()
    plans = _counted(monkeypatch, att_host, "build_hard_plan")
    launches = _counted(monkeypatch, groups, "att_hard_negatives")
    new_loss, new_out = step()
    assert plans.calls == 1 and plans.results[0] is not None and plans.results[0].k == 18 and launches.calls == 1
    monkeypatch.setattr(att_host, "build_hard_plan", lambda *a, **kw: None)      # the host route: gather, .cpu(), numpy sort
    old_loss, old_out = step()
    assert launches.calls == 1
    assert torch.equal(new_out, old_out) and torch.equal(new_loss, old_loss) and float(new_loss) > 0
