"""CPU: the score-free host plans of the two consumers of the attention map that rank rows on the device
(tvqaplus_amd/att_host.py: build_hard_plan, build_predict_rows; kernels: csrc/score_rows.hip).  The kernel is replaced here by a
numpy stand-in with the kernel's ordering rule, so these run without a GPU; tests/test_hip_score_rows.py runs the kernels."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import Fixture
from tvqaplus_amd import att_host

HARD_CASES = {"att_hinge_hard": (42, 170), "att_lse_pool_mix": (50, 192), "att_hinge_pool": (41, 246)}


def _load(name):
    fx = Fixture(name)
    cfg = json.loads(str(fx["cfg"]))
    scores = torch.from_numpy(fx["scores"])
    labels = [[torch.from_numpy(l) for l in per] for per in fx["labels"]]
    N = scores.shape[0]
    batch = SimpleNamespace(target=torch.from_numpy(fx["target"]), att_labels=labels, anno_st_idx=[cfg["start"]] * N,
                            use_hard_negatives=cfg["hard"])
    model = SimpleNamespace(num_negatives=cfg["num_negatives"], negative_pool_size=cfg["pool"], num_hard=cfg["num_hard"],
                            drop_topk=cfg["drop_topk"], att_loss_type=cfg["loss_type"], margin=0.1, alpha=20.0)
    return fx, cfg, scores, batch, model


def resolve_numpy(plan, scores: np.ndarray):
    """Stand-in for stage_att_hard_negatives: position q of a row's negatives in descending score order, equal scores by region
    (rank of negative i = number of negatives j with s_j > s_i or (s_j == s_i and j < i))."""
    Lr = scores.shape[-1]
    neg = np.zeros((plan.m, 5), dtype=np.int64)
    for k in range(plan.k):
        b, a, g, w = plan.heads[k]
        row = scores[b, a, g, w]
        nr = np.asarray([r for r in range(Lr) if (int(plan.negbits[k]) >> r) & 1], dtype=np.int64)
        order = nr[np.argsort(-row[nr], kind="stable")]
        for m in range(int(plan.slot_begin[k]), int(plan.slot_begin[k + 1])):
            neg[m] = (b, a, g, w, order[plan.slot_q[m]])
    pos = np.concatenate([plan.heads[plan.pos_row], plan.pos_region[:, None]], axis=1)
    return pos, neg


@pytest.mark.parametrize("name", sorted(HARD_CASES))
def test_hard_plan_reproduces_build_att_pairs(name):
    fx, cfg, scores, batch, model = _load(name)
    torch.manual_seed(cfg["seed"])
    pos, neg = att_host.build_att_pairs(model, batch, scores)
    state = torch.get_rng_state()
    torch.manual_seed(cfg["seed"])
    plan = att_host.build_hard_plan(model, batch)
    assert plan is not None
    assert torch.equal(torch.get_rng_state(), state)              # the reference's draws, all of them, nothing else
    assert (plan.k, plan.m) == HARD_CASES[name]
    got_pos, got_neg = resolve_numpy(plan, scores.numpy())
    assert np.array_equal(got_pos, pos) and np.array_equal(got_neg, neg)


@pytest.mark.parametrize("name,n_rows", [("att_lse_random", 108), ("att_hinge_hard", 102)])
def test_predict_rows_reproduce_the_fixture(name, n_rows):
    fx, cfg, scores, batch, model = _load(name)
    N, Li = scores.shape[0], cfg["Li"]
    boxes = fx["boxes"].tolist()
    rows = att_host.build_predict_rows(torch.from_numpy(fx["words"]), fx["vocab"].tolist(), boxes, [cfg["start"]] * N, scores.shape)
    assert rows.shape == (n_rows, 4) and rows.dtype == np.int64
    sc, wd = scores.numpy(), fx["words"]
    got = [{str(a): [] for a in range(sc.shape[1])} for _ in range(N)]
    for b, a, g, w in rows.tolist():
        row = sc[b, a, g, w]
        keep = np.flatnonzero(row >= np.float32(0.2))
        keep = keep[np.argsort(row[keep], kind="stable")]
        got[b][str(a)].append({"pred": [float(v) for v in row[keep]], "bbox": [boxes[b][g - cfg["start"]][int(i)] for i in keep],
                               "word": int(wd[b, a, w]), "qid": b, "vid_name": "v%d" % b, "img_idx": 100 + g})
    assert got == json.loads(str(fx["preds"]))


def test_plan_that_cannot_be_exact_is_declined():
    fx, cfg, scores, batch, model = _load("att_hinge_hard")
    Lr = scores.shape[-1]
    torch.manual_seed(0)
    state = torch.get_rng_state()
    model.drop_topk = Lr                                            # top-k mode: every row runs out of negatives
    assert att_host.build_hard_plan(model, batch) is None
    fx, cfg, scores, batch, model = _load("att_lse_pool_mix")
    assert model.num_hard < model.num_negatives                     # the fixture mixes easy negatives in
    model.negative_pool_size = Lr                                   # the hard pool swallows every negative: the easy pool is empty
    assert att_host.build_hard_plan(model, batch) is None
    fx, cfg, scores, batch, model = _load("att_hinge_pool")
    model.drop_topk = Lr                                            # pool mode: nothing left for the hard pool
    assert att_host.build_hard_plan(model, batch) is None
    assert torch.equal(torch.get_rng_state(), state)              # a declined plan has drawn nothing


def test_hard_plan_with_placeholder_targets_uses_candidate_zero():
    fx, cfg, scores, batch, model = _load("att_hinge_hard")
    torch.manual_seed(cfg["seed"])
    a = att_host.build_hard_plan(model, batch)
    torch.manual_seed(cfg["seed"])
    b = att_host.build_hard_plan(model, batch, placeholder_targets=True)
    assert (b.heads[:, 1] == 0).all()
    assert np.array_equal(a.heads[:, [0, 2, 3]], b.heads[:, [0, 2, 3]]) and np.array_equal(a.heads[:, 1], fx["target"][a.heads[:, 0]])
    assert np.array_equal(a.slot_q, b.slot_q) and np.array_equal(a.negbits, b.negbits) and np.array_equal(a.pos_region, b.pos_region)


def test_score_row_symbols_answer_without_a_gpu():
    from tvqaplus_amd import _lib, groups
    lib = _lib.load()
    for name in ("stage_score_rows_supported", "stage_att_predict", "stage_att_hard_negatives"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert [lib.stage_score_rows_supported(v) for v in (1, 20, 64, 0, 65)] == [1, 1, 1, 0, 0]
    assert groups.score_rows_supported(20) and not groups.score_rows_supported(65)
    assert lib.stage_hip_abi_version() == 7
