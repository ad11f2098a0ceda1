"""Multi-proposal head without a GPU: the new symbols at the C boundary, the host statement of the top-K span order and the host
half of get_proposals against the reference's own results (tests/golden/topk_spans.json, written by make_golden_topk.py)."""
import contextlib
import io
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("stage_topk_spans_supported", "stage_gt_spans_topk", "stage_topk_spans", "stage_grp_pool_cls_bwd_s")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "topk_spans.json")) as f:
        return json.load(f)


def test_new_symbols_in_header_binding_and_library():
    from tvqaplus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "stage_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # argument kinds the header parser of tests/test_abi.py knows: pointers / int / long long / float
    I, LL, F, P = _lib.I, _lib.LL, _lib.F, _lib.P
    assert _lib.SIGNATURES["stage_topk_spans_supported"] == (I, [I, I])
    assert _lib.SIGNATURES["stage_gt_spans_topk"] == (I, [P, P, P, P, P, I, I, I, I, P])
    assert _lib.SIGNATURES["stage_topk_spans"] == (I, [P, I, P, P, LL, I, I, P])
    SZ = _lib.SZ
    assert _lib.SIGNATURES["stage_grp_pool_cls_bwd_s"] == (I, [P, P, P, P, P, P, P, P, SZ, P, SZ, I, I, I, I, LL, I, F, P, P])    # `slots` behind P
    assert int(re.search(r"#define STAGE_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 7 == _lib.ABI_VERSION == lib.stage_hip_abi_version()
    assert int(re.search(r"#define STAGE_TOPK_MAX (\d+)", hdr).group(1)) == 8 == _lib.STAGE_TOPK_MAX


@pytest.mark.parametrize("Li,K,ok", [(1, 1, 1), (2048, 8, 1), (2049, 1, 0), (5, 0, 0), (5, 9, 0), (0, 1, 0), (300, 5, 1)])
def test_supported_truth_table(Li, K, ok):
    from tvqaplus_amd import _lib, groups
    assert _lib.load().stage_topk_spans_supported(Li, K) == ok
    assert groups.topk_spans_supported(Li, K) is bool(ok)


def test_unsupported_shapes_are_declined_before_any_launch():
    """STAGE_ERR_SHAPE comes back from the argument check: no pointer is read, no GPU is needed."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    assert lib.stage_topk_spans(None, 0, None, None, 4, 2049, 1, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_topk_spans(None, 0, None, None, 4, 5, 9, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_topk_spans(None, 0, None, None, 4, 5, 0, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_gt_spans_topk(None, None, None, None, None, 4, 5, 2049, 3, None) == _lib.STAGE_ERR_SHAPE
    assert lib.stage_gt_spans_topk(None, None, None, None, None, 4, 5, 12, 9, None) == _lib.STAGE_ERR_SHAPE
    for slots in (0, 10):
        assert lib.stage_grp_pool_cls_bwd_s(None, None, None, None, None, None, None, None, 0, None, 0, 4, 5, 12, 128, 6, slots, 0.0,
                                            None, None) == _lib.STAGE_ERR_SHAPE


def test_find_max_triples_batch_on_the_host_equals_the_reference(golden):
    from tvqaplus_amd.evaluation import find_max_triples_batch
    for c in golden["cases"]:
        p_st, p_ed = torch.tensor(c["p_st"], dtype=torch.float32), torch.tensor(c["p_ed"], dtype=torch.float32)
        for thd, key in ((None, "triples"), (golden["prob_thd"], "triples_thd")):
            span, conf = find_max_triples_batch(p_st, p_ed, c["K"], prob_thd=thd)
            assert span.shape == (len(c["p_st"]), c["K"], 2) and conf.shape == (len(c["p_st"]), c["K"])
            for r, ref in enumerate(c[key]):
                # the reference lists a zero of the lower triangle where a row has no further pair: padding here
                ref = [t for t in ref if t[0] <= t[1]]
                for k in range(c["K"]):
                    got = (int(span[r, k, 0]), int(span[r, k, 1]), float(conf[r, k]))
                    if k < len(ref):
                        assert got[:2] == (ref[k][0], ref[k][1]), (c["Li"], c["K"], key, r, k)
                        assert abs(got[2] - ref[k][2]) <= 1e-6 * abs(ref[k][2]), (c["Li"], c["K"], key, r, k)
                    else:
                        assert got == (-1, -1, 0.0), (c["Li"], c["K"], key, r, k)
        if 1 < c["Li"] and c["Li"] * (c["Li"] + 1) // 2 < c["K"]:           # (Li = 1 has no lower triangle: the reference's list is short)
            assert any(t[0] > t[1] for row in c["triples"] for t in row)     # the fixture does hold such rows


def test_host_order_rule_on_exact_ties():
    """All products equal: ascending st * L + ed decides, and the lower triangle never appears."""
    from tvqaplus_amd.evaluation import find_max_triples_batch
    p = torch.full((2, 4), 0.25)
    span, conf = find_max_triples_batch(p, p, 6)
    assert span[0].tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 1], [1, 2]] and span[1].tolist() == span[0].tolist()
    assert torch.equal(conf, torch.full((2, 6), 0.0625))


def test_proposal_rows_reproduces_the_reference_span_lists(golden):
    """The factored host loop on the reference's unthresholded triples: the label's span first, then the survivors by rank; windows as
    expand_span makes them."""
    from tvqaplus_amd.stage import proposal_rows
    seen_multi = 0
    for c in golden["cases"]:
        K, N = c["K"], len(c["lab_st"])
        host = []
        for k in range(K):      # (Li = 1: the reference's list is shorter than K -- the kernel's padding stands in)
            rank = [c["triples"][n][k] if k < len(c["triples"][n]) else [-1, -1, 0.0] for n in range(N)]
            host += [[float(t[0]) for t in rank], [float(t[1]) for t in rank], [float(t[2]) for t in rank]]
        answers = [float((3 * n + 1) % 5) for n in range(N)]
        host += [[float(v) for v in c["lab_st"]], [float(v) for v in c["lab_ed"]], answers]
        src, wins, inv, tgt = proposal_rows(host, N, K, golden["iou_thd"], golden["prob_thd"], golden["extra_span_length"])
        exp_src = [n for n in range(N) for _ in c["spans"][n]]
        exp_win = [v for n in range(N) for w in c["windows"][n] for v in w]
        assert src == exp_src and wins == exp_win, (c["Li"], K)
        assert tgt == [int(answers[n]) for n in exp_src]
        assert len(inv) == N * (K + 1)
        p = 0
        for n in range(N):
            cnt = len(c["spans"][n])
            assert inv[(K + 1) * n:(K + 1) * (n + 1)] == list(range(p, p + cnt)) + [-1] * (K + 1 - cnt)
            # label first
            assert wins[2 * p:2 * p + 2] == [max(0, c["lab_st"][n] - golden["extra_span_length"]),
                                             c["lab_ed"][n] + 1 + golden["extra_span_length"]]
            p += cnt
            seen_multi += cnt >= 3
    assert seen_multi >= 5          # examples with two or more predicted spans next to the label's


def test_proposal_rows_skips_padding_and_needs_no_answer_row():
    from tvqaplus_amd.stage import proposal_rows
    # rank 1 is padding (-1, -1, 0); a threshold of 0 must not turn it into a span
    host = [[2.0], [3.0], [0.5], [-1.0], [-1.0], [0.0], [2.0], [3.0]]
    src, wins, inv, tgt = proposal_rows(host, 1, 2, 0.5, 0.0, 1)
    assert (src, wins, inv, tgt) == ([0, 0], [1, 5, 1, 5], [0, 1, -1], [])


def _opt(**kw):
    from tvqaplus_amd.synth import make_opt
    return make_opt(hsz=16, embedding_size=8, vfeat_size=8, **kw)


def test_max_num_proposal_option():
    from tvqaplus_amd.stage import STAGE
    with contextlib.redirect_stdout(io.StringIO()):
        opt = _opt()
        if hasattr(opt, "max_num_proposal"):
            delattr(opt, "max_num_proposal")
        assert STAGE(opt).max_num_proposal == 1                  # absent: today's behaviour
        for k in (1, 3, 8):
            opt.max_num_proposal = k
            assert STAGE(opt).max_num_proposal == k
        for k in (0, 9, -1):
            opt.max_num_proposal = k
            with pytest.raises(ValueError):
                STAGE(opt)


def test_prediction_writer_default_file_is_unchanged(tmp_path):
    """n_best = 1 writes the bytes of a writer built without the argument; n_best = 3 adds ts_nbest beside the records (CPU tensors: the
    torch statement of both decoders)."""
    from tvqaplus_amd.evaluation import PredictionWriter, find_max_triples_batch
    g = torch.Generator().manual_seed(5)
    N, NA, Li = 3, 5, 9
    outputs = dict(answer=torch.randn(N, NA, generator=g), t_scores=torch.softmax(torch.randn(N, NA, Li, 2, generator=g) * 2, dim=2))
    qids, img = [11, 12, 13], [[3, 9], [4, 10], [8, 14]]
    files = []
    for i, w in enumerate((PredictionWriter(), PredictionWriter(n_best=1), PredictionWriter(n_best=3))):
        w.add_batch(outputs, qids, img)
        w.save(str(tmp_path / ("p%d.json" % i)))
        files.append(open(str(tmp_path / ("p%d.json" % i)), "rb").read())
    assert files[0] == files[1] and b"ts_nbest" not in files[0]
    rec = json.loads(files[2])
    assert rec["ts_answer"] == json.loads(files[0])["ts_answer"]
    pred = outputs["answer"].max(1)[1]
    for n, qid in enumerate(qids):
        nb = rec["ts_nbest"][str(qid)]
        assert len(nb) == 3 and nb[0][:2] == rec["ts_answer"][str(qid)][0]
        span, conf = find_max_triples_batch(outputs["t_scores"][n, pred[n], :, 0][None], outputs["t_scores"][n, pred[n], :, 1][None], 3)
        off = (img[n][0] % 6) / 3
        assert nb == [[int(s) * 2 + off, (int(e) + 1) * 2 + off, float(c)] for (s, e), c in zip(span[0].tolist(), conf[0].tolist())]
    with pytest.raises(ValueError):
        PredictionWriter(n_best=0)
