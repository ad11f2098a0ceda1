"""-m gpu: the K-group launch path (tvqaplus_amd/groups.py, csrc/groups.hip: one C call per fused-op group) against the per-op
path (tvqaplus_amd/ops.py: one call per kernel).  Both run the same kernels in the same order with the same dropout streams, so
outputs are expected to be IDENTICAL, dropout on; parameter gradients may differ at the ulp level (fused residual-gradient adds,
the order autograd sums the contributions of a shared module), hence a tight tolerance there instead of equality."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _build(kw, seed=3):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        model = STAGE(make_opt(**kw))
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    # dense rows here: the comparison is "same kernels, same dropout stream"; ragged token rows index the dropout counter by compact
    # row and are held to the dense path in tests/test_hip_ragged.py
    model.use_ragged = False
    return model


def _step(model, batch, use_groups, sup):
    model.use_groups = use_groups
    model._seed_state = 12345          # identical dropout streams
    torch.manual_seed(11)              # identical negative sampling of the attention loss
    for p in model.parameters():
        p.grad = None
    (out, targets), att_loss, _, t_loss, t_scores, other = model.forward_main(batch)
    loss = F.cross_entropy(out, targets, reduction="sum") * (len(batch.qid) / len(targets)) + 0.5 * t_loss
    if sup:
        loss = loss + 0.1 * att_loss
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return out.detach().clone(), t_scores.detach().clone(), {k: v.detach().clone() for k, v in other.items()}, float(loss), grads, model._seed_state


CASES = [
    # the bench configuration's kernels (D = 128: register-resident / LDS-staged attention, fused attention backward, streaming GEMMs)
    (dict(hsz=128, add_local=True, dropout=0.1, use_sup_att=True), dict(N=2, Li=24, Lr=20, Lw=50, Lqa=40, att_imgs=2, att_words=2)),
    (dict(hsz=128, add_local=False, dropout=0.1), dict(N=3, Li=10, Lr=20, Lw=32, Lqa=17)),
    # small odd shapes: tiled GEMM fallbacks, generic attention backward; one stream only
    (dict(hsz=32, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.2), dict(N=2, Li=5, Lr=7, Lw=9, Lqa=6, wd_size=48, vfeat_size=40)),
    (dict(hsz=64, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.1, sub_flag=False), dict(N=2, Li=5, Lr=8, Lw=9, Lqa=6, wd_size=48, vfeat_size=40)),
    # self-attention blocks stay per-op, the other groups still run grouped; three conv layers per block; 256-wide rows
    (dict(hsz=64, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.1, input_encoder_n_heads=2, cls_encoder_n_conv=3),
     dict(N=2, Li=4, Lr=6, Lw=7, Lqa=6, wd_size=48, vfeat_size=40)),
    (dict(hsz=256, embedding_size=48, vfeat_size=40, add_local=True, dropout=0.1), dict(N=1, Li=4, Lr=10, Lw=70, Lqa=9, wd_size=48, vfeat_size=40)),
]


@pytest.fixture
def no_fused_cat3(monkeypatch):
    """The sequencing claim (group path == per-op path, bit for bit in the outputs) is about the SAME kernels: the fused
    LayerNorm / Linear kernels of csrc/cat3_fused.hip, which only the group path runs, are switched off; they are held to the
    two-kernel path separately (test_fused_cat3_*, test_group_path_with_fused_kernels_close_to_per_op_path)."""
    monkeypatch.setenv("STAGE_NO_CAT3_FUSED", "1")


@pytest.mark.parametrize("case", range(len(CASES)))
def test_group_path_equals_per_op_path(hip_device, case, no_fused_cat3):
    from tvqaplus_amd.synth import make_batch
    kw, shape = CASES[case]
    model = _build(kw).to(hip_device).train()
    if kw.get("input_encoder_n_heads"):
        model.mha_dropout_override = None
    batch = make_batch(seed=5, **shape).to(hip_device)
    sup = bool(kw.get("use_sup_att"))
    o1, t1, m1, l1, g1, s1 = _step(model, batch, False, sup)
    o2, t2, m2, l2, g2, s2 = _step(model, batch, True, sup)
    assert s1 == s2, "the two paths must consume the dropout stream identically"
    assert torch.equal(o1, o2) and torch.equal(t1, t2), (float((o1 - o2).abs().max()), float((t1 - t2).abs().max()))
    for k in m1:
        assert torch.equal(m1[k], m2[k]), k
    assert abs(l1 - l2) <= 2e-6 * (1 + abs(l1)), (l1, l2)       # the fused loss kernels sum in their own (fixed) order
    exact, inexact = 0, []
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None), k
        if g1[k] is None:
            continue
        same = torch.equal(g1[k], g2[k])
        exact += int(same)
        if not same:
            inexact.append(k)
        scale = float(g1[k].abs().max()) + 1e-12
        assert float((g1[k] - g2[k]).abs().max()) <= 2e-5 * scale + 1e-7, (k, float((g1[k] - g2[k]).abs().max()), scale)
    # Bit-for-bit agreement is NOT expected for the gradients: the temporal head's group folds the residual-gradient adds into
    # the LayerNorm backward's final multiply-add (one rounding instead of autograd's separate add kernel), and a module shared
    # by several streams has its contributions summed by autograd in graph order, which differs between the two graphs.
    # Everything upstream of either inherits ulp-level differences; the scorers behind them agree exactly.
    assert exact >= 4, (exact, inexact[:8])


def test_group_path_with_fused_kernels_close_to_per_op_path(hip_device):
    """The default group path (fused LayerNorm + Linear forward / backward of the three [a, b, a*b] blocks) against the per-op path
    at the bench configuration's kernels, dropout on: outputs to 1e-5 of their scale, the loss to 1e-6, parameter gradients to
    2e-3 of theirs (a ReLU gate whose pre-activation is rounding noise may open on one side only)."""
    from tvqaplus_amd.synth import make_batch
    kw, shape = CASES[0]
    model = _build(kw).to(hip_device).train()
    batch = make_batch(seed=5, **shape).to(hip_device)
    o1, t1, m1, l1, g1, s1 = _step(model, batch, False, True)
    o2, t2, m2, l2, g2, s2 = _step(model, batch, True, True)
    assert s1 == s2
    assert float((o1 - o2).abs().max()) <= 1e-5 * (1 + float(o1.abs().max()))
    assert float((t1 - t2).abs().max()) <= 1e-5 * (1 + float(t1[t1 > -1e9].abs().max()))
    assert abs(l1 - l2) <= 1e-5 * (1 + abs(l1))
    for k in g1:
        if g1[k] is None:
            continue
        scale = float(g1[k].abs().max()) + 1e-12
        assert float((g1[k] - g2[k]).abs().max()) <= 2e-3 * scale + 2e-6, (k, float((g1[k] - g2[k]).abs().max()), scale)


def test_group_path_eval_and_inference_equal_per_op_path(hip_device, no_fused_cat3):
    from tvqaplus_amd.synth import make_batch
    kw, shape = CASES[0]
    model = _build(kw).to(hip_device).eval()
    batch = make_batch(seed=6, **shape).to(hip_device)
    outs = []
    for g in (False, True):
        model.use_groups = g
        with torch.no_grad():
            out, _, _, t_loss, t_prob, other = model.forward_main(batch)
        outs.append((out.clone(), t_prob.clone(), float(t_loss)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert abs(outs[0][2] - outs[1][2]) <= 2e-6 * (1 + abs(outs[0][2]))


def test_group_path_issues_few_host_calls(hip_device):
    """What the groups are for: the number of C-ABI calls the Python thread makes per training step."""
    from tvqaplus_amd import ops
    from tvqaplus_amd.synth import make_batch
    kw, shape = CASES[0]
    model = _build(kw).to(hip_device).train()
    batch = make_batch(seed=5, **shape).to(hip_device)
    counts = {}
    import tvqaplus_amd._lib as L
    lib = L.load()

    def run(flag):
        n = [0]
        real = {}
        names = [k for k in L.SIGNATURES if not k.endswith("_bytes") and "supported" not in k and "recomputes" not in k
                 and k not in ("stage_hip_abi_version", "stage_hip_error_string")]
        for k in names:
            real[k] = getattr(lib, k)

            def wrap(*a, _f=real[k]):
                n[0] += 1
                return _f(*a)
            setattr(lib, k, wrap)
        ops._FN.clear()
        try:
            _step(model, batch, flag, True)
        finally:
            for k in names:
                setattr(lib, k, real[k])
            ops._FN.clear()
        return n[0]
    counts["per_op"], counts["groups"] = run(False), run(True)
    assert counts["groups"] <= 45 and counts["groups"] * 4 <= counts["per_op"], counts


@pytest.mark.parametrize("which,dims,p", [
    ("qa_ctx", dict(N=2, NA=5, Li=12, Lqa=40, Lr=20), 0.1),      # broadcast `a` (rep = Li): LDS image + slab sum
    ("qa_ctx", dict(N=1, NA=5, Li=31, Lqa=29, Lr=10), 0.0),      # inner <= 32: one padded tile per frame, no dropout
    ("qa_ctx", dict(N=1, NA=5, Li=29, Lqa=29, Lr=10), 0.2),      # ... with dropout; a chunk of frames that is not a multiple of four
    ("qa_ctx", dict(N=3, NA=5, Li=7, Lqa=40, Lr=12), 0.1),       # inner = 40, 7 frames: the last group of four is ragged
    ("concat_fc", dict(U=4096 + 77), 0.1),                        # rep = 1, last tile partly filled
    ("concat_fc", dict(U=9000), 0.0),
])
def test_fused_cat3_backward_equals_gemm_plus_layernorm_backward(hip_device, which, dims, p):
    """csrc/cat3_fused.hip (the Linear's input gradient never leaves the compute unit) against the two-kernel path it replaces
    (dX GEMM -> 3D-wide tensor -> LayerNorm backward): same gradients to fp32 rounding (both products are the two-way fp16 split;
    the summation orders differ).  Kernel against kernel: the independent fp64 reference of the fused backward kernels is
    tests/test_hip_cat3_fp64.py."""
    import os
    from tvqaplus_amd import groups
    g = torch.Generator().manual_seed(7)
    D = 128
    dev = hip_device

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)
    ln_w, ln_b = (1.0 + 0.1 * torch.randn(3 * D, generator=g)).to(dev).requires_grad_(), rnd(3 * D, scale=0.1).requires_grad_()
    W, c = rnd(D, 3 * D, scale=0.08).requires_grad_(), rnd(D, scale=0.1).requires_grad_()
    seeds = [11, 12, 13]
    results = []
    for fused in (False, True):
        # same forward in both runs (the two-kernel one: identical ReLU masks); only the backward differs
        os.environ["STAGE_NO_CAT3_FUSED_FWD"] = "1"
        if fused:
            os.environ.pop("STAGE_NO_CAT3_FUSED", None)
        else:
            os.environ["STAGE_NO_CAT3_FUSED"] = "1"
        try:
            gg = torch.Generator().manual_seed(3)
            if which == "qa_ctx":
                N, NA, Li, Lqa, Lr = (dims[k] for k in ("N", "NA", "Li", "Lqa", "Lr"))
                qa = (torch.randn(N, NA, Lqa, D, generator=gg)).to(dev).requires_grad_()
                cx = (torch.randn(N, Li, Lr, D, generator=gg)).to(dev).requires_grad_()
                qm = (torch.rand(N, NA, Lqa, generator=gg) > 0.2).float().to(dev)
                cm = (torch.rand(N, Li, Lr, generator=gg) > 0.2).float().to(dev)
                mixed, S, Sn = groups.qa_ctx(qa, cx, qm, cm, 10.0, p, seeds, [ln_w, ln_b, W, c])
                go = torch.randn(mixed.shape, generator=gg).to(dev)
                (mixed * go).sum().backward()
                outs = [qa.grad, cx.grad]
            else:
                U = dims["U"]
                s = torch.randn(U, D, generator=gg).to(dev).requires_grad_()
                v = torch.randn(U, D, generator=gg).to(dev).requires_grad_()
                l2w, l2b = torch.ones(D, device=dev, requires_grad=True), torch.zeros(D, device=dev, requires_grad=True)
                out = groups.concat_fc(s, v, p, seeds[:1], [ln_w, ln_b, W, c, l2w, l2b])
                go = torch.randn(out.shape, generator=gg).to(dev)
                (out * go).sum().backward()
                outs = [s.grad, v.grad]
            torch.cuda.synchronize()
            results.append([t.clone() for t in outs] + [ln_w.grad.clone(), ln_b.grad.clone(), W.grad.clone(), c.grad.clone()])
        finally:
            os.environ.pop("STAGE_NO_CAT3_FUSED", None)
            os.environ.pop("STAGE_NO_CAT3_FUSED_FWD", None)
            for t in (ln_w, ln_b, W, c):
                t.grad = None
    names = ["d_a", "d_b", "d_gamma", "d_beta", "dW", "dc"]
    for nm, x, y in zip(names, results[0], results[1]):
        scale = float(x.abs().max()) + 1e-12
        err = float((x - y).abs().max())
        assert err <= 2e-5 * scale, (nm, err, scale)
    assert torch.equal(results[0][4], results[1][4]) and torch.equal(results[0][5], results[1][5])   # the weight gradient is the same kernel
    # the two paths sum in different orders: bit-identical input gradients would mean the fused kernel did not run
    assert not torch.equal(results[0][1], results[1][1])


@pytest.mark.parametrize("rep,inner,G,p", [(12, 40, 10, 0.1), (31, 29, 5, 0.0), (1, 1, 4096 + 77, 0.1), (1, 1, 9000, 0.0), (9, 11, 60, 0.2)])
def test_fused_cat3_forward_equals_layernorm_plus_gemm(hip_device, rep, inner, G, p):
    """csrc/cat3_fused.hip, forward: LayerNorm([a, b, a*b]) -> dropout -> Linear -> ReLU in one pass against the two kernels it
    replaces.  z, mean, rstd: same arithmetic in the same order (identical up to one ulp of multiply-add contraction, the dropout mask
    identical); y to fp32 rounding (both products are the two-way fp16
    split, summed in different orders); the ReLU bit masks agree wherever |y| is not rounding noise.  Kernel against kernel: the
    independent fp64 reference of the fused forward is tests/test_hip_cat3_fp64.py."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    D = 128
    U = G * rep * inner if rep > 1 else G
    g = torch.Generator().manual_seed(5)
    a = torch.randn((U // rep) if rep > 1 else U, D, generator=g).cuda()
    b = torch.randn(U, D, generator=g).cuda()
    gamma = (1 + 0.1 * torch.randn(3 * D, generator=g)).cuda()
    beta = (0.1 * torch.randn(3 * D, generator=g)).cuda()
    W = (0.08 * torch.randn(D, 3 * D, generator=g)).cuda()
    bias = (0.1 * torch.randn(D, generator=g)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.stage_cat3_ln_gemm_fwd_supported(U, D, rep, inner) == 1
    outs = []
    for fused in (False, True):
        z = torch.empty(U, 3 * D, device="cuda"); mean = torch.empty(U, device="cuda"); rstd = torch.empty(U, device="cuda")
        y = torch.empty(U, D, device="cuda"); mask = torch.zeros(D // 32, U, dtype=torch.int32, device="cuda")
        if fused:
            wsb = lib.stage_cat3_ln_gemm_fwd_ws_bytes()
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            _lib.check(lib.stage_cat3_ln_gemm_fwd(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), W.data_ptr(), bias.data_ptr(),
                                                  z.data_ptr(), mean.data_ptr(), rstd.data_ptr(), y.data_ptr(), mask.data_ptr(), U, D, rep, inner,
                                                  1e-5, p, 4242, ws.data_ptr(), wsb, st), "fused fwd")
        else:
            _lib.check(lib.stage_cat3_layernorm_fwd(a.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                                    rstd.data_ptr(), U, D, rep, inner, 1e-5, p, 4242, st), "ln fwd")
            _lib.check(lib.stage_gemm_nt_mask(z.data_ptr(), None, W.data_ptr(), bias.data_ptr(), y.data_ptr(), mask.data_ptr(), U, D, 3 * D, 1, st),
                       "gemm")
        torch.cuda.synchronize()
        outs.append((z, mean, rstd, y, mask))
    (z0, m0, r0, y0, k0), (z1, m1, r1, y1, k1) = outs
    # same operations in the same order; the compiler may contract a multiply-add differently in the two kernels: 1 ulp
    assert torch.equal(m0, m1) and float(((r0 - r1) / r0).abs().max()) < 3e-7
    assert float((z0 - z1).abs().max()) <= 4e-7 * float(z0.abs().max()) and torch.equal(z0 == 0, z1 == 0)
    scale = float(y0.abs().max())
    assert float((y0 - y1).abs().max()) <= 2e-6 * scale + 1e-6
    # mask bits: bit b of word w of row m <=> y[m, 32 w + b] > 0
    bits = lambda k: ((k.unsqueeze(-1) >> torch.arange(32, device="cuda", dtype=torch.int32)) & 1).permute(1, 0, 2).reshape(U, D).bool()
    assert torch.equal(bits(k1), y1 > 0)
    assert float((bits(k0) != bits(k1)).float().mean()) < 1e-4


def test_gradient_sink_orders_contributions_across_streams(hip_device):
    """groups._Sink / _ParamGate (the gradients of modules applied to several branches leave the graph once, summed OUTSIDE autograd's
    edges): with branch streams the contributions are produced on different streams.  Three streams, each kept busy by a large product in
    front of its contribution, then the gate's backward on the main stream: the totals must be exact (the unordered version added into
    accumulators that were still being written)."""
    import types
    from tvqaplus_amd import groups
    big = torch.randn(4096, 4096, device="cuda")
    for trial in range(8):              # (the unordered version got 3 of 8 trials wrong)
        sink = groups._Sink(2)
        streams = [torch.cuda.Stream() for _ in range(3)]
        main = torch.cuda.current_stream()
        for k, s in enumerate(streams):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                x = big @ big                                 # the contribution below is ready late
                g0 = x[:256, :256] * 0.0 + float(k + 1)
                g1 = x[:128, :512] * 0.0 + float(10 * (k + 1))
                sink.add([0, 1], [g0, g1])
        res = groups._ParamGate.backward(types.SimpleNamespace(sink=sink), None, None)
        assert res[0] is None
        torch.cuda.synchronize()
        assert float(res[1].min()) == float(res[1].max()) == 6.0, (trial, float(res[1].min()), float(res[1].max()))
        assert float(res[2].min()) == float(res[2].max()) == 60.0, (trial, float(res[2].min()), float(res[2].max()))
        assert sink.acc == [None, None]


@pytest.mark.parametrize("P,C,with_att,with_ts,dev_scale,ignored", [(19, 5, True, True, False, 0), (32, 5, True, False, True, 3),
                                                                  (1, 5, False, True, False, 0), (300, 7, True, True, False, 11)])
def test_reference_loss_matches_the_eager_lines(hip_device, P, C, with_att, with_ts, dev_scale, ignored):
    """tvqaplus_amd.stage.reference_loss (csrc/groups.hip: train_loss_kernel, one launch) against the eager lines of the reference's
    training loop (main.py:55-60: CrossEntropyLoss(reduction="sum") * len(qids) / len(targets) + weighted side losses): value and
    every gradient.  fp32 against fp32: 1e-6 relative (the order of the row sums differs)."""
    from tvqaplus_amd.stage import reference_loss
    g = torch.Generator().manual_seed(P * 7 + C)
    logits = (3.0 * torch.randn(P, C, generator=g)).cuda()
    targets = torch.randint(0, C, (P,), generator=g).cuda()
    if ignored:
        targets[torch.randperm(P, generator=g)[:ignored].cuda()] = -100
    att = torch.rand((), generator=g).cuda() * 4 if with_att else 0
    ts = torch.rand((), generator=g).cuda() * 9 if with_ts else 0
    n_examples = 16
    sc = float(n_examples) / P
    scale = torch.tensor(sc, device="cuda") if dev_scale else None
    grads = []
    for fused in (False, True):
        x = logits.clone().requires_grad_()
        a = att.clone().requires_grad_() if with_att else 0
        t = ts.clone().requires_grad_() if with_ts else 0
        if fused:
            loss = reference_loss(x, targets, a, t, n_examples, 0.1, 0.5, scale=scale)
        else:
            loss = F.cross_entropy(x, targets, reduction="sum") * (scale if dev_scale else sc) + 0.1 * a + 0.5 * t
        (loss * 1.7).backward()
        grads.append((loss.detach(), x.grad, a.grad if with_att else None, t.grad if with_ts else None))
    (l0, gx0, ga0, gt0), (l1, gx1, ga1, gt1) = grads
    assert abs(float(l0) - float(l1)) <= 1e-6 * (1 + abs(float(l0)))
    assert float((gx0 - gx1).abs().max()) <= 1e-6 * (1 + float(gx0.abs().max()))
    if with_att:
        assert abs(float(ga0) - float(ga1)) <= 1e-7
    if with_ts:
        assert abs(float(gt0) - float(gt1)) <= 1e-7
