"""-m gpu: the fp32 model on half-precision FEATURES (qas_bert / sub_bert / vid stored as fp16 or bf16).

Run A hands the model the half-precision tensors; run B hands it the same values cast back to float32 -- what the model made of such
features on entry before it read them in place (csrc/feat16.hip).  The conversion is exact, so A must compute B's function: same
proposal set, outputs and losses within the project's 1e-3, parameter gradients within 6e-3 (tests/test_hip_stage.py: TOL / GTOL), the
same units dropped, the same ragged context layout -- and no fp32 copy of the features on the device.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import UNDEFINED_GRADS, Fixture, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3          # tests/test_hip_stage.py
GTOL = 6e-3
FEATURES = ("qas_bert", "sub_bert", "vid")
FIXTURES = ["small_local_train", "mid_train", "small_supatt_train", "tiny_inference"]


def _model_from(fx, device):            # as tests/test_hip_stage.py::_model_from
    from tvqaplus_amd.stage import STAGE
    model = STAGE(fx.opt)
    model.load_state_dict(fx.group("param"), strict=True)
    model.mha_dropout_override = 0.0
    return model.to(device)


def _with_features(batch, dtypes, back_to_float):
    """A copy of ``batch`` whose features are cast to ``dtypes[name]`` (run A) and, for run B, back to float32."""
    from tvqaplus_amd.synth import Batch
    out = Batch(batch)
    for k in FEATURES:
        t = batch[k].to(dtypes.get(k, torch.float32))
        out[k] = t.float() if back_to_float else t
    return out


def _train_step(model, batch, seed, sup_att):
    """One seeded training step: the dropout stream is re-derived from the seed, so two calls drop the same units."""
    model.train()
    model.zero_grad(set_to_none=True)
    model._seed_state = None
    torch.manual_seed(seed)
    (out, targets), att_loss, _, t_loss, t_scores, _ = model.forward_main(batch)
    loss = F.cross_entropy(out, targets, reduction="sum") * (len(batch.qid) / len(targets)) + 0.5 * t_loss
    if sup_att:
        loss = loss + 0.1 * att_loss
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    return dict(targets=targets.cpu(), logits=out.detach(), t_scores=t_scores.detach(), loss=loss.detach(), grads=grads,
                ctx=set(model.last_ragged_ctx), ragged=model.last_ragged is not None)


def _assert_same_step(a, b, skip=()):
    assert torch.equal(a["targets"], b["targets"]), "proposal set differs"
    for k in ("logits", "t_scores", "loss"):
        assert rel_err(a[k], b[k]) < TOL, (k, rel_err(a[k], b[k]))
    errs = {k: rel_err(g, b["grads"][k]) for k, g in a["grads"].items() if k not in skip}
    worst = max(errs.items(), key=lambda kv: kv[1])
    assert worst[1] < GTOL, (worst, sorted((k, "%.1e" % e) for k, e in errs.items() if e >= GTOL))
    assert a["ragged"] == b["ragged"]
    assert a["ctx"] == b["ctx"], "half-precision features changed the context layout: %s vs %s" % (a["ctx"], b["ctx"])


@functools.lru_cache(maxsize=None)
def _fixture_runs(name, dtype):
    """(A, B) of one fixture, computed once: the parity test of every fixture and the test over all of them share it."""
    dev = torch.device("cuda:0")
    fx = Fixture(name)
    model = _model_from(fx, dev)
    host = fx.batch()
    dtypes = {k: dtype for k in FEATURES}
    seed = int(fx["att_seed"]) if "att_seed" in fx.z.files else 0
    runs = []
    for back in (False, True):
        batch = _with_features(host, dtypes, back).to(dev)
        if fx.mode == "train":
            runs.append(_train_step(model, batch, seed, bool(fx.opt.use_sup_att)))
        else:
            model.eval()
            model.inference_mode = True
            with torch.no_grad():
                res = model(batch)
            runs.append(dict(answer=res["answer"], t_scores=res["t_scores"], ctx=set(model.last_ragged_ctx)))
    return runs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_half_features_compute_the_upcast_run(hip_device, name, dtype):
    a, b = _fixture_runs(name, dtype)
    if "grads" in a:
        _assert_same_step(a, b, skip=UNDEFINED_GRADS.get(name, ()))
    else:
        assert rel_err(a["answer"], b["answer"]) < TOL and rel_err(a["t_scores"], b["t_scores"]) < TOL
        assert a["ctx"] == b["ctx"]


def test_a_fixture_keeps_its_ragged_context_layout(hip_device):
    """At least one of the fixtures runs its context streams ragged on float32 features -- and therefore (the test above) on
    half-precision ones: before the features were read in place such a step fell back to the padded rows."""
    kept = {name: _fixture_runs(name, torch.float16)[1]["ctx"] for name in FIXTURES}
    assert any(kept.values()), kept
    for name in FIXTURES:
        assert _fixture_runs(name, torch.float16)[0]["ctx"] == kept[name], name


def _synthetic(dev, hsz, wd, vf, sup_att, seed=21, dropout=0.1):
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_opt
    torch.manual_seed(seed)
    model = STAGE(make_opt(hsz=hsz, embedding_size=wd, vfeat_size=vf, dropout=dropout, add_local=True, use_sup_att=sup_att))
    with torch.no_grad():
        for q in model.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return model.to(dev)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_dropout_step_drops_the_same_units(hip_device, dtype):
    """dropout 0.1, dense grouped path (hsz 32): both runs seeded identically, as tests/test_hip_dropout_parity.py seeds its runs"""
    from tvqaplus_amd.synth import make_batch
    model = _synthetic(hip_device, 32, 64, 32, False)
    host = make_batch(N=2, Li=5, Lr=6, Lw=7, Lqa=8, wd_size=64, vfeat_size=32, seed=33)
    dtypes = {k: dtype for k in FEATURES}
    a = _train_step(model, _with_features(host, dtypes, False).to(hip_device), 77, False)
    b = _train_step(model, _with_features(host, dtypes, True).to(hip_device), 77, False)
    _assert_same_step(a, b)


@functools.lru_cache(maxsize=None)
def _ragged_model_and_batch(dropout=0.1):
    from tvqaplus_amd.synth import make_batch
    dev = torch.device("cuda:0")
    model = _synthetic(dev, 128, 64, 48, True, dropout=dropout)   # tests/test_hip_dropout_parity.py's configuration: ragged, both streams
    host = make_batch(N=3, Li=8, Lr=10, Lw=12, Lqa=14, wd_size=64, vfeat_size=48, seed=33, att_imgs=2, att_words=2)
    return model, host


@pytest.mark.parametrize("case", ["fp16", "bf16", "mixed"])
def test_ragged_dropout_step_and_mixed_dtypes(hip_device, case):
    """hsz 128, dropout 0.1, supervised attention: the ragged layout with both context streams compact.  ``mixed``: every feature
    tensor of one batch has its own type (vid fp16, sub_bert float32, qas_bert bf16)."""
    model, host = _ragged_model_and_batch()
    dtypes = {"fp16": {k: torch.float16 for k in FEATURES}, "bf16": {k: torch.bfloat16 for k in FEATURES},
              "mixed": {"vid": torch.float16, "sub_bert": torch.float32, "qas_bert": torch.bfloat16}}[case]
    a = _train_step(model, _with_features(host, dtypes, False).to(hip_device), 77, True)
    b = _train_step(model, _with_features(host, dtypes, True).to(hip_device), 77, True)
    assert b["ragged"] and b["ctx"] == {"sub", "vid"}
    _assert_same_step(a, b)


def test_misaligned_features_take_the_upcast_path(hip_device):
    """sub_bert as a view that starts one element (2 bytes) into its buffer: the 8-byte loads of the in-place path do not apply, the
    stream is upcast as before (padded rows) and agrees with run B.

    Dropout 0 here, unlike the tests above: A's subtitle stream runs on the padded rows and B's on the compact ones, and a dropout
    site indexes its stream by the row of the layout it runs on (tests/test_hip_dropout_parity.py: ``ctx(name)``), so at p > 0 the
    two layouts drop different units and compute different functions by design.  At p = 0 they are one function, held to TOL / GTOL."""
    from tvqaplus_amd import groups
    model, host = _ragged_model_and_batch(dropout=0.0)
    dtypes = {k: torch.float16 for k in FEATURES}
    ha = _with_features(host, dtypes, False).to(hip_device)
    sub = ha["sub_bert"]
    buf = torch.zeros(sub.numel() + 4, dtype=sub.dtype, device=sub.device)
    buf[1: 1 + sub.numel()] = sub.reshape(-1)
    ha["sub_bert"] = buf[1: 1 + sub.numel()].view(sub.shape)
    assert ha["sub_bert"].data_ptr() % 8 == 2 and not groups.feat16_ok(ha["sub_bert"]) and groups.feat16_ok(ha["vid"])
    a = _train_step(model, ha, 77, True)
    b = _train_step(model, _with_features(host, dtypes, True).to(hip_device), 77, True)
    assert "sub" not in a["ctx"] and "vid" in a["ctx"]
    a["ctx"] = b["ctx"]                                   # (the layouts differ by construction here; everything else must agree)
    _assert_same_step(a, b)


def test_no_fp32_copy_of_the_features(hip_device):
    """Peak device memory of a step (forward + backward) above what is allocated before it: with half-precision features it must
    not exceed the same quantity of the upcast batch.  (An upcast on entry exceeds it by the retained fp32 copies.)"""
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    torch.manual_seed(5)
    model = STAGE(make_opt()).to(hip_device)
    host = make_batch(N=2, Li=32, Lw=32, Lr=8, wd_size=768, vfeat_size=300)
    dtypes = {k: torch.float16 for k in FEATURES}
    batches = {"half": _with_features(host, dtypes, False).to(hip_device), "upcast": _with_features(host, dtypes, True).to(hip_device)}

    def step(batch):
        _train_step(model, batch, 3, False)
        model.zero_grad(set_to_none=True)

    peak = {}
    for name in ("half", "upcast", "half", "upcast"):           # first round: warm-up (layout staging buffers, allocator pools)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(batches[name])
        peak[name] = torch.cuda.max_memory_allocated() - base
    print("step peak above the resident batch: half %.2f MB, upcast %.2f MB" % (peak["half"] / 2 ** 20, peak["upcast"] / 2 ** 20))
    assert peak["half"] <= peak["upcast"], peak


def test_prefetcher_delivers_fp16_features(hip_device):
    from tvqaplus_amd.prefetch import BatchPrefetcher
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    torch.manual_seed(2)
    model = STAGE(make_opt(hsz=32, embedding_size=64, vfeat_size=32)).to(hip_device).eval()
    host = make_batch(N=2, Li=5, Lr=6, Lw=7, Lqa=8, wd_size=64, vfeat_size=32, seed=9)
    got = next(BatchPrefetcher([host], hip_device, feature_dtype=torch.float16))
    torch.cuda.synchronize()
    for k, v in host.items():
        if not torch.is_tensor(v):
            continue
        if k in FEATURES:
            assert got[k].dtype == torch.float16 and torch.equal(got[k].cpu(), v.half()), k
        else:
            assert got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v), k          # masks, labels, indices: untouched
    for kk, vv in host["ts_label"].items():
        assert got["ts_label"][kk].dtype == vv.dtype and torch.equal(got["ts_label"][kk].cpu(), vv)
    by_hand = _with_features(host, {k: torch.float16 for k in FEATURES}, False).to(hip_device)
    with torch.no_grad():
        out_p = model.forward_main(got)
        out_h = model.forward_main(by_hand)
    assert torch.equal(out_p[0], out_h[0])                       # logits
    assert torch.equal(out_p[4], out_h[4])                       # temporal probabilities
    with pytest.raises(ValueError):
        BatchPrefetcher([host], hip_device, feature_dtype=torch.float64)
