"""FlatAdam (tvqaplus_amd/optim.py, csrc/flat_adam.hip) on the GPU: the clip + Adam step on the packed gradient buffer against torch's
own Adam in fp64, its repeatability, the state_dict interchange with torch.optim.Adam, the launch diet, and three steps of a model.

Shapes sit at the chunk boundaries of the kernel (1024 elements), not at model size.  The tolerance of the comparisons is MEASURED in the
test: E = the largest error of torch's CPU fp32 Adam against torch's CPU fp64 Adam on the same fp32 gradient sequence, over all
parameters and moments; FlatAdam must lie within 4 E plus one fp32 ulp of the value (the kernel evaluates the same fp32 expressions in a
possibly different order -- the same error class; the factor covers the ordering)."""
import contextlib
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import Fixture

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3,), (1023,), (1024,), (1025,), (7, 5, 3, 2), (2049,), (300, 128), (6,)]
STEPS, LR, MAX_NORM = 8, 1e-3, 10.0
SCALES = (0.01, 50.0, 1e-9, 1.0)
WDS = (0.0, 3e-7, 0.1)
# phase of the scale cycle per parameter: a parameter's scale is SCALES[(step + PHASE[i]) % 4].  The six larger tensors sit at phases 0 / 2,
# so in even steps all of them are small (0.01 or 1e-9) and the total norm is decided by the two 3- and 6-element tensors: steps 2 and
# 6 stay below the clip threshold, every other step is far above it
PHASE = (0, 1, 0, 2, 0, 2, 0, 2, 1)
LAST_ABSENT = 3          # the last parameter has no gradient in the first 3 steps; parameter 0 never has one
NORM_RTOL = 2e-6         # derived: fixed-order tree sums of <= 2^20 squares, ~20 levels x 2^-24 on the sum, half of it on the root


def _initial():
    g = torch.Generator().manual_seed(1234)
    return [torch.randn(s, generator=g) for s in SHAPES]


def _gradients():
    """grads[step][i]: fp32 tensor or None; the scale cycles through SCALES per (parameter, step), see PHASE."""
    g = torch.Generator().manual_seed(4321)
    out = []
    for t in range(STEPS):
        row = []
        for i, s in enumerate(SHAPES):
            x = torch.randn(s, generator=g) * SCALES[(t + PHASE[i]) % 4]
            row.append(None if i == 0 or (i == len(SHAPES) - 1 and t < LAST_ABSENT) else x)
        out.append(row)
    return out


def _lr_at(t):
    return LR if t < 5 else LR / 2        # halved after step 5


def _torch_cpu_run(dtype, wd):
    """clip_grad_norm_ + torch.optim.Adam on the CPU in `dtype`: per step the norm and the clipped gradients, at the end the state."""
    params = [torch.nn.Parameter(x.to(dtype)) for x in _initial()]
    opt = torch.optim.Adam(params, lr=LR, weight_decay=wd)
    norms, clipped = [], []
    for t, row in enumerate(_gradients()):
        opt.param_groups[0]["lr"] = _lr_at(t)
        for p, g in zip(params, row):
            p.grad = None if g is None else g.to(dtype)
        norms.append(torch.nn.utils.clip_grad_norm_(params, MAX_NORM).double())
        clipped.append([None if p.grad is None else p.grad.detach().clone() for p in params])
        opt.step()
    return dict(params=[p.detach() for p in params], norms=norms, clipped=clipped,
                exp_avg=[opt.state[p].get("exp_avg") for p in params], exp_avg_sq=[opt.state[p].get("exp_avg_sq") for p in params],
                steps=[float(opt.state[p]["step"]) if "step" in opt.state[p] else None for p in params])


_REF = {}


def _reference(wd):
    """fp64 run, and E of the fp32 run against it (computed once per weight decay, shared by the tests, never modified)."""
    if wd not in _REF:
        r64, r32 = _torch_cpu_run(torch.float64, wd), _torch_cpu_run(torch.float32, wd)
        E = 0.0
        for key in ("params", "exp_avg", "exp_avg_sq"):
            for a, b in zip(r32[key], r64[key]):
                if a is not None:
                    E = max(E, float((a.double() - b).abs().max()))
        assert r64["steps"] == [None] + [float(STEPS)] * (len(SHAPES) - 2) + [float(STEPS - LAST_ABSENT)]
        _REF[wd] = (r64, E, max(float(abs(a - b) / b) for a, b in zip(r32["norms"], r64["norms"])))
    return _REF[wd]


def _ulp(ref64):
    a = ref64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _excess(got, ref64, E):
    """max of |got - ref| - (4 E + ulp(ref)) over the tensor: <= 0 passes.  Also returns the plain max error."""
    d = (got.detach().double().cpu() - ref64).abs()
    return float((d - (4 * E + _ulp(ref64))).max()), float(d.max())


def _flat_run(dev, wd, max_grad_norm=MAX_NORM, separate_clip=False, first=0, last=STEPS, start=None, load=None):
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam
    params = [torch.nn.Parameter(x.clone().to(dev)) for x in (start if start is not None else _initial())]
    bucket = parallel.FlatGradBucket(params)
    opt = FlatAdam(bucket, lr=LR, weight_decay=wd, max_grad_norm=max_grad_norm)
    if load is not None:
        opt.load_state_dict(load)
    norms, clipped = [], []
    grads = _gradients()
    for t in range(first, last):
        opt.param_groups[0]["lr"] = _lr_at(t)
        for p, g in zip(params, grads[t]):
            p.grad = None if g is None else g.to(dev)
        if separate_clip:                      # the training loop's order: all_reduce (packs, keeps grad = None where there is none), clip, step
            bucket.all_reduce()
            norms.append(bucket.clip_grad_norm_(MAX_NORM).clone())
            opt.step()
        else:
            opt.step()
            norms.append(opt.last_grad_norm.clone())
        clipped.append([None if p.grad is None else p.grad.detach().clone() for p in params])
    return dict(params=params, opt=opt, bucket=bucket, norms=norms, clipped=clipped)


def _check_against(run, r64, E, tag):
    """Parameters, moments, clipped gradients and steps of a FlatAdam run against the fp64 run, to the 4 E + ulp rule."""
    opt, worst = run["opt"], {}
    for i, p in enumerate(run["params"]):
        st = opt.state[p] if p in opt.state else {}
        if r64["steps"][i] is None:
            assert len(st) == 0, i
            continue
        assert float(st["step"]) == r64["steps"][i], (i, float(st["step"]))
        for key, got, ref in (("param", p, r64["params"][i]), ("exp_avg", st["exp_avg"], r64["exp_avg"][i]),
                              ("exp_avg_sq", st["exp_avg_sq"], r64["exp_avg_sq"][i])):
            ex, err = _excess(got, ref, E)
            worst[key] = max(worst.get(key, 0.0), err)
            assert ex <= 0.0, (tag, key, i, err, E)
    for t, row in enumerate(run["clipped"]):
        for i, g in enumerate(row):
            assert (g is None) == (r64["clipped"][t][i] is None), (t, i)
            if g is not None:
                ex, err = _excess(g, r64["clipped"][t][i], E)
                worst["grad"] = max(worst.get("grad", 0.0), err)
                assert ex <= 0.0, (tag, "grad", t, i, err, E)
    print("%s: E(fp32 torch vs fp64) %.3g; FlatAdam max errors %s" % (tag, E, {k: "%.3g" % v for k, v in worst.items()}))
    return worst


# ---- 1. against torch in fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", WDS)
def test_matches_torch_adam_fp64(hip_device, wd):
    """clip_grad_norm_(10) + torch.optim.Adam on the CPU in fp64, same fp32 gradients: every parameter, moment and clipped gradient
    within 4 E + 1 ulp (E: torch's own CPU fp32 run against the fp64 run, measured here), the norm of every step within 2e-6 relative,
    per-parameter steps [none, 8, ..., 8, 5] as torch's, parameter 0 untouched bit for bit.
    Observed on the MI355X (E = 7.2e-7 / 6.7e-7 / 6.9e-7 at weight decay 0 / 3e-7 / 0.1): parameters 7.2e-7 / 6.7e-7 / 6.9e-7 (the fp32
    rounding of values up to 4.07), exp_avg 3.7e-8 / 3.2e-8 / 4.9e-8, exp_avg_sq 1.8e-8 / 2.0e-8 / 1.8e-8, clipped gradients 3.7e-7, norm
    8.2e-8 relative (torch's CPU fp32 norm: 1.8e-7)."""
    r64, E, norm_rel32 = _reference(wd)
    init = _initial()
    run = _flat_run(hip_device, wd)
    _check_against(run, r64, E, "wd=%g" % wd)
    rel = max(float(abs(n.double().cpu() - ref) / ref) for n, ref in zip(run["norms"], r64["norms"]))
    print("norm: FlatAdam max relative error %.3g (torch CPU fp32: %.3g)" % (rel, norm_rel32))
    assert rel <= NORM_RTOL, rel
    opt = run["opt"]
    assert torch.equal(run["params"][0].detach().cpu(), init[0])
    assert float(opt.exp_avg[0]) == 0.0 and float(opt.exp_avg_sq[0]) == 0.0 and float(opt._steps[0]) == 0.0
    assert [float(s) for s in opt._steps.cpu()] == [0.0] + [8.0] * (len(SHAPES) - 2) + [5.0]


# ---- 2. max_grad_norm=None --------------------------------------------------------------------------------------------------------
def test_separate_clip_gives_the_same_update(hip_device):
    wd = 3e-7
    r64, E, _ = _reference(wd)
    run = _flat_run(hip_device, wd, max_grad_norm=None, separate_clip=True)
    _check_against(run, r64, E, "separate clip")
    rel = max(float(abs(n.double().cpu() - ref) / ref) for n, ref in zip(run["norms"], r64["norms"]))
    assert rel <= NORM_RTOL, rel


def test_without_a_clip_the_gradient_buffer_is_only_read(hip_device):
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam
    params = [torch.nn.Parameter(x.to(hip_device)) for x in _initial()]
    bucket = parallel.FlatGradBucket(params)
    opt = FlatAdam(bucket, lr=LR, max_grad_norm=None)
    for p, g in zip(params, _gradients()[1]):           # (norm far above 10: a clip would rescale)
        p.grad = None if g is None else g.to(hip_device)
    bucket.pack()
    before = bucket.flat.clone()
    opt.step()
    assert torch.equal(bucket.flat, before)
    ref = torch.linalg.vector_norm(before.double())
    assert float(ref) > MAX_NORM and abs(float(opt.last_grad_norm) - float(ref)) <= NORM_RTOL * float(ref)
    assert float(opt.state[params[1]]["step"]) == 1.0   # the step count moves without a clip too


# ---- 3. bitwise repeatability -----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(hip_device):
    a, b = _flat_run(hip_device, 3e-7), _flat_run(hip_device, 3e-7)
    for x, y in zip(a["params"], b["params"]):
        assert torch.equal(x, y)
    assert torch.equal(a["opt"].exp_avg, b["opt"].exp_avg) and torch.equal(a["opt"].exp_avg_sq, b["opt"].exp_avg_sq)
    assert torch.equal(a["opt"]._steps, b["opt"]._steps)
    assert torch.equal(torch.stack(a["norms"]), torch.stack(b["norms"]))
    assert torch.equal(a["bucket"].flat, b["bucket"].flat)


# ---- 4. state_dict interchange ----------------------------------------------------------------------------------------------------
def test_state_dict_interchange_with_torch_adam(hip_device):
    """4 steps of torch.optim.Adam(fused=True) on the device, its state loaded into FlatAdam, 4 more steps with both: equal to the rule of
    test 1; FlatAdam's state_dict loads back into a fresh torch.optim.Adam; the loaded moments still alias the flat buffers."""
    wd, half = 3e-7, 4
    _, E, _ = _reference(wd)
    grads = _gradients()
    tparams = [torch.nn.Parameter(x.to(hip_device)) for x in _initial()]
    topt = torch.optim.Adam(tparams, lr=LR, weight_decay=wd, fused=True)

    def torch_steps(first, last):
        for t in range(first, last):
            topt.param_groups[0]["lr"] = _lr_at(t)
            for p, g in zip(tparams, grads[t]):
                p.grad = None if g is None else g.to(hip_device)
            torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM)
            topt.step()

    torch_steps(0, half)
    saved = copy.deepcopy(topt.state_dict())
    run = _flat_run(hip_device, wd, first=half, last=STEPS, start=[p.detach().cpu() for p in tparams], load=saved)
    torch_steps(half, STEPS)
    opt = run["opt"]
    lo, hi = opt.exp_avg.data_ptr(), opt.exp_avg.data_ptr() + 4 * opt.exp_avg.numel()
    worst = 0.0
    for i, (p, q) in enumerate(zip(run["params"], tparams)):
        if i == 0:
            assert p not in opt.state or len(opt.state[p]) == 0
            assert torch.equal(p, q)
            continue
        assert lo <= opt.state[p]["exp_avg"].data_ptr() < hi, i
        assert float(opt.state[p]["step"]) == float(topt.state[q]["step"]), i
        for got, ref in ((p, q), (opt.state[p]["exp_avg"], topt.state[q]["exp_avg"]),
                         (opt.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"])):
            ex, err = _excess(got, ref.detach().double().cpu(), E)
            worst = max(worst, err)
            assert ex <= 0.0, (i, err, E)
    print("after load_state_dict + 4 steps: max |FlatAdam - torch fused| %.3g (E %.3g)" % (worst, E))
    # and back: a fresh torch Adam takes FlatAdam's state
    fresh_params = [torch.nn.Parameter(p.detach().clone()) for p in run["params"]]
    fresh = torch.optim.Adam(fresh_params, lr=LR, weight_decay=wd, fused=True)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert fresh.param_groups[0]["lr"] == _lr_at(STEPS - 1) and fresh.param_groups[0]["weight_decay"] == wd
    for i, (p, q) in enumerate(zip(run["params"], fresh_params)):
        if i == 0:
            assert len(fresh.state[q]) == 0
            continue
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(fresh.state[q][key], opt.state[p][key]), (i, key)
    for q, g in zip(fresh_params, grads[0]):
        q.grad = None if g is None else g.to(hip_device)
    fresh.step()                                          # (usable as it is: one more torch step runs)
    assert float(fresh.state[fresh_params[1]]["step"]) == STEPS + 1


# ---- 5. one library call ----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _count_calls():
    """Every launching C-ABI call the Python thread makes, by name (the wrapping of tests/test_hip_eval_head.py)."""
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


def test_one_library_call_per_step_and_no_flag_upload_in_steady_state(hip_device):
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam
    params = [torch.nn.Parameter(x.to(hip_device)) for x in _initial()]
    bucket = parallel.FlatGradBucket(params)
    opt = FlatAdam(bucket, lr=LR, weight_decay=3e-7, max_grad_norm=MAX_NORM)
    grads = _gradients()

    def give(t):
        for p, g in zip(params, grads[t]):
            p.grad = None if g is None else g.to(hip_device)

    give(0)
    with _count_calls() as seen:
        opt.step()
    assert seen == {"stage_flat_adam_step": 1}, seen
    assert opt.flag_uploads == 1
    give(1)
    with _count_calls() as seen:
        opt.step()
    assert seen == {"stage_flat_adam_step": 1}, seen
    assert opt.flag_uploads == 1                          # the same parameters carry a gradient: nothing copied
    give(LAST_ABSENT)                                     # the last parameter joins
    opt.step()
    assert opt.flag_uploads == 2
    assert [float(s) for s in opt._steps.cpu()] == [0.0] + [3.0] * (len(SHAPES) - 2) + [1.0]


def test_edges_no_gradient_zero_grad_and_malformed_state(hip_device):
    """A step in which no parameter has a gradient changes nothing and reports norm 0; zero_grad only drops gradients; load_state_dict
    runs the optimizer's hooks and refuses a state without Adam's keys."""
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam
    params = [torch.nn.Parameter(x.to(hip_device)) for x in _initial()]
    bucket = parallel.FlatGradBucket(params)
    opt = FlatAdam(bucket, lr=LR, max_grad_norm=MAX_NORM)
    for p, g in zip(params, _gradients()[0]):
        p.grad = None if g is None else g.to(hip_device)
    opt.step()
    assert float(opt.last_grad_norm) > 0.0
    before = [p.detach().clone() for p in params]
    steps = opt._steps.clone()
    opt.zero_grad()
    assert all(p.grad is None for p in params)
    with _count_calls() as seen:
        opt.step()
    assert not seen and float(opt.last_grad_norm) == 0.0 and torch.equal(opt._steps, steps)
    assert all(torch.equal(a, p) for a, p in zip(before, params))
    with pytest.raises(ValueError):
        opt.zero_grad(set_to_none=False)
    sd = copy.deepcopy(opt.state_dict())
    hooked = []
    opt.register_load_state_dict_pre_hook(lambda o, d: hooked.append("pre"))
    opt.register_load_state_dict_post_hook(lambda o: hooked.append("post"))
    opt.load_state_dict(sd)
    assert hooked == ["pre", "post"] and torch.equal(opt._steps, steps)
    m = opt.exp_avg.clone()
    opt.load_state_dict(opt.state_dict())                # its own state, whose tensors are the flat buffers themselves
    assert torch.equal(opt.exp_avg, m) and torch.equal(opt._steps, steps) and float(m.abs().max()) > 0.0
    del sd["state"][1]["exp_avg_sq"]
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)


# ---- 6. whole model ---------------------------------------------------------------------------------------------------------------
def _model_run(dev, which, steps=3):
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam
    from tvqaplus_amd.stage import STAGE
    fx = Fixture("tiny_train")
    model = STAGE(fx.opt)                                 # (the fixture's configuration has dropout 0)
    model.load_state_dict(fx.group("param"), strict=True)
    model.mha_dropout_override = 0.0
    model = model.to(dev).train()
    batch = fx.batch().to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    if which == "flat":
        opt = FlatAdam(bucket, lr=LR, weight_decay=3e-7, max_grad_norm=MAX_NORM)
    else:
        opt = torch.optim.Adam(params, lr=LR, weight_decay=3e-7, **{which: True})
    n, losses = len(batch.qid), []
    for _ in range(steps):
        torch.manual_seed(7)
        bucket.zero()
        (out, targets), att_loss, _, t_loss, _ = model(batch)
        loss = F.cross_entropy(out, targets, reduction="sum") * (1.0 * n / len(targets)) + 0.1 * att_loss + 0.5 * t_loss
        loss.backward()
        bucket.all_reduce()
        if which != "flat":
            bucket.clip_grad_norm_(MAX_NORM)
        opt.step()
        losses.append(loss.detach().double().cpu())
    return [p.detach().double().cpu() for p in params], losses


def test_three_model_steps_against_torch_fused_adam(hip_device):
    """tiny_train's model and batch, 3 steps from the same state: FlatAdam(max_grad_norm=10) against bucket.clip_grad_norm_(10) +
    Adam(fused=True).  Bound: 4 x the difference between torch's own fused=True and foreach=True runs (measured here) + one ulp, for
    the parameters and for the losses, which must be finite."""
    pf, lf = _model_run(hip_device, "fused")
    pe, le = _model_run(hip_device, "foreach")
    pn, ln = _model_run(hip_device, "flat")
    D = max(float((a - b).abs().max()) for a, b in zip(pf, pe))
    DL = max(float((a - b).abs()) for a, b in zip(lf, le))
    err = max(float((a - b).abs().max()) for a, b in zip(pn, pf))
    errl = max(float((a - b).abs()) for a, b in zip(ln, lf))
    print("params: fused vs foreach %.3g, FlatAdam vs fused %.3g; losses: %.3g, %.3g (%s)" % (D, err, DL, errl, [float(x) for x in ln]))
    assert all(bool(torch.isfinite(x)) for x in ln + lf)
    for a, b in zip(pn, pf):
        assert float(((a - b).abs() - (4 * D + _ulp(b))).max()) <= 0.0, (err, D)
    for a, b in zip(ln, lf):
        assert float((a - b).abs() - (4 * DL + _ulp(b))) <= 0.0, (errl, DL)
