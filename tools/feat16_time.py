"""Half-precision features in the fp32 model (csrc/feat16.hip): the numbers of docs/findings.md entry 64.

  python tools/feat16_time.py [--bsz 16] [--steps 20] [--warmup 5] [--what stage,step]

stage  first stage of the input MLP at the bench's LIVE context rows (the ragged layout's row tables of the bench batch), subtitle
       stream (K0 768) and video stream (K0 300, L2-normalised): the fp32 entry points on the upcast rows (stage_l2norm_gather_fwd +
       stage_layernorm_fwd / stage_layernorm_gather_fwd, and their backward) against stage_feat16_ln_{fwd,bwd} on the fp16 rows.
       HIP events around each call, old / new alternating, `warmup` unrecorded runs, then median [min .. max] of `steps`.
step   training step with the loader in the loop: pinned host batches through BatchPrefetcher into the fp32 model, features stored
       as float32 and as float16: ms / step (host clock around `steps` steps ending in a synchronise), bytes copied per step, peak
       device memory.
One JSON line per measurement.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tvqaplus_amd import _lib, parallel  # noqa: E402
from tvqaplus_amd.prefetch import BatchPrefetcher  # noqa: E402
from tvqaplus_amd.stage import STAGE, reference_loss  # noqa: E402
from tvqaplus_amd.synth import Batch, make_batch, make_opt  # noqa: E402

FEATURES = ("qas_bert", "sub_bert", "vid")
EPS_LN, EPS_L2, P, SEED = 1e-5, 1e-12, 0.1, 20181


def build(args, dev):
    torch.manual_seed(2018)
    opt = make_opt(hsz=128, add_local=True, dropout=P, use_sup_att=True)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt).to(dev).train()
    host = make_batch(N=args.bsz, Li=300, Lr=20, Lw=50, Lqa=40, seed=2018, att_imgs=4, att_words=3)
    return model, host


def stats(ts):
    return dict(median_us=round(statistics.median(ts) * 1e3, 1), min_us=round(min(ts) * 1e3, 1), max_us=round(max(ts) * 1e3, 1))


def time_stage(args, model, host, dev):
    lib = _lib.load()
    with torch.no_grad():
        model(host.to(dev))                                   # one forward: the layout's row tables of this batch
    st = torch.cuda.current_stream().cuda_stream
    for name, key, l2 in (("sub", "sub_bert", 0), ("vid", "vid", 1)):
        clay = model.last_ragged_ctx.get(name)
        if clay is None:
            print(json.dumps({"stage": name, "error": "stream not ragged for this batch"}))
            continue
        x32 = host[key].to(dev)
        x16 = x32.half()
        x32 = x16.float()                                     # the upcast rows: the same values
        K0, M, src = x32.shape[-1], clay.U, clay.src_rows
        f = lambda *s: torch.empty(*s, device=dev)
        gamma, beta, dy = torch.rand(K0, device=dev) + 0.5, torch.rand(K0, device=dev), torch.randn(M, K0, device=dev)
        y, mean, rstd, xn, dg, db = f(M, K0), f(M), f(M), f(M, K0), f(K0), f(K0)
        ws_b = lib.stage_ln_bwd_ws_bytes(K0)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
        a = lambda t: t.data_ptr()

        def old_fwd():
            if l2:
                _lib.check(lib.stage_l2norm_gather_fwd(a(x32), a(src), a(xn), M, K0, EPS_L2, st), "l2")
                _lib.check(lib.stage_layernorm_fwd(a(xn), None, 0, None, a(gamma), a(beta), a(y), a(mean), a(rstd), M, K0, EPS_LN, P, SEED, st), "ln")
            else:
                _lib.check(lib.stage_layernorm_gather_fwd(a(x32), a(src), a(gamma), a(beta), a(y), a(mean), a(rstd), M, K0, EPS_LN, P, SEED, st), "ln")

        def new_fwd():
            _lib.check(lib.stage_feat16_ln_fwd(a(x16), _lib.STAGE_DT_F16, a(src), a(gamma), a(beta), a(y), a(mean), a(rstd), M, K0, l2, EPS_LN,
                                               EPS_L2, P, SEED, st), "feat16 fwd")

        def old_bwd():
            if l2:
                _lib.check(lib.stage_layernorm_bwd(a(dy), a(xn), a(mean), a(rstd), a(gamma), None, None, a(dg), a(db), M, K0, P, SEED, a(ws), ws_b,
                                                   st), "ln bwd")
            else:
                _lib.check(lib.stage_layernorm_gather_bwd(a(dy), a(x32), a(src), a(mean), a(rstd), a(gamma), a(dg), a(db), M, K0, P, SEED, a(ws),
                                                          ws_b, st), "ln bwd")

        def new_bwd():
            _lib.check(lib.stage_feat16_ln_bwd(a(dy), a(x16), _lib.STAGE_DT_F16, a(src), a(mean), a(rstd), a(dg), a(db), M, K0, l2, EPS_L2, P, SEED,
                                               a(ws), ws_b, st), "feat16 bwd")

        for what, old, new in (("fwd", old_fwd, new_fwd), ("bwd", old_bwd, new_bwd)):
            times = {"fp32_upcast": [], "fp16_in_place": []}
            for i in range(args.warmup + args.steps):
                for tag, fn in (("fp32_upcast", old), ("fp16_in_place", new)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if i >= args.warmup:
                        times[tag].append(e0.elapsed_time(e1))
            # bytes the algorithm needs: rows read (+ xn written and re-read with l2 on the fp32 path), y written / dy read
            rd = {"fp32_upcast": 4 * (3 if (l2 and what == "fwd") else 1), "fp16_in_place": 2}
            rec = dict(stage=name, what=what, rows=M, K0=K0, l2=l2)
            for tag, ts in times.items():
                s = stats(ts)
                s["GBps"] = round(M * K0 * (rd[tag] + 4) / (s["median_us"] * 1e-6) / 1e9, 0)
                rec[tag] = s
            print(json.dumps(rec), flush=True)


def time_step(args, model, host, dev):
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    n = len(host.qid)

    def step(batch):
        bucket.zero()
        (out, targets), att_loss, _, t_loss, _ = model(batch)
        loss = reference_loss(out, targets, att_loss, t_loss, n, 0.1, 0.5, scale=1.0 * n / len(targets))
        loss.backward()
        bucket.all_reduce()                                     # (one process: packs the gradients into the flat buffer)
        bucket.clip_grad_norm_(10.0)
        optimizer.step()

    state = {k: v.clone() for k, v in model.state_dict().items()}
    for tag, dt in (("fp32_features", torch.float32), ("fp16_features", torch.float16)):
        model.load_state_dict(state)
        pinned = Batch(host)                                    # the loader's batch: features stored in `dt`, everything pinned
        nbytes = 0
        for k, v in host.items():
            if torch.is_tensor(v):
                pinned[k] = (v.to(dt) if k in FEATURES else v).pin_memory()
                nbytes += pinned[k].numel() * pinned[k].element_size()
        total = args.warmup + args.steps
        feed = BatchPrefetcher((pinned for _ in range(total)), dev, feature_dtype=dt)
        for _ in range(args.warmup):
            step(next(feed))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(next(feed))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        print(json.dumps(dict(step=tag, ms_per_step=round(ms, 3), MB_copied_per_step=round(nbytes / 1e6, 1),
                              peak_MB=round(torch.cuda.max_memory_allocated() / 1e6, 1),
                              ragged_ctx=sorted(model.last_ragged_ctx))), flush=True)
        del feed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--what", default="stage,step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    model, host = build(args, dev)
    if "stage" in args.what:
        time_stage(args, model, host, dev)
    if "step" in args.what:
        time_step(args, model, host, dev)


if __name__ == "__main__":
    main()
