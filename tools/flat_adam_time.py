"""FlatAdam against the clip + torch Adam it replaces, inside the training step (docs/findings.md entry 67).

  python tools/flat_adam_time.py [--bsz 16,2] [--steps 200] [--block 20] [--warmup 10]

One process; per batch size three copies of the bench model (same initial state, same resident batch), each with its own optimizer:

  A   bucket.clip_grad_norm_(10) + torch.optim.Adam(fused=True)      -- the sequence bench.py times
  A'  the same again                                                  -- the spread of A against itself
  B   tvqaplus_amd.optim.FlatAdam(max_grad_norm=10)                   -- bench.train_step unchanged: its bucket's clip is a no-op

`warmup` steps each, then blocks of `block` steps in the order A, B, A', A, B, A', ... until every configuration has `steps` timed steps.
Per block: host clock from the first issue to the end of a final synchronise (step ms) and to the end of issuing, minus the time spent
waiting in Event.synchronize (host issue ms, bench.py's definition).  Reported per configuration: mean over all steps, and median
[min .. max] of the per-block means.  One JSON line per batch size, then a table.

Launches per step come from a separate run under the profiler (never while timing):

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/flat_adam_time.py --only B --bsz 2 --warmup 3 --steps K
  python tools/flat_adam_time.py --count_db DIR/.../*.db          # dispatches in the trace

with two values of K: (count(K2) - count(K1)) / (K2 - K1) is the launches of one step without the start-up work.
"""
import argparse
import contextlib
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_db(path):
    import sqlite3
    c = sqlite3.connect(path)
    tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'") if r[0].startswith("rocpd_kernel_dispatch")]
    return sum(c.execute("select count(*) from %s" % t).fetchone()[0] for t in tabs)


def bench_defaults():
    """bench.py's own argument defaults (its model and batch shape), so that this tool follows them when they move."""
    import bench
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        return bench.parse()
    finally:
        sys.argv = argv


def build(bsz, dev):
    import torch
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    b = bench_defaults()
    torch.manual_seed(2018)       # bench.py: main()
    opt = make_opt(hsz=b.hsz, add_local=True, dropout=0.1, use_sup_att=not b.no_sup_att, input_encoder_n_heads=b.heads,
                   cls_encoder_n_heads=b.heads, storage_dtype=b.storage)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt)
    batch = make_batch(N=bsz, Li=b.frames, Lr=b.regions, Lw=b.sub_words, Lqa=b.qa_words, seed=2018, ragged=not b.dense,
                       att_imgs=b.att_imgs if not b.no_sup_att else 0, att_words=b.att_words).to(dev)
    return model.to(dev).train(), batch


def configure(model, which):
    import torch
    from tvqaplus_amd import parallel
    from tvqaplus_amd.optim import FlatAdam

    class NoClipBucket(parallel.FlatGradBucket):
        def clip_grad_norm_(self, max_norm, eps=1e-6):      # FlatAdam clips inside its step
            return None

    params = [p for p in model.parameters() if p.requires_grad]
    if which == "B":
        bucket = NoClipBucket(params)
        return params, bucket, FlatAdam(bucket, lr=1e-3, weight_decay=3e-7, max_grad_norm=10.0)
    return params, parallel.FlatGradBucket(params), torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)


def run_shape(args, bsz, dev, names):
    import torch
    import bench
    cfgs = {}
    for name in names:
        model, batch = build(bsz, dev)        # (the same seed: identical initial state and batch for every configuration)
        cfgs[name] = (model,) + configure(model, "B" if name == "B" else "A")
    n = len(batch.qid)

    def steps(name, k):
        model, params, bucket, optimizer = cfgs[name]
        for _ in range(k):
            bench.train_step(model, batch, bucket, params, optimizer, n, 1)

    gc.collect()
    for name in names:
        steps(name, args.warmup)
    torch.cuda.synchronize()
    gc.freeze()
    waits = [0.0]
    ev_sync = torch.cuda.Event.synchronize

    def timed_sync(self):
        t = time.perf_counter()
        ev_sync(self)
        waits[0] += time.perf_counter() - t
    torch.cuda.Event.synchronize = timed_sync
    rec = {name: dict(step=[], issue=[]) for name in names}
    try:
        for _ in range((args.steps + args.block - 1) // args.block):
            for name in names:
                torch.cuda.synchronize()
                waits[0] = 0.0
                t0 = time.perf_counter()
                steps(name, args.block)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                rec[name]["step"].append(1e3 * (t2 - t0) / args.block)
                rec[name]["issue"].append(1e3 * (t1 - t0 - waits[0]) / args.block)
    finally:
        torch.cuda.Event.synchronize = ev_sync
        gc.unfreeze()
    b = bench_defaults()
    out = dict(bsz=bsz, block=args.block, warmup=args.warmup,
               shape=dict(hsz=b.hsz, frames=b.frames, regions=b.regions, sub_words=b.sub_words, qa_words=b.qa_words, storage=b.storage))
    for name in names:
        out[name] = dict(timed_steps=len(rec[name]["step"]) * args.block)
        for key in ("step", "issue"):
            v = rec[name][key]
            out[name][key + "_ms"] = dict(mean=round(statistics.fmean(v), 4), median=round(statistics.median(v), 4),
                                          min=round(min(v), 4), max=round(max(v), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", default="16,2")
    ap.add_argument("--steps", type=int, default=200, help="timed steps per configuration (rounded up to whole blocks)")
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=("A", "B"), default=None, help="one configuration, --steps steps in one block (profiler runs)")
    ap.add_argument("--count_db", default=None, help="print the number of kernel dispatches in a rocprofv3 database and exit")
    args = ap.parse_args()
    if args.count_db:
        print(count_db(args.count_db))
        return
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    names = ["A", "B", "A'"] if args.only is None else [args.only]
    if args.only is not None:
        args.block = args.steps
    rows = []
    for bsz in [int(x) for x in args.bsz.split(",")]:
        out = run_shape(args, bsz, dev, names)
        print(json.dumps(out), flush=True)
        rows.append(out)
    print("%-4s %-3s %7s | %-36s | %-36s" % ("bsz", "cfg", "steps", "step ms  mean  median [min .. max]", "host issue ms  mean  median [min .. max]"))
    for out in rows:
        for name in names:
            s, i = out[name]["step_ms"], out[name]["issue_ms"]
            print("%-4d %-3s %7d | %8.3f %8.3f [%7.3f .. %7.3f] | %8.3f %8.3f [%7.3f .. %7.3f]" % (
                out["bsz"], name, out[name]["timed_steps"], s["mean"], s["median"], s["min"], s["max"], i["mean"], i["median"], i["min"], i["max"]))


if __name__ == "__main__":
    main()
