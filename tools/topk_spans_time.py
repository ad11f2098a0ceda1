"""What the top-K span kernel and a training step with max_num_proposal > 1 cost: the numbers of the multi-proposal finding in
docs/findings.md.

  python tools/topk_spans_time.py [--bsz 16] [--li 300] [--reps 200] [--block 40] [--rounds 6] [--warmup 10] [--k 5]

1. Kernel: stage_gt_spans next to stage_gt_spans_topk at K = 1 / 5 / 8 on (bsz, 5, li, 2) scores, event-timed over `reps`
   back-to-back launches after a warm-up (us per launch, launch gaps included -- the kernels are latency class), three repeats each.
2. Step: the bench-shape training loop (synth.make_batch and the model options as bench.py builds them, stage.reference_loss, flat
   clip, torch's fused Adam) on ONE model whose max_num_proposal is switched between 1 and `k` in interleaved blocks of `block`
   steps; every block ends in one synchronisation and the host clock runs over the block.  The mean number of classifier rows per
   step is reported beside the time: a model whose temporal scores are still flat proposes nothing above the confidence threshold,
   and the step then differs by the span kernel and the longer read-back alone.

One JSON line per measurement.
"""
import argparse
import contextlib
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tvqaplus_amd import groups, parallel  # noqa: E402
from tvqaplus_amd.stage import STAGE, reference_loss  # noqa: E402
from tvqaplus_amd.synth import make_batch, make_opt  # noqa: E402

ATT_W, TS_W = 0.1, 0.5


def time_kernels(dev, N, Li, reps):
    g = torch.Generator().manual_seed(1)
    t = (torch.randn(N, 5, Li, 2, generator=g) * 3).to(dev)
    target = torch.randint(0, 5, (N,), generator=g).to(dev)
    st = torch.randint(0, Li, (N,), generator=g).to(dev)
    calls = [("stage_gt_spans", lambda: groups.gt_spans(t, target, st, st))]
    for K in (1, 5, 8):
        calls.append(("stage_gt_spans_topk K=%d" % K, lambda K=K: groups.gt_spans_topk(t, target, st, st, K)))
    for name, fn in calls:
        for _ in range(20):
            fn()
        us = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / reps)
        print(json.dumps(dict(kernel=name, N=N, Li=Li, us_per_launch=[round(u, 2) for u in us], reps=reps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, default=16)
    ap.add_argument("--li", type=int, default=300)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    time_kernels(dev, args.bsz, args.li, args.reps)

    torch.manual_seed(2018)
    opt = make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True, input_encoder_n_heads=0, cls_encoder_n_heads=0,
                   storage_dtype="fp32")
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt).to(dev).train()
    batch = make_batch(N=args.bsz, Li=args.li, Lr=20, Lw=50, Lqa=40, seed=2018, ragged=True, att_imgs=4, att_words=3).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    n = args.bsz
    rows = {1: [], args.k: []}

    def step(k):
        model.max_num_proposal = k
        bucket.zero()
        (outputs, targets), att_loss, _, temporal_loss, _ = model(batch)
        rows[k].append(len(targets))
        loss = reference_loss(outputs, targets, att_loss, temporal_loss, n, ATT_W, TS_W, scale=1.0 * n / len(targets))
        loss.backward()
        bucket.all_reduce()
        bucket.clip_grad_norm_(10.0)
        optimizer.step()

    variants = (1, args.k)
    for k in variants:
        for _ in range(args.warmup):
            step(k)
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    blocks = {k: [] for k in variants}
    for r in range(args.rounds):
        for k in (variants if r % 2 == 0 else variants[::-1]):
            rows[k].clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.block):
                step(k)
            torch.cuda.synchronize()
            blocks[k].append(((time.perf_counter() - t0) * 1e3 / args.block, sum(rows[k]) / len(rows[k])))
    med = {k: statistics.median(b[0] for b in blocks[k]) for k in variants}
    for k in variants:
        print(json.dumps(dict(max_num_proposal=k, median_ms_per_step=round(med[k], 4), blocks_ms_per_step=[round(b[0], 4) for b in blocks[k]],
                              mean_rows_per_step=[round(b[1], 2) for b in blocks[k]], block_steps=args.block, bsz=args.bsz)), flush=True)
    spread = max(b[0] for b in blocks[1]) - min(b[0] for b in blocks[1])
    print(json.dumps(dict(summary="topk_spans_time", k=args.k, k1_spread_ms=round(spread, 4),
                          k_minus_1_ms=round(med[args.k] - med[1], 4))), flush=True)


if __name__ == "__main__":
    main()
