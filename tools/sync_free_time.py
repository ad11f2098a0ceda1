"""What the proposal read-back costs a training step, and what opt.device_proposals costs instead: the numbers of docs/findings.md
entry 74.

  python tools/sync_free_time.py [--bsz 16 4 2] [--block 40] [--rounds 6] [--warmup 10]

The bench-shape training loop (synth.make_batch and the model options as bench.py builds them, stage.reference_loss, flat clip,
torch's fused Adam) per batch size, two variants in ONE process on ONE model, in interleaved blocks of `block` steps:

  off   model.device_proposals = False: the span table is read back, proposal_rows runs on the host, the rows are uploaded;
        scale = n / len(targets) on the host (the loop bench.py times)
  on    model.device_proposals = True: the decision kernel, (max_num_proposal + 1) * n rows, scale = model.last_proposals.scale

Rounds alternate the order (off, on / on, off), so each variant takes each position equally often.  Every block ends in one
synchronisation; the host clock runs over the block.  One JSON line per (batch size, variant) -- median ms / step over its blocks,
the blocks themselves, the rows the classifier saw -- and one summary line per batch size: on - off against the block-to-block
spread of `off`.  The numbers are written down as they come, a loss included.
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

from tvqaplus_amd import parallel  # noqa: E402
from tvqaplus_amd.stage import STAGE, reference_loss  # noqa: E402
from tvqaplus_amd.synth import make_batch, make_opt  # noqa: E402

ATT_W, TS_W = 0.1, 0.5


def measure(bsz, args, dev):
    torch.manual_seed(2018)
    opt = make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True, input_encoder_n_heads=0, cls_encoder_n_heads=0,
                   storage_dtype="fp32")
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt).to(dev).train()
    batch = make_batch(N=bsz, Li=300, Lr=20, Lw=50, Lqa=40, seed=2018, ragged=True, att_imgs=4, att_words=3).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    rows = {}

    def step(variant):
        model.device_proposals = variant == "on"
        bucket.zero()
        (outputs, targets), att_loss, _, temporal_loss, _ = model(batch)
        scale = model.last_proposals.scale if variant == "on" else 1.0 * bsz / len(targets)
        loss = reference_loss(outputs, targets, att_loss, temporal_loss, bsz, ATT_W, TS_W, scale=scale)
        loss.backward()
        bucket.all_reduce()
        bucket.clip_grad_norm_(10.0)
        optimizer.step()
        rows[variant] = len(targets)
        assert model.last_proposals.on_device == (variant == "on")

    variants = ("off", "on")
    for v in variants:
        for _ in range(args.warmup):
            step(v)
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    blocks = {v: [] for v in variants}
    for r in range(args.rounds):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.block):
                step(v)
            torch.cuda.synchronize()
            blocks[v].append((time.perf_counter() - t0) * 1e3 / args.block)
    gc.unfreeze()
    med = {v: statistics.median(blocks[v]) for v in variants}
    for v in variants:
        print(json.dumps(dict(variant=v, bsz=bsz, median_ms_per_step=round(med[v], 4),
                              blocks_ms_per_step=[round(b, 4) for b in blocks[v]], block_steps=args.block, classifier_rows=rows[v])),
              flush=True)
    spread = max(blocks["off"]) - min(blocks["off"])
    print(json.dumps(dict(summary="sync_free_time", bsz=bsz, off_spread_ms=round(spread, 4),
                          on_minus_off_ms=round(med["on"] - med["off"], 4),
                          on_over_off=round(med["on"] / med["off"], 4),
                          beyond_spread_of_off=bool(abs(med["on"] - med["off"]) > spread))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, nargs="+", default=[16, 4, 2])
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    for bsz in args.bsz:
        measure(bsz, args, dev)


if __name__ == "__main__":
    main()
