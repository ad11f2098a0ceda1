"""What the per-step logging of the caller's loop costs, and what the run meter costs instead: the numbers of docs/findings.md entry 69.

  python tools/meter_time.py [--bsz 16] [--block 50] [--rounds 6] [--warmup 10] [--read_every 100]

The bench-shape training loop (synth.make_batch and the model options as bench.py builds them, stage.reference_loss, flat clip,
torch's fused Adam), three variants in ONE process, in interleaved blocks of `block` steps:

  none    no logging lines at all (the loop bench.py times)
  items   the literal main.py:69-74 behind the step: loss.data.item(), float(att_loss), float(temporal_loss), cls_loss.item(),
          pred_ids.eq(targets.data).tolist() -- five blocking read-backs.  reference_loss does not leave the weighted parts behind,
          so this variant forms them under no_grad first (main.py:55-59's three lines), as a loop that logs them has to
  meter   reference_loss(meter=m) + m.update_grad_norm(norm), m.read() + m.reset() every `read_every` steps

Every block ends in one synchronisation; the host clock runs over the block.  One JSON line per variant (median ms / step over its
blocks and the blocks themselves) and a summary line: meter - none and items - none against the block-to-block spread of `none`.
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
from tvqaplus_amd.meter import RunMeter  # noqa: E402
from tvqaplus_amd.stage import STAGE, reference_loss  # noqa: E402
from tvqaplus_amd.synth import make_batch, make_opt  # noqa: E402

ATT_W, TS_W = 0.1, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsz", type=int, default=16)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--read_every", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(2018)
    opt = make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True, input_encoder_n_heads=0, cls_encoder_n_heads=0,
                   storage_dtype="fp32")
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt).to(dev).train()
    batch = make_batch(N=args.bsz, Li=300, Lr=20, Lw=50, Lqa=40, seed=2018, ragged=True, att_imgs=4, att_words=3).to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    criterion = torch.nn.CrossEntropyLoss(reduction="sum")
    meter = RunMeter(dev)
    meter.reset()
    n = args.bsz
    log = dict(loss=[], att=[], ts=[], cls=[], corrects=[])
    metered = [0]

    def step(variant):
        bucket.zero()
        (outputs, targets), att_loss, _, temporal_loss, _ = model(batch)
        scale = 1.0 * n / len(targets)
        loss = reference_loss(outputs, targets, att_loss, temporal_loss, n, ATT_W, TS_W, scale=scale,
                              meter=meter if variant == "meter" else None)
        loss.backward()
        bucket.all_reduce()
        norm = bucket.clip_grad_norm_(10.0)
        optimizer.step()
        if variant == "items":
            with torch.no_grad():
                att_w = ATT_W * att_loss
                ts_w = TS_W * temporal_loss
                cls_loss = criterion(outputs, targets) * scale
            log["loss"].append(loss.data.item())
            log["att"].append(float(att_w))
            log["ts"].append(float(ts_w))
            log["cls"].append(cls_loss.item())
            pred_ids = outputs.data.max(1)[1]
            log["corrects"] += pred_ids.eq(targets.data).tolist()
        elif variant == "meter":
            meter.update_grad_norm(norm)
            metered[0] += 1
            if metered[0] % args.read_every == 0:
                state = meter.read()
                meter.reset()
                assert state.steps == args.read_every and state.nonfinite_steps == 0, (state.steps, state.nonfinite_steps)

    variants = ("none", "items", "meter")
    for v in variants:
        for _ in range(args.warmup):
            step(v)
    torch.cuda.synchronize()
    gc.collect()
    gc.freeze()
    blocks = {v: [] for v in variants}
    for r in range(args.rounds):
        order = variants[r % 3:] + variants[:r % 3]          # every variant takes every position of a round
        for v in order:
            for k in log:
                log[k].clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.block):
                step(v)
            torch.cuda.synchronize()
            blocks[v].append((time.perf_counter() - t0) * 1e3 / args.block)
    med = {v: statistics.median(blocks[v]) for v in variants}
    for v in variants:
        print(json.dumps(dict(variant=v, median_ms_per_step=round(med[v], 4), blocks_ms_per_step=[round(b, 4) for b in blocks[v]],
                              block_steps=args.block, bsz=args.bsz)), flush=True)
    spread = max(blocks["none"]) - min(blocks["none"])
    print(json.dumps(dict(summary="meter_time", none_spread_ms=round(spread, 4), meter_minus_none_ms=round(med["meter"] - med["none"], 4),
                          items_minus_none_ms=round(med["items"] - med["none"], 4),
                          meter_within_spread_of_none=bool(abs(med["meter"] - med["none"]) <= spread),
                          read_every=args.read_every)), flush=True)


if __name__ == "__main__":
    main()
