#!/usr/bin/env python
"""Link-inclusive training step with padded and with packed context features (tvqaplus_amd/packed.py), one process.

The bench batch (synth.make_batch defaults, seed 2018, bench.py's attention labels) and the bench training step (bench.train_step:
forward, fused loss, backward, clip, fused Adam).  In the first four columns every step takes its batch from PINNED host memory through
tvqaplus_amd.prefetch.BatchPrefetcher (the host tensors already have the column's feature type, as a dataset stored in that type would
deliver them: the staging copy is skipped and the column times the link, not a host conversion); the last two keep the batch resident.

    padded_fp32  padded_fp16  packed_fp32  packed_fp16  resident  resident_packed

Per column: ms/step (median over --rounds passes of --steps steps, each after --warmup steps; event-timed per step; the passes visit
the columns in rotated order and their medians are listed one by one; min / max and the 10th / 90th percentile are the column's own
spread), bytes sent per step, and -- packed columns -- the event-timed duration of stage_pack_unpack at the subtitle stream's shape
with the bytes it moves per second.  One JSON line per column: profiles/packed_h2d_b16.jsonl (and stdout).

    timeout -k 10 600 python tools/packed_h2d_time.py
"""
import argparse
import contextlib
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pin(batch):
    from tvqaplus_amd.packed import PackedFeatures
    for k, v in list(batch.items()):
        if torch.is_tensor(v):
            batch[k] = v.pin_memory()
        elif isinstance(v, PackedFeatures):
            batch[k] = PackedFeatures(v.data.pin_memory(), v.lens, v.L)
    return batch


def _sent_bytes(batch):
    from tvqaplus_amd.packed import PackedFeatures
    n = 0
    for v in batch.values():
        if torch.is_tensor(v):
            n += v.numel() * v.element_size()
        elif isinstance(v, PackedFeatures):
            n += v.nbytes
        elif isinstance(v, dict):
            n += sum(t.numel() * t.element_size() for t in v.values() if torch.is_tensor(t))
    return n


def _half(batch):
    out = type(batch)(batch)
    for k in ("qas_bert", "sub_bert", "vid"):
        out[k] = batch[k].to(torch.float16)
    return out


def _unpack_time(pf, reps=20, warm=3):
    """Event-timed stage_pack_unpack (image + mask) of a resident packed stream: (median ms, bytes read + written)."""
    from tvqaplus_amd import _lib
    from tvqaplus_amd.ops import _stream
    lib = _lib.load()
    N, Li, L, K = pf.shape
    rb = K * pf.data.element_size()
    ptab = torch.from_numpy(pf.ptab().reshape(-1)).to(pf.device)
    dense = torch.empty(N, Li, L, K, dtype=pf.dtype, device=pf.device)
    mask = torch.empty(N, Li, L, dtype=torch.float32, device=pf.device)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    cur = torch.cuda.current_stream()
    for i in range(warm + reps):
        if i >= warm:
            ev[i - warm][0].record(cur)
        _lib.check(lib.stage_pack_unpack(pf.data.data_ptr(), ptab.data_ptr(), dense.data_ptr(), mask.data_ptr(), N * Li, L, rb, _stream()),
                   "stage_pack_unpack")
        if i >= warm:
            ev[i - warm][1].record(cur)
    torch.cuda.synchronize()
    ms = statistics.median(a.elapsed_time(b) for a, b in ev)
    return ms, pf.P * rb + N * Li * L * rb + N * Li * L * 4 + 8 * N * Li


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="passes over the columns (rotated order); --steps timed steps per column and pass")
    ap.add_argument("--bsz", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_h2d_b16.jsonl"))
    args = ap.parse_args()
    assert args.steps >= 20 and args.warmup >= 5
    import bench
    from tvqaplus_amd import parallel
    from tvqaplus_amd.packed import pack_batch
    from tvqaplus_amd.prefetch import BatchPrefetcher
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    # ONE copy stream for every column, created before the model creates its branch streams: a new stream per prefetcher is mapped onto
    # the hardware queues anew, and whether the copy then overlaps the step would differ from column to column
    copy_stream = torch.cuda.Stream(device=device)
    torch.manual_seed(2018)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True)).to(device).train()
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    padded = make_batch(N=args.bsz, seed=2018, att_imgs=4, att_words=3)
    packed = pack_batch(padded, check=True)
    columns = [("padded_fp32", padded, True), ("padded_fp16", _half(padded), True), ("packed_fp32", packed, True),
               ("packed_fp16", _half(packed), True), ("resident", padded, False), ("resident_packed", packed, False)]
    gc.collect()
    # every column's source is set up ONCE (pinned host tensors / resident device tensors); the columns are then timed in --rounds
    # passes, each pass in a rotated order, so that a drift of the machine (other tenants on the host link, clocks) shows up as a
    # difference between a column's rounds instead of a difference between columns
    src, sent = {}, {}
    for name, host, fed in columns:
        sent[name] = _sent_bytes(host)
        src[name] = _pin(type(host)(host)) if fed else host.to(device)
    times = {name: [] for name, _, _ in columns}
    ctx, last_loss = {}, {}
    for rnd in range(args.rounds):
        order = columns[rnd % len(columns):] + columns[:rnd % len(columns)]
        for name, _, fed in order:
            if fed:
                feed = BatchPrefetcher((src[name] for _ in range(args.warmup + args.steps)), device, stream=copy_stream)
                nxt = lambda: next(feed)
            else:
                nxt = lambda: src[name]
            for _ in range(args.warmup):
                bench.train_step(model, nxt(), bucket, params, optimizer, args.bsz)
            gc.freeze()
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            cur = torch.cuda.current_stream()
            torch.cuda.synchronize()
            marks[0].record(cur)
            for i in range(args.steps):
                loss = bench.train_step(model, nxt(), bucket, params, optimizer, args.bsz)
                marks[i + 1].record(cur)
            torch.cuda.synchronize()
            times[name].append(sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)))
            ctx[name], last_loss[name] = sorted(model.last_ragged_ctx), float(loss.detach())
            del nxt
            if fed:
                del feed
            gc.unfreeze()
            gc.collect()
    records = []
    for name, _, fed in columns:
        ms = sorted(t for r in times[name] for t in r)
        rec = {"column": name, "bsz": args.bsz, "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup,
               "ms_per_step_median": round(statistics.median(ms), 4), "ms_median_by_round": [round(statistics.median(r), 4) for r in times[name]],
               "ms_min": round(ms[0], 4), "ms_p10": round(ms[len(ms) // 10], 4), "ms_p90": round(ms[-1 - len(ms) // 10], 4),
               "ms_max": round(ms[-1], 4), "bytes_sent_per_step": sent[name] if fed else 0, "batch_bytes": sent[name],
               "loss": last_loss[name], "ragged_ctx": ctx[name]}
        if "packed" in name:
            pf = src[name].sub_bert.to(device)
            t, moved = _unpack_time(pf)
            rec.update(unpack_sub_ms=round(t, 4), unpack_sub_bytes=moved, unpack_sub_GBps=round(moved / t / 1e6, 1),
                       unpack_sub_shape=list(pf.shape), unpack_sub_dtype=str(pf.dtype).replace("torch.", ""))
            del pf
        records.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
