"""Times the two consumers of the attention map that csrc/score_rows.hip serves, at the bench shape, on the GPU:

  predict   att_host.get_att_prediction on a resident (16, 5, 300, 40, 20) map, 20 annotated images per example and 5 vocabulary
            words per statement (K = 8000 rows)
  hard      bench.py's training step and batch with batch.use_hard_negatives = True

Each is timed on the host route (the code a tree without the row kernels runs: the whole-map read-back and Python loop; the gather
+ .cpu() + numpy sort) and on the device route, ALTERNATING blocks of --iters calls in one process (--rounds blocks each), a host
clock around work that ends in a device synchronise.  --root PATH times another checkout of this project (one without the device
route reports the host route only).  --trace: few iterations of the device routes only, for a rocprofv3 --kernel-trace --stats run.
One JSON line on stdout."""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--what", choices=("predict", "hard", "both"), default="both")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np
import torch

import bench
from tvqaplus_amd import att_host, parallel
from tvqaplus_amd.stage import STAGE
from tvqaplus_amd.synth import make_batch, make_opt

if not torch.cuda.is_available():
    sys.exit("score_rows_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
HAS_DEVICE_ROUTE = hasattr(att_host, "build_hard_plan")
ROUTES = (["device"] if args.trace else ["host", "device"]) if HAS_DEVICE_ROUTE else ["host"]
if args.trace:
    args.warmup, args.iters, args.rounds = 2, 3, 1


@contextlib.contextmanager
def route(name):
    """host: switch the device route off the way a shape outside it would (nothing else changes)."""
    if name == "device" or not HAS_DEVICE_ROUTE:
        yield
        return
    keep = att_host._score_rows_ok, att_host.build_hard_plan
    att_host._score_rows_ok, att_host.build_hard_plan = (lambda s: False), (lambda *a, **k: None)
    try:
        yield
    finally:
        att_host._score_rows_ok, att_host.build_hard_plan = keep


def timed(fn):
    """ms per call: --warmup calls, then --rounds alternating blocks of --iters calls per route, each call ended by a synchronise."""
    out = {r: [] for r in ROUTES}
    for r in ROUTES:
        with route(r):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in ROUTES:
            with route(r):
                for _ in range(args.iters):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    out[r].append((time.perf_counter() - t) * 1e3)
    return {r: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3),
                    block_medians_ms=[round(statistics.median(v[i:i + args.iters]), 3) for i in range(0, len(v), args.iters)])
            for r, v in out.items()}


rec = {"root": os.path.abspath(args.root), "device_route_present": HAS_DEVICE_ROUTE, "iters": args.iters, "rounds": args.rounds}

if args.what in ("predict", "both"):
    N, NA, Li, Lqa, Lr, n_img, n_voc = 16, 5, 300, 40, 20, 20, 5
    g = torch.Generator().manual_seed(2018)
    scores = (torch.randn(N, NA, Li, Lqa, Lr, generator=g) * 0.12).clamp_(-1, 1).to(dev)       # cosine-like: ~5 % of the scores >= 0.2
    words = torch.randint(100, 30000, (N, NA, Lqa), generator=g)
    for b in range(N):
        for a in range(NA):
            words[b, a, torch.randperm(Lqa, generator=g)[:n_voc]] = torch.randint(1, 51, (n_voc,), generator=g)
    kw = dict(object_vocab=list(range(1, 51)), words=words, vid_names=["v%d" % b for b in range(N)], qids=list(range(N)),
              img_indices=[list(range(Li))] * N, boxes=[[[[i, r, r + 1, r + 2] for r in range(Lr)] for i in range(n_img)]] * N,
              start_indices=[7] * N)
    res = {}

    def predict():
        res["out"] = att_host.get_att_prediction(scores, **kw)
    K = N * NA * n_img * n_voc
    rec["predict"] = dict(timed(predict), rows=K, d2h_bytes_host_route=scores.numel() * 4, d2h_bytes_device_route=K * (2 * Lr + 1) * 4,
                          detections=sum(len(d) for q in res["out"] for d in q.values()),
                          boxes=sum(len(x["pred"]) for q in res["out"] for d in q.values() for x in d))
    if len(ROUTES) == 2:      # the two routes return the same thing
        with route("host"):
            host = att_host.get_att_prediction(scores, **kw)
        rec["predict"]["routes_equal"] = host == res["out"]
    del scores

if args.what in ("hard", "both"):
    torch.manual_seed(2018)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(make_opt(hsz=128, add_local=True, dropout=0.1, use_sup_att=True)).to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
    batch = make_batch(N=16, Li=300, Lr=20, Lw=50, Lqa=40, seed=2018, att_imgs=4, att_words=3).to(dev)
    batch.use_hard_negatives = True
    rec["hard_step"] = timed(lambda: bench.train_step(model, batch, bucket, params, optimizer, 16))

print(json.dumps(rec))
