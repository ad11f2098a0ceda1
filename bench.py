#!/usr/bin/env python
"""bench.py -- QA-examples/sec (5-candidate fwd+bwd, full training step) of the MI355X-native STAGE at B=16 per GPU,
plus the K1 (StructuredAttention forward) roofline line and a CPU baseline of the same step (oracle port).

    python bench.py [--gpus N --steps K --warmup W]          # N=1 default
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W                # N>1: one rank per GPU over RCCL (driver does this)

Workload (BASELINE.json configs[1]): full STAGE, hsz=128, 300 frames x 20 regions, 50 subtitle
words/frame, 40 QA words, 5 candidates, global B=16 (the metric's "at B=16": --scaling strong, the default, shards the 16 examples
over the GPUs, SURVEY.md 8d / BASELINE.json configs[3]; --scaling weak keeps 16 examples PER GPU -- at N=1 the two are the same step),
--add_local --use_sup_att (run_main.sh:45 always passes it), dropout 0.1, fp32, synthetic ragged features seeded 2018.
One step = forward + loss (main.py:55-60: CE_sum * len(qids)/len(targets) + 0.1 * att_loss + 0.5 * temporal_loss, the ratio
taken over the GATHERED batch as the reference's DataParallel does) + backward + grad all-reduce (N>1) +
clip_grad_norm_(10) + Adam step, i.e. everything main.py:53-66 does per batch.  Inputs are resident in HBM.
Developer flags (not the headline line): --dense (all-ones masks), --heads 4, --no_sup_att, --h2d,
--storage bf16 (the bf16 storage mode of BASELINE.json configs[4] at these shapes; `dtype` then says "bf16").

A plain run sets up, warms up, times the --steps steps and prints the result line (metric, value, unit, higher_is_better, dtype,
ms_per_step, the host-side split of the timed steps).  --full adds everything else the record can hold, each after the timed steps:
the torch.profiler device-time pass, the K1 roofline lines (isolated launches and in-step events), the rocprofv3 counter passes,
the whole-step roofline, the child runs of side_records() and the CPU baseline; the --no_* flags still drop single parts of it.
--dump-outputs DIR writes what the last timed step computed (logits, targets, losses, temporal scores, the clipped gradient and the
updated parameters) as DIR/<name>.npy, float32 / float64; inputs and initial weights are seeded, so two builds can be compared.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bsz", type=int, default=16, help="examples per GPU")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--sub_words", type=int, default=50)
    ap.add_argument("--qa_words", type=int, default=40)
    ap.add_argument("--hsz", type=int, default=128)
    ap.add_argument("--dense", action="store_true", help="all-ones masks instead of ragged lengths")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong",
                    help="strong (default; the metric is quoted at B=16): --bsz examples in total, sharded over the GPUs (SURVEY 8d, "
                         "BASELINE configs[3]); weak: --bsz examples per GPU")
    ap.add_argument("--heads", type=int, default=0, help="self-attention heads in both encoders (BASELINE config 3: 4)")
    ap.add_argument("--no_sup_att", action="store_true", help="drop the supervised attention loss term (round-1 workload)")
    ap.add_argument("--att_imgs", type=int, default=4, help="annotated frames per question (synthetic att_labels)")
    ap.add_argument("--att_words", type=int, default=3, help="labelled object words per annotated frame")
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--storage", choices=["fp32", "bf16"], default="fp32",
                    help="bf16: the bf16 storage mode (BASELINE configs[4]); the headline line is the fp32 default")
    ap.add_argument("--streams", type=int, default=-1, choices=(-1, 0, 1, 2, 3, 4),
                    help="branch streams of the model (stage.py: use_streams; -1 = its default, 3): 0 one stream, 1 the statement branch on a "
                         "side stream, 2 + the video input MLP / encoder, 3 + the video attention with its forward fenced behind the subtitle "
                         "attention, 4 without the fence (fastest; the K1 forward kernels then run next to another branch and their in-step "
                         "timings stop being a statement about the kernel)")
    ap.add_argument("--fp32_inputs", action="store_true", help="--storage bf16: keep the resident feature tensors fp32 (the model then rounds them "
                    "to bf16 inside every step); default: resident as bf16, the way prefetch.BatchPrefetcher(stage_dtype=bf16) delivers them")
    ap.add_argument("--config", choices=("default", "stress"), default="default",
                    help="stress = BASELINE.json configs[4]: bf16 weights / activations with fp32 softmax accumulate, hsz = 256, 512 "
                         "subtitle words per frame (sets --hsz 256 --sub_words 512 --storage bf16; the roofline line is the long-row "
                         "attention kernel).  The headline line is the default config")
    ap.add_argument("--no_roofline", action="store_true")
    ap.add_argument("--gc", choices=("freeze", "default", "off"), default="freeze",
                    help="cyclic garbage collector during the timed steps: freeze (default) = gc.freeze() after the warm-up")
    ap.add_argument("--adam", choices=["fused", "foreach"], default="fused", help="torch.optim.Adam implementation (same update)")
    ap.add_argument("--clip", choices=["flat", "torch"], default="flat", help="clip_grad_norm_(10): on the packed gradient buffer "
                    "(parallel.FlatGradBucket.clip_grad_norm_: one reduction + one multiply) or torch.nn.utils.clip_grad_norm_ (same update)")
    ap.add_argument("--loss", choices=["fused", "eager"], default="fused", help="the training loop's loss line (main.py:55-60): "
                    "tvqaplus_amd.stage.reference_loss (one launch forward, the same value) or the eager torch expression (child record eager_loss)")
    ap.add_argument("--dump_steps", action="store_true", help="developer: add every timed step's duration (ms) to the record")
    ap.add_argument("--no_device_time", action="store_true", help="skip the torch.profiler pass behind device_ms_per_step")
    ap.add_argument("--only_roofline", action="store_true")
    ap.add_argument("--with_bwd", action="store_true", help="with --only_roofline: the fused K1 backward as well (the PMC child)")
    ap.add_argument("--no_pmc", action="store_true", help="do not measure `traffic` with rocprofv3 counter passes in this run")
    ap.add_argument("--cpu_seconds", type=float, default=20.0, help="CPU-baseline time budget")
    ap.add_argument("--cpu_all_threads", action="store_true", help="also time the CPU baseline on os.cpu_count() threads (minutes)")
    ap.add_argument("--cpu_probe_threads", type=int, default=0, help="internal: time a short CPU-oracle step at this thread count and exit")
    ap.add_argument("--no_mask_host", action="store_true", help="developer: strip the loader's host copies of the mask lengths from the batch, "
                    "as a batch from the reference's own prepare_inputs looks: the ragged layout then costs one mask read-back per step")
    ap.add_argument("--reference_batch", action="store_true", help="the batch as the reference's own loader delivers it (tvqa_dataset.py:631-688 "
                    "prepare_inputs): no mask_host (ragged tables from one mask read-back) and no target_list (the attention-loss pairs take the "
                    "answer indices on the device)")
    ap.add_argument("--no_children", action="store_true", help="skip the side measurements run as child processes (exact-fp32 step, "
                    "all-ones-mask step with its in-step K1 timing, the configs[4] stress step)")
    ap.add_argument("--h2d", action="store_true", help="developer mode: every step takes its batch from pinned host memory "
                    "through tvqaplus_amd.prefetch.BatchPrefetcher (PCIe-inclusive rate for DESIGN.md; never the headline value)")
    ap.add_argument("--full", action="store_true", help="also the measurements beside the headline line (device-time pass, rooflines, "
                    "counter passes, child runs, CPU baseline); without it a run times the steps and prints the result line only")
    ap.add_argument("--dump-outputs", dest="dump_outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if not args.full:
        args.no_device_time = args.no_roofline = args.no_pmc = args.no_children = args.no_cpu_baseline = True
    if args.config == "stress":
        args.hsz, args.sub_words, args.storage = 256, 512, "bf16"
        args.cpu_seconds = min(args.cpu_seconds, 5.0)
    return args


EAGER_LOSS = False    # --loss fused|eager: the caller's loss line (main.py:55-60) as tvqaplus_amd.stage.reference_loss (one launch) or as the eager torch expression
CLIP_FLAT = True      # --clip flat|torch: clip_grad_norm_ on the flat gradient buffer (one norm + one multiply) or torch's per-tensor form


def train_step(model, batch, bucket, params, optimizer, n_examples, world=1, keep=None):
    from tvqaplus_amd import parallel
    bucket.zero()
    (out, targets), att_loss, _, t_loss, t_scores = model(batch)
    if keep is not None:       # --dump-outputs: the step's outputs as its caller receives them
        keep.update(logits=out, targets=targets, att_loss=att_loss, temporal_loss=t_loss, temporal_scores=t_scores)
    # main.py:59 -- len(qids) / len(targets) of the gathered batch (N_new is data dependent with add_local)
    scale = (1.0 * n_examples / len(targets)) if world == 1 else parallel.global_loss_scale(n_examples, len(targets), out.device, as_tensor=True)
    if EAGER_LOSS or out.dtype != torch.float32:
        loss = F.cross_entropy(out, targets, reduction="sum") * scale + 0.1 * att_loss + 0.5 * t_loss   # att_weight 0.1, ts_weight 0.5 (config.py)
    else:   # the same value in one launch (tvqaplus_amd.stage.reference_loss; --loss eager runs the line above: child record eager_loss)
        from tvqaplus_amd.stage import reference_loss
        loss = reference_loss(out, targets, att_loss, t_loss, n_examples, 0.1, 0.5, scale=scale)
    loss.backward()
    bucket.all_reduce()
    if CLIP_FLAT:
        bucket.clip_grad_norm_(10.0)                         # the same clip on the packed buffer (parallel.FlatGradBucket)
    else:
        torch.nn.utils.clip_grad_norm_(params, 10.0)
    optimizer.step()
    return loss


DUMP_LIMIT = 64 << 20     # bytes over all files of --dump-outputs


def dump_outputs(path, arrays):
    """--dump-outputs: each tensor (or number) as path/<name>.npy -- float64 stays float64, integers become float64 (exact), every
    other float type float32.  An array that would take the total past DUMP_LIMIT is replaced by a fixed, seeded sample of its
    elements (flat, in index order: the same positions for the same shape in every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    used = 0
    for name in sorted(arrays):
        v = arrays[name]
        t = (v.detach() if torch.is_tensor(v) else torch.tensor(v)).cpu()
        a = (t.double() if (t.dtype == torch.float64 or not t.is_floating_point()) else t.float()).numpy()
        if used + a.nbytes > DUMP_LIMIT:
            keep = max(0, DUMP_LIMIT - used) // a.itemsize
            a = a.reshape(-1)[torch.randperm(a.size, generator=torch.Generator().manual_seed(2018))[:keep].sort().values.numpy()]
        np.save(os.path.join(path, name + ".npy"), a)
        used += a.nbytes


def _profile_traffic(name, kernel="str_attn_fwd"):
    """WRITE_SIZE + 2 * FETCH_SIZE (KiB -> bytes) of a kernel from a committed rocprofv3 PMC summary, or None."""
    path = os.path.join(ROOT, "profiles", name)
    try:
        vals = {}
        with open(path) as f:
            for line in f:
                if kernel in line and ("FETCH_SIZE" in line or "WRITE_SIZE" in line):
                    key = "FETCH_SIZE" if "FETCH_SIZE" in line else "WRITE_SIZE"
                    vals[key] = float(line.rsplit("avg=", 1)[1])
        if len(vals) == 2:
            return round((vals["WRITE_SIZE"] + 2.0 * vals["FETCH_SIZE"]) * 1024.0)
    except (OSError, ValueError, IndexError):
        pass
    return None


def pmc_traffic_in_run(args):
    """HBM bytes per launch of the K1 kernels MEASURED IN THIS RUN: two rocprofv3 counter passes (FETCH_SIZE, then WRITE_SIZE; counters +
    kernel trace only, as MI355X_MICROARCH.md prescribes: separate passes, KiB units, FETCH_SIZE x 2 on gfx950) around a child
    ``bench.py --only_roofline --with_bwd``.  {(direction, stream): bytes} for what could be measured; {} when rocprofv3 is missing,
    fails or takes too long (the record then quotes the committed profiles and says so)."""
    import collections, csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {}
    names = {("fwd", "vid"): ("str_attn_fwd_reg_kernel", ""), ("fwd", "sub"): ("str_attn_fwd_d128_kernel", ""),
             ("bwd", "vid"): ("str_attn_bwd_fused_kernel", "<2,"), ("bwd", "sub"): ("str_attn_bwd_fused_kernel", "<4,")}
    got = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="stage_pmc_", dir="/tmp")
            try:
                cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                       os.path.abspath(__file__), "--only_roofline", "--with_bwd", "--bsz", str(args.bsz), "--frames", str(args.frames),
                       "--regions", str(args.regions), "--sub_words", str(args.sub_words), "--qa_words", str(args.qa_words),
                       "--hsz", str(args.hsz)]
                subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=240, check=True)
                per = collections.defaultdict(float)            # (key, dispatch) -> KiB, summed over the counter's instances
                for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                    with open(f) as fh:
                        for row in csv.DictReader(fh):
                            if row.get("Counter_Name") != ctr:
                                continue
                            kn = row.get("Kernel_Name", "")
                            for key, (sub, tmpl) in names.items():
                                if sub in kn and (not tmpl or (sub + tmpl) in kn.replace(" ", "")):
                                    per[(key, row.get("Dispatch_Id"))] += float(row["Counter_Value"])
                by_key = collections.defaultdict(list)
                for (key, _), v in per.items():
                    by_key[key].append(v)
                for key, vs in by_key.items():
                    got.setdefault(key, {})[ctr] = sum(vs) / len(vs)
            finally:
                shutil.rmtree(d, ignore_errors=True)
    except Exception:                                            # noqa: BLE001 -- any profiler problem: fall back, never fail the bench
        return {}
    return {key: round((v["WRITE_SIZE"] + 2.0 * v["FETCH_SIZE"]) * 1024.0) for key, v in got.items() if len(v) == 2}


def pmc_step_traffic(args, steps=6, warm=2):
    """HBM bytes of the WHOLE step measured in this run: two rocprofv3 counter passes (FETCH_SIZE, then WRITE_SIZE;
    counters + kernel trace only; KiB units, FETCH_SIZE x 2 on gfx950 -- MI355X_MICROARCH.md) around a child bench.py on ONE stream
    (steps + warm train steps of the headline batch).  Returns {"bytes_per_step", "per_kernel": [(name, calls/step, MB/step)],
    "k1": {(dir, stream): bytes per launch IN the step}} or {}.  The child's one-off kernels (model init, synthetic batch) are counted in:
    < 2 % of the total at these step counts -- said in the record."""
    import collections, csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {}
    n_steps = steps + warm
    tot = collections.defaultdict(lambda: [0, 0.0, 0.0])           # kernel -> [dispatches, fetch KiB, write KiB]
    k1names = {("fwd", "vid"): ("str_attn_fwd_reg_kernel", ""), ("fwd", "sub"): ("str_attn_fwd_d128_kernel", ""),
               ("bwd", "vid"): ("str_attn_bwd_fused_kernel", "<2,"), ("bwd", "sub"): ("str_attn_bwd_fused_kernel", "<4,")}
    k1 = collections.defaultdict(lambda: collections.defaultdict(list))
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="stage_pmc_step_", dir="/tmp")
            try:
                cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                       os.path.abspath(__file__), "--steps", str(steps), "--warmup", str(warm), "--no_cpu_baseline", "--no_pmc", "--no_children",
                       "--no_roofline", "--no_device_time", "--streams", "0", "--bsz", str(args.bsz), "--frames", str(args.frames),
                       "--regions", str(args.regions), "--sub_words", str(args.sub_words), "--qa_words", str(args.qa_words),
                       "--hsz", str(args.hsz)]
                subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=300, check=True)
                per = collections.defaultdict(float)
                name = {}
                for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                    with open(f) as fh:
                        for row in csv.DictReader(fh):
                            if row.get("Counter_Name") != ctr:
                                continue
                            per[row["Dispatch_Id"]] += float(row["Counter_Value"])
                            name[row["Dispatch_Id"]] = row.get("Kernel_Name", "")
                for disp, v in per.items():
                    kn = name[disp]
                    t = tot[kn]
                    if ctr == "FETCH_SIZE":
                        t[0] += 1
                        t[1] += v
                    else:
                        t[2] += v
                    for key, (sub, tmpl) in k1names.items():
                        if sub in kn and (not tmpl or (sub + tmpl) in kn.replace(" ", "")):
                            k1[key][ctr].append(v)
            finally:
                shutil.rmtree(d, ignore_errors=True)
    except Exception:                                            # noqa: BLE001 -- any profiler problem: no record, never a failed bench
        return {}
    if not tot:
        return {}
    rows = sorted(((2.0 * f + w) * 1024.0 / n_steps, kn, n / float(n_steps)) for kn, (n, f, w) in tot.items())[::-1]
    total = sum(r[0] for r in rows)
    out = {"bytes_per_step": round(total), "steps_profiled": n_steps,
           "per_kernel": [(kn.split("(")[0][-60:], round(c, 2), round(b / 1e6, 1)) for b, kn, c in rows[:24]]}
    out["k1"] = {key: round((sum(v["WRITE_SIZE"]) / len(v["WRITE_SIZE"]) + 2.0 * sum(v["FETCH_SIZE"]) / len(v["FETCH_SIZE"])) * 1024.0)
                 for key, v in k1.items() if v.get("WRITE_SIZE") and v.get("FETCH_SIZE")}
    return out


def step_flops(args):
    """fp32-equivalent floating-point operations of one training step at the headline shapes (SURVEY 8d "whole-step floors": dense GEMM
    work only -- Linear / 1x1-conv products and the two contractions of the attention -- forward x 3 for the backward's dX and dW):
    N examples, 5 candidates, Li frames, Lr regions, Lw subtitle words, Lqa statement words, D = hsz, 768 -> 300 -> D input MLPs."""
    N, A, Li, Lr, Lw, Lqa, D = args.bsz, 5, args.frames, args.regions, args.sub_words, args.qa_words, args.hsz
    U = N * A * Li * Lqa
    qa_rows, sub_rows, vid_rows = N * A * Lqa, N * Li * Lw, N * Li * Lr
    mlp = 2.0 * (qa_rows + sub_rows) * (768 * 300 + 300 * D) + 2.0 * vid_rows * (300 * 300 + 300 * D)
    enc_in = 2.0 * (qa_rows + sub_rows + vid_rows) * 2 * D * D                 # two 1x1 convolutions per input-encoder application
    k1 = 2.0 * 2.0 * U * (Lr + Lw) * D                                         # scores + weighted sum, both streams
    cat3 = 3 * 2.0 * U * 3 * D * D                                             # two c2q projections + concat_fc
    enc_cls = 2.0 * U * 2 * D * D
    fwd = mlp + enc_in + k1 + cat3 + enc_cls
    return {"forward": fwd, "step": 3.0 * fwd}


def _event_times(launch, stream, reps=30, warm=5):
    """Per-launch times (ms, sorted) with events on the stream the kernels are launched on."""
    for _ in range(warm):
        launch()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record(stream)
        launch()
        e.record(stream)
    torch.cuda.synchronize()
    return sorted(s.elapsed_time(e) for s, e in ev)


def _k1_inputs(args, device, dense):
    from tvqaplus_amd.synth import make_batch
    N, NA, Li, Lqa, Lr, D = args.bsz, 5, args.frames, args.qa_words, args.regions, args.hsz
    g = torch.Generator().manual_seed(2018)
    b = make_batch(N=N, Li=Li, Lr=Lr, Lw=2, Lqa=Lqa, wd_size=4, vfeat_size=4, seed=2018, ragged=not dense)
    Cn = F.normalize(torch.randn(N, NA, Lqa, D, generator=g), dim=-1).to(device)
    Q = torch.randn(N, Li, Lr, D, generator=g).to(device)
    return (N, NA, Li, Lqa, Lr, D), g, Cn, Q, b.qas_mask.to(device).contiguous(), b.vid_mask.to(device).contiguous()


def k1_roofline(args, device, dense=None):
    """Isolated StructuredAttention forward kernel timed with events on the launch stream (video-stream shape by default;
    the caller swaps args.regions for the subtitle stream; dense = all-ones masks: no store-only frames)."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    dense = args.dense if dense is None else dense
    (N, NA, Li, Lqa, Lr, D), g, Cn, Q, cm, qm = _k1_inputs(args, device, dense)
    A = torch.empty(N, NA, Li, Lqa, D, device=device)
    S = torch.empty(N, NA, Li, Lqa, Lr, device=device)
    Sn = torch.empty_like(S)
    stream = torch.cuda.current_stream()

    def launch():
        _lib.check(lib.stage_str_attn_fwd(Cn.data_ptr(), Q.data_ptr(), cm.data_ptr(), qm.data_ptr(), A.data_ptr(),
                                          S.data_ptr(), Sn.data_ptr(), N, NA, Li, Lqa, Lr, D, 10.0, 0.0, 0,
                                          stream.cuda_stream), "stage_str_attn_fwd")
    ms = _event_times(launch, stream)
    avg_ms = sum(ms) / len(ms)
    U = N * NA * Li * Lqa
    # algorithmic bytes: inputs once + A + S + S_ written once, fp32
    alg = 4 * (N * NA * Lqa * D + N * Li * Lr * D + N * NA * Lqa + N * Li * Lr + U * D + 2 * U * Lr)
    achieved = alg / (avg_ms * 1e-3) / 1e9
    # HBM bytes per launch: NOT measured in this run -- parsed from the builder's PMC passes committed under profiles/
    # (tools/pmc_run.sh: WRITE_SIZE + 2 x FETCH_SIZE in KiB, the x2 being the gfx950 FETCH_SIZE correction of
    # MI355X_MICROARCH.md); only quoted for the exact shapes those passes ran (`traffic_source` says which file)
    traffic = src = None
    if (N, NA, Li, Lqa, D) == (16, 5, 300, 40, 128) and not dense and Lr in (20, 50):
        for rnd in ("r05", "r04", "r03", "r02"):
            src = "profiles/%s_k1_fwd_pmc_%s.txt" % (rnd, "vid" if Lr == 20 else "sub")
            traffic = _profile_traffic(os.path.basename(src), "str_attn_fwd")
            if traffic is not None:
                break
        if traffic is None:
            src = None
    return {"bound": "hbm", "kernel": "str_attn_fwd_reg_kernel" if Lr <= 32 else "str_attn_fwd_d128_kernel", "achieved": round(achieved, 1), "peak": 8000.0,
            "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "traffic": traffic,
            "traffic_source": (src + " (builder's rocprofv3 PMC pass, not measured in this run)") if src else None,
            "algorithmic_bytes": alg, "masks": "all-ones" if dense else "ragged",
            "avg_us": round(avg_ms * 1e3, 1), "min_us": round(ms[0] * 1e3, 1),
            "shape": {"N": N, "NA": NA, "Li": Li, "Lqa": Lqa, "Lr": Lr, "D": D}}


def k1k2_roofline(args, device, model):
    """'if K1+K2 are fused ... report both the isolated-K1 number and the fused number'.  K1 + K2 (StructuredAttention +
    c2q_down_projection, model/stage.py:365-387) as the model issues them: ONE group call (stage_grp_qa_ctx_fwd: K1 forward kernel + the
    fused LayerNorm -> dropout -> Linear -> ReLU kernel), training mode, events on the launch stream.  Algorithmic bytes: the inputs + the
    block's output `mixed` + the two score maps (the attended tensor and the 3D-wide concat are internal)."""
    (N, NA, Li, Lqa, Lr, D), g, Cn, Q, cm, qm = _k1_inputs(args, device, args.dense)
    qa = torch.randn(N, NA, Lqa, D, generator=g).to(device)
    stream = torch.cuda.current_stream()
    was = model.training
    model.train()

    def launch():
        with torch.no_grad():
            model.qa_ctx_attention(qa, Q, cm, qm)
    try:
        ms = _event_times(launch, stream, reps=20, warm=3)
    finally:
        model.train(was)
    avg_ms = sum(ms) / len(ms)
    U = N * NA * Li * Lqa
    alg = 4 * (N * NA * Lqa * D + N * Li * Lr * D + N * NA * Lqa + N * Li * Lr + U * D + 2 * U * Lr)
    gbs = alg / (avg_ms * 1e-3) / 1e9
    # K2 is a dense 3D -> D contraction: compute bound in fp32 (94.4 GFLOP per instance + K1's two small products);
    # priced against the dense fp32 matrix-core peak (the products run as fp16 pairs, three MFMAs each: fp32-equivalent FLOPs)
    flops = 2.0 * U * (3 * D) * D + 2.0 * 2.0 * U * Lr * D
    tf = flops / (avg_ms * 1e-3) / 1e12
    return {"bound": "mfma", "kernel": "K1 + K2 group forward (stage_grp_qa_ctx_fwd: str_attn_fwd + cff_fwd_kernel; since round 6 the 1.47 GB "
            "normalised concat is not written: the backward rebuilds it, csrc/cat3_bwd_dw.hip)", "achieved": round(tf, 1), "peak": 157.3, "unit": "TFLOP/s",
            "frac": round(tf / 157.3, 4), "flops_fp32_equivalent": flops,
            # the same time against the pipe the instructions actually issue on: three v_mfma_f32_32x32x16_f16 per fp32 product
            "mfma_issued_tflops_f16": round(3.0 * tf, 1), "peak_f16": 2500.0, "frac_of_f16_peak": round(3.0 * tf / 2500.0, 4),
            "hbm_gbs_algorithmic": round(gbs, 1),
            "hbm_frac_algorithmic": round(gbs / 8000.0, 4), "traffic": None, "algorithmic_bytes": alg,
            "avg_us": round(avg_ms * 1e3, 1), "min_us": round(ms[0] * 1e3, 1),
            "shape": {"N": N, "NA": NA, "Li": Li, "Lqa": Lqa, "Lr": Lr, "D": D}}


def k1_long_roofline(args, device):
    """BASELINE.json configs[4]: the long-row StructuredAttention forward (csrc/str_attn_long.hip; rows of 512 subtitle words, D = 256,
    bf16 operands / output, fp32 scores, softmax and accumulation), the C-ABI call alone, events on the launch stream."""
    from tvqaplus_amd import _lib
    from tvqaplus_amd.synth import make_batch
    lib = _lib.load()
    N, NA, Li, Lqa, Lr, D = args.bsz, 5, args.frames, args.qa_words, args.sub_words, args.hsz
    bf = args.storage == "bf16"
    dt = torch.bfloat16 if bf else torch.float32
    g = torch.Generator().manual_seed(2018)
    b = make_batch(N=N, Li=Li, Lr=Lr, Lw=2, Lqa=Lqa, wd_size=4, vfeat_size=4, seed=2018, ragged=not args.dense)
    Cn = F.normalize(torch.randn(N, NA, Lqa, D, generator=g), dim=-1).to(device).to(dt)
    Q = torch.randn(N, Li, Lr, D, generator=g).to(device).to(dt)
    Qn = F.normalize(Q.float(), dim=-1).to(dt)
    cm, qm = b.qas_mask.to(device).contiguous(), b.vid_mask.to(device).contiguous()
    A = torch.empty(N, NA, Li, Lqa, D, device=device, dtype=dt)
    S = torch.empty(N, NA, Li, Lqa, Lr, device=device)
    Sn = torch.empty_like(S)
    stream = torch.cuda.current_stream()

    def launch():
        _lib.check(lib.stage_str_attn_long_fwd(Cn.data_ptr(), Q.data_ptr(), Qn.data_ptr(), cm.data_ptr(), qm.data_ptr(), A.data_ptr(),
                                               S.data_ptr(), Sn.data_ptr(), N, NA, Li, Lqa, Lr, D, 10.0, int(bf), stream.cuda_stream),
                   "stage_str_attn_long_fwd")
    ms = _event_times(launch, stream, reps=10, warm=2)
    avg_ms = sum(ms) / len(ms)
    U = N * NA * Li * Lqa
    es = 2 if bf else 4
    alg = es * (N * NA * Lqa * D + 2 * N * Li * Lr * D + U * D) + 4 * (N * NA * Lqa + N * Li * Lr + 2 * U * Lr)
    achieved = alg / (avg_ms * 1e-3) / 1e9
    flops = 2 * 2 * U * Lr * D
    # HBM bytes per launch from the builder's committed counter passes (published stress shape only; `traffic_source` says which file)
    traffic = src = None
    if (N, NA, Li, Lqa, Lr, D, bf, args.dense) == (16, 5, 300, 40, 512, 256, True, False):
        for rnd in ("r05",):
            src = "profiles/%s_k1_long_fwd_pmc.txt" % rnd
            traffic = _profile_traffic(os.path.basename(src), "str_attn_long_fwd")
            if traffic is not None:
                break
        if traffic is None:
            src = None
    return {"bound": "hbm", "kernel": "str_attn_long_fwd (%s storage)" % args.storage, "achieved": round(achieved, 1), "peak": 8000.0,
            "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "traffic": traffic,
            "traffic_source": (src + " (builder's rocprofv3 PMC pass, not measured in this run)") if src else None, "algorithmic_bytes": alg,
            "tflops": round(flops / (avg_ms * 1e-3) / 1e12, 1), "avg_us": round(avg_ms * 1e3, 1), "min_us": round(ms[0] * 1e3, 1),
            "shape": {"N": N, "NA": NA, "Li": Li, "Lqa": Lqa, "Lr": Lr, "D": D}}


def k1_bwd_roofline(args, device):
    """Isolated fused StructuredAttention backward (schedule + one-pass kernel + ordered slab sum = one C-ABI call), events on
    the launch stream.  Algorithmic bytes: dA, Q, Qn, Cn, S_ read once; dQraw, dQn, dCn written once (fp32)."""
    from tvqaplus_amd import _lib
    lib = _lib.load()
    (N, NA, Li, Lqa, Lr, D), g, Cn, Q, cm, qm = _k1_inputs(args, device, args.dense)
    st = torch.cuda.current_stream()
    Qn = torch.empty_like(Q)
    _lib.check(lib.stage_l2norm_fwd(Q.data_ptr(), Qn.data_ptr(), None, N * Li * Lr, D, 1e-12, 0.0, 0, st.cuda_stream), "l2norm")
    A = torch.empty(N, NA, Li, Lqa, D, device=device)
    S = torch.empty(N, NA, Li, Lqa, Lr, device=device)
    Sn = torch.empty_like(S)
    _lib.check(lib.stage_str_attn_fwd(Cn.data_ptr(), Q.data_ptr(), cm.data_ptr(), qm.data_ptr(), A.data_ptr(), S.data_ptr(),
                                      Sn.data_ptr(), N, NA, Li, Lqa, Lr, D, 10.0, 0.0, 0, st.cuda_stream), "fwd")
    del S
    dA = A.normal_()        # reuse the buffer: any gradient values do
    wsb = lib.stage_str_attn_bwd_fused_ws_bytes(N, NA, Li, Lqa, D)
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=device)
    dQ, dQn, dCn = torch.empty_like(Q), torch.empty_like(Q), torch.empty_like(Cn)

    def launch():
        _lib.check(lib.stage_str_attn_bwd_fused(dA.data_ptr(), None, Cn.data_ptr(), Q.data_ptr(), Qn.data_ptr(), Sn.data_ptr(),
                                                qm.data_ptr(), dQ.data_ptr(), dQn.data_ptr(), dCn.data_ptr(), N, NA, Li, Lqa, Lr, D,
                                                10.0, ws.data_ptr(), wsb, st.cuda_stream), "stage_str_attn_bwd_fused")
    ms = _event_times(launch, st, reps=20, warm=3)
    avg_ms = sum(ms) / len(ms)
    U = N * NA * Li * Lqa
    # SURVEY.md 8d's list: dA, Q, C, S_ read; dC, dQ written (the kernel's separate Qn / dQn planes are an interface detail and
    # show up in `traffic`, not here)
    alg = 4 * (U * D + U * Lr + 2 * N * Li * Lr * D + 2 * N * NA * Lqa * D)
    achieved = alg / (avg_ms * 1e-3) / 1e9
    traffic = src = None
    if (N, NA, Li, Lqa, D) == (16, 5, 300, 40, 128) and not args.dense and Lr in (20, 50):
        for rnd in ("r05", "r04", "r03", "r02"):
            src = "profiles/%s_k1_bwd_pmc_%s.txt" % (rnd, "vid" if Lr == 20 else "sub")
            traffic = _profile_traffic(os.path.basename(src), "str_attn_bwd_fused")
            if traffic is not None:
                break
        if traffic is None:
            src = None
    return {"bound": "hbm", "kernel": "str_attn_bwd_fused_kernel (+ schedule, slab sum)", "achieved": round(achieved, 1),
            "peak": 8000.0, "unit": "GB/s", "frac": round(achieved / 8000.0, 4), "traffic": traffic,
            "traffic_source": (src + " (builder's rocprofv3 PMC pass, not measured in this run)") if src else None,
            "algorithmic_bytes": alg, "avg_us": round(avg_ms * 1e3, 1), "min_us": round(ms[0] * 1e3, 1),
            "shape": {"N": N, "NA": NA, "Li": Li, "Lqa": Lqa, "Lr": Lr, "D": D}}


def device_time(step, n=3):
    """(summed kernel time per step in ms, kernel launches per step) from a torch.profiler device-activity pass over n steps;
    (None, None) if the profiler is unavailable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                step()
            torch.cuda.synchronize()
        dev = torch.autograd.DeviceType.CUDA
        ks = [e for e in prof.events() if e.device_type == dev and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        if not ks:
            return None, None
        return round(sum(e.time_range.elapsed_us() for e in ks) / n / 1e3, 3), round(len(ks) / n, 1)
    except Exception:   # noqa: BLE001 -- diagnostics only, never fails the bench
        return None, None


def child_bench(extra, env=None, timeout=240):
    """One more bench.py as a child process (its own HIP context: environment switches of the library are read once per process),
    N = 1, without CPU baseline / counter passes / children of its own.  Returns its JSON record or {"error": ...}."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--full", "--no_cpu_baseline", "--no_pmc", "--no_children"] + list(extra)
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    try:
        out = subprocess.run(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, check=True).stdout.decode()
        return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    except Exception as ex:   # noqa: BLE001 -- side measurements never fail the bench
        return {"error": repr(ex)[:200]}


def side_records(args):
    """Measurements the headline line is read next to ("bench hygiene"), each a short child run at the headline shapes:
    * exact_f32: the step with STAGE_GEMM_F32=1 -- every product on v_mfma_f32 (no fp16 pairs, dense rows: the ragged / fused kernels
      are fp16-pair kernels), i.e. what the `dtype: f32` label costs when taken literally;
    * dense: all-ones masks (nothing to skip for the ragged-row layout), with the K1 forward kernels timed inside its steps;
    * stress: BASELINE.json configs[4] (bf16 storage, hsz 256, 512-word subtitle rows), three steps, with the long-row K1 forward;
    * one_stream / all_branches: the same step with the model's branch streams off (--streams 0: every kernel on one stream, what
      rounds 1-3 and the first half of round 4 measured) and fully on (--streams 4: the video attention on its side stream too, unfenced)."""
    shp = ["--bsz", str(args.bsz), "--frames", str(args.frames), "--regions", str(args.regions), "--qa_words", str(args.qa_words)]
    out = {}
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "6", "--warmup", "3", "--no_roofline",
                           "--no_device_time"], env={"STAGE_GEMM_F32": "1"})
    out["exact_f32"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"], "note": "STAGE_GEMM_F32=1: v_mfma_f32 products, dense rows",
                         "ragged_rows": "not available: the ragged-row groups are built on the fused [a,b,a*b] kernels, which exist as "
                                        "fp16-pair kernels only; by the row ratio of this batch the strict-fp32 step on ragged rows would "
                                        "be ~0.77 x this figure (an estimate, not a measurement)"}
                        if "ms_per_step" in r else r)
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "6", "--warmup", "3", "--dense",
                           "--no_device_time"])
    if "ms_per_step" in r:
        out["dense"] = {"ms_per_step": r["ms_per_step"], "value": r["value"]}
        for k_src, k_dst in (("roofline", "roofline_dense"), ("roofline_sub", "roofline_sub_dense")):
            if k_src in r:
                out[k_dst] = {k: r[k_src].get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_us", "min_us", "timed",
                                                            "isolated_avg_us", "isolated_frac", "algorithmic_bytes", "masks", "traffic")}
    else:
        out["dense"] = r
    for key, lv in (("one_stream", "0"), ("all_branches", "4")):
        # (one stream: with the K1 forward kernels timed inside its steps -- in the headline run the subtitle attention shares the chip
        # with the video branch's encoder, which shows in ITS duration; here nothing runs beside it)
        r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "10", "--warmup", "4",
                               "--no_device_time", "--streams", lv] + (["--no_pmc"] if lv == "0" else ["--no_roofline"]))
        out[key] = {"ms_per_step": r["ms_per_step"], "value": r["value"], "streams": int(lv)} if "ms_per_step" in r else r
        if lv == "0" and "ms_per_step" in r:
            out[key]["k1_forward_in_step"] = {nm: {k: r[src].get(k) for k in ("frac", "achieved", "avg_us", "min_us")}
                                              for nm, src in (("video", "roofline"), ("subtitle", "roofline_sub")) if src in r}
    # reference_batch: the batch stripped of the two host-side extras tvqaplus_amd.synth / prefetch attach (mask_host, target_list) -- what
    # /root/reference/tvqa_dataset.py:631-688 hands to main.py: one mask read-back per step, answer indices taken on the device
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "10", "--warmup", "4", "--no_roofline",
                           "--no_device_time", "--reference_batch"])
    out["reference_batch"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"], "host_issue_ms_per_step": r.get("host_issue_ms_per_step"),
                               "host_wait_ms_per_step": r.get("host_wait_ms_per_step"),
                               "note": "batch without mask_host / target_list, as prepare_inputs (tvqa_dataset.py:631-688) delivers it"}
                              if "ms_per_step" in r else r)
    # strong_n2_sim: the step ONE of 8 ranks runs under strong scaling of the global B=16 (2 examples per GPU, BASELINE configs[3]) --
    # on this one GPU, without the two collectives (2.2 MB all-reduce + logits all-gather, both latency-bound): the host-issue bound of
    # the sharded step on the record.  predicted_8gpu_value = 16 examples / this step time (an upper bound: no collective time in it)
    r = child_bench(shp[2:] + ["--bsz", "2", "--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "20", "--warmup", "5",
                               "--no_roofline", "--no_device_time"])
    out["strong_n2_sim"] = ({"ms_per_step": r["ms_per_step"], "examples_per_gpu": 2, "host_issue_ms_per_step": r.get("host_issue_ms_per_step"),
                             "host_wait_ms_per_step": r.get("host_wait_ms_per_step"),
                             "predicted_8gpu_value": round(16.0 / (r["ms_per_step"] * 1e-3), 1),
                             "note": "single-GPU step at 2 examples = what each of 8 ranks runs at global B=16 (collectives excluded)"}
                            if "ms_per_step" in r else r)
    # heads4: BASELINE.json configs[2] (region / word self-attention in both encoders, model/self_attention.py:35-71)
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "6", "--warmup", "3", "--no_roofline",
                           "--heads", "4"])
    out["heads4"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"], "launches_per_step": r.get("launches_per_step"),
                      "host_issue_ms_per_step": r.get("host_issue_ms_per_step"), "note": "configs[2]: --heads 4 in both encoders"}
                     if "ms_per_step" in r else r)
    # cat3_dw: the backward of the [a,b,a*b] blocks with the Linear's gradients inside and no saved z (csrc/cat3_bwd_dw.hip, VERDICT r5
    # item 1) is the default since round 6; this child is the step WITHOUT it (profiles/r06_cat3_dw_ab.txt)
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "6", "--warmup", "3", "--no_roofline",
                           "--no_device_time"], env={"STAGE_CAT3_DW": "0"})
    out["cat3_dw_off"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"],
                           "note": "STAGE_CAT3_DW=0: forward saves z, cf_bwd_kernel + weight-gradient GEMM on z (the round-5 path)"}
                          if "ms_per_step" in r else r)
    r = child_bench(shp + ["--sub_words", str(args.sub_words), "--hsz", str(args.hsz), "--steps", "12", "--warmup", "6", "--no_roofline",
                           "--no_device_time", "--loss", "eager"])
    out["eager_loss"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"],
                          "note": "--loss eager: the loss line of main.py:55-60 as the eager torch expression (~20 small launches behind the "
                                  "proposal read-back) instead of tvqaplus_amd.stage.reference_loss"} if "ms_per_step" in r else r)
    r = child_bench(shp + ["--config", "stress", "--steps", "3", "--warmup", "2", "--no_device_time"], timeout=300)
    out["stress"] = ({"ms_per_step": r["ms_per_step"], "value": r["value"], "dtype": r.get("dtype"), "workload": r["config"]["workload"],
                      "peak_hbm_gib": r["config"].get("peak_hbm_gib"), "roofline": r.get("roofline")} if "ms_per_step" in r else r)
    return out


def cpu_baseline(args, opt):
    """The oracle (CPU port of the reference path, plain torch fp32) on the host cores: same step, bounded sample."""
    from oracle import stage_oracle as O
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch
    # torch's CPU kernels stop scaling (and thrash) far below a 256-thread host: 32 threads is the main sample, one short
    # sample on every hardware thread is reported next to it (`all_threads`); `value` / `cores` = the faster of the two
    cores = min(32, os.cpu_count() or 1)
    cpu_model = "?"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    B = args.bsz if args.cpu_seconds >= 15 else 1      # the bench batch itself when the budget allows one step of it (~20 s)
    sup = not args.no_sup_att
    batch = make_batch(N=B, Li=args.frames, Lr=args.regions, Lw=args.sub_words, Lqa=args.qa_words, seed=2018,
                       ragged=not args.dense, att_imgs=args.att_imgs if sup else 0, att_words=args.att_words)
    torch.manual_seed(2018)
    import contextlib
    with contextlib.redirect_stdout(open(os.devnull, "w")):   # STAGE.__init__ prints which branches are active
        ref_model = STAGE(opt)
    P = {k: v.clone().requires_grad_(v.is_floating_point() and not k.endswith(".pe"))
         for k, v in ref_model.state_dict().items()}
    params = [v for v in P.values() if v.requires_grad]
    optim = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7)

    def step():
        optim.zero_grad(set_to_none=True)
        out = O.stage_forward(P, opt, batch, training=True)
        loss = O.training_loss(out, n_examples=len(batch.qid))
        if sup:   # the supervised attention term on the oracle's own attention map (host index building is shared code)
            from tvqaplus_amd import att_host
            loss = loss + 0.1 * att_host.get_att_loss(opt, out["vid_raw_s"].squeeze(2) if out["vid_raw_s"].dim() == 6 else out["vid_raw_s"], batch)[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        optim.step()

    def sample(threads, seconds, warm=True):
        torch.set_num_threads(threads)
        if warm:
            step()  # warm-up (allocator, thread pool)
        t0 = time.time()
        n = 0
        while n < 1 or (time.time() - t0 < seconds and n < 50):
            step()
            n += 1
        return n, time.time() - t0

    # which thread count: MEASURED here on a short version of the same step (1 example x 24 frames), `cores` threads against every
    # hardware thread of the host -- torch's CPU kernels thrash far below a 256-thread width (round 3: one full step took 95.7 s on 256
    # threads against 1.1 s on 32), so the wide sample must stay small to keep the run bounded
    probe = {}
    host_threads = os.cpu_count() or 1
    if host_threads > cores and args.cpu_probe_threads == 0:
        # each width in its own child process under a wall-clock limit: the all-threads run of even this short step took 94 s here
        import subprocess
        for th in (cores, host_threads):
            cmd = [sys.executable, os.path.abspath(__file__), "--cpu_probe_threads", str(th), "--regions", str(args.regions), "--sub_words",
                   str(args.sub_words), "--qa_words", str(args.qa_words), "--hsz", str(args.hsz)] + (["--no_sup_att"] if not sup else [])
            try:
                out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=20, check=True).stdout.decode()
                probe[str(th)] = float(out.strip().splitlines()[-1])
            except subprocess.TimeoutExpired:
                probe[str(th)] = "> 20 (killed)"
            except Exception:   # noqa: BLE001
                probe[str(th)] = None
    if args.cpu_probe_threads > 0:       # child mode: seconds per step of the short shape at the given width, printed
        batch = make_batch(N=1, Li=24, Lr=args.regions, Lw=args.sub_words, Lqa=args.qa_words, seed=2018, ragged=not args.dense,
                           att_imgs=min(args.att_imgs, 2) if sup else 0, att_words=args.att_words)
        n_p, dt_p = sample(args.cpu_probe_threads, 1.5)
        print("%.4f" % (dt_p / n_p))
        return None
    n, dt = sample(cores, 0.7 * args.cpu_seconds, warm=B == 1)
    rec = {"value": round(B * n / dt, 4), "unit": "QA-examples/s", "cores": cores, "host_cores": os.cpu_count(),
           "cpu_model": cpu_model, "kind": "port",
           "sample": "%d full training steps of B=%d x %d frames (same per-example shapes, dropout 0.1) in %.1f s"
                     % (n, B, args.frames, dt)}
    host = os.cpu_count() or 1
    # SURVEY 8d asks for os.cpu_count() threads.  Measured (round 3, EPYC 9575F, 256 hardware threads): ONE step took 95.7 s on
    # 256 threads against 1.1 s on 32 -- torch's CPU kernels thrash far below that width -- so the all-threads sample is
    # opt-in (it alone would take minutes) and 32 threads is the reported baseline
    if probe:
        rec["thread_probe_s_per_step"] = dict(probe, shape="1 example x 24 frames, same per-frame shapes, measured in this run "
                                                           "(one child process per width, 20 s limit)")
    if host > cores and args.cpu_all_threads:
        n2, dt2 = sample(host, 0.3 * args.cpu_seconds)
        rec["all_threads"] = {"cores": host, "value": round(B * n2 / dt2, 4),
                              "sample": "%d steps in %.1f s" % (n2, dt2)}
        if rec["all_threads"]["value"] > rec["value"]:   # report the better configuration as the baseline
            rec["all_threads"], rec["value"], rec["cores"], rec["sample"] = (
                {"cores": cores, "value": rec["value"], "sample": rec["sample"]}, rec["all_threads"]["value"], host,
                "%d full training steps of B=%d x %d frames in %.1f s" % (n2, B, args.frames, dt2))
    return rec


def main():
    args = parse()
    global CLIP_FLAT, EAGER_LOSS
    CLIP_FLAT = args.clip == "flat"
    EAGER_LOSS = args.loss == "eager"
    from tvqaplus_amd import parallel
    from tvqaplus_amd.stage import STAGE
    from tvqaplus_amd.synth import make_batch, make_opt
    # STAGE_BENCH_SHARED_GPU (test hook, tests/test_parallel_hip.py): every rank on cuda:0, collectives over gloo -- the N > 1 control
    # flow of this file (barriers, max over ranks, the all-rank passes after the timed region) on a one-GPU box
    shared = os.environ.get("STAGE_BENCH_SHARED_GPU") is not None
    rank, local, world = parallel.init_from_env(backend="gloo" if shared else None)
    if shared:
        local = 0
    if args.cpu_probe_threads > 0:      # CPU-only child of cpu_baseline()
        from tvqaplus_amd.synth import make_opt as _mo
        cpu_baseline(args, _mo(hsz=args.hsz, add_local=True, dropout=0.1, use_sup_att=not args.no_sup_att))
        return
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if args.only_roofline and args.config == "stress":   # the long-row attention forward alone (PMC passes: tools/round_profile.sh)
        print(json.dumps({"long": k1_long_roofline(args, device)}))
        return
    if args.only_roofline:  # developer shortcut: just the K1 kernel line (video and subtitle stream shapes)
        print(json.dumps({"vid": k1_roofline(args, device)}))
        if args.with_bwd:
            print(json.dumps({"vid_bwd": k1_bwd_roofline(args, device)}))
        args.regions = args.sub_words
        print(json.dumps({"sub": k1_roofline(args, device)}))
        if args.with_bwd:
            print(json.dumps({"sub_bwd": k1_bwd_roofline(args, device)}))
        return
    torch.manual_seed(2018)
    sup = not args.no_sup_att
    opt = make_opt(hsz=args.hsz, add_local=True, dropout=0.1, use_sup_att=sup, input_encoder_n_heads=args.heads,
                   cls_encoder_n_heads=args.heads, storage_dtype=args.storage)
    import contextlib
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        model = STAGE(opt)
    model = model.to(device).train()
    if args.streams >= 0:
        model.use_streams = args.streams
    params = [p for p in model.parameters() if p.requires_grad]
    bucket = parallel.FlatGradBucket(params)
    # torch.optim.Adam, as main.py:209; fused=True is the same update as ONE multi-tensor kernel instead of ~10 (--adam foreach =
    # torch's default implementation)
    optimizer = None
    if args.adam == "fused":
        try:
            optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7, fused=True)
        except (RuntimeError, TypeError):
            args.adam = "foreach"
    if optimizer is None:
        optimizer = torch.optim.Adam(params, lr=1e-3, weight_decay=3e-7)
    if args.scaling == "strong":      # global batch of --bsz examples, example-major shards
        full = make_batch(N=args.bsz, Li=args.frames, Lr=args.regions, Lw=args.sub_words, Lqa=args.qa_words, seed=2018,
                          ragged=not args.dense, att_imgs=args.att_imgs if sup else 0, att_words=args.att_words)
        batch = parallel.shard_batch(full, rank, world).to(device)
        n_local = len(batch.qid)
        assert n_local > 0, "strong scaling needs at least one example per GPU (use parallel.CandidateLayout beyond that)"
    else:
        batch = make_batch(N=args.bsz, Li=args.frames, Lr=args.regions, Lw=args.sub_words, Lqa=args.qa_words,
                           seed=2018 + rank, ragged=not args.dense, att_imgs=args.att_imgs if sup else 0,
                           att_words=args.att_words).to(device)
        n_local = args.bsz
    n_global = args.bsz if args.scaling == "strong" else world * args.bsz
    if args.storage == "bf16" and not args.fp32_inputs:
        # bf16 storage mode: the features are rounded to bf16 ONCE on entry (stage.py: base_encoder); a loader for that mode stages them
        # as bf16 (tvqaplus_amd/prefetch.py, bit-identical), so the resident batch of the timed region holds them as bf16
        for k in ("vid", "sub_bert"):
            if getattr(batch, k, None) is not None and getattr(batch, k).dtype == torch.float32:
                setattr(batch, k, getattr(batch, k).to(torch.bfloat16))
    if args.no_mask_host or args.reference_batch:
        batch.pop("mask_host", None)
    if args.reference_batch:
        batch.pop("target_list", None)

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    if args.h2d:
        # PCIe-inclusive variant: the same host batch (pinned once) is re-sent every step, overlapped with the previous step
        from tvqaplus_amd.prefetch import BatchPrefetcher
        host = make_batch(N=args.bsz, Li=args.frames, Lr=args.regions, Lw=args.sub_words, Lqa=args.qa_words,
                          seed=2018 + rank, ragged=not args.dense, att_imgs=args.att_imgs if sup else 0,
                          att_words=args.att_words)
        for k, v in host.items():
            if torch.is_tensor(v):
                host[k] = v.pin_memory()
        feed = BatchPrefetcher((host for _ in range(args.warmup + args.steps)), device)
        nxt = lambda: next(feed)
        batch_dev = lambda: host.to(device)
    else:
        nxt = lambda: batch
    import gc
    if args.gc == "freeze":
        gc.collect()      # (the collection itself BEFORE the warm-up: ~0.1 s of host time right in front of the timed region would
                          # let the GPU fall back to its idle clocks)
    for _ in range(args.warmup):
        train_step(model, nxt(), bucket, params, optimizer, n_local, world)
    # Python's cyclic collector: a full (generation 2) collection walks every tracked object of the process -- millions once torch
    # is imported -- and one lands around the 15th training step (measured: a single 29.6 ms step among 19.9 ms ones, i.e. +0.5 ms
    # on the mean of 20 steps).  The objects alive after the warm-up (modules, parameters, the batch) are permanent, so they are
    # moved out of the collector's sight (gc.freeze, what long-running Python services do); the collector stays ON for what the
    # steps allocate.  --gc default leaves everything as the interpreter ships it.
    if args.gc == "freeze":
        gc.freeze()
    elif args.gc == "off":
        gc.disable()
    # host-side bookkeeping of the timed region (a few perf_counter reads and one event record per step; no synchronisation):
    # time the host spends WAITING for the device (the per-step proposal read-back, tvqaplus_amd/stage.py: get_proposals) vs
    # issuing work, and one event per step boundary for the spread of the step times
    waits = [0.0]
    _ev_sync = torch.cuda.Event.synchronize

    def _timed_sync(self):
        t = time.perf_counter()
        _ev_sync(self)
        waits[0] += time.perf_counter() - t
    torch.cuda.Event.synchronize = _timed_sync
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    stream = torch.cuda.current_stream()
    # the K1 forward kernels of every timed step carry an event pair on their launch stream (include/stage_hip.h:
    # stage_k1_fwd_timer): their duration INSIDE the timed region is what `roofline` quotes
    from tvqaplus_amd import _lib as _L
    lib = _L.load()
    k1_ev = {}
    # (only when this rank's step runs the full --bsz examples: under strong scaling with N > 1 a rank's kernels see bsz / N examples --
    # their in-step durations say nothing about the published shape, and the roofline record keeps its isolated full-shape launches)
    if rank == 0 and args.storage == "fp32" and args.hsz == 128 and not args.no_roofline and n_local == args.bsz:
        for lr in {args.regions, args.sub_words}:
            if lr <= 64:
                k1_ev[lr] = [(lib.stage_timer_create(), lib.stage_timer_create()) for _ in range(args.steps)]
    last = {} if args.dump_outputs else None
    sync()
    t0 = time.perf_counter()
    marks[0].record(stream)
    for i in range(args.steps):
        for lr, evs in k1_ev.items():
            lib.stage_k1_fwd_timer(evs[i][0], evs[i][1], lr)
        loss = train_step(model, nxt(), bucket, params, optimizer, n_local, world, keep=last if i == args.steps - 1 else None)
        marks[i + 1].record(stream)
    t_issued = time.perf_counter()
    sync()
    dt = time.perf_counter() - t0
    lib.stage_k1_fwd_timer(None, None, 0)
    if last is not None and rank == 0:
        dump_outputs(args.dump_outputs, dict(last, loss=loss, grad=bucket.flat,
                                             params=torch.cat([p.detach().reshape(-1) for p in params])))
    k1_in_step = {}
    for lr, evs in k1_ev.items():
        ts = sorted(lib.stage_timer_elapsed_ms(a, b) for a, b in evs)
        for a, b in evs:
            lib.stage_timer_destroy(a)
            lib.stage_timer_destroy(b)
        if ts and ts[0] > 0:
            k1_in_step[lr] = ts
    torch.cuda.Event.synchronize = _ev_sync
    host_issue_ms = 1e3 * (t_issued - t0 - waits[0]) / args.steps
    host_wait_ms = 1e3 * waits[0] / args.steps
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    if world > 1:
        t = torch.tensor([dt], device="cpu" if shared else device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    loss_v = float(loss.detach())
    peak_gb = torch.cuda.max_memory_allocated() / 2 ** 30

    # device time per step: a torch.profiler pass over 3 extra steps AFTER the timed region -- on EVERY rank (the step contains the
    # gradient all-reduce: rank 0 alone would wait for its peers forever)
    dev_ms = None
    if not args.no_device_time:
        dev_ms = device_time(
            lambda: train_step(model, nxt() if not args.h2d else batch_dev(), bucket, params, optimizer, n_local, world))
    if rank == 0:
        rec = {
            "metric": "QA-examples/sec (5-candidate fwd+bwd) at B=16",
            "value": round(n_global * args.steps / dt, 3),
            "unit": "QA-examples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32" if args.storage == "fp32" else "bf16", "data": "synthetic" + (" (re-sent from pinned host memory every step)" if args.h2d else ""),
            "config": {"baseline_config": "configs[4] (bf16 / D=256 / T_sub=512 stress)" if args.config == "stress" else "configs[1]",
                       "workload": "STAGE train step B=%d/GPU x5 cand x%d frames x%d regions x%d sub x%d QA words, hsz=%d, "
                                   "add_local%s%s, dropout 0.1, %s masks; %s"
                                   % (n_local, args.frames, args.regions, args.sub_words, args.qa_words, args.hsz,
                                      " + supervised attention loss" if sup else "",
                                      (" + %d-head self-attention" % args.heads) if args.heads else "",
                                      "all-ones" if args.dense else "ragged",
                                      "bf16 activations / bf16-rounded weights, fp32 statistics, softmax and accumulation"
                                      if args.storage == "bf16" else
                                      "fp32 via fp16-split MFMA GEMMs (error below an fp32 FMA chain)"),
                       "step": "fwd + loss (main.py:55-60) + bwd + grad all-reduce + clip_grad_norm_ + Adam (torch.optim.Adam, %s)" % args.adam,
                       "global_batch": n_global, "parallelism": "dp%d (example-sharded, flat 2.2MB grad "
                                                                  "all-reduce over RCCL)" % world,
                       "final_loss": round(loss_v, 4), "peak_hbm_gib": round(peak_gb, 2)},
        }
        # where the step time goes, so that a host-bound box is visible in the record: host_issue = python / launch time per
        # step (waits excluded), host_wait = time blocked on the proposal read-back, device = summed kernel time per step from
        # a torch.profiler (roctracer) pass over 3 extra steps AFTER the timed region, step_ms = spread of the timed steps
        rec["host_issue_ms_per_step"] = round(host_issue_ms, 3)
        rec["host_wait_ms_per_step"] = round(host_wait_ms, 3)
        rec["step_ms"] = {"min": round(step_ms[0], 3), "median": round(step_ms[len(step_ms) // 2], 3), "max": round(step_ms[-1], 3)}
        if args.dump_steps:
            rec["step_ms_all"] = [round(marks[i].elapsed_time(marks[i + 1]), 2) for i in range(args.steps)]
        if dev_ms is not None:
            rec["device_ms_per_step"], rec["launches_per_step"] = dev_ms
            if int(model.use_streams) > 0:
                rec["device_ms_note"] = "sum of kernel durations: kernels of different branch streams overlap, the sum may exceed the step"
        if not args.no_roofline and args.config == "stress":
            rec["roofline"] = k1_long_roofline(args, device)
        elif not args.no_roofline:   # rank 0's GPU, after the timed region (the other ranks wait at the final barrier)
            rec["roofline"] = k1_roofline(args, device)
            rec["roofline_dense"] = k1_roofline(args, device, dense=True)
            rec["roofline_bwd"] = k1_bwd_roofline(args, device)
            sub_args = argparse.Namespace(**vars(args))
            sub_args.regions = args.sub_words          # the same kernel family on the subtitle stream (50 words per frame)
            rec["roofline_sub"] = k1_roofline(sub_args, device)
            rec["roofline_sub_bwd"] = k1_bwd_roofline(sub_args, device)
            if args.storage == "fp32" and args.hsz == 128:
                rec["roofline_k1k2"] = k1k2_roofline(args, device, model)
            # the same kernels INSIDE the timed steps (training mode, dropout on): `achieved` / `frac` / `avg_us` from there; the
            # back-to-back sequence above stays as `isolated_*` (30 launches in a row run into the chip's power management)
            for name, lr in (("roofline", args.regions), ("roofline_sub", args.sub_words)):
                ts = k1_in_step.get(lr)
                if ts:
                    r = rec[name]
                    avg = sum(ts) / len(ts)
                    r["isolated_avg_us"], r["isolated_min_us"], r["isolated_frac"] = r["avg_us"], r["min_us"], r["frac"]
                    r["avg_us"], r["min_us"] = round(avg * 1e3, 1), round(ts[0] * 1e3, 1)
                    r["achieved"] = round(r["algorithmic_bytes"] / (avg * 1e-3) / 1e9, 1)
                    r["frac"] = round(r["achieved"] / 8000.0, 4)
                    r["timed"] = "HIP events on the launch stream around the kernel in each of the %d timed training steps" % len(ts)
            if (world == 1 and not args.no_pmc and not args.dense and args.storage == "fp32" and
                    (args.bsz, args.frames, args.qa_words, args.hsz, args.regions, args.sub_words) == (16, 300, 40, 128, 20, 50)):
                # `traffic` as an observation of THIS box, not a constant from the repo (published shapes only)
                meas = pmc_traffic_in_run(args)
                for name, key in (("roofline", ("fwd", "vid")), ("roofline_sub", ("fwd", "sub")), ("roofline_bwd", ("bwd", "vid")),
                                  ("roofline_sub_bwd", ("bwd", "sub"))):
                    if key in meas:
                        rec[name]["traffic"] = meas[key]
                        rec[name]["traffic_source"] = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes in this run "
                                                       "(WRITE_SIZE + 2 x FETCH_SIZE, KiB; MI355X_MICROARCH.md)")
        # ragged token rows of this batch (tvqaplus_amd/ragged.py): what the step computed instead of every padded row
        lay = getattr(model, "last_ragged", None)
        if lay is not None:
            dense_rows = lay.N * lay.NA * lay.Li * lay.Lqa
            rr = {"statement_rows": lay.U, "of_padded": dense_rows, "fraction": round(lay.U / dense_rows, 4),
                  "attention_output_rows": lay.Fc, "halo_words": lay.tab.halo}
            for name, cl in getattr(model, "last_ragged_ctx", {}).items():
                rr[name + "_rows"] = {"rows": cl.U, "of_padded": cl.tab.N * cl.tab.Li * cl.tab.L,
                                      "fraction": round(cl.U / float(cl.tab.N * cl.tab.Li * cl.tab.L), 4), "halo": cl.tab.halo}
            rec["config"]["ragged_rows"] = rr
            # the K1 forward kernels inside the step write A for the live frames only and read compact region rows: their bytes in THIS
            # layout next to the SURVEY 8d figure `achieved` / `frac` are quoted on (which counts every padded row)
            for name, key, lr in (("roofline", "vid", args.regions), ("roofline_sub", "sub", args.sub_words)):
                r = rec.get(name)
                cl = getattr(model, "last_ragged_ctx", {}).get(key)
                if r and r.get("timed"):
                    qrows = cl.U if cl is not None else lay.N * lay.Li * lr
                    b_here = 4 * (lay.N * lay.NA * lay.Lqa * args.hsz + qrows * args.hsz + lay.N * lay.NA * lay.Lqa + lay.N * lay.Li * lr
                                  + (lay.Fc - lay.N * lay.NA * lay.Lqa) * args.hsz + 2 * dense_rows * lr)
                    # `achieved` / `frac` = the bytes THIS launch moves / its time (the units the launch processes); the
                    # figure on the reference's dense 696 / 1001 MB (what rounds 1-4 quoted as `frac`) stays as *_reference_bytes
                    r["achieved_reference_bytes"], r["frac_reference_bytes"] = r["achieved"], r["frac"]
                    r["reference_algorithmic_bytes"] = r["algorithmic_bytes"]
                    r["algorithmic_bytes"] = r["bytes_this_layout"] = b_here
                    r["achieved"] = r["achieved_this_layout"] = round(b_here / (r["avg_us"] * 1e-6) / 1e9, 1)
                    r["frac"] = r["frac_this_layout"] = round(r["achieved"] / 8000.0, 4)
                    r["bytes_note"] = ("algorithmic bytes of the ragged launch: A rows of live frames only, compact region rows; "
                                       "score maps dense (they are outputs)")
        if (world == 1 and not args.no_pmc and not args.no_roofline and not args.dense and args.storage == "fp32" and args.config == "default"
                and not args.heads and not args.h2d and int(model.use_streams) >= 0 and
                (args.bsz, args.frames, args.qa_words, args.hsz, args.regions, args.sub_words) == (16, 300, 40, 128, 20, 50)):
            # whole-step roofline: counter bytes of every kernel of the step (one-stream child under rocprofv3) over
            # the step time of THIS run, and the step's fp32-equivalent GEMM work over the fp32 matrix peak
            st = pmc_step_traffic(args)
            if st:
                fl = step_flops(args)
                ms = rec["ms_per_step"]
                rec["step_roofline"] = {
                    "hbm_bytes_per_step": st["bytes_per_step"], "hbm_achieved_gbs": round(st["bytes_per_step"] / (ms * 1e-3) / 1e9, 1),
                    "hbm_peak_gbs": 8000.0, "hbm_frac": round(st["bytes_per_step"] / (ms * 1e-3) / 8e12, 4),
                    "flops_per_step_fp32_equiv": round(fl["step"]), "achieved_tflops": round(fl["step"] / (ms * 1e-3) / 1e12, 2),
                    "mfma_f32_peak_tflops": 157.3, "mfma_frac": round(fl["step"] / (ms * 1e-3) / 157.3e12, 4),
                    "traffic_source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over a one-stream child of %d steps in this run "
                                      "(WRITE_SIZE + 2 x FETCH_SIZE; its one-off setup kernels are counted in: < 2 %%)" % st["steps_profiled"],
                    "flops_note": "GEMM-shaped work only (Linear / 1x1 conv / attention contractions), forward x 3; every product runs as "
                                  "three fp16 MFMA products (2.5 PFLOP/s pipe): the fp32 peak is the yardstick of the arithmetic, not of the pipe",
                    "top_kernels_calls_mb_per_step": st["per_kernel"][:12]}
                # weak #9 of VERDICT r5: `traffic` and `algorithmic_bytes` of ONE launch -- the K1 kernels as they ran IN the step
                for name, key in (("roofline", ("fwd", "vid")), ("roofline_sub", ("fwd", "sub")), ("roofline_bwd", ("bwd", "vid")),
                                  ("roofline_sub_bwd", ("bwd", "sub"))):
                    r = rec.get(name)
                    if r and key in st["k1"]:
                        if "traffic" in r:
                            r["traffic_isolated_dense_launch"] = r["traffic"]
                            r["traffic_isolated_pairs_with"] = r.get("reference_algorithmic_bytes", r.get("algorithmic_bytes"))
                        r["traffic"] = st["k1"][key]
                        r["traffic_source"] = ("in-step launch (ragged layout), rocprofv3 --pmc passes over the one-stream child of this run; "
                                               "pairs with algorithmic_bytes of the same launch")
                        if r.get("algorithmic_bytes"):
                            r["traffic_over_algorithmic"] = round(r["traffic"] / float(r["algorithmic_bytes"]), 3)
        rec["config"]["harness"] = {"gc": args.gc, "adam": args.adam, "clip": args.clip, "loss": args.loss, "ragged_rows": lay is not None,
                                    "branch_streams": int(model.use_streams)}
        if args.storage == "bf16":
            rec["config"]["harness"]["resident_features"] = "fp32" if args.fp32_inputs else "bf16 (as the bf16-staging prefetcher delivers them)"
        if (world == 1 and not args.no_children and args.config == "default" and not args.dense and args.storage == "fp32" and not args.heads
                and not args.h2d):
            side = side_records(args)
            if "roofline_dense" in side and "roofline_dense" in rec:          # in-step timing replaces the isolated sequence
                side["roofline_dense"]["shape"] = rec["roofline_dense"].get("shape")
            rec.update(side)
        if world == 1 and not args.no_cpu_baseline:
            rec["cpu_baseline"] = cpu_baseline(args, opt)
        print(json.dumps(rec))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
