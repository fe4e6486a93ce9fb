#!/usr/bin/env python3
"""Evaluation pass, eager against immtsf.EvalStep: cfg2, bf16 mode, 64 windows, 200 distinct synthetic batches drawn from 8 recurring
shapes, model and fusion in eval().  In ONE process, after warming every shape, three alternating passes of
  (a) lib.evaluation.evaluation() with immtsf.config.eval_engine off (the eager forward + the metrics as torch ops), and
  (b) the same call with the engine on (replayed forward graph + fused metric kernel),
each ending in its own synchronising read, host clock around the whole pass.  Prints one JSON line: ms per batch for both, the spread
over the three passes, and kernel launches per batch for both (the library's timing tap does not see torch's kernels, so launches are
counted by torch.profiler on one extra pass each; --no-launch-count skips that).

usage: python tools/eval_bench.py [--batches 200] [--windows 64] [--passes 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WINDOWS = (64, 60, 56, 52, 48, 44, 40, 36)      # the 8 recurring shapes: full batches and the ragged ends of several loaders


def make_batches(n, windows, dev):
    import bench
    scale = windows / 64.0
    out = []
    for i in range(n):
        B = max(1, int(round(WINDOWS[i % len(WINDOWS)] * scale)))
        cpu, _ = bench.synth_batch(1000 + i, B)
        out.append({k: v.to(dev) for k, v in cpu.items()})
    return out


def timed_pass(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def count_launches(fn, n_batches):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = graphs = 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            kernels += 1
        elif e.name in ("hipGraphLaunch", "cudaGraphLaunch"):
            graphs += 1
    return {"device_kernels_per_batch": round(kernels / n_batches, 2), "graph_launches_per_batch": round(graphs / n_batches, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from immtsf import config
    from lib.evaluation import _eval_steps, evaluation
    dev = torch.device("cuda:0")
    w = bench.Workload("cfg2", dev, args.windows, args.precision)      # its trainer stays alive, as in a training process that validates:
    model, fusion = w.model.eval(), w.fusion.eval()                     # the bf16 parameter twins are registered on both paths
    batches = make_batches(args.batches, args.windows, dev)

    def run(engine):
        config.eval_engine = engine
        try:
            return evaluation(model, fusion, batches)
        finally:
            config.eval_engine = False

    # warm every shape on both paths (the engine captures a shape at its second sighting: two passes)
    run(False)
    run(True)
    run(True)
    ev = next(iter(_eval_steps[model].values()))
    eager_ms, engine_ms, res = [], [], {}
    for _ in range(args.passes):
        ms, res["eager"] = timed_pass(lambda: run(False))
        eager_ms.append(ms / len(batches))
        r0 = ev.replays
        ms, res["engine"] = timed_pass(lambda: run(True))
        engine_ms.append(ms / len(batches))
        assert ev.replays - r0 == len(batches), "a timed engine pass ran a batch eagerly"
    line = {
        "tool": "eval_bench", "config": "cfg2", "precision": args.precision, "windows": args.windows, "batches": len(batches),
        "shapes": len(WINDOWS), "passes": args.passes,
        "eager_ms_per_batch": round(min(eager_ms), 4), "eager_ms_per_batch_passes": [round(v, 4) for v in eager_ms],
        "eager_spread_ms": round(max(eager_ms) - min(eager_ms), 4),
        "engine_ms_per_batch": round(min(engine_ms), 4), "engine_ms_per_batch_passes": [round(v, 4) for v in engine_ms],
        "engine_spread_ms": round(max(engine_ms) - min(engine_ms), 4),
        "speedup": round(min(eager_ms) / min(engine_ms), 2),
        "engine_graphs_cached": len(ev._graphs),
        "metrics_eager": res["eager"], "metrics_engine": res["engine"],
    }
    if not args.no_launch_count:
        try:
            line["eager_launches"] = count_launches(lambda: run(False), len(batches))
            line["engine_launches"] = count_launches(lambda: run(True), len(batches))
        except Exception as e:      # a profiler that cannot trace here must not cost the timing line
            line["launch_count_error"] = repr(e)
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
