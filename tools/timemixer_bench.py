#!/usr/bin/env python3
"""TimeMixer.forecasting() forward + backward, fused (csrc/timemixer.hip: one launch forward, two backward) against composed
(IMMTSF_TIMEMIXER_FUSED=0: one embedding kernel per scale, torch element-wise ops around immtsf.ops.linear calls): the reference's
settings -- d_model 16, d_ff 32, e_layers 2, three halvings, moving_avg 25, dropout 0.1 in training mode, fp32 -- with C 5 and
input_len = pred_len = 24, at B in {4, 64, 4096} windows.  Per B, in ONE process, after warming both paths: alternating passes of
`--iters` eager steps each, then alternating passes of replays of each path's captured hipGraph (torch.cuda.graph over forward +
backward), host clock around a pass with a synchronise at its end.  Prints one JSON line per B: microseconds per step for both paths in
both modes (best pass, and all passes), and the device-kernel count of one replay of each graph (torch.profiler).

The driver (no --one) runs every B as a child process under its own time limit and stops at the first that fails.

usage: python tools/timemixer_bench.py [--iters 200] [--passes 3] [--limit 180] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCHES = (4, 64, 4096)
C, S, P, K, D, DFF, E = 5, 24, 24, 25, 16, 32, 2


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and
               "memset" not in e.name.lower())


def one(B, iters, passes):
    import torch
    from immtsf import config
    from models.TimeMixer import TimeMixer
    dev = torch.device("cuda:0")

    def cfg():      # the constructor writes the clipped down_sampling_layers back: one namespace per model
        return types.SimpleNamespace(input_len=S, pred_len=P, enc_in=C, c_out=C, batch_size=B, device=str(dev), moving_avg=K, d_model=D,
                                     d_ff=DFF, e_layers=E, dropout=0.1, embed="timeF", freq="h", top_k=5, decomp_method="moving_avg",
                                     channel_independence=1, down_sampling_layers=3, down_sampling_method="avg", down_sampling_window=2)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    tp = torch.sort(torch.rand(B, S, generator=g), 1).values.to(dev)
    tpp = torch.sort(torch.rand(B, P, generator=g), 1).values.to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)
    models = {"fused": TimeMixer(cfg()).to(dev).train(), "composed": TimeMixer(cfg()).to(dev).train()}
    config.enable_device_counters(dev)      # a replayed graph draws fresh dropout masks

    def step(name):
        m = models[name]
        config.timemixer_fused = name == "fused"
        out = m.forecasting(tpp, data, tp, mask)
        (out * up).sum().backward()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    graphs = {}
    for name, m in models.items():
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                m.zero_grad(set_to_none=True)
                step(name)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        m.zero_grad(set_to_none=True)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            step(name)
        graphs[name].replay()
    assert models["fused"].fused_calls > 0 and models["composed"].fused_calls == 0
    torch.cuda.synchronize()
    eager = {n: [] for n in models}
    replay = {n: [] for n in models}
    for _ in range(passes):
        for name in models:
            eager[name].append(timed(lambda: step(name), iters))
    for _ in range(passes):
        for name in models:
            replay[name].append(timed(graphs[name].replay, iters))
    config.timemixer_fused = True
    line = {"tool": "timemixer_bench", "B": B, "C": C, "S": S, "P": P, "k": K, "d_model": D, "d_ff": DFF, "e_layers": E, "dropout": 0.1, "precision": "fp32", "iters": iters, "passes": passes}
    for name in models:
        line[f"{name}_eager_us"] = round(min(eager[name]), 2)
        line[f"{name}_eager_us_passes"] = [round(v, 2) for v in eager[name]]
        line[f"{name}_replay_us"] = round(min(replay[name]), 2)
        line[f"{name}_replay_us_passes"] = [round(v, 2) for v in replay[name]]
        try:
            line[f"{name}_graph_kernels"] = count_kernels(graphs[name].replay)
        except Exception as e:      # a profiler that cannot trace here must not cost the timing line
            line[f"{name}_graph_kernels"] = repr(e)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds a child process may take")
    ap.add_argument("--one", type=int, default=None, help="run this B in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.passes)
    lines = []
    for B in BATCHES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--iters", str(args.iters),
               "--passes", str(args.passes)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:      # nothing more goes to the GPU after a failure
            sys.exit(f"timemixer_bench: B = {B} ended with status {r.returncode}")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
