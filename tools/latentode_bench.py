#!/usr/bin/env python3
"""LatentODE.forecasting() forward + backward, fused (csrc/latent_ode.hip: one launch forward, two backward) against composed
(IMMTSF_LATENTODE_FUSED=0: the reference's Python loop over the observed points on torch ops): the reference's defaults -- latents 20,
rec_dims 32, units 32, gru_units 32, fp32 -- with C 5 and L = Lp = 24 (config 2's window) on one shared time axis (observed times sorted
uniform draws in [0, 1], forecast times in (1, 2]), at B = 64 windows, every parameter 0.1 randn off its init (the biases start at
zero).  In ONE process, after warming both paths: alternating passes of `--iters` eager steps each, then passes of replays of the fused
path's captured hipGraph (torch.cuda.graph over forward + backward), host clock around a pass with a synchronise at its end.  Prints
one JSON line per B: microseconds per step for both paths (best pass, and all passes), the device-kernel count of one eager step of each
path and of one replay of the fused graph (torch.profiler), all kernels and the backbone's own (lo_*), and the step plan's totals.  The
composed path is captured last and is refused (it copies the step plan to the host): its replay time is then null and the line
carries the error.

The driver (no --one) runs every B as a child process under its own time limit and stops at the first that fails.

usage: python tools/latentode_bench.py [--iters 20] [--passes 3] [--limit 300] [--out FILE]
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

BATCHES = (64,)
C, S, P = 5, 24, 24


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and
             "memset" not in e.name.lower()]
    return len(names), sum(1 for n in names if "lo_" in n)


def one(B, iters, passes):
    import torch
    from immtsf import config
    from models.LatentODE import LatentODE, step_plan
    dev = torch.device("cuda:0")

    def model():
        torch.manual_seed(0)
        m = LatentODE(types.SimpleNamespace(C=C, device=dev, dataset="bench"))
        gp = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=gp).to(dev))
        return m.train()
    g = torch.Generator().manual_seed(1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    tp = torch.sort(torch.rand(S, generator=g)).values.to(dev)
    tpp = (1.0 + torch.sort(torch.rand(P, generator=g) * 0.999 + 0.001).values).to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)
    models = {"fused": model(), "composed": model()}

    def step(name):
        m = models[name]
        config.latentode_fused = name == "fused"
        out = m.forecasting(tpp, data, tp, mask)
        (out * up).sum().backward()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    def warm(name):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                models[name].zero_grad(set_to_none=True)
                step(name)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        models[name].zero_grad(set_to_none=True)

    def capture(name):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(name)
        graph.replay()
        torch.cuda.synchronize()
        return graph

    for name in models:
        warm(name)
    graphs = {"fused": capture("fused")}
    assert models["fused"].fused_calls > 0 and models["composed"].fused_calls == 0
    eager = {n: [] for n in models}
    replay = {n: [] for n in models}
    for _ in range(passes):
        for name in models:
            eager[name].append(timed(lambda: step(name), iters))
    for _ in range(passes):
        replay["fused"].append(timed(graphs["fused"].replay, iters))
    euler, nsub, _ = step_plan(tp)
    line = {"tool": "latentode_bench", "B": B, "C": C, "L": S, "Lp": P, "latents": 20, "rec_dims": 32, "units": 32, "gru_units": 32,
            "precision": "fp32", "iters": iters, "passes": passes, "euler_steps": int(euler.sum()),
            "encoder_rk4_steps": int(((nsub - 1) * (~euler)).sum())}
    for name in models:
        line[f"{name}_eager_us"] = round(min(eager[name]), 2)
        line[f"{name}_eager_us_passes"] = [round(v, 2) for v in eager[name]]
        try:      # the launches of ONE eager step (a profiler that cannot trace here must not cost the timing line)
            line[f"{name}_step_kernels"], line[f"{name}_step_lo_kernels"] = count_kernels(lambda: step(name))
        except Exception as e:
            line[f"{name}_step_kernels"] = repr(e)
    line["fused_replay_us"] = round(min(replay["fused"]), 2)
    line["fused_replay_us_passes"] = [round(v, 2) for v in replay["fused"]]
    try:
        line["fused_graph_kernels"], line["fused_graph_lo_kernels"] = count_kernels(graphs["fused"].replay)
    except Exception as e:
        line["fused_graph_kernels"] = repr(e)
    # last, because a refused capture ends this process's GPU work: the composed path copies the step plan to the host, and a stream
    # that is capturing refuses that copy
    try:
        graphs["composed"] = capture("composed")
        for _ in range(passes):
            replay["composed"].append(timed(graphs["composed"].replay, iters))
        line["composed_replay_us"] = round(min(replay["composed"]), 2)
        line["composed_replay_us_passes"] = [round(v, 2) for v in replay["composed"]]
    except Exception as e:
        line["composed_replay_us"] = None
        line["composed_capture_error"] = str(e).splitlines()[0][:160]
    config.latentode_fused = True
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
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
            sys.exit(f"latentode_bench: B = {B} ended with status {r.returncode}")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
