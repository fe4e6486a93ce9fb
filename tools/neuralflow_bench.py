#!/usr/bin/env python3
"""NeuralFlow.forecasting() forward + backward, fused (csrc/neural_flow.hip: two launches forward, three backward) against composed
(IMMTSF_NEURALFLOW_FUSED=0: the reference's Python loop over the observed points on torch ops): the widths the reference's main.py forces
for this model -- coupling flow, 2 flow layers, hidden [32, 32, 32], rec_dims 40, latents 20, fp32, the time net of --time-net
(TimeLinear, or TimeTanh: the kernels' TimeTanh instance, which the tool admits with config.neuralflow_tanh_fused) -- with C 5 and
L = Lp = 24 (config 2's window), every window with its own times (observed times sorted uniform draws in [0, 0.6], forecast times in
[0.62, 1]), at B = 64 windows, every parameter 0.1 randn off its init.  In ONE process, after warming both paths: alternating passes of
`--iters` eager steps each, then passes of replays of each path's captured hipGraph (torch.cuda.graph over forward + backward; neither
path syncs with the host), host clock around a pass with a synchronise at its end.  Prints one JSON line per B: microseconds per step
for both paths, eager and replayed (best pass, and all passes), and the device-kernel count of one eager step and of one replay of each
path's graph (torch.profiler), all kernels and the backbone's own (nf_*).

The driver (no --one) runs every B as a child process under its own time limit and stops at the first that fails.

usage: python tools/neuralflow_bench.py [--time-net TimeLinear|TimeTanh] [--iters 20] [--passes 3] [--limit 300] [--out FILE]
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
    return len(names), sum(1 for n in names if "nf_" in n)


def one(B, iters, passes, time_net):
    import torch
    from immtsf import config
    from models.NeuralFlow import NeuralFlow
    dev = torch.device("cuda:0")
    config.neuralflow_tanh_fused = True      # only a TimeTanh model reads it

    def model():
        torch.manual_seed(0)
        m = NeuralFlow(types.SimpleNamespace(input_len=S, pred_len=P, enc_in=C, device=dev, nf_time_net=time_net))
        gp = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=gp).to(dev))
        return m.train()
    g = torch.Generator().manual_seed(1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    data = data * mask
    tp = torch.sort(torch.rand(B, S, generator=g) * 0.6, dim=1).values.to(dev)
    tpp = (0.62 + torch.sort(torch.rand(B, P, generator=g) * 0.38, dim=1).values).to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)
    models = {"fused": model(), "composed": model()}

    def step(name):
        m = models[name]
        config.neuralflow_fused = name == "fused"
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
    graphs = {name: capture(name) for name in models}
    assert models["fused"].fused_calls > 0 and models["composed"].fused_calls == 0
    eager = {n: [] for n in models}
    replay = {n: [] for n in models}
    for _ in range(passes):
        for name in models:
            eager[name].append(timed(lambda: step(name), iters))
    for _ in range(passes):
        for name in models:
            replay[name].append(timed(graphs[name].replay, iters))
    a = models["fused"].nf_args
    line = {"tool": "neuralflow_bench", "B": B, "C": C, "L": S, "Lp": P, "latents": a.latents, "rec_dims": a.rec_dims,
            "hidden": [a.hidden_dim] * a.hidden_layers, "flow_layers": a.flow_layers, "time_net": a.time_net, "precision": "fp32",
            "iters": iters, "passes": passes}
    for name in models:
        line[f"{name}_eager_us"] = round(min(eager[name]), 2)
        line[f"{name}_eager_us_passes"] = [round(v, 2) for v in eager[name]]
        line[f"{name}_replay_us"] = round(min(replay[name]), 2)
        line[f"{name}_replay_us_passes"] = [round(v, 2) for v in replay[name]]
        try:      # the launches of ONE step (a profiler that cannot trace here must not cost the timing line)
            line[f"{name}_step_kernels"], line[f"{name}_step_nf_kernels"] = count_kernels(lambda: step(name))
            line[f"{name}_graph_kernels"], line[f"{name}_graph_nf_kernels"] = count_kernels(graphs[name].replay)
        except Exception as e:
            line[f"{name}_step_kernels"] = repr(e)
    config.neuralflow_fused = True
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--one", type=int, default=None, help="run this B in this process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--time-net", default="TimeLinear", choices=("TimeLinear", "TimeTanh"))
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.passes, args.time_net)
    lines = []
    for B in BATCHES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--iters", str(args.iters),
               "--passes", str(args.passes), "--time-net", args.time_net]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:      # nothing more goes to the GPU after a failure
            sys.exit(f"neuralflow_bench: B = {B} ended with status {r.returncode}")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
