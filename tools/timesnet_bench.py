#!/usr/bin/env python3
"""TimesNet.forecasting() forward + backward with the period selection as the project's own launches (immtsf.ops.timesnet_spectrum,
csrc/timesnet_spectrum.hip: a direct DFT, two launches forward and one backward per TimesBlock) against IMMTSF_TIMESNET_SPECTRUM_FUSED=0
(torch.fft.rfft / abs / mean / cat / topk / index_select / softmax / pad and autograd's mirror of each), fp32, at two shapes: cfg4's (64
windows, input_len = pred_len = 32, d_model 16, d_ff 32, top_k 5, 2 layers, 6 Inception kernels) and a long wide one (64 windows, input_len
= pred_len = 96, d_model 64: a (192, 64) tile per window, the largest the route is required to take).  Per shape, in ONE process, after
warming both paths: alternating passes of `--iters` eager steps each, then alternating passes of replays of each path's captured hipGraph
(torch.cuda.graph over forward + backward), host clock around a pass with a synchronise at its end.  Prints one JSON line per shape:
microseconds per step for both paths in both modes (best pass, and all passes) and the number of kernel nodes of each graph (read from
the graph itself; the library's timing tap does not see torch's kernels).

With --model the two paths differ in what is AROUND the TimesBlock loop instead (the period selection stays on its default):
  fused   config.timesnet_model_fused on: the front end one HIP launch (csrc/timesnet_model.hip) and the output tail one, two each backward;
  torch   IMMTSF_TIMESNET_MODEL_FUSED=0: pad / instance norm / cat / DataEmbedding / cat / permuted predict_linear, and layer_norm + projection
          over all rows + de-normalisation + slice.
IMMTSF_TIMESNET_MODEL_SAVE_E=1 makes the fused front end keep its embedded rows for the backward instead of forming them again.

The driver (no --one) runs every shape as a child process under its own time limit and stops at the first that fails.

usage: python tools/timesnet_bench.py [--model] [--iters 200] [--passes 3] [--limit 240] [--out FILE]
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

SHAPES = {      # name -> B, input_len, pred_len, enc_in, d_model, d_ff, top_k, e_layers, num_kernels
    "cfg4": dict(B=64, input_len=32, pred_len=32, enc_in=8, d_model=16, d_ff=32, top_k=5, e_layers=2, num_kernels=6),
    "t192n64": dict(B=64, input_len=96, pred_len=96, enc_in=8, d_model=64, d_ff=64, top_k=5, e_layers=2, num_kernels=2),
}
PATHS = ("fused", "torch")


def count_kernels(graph):
    """the kernel nodes of a captured graph (torch.cuda.CUDAGraph(keep_graph=True)), child graphs included: read from the graph itself
    (hipGraphGetNodes / hipGraphNodeGetType), so nothing has to trace a replay"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    KERNEL, CHILD = 0, 4      # hipGraphNodeTypeKernel, hipGraphNodeTypeGraph

    def nodes_of(g):
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(g, None, ctypes.byref(n)) != 0:
            raise RuntimeError("hipGraphGetNodes failed")
        arr = (ctypes.c_void_p * max(n.value, 1))()
        if n.value and hip.hipGraphGetNodes(g, arr, ctypes.byref(n)) != 0:
            raise RuntimeError("hipGraphGetNodes failed")
        return [ctypes.c_void_p(arr[i]) for i in range(n.value)]

    def count(g):
        total = 0
        for node in nodes_of(g):
            t = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(node, ctypes.byref(t)) != 0:
                raise RuntimeError("hipGraphNodeGetType failed")
            if t.value == KERNEL:
                total += 1
            elif t.value == CHILD:
                child = ctypes.c_void_p()
                if hip.hipGraphChildGraphNodeGetGraph(node, ctypes.byref(child)) != 0:
                    raise RuntimeError("hipGraphChildGraphNodeGetGraph failed")
                total += count(child)
        return total

    return count(ctypes.c_void_p(graph.raw_cuda_graph()))


KNOBS = {False: "timesnet_spectrum_fused", True: "timesnet_model_fused"}      # --model -> the config attribute the two paths differ in


def make(shape, B=None, seed=0, model=False):
    """-> (models {path: TimesNet}, step(path) -> forecast: one forward + backward of that path's model on one fixed batch).  Both models
    start from the same parameters.  model: the paths differ in config.timesnet_model_fused instead of config.timesnet_spectrum_fused."""
    import torch
    from immtsf import config
    from models.TimesNet import TimesNet
    s = dict(SHAPES[shape])
    B0 = s.pop("B")
    B = B0 if B is None else int(B)
    dev = torch.device("cuda:0")
    cfg = types.SimpleNamespace(batch_size=B, device=str(dev), dropout=0.0, embed="fixed", freq="h", c_out=s["enc_in"], **s)
    S, P, C = s["input_len"], s["pred_len"], s["enc_in"]
    g = torch.Generator().manual_seed(seed + 1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    tp = torch.sort(torch.rand(B, S, generator=g), 1).values.to(dev)
    tpp = torch.sort(torch.rand(B, P, generator=g), 1).values.to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)
    data = data * mask
    models = {}
    for name in PATHS:
        torch.manual_seed(seed)
        models[name] = TimesNet(cfg).to(dev).train()

    def step(name):
        knob = KNOBS[bool(model)]
        was, bound = getattr(config, knob), config.timesnet_model_max_work
        setattr(config, knob, name == "fused")
        if model:
            config.timesnet_model_max_work = None      # the kernels at every shape: this tool is what the routing bound is read from
        try:
            out = models[name].forecasting(tpp, data, tp, mask)
            (out * up).sum().backward()
        finally:
            setattr(config, knob, was)
            config.timesnet_model_max_work = bound
        return out

    return models, step


def capture(models, step, name):
    """the path's forward + backward as a replayable graph (warmed on a side stream first) -> (graph, the forecast it rewrites)"""
    import torch
    m = models[name]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            m.zero_grad(set_to_none=True)
            step(name)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph(keep_graph=True)      # (count_kernels reads its nodes)
    with torch.cuda.graph(graph):
        out = step(name)
    graph.replay()
    torch.cuda.synchronize()
    return graph, out


def spectrum_calls(model):
    return sum(blk.spectrum_calls for blk in model.model)


def one(shape, iters, passes, model=False):
    import torch
    models, step = make(shape, model=model)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    graphs = {name: capture(models, step, name)[0] for name in PATHS}
    if model:
        assert models["fused"].fused_calls > 0 and models["torch"].fused_calls == 0
    else:
        assert spectrum_calls(models["fused"]) > 0 and spectrum_calls(models["torch"]) == 0
    eager = {n: [] for n in PATHS}
    replay = {n: [] for n in PATHS}
    for _ in range(passes):
        for name in PATHS:
            eager[name].append(timed(lambda: step(name), iters))
    for _ in range(passes):
        for name in PATHS:
            replay[name].append(timed(graphs[name].replay, iters))
    s = SHAPES[shape]
    line = {"tool": "timesnet_bench", "what": "model stages" if model else "period selection", "shape": shape, **s, "T": s["input_len"] + s["pred_len"], "precision": "fp32", "iters": iters,
            "passes": passes}
    for name in PATHS:
        line[f"{name}_eager_us"] = round(min(eager[name]), 2)
        line[f"{name}_eager_us_passes"] = [round(v, 2) for v in eager[name]]
        line[f"{name}_replay_us"] = round(min(replay[name]), 2)
        line[f"{name}_replay_us_passes"] = [round(v, 2) for v in replay[name]]
        try:
            line[f"{name}_graph_kernels"] = count_kernels(graphs[name])
        except Exception as e:      # a runtime that cannot list the nodes must not cost the timing line
            line[f"{name}_graph_kernels"] = repr(e)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--one", default=None, choices=sorted(SHAPES), help="run this shape in this process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", action="store_true", help="the fused front end and tail against IMMTSF_TIMESNET_MODEL_FUSED=0")
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.passes, args.model)
    lines = []
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", shape, "--iters", str(args.iters),
               "--passes", str(args.passes)] + (["--model"] if args.model else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:      # nothing more goes to the GPU after a failure
            sys.exit(f"timesnet_bench: shape {shape} ended with status {r.returncode}")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
