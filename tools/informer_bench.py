#!/usr/bin/env python3
"""An Informer-shaped stack (tests/informer_cases.Stack: the product's layers composed as the reference's models/Informer.py composes
them) forward + backward at the reference's options -- e_layers 2, d_layers 1, factor 3, d_model 512, n_heads 2, d_ff 2048, distil on,
gelu, dropout 0.1, fp32 -- two ways:
  fused      config.informer_fused on: ProbAttention two HIP launches per direction (csrc/prob_attn.hip), ConvLayer's BatchNorm + ELU +
             MaxPool on rows (csrc/conv_distil.hip);
  composed   IMMTSF_INFORMER_FUSED=0: torch gather / sort / scatter, nn.BatchNorm1d, nn.MaxPool1d around the same GEMMs and joints.
In ONE process, after warming both paths: alternating passes of eager steps, then alternating passes of replays of each path's captured
hipGraph (torch.cuda.graph over forward + backward; the samples are drawn on the device inside the graph), host clock around a pass with
a synchronise at its end; a pass runs the number of steps that fills about `--seconds`.  Prints one JSON line: microseconds per step for
both paths in both modes (best pass, and all passes: their min - max is the run-to-run spread), and the device-kernel count of the step each graph captured
(counted on an eager run of the same step: the profiler does not trace the kernels of a replayed graph).

With --model the module is models.Informer of this build and the two ways differ in what is AROUND the layers (the layers stay fused):
  fused      config.informer_model_fused on: the front end one HIP launch and the output tail one (csrc/informer.hip), two each backward;
  composed   IMMTSF_INFORMER_MODEL_FUSED=0: pad / masked norm / cat as torch ops, DataEmbedding, Decoder's own norm and projection.
It then prints one line for the shape above and one for a small shape (B 64, input_len 96, pred_len 24, C 7, d_model 64, d_ff 256).

usage: python tools/informer_bench.py [--model] [--batch 32] [--len 96] [--pred 96] [--channels 8] [--passes 5] [--seconds 0.5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATHS = ("fused", "composed")


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and
               "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--len", type=int, default=96)
    ap.add_argument("--pred", type=int, default=96)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out")
    ap.add_argument("--model", action="store_true", help="models.Informer, fused stages against IMMTSF_INFORMER_MODEL_FUSED=0")
    a = ap.parse_args()
    run(a, a.batch, a.len, a.pred, a.channels, 512, 2048)
    if a.model:
        run(a, 64, 96, 24, 7, 64, 256)


def run(a, B, S, P, C, d_model, d_ff):
    import torch
    import informer_cases as IC
    from immtsf import config, step_plan
    dev = torch.device("cuda:0")
    opts = dict(C=C, c_out=C, input_len=S, pred_len=P, d_model=d_model, n_heads=2, d_ff=d_ff, e_layers=2, d_layers=1, factor=3, distil=True,
                activation="gelu", embed="fixed", freq="h")
    if a.model:
        from models.Informer import Informer as Model
        knob = "informer_model_fused"
    else:
        Model, knob = IC.Stack, "informer_fused"
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    tp = torch.sort(torch.rand(B, S, generator=g), 1).values.to(dev)
    tpp = torch.sort(torch.rand(B, P, generator=g), 1).values.to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)
    models = {n: Model(IC.config(opts, batch_size=B, device=str(dev), dropout=0.1)).to(dev).train() for n in PATHS}
    config.enable_device_counters(dev)      # a replayed graph draws fresh dropout masks

    def step(name):
        m = models[name]
        setattr(config, knob, name == "fused")
        m.zero_grad(set_to_none=True)
        (m.forecasting(tpp, data, tp, mask) * up).sum().backward()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    graphs = {}
    for name in PATHS:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step(name)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        step_plan.collect_before_capture()
        with torch.cuda.graph(graphs[name]):
            step(name)
        graphs[name].replay()
    torch.cuda.synchronize()
    eager, replay = {n: [] for n in PATHS}, {n: [] for n in PATHS}
    n_e = {n: max(3, int(a.seconds * 1e6 / timed(lambda: step(n), 3))) for n in PATHS}
    for _ in range(a.passes):
        for n in PATHS:
            eager[n].append(timed(lambda: step(n), n_e[n]))
    n_r = {n: max(3, int(a.seconds * 1e6 / timed(graphs[n].replay, 3))) for n in PATHS}
    for _ in range(a.passes):
        for n in PATHS:
            replay[n].append(timed(graphs[n].replay, n_r[n]))
    res = {"tool": "informer_bench", "what": "model stages" if a.model else "layers", "B": B, "L": S, "pred": P, "C": C, "d_model": d_model,
           "eager_us": {n: round(min(eager[n]), 1) for n in PATHS}, "replay_us": {n: round(min(replay[n]), 1) for n in PATHS},
           "eager_us_all": {n: [round(t, 1) for t in eager[n]] for n in PATHS},
           "replay_us_all": {n: [round(t, 1) for t in replay[n]] for n in PATHS},
           "graph_kernels": {n: count_kernels(lambda: step(n)) for n in PATHS}}
    setattr(config, knob, True)      # the next shape starts from the default
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
