#!/usr/bin/env python3
"""TTM.forecasting() forward + backward at the reference's TTM defaults -- d_model 1024, AP_levels 3, e_layers 3, d_layers 2, d_d_model 64,
mix_channel, decoder, use_norm, C 8, input_len = pred_len = 33, patch_size 6, stride 24, fp32 -- three ways:
  fused      the product with config.ttm_fused on: every narrow mixer block one HIP launch (csrc/ttm.hip), dropout 0.1 in training mode;
  composed   the product with IMMTSF_TTM_FUSED=0: torch permutes and element-wise ops around immtsf.ops.linear / layer_norm, dropout 0.1;
  torch      the yardstick: the reference's formulation on stock PyTorch (tests/ttm_ref.py in fp32 on the GPU, which applies NO dropout:
             it does less work than the other two).
Per B, in ONE process, after warming every path: alternating passes of eager steps, then alternating passes of replays of each path's
captured hipGraph (torch.cuda.graph over forward + backward), host clock around a pass with a synchronise at its end; a pass runs the
number of steps that fills about `--seconds`.  Prints one JSON line per B: microseconds per step for the three paths in both modes (best
pass, and all passes: their min - max is the run-to-run spread), and the device-kernel count of one replay of each graph.

The driver (no --one) runs B = 4, 64 and the largest power of two <= --largest that fits in memory, each as a child process under its own
time limit; a child that runs out of memory ends with status 3 and the driver halves B; any other failure stops the driver.

usage: python tools/ttm_bench.py [--passes 5] [--seconds 0.5] [--largest 4096] [--limit 300] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OPTS = dict(enc_in=8, input_len=33, pred_len=33, patch_size=6, stride=24, d_model=1024, AP_levels=3, e_layers=3, d_layers=2, d_d_model=64,
            mode="mix_channel", use_decoder=True, use_norm=1)
PATHS = ("fused", "composed", "torch")


def count_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and
               "memset" not in e.name.lower())


def one(B, passes, seconds):
    import torch
    import ttm_ref
    from immtsf import config, step_plan
    from models.TTM import TTM
    dev = torch.device("cuda:0")
    C, S, P = OPTS["enc_in"], OPTS["input_len"], OPTS["pred_len"]
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    data = torch.randn(B, S, C, generator=g).to(dev)
    mask = (torch.rand(B, S, C, generator=g) < 0.7).float().to(dev)
    tp = torch.sort(torch.rand(B, S, generator=g), 1).values.to(dev)
    tpp = torch.sort(torch.rand(B, P, generator=g), 1).values.to(dev)
    up = torch.randn(B, P, C, generator=g).to(dev)

    def cfg():      # the constructor writes n_vars and num_patches back: one namespace per model
        return types.SimpleNamespace(batch_size=B, device=str(dev), dropout=0.1, **OPTS)
    models = {"fused": TTM(cfg()).to(dev).train(), "composed": TTM(cfg()).to(dev).train()}
    ref = {k: v.detach().clone().requires_grad_(True) for k, v in models["fused"].state_dict().items()}
    config.enable_device_counters(dev)      # a replayed graph draws fresh dropout masks

    def step(name):
        if name == "torch":
            for v in ref.values():
                v.grad = None
            out = ttm_ref.forward(ref, data, mask, tp, P, OPTS)
        else:
            m = models[name]
            config.ttm_fused = name == "fused"
            m.zero_grad(set_to_none=True)
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
    try:
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
    except RuntimeError as e:      # torch.cuda.OutOfMemoryError is one; inside a capture the allocator's failure can be a plain one
        if not (isinstance(e, torch.cuda.OutOfMemoryError) or "out of memory" in str(e).lower()):
            raise
        print(json.dumps({"tool": "ttm_bench", "B": B, "oom": True}), flush=True)
        sys.exit(3)
    blocks = len(models["fused"].mixer_blocks())
    assert models["fused"].fused_blocks == blocks and models["composed"].fused_blocks == 0
    eager = {n: [] for n in PATHS}
    replay = {n: [] for n in PATHS}
    n_e = {n: max(3, int(seconds * 1e6 / timed(lambda: step(n), 3))) for n in PATHS}
    n_r = {n: max(3, int(seconds * 1e6 / timed(graphs[n].replay, 3))) for n in PATHS}
    for _ in range(passes):
        for name in PATHS:
            eager[name].append(timed(lambda: step(name), n_e[name]))
    for _ in range(passes):
        for name in PATHS:
            replay[name].append(timed(graphs[name].replay, n_r[name]))
    config.ttm_fused = True
    line = {"tool": "ttm_bench", "B": B, **{k: OPTS[k] for k in ("enc_in", "input_len", "patch_size", "stride", "d_model", "AP_levels",
                                                               "e_layers", "d_layers", "d_d_model")},
            "mixer_blocks": blocks, "dropout": 0.1, "precision": "fp32", "passes": passes,
            "peak_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    for name in PATHS:
        line[f"{name}_eager_us"] = round(min(eager[name]), 1)
        line[f"{name}_eager_us_passes"] = [round(v, 1) for v in eager[name]]
        line[f"{name}_replay_us"] = round(min(replay[name]), 1)
        line[f"{name}_replay_us_passes"] = [round(v, 1) for v in replay[name]]
        try:
            line[f"{name}_graph_kernels"] = count_kernels(graphs[name].replay)
        except Exception as e:      # a profiler that cannot trace here must not cost the timing line
            line[f"{name}_graph_kernels"] = repr(e)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="about how long one timed pass runs")
    ap.add_argument("--largest", type=int, default=4096, help="the power of two the search for the largest B starts at")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child process may take")
    ap.add_argument("--one", type=int, default=None, help="run this B in this process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.passes, args.seconds)
    lines = []

    def child(B):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(B), "--passes",
               str(args.passes), "--seconds", str(args.seconds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.extend(ln for ln in r.stdout.splitlines() if ln.startswith("{"))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return r.returncode
    for B in (4, 64):
        rc = child(B)
        if rc != 0:      # nothing more goes to the GPU after a failure
            sys.exit(f"ttm_bench: B = {B} ended with status {rc}")
    B = args.largest
    while B > 64:
        rc = child(B)
        if rc == 0:
            break
        if rc != 3:
            sys.exit(f"ttm_bench: B = {B} ended with status {rc}")
        B //= 2


if __name__ == "__main__":
    main()
