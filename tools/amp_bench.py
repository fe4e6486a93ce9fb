"""`scaler.step(opt); scaler.update()` of immtsf.optim.FusedAdam under torch.amp.GradScaler: the loss-scale route (the scale, the clip on
the stored gradient and the skip decision inside immtsf_adam_prepare_scaled / immtsf_adam_range_scaled) against GradScaler's generic
route (IMMTSF_OPTIM_AMP=0: a foreach unscale over every .grad, a host read of found_inf, then the plain fused step).

    python tools/amp_bench.py [--elements 8000000] [--tensors 300] [--iters 200] [--rounds 5] [--out FILE.md]

Method: both routes live in one process on their own parameters and are timed in alternating rounds; a step is timed by a host clock
around the two calls ending in a device synchronise (the generic route synchronises by itself, the other must be made to), after a
warm-up of every route; the gradient is refilled (scaled, finite) before each step outside the timed stretch, the clip is pending as
in main.py's loop.  Reported: the median step of every round, then median and range over the rounds.  Kernel launches per step are
counted in a separate pass under torch.profiler (tracing slows the host: never in the timed pass).  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def build(dev, elements, tensors, amp, seed=0):
    from immtsf import config, optim
    gen = torch.Generator().manual_seed(seed)
    # unequal sizes, none a multiple of 8, summing to ~`elements` (cfg2's parameter count is ~8.0 M over a few hundred tensors)
    w = torch.rand(tensors, generator=gen) + 0.05
    sizes = [int(x) | 1 for x in (w / w.sum() * elements).tolist()]
    params = [torch.nn.Parameter(torch.randn(k, generator=gen).to(dev)) for k in sizes]
    old = config.optim_amp
    config.optim_amp = amp
    try:
        opt = optim.Adam(params, lr=1e-3, weight_decay=0.01)
    finally:
        config.optim_amp = old
    assert isinstance(opt, optim.FusedAdam) and opt._step_supports_amp_scaling == amp
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    scaler.scale(torch.zeros((), device=dev))                       # (creates the scale tensors)
    grad = torch.randn(opt.flat_grad.numel(), generator=gen).to(dev) * 1e-3 * 65536.0
    return dict(params=params, opt=opt, scaler=scaler, grad=grad, n=sum(sizes))


def one_step(r, timed=True):
    from immtsf import optim
    r["opt"].zero_grad()
    r["opt"].flat_grad.copy_(r["grad"])
    optim.clip_grad_norm_(r["params"], 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r["scaler"].step(r["opt"])
    r["scaler"].update()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launches(r, steps=5):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                r["scaler"].step(r["opt"])
                r["scaler"].update()
                r["opt"].flat_grad.copy_(r["grad"])                  # (one copy kernel per step: subtracted below)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                   and "Memset" not in e.name]
        return (len(kernels) - steps) / steps
    except Exception as e:                                            # noqa: BLE001  (a profiler that is not there is not a timing failure)
        print(f"launch count not measured: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=8_000_000)
    ap.add_argument("--tensors", type=int, default=300)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("amp_bench needs the GPU: a CPU run would time nothing this project runs")
    dev = torch.device("cuda:0")
    routes = {"loss-scale route": build(dev, a.elements, a.tensors, True), "generic route (IMMTSF_OPTIM_AMP=0)": build(dev, a.elements, a.tensors, False)}
    for r in routes.values():
        for _ in range(20):
            one_step(r)
    med = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, r in routes.items():
            med[k].append(statistics.median(one_step(r) for _ in range(a.iters)) * 1e6)
    res = {"elements": next(iter(routes.values()))["n"], "tensors": a.tensors, "iters": a.iters, "rounds": a.rounds}
    lines = ["# `scaler.step(opt); scaler.update()` under torch.amp.GradScaler", "",
             f"{res['elements']} parameters in {a.tensors} tensors, fp32, clip pending, finite gradients; host clock around the two calls "
             f"ending in a device synchronise; median of {a.iters} steps per round, {a.rounds} alternating rounds (`tools/amp_bench.py`).", "",
             "| route | step, median of the rounds (us) | rounds, min - max (us) | kernel launches per step |", "|---|---|---|---|"]
    for k, r in routes.items():
        n_launch = launches(r)
        res[k] = {"us_median": statistics.median(med[k]), "us_rounds": med[k], "launches_per_step": n_launch}
        lines.append(f"| {k} | {statistics.median(med[k]):.1f} | {min(med[k]):.1f} - {max(med[k]):.1f} | "
                     f"{'not measured' if n_launch is None else f'{n_launch:.1f}'} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
