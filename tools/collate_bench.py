#!/usr/bin/env python3
"""ResidentStore.collate() in its three forms -- standard, CRU (raw times) and LatentODE (one shared time axis per batch,
csrc/collate.hip immtsf_collate_union) -- against a host baseline, on a synthetic store: 512 windows, C 5, 24 to 48 rows per window
on a 0.01 grid over [0, 48) (history 24), two notes of 16 numbers per window, batches of 64 in window order.

The host baseline is the numpy restatement of the reference's collates that the tests pin to the real reference
(oracle/collate_ref.py, tests/collate_forms_ref.py; tau and the padded note embeddings included) plus the host-to-device copy of its
dict.  Per form, the median over `--passes` passes (a pass is every batch once; figures are per batch) of

  host_us      host clock around collate(), which returns once its launches are queued: what the host spends per batch
  device_us    hipEvents around the same calls: the span on the stream from the first copy to the last kernel
  baseline_us  host clock around restatement + copies, synchronised at the end of the pass

and for the ODE form also axis_us (the host's np.unique over the batch's row times and the count below history, alone),
kernel_us (events around immtsf_collate_union alone, axis already on the device), the mean T and n_obs, and the bytes that launch
writes per second.  Prints one JSON line per form.  No threshold is attached.

usage: python tools/collate_bench.py [--windows 512] [--batch 64] [--channels 5] [--passes 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HISTORY, PRED_WINDOW, D_M = 24.0, 24.0, 16


def make_chunks(W, Cn, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    emb = torch.from_numpy(rng.normal(size=(2 * W, D_M)).astype(np.float32))
    chunks = []
    for w in range(W):
        n = int(rng.integers(24, 49))
        t = np.sort(rng.choice(4700, size=n, replace=False)).astype(np.float32) * np.float32(0.01)
        t[0], t[-1] = np.float32(0.0), np.float32(47.0)          # a row on each side of history
        m = (rng.random((n, Cn)) < 0.7).astype(np.float32)
        v = rng.normal(size=(n, Cn)).astype(np.float32) * m
        chunks.append((f"w{w}", torch.from_numpy(t), torch.from_numpy(v), torch.from_numpy(m),
                       [(1.0, emb[2 * w]), (5.0, emb[2 * w + 1])]))
    return chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--channels", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    import collate_forms_ref as F
    from immtsf import _lib
    from immtsf.data import ResidentStore
    from oracle import collate_ref as R
    dev = torch.device("cuda:0")
    lib = _lib.load()
    chunks = make_chunks(a.windows, a.channels)
    store = ResidentStore.from_chunks(chunks, HISTORY, PRED_WINDOW, dev)
    host = [(c[1].numpy(), c[2].numpy(), c[3].numpy(), np.array([t for t, _ in c[4]], np.float32),
             np.stack([e.numpy() for _, e in c[4]])) for c in chunks]
    batches = [np.arange(i, min(i + a.batch, a.windows)) for i in range(0, a.windows, a.batch)]
    tmax = HISTORY + PRED_WINDOW
    base = {"standard": lambda sel: R.series_collate(sel, HISTORY, tmax), "cru": lambda sel: F.cru_collate(sel, HISTORY),
            "ode": lambda sel: F.ode_collate(sel, HISTORY, tmax)}
    med = lambda xs: round(statistics.median(xs), 1)      # noqa: E731
    lines = []
    for form in ("standard", "cru", "ode"):
        for ids in batches:                                # warm: allocator blocks, pinned blocks, code objects
            store.collate(ids, form=form)
        torch.cuda.synchronize()
        host_us, dev_us, base_us = [], [], []
        for _ in range(a.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for ids in batches:
                store.collate(ids, form=form)
            e1.record()
            host_us.append((time.perf_counter() - t0) * 1e6 / len(batches))
            torch.cuda.synchronize()
            dev_us.append(e0.elapsed_time(e1) * 1e3 / len(batches))
            t0 = time.perf_counter()
            for ids in batches:
                sel = [host[i] for i in ids]
                d = base[form](sel)
                d.update({k: v for k, v in R.notes_collate(sel).items() if k in ("tau", "notes_embeddings")})
                d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev, non_blocking=True) for k, v in d.items()}
            torch.cuda.synchronize()
            base_us.append((time.perf_counter() - t0) * 1e6 / len(batches))
        line = {"form": form, "windows": a.windows, "batch": a.batch, "C": a.channels, "passes": a.passes, "host_us": med(host_us),
                "device_us": med(dev_us), "baseline_us": med(base_us)}
        if form == "ode":
            axis_us, kern_us, Ts, nobs, written = [], [], [], [], 0
            for p in range(a.passes):
                t0 = time.perf_counter()
                axes = [store._union_axis(ids.astype(np.int32)) for ids in batches]
                axis_us.append((time.perf_counter() - t0) * 1e6 / len(batches))
                total = 0.0
                for ids, (axis, n_obs) in zip(batches, axes):
                    B, T = len(ids), len(axis)
                    ids_dev = torch.from_numpy(ids.astype(np.int32)).to(dev)
                    axis_dev = torch.from_numpy(axis).to(dev)
                    o = [torch.empty(s, device=dev) for s in ((n_obs,), (B, n_obs, store.C), (B, n_obs, store.C), (T - n_obs,),
                                                              (B, T - n_obs, store.C), (B, T - n_obs, store.C))]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    _lib.check(lib.immtsf_collate_union(C.byref(store._struct), _lib.ptr(ids_dev), B, _lib.ptr(axis_dev), T, n_obs,
                                                        float(store.time_max), *[_lib.ptr(t) for t in o], _lib.stream_ptr()), "collate_union")
                    e1.record()
                    torch.cuda.synchronize()
                    total += e0.elapsed_time(e1) * 1e3
                    if p == 0:
                        Ts.append(T)
                        nobs.append(n_obs)
                        written += 4 * (T + 2 * B * T * store.C)
                kern_us.append(total / len(batches))
            line.update(axis_us=med(axis_us), kernel_us=med(kern_us), T_mean=round(sum(Ts) / len(Ts), 1),
                        n_obs_mean=round(sum(nobs) / len(nobs), 1), written_bytes_per_batch=written // len(batches),
                        written_GBps=round(written / len(batches) / (med(kern_us) * 1e-6) / 1e9, 2))
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
