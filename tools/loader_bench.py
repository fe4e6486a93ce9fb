#!/usr/bin/env python3
"""One epoch of immtsf.data.ResidentLoader against the path it replaces -- `store.collate(ids)` per batch, each call uploading its own
window ids -- on a seeded synthetic store at cfg2's batch shape: 64 windows per batch, C = 8, up to 32 history and 32 prediction rows
and 1..32 notes of 768 numbers per window; 512 windows, so an epoch is 8 batches, shuffled.

Per form ("standard": one launch per batch, immtsf_collate_batch; "patch": tPatchGNN's, which is cfg2's backbone and keeps its kernels),
`--repeats` epochs of each path, alternating, after `--warmup` epochs of each; a torch.cuda.Event pair around every epoch (the span on
the stream from the first copy to the last kernel) and the host clock around the same loop (what the host spends queueing it).  Prints
one JSON line per form with the medians per epoch, the launches and the host-to-device copies per batch.  No threshold is attached.

usage: python tools/loader_bench.py [--windows 512] [--batch 64] [--repeats 20] [--warmup 3] [--out FILE]
"""
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

HISTORY, PRED_WINDOW, C, D_M, ROWS, N_MAX = 24.0, 24.0, 8, 768, 32, 32


def make_store(W, dev, seed=0):
    import numpy as np

    from immtsf.data import ResidentStore
    rng = np.random.default_rng(seed)
    tt, row_off, tau, note_off = [], [0], [], [0]
    for _ in range(W):
        nh, npred = int(rng.integers(ROWS // 2, ROWS + 1)), int(rng.integers(ROWS // 2, ROWS + 1))
        tt.append(np.concatenate([np.sort(rng.choice(2400, nh, replace=False)), 2400 + np.sort(rng.choice(2400, npred, replace=False))])
                  .astype(np.float32) * np.float32(0.01))
        row_off.append(row_off[-1] + nh + npred)
        n = int(rng.integers(1, N_MAX + 1))
        tau.append(np.sort(rng.random(n) * HISTORY).astype(np.float32))
        note_off.append(note_off[-1] + n)
    R, S = row_off[-1], note_off[-1]
    mask = (rng.random((R, C)) < 0.7).astype(np.float32)
    vals = rng.normal(size=(R, C)).astype(np.float32) * mask
    emb = rng.normal(size=(S, D_M)).astype(np.float32)
    return ResidentStore(np.concatenate(tt), vals, mask, np.array(row_off, np.int64), np.concatenate(tau), np.arange(S, dtype=np.int64),
                         np.array(note_off, np.int64), emb, HISTORY, PRED_WINDOW, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats must be at least 10")
    import numpy as np
    import torch

    from immtsf.data import ResidentLoader
    dev = torch.device("cuda:0")
    store = make_store(a.windows, dev)
    n_batches = -(-a.windows // a.batch)
    med = lambda xs: round(statistics.median(xs), 1)      # noqa: E731
    lines = []
    for form, patch in (("standard", None), ("patch", (8, 3, 8))):
        loader = ResidentLoader(store, np.arange(a.windows), a.batch, True, patch=patch, generator=torch.Generator().manual_seed(1))
        order_gen = torch.Generator().manual_seed(1)

        def resident():
            for _ in loader:
                pass

        def per_batch():      # the same epoch order, every batch through collate() with its own id upload
            order = torch.randperm(a.windows, generator=order_gen).numpy()
            for k in range(0, a.windows, a.batch):
                store.collate(order[k:k + a.batch], patch=patch)

        paths = {"resident": resident, "per_batch": per_batch}
        counts = {}
        for name, fn in paths.items():         # warm: allocator blocks, pinned blocks, code objects, the patch populations
            for _ in range(a.warmup):
                fn()
            who = loader if name == "resident" else store      # the loader counts its epoch upload and what its batches issue
            c0, l0 = who.h2d_copies, who.launches
            fn()
            counts[name] = ((who.launches - l0) / n_batches, (who.h2d_copies - c0) / n_batches)
        torch.cuda.synchronize()
        dev_us = {k: [] for k in paths}
        host_us = {k: [] for k in paths}
        for _ in range(a.repeats):
            for name, fn in paths.items():     # alternating: both paths see the same machine
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                host_us[name].append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
                dev_us[name].append(e0.elapsed_time(e1) * 1e3)
        line = {"form": form, "windows": a.windows, "batch": a.batch, "batches_per_epoch": n_batches, "C": C, "d_m": D_M,
                "repeats": a.repeats, "warmup": a.warmup}
        for name in paths:
            line[name] = {"epoch_device_us": med(dev_us[name]), "epoch_host_us": med(host_us[name]),
                          "device_us_min_max": [round(min(dev_us[name]), 1), round(max(dev_us[name]), 1)],
                          "launches_per_batch": counts[name][0], "h2d_copies_per_batch": round(counts[name][1], 3)}
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
