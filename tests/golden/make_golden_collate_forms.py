#!/usr/bin/env python3
"""Golden vectors for the CRU and LatentODE forms of the batch builder from the REAL reference data path.

Run where the reference tree is at hand (IMMTSF_REFERENCE names it, as for make_golden.py):

    python tests/golden/make_golden_collate_forms.py

Reuses the synthetic on-disk dataset of make_golden_collate.py (`write_dataset`, `ref_args`; its bytes are kept in
collate_standard.npz), runs the unmodified `lib.parse_datasets.parse_datasets` on it with model="CRU" and model="LatentODE" -- the two
models whose loaders use `variable_time_collate_fn_CRU` / `variable_time_collate_fn_ODE` -- and records, as the other collate fixtures do,

  * the dataset's chunk list, flattened CSR style,
  * every batch dict the (unshuffled) val/test loaders produce, batch size 4          -> collate_cru.npz, collate_ode.npz

and, for the ODE form, hand-made batches passed straight to `variable_time_collate_fn_ODE` with the float32 `time_max` tensor that
parse_datasets passes (collate_ode_edge.npz): duplicated timestamps on both sides of `history`, one window, windows that share no
time, a window listed twice, every time on one side of `history` (a zero-length half), and four channels (a row of 16 bytes).

The fixtures hold tensors only.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_shims  # noqa: E402
from make_golden_collate import dump_chunks, ref_args, write_dataset  # noqa: E402

HISTORY, PRED_WINDOW = 24, 24

# name: (C, the windows' row times, the batch as indices into them)
EDGE = {
    # window 0 has two rows at 3.25 (history side), window 2 two rows at 24.0 (prediction side); 23.999 sits just below history
    "dups": (3, [[0.5, 3.25, 3.25, 10.0, 24.0, 30.5], [3.25, 7.0, 23.999, 25.0, 47.0], [0.5, 24.0, 24.0, 40.0]], [0, 1, 2]),
    "one_window": (3, [[1.0, 2.5, 23.0, 24.5, 40.0]], [0]),
    "disjoint": (3, [[0.25, 5.0, 30.0], [0.5, 6.0, 31.0, 32.0], [7.0, 33.0]], [0, 1, 2]),
    "twice": (3, [[0.5, 3.0, 25.0], [1.5, 3.0, 26.0, 27.0]], [0, 1, 0]),
    "all_pred": (3, [[24.0, 30.0], [25.0, 30.0, 41.5]], [0, 1]),
    "all_obs": (3, [[0.0, 3.0], [1.0, 3.0, 23.5]], [1, 0]),
    "four_channels": (4, [[0.5, 2.0, 9.0, 24.0, 30.5, 33.0], [2.0, 7.0, 23.0, 25.0, 47.0], [0.5, 24.0, 40.0, 40.0]], [2, 0, 1]),
}


def record_loaders(pdmod, root, model, name, emb_of):
    args = ref_args(root, model)
    res = pdmod.parse_datasets(args, show_summary=False)
    ds = res["ds"]
    out = {"history": np.float64(args.history), "pred_window": np.float64(args.pred_window)}
    for k, v in dump_chunks(ds.chunks, emb_of).items():
        out["chunks." + k] = v
    nb = 0
    for split in ("val_dataloader", "test_dataloader"):
        loader = res[split]
        idx = list(loader.dataset.indices)
        bs = args.batch_size
        for bi, batch in enumerate(loader):
            out[f"b{nb}.window_ids"] = np.array(idx[bi * bs:(bi + 1) * bs], dtype=np.int64)
            for k, v in batch.items():
                out[f"b{nb}.{k}"] = v.numpy()
            nb += 1
    out["n_batches"] = np.int64(nb)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "chunks", len(ds.chunks), "batches", nb, {k: tuple(v.shape) for k, v in batch.items()})


def record_edge(pdmod):
    args = argparse.Namespace(history=HISTORY, pred_window=PRED_WINDOW, device=torch.device("cpu"))
    tm = torch.tensor(HISTORY + PRED_WINDOW, dtype=torch.float32)       # what parse_datasets hands its collate
    g = torch.Generator().manual_seed(0)
    out = {"history": np.float64(HISTORY), "pred_window": np.float64(PRED_WINDOW), "names": np.array(list(EDGE))}
    for name, (C, times, ids) in EDGE.items():
        wins = []
        for ts in times:
            t = torch.tensor(ts, dtype=torch.float32)
            m = (torch.rand(len(ts), C, generator=g) < 0.7).float()
            wins.append((name, t, torch.randn(len(ts), C, generator=g) * m, m))
        batch = pdmod.variable_time_collate_fn_ODE([wins[i] for i in ids], args, tm)
        out[f"{name}.tt"] = np.concatenate([w[1].numpy() for w in wins])
        out[f"{name}.vals"] = np.concatenate([w[2].numpy() for w in wins])
        out[f"{name}.mask"] = np.concatenate([w[3].numpy() for w in wins])
        out[f"{name}.tt_off"] = np.cumsum([0] + [len(ts) for ts in times]).astype(np.int64)
        out[f"{name}.window_ids"] = np.array(ids, dtype=np.int64)
        for k, v in batch.items():
            out[f"{name}.out.{k}"] = v.numpy()
        print("edge", name, {k: tuple(v.shape) for k, v in batch.items()})
    np.savez_compressed(os.path.join(HERE, "collate_ode_edge.npz"), **out)


def main():
    _install_shims()
    import prettytable
    prettytable.PrettyTable = type("PrettyTable", (), {"__init__": lambda s, *a, **k: None, "add_row": lambda s, *a: None,
                                                       "__str__": lambda s: ""})
    import lib.parse_datasets as pdmod
    root = tempfile.mkdtemp(prefix="immtsf_syn_")
    files = write_dataset(root)
    emb_of = {k.split("/")[0]: v for k, v in files.items() if k.endswith("/emb")}
    record_loaders(pdmod, root, "CRU", "collate_cru", emb_of)
    record_loaders(pdmod, root, "LatentODE", "collate_ode", emb_of)
    record_edge(pdmod)


if __name__ == "__main__":
    main()
