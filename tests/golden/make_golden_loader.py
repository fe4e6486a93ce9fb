#!/usr/bin/env python3
"""Golden vectors for the resident loaders (lib.parse_datasets on ResidentLoader) from the REAL reference data path.

Run on the CPU where the reference tree is at hand (IMMTSF_REFERENCE names it, as for make_golden.py):

    python tests/golden/make_golden_loader.py

Writes the seeded synthetic dataset of tests/loader_dataset.py to a temp dir and runs the unmodified `lib.parse_datasets.parse_datasets`
and `get_input_and_pred_len` on it, batch_size 4.  Recorded (tensors, lists and numbers only):

  loader_meta.npz      the chunk ids, the three index lists of both split methods, input_dim, time_max, the digest of the CSV bytes,
                       and the chunk ids of the unimodal run (enable_text=False)
  loader_<model>.npz   for DLinear / tPatchGNN / CRU / LatentODE: every tensor of the first and the last (partial) validation batch and of
                       the first training batch under torch.manual_seed(7), the window ids of each, get_input_and_pred_len's answer
                       under torch.manual_seed(5), and (tPatchGNN) the patch options parse_datasets wrote back
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_shims  # noqa: E402
from loader_dataset import MODELS, loader_args, write_dataset  # noqa: E402


def main():
    _install_shims()
    import prettytable
    prettytable.PrettyTable = type("PrettyTable", (), {"__init__": lambda s, *a, **k: None, "add_row": lambda s, *a: None,
                                                       "__str__": lambda s: ""})
    import lib.parse_datasets as pdmod
    root = tempfile.mkdtemp(prefix="immtsf_loader_")
    digest = write_dataset(root)
    cpu = torch.device("cpu")
    meta = {"csv_sha256": np.array(digest)}
    for method in ("sample", "instance"):
        res = pdmod.parse_datasets(loader_args(root, "DLinear", cpu, method), show_summary=False)
        meta["chunk_ids"] = np.array([c[0] for c in res["ds"].chunks])
        meta["input_dim"] = np.int64(res["input_dim"])
        meta["time_max"] = res["time_max"].numpy()
        for split in ("train", "val", "test"):
            dl = res[f"{split}_dataloader"]
            meta[f"{method}.{split}_idx"] = np.array([] if dl is None else list(dl.dataset.indices), dtype=np.int64)
    res = pdmod.parse_datasets(loader_args(root, "DLinear", cpu, enable_text=False), show_summary=False)
    meta["unimodal.chunk_ids"] = np.array([c[0] for c in res["ds"].chunks])
    batch = next(iter(res["val_dataloader"]))
    meta["unimodal.keys"] = np.array(sorted(batch))
    meta["unimodal.tau_shape"] = np.array(batch["tau"].shape, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "loader_meta.npz"), **meta)
    print("meta: chunks", len(meta["chunk_ids"]), {k: len(v) for k, v in meta.items() if k.endswith("_idx")},
          "unimodal chunks", len(meta["unimodal.chunk_ids"]))

    for model in MODELS:
        args = loader_args(root, model, cpu)
        res = pdmod.parse_datasets(args, show_summary=False)
        index_of = {c[0]: i for i, c in enumerate(res["ds"].chunks)}
        seen = []
        for split in ("train_dataloader", "val_dataloader"):
            dl = res[split]

            def spy(items, orig=dl.collate_fn):
                seen.append([index_of[it[0]] for it in items])
                return orig(items)
            dl.collate_fn = spy
        out = {}
        torch.manual_seed(5)
        out["input_and_pred_len"] = np.array(pdmod.get_input_and_pred_len(res), dtype=np.int64)
        if model == "tPatchGNN":
            out["patch"] = np.array([args.patch_size, args.npatch, args.patch_stride], dtype=np.int64)
        val = list(res["val_dataloader"])
        val_ids = seen[-len(val):]
        assert len(val) >= 2 and len(val_ids[-1]) < args.batch_size, "the last validation batch must be partial"
        torch.manual_seed(7)
        train0 = next(iter(res["train_dataloader"]))
        for name, batch, ids in (("val_first", val[0], val_ids[0]), ("val_last", val[-1], val_ids[-1]), ("train_first", train0, seen[-1])):
            out[f"{name}.window_ids"] = np.array(ids, dtype=np.int64)
            for k, v in batch.items():
                out[f"{name}.{k}"] = v.numpy()
        np.savez_compressed(os.path.join(HERE, f"loader_{model}.npz"), **out)
        print(model, out["input_and_pred_len"], {k: v.shape for k, v in out.items() if k.startswith("val_last.")})


if __name__ == "__main__":
    main()
