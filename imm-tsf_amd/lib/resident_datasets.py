"""`parse_datasets` / `get_input_and_pred_len` with the reference's names and results (lib/parse_datasets.py:479-512, 636-854), on
the resident store: the dataset is windowed once by `ResidentStore.from_dataset_dir`, lives in HBM, and the three loaders are
`immtsf.data.ResidentLoader`s that build every batch on the device -- the same dicts the reference's collate functions return, bit
for bit, plus the packed ragged note index.

How an unedited `main.py` reaches them: `lib.parse_datasets` remains the reference's module (its file, its dataset class, its collate
functions, `show_ds_summary`), and when it is imported with this tree in front, `install()` below replaces its two entry points with
the ones defined here (immtsf/dropin.py, overlay_module).  With no reference tree on the path `lib.parse_datasets` is this module.

What the resident path does not cover is handed to the reference's own two functions, and raises NotImplementedError when there are
none: raw-text mode (`enable_text and not use_text_embeddings`), an `args.device` that is not a GPU, and IMMTSF_RESIDENT_LOADER=0
(`immtsf.config.resident_loader`).
"""
import os
from collections import defaultdict

import torch

from immtsf import config

_ref_module = None      # the reference's lib.parse_datasets, once install() has met it
_ref_entry = {}         # its own parse_datasets / get_input_and_pred_len


def install(module):
    """make the reference's module `module` serve the resident entry points (its own are kept for what is handed back to them)"""
    global _ref_module
    _ref_module = module
    for name, fn in (("parse_datasets", parse_datasets), ("get_input_and_pred_len", get_input_and_pred_len)):
        _ref_entry[name] = getattr(module, name, None)
        setattr(module, name, fn)
    module.split_indices, module.ResidentDataset = split_indices, ResidentDataset


def _reference():
    """the reference's module of these entry points, or None when no reference tree is on the path"""
    return _ref_module


def _delegate(name, why):
    fn = _ref_entry.get(name)
    if fn is None:
        raise NotImplementedError(f"lib.parse_datasets.{name}: {why} is not built on the resident store, and no reference tree "
                                  f"is on sys.path to hand it to")
    return fn


def split_indices(chunk_ids, split_method):
    """-> (train_idx, val_idx, test_idx): positions into `chunk_ids` ("<record>_chunk<k>" strings), as the reference splits them
    (lib/parse_datasets.py:688-732).  "sample": 60/20/20 of each record's chunks in chunk order; "instance": whole records, 60/20/20
    of the sorted record ids by sklearn's train_test_split with random_state 42.  Host only."""
    if split_method == "instance":
        from sklearn.model_selection import train_test_split
        rec_of = [cid.rsplit("_chunk", 1)[0] for cid in chunk_ids]
        train_recs, test_recs = train_test_split(sorted(set(rec_of)), train_size=0.8, random_state=42, shuffle=True)
        train_recs, val_recs = train_test_split(train_recs, train_size=0.75, random_state=42, shuffle=False)
        pick = lambda recs: [i for i, r in enumerate(rec_of) if r in recs]      # noqa: E731
        return pick(train_recs), pick(val_recs), pick(test_recs)
    if split_method == "sample":
        grouped = defaultdict(list)
        for i, cid in enumerate(chunk_ids):
            rec_id, idx_str = cid.rsplit("_chunk", 1)
            grouped[rec_id].append((int(idx_str), i))
        train_idx, val_idx, test_idx = [], [], []
        for lst in grouped.values():
            lst.sort(key=lambda x: x[0])
            t_end, v_end = int(len(lst) * 0.6), int(len(lst) * 0.8)
            train_idx += [i for _, i in lst[:t_end]]
            val_idx += [i for _, i in lst[t_end:v_end]]
            test_idx += [i for _, i in lst[v_end:]]
        return train_idx, val_idx, test_idx
    raise ValueError(f"Unknown split_method: {split_method!r}")


class ResidentDataset:
    """`ds` of the returned dict: the store and its chunk ids, not a list of per-window tensors"""

    def __init__(self, store, chunk_ids):
        self.store, self.chunk_ids = store, list(chunk_ids)

    def __len__(self):
        return len(self.chunk_ids)


def _resident(args):
    return (config.resident_loader and torch.device(args.device).type == "cuda"
            and not (args.enable_text and not args.use_text_embeddings))


def parse_datasets(args, show_summary=True):
    if not _resident(args):
        why = ("IMMTSF_RESIDENT_LOADER=0" if not config.resident_loader else
               f"device {args.device}" if torch.device(args.device).type != "cuda" else "raw-text mode")
        return _delegate("parse_datasets", why)(args, show_summary)
    from immtsf.data import ResidentLoader, ResidentStore
    ref = _reference()
    # a relative data_root is relative to the tree that holds the data: the reference's, when this module stands in front of one
    here = os.path.dirname(ref.__file__ if ref is not None else __file__)
    base = args.data_root if os.path.isabs(args.data_root) else os.path.abspath(os.path.join(here, "..", args.data_root))
    dataset_path = os.path.join(base, args.dataset)
    print(f"Using dataset path: {dataset_path}")
    store, chunk_ids = ResidentStore.from_dataset_dir(
        dataset_path, args.history, args.pred_window, args.stride, args.device, time_unit=args.time_unit,
        llm_model_fusion=args.llm_model_fusion, llm_layers_fusion=args.llm_layers_fusion, max_length=args.max_length,
        rec_ids=getattr(args, "rec_ids", None), unit_scale=getattr(args, "unit_scale", None), normalize=True,
        enable_text=bool(args.enable_text), verbose=True)
    if show_summary and ref is not None:
        ref.show_ds_summary(args)
    ds = ResidentDataset(store, chunk_ids)
    train_idx, val_idx, test_idx = split_indices(chunk_ids, args.split_method)
    print(f"After chunking & splitting ({args.split_method}): train={len(train_idx)}, val={len(val_idx)}, test={len(test_idx)}")
    form, patch = "standard", None
    if args.model == "tPatchGNN":
        args.patch_size = args.patch_size or args.history // 5
        args.npatch = args.npatch or 5
        args.patch_stride = args.patch_stride or args.patch_size
        patch = (args.patch_size, args.npatch, args.patch_stride)
        print(f"Using Patch Collate Fn: patch_size={args.patch_size}, npatch={args.npatch}, patch_stride={args.patch_stride}")
    elif args.model == "CRU":
        form = "cru"
        print("Using CRU Specific Collate Fn")
    elif args.model == "LatentODE":
        form = "ode"
        print("Using ODE Specific Collate Fn")
    else:
        print("Using Standard Collate Fn")
    loader = lambda idx, shuffle: ResidentLoader(store, idx, args.batch_size, shuffle, form=form, patch=patch)      # noqa: E731
    return {
        "train_dataloader": loader(train_idx, True),
        "val_dataloader": loader(val_idx, False),
        "test_dataloader": loader(test_idx, False) if test_idx else None,
        "input_dim": store.C,
        "time_max": torch.tensor(args.history + args.pred_window, dtype=torch.float32, device=args.device),
        "ds": ds,
    }


def get_input_and_pred_len(data_obj):
    """(largest observed_data.shape[1], largest data_to_predict.shape[1]) over one epoch of every split, as the reference finds by
    building every batch (lib/parse_datasets.py:479-512) -- here from the store's host metadata, without a batch: the longest history /
    prediction slice of the split's windows; for tPatchGNN's form axis 1 of observed_data is the patch axis, so npatch; for LatentODE's
    it is the number of distinct history times of a BATCH, so each split's batches are formed on the host (the train split in the
    order its next epoch would have, drawing from the RNG what the reference's scan draws)."""
    from immtsf.data import ResidentLoader
    splits = [("train", data_obj["train_dataloader"]), ("val", data_obj["val_dataloader"])]
    if data_obj.get("test_dataloader") is not None:
        splits.append(("test", data_obj["test_dataloader"]))
    if not all(isinstance(dl, ResidentLoader) for _, dl in splits):
        return _delegate("get_input_and_pred_len", "a loader that is not a ResidentLoader")(data_obj)
    max_input_len, max_pred_len = 0, 0
    for name, dl in splits:
        print(f"Scanning {name} split ({len(dl)} batches)...")
        st, ids = dl.store, dl.window_ids[dl._epoch_order()]
        if not len(ids):
            continue
        if dl.form == "ode":
            for k in range(0, len(ids), dl.batch_size):
                axis, n_obs = st._union_axis(ids[k:k + dl.batch_size])
                max_input_len, max_pred_len = max(max_input_len, n_obs), max(max_pred_len, len(axis) - n_obs)
            continue
        max_input_len = max(max_input_len, dl.patch[1] if dl.patch is not None else int(st.hist_len[ids].max()))
        max_pred_len = max(max_pred_len, int(st.pred_len[ids].max()))
    return max_input_len, max_pred_len

