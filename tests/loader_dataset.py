"""The seeded synthetic dataset of the loader tests, in the reference's on-disk layout (processed/<entity>/time_series.csv +
text_embeddings_model=TOY16_layers=full_maxlen=1024.pt + text.csv).  tests/golden/make_golden_loader.py writes it for the reference's
`parse_datasets`, tests/test_gpu_loader.py writes the identical files again for this build's (the CSV bytes are pinned by a digest in the
fixture).

6 entities, C = 3, d_m = 16, hours as the unit, history = pred_window = stride = 24.  An entity observed over D days yields D - 2
windows.  Built in on purpose:
  * ent05 spans 3 days: ONE window, so its sample split has int(1 * 0.6) == int(1 * 0.8) == 0 -- no train and no validation window;
  * ent00's window 3 holds exactly one note (it is ent00's validation window);
  * ent01's window 2 holds exactly one history row (it is ent01's validation window);
  * ent02's window 5 holds no note: it is dropped and still uses up a chunk number.
"""
import argparse
import hashlib
import os

import numpy as np
import pandas as pd
import torch

DAYS = [7, 6, 12, 12, 8, 3]
C, D_M = 3, 16
HISTORY = PRED_WINDOW = STRIDE = 24
MODELS = ("DLinear", "tPatchGNN", "CRU", "LatentODE")
EMB_NAME = "text_embeddings_model=TOY16_layers=full_maxlen=1024.pt"
NINE = ["ent00", "ent01"]       # the entities whose 5 + 4 windows make the 9-window store of the kernel tests


def write_dataset(root, seed=23):
    """-> sha256 over the time_series.csv bytes of all entities"""
    rng = np.random.default_rng(seed)
    digest = hashlib.sha256()
    t0 = pd.Timestamp("2022-05-01 00:00:00")
    for e, days in enumerate(DAYS):
        ent = f"ent{e:02d}"
        d = os.path.join(root, "SYN", "processed", ent)
        os.makedirs(d)
        grid = np.arange(0, days * 86400, 600)
        secs = np.sort(rng.choice(grid[1:-1], size=12 * days, replace=False))
        secs = np.concatenate([[0], secs, [days * 86400 - 600]])       # the span is fixed: D - 2 windows
        if e == 1:          # one history row in window 2: nothing in [48 h, 72 h) but one observation at 50 h
            secs = np.concatenate([secs[(secs < 48 * 3600) | (secs >= 72 * 3600)], [50 * 3600]])
            secs = np.sort(secs)
        n = len(secs)
        vals = rng.normal(size=(n, C)) * (1 + 0.5 * e) + e
        vals[rng.random((n, C)) < 0.3] = np.nan
        vals[0, :] = rng.normal(size=C)
        if e == 1:
            vals[secs == 50 * 3600, :] = rng.normal(size=C)     # ... and it is observed
        df = pd.DataFrame({"date_time": [str(t0 + pd.Timedelta(seconds=int(s))) for s in secs], "record_id": ent})
        for c in range(C):
            df[f"f{c}"] = vals[:, c]
        ts_path = os.path.join(d, "time_series.csv")
        df.to_csv(ts_path, index=False)
        digest.update(open(ts_path, "rb").read())
        rel = np.sort(rng.random(5 * days) * days * 24)
        if e == 0:          # one note in window 3
            rel = np.sort(np.concatenate([rel[(rel < 72) | (rel >= 96)], [80.25]]))
        if e == 2:          # no note in window 5
            rel = rel[(rel < 120) | (rel >= 144)]
        rel = rel.astype(np.float32)
        emb = rng.normal(size=(len(rel), D_M)).astype(np.float32)
        torch.save({"embeddings": torch.from_numpy(emb), "rel_times": torch.from_numpy(rel)}, os.path.join(d, EMB_NAME))
        # the same notes as raw text (what enable_text=False windows by), at whole seconds
        when = [str(t0 + pd.Timedelta(seconds=int(round(float(r) * 3600)))) for r in rel]
        pd.DataFrame({"date_time": when, "record_id": ent, "text": [f"note {i}" for i in range(len(rel))]}).to_csv(
            os.path.join(d, "text.csv"), index=False)
    return digest.hexdigest()


def loader_args(root, model, device, split_method="sample", enable_text=True):
    """the namespace parse_datasets reads; tPatchGNN's patch options are left unset so that the defaults are written back"""
    return argparse.Namespace(
        data_root=root, dataset="SYN", device=device, history=HISTORY, pred_window=PRED_WINDOW, stride=STRIDE, time_unit="hours",
        enable_text=enable_text, use_text_embeddings=True, llm_model_fusion="TOY16", llm_layers_fusion=None, max_length=1024,
        split_method=split_method, model=model, batch_size=4, patch_size=None, npatch=None, patch_stride=None, rec_ids=None)
