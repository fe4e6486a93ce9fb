"""CPU restatement (numpy) of the reference's CRU and LatentODE collates -- TEST INFRASTRUCTURE ONLY (the oracle for
`ResidentStore.collate(form="cru" | "ode")`, SURVEY 8f row 1, and the host baseline of tools/collate_bench.py).

Pinned by tests/test_collate_forms_ref.py against tests/golden/collate_{cru,ode,ode_edge}.npz, which hold what the real reference
produced (tests/golden/make_golden_collate_forms.py).

Follows, by behaviour:
  * lib/parse_datasets.py:369-408  variable_time_collate_fn_CRU (the standard split and zero padding, times left as stored)
  * lib/parse_datasets.py:411-471  variable_time_collate_fn_ODE (one sorted distinct time axis per batch, values and masks scattered
                                   onto a (B, T, C) grid, times normalised and then jittered by j * eps, split at `history`)
  * lib/utils.py:335-347           normalize_masked_tp

A `chunk` is what oracle/collate_ref.py takes: (tt [L] f32 non-decreasing chunk-relative times, vals [L,C] f32, mask [L,C] f32, ...);
only the first three entries are read here.
"""
import numpy as np

from oracle.collate_ref import normalize_tp, series_collate


def cru_collate(chunks, history):
    """the standard collate with the times left raw.  series_collate divides by its scale in fp32; at time_max = 1 the scale is 1
    and t / 1 is t, so the standard restatement is reused instead of being copied"""
    return series_collate([tuple(c[:3]) + (None, None) for c in chunks], history, 1.0)


def union_axis(chunks, history):
    """-> (the sorted distinct fp32 times over all rows of the batch, how many of them lie below float32(history))"""
    axis = np.unique(np.concatenate([np.asarray(c[0], dtype=np.float32) for c in chunks]))
    return axis, int((axis < np.float32(history)).sum())


def ode_collate(chunks, history, time_max):
    """LatentODE's collate.  Time j is fl(fl(u_j / scale) + fl(float(j) * eps)) with eps = fl(finfo(float32).eps * time_max): torch
    rounds each operation to fp32, and so does numpy on float32 arrays.  A window's rows are written in order, so of several rows
    with one timestamp the last stays (what index_put does on the CPU); a window listed twice gives two equal grid rows."""
    axis, n_obs = union_axis(chunks, history)
    B, T, C = len(chunks), len(axis), chunks[0][1].shape[1]
    vals = np.zeros((B, T, C), dtype=np.float32)
    mask = np.zeros((B, T, C), dtype=np.float32)
    for b, c in enumerate(chunks):
        idx = np.searchsorted(axis, np.asarray(c[0], dtype=np.float32))
        for r, j in enumerate(idx):
            vals[b, j] = c[1][r]
            mask[b, j] = c[2][r]
    eps = np.float32(np.finfo(np.float32).eps) * np.float32(time_max)
    jitter = (np.arange(T).astype(np.float32) * eps).astype(np.float32)
    tp = (normalize_tp(axis, time_max) + jitter).astype(np.float32)
    return {
        "observed_tp": tp[:n_obs],
        "observed_data": vals[:, :n_obs],
        "observed_mask": mask[:, :n_obs],
        "tp_to_predict": tp[n_obs:],
        "data_to_predict": vals[:, n_obs:],
        "mask_predicted_data": mask[:, n_obs:],
    }


def edge_cases(z):
    """the hand-made batches of collate_ode_edge.npz: name -> (chunks [(tt, vals, mask)], window ids, the reference's six tensors)"""
    out = {}
    for name in [str(n) for n in z["names"]]:
        off = z[f"{name}.tt_off"]
        chunks = [(z[f"{name}.tt"][a:b], z[f"{name}.vals"][a:b], z[f"{name}.mask"][a:b]) for a, b in zip(off[:-1], off[1:])]
        want = {k[len(name) + 5:]: z[k] for k in z.files if k.startswith(name + ".out.")}
        out[name] = (chunks, [int(i) for i in z[f"{name}.window_ids"]], want)
    return out
