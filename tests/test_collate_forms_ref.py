"""The numpy restatement of the reference's CRU and LatentODE collates (tests/collate_forms_ref.py) against what the REAL reference
produced (tests/golden/collate_{cru,ode,ode_edge}.npz): every tensor equal in shape, dtype and bits."""
import os

import numpy as np
import pytest

import collate_forms_ref as F
from oracle import collate_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ["data_to_predict", "mask_predicted_data", "observed_data", "observed_mask", "observed_tp", "tp_to_predict"]


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    zs = np.load(os.path.join(GOLDEN, "collate_standard.npz"))
    emb = {int(k[8:10]): zs[k] for k in zs.files if k.startswith("file.ent") and k.endswith("/emb")}
    chunks = []
    for c in R.chunks_from_golden(z):
        ne = np.stack([emb[int(e)][int(r)] for e, r in zip(c["note_ent"], c["note_row"])]) if len(c["note_row"]) \
            else np.zeros((0, 16), np.float32)
        chunks.append((c["tt"], c["vals"], c["mask"], c["note_t"], ne))
    return z, chunks


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["collate_cru", "collate_ode"])
def test_restatement_matches_reference_loaders(name):
    z, chunks = load(name)
    hist, tmax = float(z["history"]), float(z["history"] + z["pred_window"])
    assert int(z["n_batches"]) >= 4
    for b in range(int(z["n_batches"])):
        sel = [chunks[i] for i in z[f"b{b}.window_ids"]]
        got = F.cru_collate(sel, hist) if name == "collate_cru" else F.ode_collate(sel, hist, tmax)
        got.update({k: v for k, v in R.notes_collate(sel).items() if k in ("tau", "notes_embeddings")})
        keys = [k[len(f"b{b}."):] for k in z.files if k.startswith(f"b{b}.") and not k.endswith("window_ids")]
        assert sorted(keys) == sorted(got.keys())
        for k in keys:
            assert same(got[k], z[f"b{b}.{k}"]), (name, b, k)


def test_fixtures_hold_what_they_are_for():
    """ragged lengths and raw times in the CRU batches; a shared axis longer than any window in the ODE batches"""
    z, chunks = load("collate_cru")
    assert max(float(z[f"b{b}.tp_to_predict"].max()) for b in range(int(z["n_batches"]))) > 1.0      # not normalised
    z, chunks = load("collate_ode")
    for b in range(int(z["n_batches"])):
        ids = z[f"b{b}.window_ids"]
        T = z[f"b{b}.observed_tp"].shape[0] + z[f"b{b}.tp_to_predict"].shape[0]
        assert z[f"b{b}.observed_tp"].ndim == 1 and T >= max(len(chunks[i][0]) for i in ids)
        if len(ids) > 1:
            assert T > max(len(chunks[i][0]) for i in ids)
        tp = np.concatenate([z[f"b{b}.observed_tp"], z[f"b{b}.tp_to_predict"]])
        assert np.all(np.diff(tp) > 0)


def test_restatement_matches_reference_on_edge_batches():
    z = np.load(os.path.join(GOLDEN, "collate_ode_edge.npz"))
    hist, tmax = float(z["history"]), float(z["history"] + z["pred_window"])
    cases = F.edge_cases(z)
    assert {"dups", "one_window", "disjoint", "twice", "all_pred", "all_obs", "four_channels"} <= set(cases)
    for name, (chunks, ids, want) in cases.items():
        got = F.ode_collate([chunks[i] for i in ids], hist, tmax)
        assert sorted(got) == sorted(want) == SIX
        for k in SIX:
            assert same(got[k], want[k]), (name, k)
    # the cases are what their names say
    chunks, ids, want = cases["dups"]
    assert any(np.any(np.diff(c[0][c[0] < hist]) == 0) for c in chunks) and any(np.any(np.diff(c[0][c[0] >= hist]) == 0) for c in chunks)
    assert len(cases["one_window"][1]) == 1
    chunks, ids, want = cases["disjoint"]
    assert want["observed_tp"].shape[0] + want["tp_to_predict"].shape[0] == sum(len(chunks[i][0]) for i in ids)
    chunks, ids, want = cases["twice"]
    assert len(ids) > len(set(ids))
    first, again = [b for b, i in enumerate(ids) if i == ids[0]][:2]
    assert np.array_equal(want["observed_data"][first], want["observed_data"][again])
    assert cases["all_pred"][2]["observed_tp"].shape == (0,) and cases["all_obs"][2]["tp_to_predict"].shape == (0,)
