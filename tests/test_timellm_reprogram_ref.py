"""CPU checks behind tests/test_gpu_timellm_reprogram.py: the float64 restatement of TimeLLM's prototype stage
(tests/timellm_reprogram_ref.py) equals the torch expressions -- nn.Linear composition as models/TimeLLM.py and its ReprogrammingLayer
write it, gradients by autograd -- and the FOLDED formulas csrc/timellm_reprogram.hip implements equal the restatement, outputs and all
six gradients, the gradient through r = rowsum([Wk; Wv]) included.  Both in float64 to 1e-10 of each tensor's largest element."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timellm_reprogram_cases as K  # noqa: E402
import timellm_reprogram_ref as R  # noqa: E402


def _close(got, want, bar=1e-10):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return np.abs(got - want).max() <= bar * max(np.abs(want).max(), 1e-300)


def folded(t):
    """the fold in float64 numpy: {"k", "v", six gradients}.  P = E [Wk^T | Wv^T]; [k|v] = W_map P + b_map (x) r + [bk|bv];
    G = [dk|dv]: dW_map = G P^T, db_map = G r, d[bk|bv] = colsum(G), dP = W_map^T G, d[Wk; Wv] = dP^T E + colsum(G * b_map[:, None]) 1^T"""
    f = {k: np.asarray(v, np.float64) for k, v in t.items()}
    D = f["Wk"].shape[0]
    Wkv = np.concatenate([f["Wk"], f["Wv"]], 0)               # (2 D, d_llm)
    P = f["E"] @ Wkv.T                                        # (V, 2 D)
    r = Wkv.sum(1)
    kv = f["W_map"] @ P + np.outer(f["b_map"], r) + np.concatenate([f["bk"], f["bv"]])
    G = np.concatenate([f["dk"], f["dv"]], 1)                 # (S, 2 D)
    dP = f["W_map"].T @ G
    dWkv = dP.T @ f["E"] + (G * f["b_map"][:, None]).sum(0)[:, None]
    dbkv = G.sum(0)
    return {"k": kv[:, :D], "v": kv[:, D:], "W_map": G @ P.T, "b_map": G @ r, "Wk": dWkv[:D], "Wv": dWkv[D:], "bk": dbkv[:D], "bv": dbkv[D:]}


@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=K.IDS)
def test_restatement_equals_the_torch_expressions(i):
    t = K.inputs(i)
    S, V, d, H, dkeys = K.SHAPES[i]
    D = H * dkeys
    mapping, key, value = torch.nn.Linear(V, S).double(), torch.nn.Linear(d, D).double(), torch.nn.Linear(d, D).double()
    with torch.no_grad():
        for lin, w, b in ((mapping, "W_map", "b_map"), (key, "Wk", "bk"), (value, "Wv", "bv")):
            lin.weight.copy_(torch.tensor(t[w]).double())
            lin.bias.copy_(torch.tensor(t[b]).double())
    E = torch.tensor(t["E"]).double()
    src = mapping(E.permute(1, 0)).permute(1, 0)              # models/TimeLLM.py forecasting(), reference :256
    k, v = key(src), value(src)                               # ReprogrammingLayer.forward, reference :45-46
    ((k * torch.tensor(t["dk"]).double()).sum() + (v * torch.tensor(t["dv"]).double()).sum()).backward()
    ref = K.reference(i)
    assert _close(ref["k"], k.detach().numpy()) and _close(ref["v"], v.detach().numpy())
    for name, p in (("W_map", mapping.weight), ("b_map", mapping.bias), ("Wk", key.weight), ("bk", key.bias), ("Wv", value.weight),
                    ("bv", value.bias)):
        assert _close(ref[name], p.grad.numpy()), name


@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=K.IDS)
def test_folded_formulas_equal_the_restatement(i):
    got, ref = folded(K.inputs(i)), K.reference(i)
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert _close(got[name], ref[name]), name


def test_cases_exercise_the_r_term():
    """every case has non-zero b_map and biases, and the gradient through r is a visible part of d[Wk; Wv]"""
    for i in range(len(K.SHAPES)):
        t = K.inputs(i)
        assert all(np.abs(t[n]).min() > 0 for n in ("b_map", "bk", "bv"))
        term = (np.concatenate([t["dk"], t["dv"]], 1).astype(np.float64) * t["b_map"].astype(np.float64)[:, None]).sum(0)
        ref = K.reference(i)
        assert np.abs(term).max() > 1e-3 * max(np.abs(ref["Wk"]).max(), np.abs(ref["Wv"]).max())
    assert R.PARAMS == ("W_map", "b_map", "Wk", "bk", "Wv", "bv")
