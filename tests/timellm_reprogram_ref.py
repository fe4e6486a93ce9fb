"""float64 restatement of TimeLLM's prototype stage AS THE REFERENCE WRITES IT (models/TimeLLM.py:256-257 with the reprogramming
layer's two projections, :44-47): the mapping layer over the transposed word embeddings, then the key and the value projection of the
mapped table -- no fold -- and its analytic gradients for the six parameters.  numpy only; tests/test_timellm_reprogram_ref.py pins it to
the torch expressions (nn.Linear composition + autograd) and checks the folded formulas of csrc/timellm_reprogram.hip against it."""
import numpy as np

PARAMS = ("W_map", "b_map", "Wk", "bk", "Wv", "bv")


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


def mapped(E, W_map, b_map):
    """src = mapping_layer(E^T)^T: (S, d_llm)"""
    E, W_map, b_map = _f64(E, W_map, b_map)
    return W_map @ E + b_map[:, None]


def forward(E, W_map, b_map, Wk, bk, Wv, bv):
    """(k, v), each (S, D): key_projection(src), value_projection(src)"""
    Wk, bk, Wv, bv = _f64(Wk, bk, Wv, bv)
    src = mapped(E, W_map, b_map)
    return src @ Wk.T + bk, src @ Wv.T + bv


def backward(E, W_map, b_map, Wk, bk, Wv, bv, dk, dv):
    """the gradients of sum(k * dk) + sum(v * dv) for the six parameters, in PARAMS order, by the chain rule through src"""
    E, Wk, Wv, dk, dv = _f64(E, Wk, Wv, dk, dv)
    src = mapped(E, W_map, b_map)
    dsrc = dk @ Wk + dv @ Wv                      # (S, d_llm)
    return {"W_map": dsrc @ E.T, "b_map": dsrc.sum(1), "Wk": dk.T @ src, "bk": dk.sum(0), "Wv": dv.T @ src, "bv": dv.sum(0)}
