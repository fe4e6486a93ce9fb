"""Cases for TimeLLM's folded prototype operator (immtsf.ops.timellm_prototypes, csrc/timellm_reprogram.hip): seeded fp32 inputs, and
for each case the float64 restatement's outputs and gradients (tests/timellm_reprogram_ref.py), computed once and shared.

Shapes (S, V, d_llm, H, d_keys), D = H d_keys: a single row and a single vocabulary entry; S below, off and across the 64-row tile;
V below one split of the reduction, prime, and spanning several splits; the smallest (16) and the largest (128) 2 D; d_llm off the 16 and
the 128 column tiles.  b_map and the projection biases are non-zero, so the b_map (x) rowsum term and its gradient are exercised."""
import functools

import numpy as np

import timellm_reprogram_ref as R

SHAPES = [(1, 1, 8, 1, 8), (20, 320, 128, 2, 8), (70, 1031, 64, 8, 2), (130, 5003, 72, 4, 8), (65, 2500, 128, 8, 8)]
IDS = ["S%d-V%d-d%d-H%d-dk%d" % s for s in SHAPES]
NAMES = ("E",) + R.PARAMS + ("dk", "dv")


@functools.lru_cache(maxsize=None)
def inputs(i):
    """fp32 arrays by name: E, the six parameters, and the upstream gradients dk, dv"""
    S, V, d, H, dkeys = SHAPES[i]
    D = H * dkeys
    g = np.random.default_rng(4100 + i)
    n = lambda *s: g.standard_normal(s)      # noqa: E731
    t = {"E": 0.5 * n(V, d), "W_map": n(S, V) / np.sqrt(V), "b_map": 0.5 * n(S), "Wk": n(D, d) / np.sqrt(d), "bk": 0.5 * n(D),
         "Wv": n(D, d) / np.sqrt(d), "bv": 0.5 * n(D), "dk": n(S, D), "dv": n(S, D)}
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in t.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(i):
    """float64, as the reference writes the stage: {"k", "v", and the six gradients by parameter name}; shared, read-only"""
    t = inputs(i)
    k, v = R.forward(*[t[n] for n in ("E",) + R.PARAMS])
    out = {"k": k, "v": v, **R.backward(*[t[n] for n in NAMES])}
    for a in out.values():
        a.setflags(write=False)
    return out
