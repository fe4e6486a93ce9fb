#!/usr/bin/env python3
"""Reference values of `lib.evaluation.evaluation()` (reference lib/evaluation.py:192-283) for stored predictions.

Run in the build container only (needs the reference checkout that make_golden.py points at):

    cd /tmp && python <repo>/tests/golden/make_golden_eval.py

Three batches with C = 7 and (B, Lp) = (8, 12), (5, 30), (3, 1): truths of both signs (z-scored data), about 10 % of them exactly 0,
a 0/1 mask that leaves variable 3 out in every batch, predictions = truth + noise.  The reference's own evaluation() is driven with
a stub model whose `forecasting` hands back the stored prediction (fusion=None, enable_text=False) on the CPU in fp32; recorded are
the inputs and the five floats it returns.  Tensors and numbers only -- no reference source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _install_shims  # noqa: E402

SHAPES = ((8, 12), (5, 30), (3, 1))
C = 7
MASKED_VAR = 3


def make_batches(seed=2030):      # a seed whose data gives a NEGATIVE MAPE (the divisor is signed: routine on z-scored data)
    rng = np.random.default_rng(seed)
    out = []
    for B, Lp in SHAPES:
        truth = rng.normal(size=(B, Lp, C)).astype(np.float32)
        truth[rng.random((B, Lp, C)) < 0.10] = 0.0
        mask = (rng.random((B, Lp, C)) < 0.7).astype(np.float32)
        mask[..., MASKED_VAR] = 0.0
        pred = (truth + 0.3 * rng.normal(size=(B, Lp, C))).astype(np.float32)
        out.append((truth, mask, pred))
    return out


class _Stub:
    """model.forecasting(...) -> the stored prediction of the batch under evaluation"""

    def __init__(self, preds):
        self.preds, self.i = preds, 0

    def forecasting(self, tp, x, t, m):
        p = self.preds[self.i]
        self.i += 1
        return p


def main():
    _install_shims()
    import lib.evaluation as ref_eval
    batches = make_batches()
    loader = [{"tp_to_predict": torch.zeros(t.shape[0], t.shape[1]), "observed_data": None, "observed_tp": None, "observed_mask": None,
               "data_to_predict": torch.from_numpy(t), "mask_predicted_data": torch.from_numpy(m)} for t, m, _ in batches]
    res = ref_eval.evaluation(_Stub([torch.from_numpy(p) for _, _, p in batches]), None, loader, enable_text=False)
    arrays = {}
    for i, (t, m, p) in enumerate(batches):
        arrays[f"data_to_predict_{i}"], arrays[f"mask_predicted_data_{i}"], arrays[f"pred_{i}"] = t, m, p
    for k in ("loss", "mse", "mae", "rmse", "mape"):
        arrays[f"ref_{k}"] = np.float64(res[k])
    arrays["masked_var"] = np.int64(MASKED_VAR)
    np.savez(os.path.join(HERE, "eval_metrics.npz"), **arrays)
    print({k: res[k] for k in ("loss", "mse", "mae", "rmse", "mape")})


if __name__ == "__main__":
    main()
