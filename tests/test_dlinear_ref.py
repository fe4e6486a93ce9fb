"""CPU checks of the fused DLinear path's yardstick and limits: the float64 restatement (tests/dlinear_ref.py) against the real
reference's goldens -- shared weights (model_dlinear.npz) and one set per channel (model_dlinear_individual.npz, written by
tests/golden/make_golden_dlinear.py) -- outputs to 1e-6, every gradient to 1e-5 of the largest gradient; and the library's limit and
workspace queries, which are host arithmetic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dlinear_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name,individual", [("model_dlinear", False), ("model_dlinear_individual", True)])
def test_restatement_matches_reference_golden(name, individual):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    C, S, P, k = 3, 8, 6, 5
    par = R.golden_params(z, individual, C)
    Lp = z["tpp"].shape[1]
    y = R.forward(z["data"], z["mask"], z["tp"], Lp, k, *par["p."])
    assert y.shape == z["out"].shape
    assert np.abs(y - z["out"]).max() < 1e-6
    dWs, dWt, dWu, db = R.backward(z["data"], z["mask"], z["tp"], k, S, P, z["upstream"], individual)
    want = par["g."]
    gmax = max(np.abs(g).max() for g in want)
    for got, ref in zip((dWs, dWt, dWu, db, db, db), want):
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() < 1e-5 * gmax
    if individual:      # the fixture's channels do differ, so a kernel that shared one set would not pass it
        assert np.abs(par["p."][0][0] - par["p."][0][1]).max() > 1e-2


def test_restatement_edges():
    """what the formulas say at the corners the kernels must get right: a column without observations (mean 0, std sqrt(1e-5), xn = 0),
    masked / padded positions holding -mean / std, and k = 1 (trend = xn, seasonal = 0)"""
    data = np.array([[[2.0, 5.0], [4.0, 7.0]]])      # (1, 2, 2)
    mask = np.array([[[1.0, 0.0], [1.0, 0.0]]])
    seas, trend, t, mean, std = R.stage(data, mask, np.array([[0.25, 0.5]]), 4, 1)
    assert mean.tolist() == [[3.0, 0.0]]
    np.testing.assert_allclose(std, [[np.sqrt(1.0 + 1e-5), np.sqrt(1e-5)]])
    np.testing.assert_allclose(trend[0, 0], np.array([-1.0, 1.0, -3.0, -3.0]) / std[0, 0])      # padding holds -mean / std
    assert not seas.any() and not trend[0, 1].any()
    assert t.tolist() == [[0.25, 0.5, 0.0, 0.0]]
    # k wider than the series: every window is the clamped ends plus the whole series
    _, trend9, _, _, _ = R.stage(data, mask, np.array([[0.25, 0.5]]), 4, 9)
    xn = trend[0, 0]
    want = [(xn.sum() + (4 - l) * xn[0] + (l + 1) * xn[3]) / 9 for l in range(4)]
    np.testing.assert_allclose(trend9[0, 0], want)


def test_supported_and_workspace_queries_run_without_gpu():
    from immtsf import _lib
    lib = _lib.load()
    sup = lib.immtsf_dlinear_supported
    for ind in (0, 1):
        assert sup(24, 24, 5, 25, ind) == 1            # cfg1: the window is wider than the series
        assert sup(128, 128, 8, 25, ind) == 1 and sup(1, 1, 1, 1, ind) == 1 and sup(8, 6, 1000, 1001, ind) == 1
        assert sup(129, 24, 5, 25, ind) == 0 and sup(24, 129, 5, 25, ind) == 0
        assert sup(24, 24, 5, 4, ind) == 0 and sup(24, 24, 5, 0, ind) == 0      # even / empty windows: the composed path's error
        assert sup(0, 24, 5, 25, ind) == 0 and sup(24, 0, 5, 25, ind) == 0 and sup(24, 24, 0, 25, ind) == 0
    ws = lib.immtsf_dlinear_workspace_bytes
    nv = (3 * 24 * 24 + 24) * 4
    assert ws(4, 24, 24, 5, 0) == 3 * nv + 256         # 20 rows in shares of at least 8: three slabs
    assert ws(4096, 24, 24, 5, 0) == 256 * nv + 256    # never more slabs than 256
    assert ws(16, 128, 128, 8, 1) == 8 * 2 * (3 * 128 * 128 + 128) * 4 + 256      # per channel: 16 windows, two slabs
    assert ws(4, 129, 24, 5, 0) == 0 and ws(0, 24, 24, 5, 0) == 0
    # the sizes grow with the batch up to the slab cap and never shrink
    sizes = [ws(b, 32, 32, 8, 0) for b in (1, 2, 16, 130, 5000)]
    assert sizes == sorted(sizes) and sizes[0] > 0
