"""tests/timesnet_spectrum_ref.py (the float64 reference the GPU tests of immtsf.ops.timesnet_spectrum compare with) pinned on the CPU:
(a) against torch.fft.rfft in float64 + autograd through the formula of models/TimesNet.py fft_for_period_device followed by softmax and
the padded transpose, (b) against timesnet_periods_ref.spectrum_topk for the selection, (c) against period_rows_ref for the periods and
row counts, (d) the separation that keeps fp32 round-off from being able to change a selection: on every case of the table the weakest
selected mean amplitude is at least twice the strongest unselected one (the condition test_timesnet_periods_ref.py states), and
consecutive selected ones differ by 5 % at least (round-off is 1e-5 of the strongest line at most), so the ORDER is safe too.  A
selection mismatch on the GPU is then a bug."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timesnet_periods_ref as P  # noqa: E402
import timesnet_spectrum_ref as S  # noqa: E402

ALL = sorted(S.CASES) + [S.PAST[0]]


def _rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def _dims(name):
    return S.PAST[1] if name == S.PAST[0] else S.CASES[name]


def test_case_table_is_the_issue_s():
    assert [S.CASES[n][:4] for n in ("a", "c", "one", "odd", "cfg4", "wide")] == [(3, 30, 8, 5), (2, 66, 8, 4), (1, 7, 1, 1), (5, 33, 3, 2),
                                                                               (2, 64, 16, 5), (2, 192, 64, 5)]
    for name in ALL:      # a Nyquist line wherever T is even and more than one line is planted
        B, T, N, k, freqs, amps, seed = _dims(name)
        assert T % 2 == 1 or k == 1 or T // 2 in freqs, name
        assert S.case_input(name).shape == (B, T, N) and S.case_input(name).dtype == torch.float32


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_a_values_and_gradient_vs_rfft_autograd(name, scaled):
    """scaled: x times 4 / T -- amplitudes of order one, so the softmax is not saturated and the gradient through w is not negligible"""
    from models.TimesNet import fft_for_period_device
    B, T, N, k, freqs, amps, seed = _dims(name)
    x = S.case_input(name).double() * (4.0 / T if scaled else 1.0)
    r = S.spectrum_ref(x, k)
    g = torch.Generator().manual_seed(seed + 100)
    g_w = torch.randn(B, k, generator=g, dtype=torch.float64)
    g_xl = torch.randn(2 * T * B, N, generator=g, dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    top, weight = fft_for_period_device(xa, k)
    w = F.softmax(weight, dim=1)
    xl = F.pad(xa.transpose(0, 1), (0, 0, 0, 0, 0, T)).reshape(2 * T * B, N)
    amp = torch.fft.rfft(x, dim=1).abs()
    assert top.tolist() == r["top"]
    assert _rel(r["amp"], amp) <= 1e-12
    assert _rel(r["amp_mean"], amp.mean(-1)) <= 1e-12
    assert _rel(r["freq"][1:], amp.mean(0).mean(-1)[1:]) <= 1e-12 and float(r["freq"][0]) == 0.0
    assert _rel(r["weight"], weight.detach()) <= 1e-12
    assert _rel(r["w"], w.detach()) <= 1e-12
    assert torch.equal(r["xl"], xl.detach())
    for gw, gx in ((g_w, g_xl), (g_w, None), (None, g_xl)):
        xa.grad = None
        loss = (w * gw).sum() if gw is not None else 0.0
        loss = loss + ((xl * gx).sum() if gx is not None else 0.0)
        loss.backward(retain_graph=True)
        want = xa.grad
        got = S.spectrum_grad_ref(x, k, gw, gx)
        if float(want.abs().max()) == 0.0:      # (k == 1: w is the constant 1)
            assert float(got.abs().max()) <= 1e-15
        else:
            assert _rel(got, want) <= 1e-12, (gw is not None, gx is not None)
        if gw is None:
            assert torch.equal(got, gx.reshape(2 * T, B, N)[:T].transpose(0, 1))


@pytest.mark.parametrize("name", ALL)
def test_b_c_selection_periods_rows(name):
    B, T, N, k, freqs, amps, seed = _dims(name)
    x = S.case_input(name)
    r = S.case_reference(name)
    top, freq, weight = P.spectrum_topk(x, k)
    assert r["top"] == top.tolist() == list(freqs)
    assert _rel(r["freq"], freq) <= 1e-12 and _rel(r["weight"], weight) <= 1e-12
    assert all(f >= 1 for f in r["top"])
    period, rows = P.period_rows_ref(r["top"], T, B)
    assert r["period"].dtype == np.int32 and r["rows"].dtype == np.int32
    assert np.array_equal(r["period"], period) and np.array_equal(r["rows"], rows)
    assert r["period"].tolist() == [T // f for f in freqs]


@pytest.mark.parametrize("name", ALL)
def test_d_selected_lines_are_separated(name):
    k = _dims(name)[3]
    r = S.case_reference(name)
    freq, top = r["freq"], r["top"]
    rest = freq.clone()
    rest[top] = 0
    assert float(freq[top[-1]]) >= 2.0 * float(rest.max()), (float(freq[top[-1]]), float(rest.max()))
    sel = freq[top]
    assert bool((sel[:-1] >= 1.05 * sel[1:]).all()), sel.tolist()
    assert len(top) == k


def test_equal_values_go_to_the_lower_index_and_zero_series():
    assert S.topk_low_index(torch.tensor([0.0, 1.0, 1.0, 2.0, 1.0]), 3) == [3, 1, 2]
    # the unit impulse: every amplitude is exactly 1, the constant term is zeroed -> 1..k, weights 1, w = 1 / k
    x = torch.zeros(2, 16, 3, dtype=torch.float64)
    x[:, 0] = 1.0
    r = S.spectrum_ref(x, 4)
    assert r["top"] == [1, 2, 3, 4] and bool((r["weight"] == 1.0).all()) and bool((r["w"] == 0.25).all())
    # the zero series: f = 0 leads the ties, its period is T; the gradient through w is 0, not NaN
    z = torch.zeros(2, 16, 3, dtype=torch.float64)
    r = S.spectrum_ref(z, 3)
    assert r["top"] == [0, 1, 2] and r["period"].tolist() == [16, 16, 8] and r["rows"].tolist() == [32, 32, 32]
    assert np.array_equal(r["period"], P.period_rows_ref(r["top"], 16, 2)[0])
    g = torch.Generator().manual_seed(1)
    g_w, g_xl = torch.randn(2, 3, generator=g, dtype=torch.float64), torch.randn(64, 3, generator=g, dtype=torch.float64)
    dx = S.spectrum_grad_ref(z, 3, g_w, g_xl)
    assert torch.equal(dx, g_xl.reshape(32, 2, 3)[:16].transpose(0, 1))


def test_knob_and_bindings():
    from immtsf import _lib, config
    assert config.timesnet_spectrum_fused is (os.environ.get("IMMTSF_TIMESNET_SPECTRUM_FUSED", "1") != "0")
    assert {"immtsf_timesnet_spectrum_ok", "immtsf_timesnet_spectrum_fwd", "immtsf_timesnet_spectrum_select",
            "immtsf_timesnet_spectrum_bwd"} <= set(_lib.exported_names())
    lib = _lib.load()
    for name in sorted(S.CASES):
        B, T, N, k = S.CASES[name][:4]
        assert lib.immtsf_timesnet_spectrum_ok(T, N, k) == 1, name
    B, T, N, k = S.PAST[1][:4]
    assert lib.immtsf_timesnet_spectrum_ok(T, N, k) == 0 and lib.immtsf_timesnet_spectrum_ok(T - 2, N, k) == 1
    assert lib.immtsf_timesnet_spectrum_ok(64, 16, 5) == 1 and lib.immtsf_timesnet_spectrum_ok(16, 4, 9) == 0      # k <= F - 1
