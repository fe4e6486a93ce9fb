"""tests/timesnet_periods_ref.py (the float64 reference the GPU tests of TimesNet's period kernels compare with) against the project's own
plain-torch statements of the same thing, on the CPU: the tap order of its merged kernel against layers.Conv_Blocks.Inception_Block_V1
image by image, its composition against TimesBlock(cfg).double() (models/TimesNet.py:76-91, the branch a CPU tensor takes), and the
conditions under which a float32 device top-k must equal the float64 one for every spectral batch the GPU tests use."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timesnet_periods_ref as R  # noqa: E402


def _rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def _block(Cin, Cout, n, seed):
    from layers.Conv_Blocks import Inception_Block_V1
    torch.manual_seed(seed)
    blk = Inception_Block_V1(Cin, Cout, num_kernels=n).double()
    with torch.no_grad():
        for c in blk.kernels:
            c.bias.uniform_(-0.2, 0.2)
    return blk


def test_period_rows_ref_by_hand():
    period, rows = R.period_rows_ref([0, 1, 2, 7, 6, 3], 14, 3)
    assert period.dtype == np.int32 and rows.dtype == np.int32
    assert period.tolist() == [14, 14, 7, 2, 2, 4]
    assert rows.tolist() == [42, 42, 42, 42, 42, 48]


@pytest.mark.parametrize("Cin,Cout,n,B,total,periods,act", [
    (3, 5, 3, 2, 15, [15, 7, 5, 2, 2, 1], "gelu"),
    (4, 2, 2, 3, 14, [14, 4, 2, 3], None),
    (2, 3, 1, 1, 9, [9, 2, 1], "gelu"),
])
@pytest.mark.parametrize("shared", [True, False])
def test_conv_periods_ref_is_the_inception_block_image_by_image(Cin, Cout, n, B, total, periods, act, shared):
    """the merge written out here -- the mean of the n kernels, each zero-padded to (2n-1) x (2n-1), flattened tap-major / channel-minor --
    and conv_periods_ref on it against the block itself (the mean of n same-padded convolutions) on every image; 1e-12: pins the tap order"""
    blk = _block(Cin, Cout, n, seed=Cin * 10 + Cout)
    KS, Lmax, k = 2 * n - 1, 2 * total, len(periods)
    Wsum = torch.zeros(Cout, Cin, KS, KS, dtype=torch.float64)
    for i, c in enumerate(blk.kernels):
        r = n - 1 - i
        Wsum[:, :, r:KS - r, r:KS - r] += c.weight.detach()
    Weff = (Wsum / n).permute(0, 2, 3, 1).reshape(Cout, KS * KS * Cin)
    beff = torch.stack([c.bias.detach() for c in blk.kernels]).mean(0)
    W2, b2, K2 = R.merged_kernel([c.weight.detach() for c in blk.kernels], [c.bias.detach() for c in blk.kernels])
    assert K2 == KS and torch.equal(W2, Weff) and torch.equal(b2, beff)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*(() if shared else (k,)), Lmax * B, Cin, generator=g, dtype=torch.float64)
    y, valid = R.conv_periods_ref(x, periods, Weff, beff, KS, B, Lmax, act)
    assert y.shape == (k, Lmax * B, Cout) and valid.shape == (k, Lmax * B)
    for j, p in enumerate(periods):
        length = -(-total // p) * p
        assert int(valid[j].sum()) == length * B and bool(valid[j, :length * B].all())
        xj = x if shared else x[j]
        img = xj[:length * B].reshape(length, B, Cin).permute(1, 2, 0).reshape(B, Cin, length // p, p)
        want = blk(img)
        if act == "gelu":
            want = F.gelu(want)
        want = want.reshape(B, Cout, length).permute(2, 0, 1).reshape(length * B, Cout)
        assert _rel(y[j, :length * B], want.detach()) <= 1e-12, j
        assert not y[j, length * B:].any()


def _cfg(input_len, pred_len, d_model, d_ff, num_kernels, top_k):
    return types.SimpleNamespace(input_len=input_len, pred_len=pred_len, d_model=d_model, d_ff=d_ff, num_kernels=num_kernels, top_k=top_k)


BLOCK_CFGS = {"a": _cfg(18, 12, 8, 16, 3, 5), "b": _cfg(18, 12, 8, 16, 3, 5), "c": _cfg(40, 26, 8, 16, 2, 4)}


@pytest.mark.parametrize("name", ["a", "c"])
def test_composition_is_timesblock_double(name):
    """period_rows_ref + conv_periods_ref (twice) + period_aggregate_ref with the float64 top-k against TimesBlock(cfg).double() on the
    CPU (x.is_cuda is false: the plain-torch loop over host periods): output and data gradient to 1e-12"""
    from models.TimesNet import TimesBlock
    cfg = BLOCK_CFGS[name]
    B, total, N, freqs, amps, seed = R.BLOCK_BATCHES[name]
    assert total == cfg.input_len + cfg.pred_len and N == cfg.d_model and len(freqs) == cfg.top_k
    torch.manual_seed(3)
    blk = TimesBlock(cfg).double()
    with torch.no_grad():
        for inc in (blk.conv[0], blk.conv[2]):
            for c in inc.kernels:
                c.bias.uniform_(-0.2, 0.2)
    x = R.spectral_batch(B, total, N, freqs, amps, seed).double()
    up = torch.randn(B, total, N, dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    want = blk(xa)
    (want * up).sum().backward()
    xb = x.clone().requires_grad_(True)
    top, _, weight = R.spectrum_topk(xb, cfg.top_k)
    blocks = [([c.weight for c in inc.kernels], [c.bias for c in inc.kernels]) for inc in (blk.conv[0], blk.conv[2])]
    got = R.timesblock_ref(xb, top, weight, blocks, B, total)
    (got * up).sum().backward()
    assert _rel(got.detach(), want.detach()) <= 1e-12
    assert _rel(xb.grad, xa.grad) <= 1e-12


def test_period_aggregate_ref_by_loop():
    B, total, N, k = 2, 5, 3, 4
    Lmax = 2 * total
    g = torch.Generator().manual_seed(1)
    Y = torch.randn(k, Lmax * B, N, generator=g, dtype=torch.float64)
    w = torch.rand(B, k, generator=g, dtype=torch.float64)
    x = torch.randn(B, total, N, generator=g, dtype=torch.float64)
    want = x.clone()
    for b in range(B):
        for t in range(total):
            for j in range(k):
                want[b, t] += w[b, j] * Y[j, t * B + b]
    assert _rel(R.period_aggregate_ref(Y, w, x, B, total, Lmax), want) <= 1e-14


@pytest.mark.parametrize("name", sorted(R.BLOCK_BATCHES))
def test_spectral_batches_select_their_lines_with_a_margin(name):
    """what the GPU comparison of a whole TimesBlock rests on: the float64 top-k of the batch is exactly its lines, in the order of their
    amplitudes, and the weakest selected mean amplitude is at least twice the strongest unselected one -- float32 FFT round-off (1e-6 of
    the strongest line) cannot move a frequency across a factor of two, so the device selects the same set"""
    B, total, N, freqs, amps, seed = R.BLOCK_BATCHES[name]
    x = R.spectral_batch(B, total, N, freqs, amps, seed)
    assert x.dtype == torch.float32 and x.shape == (B, total, N)
    k = len(freqs)
    top, freq, _ = R.spectrum_topk(x, k)
    assert top.tolist() == list(freqs)
    rest = freq.clone()
    rest[top] = 0
    assert float(freq[top[-1]]) >= 2.0 * float(rest.max()), (float(freq[top[-1]]), float(rest.max()))
    # and the periods the configuration is meant to reach
    period, _ = R.period_rows_ref(top, total, B)
    assert period.tolist() == [total // f for f in freqs]
