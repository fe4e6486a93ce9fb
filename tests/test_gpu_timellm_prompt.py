"""GPU checks of TimeLLM's prompt statistics in one launch: immtsf.ops.timellm_prompt_stats (csrc/timellm_prompt.hip) against the float64
restatement tests/timellm_prompt_ref.py (pinned to the torch expressions on the CPU in tests/test_timellm_prompt_ref.py) over the
windows of tests/timellm_prompt_cases.py, and models/TimeLLM.py through _get_prompt() / forecasting().
Bars: min, max, median are selections -- bit-equal.  Trend within L^2 2^-23 max|x| of float64 (the bound of a sequential fp32 sum of L
differences of magnitude <= 2 max|x|), its sign equal wherever the case module asserted the margin.  Lag lists identical to the
restatement's (the case module asserted the gaps that let float64 alone decide the order)."""
import functools
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timellm_prompt_cases as K  # noqa: E402
from test_timellm_prompt_ref import lag_classes, torch_expressions  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def _run(i):
    """the op on case i, once: (x on the device, stats and lags on the host)"""
    from immtsf import ops
    case = K.CASES[i]
    x = torch.tensor(case.x).to(_dev())
    stats, lags = ops.timellm_prompt_stats(x, case.top_k)
    assert stats.shape == (x.shape[0], 3 * case.C + 1) and stats.dtype == torch.float32
    assert lags.shape == (x.shape[0], case.top_k) and lags.dtype == torch.int32
    assert stats.untyped_storage().data_ptr() == lags.untyped_storage().data_ptr()                      # one device buffer
    assert lags.data_ptr() == stats.data_ptr() + 4 * (3 * case.C + 1)
    return x, stats.cpu().numpy(), lags.cpu().numpy()


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_min_max_median_are_bit_equal(i):
    case, C = K.CASES[i], K.CASES[i].C
    x, stats, _ = _run(i)
    want, got = case.stats64[:, :3 * C].astype(np.float32), stats[:, :3 * C]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])          # signed zeros included
    o = case.ordinary
    xo = x[o]
    ref = torch.cat([xo.min(dim=1)[0], xo.max(dim=1)[0], xo.median(dim=1).values], dim=1).cpu().numpy()
    assert np.array_equal(_bits(got[o]), _bits(ref))


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_trend_value_and_sign(i):
    case, C, L = K.CASES[i], K.CASES[i].C, K.CASES[i].L
    _, stats, _ = _run(i)
    for b, kind in enumerate(case.kinds):
        got, want = float(stats[b, 3 * C]), float(case.stats64[b, 3 * C])
        if kind == K.NAN:
            assert np.isnan(got) == np.isnan(want)
            continue
        bound = L * L * 2.0 ** -23 * float(np.abs(case.x[b]).max())
        print(f"{K.IDS[i]} window {b} ({kind}): trend {got:.9g}, float64 {want:.9g}, |diff| {abs(got - want):.3g}, bound {bound:.3g}")
        assert abs(got - want) <= bound
        if kind == K.ORDINARY:
            assert (got > 0) == (want > 0)
        if kind == K.CONSTANT or L == 1:
            assert got == 0.0


@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.IDS)
def test_lags(i):
    case, L, k = K.CASES[i], K.CASES[i].L, K.CASES[i].top_k
    x, _, lags = _run(i)
    assert np.array_equal(lags, case.lags64), (lags, case.lags64)
    _, _, _, _, fft = torch_expressions(x[case.ordinary], k)
    for b, ref in zip(case.ordinary, fft.cpu().tolist()):
        assert lag_classes(lags[b], L) == lag_classes(ref, L), (lags[b], ref)
    nan = lags[case.window(K.NAN)][:min(k, L)]
    assert ((0 <= nan) & (nan < L)).all() and len(set(nan.tolist())) == len(nan)
    assert lags[case.window(K.CONSTANT)].tolist() == [min(j, L - 1) for j in range(k)]


@pytest.mark.parametrize("i", [K.SHAPES.index((5, 32, 8, 5)), K.SHAPES.index((2, 257, 2, 7))], ids=["cfg5", "L257"])
def test_two_runs_give_the_same_bytes(i):
    from immtsf import ops
    case = K.CASES[i]
    x = torch.tensor(case.x).to(_dev())
    a = ops.timellm_prompt_packed(x, case.top_k).view(torch.int32).cpu()
    b = ops.timellm_prompt_packed(x.clone(), case.top_k).view(torch.int32).cpu()
    assert torch.equal(a, b)


def test_no_sync_inside_the_op():
    from immtsf import ops
    case = K.CASES[K.SHAPES.index((5, 32, 8, 5))]
    x = torch.tensor(case.x).to(_dev())
    ops.timellm_prompt_stats(x, case.top_k)         # the library is loaded and the kernel's code object is resident
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats, lags = ops.timellm_prompt_stats(x, case.top_k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(lags.cpu().numpy(), case.lags64)


def _model(dev, L=16, C=3, top_k=3):
    """an offline TimeLLM with the golden test's configuration (tests/test_gpu_fusion.py), input_len / C / top_k as asked"""
    from models.TimeLLM import TimeLLM
    cfg = types.SimpleNamespace(input_len=L, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=top_k, C=C, llm_model_timellm="GPT2", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device=str(dev),
                                immtsf_offline_llm=dict(vocab_size=320, n_positions=512, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0))
    torch.manual_seed(0)
    m = TimeLLM(cfg).to(dev)
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    return m


def test_unsupported_shapes_take_the_torch_path():
    from immtsf import _lib, ops
    dev = _dev()
    assert ops.timellm_prompt_supported(2048, 8, 64) and ops.timellm_prompt_supported(256, 64, 1)
    for L, C, k in [(2049, 1, 3), (1, 65, 3), (16, 3, 65), (2048, 9, 3), (257, 64, 3), (0, 3, 3), (16, 0, 3), (16, 3, 0)]:
        assert not ops.timellm_prompt_supported(L, C, k), (L, C, k)
    with pytest.raises(_lib.ImmtsfError):
        ops.timellm_prompt_stats(torch.zeros(1, 2049, 1, device=dev), 3)
    from immtsf import config
    m = _model(dev, top_k=65)            # one past the top_k limit: min(top_k, L) lags, padded
    x = torch.tensor(K.CASES[K.SHAPES.index((4, 16, 3, 3))].x[:4]).to(dev)
    default = config.timellm_prompt_fused
    try:
        config.timellm_prompt_fused = True
        prompts = m._get_prompt(x)
    finally:
        config.timellm_prompt_fused = default
    assert m.prompt_stat_calls == 0 and len(prompts) == 4
    assert len(re.search(r"Top lags \[([\d, ]+)\]", prompts[0]).group(1).split(",")) == 65


def test_module_prompt_knob_on_and_off():
    """the same skeleton and the same numbers with the knob on and off: strings equal after mapping each lag to min(tau, L - tau)"""
    from immtsf import config
    dev = _dev()
    m = _model(dev)
    case = K.CASES[K.SHAPES.index((4, 16, 3, 3))]
    x = torch.from_numpy(case.x[case.ordinary]).to(dev)
    pat = r"Top lags \[([\d, ]+)\]"
    fold = lambda q: re.sub(pat, lambda h: "Top lags " + str(lag_classes(h.group(1).split(","), 16)), q)      # noqa: E731
    default = config.timellm_prompt_fused
    try:
        config.timellm_prompt_fused = True
        on = m._get_prompt(x)
        assert m.prompt_stat_calls == 1
        config.timellm_prompt_fused = False
        off = m._get_prompt(x)
        assert m.prompt_stat_calls == 1
    finally:
        config.timellm_prompt_fused = default
    assert [fold(q) for q in on] == [fold(q) for q in off]
    # and the fused path spells the restatement's numbers: selections bit for bit, the asserted trend sign, the identical lag list
    assert on == m._format_prompts(torch.from_numpy(case.stats64[case.ordinary]).float(), torch.from_numpy(case.lags64[case.ordinary]))
    cpu = m._get_prompt(x.cpu())                       # a CPU tensor still returns the torch path's prompt
    assert m.prompt_stat_calls == 1 and [fold(q) for q in cpu] == [fold(q) for q in off]


def test_forecasting_counts_prompt_stat_calls():
    from immtsf import config
    dev = _dev()
    config.precision = "fp32"
    m = _model(dev).eval()
    g = torch.Generator().manual_seed(1)
    data = torch.randn(3, 12, 3, generator=g).to(dev)
    mask = (torch.rand(3, 12, 3, generator=g) < 0.8).float().to(dev)
    tp = torch.sort(torch.rand(3, 12, generator=g), 1).values.to(dev)
    tpp = torch.rand(3, 5, generator=g).to(dev)
    outs, default = [], config.timellm_prompt_fused
    try:
        for n, fused in ((1, True), (2, True), (2, False)):
            config.timellm_prompt_fused = fused
            outs.append(m.forecasting(tpp, data * mask, tp, mask))
            assert m.prompt_stat_calls == n
    finally:
        config.timellm_prompt_fused = default
    assert outs[0].shape == (3, 5, 3) and torch.isfinite(outs[0]).all()
    # the same prompt, the same tokens: what is left between two calls is the body's own rounding
    diff = float((outs[0] - outs[1]).detach().abs().max()) / float(outs[0].detach().abs().max())
    print(f"two forecasting() calls on one prompt: relative difference {diff:.3g}")
    assert diff <= 1e-4          # (the forward's bar of the golden test)
