"""CPU checks around TimeLLM's fused prompt statistics (immtsf.ops.timellm_prompt_stats, csrc/timellm_prompt.hip): the float64
restatement tests/timellm_prompt_ref.py against the torch expressions of models/TimeLLM.py _get_prompt evaluated in float64; the string
formatting helper, which takes host tensors only; header and binding on the two new symbols."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timellm_prompt_cases as K  # noqa: E402
import timellm_prompt_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def torch_expressions(x, top_k):
    """_get_prompt's own expressions (models/TimeLLM.py), on whatever dtype and device x has"""
    L = x.shape[1]
    mins, maxs = x.min(dim=1)[0], x.max(dim=1)[0]
    meds = x.median(dim=1).values
    trend = x.diff(dim=1).sum(dim=1).mean(dim=1)
    spec = torch.fft.rfft(x.permute(0, 2, 1), dim=-1)
    corr = torch.fft.irfft(spec * spec.conj(), n=L, dim=-1).mean(dim=1)
    _, lags = corr.topk(min(top_k, L), dim=-1)
    if lags.size(1) < top_k:
        lags = torch.cat([lags, lags[:, -1, None].repeat(1, top_k - lags.size(1))], dim=-1)
    return mins, maxs, meds, trend, lags


def lag_classes(lags, L):
    return sorted(min(int(v), L - int(v)) for v in lags)


def _model():
    """an offline TimeLLM with the golden test's configuration, on the CPU"""
    from models.TimeLLM import TimeLLM
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="GPT2", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device="cpu",
                                immtsf_offline_llm=dict(vocab_size=320, n_positions=512, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0))
    return TimeLLM(cfg)


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_restatement_equals_the_torch_expressions_in_float64(case):
    """ordinary windows: min, max and median equal, trend within 1e-12 relative, lag lists equal as classes {tau, L - tau} (inside a
    pair the FFT's order is rounding noise)"""
    x = torch.from_numpy(case.x[case.ordinary]).double()
    mins, maxs, meds, trend, lags = torch_expressions(x, case.top_k)
    C = case.C
    for i, b in enumerate(case.ordinary):
        s = case.stats64[b]
        assert np.array_equal(s[:C], mins[i].numpy()) and np.array_equal(s[C:2 * C], maxs[i].numpy())
        assert np.array_equal(s[2 * C:3 * C], meds[i].numpy())
        assert abs(s[3 * C] - float(trend[i])) <= 1e-12 * max(abs(float(trend[i])), 1e-300)
        assert lag_classes(case.lags64[b], case.L) == lag_classes(lags[i].tolist(), case.L), (case.lags64[b], lags[i])


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_restatement_on_the_special_windows(case):
    C, L, k = case.C, case.L, case.top_k
    pad = [min(i, L - 1) for i in range(k)]
    s, lg = case.stats64[case.window(K.CONSTANT)], case.lags64[case.window(K.CONSTANT)]
    assert np.array_equal(s[:3 * C], np.full(3 * C, 0.75)) and s[3 * C] == 0.0 and list(lg) == pad
    b = case.window(K.SIGNED_ZERO)
    s = case.stats64[b]
    assert np.signbit(s[0]) and np.signbit(s[C]) and np.signbit(s[2 * C]) and s[0] == 0.0          # all -0.0
    if C >= 2:      # +0.0 first, then -0.0: min and max are the first element; the median is the element of index (L - 1) // 2
        assert not np.signbit(s[1]) and not np.signbit(s[C + 1]) and bool(np.signbit(s[2 * C + 1])) == ((L - 1) // 2 >= 1)
    b = case.window(K.NAN)
    s, lg = case.stats64[b], case.lags64[b]
    assert np.isnan(s[[C - 1, 2 * C - 1, 3 * C - 1]]).all() and np.isnan(s[:3 * C]).sum() == 3 and list(lg) == pad


def test_format_helper_reproduces_the_torch_path_byte_for_byte():
    """_format_prompts on HOST tensors (the statistics packed as the op packs them) against _get_prompt's torch path on the same CPU
    windows; the golden's prompt0 anchors the all-zero window"""
    m = _model()
    case = K.CASES[K.SHAPES.index((4, 16, 3, 3))]
    x = torch.from_numpy(case.x[case.ordinary])
    mins, maxs, meds, trend, lags = torch_expressions(x, m.top_k)
    stats = torch.cat([mins, maxs, meds, trend[:, None]], dim=1)
    assert stats.dtype == torch.float32 and not stats.is_cuda
    before = m.prompt_stat_calls
    assert m._format_prompts(stats, lags.to(torch.int32)) == m._get_prompt(x)
    assert m.prompt_stat_calls == before                       # a CPU tensor takes the torch path
    # the restatement's numbers, cast to fp32, spell the same text up to the order inside a lag pair
    mine = m._format_prompts(torch.from_numpy(case.stats64[case.ordinary]).float(), torch.from_numpy(case.lags64[case.ordinary]).int())
    pat = r"Top lags \[([\d, ]+)\]"
    for a, b, row in zip(mine, m._get_prompt(x), case.stats64[case.ordinary]):
        # min, max, median are selections: the same floats.  The fp32 torch trend only has to have the float64 trend's sign
        assert re.sub(pat, "", a) == re.sub(pat, "", b)
        assert ("Trend upward" in a) == (row[-1] > 0)
        assert lag_classes(re.search(pat, a).group(1).split(","), 16) == lag_classes(re.search(pat, b).group(1).split(","), 16)
    z = np.load(os.path.join(GOLDEN, "model_timellm.npz"))
    p0 = str(z["prompt0"])
    lags0 = torch.tensor([[int(v) for v in re.search(pat, p0).group(1).split(",")]], dtype=torch.int32)
    assert m._format_prompts(torch.zeros(1, 10), lags0) == [p0]
    assert m._get_prompt(torch.zeros(1, 16, 3))[0] == p0


def test_header_and_binding_agree_on_the_new_symbols():
    from immtsf import _lib
    src = open(os.path.join(ROOT, "include", "immtsf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("immtsf_timellm_prompt_supported", "immtsf_timellm_prompt_stats"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, f"{name} is not declared in include/immtsf.h"
        assert name in _lib.exported_names()
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == len(decl.group(1).split(",")), (name, fn.argtypes, decl.group(1))
    lib = _lib.load()
    assert lib.immtsf_timellm_prompt_supported(2048, 8, 64) == 1 and lib.immtsf_timellm_prompt_supported(32, 8, 5) == 1
    # outside the envelope the host wrapper answers before it looks at a pointer or launches anything
    assert lib.immtsf_timellm_prompt_stats(None, 1, 2049, 1, 3, None, None) == -3


def test_op_refuses_cpu_tensors():
    from immtsf import ops
    from immtsf._lib import ImmtsfError
    with pytest.raises(ImmtsfError):
        ops.timellm_prompt_stats(torch.zeros(2, 16, 3), 3)
