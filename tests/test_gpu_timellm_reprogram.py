"""GPU checks of TimeLLM's word prototypes in folded form: immtsf.ops.timellm_prototypes (csrc/timellm_reprogram.hip) against the float64
restatement of the stage as the reference writes it (tests/timellm_reprogram_ref.py, pinned on the CPU by
tests/test_timellm_reprogram_ref.py) over tests/timellm_reprogram_cases.py, and models/TimeLLM.py with the knob on against off.

Every comparison is element by element, relative to the largest element of the tensor.  Bars: fp32 mode the project's own (DESIGN 4j /
4l), 1e-4 for outputs and 3e-4 for gradients, with the absolute floor of test_timellm_forecasting_vs_reference_golden under dbk.  bf16
mode: 4 x the error of the as-written composition under torch.autocast(bfloat16) on the same GPU against float64, measured here per
shape and tensor (DESIGN 4l's precedent; the margin covers the different rounding points of the two groupings)."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timellm_reprogram_cases as K  # noqa: E402
import timellm_reprogram_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
OUTS = ("k", "v")
FLOOR = {"bk": 1e-4}
EUNSUPPORTED = -3            # IMMTSF_EUNSUPPORTED (include/immtsf.h)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _tensors(i):
    t = {n: torch.tensor(a).to(_dev()) for n, a in K.inputs(i).items()}
    for n in R.PARAMS:
        t[n].requires_grad_(True)
    return t


def _op(i, precision):
    """one forward + backward of the operator on case i: {"k", "v", six gradients} on the host"""
    from immtsf import ops
    t = _tensors(i)
    assert ops.timellm_prototypes_supported(t["E"], t["W_map"], t["Wk"], t["Wv"])
    k, v = ops.timellm_prototypes(*[t[n] for n in ("E",) + R.PARAMS], precision=precision)
    S, _, _, H, dkeys = K.SHAPES[i]
    assert k.shape == v.shape == (S, H * dkeys) and k.dtype == v.dtype == torch.float32 and k.is_contiguous() and v.is_contiguous()
    torch.autograd.backward([k, v], [t["dk"], t["dv"]])
    assert t["E"].grad is None
    out = {"k": k, "v": v, **{n: t[n].grad for n in R.PARAMS}}
    return {n: a.detach().cpu().numpy() for n, a in out.items()}


@functools.lru_cache(maxsize=None)
def _run(i, precision):
    return _op(i, precision)


def _err(got, want, floor=0.0):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), floor))


@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=K.IDS)
def test_fp32_against_float64(i):
    got, ref = _run(i, "fp32"), K.reference(i)
    errs = {n: _err(got[n], ref[n], FLOOR.get(n, 0.0)) for n in ref}
    print("fp32", K.IDS[i], {n: "%.2e" % e for n, e in errs.items()})
    for n, e in errs.items():
        assert e <= (1e-4 if n in OUTS else 3e-4), (n, e)


@functools.lru_cache(maxsize=None)
def _autocast(i):
    """the stage as written, nn.functional.linear three times, under torch.autocast(bfloat16) on the GPU"""
    t = _tensors(i)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        src = torch.nn.functional.linear(t["E"].permute(1, 0), t["W_map"], t["b_map"]).permute(1, 0)
        k = torch.nn.functional.linear(src, t["Wk"], t["bk"])
        v = torch.nn.functional.linear(src, t["Wv"], t["bv"])
    ((k.float() * t["dk"]).sum() + (v.float() * t["dv"]).sum()).backward()
    out = {"k": k.float(), "v": v.float(), **{n: t[n].grad for n in R.PARAMS}}
    return {n: a.detach().cpu().numpy() for n, a in out.items()}


@pytest.mark.parametrize("i", range(len(K.SHAPES)), ids=K.IDS)
def test_bf16_within_four_times_the_autocast_composition(i):
    got, auto, ref = _run(i, "bf16"), _autocast(i), K.reference(i)
    mine = {n: _err(got[n], ref[n]) for n in ref}
    theirs = {n: _err(auto[n], ref[n]) for n in ref}
    print("bf16", K.IDS[i], {n: "%.2e / %.2e" % (mine[n], theirs[n]) for n in ref})
    for n in ref:
        assert mine[n] <= 4.0 * theirs[n], (n, mine[n], theirs[n])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_runs_give_the_same_bytes(precision):
    i = 3                                     # several splits of V in both directions, S across three row tiles
    a, b = _run(i, precision), _op(i, precision)
    for n in a:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n


def test_unsupported_shapes_are_refused():
    from immtsf import _lib, ops
    dev = _dev()
    lib = _lib.load()
    f = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    E, W_map = f(40, 64), f(10, 40)
    assert ops.timellm_prototypes_supported(E, W_map, f(64, 64), f(64, 64))            # 2 D = 128
    assert not ops.timellm_prototypes_supported(E, W_map, f(72, 64), f(72, 64))        # 2 D = 144
    assert not ops.timellm_prototypes_supported(E, W_map, f(12, 64), f(12, 64))        # 2 D = 24: no multiple of 16
    assert not ops.timellm_prototypes_supported(f(40, 60), W_map, f(8, 60), f(8, 60))  # d_llm = 60: no multiple of 8
    assert not ops.timellm_prototypes_supported(E.clone().requires_grad_(True), W_map, f(8, 64), f(8, 64))
    assert not ops.timellm_prototypes_supported(E.cpu(), W_map.cpu(), f(8, 64).cpu(), f(8, 64).cpu())
    with pytest.raises(_lib.ImmtsfError):
        ops.timellm_prototypes(E, W_map, f(10), f(72, 64), f(72), f(72, 64), f(72))
    assert lib.immtsf_timellm_prototypes_supported(10, 40, 64, 72) == 0
    assert lib.immtsf_timellm_prototypes_scratch_bytes(10, 40, 64, 72, 0) == 0
    none = [None] * 6
    nil = ctypes.c_void_p(None)
    assert lib.immtsf_timellm_prototypes_forward(0, nil, nil, *none, 10, 40, 64, 72, None, None, None, None, nil, 0, None) == EUNSUPPORTED
    assert lib.immtsf_timellm_prototypes_backward(0, nil, nil, *none, 10, 40, 64, 72, *none, nil, 0, None) == EUNSUPPORTED
    assert lib.immtsf_timellm_prototypes_forward(0, nil, nil, *none, 10, 40, 60, 8, None, None, None, None, nil, 0, None) == EUNSUPPORTED


def _model(ts_vocab):
    from models.TimeLLM import TimeLLM
    dev = _dev()
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=ts_vocab, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=2, llm_model_timellm="GPT2", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=2, device=str(dev),
                                immtsf_offline_llm=dict(vocab_size=320, n_positions=512, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0))
    torch.manual_seed(77)
    m = TimeLLM(cfg).to(dev).train()
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    m.reprogramming_layer.dropout.p = 0.0
    g = torch.Generator().manual_seed(78)
    B, L, C, Lp = 2, 16, 2, 8
    data = torch.randn(B, L, C, generator=g).to(dev)
    mask = (torch.rand(B, L, C, generator=g) > 0.2).float().to(dev)
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values.to(dev)
    tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values.to(dev)
    up = torch.randn(B, Lp, C, generator=g).to(dev)
    return m, (tpp, data * mask, tp, mask), up


def _step(m, batch, up):
    for p in m.parameters():
        p.grad = None
    out = m.forecasting(*batch)
    (out * up).sum().backward()
    return out.detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.requires_grad}


def test_module_knob_on_equals_off():
    from immtsf import config
    m, batch, up = _model(200)
    S, d, D = 200, 768, 16
    assert S * d > 2 * D * (d + S)                       # the gate opens: the ratio is about 5
    saved = config.precision, config.timellm_reprogram_fused
    try:
        config.precision = "fp32"
        config.timellm_reprogram_fused = False
        out0, g0 = _step(m, batch, up)
        assert m.reprogram_fused_calls == 0
        config.timellm_reprogram_fused = True
        out1, g1 = _step(m, batch, up)
        assert m.reprogram_fused_calls == 1
    finally:
        config.precision, config.timellm_reprogram_fused = saved
    e = _err(out1, out0)
    print("module out", "%.2e" % e)
    assert e <= 1e-4
    assert sorted(g0) == sorted(g1) and any("mapping_layer" in n for n in g1)
    for n in g0:
        e = _err(g1[n], g0[n], 1e-4 if n.endswith("key_projection.bias") else 0.0)
        print("module grad", n, "%.2e" % e)
        assert e <= 3e-4, (n, e)


def test_module_gate_stays_closed_at_a_small_vocabulary():
    from immtsf import config
    m, batch, up = _model(20)
    saved = config.precision, config.timellm_reprogram_fused
    try:
        config.precision = "fp32"
        config.timellm_reprogram_fused = True
        _step(m, batch, up)
    finally:
        config.precision, config.timellm_reprogram_fused = saved
    assert m.reprogram_fused_calls == 0                  # 20 * 768 < 32 * (768 + 20)
