"""GPU checks of config.frozen_products = "split" (DESIGN 4u): the frozen GPT-2 / Llama / BERT bodies and the three note-embedding
operators with their weight products on csrc/gemm_split.hip, in fp32 mode, against the float64 restatements and on the cases of
tests/test_gpu_gpt2.py, test_gpu_llama_body.py, test_gpu_bert_body.py, test_gpu_note_embed.py, test_gpu_bert_embed.py and
test_gpu_llama_embed.py (imported): the two smallest (shape, layers) cases of each body list by row count -- for Llama and BERT the
smaller on the first body of the file and the larger on its last, so that two widths are covered -- and both note batches, the Llama
ones on the first and the last body.
Bars: the project's fp32 bars of those files, 1e-4 for an output and 3e-4 for a gradient, relative to the largest element.  Each test
prints the split error next to the same case's fp32-mode and bf16-mode errors (the table of DESIGN 4u)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_bert_body as TB  # noqa: E402
import test_gpu_bert_embed as EB  # noqa: E402
import test_gpu_gpt2 as TG  # noqa: E402
import test_gpu_llama_body as TL  # noqa: E402
import test_gpu_llama_embed as EL  # noqa: E402
import test_gpu_note_embed as EG  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_BAR, GRAD_BAR = 1e-4, 3e-4
assert (TG.OUT_BAR, TG.GRAD_BAR) == (TL.OUT_BAR, TL.GRAD_BAR) == (TB.OUT_BAR, TB.GRAD_BAR) == (OUT_BAR, GRAD_BAR)
assert EG.BAR == EB.BAR == EL.BAR == OUT_BAR


def _rows(shape):
    return shape[0] * (shape[1] + shape[2])


def _smallest(shape_cases):
    return sorted(shape_cases, key=lambda c: _rows(c[0]))[:2]


def _on_first_and_last(bodies, pair):
    names = list(bodies)
    return [(names[0],) + tuple(pair[0]), (names[-1],) + tuple(pair[1])]


GPT2_CASES = _smallest(TG.CASES)                                            # (shape, n_layer)
LLAMA_CASES = _on_first_and_last(TL.BODIES, _smallest(TL.SHAPE_CASES))      # (body, shape, n_layer)
BERT_CASES = _on_first_and_last(TB.BODIES, _smallest(TB.SHAPE_CASES))
NOTE_BATCHES = sorted(EG.BATCHES, key=lambda n: sum(EG.BATCHES[n]))[:2]
LLAMA_NOTE_CASES = _on_first_and_last(EL.BODIES, [(n,) for n in sorted(EL.BATCHES, key=lambda n: sum(EL.BATCHES[n]))[:2]])


class _Mode:
    """config.precision / config.frozen_products for one run, restored afterwards"""

    def __init__(self, precision, products):
        self.want = (precision, products)

    def __enter__(self):
        from immtsf import config
        self.was = (config.precision, config.frozen_products)
        config.precision, config.frozen_products = self.want

    def __exit__(self, *exc):
        from immtsf import config
        config.precision, config.frozen_products = self.was


def _three_ways(run):
    """run(precision) under fp32 products (before the knob is touched, and again after), split products and bf16 mode; asserts that the
    split run went through immtsf_gemm_split and that the knob at "fp32" changes no bit"""
    from immtsf import config, ops
    assert config.frozen_products == "fp32"
    before = run("fp32")
    with _Mode("fp32", "split"):
        calls = ops.split_product_calls
        split = run("fp32")
        assert ops.split_product_calls > calls, "the split kernel did not run"
        calls = ops.split_product_calls
    with _Mode("fp32", "fp32"):
        after = run("fp32")
    assert ops.split_product_calls == calls
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    with _Mode("bf16", "split"):          # bf16 mode does not read the knob
        bf = run("bf16")
    assert ops.split_product_calls == calls
    return before, split, bf


def _report(what, refs, runs, rel):
    names = ("out", "d tail")[:len(refs)]
    errs = [[rel(r[i], refs[i]) for i in range(len(refs))] for r in runs]
    for i, n in enumerate(names):
        print(f"{what} {n}: split {errs[1][i]:.2e}  fp32 {errs[0][i]:.2e}  bf16 {errs[2][i]:.2e}  (bar {(OUT_BAR, GRAD_BAR)[i]:.0e})")
    return errs[1]


@pytest.mark.parametrize("shape,n_layer", GPT2_CASES, ids=[f"B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for s, n in GPT2_CASES])
def test_gpt2_body(shape, n_layer):
    m = TG._body(n_layer, 0.0, **TG._positions(shape))

    def run(precision):
        from immtsf import config
        config.precision = precision          # tests/test_gpu_gpt2.py's _fused reads the global
        return TG._fused(m, shape)[:2]
    errs = _report(f"gpt2 body {shape} L{n_layer}", TG._reference(shape, n_layer), _three_ways(run), TG._rel)
    assert errs[0] < OUT_BAR and errs[1] < GRAD_BAR


@pytest.mark.parametrize("body,shape,n_layer", LLAMA_CASES, ids=[f"{b}_B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for b, s, n in LLAMA_CASES])
def test_llama_body(body, shape, n_layer):
    errs = _report(f"llama body {body} {shape} L{n_layer}", TL._reference(body, shape, n_layer),
                   _three_ways(lambda precision: TL._fused(body, shape, n_layer, precision)[:2]), TL._rel)
    assert errs[0] < OUT_BAR and errs[1] < GRAD_BAR


@pytest.mark.parametrize("body,shape,n_layer", BERT_CASES, ids=[f"{b}_B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for b, s, n in BERT_CASES])
def test_bert_body(body, shape, n_layer):
    errs = _report(f"bert body {body} {shape} L{n_layer}", TB._reference(body, shape, n_layer),
                   _three_ways(lambda precision: TB._fused(body, shape, n_layer, precision)[:2]), TB._rel)
    assert errs[0] < OUT_BAR and errs[1] < GRAD_BAR


@pytest.mark.parametrize("name", NOTE_BATCHES)
def test_gpt2_embed_notes(name):
    errs = _report(f"gpt2 notes {name}", (EG._reference(name),), _three_ways(lambda precision: (EG._fused(name, precision),)), EG._rel)
    assert errs[0] < OUT_BAR


@pytest.mark.parametrize("name", NOTE_BATCHES)
def test_bert_embed_notes(name):
    errs = _report(f"bert notes {name}", (EB._reference(name),), _three_ways(lambda precision: (EB._fused(name, precision),)), EB._rel)
    assert errs[0] < OUT_BAR


@pytest.mark.parametrize("body,name", LLAMA_NOTE_CASES, ids=[f"{b}_{n}" for b, n in LLAMA_NOTE_CASES])
def test_llama_embed_notes(body, name):
    errs = _report(f"llama notes {body} {name}", (EL._reference(body, name),),
                   _three_ways(lambda precision: (EL._fused(body, name, precision),)), EL._rel)
    assert errs[0] < OUT_BAR


def test_the_knob_refuses_other_values():
    from immtsf import config
    was = config.frozen_products
    try:
        config.frozen_products = "bf16x3"
        with pytest.raises(ValueError):
            config.frozen_split(0)
    finally:
        config.frozen_products = was
    assert config.frozen_split(0) is False and config.frozen_split(1) is False


def test_weight_images_follow_the_weight():
    """the (hi, lo) pair is cached per weight and remade when the weight is written in place, like the bf16 image"""
    from immtsf import ops
    TG._dev()
    m = TG._body(1, 0.0)
    W = m.h[0].mlp.c_fc.weight
    a = ops._gpt2_w_split(m, W)
    assert ops._gpt2_w_split(m, W) is a
    hi, lo = a
    assert torch.equal(hi, W.to(torch.bfloat16)) and torch.equal(lo, (W - hi.float()).to(torch.bfloat16))
    keep = W.detach().clone()
    try:
        with torch.no_grad():
            W.mul_(1.5)
        b = ops._gpt2_w_split(m, W)
        assert b is not a and torch.equal(b[0], W.to(torch.bfloat16))
    finally:
        with torch.no_grad():
            W.copy_(keep)


def _image_cases():
    """name -> (image(bf): the bf16 image (bf) or the (hi, lo) pair of the cached fp32 weight, weight(): that weight restated, the
    parameter the test writes) on the one-layer bodies of the three body test files"""
    from immtsf import ops
    g, b, m = TG._body(1, 0.0), TB._model("a", 1), TL._model("a", 1)
    Wg, att, sa = g.h[0].mlp.c_fc.weight, b.encoder.layer[0].attention.self, m.layers[0].self_attn
    qkv = (sa.q_proj, sa.k_proj, sa.v_proj)
    return {"gpt2_w16": (lambda bf: ops._gpt2_w16(g, Wg) if bf else ops._gpt2_w_split(g, Wg), lambda: Wg.detach(), Wg),
            "bert_qkv": (lambda bf: ops._bert_qkv(b, att, bf, not bf)[2],
                         lambda: torch.cat([att.query.weight, att.key.weight, att.value.weight], 0), att.key.bias),
            "llama_cat": (lambda bf: ops._llama_cat(m, sa, "qkv", qkv, bf, not bf)[1], lambda: torch.cat([p.weight for p in qkv], 0),
                          sa.k_proj.weight)}


def _is_rounding_of(img, W):
    if isinstance(img, tuple):
        return torch.equal(img[0], W.to(torch.bfloat16)) and torch.equal(img[1], (W - img[0].float()).to(torch.bfloat16))
    return torch.equal(img, W.to(torch.bfloat16))


@pytest.mark.parametrize("name", ["gpt2_w16", "bert_qkv", "llama_cat"])
def test_cached_images_follow_their_parameters(name):
    """_gpt2_w16, _bert_qkv and _llama_cat: the same object on a second call, the image equal to the weight's rounding, a new object after
    an in-place write to one of the keyed parameters (for _bert_qkv the key's bias, the fifth of its six) -- and the bf16 image and the
    (hi, lo) pair live side by side in one entry, whichever is asked for first"""
    from immtsf import ops
    TG._dev()
    image, weight, written = _image_cases()[name]
    a16 = image(True)
    assert image(True) is a16 and _is_rounding_of(a16, weight())
    pair = image(False)
    assert isinstance(pair, tuple) and image(False) is pair and _is_rounding_of(pair, weight())
    assert image(True) is a16                                   # the pair did not displace the image
    keep = written.detach().clone()
    try:
        with torch.no_grad():
            written.mul_(1.5)
        pair2 = image(False)                                    # the other way round on the new entry: the pair first
        assert pair2 is not pair and pair2[0] is not pair[0] and _is_rounding_of(pair2, weight())
        b16 = image(True)
        assert b16 is not a16 and _is_rounding_of(b16, weight())
        assert image(False) is pair2 and image(True) is b16
        if name == "bert_qkv":
            att = TB._model("a", 1).encoder.layer[0].attention.self
            assert torch.equal(ops._bert_qkv(TB._model("a", 1), att, False)[1], torch.cat([att.query.bias, att.key.bias, att.value.bias], 0))
    finally:
        with torch.no_grad():
            written.copy_(keep)


def test_timellm_end_to_end():
    """forecasting() + backward at the toy size of tests/test_gpu_gpt2.py, offline GPT-2, the model in eval mode (no dropout anywhere -- the
    reprogramming layer's and the body's draw a fresh key per call -- so that the two runs are the same function): split against fp32 products within the fp32 bars"""
    from immtsf import ops
    dev = TG._dev()

    def run():
        m, batch = TG._timellm(dev)
        m.eval()
        out = m.forecasting(*batch)
        out.square().mean().backward()
        assert m.fused_body_calls == 1
        return out.detach(), {k: p.grad.detach() for k, p in m.named_parameters() if p.requires_grad}

    with _Mode("fp32", "fp32"):
        out32, grads32 = run()
    with _Mode("fp32", "split"):
        calls = ops.split_product_calls
        out, grads = run()
        assert ops.split_product_calls > calls
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())
    eo = float((out - out32).abs().max() / out32.abs().max())
    # (the floor of smoke()'s gradient check: a parameter whose gradient is rounding noise around zero has no relative error to speak of)
    eg = max(float((grads[k] - grads32[k]).abs().max() / max(float(grads32[k].abs().max()), 1e-3)) for k in grads)
    print(f"TimeLLM toy, split vs fp32 products: out {eo:.2e} (bar {OUT_BAR:.0e})  worst parameter gradient {eg:.2e} (bar {GRAD_BAR:.0e})")
    assert eo < OUT_BAR and eg < GRAD_BAR
