"""CPU checks of the stored-bf16 Llama route: the knob parses, every new symbol is exported with the documented argument
count, and the model-side predicate of llama_embed_notes_supported / llama_body_supported (immtsf.ops._llama_model_kind: everything short
of the library's answer on widths and lengths, and of the device) gives the documented answers for CPU models."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_embed_ref as LR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"immtsf_gemm_asplit_supported": 7, "immtsf_gemm_asplit": 12, "immtsf_llama_embed_tokens_p16": 7,
           "immtsf_llama_embed_rmsnorm_p16": 8, "immtsf_llama_embed_add_rmsnorm_p16": 9, "immtsf_llama_embed_pool_p16": 11,
           "immtsf_llama_body_rmsnorm_p16": 13, "immtsf_llama_body_rmsnorm_backward_p16": 10}


@pytest.mark.parametrize("value,want", [(None, False), ("0", False), ("1", True), ("yes", False)])
def test_the_knob_parses(value, want):
    env = {k: v for k, v in os.environ.items() if k != "IMMTSF_LLAMA_STORED_BF16"}
    if value is not None:
        env["IMMTSF_LLAMA_STORED_BF16"] = value
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "imm-tsf_amd")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.check_output([sys.executable, "-c", "from immtsf import config; print(config.llama_stored_bf16)"], env=env, text=True)
    assert out.strip() == str(want)


def test_every_new_symbol_is_exported_with_its_argument_count():
    from immtsf import _lib
    lib = _lib.load()
    for name, n_args in SYMBOLS.items():
        fn = getattr(lib, name)
        assert name in _lib.exported_names() and len(fn.argtypes) == n_args, name
    # the p16 entry points take their fp32 sibling's arguments, the parameter pointer apart
    for name in SYMBOLS:
        if name.endswith("_p16"):
            assert len(getattr(lib, name).argtypes) == len(getattr(lib, name[:-4]).argtypes), name
    # the support set is immtsf_gemm_split's, and answers without a GPU
    for args in ((0, 9, 16, 16, 16, 16, 16), (1, 9, 16, 16, 16, 16, 16), (0, 9, 16, 12, 12, 12, 16), (1, 9, 12, 16, 16, 12, 12),
                 (0, 9, 16, 16, 18, 16, 16), (0, 9, 16, 16, 16, 16, 8), (2, 9, 16, 16, 16, 16, 16)):
        assert lib.immtsf_gemm_asplit_supported(*args) == lib.immtsf_gemm_split_supported(*args), args
    assert lib.immtsf_gemm_asplit_supported(0, 9, 16, 16, 16, 16, 16) and not lib.immtsf_gemm_asplit_supported(0, 9, 16, 12, 12, 12, 16)


def _build(**kw):
    args = dict(n_head=2, n_kv=1, hidden=256, inner=512, head_dim=128, rope=LR.DEFAULT_ROPE)
    args.update(kw)
    return LR.build_llama(None, 50, 1, max_pos=96, **args).requires_grad_(False)


def _store_bf16(m):
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m


def test_the_model_side_predicate(monkeypatch):
    import immtsf
    from immtsf import ops
    stored = _store_bf16(_build())
    assert stored.rotary_emb.inv_freq.dtype == torch.float32
    mixed = _store_bf16(_build())
    mixed.layers[0].mlp.up_proj.weight.data = mixed.layers[0].mlp.up_proj.weight.data.float()
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", False)
    assert ops._llama_model_kind(_build()) == "fp32"
    assert ops._llama_model_kind(stored) is None and ops._llama_model_kind(_build().to(torch.bfloat16)) is None
    assert not ops.llama_embed_notes_supported(stored, 8) and not ops.llama_body_supported(stored, 3, 5)
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", True)
    assert ops._llama_model_kind(_build()) == "fp32"
    assert ops._llama_model_kind(stored) == "bf16" and ops._llama_model_kind(_build().to(torch.bfloat16)) == "bf16"
    assert ops._llama_model_kind(mixed) is None
    assert ops._llama_model_kind(_build().to(torch.float16)) is None
    assert ops._llama_model_kind(_store_bf16(_build(hidden=128, head_dim=64))) is None
    assert ops._llama_model_kind(_store_bf16(_build(rope={"rope_type": "dynamic", "rope_theta": 10000.0, "factor": 2.0}))) is None
    assert ops._llama_model_kind(_store_bf16(_build(attention_bias=True))) is None
    assert ops._llama_model_kind(torch.nn.Linear(4, 4)) is None
    # a stored-bf16 model must sit on one CUDA device: on the CPU both front predicates still refuse it
    assert not ops.llama_embed_notes_supported(stored, 8) and not ops.llama_body_supported(stored, 3, 5)
