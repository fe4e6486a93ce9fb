"""Informer's layers are defined by this build: with no reference tree on the path the four names import from the product's `layers`
modules, a stack composed from them has exactly the golden's state_dict keys and shapes, and a CPU tensor raises ImmtsfError."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import informer_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imm-tsf_amd")


def test_the_four_names_import_standalone():
    code = """
        import layers.SelfAttention_Family as S, layers.Transformer_EncDec as T
        for mod, names in ((S, ["ProbAttention"]), (T, ["ConvLayer", "DecoderLayer", "Decoder"])):
            for n in names:
                cls = getattr(mod, n)
                assert cls.__module__ == mod.__name__ and 'imm-tsf_amd' in mod.__file__, (n, cls.__module__)
        from immtsf import config, ops
        assert config.informer_fused is True and callable(ops.prob_attention) and callable(ops.conv_distil)
        print('ok')
        """
    env = dict(os.environ, PYTHONPATH=PKG)
    env.pop("IMMTSF_INFORMER_FUSED", None)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_stack_has_the_reference_state_dict(name):
    z, params, _, _ = IC.golden(name)
    m = IC.Stack(IC.config(IC.FIXTURES[name]))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in params.items()}
    m.load_state_dict(params, strict=True)


def test_cpu_tensors_raise():
    from immtsf import ops
    from immtsf._lib import ImmtsfError
    from layers.SelfAttention_Family import ProbAttention
    from layers.Transformer_EncDec import ConvLayer
    q = torch.randn(2, 6, 2, 4)
    with pytest.raises(ImmtsfError):
        ProbAttention(False, factor=1)(q, q, q, None)
    with pytest.raises(ImmtsfError):
        ops.prob_attention(q, q, q, torch.zeros(6, 2, dtype=torch.int32), 2, 0.5, False)
    with pytest.raises(ImmtsfError):
        ConvLayer(8)(torch.randn(2, 5, 8))
    m, batch, _ = IC.golden_model("model_informer", "cpu")
    with pytest.raises(ImmtsfError):
        m.forecasting(*batch[:4])
    with pytest.raises(NotImplementedError):
        ProbAttention(False, output_attention=True)(q, q, q, None)


def test_supported_envelope_covers_the_reference_configuration():
    from immtsf import ops
    for L in (96, 336, 512):      # d_model 512 / n_heads 2 -> D = 256, factor 3
        u = min(3 * 7, L)
        assert ops.prob_attention_supported(L, L, 256, u) and ops.prob_attention_supported(L, 512, 256, u)
    assert not ops.prob_attention_supported(1025, 96, 256, 15) and not ops.prob_attention_supported(96, 96, 516, 15)
    assert ops.conv_distil_supported(512) and not ops.conv_distil_supported(6) and not ops.conv_distil_supported(1028)
