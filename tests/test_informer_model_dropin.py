"""models.Informer of this build without a GPU: the import on this tree alone, the state_dict against the goldens of the unmodified
reference, how the name resolves with a tree behind this one (immtsf/dropin.py, overlay_module), the refusal of CPU tensors and the
limits of the fused stages."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import informer_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imm-tsf_amd")


def _run(code, extra_path=""):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, extra_path]))
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)


def test_models_informer_imports_from_this_tree_alone():
    r = _run("""
        import os
        from models.Informer import Informer
        import models.Informer as M, torch.nn as nn
        assert 'imm-tsf_amd' in M.__file__ and os.path.basename(M.__file__) == 'informer_model.py', M.__file__
        assert issubclass(Informer, nn.Module) and Informer.immtsf_graphable and callable(Informer.forecasting)
        print('ok')
        """)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_state_dict_is_the_goldens(name):
    from models.Informer import Informer
    _, params, _, _ = IC.golden(name)
    cfg = IC.config(IC.FIXTURES[name])
    m = Informer(cfg)
    want = {k: tuple(v.shape) for k, v in params.items()}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    m.load_state_dict(params, strict=True)
    assert "zeros_pad" not in m.state_dict() and tuple(m.zeros_pad.shape) == (cfg.batch_size, max(cfg.input_len, cfg.pred_len), cfg.C)
    assert set(IC.Stack(cfg).state_dict()) == set(want)
    assert [type(a).__name__ for a in m.prob_attentions()] == ["ProbAttention"] * (cfg.e_layers + 2 * cfg.d_layers)
    assert m.fused_calls == 0


def _tree_behind(root, informer_source):
    (root / "models").mkdir()
    (root / "models" / "Informer.py").write_text(informer_source)


def test_a_reference_model_behind_is_replaced_by_this_builds_class(tmp_path):
    _tree_behind(tmp_path, "import torch.nn as nn\nMARK = 'behind'\nclass Informer(nn.Module):\n    def forecasting(self, *a):\n"
                           "        return 'behind'\n")
    r = _run(f"""
        import models.Informer as M
        from models.informer_model import Informer
        assert M.__file__.startswith({str(tmp_path)!r}) and M.MARK == 'behind'      # the module stays the tree's
        assert M.Informer is Informer and 'imm-tsf_amd' in __import__('inspect').getsourcefile(M.Informer)
        print('ok')
        """, str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_anything_else_behind_under_that_name_is_left_alone(tmp_path):
    _tree_behind(tmp_path, "import torch.nn as nn\nclass Informer(nn.Module):\n    tag = 'behind'\n")
    r = _run(f"""
        import models.Informer as M
        assert M.__file__.startswith({str(tmp_path)!r}) and M.Informer.tag == 'behind' and not hasattr(M.Informer, 'forecasting')
        print('ok')
        """, str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


@pytest.mark.parametrize("fused", [True, False])
def test_cpu_tensors_are_refused(fused, monkeypatch):
    from immtsf import config
    from immtsf._lib import ImmtsfError
    from models.Informer import Informer
    monkeypatch.setattr(config, "informer_model_fused", fused)
    m = Informer(IC.config(IC.FIXTURES["model_informer"]))
    z, _, _, _ = IC.golden("model_informer")
    with pytest.raises(ImmtsfError):
        m.forecasting(*(torch.from_numpy(z[k]) for k in ("tpp", "data", "tp", "mask")))
    assert m.fused_calls == 0


def test_limits_of_the_fused_stages():
    from immtsf import ops
    for dims in ((96, 24, 7, 512), (512, 512, 32, 1024), (2, 1, 1, 4)):
        assert ops.informer_model_supported(*dims), dims
    for dims in ((96, 24, 7, 516), (96, 24, 7, 1028), (96, 24, 7, 66), (513, 24, 7, 64), (96, 513, 7, 64), (96, 24, 33, 64), (96, 24, 0, 64)):
        assert not ops.informer_model_supported(*dims), dims
