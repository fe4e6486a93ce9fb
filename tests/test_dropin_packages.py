"""The mirrored packages must coexist with a reference tree placed AFTER them on sys.path: modules this build does not
mirror keep resolving to the reference, and mirrored modules re-export the reference names they do not define
(immtsf/dropin.py).  Run in subprocesses so sys.path / sys.modules of the test session stay untouched."""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imm-tsf_amd")


def _run(code, extra_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, extra_path]))
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)


def test_unmirrored_modules_and_names_resolve_to_the_tree_behind(tmp_path):
    for pkg in ("lib", "layers", "models", "fusions"):
        (tmp_path / pkg).mkdir()
    (tmp_path / "lib" / "utils.py").write_text("def where():\n    return 'behind'\n")
    (tmp_path / "lib" / "evaluation.py").write_text("def evaluation(*a):\n    return 'behind'\ndef only_behind():\n    return 7\n")
    (tmp_path / "layers" / "Embed.py").write_text("class DataEmbedding_wo_pos:\n    pass\nclass PatchEmbedding:\n    tag = 'behind'\n")
    (tmp_path / "models" / "Informer.py").write_text("from layers.Embed import DataEmbedding_wo_pos, PatchEmbedding\nclass Informer:\n    emb = PatchEmbedding\n")
    r = _run("""
        import lib.utils, lib.evaluation, layers.Embed, models.Informer, models.tPatchGNN, fusions.load_llm
        assert lib.utils.where() == 'behind'
        assert lib.evaluation.only_behind() == 7                       # re-exported
        assert lib.evaluation.evaluation.__module__ == 'lib.evaluation' and 'dropin' not in lib.evaluation.__file__
        assert lib.evaluation.evaluation.__doc__ and 'device' in lib.evaluation.evaluation.__doc__     # ours wins
        assert layers.Embed.DataEmbedding_wo_pos.__module__.endswith('_shadowed_Embed')
        assert getattr(layers.Embed.PatchEmbedding, 'tag', None) is None  # ours wins
        assert models.Informer.Informer.emb is layers.Embed.PatchEmbedding
        assert fusions.load_llm.get_context_window_size('GPT2') == 1024 and fusions.load_llm.get_d_model('Llama') == 4096
        print('ok')
        """, str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_standalone_import_without_any_reference_tree():
    r = _run("""
        import fusions.FusionModel, layers.Embed, layers.SelfAttention_Family, models.PatchTST, lib.evaluation
        print('ok')
        """, "")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def _reference_standin(root):
    """a stand-in of the reference tree under `root`: every module its packages hold, each defining the public names the reference's
    module defines as placeholder classes (tests/golden/reference_layout.json, written by tests/golden/make_golden_layout.py)"""
    with open(os.path.join(ROOT, "tests", "golden", "reference_layout.json")) as fh:
        layout = json.load(fh)
    for pkg, modules in layout.items():
        (root / pkg).mkdir(parents=True)
        for mod, names in modules.items():
            (root / pkg / f"{mod}.py").write_text("".join(f"{n} = type({n!r}, (), {{'__module__': __name__}})\n" for n in names))
    return layout


def test_reference_main_imports_resolve_with_this_tree_in_front(tmp_path):
    """the import block of the reference's main.py (lines 16-40) with this tree in front of a stand-in of the reference's; and every
    public name of a reference module this build mirrors resolves on the mirrored module (defined here or re-exported)"""
    behind = tmp_path / "reference"
    layout = _reference_standin(behind)
    mirrored = sorted(f"{pkg}.{mod}" for pkg, modules in layout.items() for mod in modules
                      if mod != "__init__" and os.path.isfile(os.path.join(PKG, pkg, f"{mod}.py")))
    assert "models.tPatchGNN" in mirrored and "lib.evaluation" in mirrored and "layers.Embed" in mirrored
    r = _run(f"""
        import importlib, json
        import lib.utils as utils
        from lib.evaluation import compute_all_losses, evaluation
        from lib.parse_datasets import parse_datasets
        from models.tPatchGNN import tPatchGNN
        from models.TimesNet import TimesNet
        from models.DLinear import DLinear
        from models.PatchTST import PatchTST
        from fusions.FusionModel import FusionModel
        from fusions.load_llm import get_context_window_size
        import models.tPatchGNN as m, lib.parse_datasets as p, fusions.FusionModel as f
        assert 'imm-tsf_amd' in m.__file__ and 'imm-tsf_amd' in f.__file__ and {str(behind)!r} in p.__file__
        assert 'imm-tsf_amd' in evaluation.__code__.co_filename
        layout = json.load(open({os.path.join(ROOT, "tests", "golden", "reference_layout.json")!r}))
        for name in {mirrored!r}:
            mod = importlib.import_module(name)
            assert 'imm-tsf_amd' in mod.__file__, name
            pkg, leaf = name.split('.')
            missing = [n for n in layout[pkg][leaf] if not hasattr(mod, n)]
            assert not missing, (name, missing)
        print('ok')
        """, str(behind))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
