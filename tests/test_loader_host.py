"""Host side of the resident loaders (no GPU): the split function of lib.resident_datasets against the index lists the REAL
reference produced (tests/golden/loader_meta.npz), ResidentLoader's epoch order against a live torch DataLoader, and what
lib.parse_datasets is, exposes and refuses with and without a reference tree behind this one."""
import argparse
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "imm-tsf_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _meta():
    return np.load(os.path.join(GOLDEN, "loader_meta.npz"))


@pytest.mark.parametrize("method", ["sample", "instance"])
def test_split_indices_match_the_reference(method):
    from lib.parse_datasets import split_indices
    z = _meta()
    got = split_indices([str(c) for c in z["chunk_ids"]], method)
    for split, idx in zip(("train", "val", "test"), got):
        assert list(idx) == z[f"{method}.{split}_idx"].tolist(), (method, split)


def test_split_fixture_holds_the_empty_validation_slice():
    """ent05 has one window: int(1 * 0.6) == int(1 * 0.8), so the sample split gives it no train and no validation window"""
    from lib.parse_datasets import split_indices
    ids = [str(c) for c in _meta()["chunk_ids"]]
    lone = [i for i, c in enumerate(ids) if c.startswith("ent05_")]
    train, val, test = split_indices(ids, "sample")
    assert len(lone) == 1 and lone[0] in test and lone[0] not in train and lone[0] not in val
    assert any(c == "ent02_chunk6" for c in ids) and "ent02_chunk5" not in ids      # the dropped window used up number 5


def test_split_unknown_method_raises():
    from lib.parse_datasets import split_indices
    with pytest.raises(ValueError, match="Unknown split_method: 'random'"):
        split_indices(["a_chunk0", "a_chunk1"], "random")


def _stub_loader(n, batch_size, shuffle, generator=None):
    from immtsf.data import ResidentLoader
    return ResidentLoader(types.SimpleNamespace(W=100), np.arange(n) + 50, batch_size, shuffle, generator=generator)


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("batch_size", [1, 4])
@pytest.mark.parametrize("n", [1, 4, 9])
def test_epoch_order_and_rng_state_match_a_live_dataloader(n, batch_size, shuffle):
    from torch.utils.data import DataLoader
    torch.manual_seed(1234 + n)
    live = DataLoader(list(range(n)), batch_size=batch_size, shuffle=shuffle)
    want = [[int(i) for b in live for i in b] for _ in range(2)]
    want_state = torch.get_rng_state()
    torch.manual_seed(1234 + n)
    dl = _stub_loader(n, batch_size, shuffle)
    got = [dl._epoch_order().tolist() for _ in range(2)]
    assert got == want
    assert torch.equal(torch.get_rng_state(), want_state)
    assert len(dl) == len(live) and len(dl.dataset) == n
    if shuffle and n == 9:
        assert got[0] != got[1] and sorted(got[0]) == list(range(9))


def test_epoch_order_follows_a_private_generator():
    from torch.utils.data import DataLoader
    live = DataLoader(list(range(9)), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(3)
    before = torch.get_rng_state()
    assert _stub_loader(9, 4, True, generator=g)._epoch_order().tolist() == [int(i) for b in live for i in b]
    assert torch.equal(torch.get_rng_state(), before)           # the global generator was not touched


def test_loader_argument_errors():
    with pytest.raises(ValueError):
        _stub_loader(4, 0, False)
    from immtsf.data import ResidentLoader
    st = types.SimpleNamespace(W=3)
    with pytest.raises(IndexError):
        ResidentLoader(st, [0, 3], 2, False)
    with pytest.raises(ValueError):
        ResidentLoader(st, [0, 1], 2, False, form="patch")
    with pytest.raises(ValueError):
        ResidentLoader(st, [0, 1], 2, False, form="cru", patch=(8, 3, 8))


def _run(code, extra_path, **env):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, extra_path]), **env)
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True, text=True, timeout=300)


def test_parse_datasets_without_a_reference_tree():
    """lib.parse_datasets is then lib.resident_datasets itself; raw-text mode and a CPU device have nowhere to go and say so"""
    import lib.parse_datasets as p
    import lib.resident_datasets as r
    assert p is r and os.path.samefile(p.__file__, os.path.join(PKG, "lib", "resident_datasets.py"))
    assert "imm-tsf_amd" in p.parse_datasets.__code__.co_filename and "imm-tsf_amd" in p.get_input_and_pred_len.__code__.co_filename
    assert p._reference() is None           # the test session has no reference tree on its path
    for name in ("variable_time_collate_fn", "patch_variable_time_collate_fn", "variable_time_collate_fn_CRU", "variable_time_collate_fn_ODE"):
        assert not hasattr(p, name)
    raw = argparse.Namespace(enable_text=True, use_text_embeddings=False, device="cuda")
    with pytest.raises(NotImplementedError, match="raw-text mode"):
        p.parse_datasets(raw)
    cpu = argparse.Namespace(enable_text=True, use_text_embeddings=True, device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="device cpu"):
        p.parse_datasets(cpu)
    with pytest.raises(NotImplementedError):
        p.get_input_and_pred_len({"train_dataloader": [], "val_dataloader": []})


def test_parse_datasets_in_front_of_a_reference_tree(tmp_path):
    """with a tree of the reference's layout behind this one: lib.parse_datasets is the module behind, `from lib.parse_datasets import
    ...` (main.py's line) gets the two entry points defined here, the collate names are that module's own, and what the resident path
    does not cover -- raw text, a CPU device, IMMTSF_RESIDENT_LOADER=0 -- is handed to that module's own entry points"""
    (tmp_path / "lib").mkdir()
    (tmp_path / "lib" / "parse_datasets.py").write_text(textwrap.dedent("""
        def parse_datasets(args, show_summary=True):
            return ("behind", show_summary)
        def get_input_and_pred_len(data_obj):
            return ("behind", len(data_obj))
        def variable_time_collate_fn(): pass
        def patch_variable_time_collate_fn(): pass
        def variable_time_collate_fn_CRU(): pass
        def variable_time_collate_fn_ODE(): pass
        def show_ds_summary(args): pass
        """))
    code = """
        import argparse, os
        from lib.parse_datasets import parse_datasets, get_input_and_pred_len
        import lib.parse_datasets as p
        from immtsf import config
        assert p.__file__.startswith(BEHIND)
        for fn in (parse_datasets, get_input_and_pred_len, p.split_indices):
            assert 'imm-tsf_amd' in fn.__code__.co_filename, fn
        for name in ('variable_time_collate_fn', 'patch_variable_time_collate_fn', 'variable_time_collate_fn_CRU',
                     'variable_time_collate_fn_ODE', 'show_ds_summary'):
            assert getattr(p, name).__code__.co_filename.startswith(BEHIND), name
        raw = argparse.Namespace(enable_text=True, use_text_embeddings=False, device='cuda')
        cpu = argparse.Namespace(enable_text=True, use_text_embeddings=True, device='cpu')
        gpu = argparse.Namespace(enable_text=True, use_text_embeddings=True, device='cuda:0')
        assert parse_datasets(raw) == ('behind', True) and parse_datasets(cpu, False) == ('behind', False)
        assert get_input_and_pred_len({'train_dataloader': [], 'val_dataloader': []}) == ('behind', 2)
        assert config.resident_loader == (os.environ.get('IMMTSF_RESIDENT_LOADER') != '0')
        if not config.resident_loader:
            assert parse_datasets(gpu) == ('behind', True)
        print('ok')
        """.replace("BEHIND", repr(str(tmp_path)))
    for env in ({}, {"IMMTSF_RESIDENT_LOADER": "0"}):
        r = _run(code, str(tmp_path), **env)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
