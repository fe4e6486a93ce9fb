"""bench.py --dump-outputs on the CPU: bench.dump_outputs replays one step of the timed path from the state before the warm-up and
writes its loss and the updated state (parameters, Adam moments) in the modules' named-parameter order, whatever the trainer's bucket
layout -- the same files however long the timed region trained; a larger state as one seeded sample of positions."""
import os
import types

import numpy as np
import torch

import bench
from immtsf.train import FlatTrainer


def _workload():
    """a two-module workload on a CPU FlatTrainer, its eager step, and the trainer's state before any step"""
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))
    fusion = torch.nn.Linear(2, 7)
    # buckets in an order unlike the modules': the dump must not follow the flat buffer
    tr = FlatTrainer([list(fusion.parameters()), list(model.parameters())], lr=1e-2)
    x = torch.randn(4, 5)

    def step():
        tr.zero_grad()
        loss = fusion(model(x)).square().mean()
        loss.backward()
        tr.sync_grads()
        tr.step()
        return loss.detach()
    return types.SimpleNamespace(model=model, fusion=fusion, trainer=tr), step, tr.snapshot()


def _named(w, flat):
    out = []
    for mod in (w.model, w.fusion):
        for _, p in mod.named_parameters():
            off = (p.data_ptr() - w.trainer.flat_param.data_ptr()) // 4
            out.append(flat[off:off + p.numel()])
    return torch.cat(out).numpy()


def test_dump_outputs_one_step_from_the_initial_state(tmp_path):
    w, step, snap = _workload()
    first = step()                                   # what the step computes from the initial state
    want = {"params": _named(w, w.trainer.flat_param).copy(), "exp_avg": _named(w, w.trainer.exp_avg).copy(),
            "exp_avg_sq": _named(w, w.trainer.exp_avg_sq).copy()}
    for _ in range(4):                               # the rest of a "timed region": the state moves on
        step()
    flushed = []
    w.trainer._flush_cb = lambda: flushed.append(True)          # (an engine's held-back optimizer step is applied before reading)
    bench.dump_outputs(w, step, snap, str(tmp_path))
    assert flushed
    assert sorted(os.listdir(tmp_path)) == ["exp_avg.npy", "exp_avg_sq.npy", "loss.npy", "params.npy"]
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and float(loss) == float(first)
    for k, v in want.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v), k
    assert np.abs(want["exp_avg"]).sum() > 0
    # the named order: the modules' parameters as they iterate, whatever the buckets
    params = torch.cat([p.detach().reshape(-1) for m in (w.model, w.fusion) for p in m.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "params.npy"), params)


def test_dump_outputs_do_not_depend_on_the_timed_steps(tmp_path):
    w, step, snap = _workload()
    for d, n in (("a", 2), ("b", 7)):
        for _ in range(n):
            step()
        bench.dump_outputs(w, step, snap, str(tmp_path / d))
    for k in ("loss", "params", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")), k


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 16)
    w, step, snap = _workload()
    n = sum(p.numel() for m in (w.model, w.fusion) for p in m.parameters())
    for d in ("a", "b"):
        bench.dump_outputs(w, step, snap, str(tmp_path / d))
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (16,) and np.all(np.diff(idx) > 0) and idx[-1] < n
    params = torch.cat([p.detach().reshape(-1) for m in (w.model, w.fusion) for p in m.parameters()]).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "params.npy"), params[idx.astype(np.int64)])
    for k in ("sample_index", "params", "exp_avg", "exp_avg_sq", "loss"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy"))
