"""The project's captures begin with a garbage collection (immtsf.step_plan.collect_before_capture): a dead step engine in a reference
cycle still owns a torch.cuda.CUDAGraph, whose destructor synchronises the device on ROCm -- illegal, and fatal, once the collector
reaches it INSIDE the next capture.  Checked by where the dead graph goes away, never by collecting inside a capture."""
import gc
import os
import sys
import weakref

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timemixer_cases as TC  # noqa: E402


class _Engine:       # FlagStep's shape: engine -> trainer -> bound method of the engine
    def __init__(self, graph):
        self.graph = graph
        self.trainer = type("T", (), {})()
        self.trainer._flush_cb = self.flush

    def flush(self):
        pass


class _Owned:
    pass


def _no_collector(fn):
    was = gc.isenabled()
    gc.disable()        # (the collector must not take the cycle by itself)
    try:
        return fn()
    finally:
        if was:
            gc.enable()


def test_helper_frees_a_dead_engine():
    from immtsf import step_plan

    def body():
        e = _Engine(_Owned())
        dead = weakref.ref(e.graph)
        del e
        assert dead() is not None           # a cycle: reference counting alone does not free it
        step_plan.collect_before_capture()
        return dead()
    assert _no_collector(body) is None


@pytest.mark.gpu
def test_dead_graph_is_gone_when_evalstep_begins_its_capture(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import immtsf
    dev = torch.device("cuda:0")
    case = TC.CASES["e_i_defaults_no_padding"]
    m = TC.make_model(dev, case).eval()
    tpp, data, tp, mask, truth = TC.make_batch(dev, case)
    batch = {"tp_to_predict": tpp, "observed_data": data, "observed_tp": tp, "observed_mask": mask, "data_to_predict": truth,
             "mask_predicted_data": (truth > -0.5).float()}
    ev = immtsf.EvalStep(m, None)
    ev(batch)                               # first sighting: eager
    seen = []

    def body():
        buf = torch.zeros(8, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            buf.add_(1)
        g.replay()
        torch.cuda.synchronize()
        e = _Engine(g)
        dead = weakref.ref(g)
        del e, g
        assert dead() is not None

        class Spy(torch.cuda.graph):
            def __enter__(self):
                seen.append(dead() is None)
                return super().__enter__()
        monkeypatch.setattr(torch.cuda, "graph", Spy)
        ev(batch)                           # second sighting: captured
    _no_collector(body)
    assert ev.captures == 1 and seen == [True]
