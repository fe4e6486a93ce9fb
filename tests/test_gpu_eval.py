"""GPU tests of the evaluation engine: the fused metric kernel (immtsf_eval_metrics_accum), the Q half of MMF_XAttn_Add with the
metric sums in one launch (immtsf_mmf_xrank_q_eval), and immtsf.EvalStep (replayed forward graph) against today's eager
lib.evaluation.evaluation().

Yardsticks.  Metrics: |got - ref| <= 1e-5 max(1, |ref|), the project's bar for evaluation().  Raw [5, C] sums: against float64 sums of
the same fp32 inputs, each within 1e-6 of the sum of the ABSOLUTE values of its terms -- the ape terms carry signs and may cancel, so
the sum itself is the wrong yardstick; fp32 rounding enters once per element (a few roundings of relative size 6e-8), the accumulation
is fp64."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_eval_golden import KEYS, close, golden_batches, sums_f64  # noqa: E402


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _check_sums(acc, ref, ref_abs, what):
    got = acc.detach().cpu().numpy()
    err = np.abs(got - ref)
    bound = 1e-6 * ref_abs
    print(what, "worst |got - ref| / sum|terms| per statistic:", [float(np.max(err[k] / np.maximum(ref_abs[k], 1e-300))) for k in range(5)])
    assert np.all(err <= bound), (what, got, ref)
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4]), what       # counts are exact


def test_metric_kernel_matches_the_reference_values():
    dev = _dev()
    from immtsf.evalstep import finish_metrics
    from immtsf.ops import eval_metrics_accum
    z, batches = golden_batches()
    acc = torch.zeros(5, 7, dtype=torch.float64, device=dev)
    ref = ref_abs = 0
    for t, m, p in batches:
        eval_metrics_accum(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(m).to(dev), acc)
        s, a = sums_f64(t, m, p)
        ref, ref_abs = ref + s, ref_abs + a
    _check_sums(acc, ref, ref_abs, "fixture")
    got = finish_metrics(acc.cpu())
    for k in KEYS:
        print(k, got[k], float(z[f"ref_{k}"]))
        assert close(got[k], float(z[f"ref_{k}"])), (k, got[k], float(z[f"ref_{k}"]))
    assert got["mape"] < 0


@pytest.mark.parametrize("C", [1, 7, 16, 33])
@pytest.mark.parametrize("rows", [1, 3, 4097])
def test_metric_kernel_shapes_off_the_fast_path(rows, C):
    dev = _dev()
    from immtsf.ops import eval_metrics_accum
    rng = np.random.default_rng(rows * 100 + C)
    t = rng.normal(size=(rows, C)).astype(np.float32)
    t[rng.random((rows, C)) < 0.1] = 0.0
    m = (rng.random((rows, C)) < 0.6).astype(np.float32)
    p = (t + 0.5 * rng.normal(size=(rows, C))).astype(np.float32)
    ref, ref_abs = sums_f64(t, m, p)
    td, md = torch.from_numpy(t).to(dev), torch.from_numpy(m).to(dev)
    acc = torch.zeros(5, C, dtype=torch.float64, device=dev)
    eval_metrics_accum(torch.from_numpy(p).to(dev), td, md, acc)
    _check_sums(acc, ref, ref_abs, f"aligned rows={rows} C={C}")
    # a contiguous view that starts one float into its buffer: no 16-byte loads
    buf = torch.zeros(rows * C + 1, device=dev)
    buf[1:] = torch.from_numpy(p).to(dev).reshape(-1)
    pv = buf[1:].view(rows, C)
    assert pv.data_ptr() % 16 != 0 and pv.is_contiguous()
    acc2 = torch.zeros(5, C, dtype=torch.float64, device=dev)
    eval_metrics_accum(pv, td, md, acc2)
    _check_sums(acc2, ref, ref_abs, f"unaligned rows={rows} C={C}")
    # accumulation: a second call ADDS
    eval_metrics_accum(pv, td, md, acc2)
    _check_sums(acc2, 2 * ref, 2 * ref_abs, f"twice rows={rows} C={C}")


def test_metric_kernel_wide_and_empty():
    dev = _dev()
    from immtsf.ops import eval_metrics_accum
    rng = np.random.default_rng(5)
    for rows, C in ((37, 300), (9, 1024)):            # beyond the unit walk: the column-per-thread form / the widest vector form
        t = rng.normal(size=(rows, C)).astype(np.float32)
        m = (rng.random((rows, C)) < 0.6).astype(np.float32)
        p = (t + 0.5 * rng.normal(size=(rows, C))).astype(np.float32)
        ref, ref_abs = sums_f64(t, m, p)
        buf = torch.zeros(rows * C + 1, device=dev)
        buf[1:] = torch.from_numpy(p).to(dev).reshape(-1)
        for pred in (torch.from_numpy(p).to(dev), buf[1:].view(rows, C)):
            acc = torch.zeros(5, C, dtype=torch.float64, device=dev)
            eval_metrics_accum(pred, torch.from_numpy(t).to(dev), torch.from_numpy(m).to(dev), acc)
            _check_sums(acc, ref, ref_abs, f"wide rows={rows} C={C}")
    acc = torch.full((5, 7), 2.0, dtype=torch.float64, device=dev)
    e = torch.zeros(0, 4, 7, device=dev)
    eval_metrics_accum(e, e, e, acc)                   # rows == 0: no launch, nothing changes
    assert torch.equal(acc, torch.full_like(acc, 2.0))


def test_metric_kernel_is_deterministic():
    dev = _dev()
    from immtsf.ops import eval_metrics_accum
    torch.manual_seed(3)
    batches = []
    for rows, C in ((4097, 7), (640, 7), (33, 7)):
        t = torch.randn(rows, C, device=dev)
        batches.append((t + 0.3 * torch.randn(rows, C, device=dev), t, (torch.rand(rows, C, device=dev) < 0.7).float()))
    accs = []
    for _ in range(2):
        acc = torch.zeros(5, 7, dtype=torch.float64, device=dev)
        for p, t, m in batches:
            eval_metrics_accum(p, t, m, acc)
        accs.append(acc)
    torch.cuda.synchronize()
    assert torch.equal(accs[0], accs[1])


@pytest.mark.parametrize("H", [1, 2, 4])
def test_q_eval_equals_q_forward_plus_metric_kernel(H):
    """immtsf_mmf_xrank_q_eval against immtsf_mmf_xrank_q_forward + immtsf_eval_metrics_accum on the same inputs (cfg2 dimensions)"""
    dev = _dev()
    from fusions.MMF_XAttn_Add import MMF_XAttn_Add
    from immtsf import config
    from immtsf.ops import MMFXRankQFn, eval_metrics_accum, mmf_xrank_q_eval
    config.precision = "fp32"
    B, T, Cc, d = 64, 32, 8, 768
    torch.manual_seed(40 + H)
    mmf = MMF_XAttn_Add(d, Cc, d, n_heads_fusion=H, dropout=0.1, kappa=0.5).to(dev).eval()
    Y, E = torch.randn(B, T, Cc, device=dev), torch.randn(B, T, d, device=dev)
    M = torch.ones(B, dtype=torch.bool, device=dev)
    M[3] = False                                       # a window without text
    M_u8 = M.view(torch.uint8)
    truth = torch.randn(B, T, Cc, device=dev)
    truth[torch.rand(B, T, Cc, device=dev) < 0.1] = 0.0
    mask = (torch.rand(B, T, Cc, device=dev) < 0.7).float()
    with torch.no_grad():
        assert mmf._rank(T)
        P, bHO = mmf.project_kv(E)
        p = mmf._params()
        out = MMFXRankQFn.apply(Y, P, bHO, M_u8, d, H, 0.5, 0.1, False, 0, 0, p[9], p[10])
        a_ref = torch.zeros(5, Cc, dtype=torch.float64, device=dev)
        eval_metrics_accum(out, truth, mask, a_ref)
        a1 = torch.zeros(5, Cc, dtype=torch.float64, device=dev)
        out1 = mmf_xrank_q_eval(Y, P, bHO, M_u8, truth, mask, a1, d, H, 0.5, 0, p[9], p[10], want_out=True)
        a2 = torch.zeros(5, Cc, dtype=torch.float64, device=dev)
        assert mmf_xrank_q_eval(Y, P, bHO, M_u8, truth, mask, a2, d, H, 0.5, 0, p[9], p[10]) is None      # Y_out = NULL
        a3 = torch.zeros(5, Cc, dtype=torch.float64, device=dev)
        mmf.forward_metrics(Y, E, M.view(B, 1), truth, mask, a3)
    torch.cuda.synchronize()
    assert torch.equal(out1, out)
    assert float((out[3] - Y[3] / 1.5).abs().max()) <= 1e-6      # the quirk kept: no text -> Y_ts / (1 + kappa)
    _, ref_abs = sums_f64(truth.cpu().numpy(), mask.cpu().numpy(), out.cpu().numpy())
    ref = a_ref.cpu().numpy()
    for a, what in ((a1, "with Y_out"), (a2, "Y_out = NULL"), (a3, "forward_metrics")):
        _check_sums(a, ref, ref_abs, f"q_eval H={H} {what}")
    assert torch.equal(a1, a2)
    mmf.train()
    with pytest.raises(RuntimeError):
        mmf.forward_metrics(Y, E, M.view(B, 1), truth, mask, a3)


def _setup(dev, ttf, mmf):
    import bench
    from fusions.FusionModel import FusionModel
    from fusions.load_llm import register_d_model
    from immtsf import config
    from models.tPatchGNN import tPatchGNN
    register_d_model("TOY48", 48)
    config.precision = "fp32"
    config.nan_check = "deferred"
    config.manual_seed(77)
    torch.manual_seed(0)
    a = types.SimpleNamespace(
        device=str(dev), hid_dim=16, C=bench.C, npatch=bench.M_PATCH, nlayer=1, te_dim=6, n_heads=1, tf_layer=1, node_dim=5,
        hop=1, outlayer="Linear", TTF_module=ttf, MMF_module=mmf, llm_model_fusion="TOY48",
        llm_layers_fusion=6, max_length=1024, use_text_embeddings=True, recency_sigma=1.0, n_heads_fusion=2,
        dropout=0.1, d_txt=32, kappa=0.5, batch_size=8)
    model = tPatchGNN(a).to(dev).eval()
    fusion = FusionModel(a).to(dev).eval()
    batches = []
    for seed in (11, 12, 13):            # the batches of tests/test_gpu_train.py::test_evaluation_metrics_match_reference_formula
        cpu_batch, _ = bench.synth_batch(seed, 8)
        b = {k: v.to(dev) for k, v in cpu_batch.items()}
        b["notes_embeddings"] = b["notes_embeddings"][..., :48].contiguous()
        batches.append(b)
    return model, fusion, batches


@pytest.mark.parametrize("ttf,mmf,text", [("TTF_T2V_XAttn", "MMF_XAttn_Add", True), ("TTF_RecAvg", "MMF_GR_Add", True),
                                          ("TTF_T2V_XAttn", "MMF_XAttn_Add", False)])
def test_evalstep_equals_eager_evaluation(ttf, mmf, text, monkeypatch):
    dev = _dev()
    import immtsf
    from immtsf import config
    from lib.evaluation import evaluation
    model, fusion, batches = _setup(dev, ttf, mmf)
    assert getattr(model, "immtsf_graphable", False)
    fus = fusion if text else None
    assert config.eval_engine is False
    ref = evaluation(model, fus, batches, enable_text=text)
    ev = immtsf.EvalStep(model, fus, enable_text=text)
    with pytest.raises(ValueError, match="empty dataloader"):
        ev.result()
    # which metric kernel serves the case: count the calls of the two wrappers (a quiet fall-back must not pass unseen)
    import fusions.MMF_XAttn_Add as xadd_mod
    from immtsf import ops
    calls = {"fused": 0, "standalone": 0}

    def counted(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f
    monkeypatch.setattr(xadd_mod, "mmf_xrank_q_eval", counted("fused", xadd_mod.mmf_xrank_q_eval))
    monkeypatch.setattr(xadd_mod, "eval_metrics_accum", counted("standalone", xadd_mod.eval_metrics_accum))
    monkeypatch.setattr(ops, "eval_metrics_accum", counted("standalone", ops.eval_metrics_accum))
    fused = text and mmf == "MMF_XAttn_Add"
    if fused:
        assert fusion.mmf._rank(batches[0]["tp_to_predict"].shape[1])      # the low-rank form takes these dimensions
    for b in batches:
        ev(b)
    first = ev.result()
    # per batch of the first pass one call: eager (1) + the graph's warm-up and capture (2) + nothing for the replays
    assert calls == ({"fused": 3, "standalone": 0} if fused else {"fused": 0, "standalone": 3}), calls
    # the three batches have ONE shape: eager at its first sighting, captured at the second, replayed from then on
    assert (ev.eager, ev.replays, ev.captures) == (1, 2, 1)
    ev.reset()
    for b in batches:
        ev(b)
    second = ev.result()
    assert (ev.eager, ev.replays, ev.captures) == (1, 5, 1) and ev.batches == 3      # the second feeding: replays only
    ev.reset()
    for b in batches:
        ev(b)
    third = ev.result()
    for got in (first, second, third):
        assert set(got) == set(KEYS) and all(isinstance(v, float) for v in got.values())
        for k in KEYS:
            print(ttf, mmf, text, k, got[k], ref[k])
            assert close(got[k], ref[k]), (k, got[k], ref[k])
    assert (ev.eager, ev.replays, ev.captures) == (1, 8, 1)


def test_evalstep_counts_replays_per_shape():
    """each batch fed twice: the second feeding of a shape is a graph replay"""
    dev = _dev()
    import immtsf
    from lib.evaluation import evaluation
    model, fusion, batches = _setup(dev, "TTF_T2V_XAttn", "MMF_XAttn_Add")
    batches[1] = {k: v[:5].contiguous() for k, v in batches[1].items()}        # a second shape
    ref = evaluation(model, fusion, batches)
    ev = immtsf.EvalStep(model, fusion)
    for b in (batches[0], batches[1]):
        ev(b)
    assert (ev.eager, ev.replays) == (2, 0)
    ev.reset()
    for b in batches:
        ev(b)
    assert (ev.eager, ev.replays, ev.captures) == (2, 3, 2)
    got = ev.result()
    for k in KEYS:
        assert close(got[k], ref[k]), (k, got[k], ref[k])
    nog = immtsf.EvalStep(model, fusion, graph=False)
    for _ in range(2):
        nog.reset()
        for b in batches:
            nog(b)
    assert nog.replays == 0 and nog.eager == 6
    res = nog.result()
    for k in KEYS:
        assert close(res[k], got[k]), (k, res[k], got[k])


def test_evaluation_opt_in_branch():
    dev = _dev()
    from immtsf import config
    from immtsf.evalstep import EvalStep
    from lib.evaluation import _eval_steps, evaluation
    model, fusion, batches = _setup(dev, "TTF_T2V_XAttn", "MMF_XAttn_Add")
    n0 = EvalStep.instances
    off = evaluation(model, fusion, batches)
    assert EvalStep.instances == n0 and model not in _eval_steps       # the default path builds no engine
    try:
        config.eval_engine = True
        on = evaluation(model, fusion, batches)
        again = evaluation(model, fusion, batches)
        assert EvalStep.instances == n0 + 1                            # one engine per (model, fusion), kept
        assert next(iter(_eval_steps[model].values())).replays >= 3
        with pytest.raises(ValueError, match="empty dataloader"):
            evaluation(model, fusion, [])
        cpu = [{k: v.cpu() for k, v in batches[0].items()}]            # CPU batches are not the engine's: the eager path answers
        with pytest.raises(RuntimeError):                              # (immtsf ops refuse CPU tensors: ImmtsfError is a RuntimeError)
            evaluation(model, fusion, cpu)
        assert EvalStep.instances == n0 + 1
    finally:
        config.eval_engine = False
    for k in KEYS:
        assert close(on[k], off[k]) and close(again[k], off[k]), (k, on[k], again[k], off[k])


def test_evalstep_refuses_training_mode():
    dev = _dev()
    import immtsf
    model, fusion, batches = _setup(dev, "TTF_T2V_XAttn", "MMF_XAttn_Add")
    ev = immtsf.EvalStep(model, fusion)
    model.train()
    with pytest.raises(RuntimeError):
        ev(batches[0])
    model.eval()
    fusion.train()
    with pytest.raises(RuntimeError):
        ev(batches[0])
    fusion.eval()
    ev(batches[0])
    assert ev.batches == 1
