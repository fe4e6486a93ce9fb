#!/usr/bin/env python3
"""bench.py -- forecast windows/sec of the multimodal-fusion training step on MI355X.

Headline workload (BASELINE.json configs[1], `--config cfg2`, the default): tPatchGNN + TTF_T2V_XAttn + MMF_XAttn_Add,
GPT-2 sized note embeddings (d_m = d_txt = 768, H = 1), a ragged batch of 64 windows (one per entity) PER GPU, bf16 MFMA
operands with fp32 accumulation, train mode with the reference's default dropout 0.1.  One step = backbone forecast ->
fusion -> masked-MSE loss -> backward -> (N>1: RCCL gradient all-reduce) -> clip_grad_norm(1.0) + Adam.  Inputs are
synthetic, generated once and resident in HBM before the timed region.  `--config cfg3|cfg4|cfg5` runs the other
BASELINE.json configurations (SURVEY 8d shapes) through the same measurement.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2] [--full] [--dump-outputs DIR]

For N>1 the driver launches one rank per GPU with torch.distributed.run; entities shard across ranks (weak scaling: 64
windows per GPU).  Rank 0 prints ONE JSON line: metric/value and `ms_per_step` of the K timed steps.  A plain run does only
that: set up, W warm-up steps, K timed steps, the line.  `--full` adds the companion measurements: `step_stats` (the step
replayed in blocks), `roofline` (dominant MFMA GEMM, timed live), `roofline_hbm` (the gather / mask path as GB/s against
8 TB/s), `sweep` (windows per GPU 64..4096), `ms_per_step_fp32` (the 1e-4 parity mode), `dropin` (the zero-edit main.py
seam: compute_all_losses + torch Adam, eager), `cpu_baseline`; `--no-roofline`, `--no-extras`, `--no-cpu-baseline` drop
single legs of it.  `--dump-outputs DIR` writes what one step of the timed path computes from the fixed inputs and initial
state (replayed after the timed region: dump_outputs) as DIR/<name>.npy.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# ---- workload constants of the headline configuration -----------------------------------------
B_PER_GPU, C, M_PATCH, L_PATCH, N_MAX, T_MAX, D_M, D_TXT, H = 64, 8, 2, 32, 32, 32, 768, 768, 1
P_DROP, KAPPA = 0.1, 0.5
PEAK_BF16_TFLOPS = 2500.0        # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_FP32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0            # HBM3E spec; ~6.3 TB/s is what a streaming copy reaches (same guide)

# BASELINE.json `configs`.  N_MAX = padded notes per window, L = history length, T = forecast steps.
CONFIGS = {
    "cfg2": dict(backbone="tPatchGNN", ttf="TTF_T2V_XAttn", mmf="MMF_XAttn_Add", llm="GPT2", d_m=768, C=8, N_MAX=32, T=32, L=32,
                 text="tPatchGNN + TTF_T2V_XAttn + MMF_XAttn_Add, GPT2 dims (d_m=d_txt=768, H=1), {B} ragged windows per GPU "
                      "(N_b~U{{1..32}}, T=32, C=8, M=2 patches, L<=32), dropout 0.1"),
    "cfg3": dict(backbone="PatchTST", ttf="TTF_T2V_XAttn", mmf="MMF_GR_Add", llm="SYN4096", d_m=4096, C=6, N_MAX=32, T=32, L=32,
                 text="PatchTST (d_model=512, d_ff=2048, 2 heads, 1 layer) + TTF_T2V_XAttn + MMF_GR_Add, LLaMA-width embeddings "
                      "(d_m=4096 -> d_txt=768), {B} ragged windows per GPU (N_b~U{{1..32}}, input_len=pred_len=32, C=6), dropout 0.1"),
    "cfg4": dict(backbone="TimesNet", ttf="TTF_RecAvg", mmf="MMF_XAttn_Add", llm="GPT2", d_m=768, C=8, N_MAX=32, T=32, L=32,
                 text="TimesNet (d_model=16, d_ff=32, top_k=5, 2 layers) + TTF_RecAvg + MMF_XAttn_Add, GPT2 dims, {B} ragged windows "
                      "per GPU (N_b~U{{1..32}}, input_len=pred_len=32, C=8), dropout 0.1; TimesNet's period selection (a host read in the "
                      "reference) stays on the device, so the step replays from a hipGraph"),
    "cfg5": dict(backbone="TimeLLM", ttf="TTF_T2V_XAttn", mmf="MMF_XAttn_Add", llm="SYN4096", d_m=4096, C=8, N_MAX=4096, T=32, L=32,
                 text="TimeLLM (random-init 6-layer GPT-2 body, offline) + TTF_T2V_XAttn + MMF_XAttn_Add, long ragged note "
                      "sequences (N_b~U{{1..4096}}, d_m=4096 -> d_txt=768), {B} windows per GPU, T=32, C=8, dropout 0.1; TimeLLM "
                      "builds its text prompts on the host like the reference, so the step is launched eagerly"),
}


def model_args(device, cfg="cfg2", batch=None):
    c = CONFIGS[cfg]
    a = types.SimpleNamespace(
        device=device, C=c["C"], TTF_module=c["ttf"], MMF_module=c["mmf"], llm_model_fusion=c["llm"], llm_layers_fusion=6,
        max_length=1024, use_text_embeddings=True, recency_sigma=1.0, n_heads_fusion=H, dropout=P_DROP, d_txt=D_TXT,
        kappa=KAPPA, batch_size=batch or B_PER_GPU)
    if c["backbone"] == "tPatchGNN":
        a.hid_dim, a.npatch, a.nlayer, a.te_dim, a.n_heads, a.tf_layer, a.node_dim, a.hop, a.outlayer = 32, M_PATCH, 1, 10, 1, 1, 10, 1, "Linear"
    elif c["backbone"] == "PatchTST":       # main.py:848-851
        a.input_len = a.pred_len = c["L"]
        a.d_model, a.d_ff, a.n_heads, a.e_layers, a.factor, a.activation, a.enc_in = 512, 2048, 2, 1, 5, "gelu", c["C"]
    elif c["backbone"] == "TimesNet":       # main.py:852-858
        a.input_len = a.pred_len = c["L"]
        a.d_model, a.d_ff, a.top_k, a.e_layers, a.num_kernels, a.enc_in, a.c_out = 16, 32, 5, 2, 6, c["C"], c["C"]
        a.embed, a.freq = "fixed", "h"
    elif c["backbone"] == "TimeLLM":
        a.input_len = a.pred_len = c["L"]
        a.use_norm, a.d_ff, a.ts_vocab_size, a.input_token_len, a.stride, a.domain_des, a.top_k = True, 32, 1000, 16, 8, "synthetic", 5
        a.llm_model_timellm, a.llm_layers_timellm, a.d_model, a.n_heads, a.immtsf_offline_llm = "GPT2", 6, 16, 8, True
    return a


def synth_batch(seed, B, cfg="cfg2", device=None):
    """SURVEY 8d synthetic ragged batch of configuration `cfg`: fp32.  CPU tensors unless `device` is given (the long
    note tensors of cfg5 -- 4 GB -- are drawn on the GPU directly).  Returns (batch dict, total number of notes)."""
    c = CONFIGS[cfg]
    Cc, NM, Tm, d_m = c["C"], c["N_MAX"], c["T"], c["d_m"]
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = {}
    if c["backbone"] == "tPatchGNN":
        # history, patched (B, M, L, C): ragged observation counts, 30 % empty patches
        cnt = rng.integers(1, L_PATCH + 1, size=(B, M_PATCH, Cc))
        cnt[rng.random((B, M_PATCH, Cc)) < 0.3] = 0
        l_idx = np.arange(L_PATCH).reshape(1, 1, L_PATCH, 1)
        obs_mask = torch.from_numpy((l_idx < cnt[:, :, None, :]).astype(np.float32))
        out["observed_data"] = torch.randn(B, M_PATCH, L_PATCH, Cc, generator=g) * obs_mask
        out["observed_tp"] = torch.sort(torch.rand(B, M_PATCH, L_PATCH, Cc, generator=g), dim=2).values * obs_mask
        out["observed_mask"] = obs_mask
    # notes (drawn right after the history so that the cfg2 batch is the one earlier rounds used)
    n_notes = torch.from_numpy(rng.integers(1, NM + 1, size=B))
    keep = (torch.arange(NM).view(1, -1) < n_notes.view(-1, 1))
    if device is not None and B * NM * d_m > (1 << 28):
        gg = torch.Generator(device=device).manual_seed(seed)
        notes = torch.randn(B, NM, d_m, generator=gg, device=device)
        notes.mul_(keep.to(device).unsqueeze(-1))
    else:
        notes = torch.randn(B, NM, d_m, generator=g) * keep.unsqueeze(-1)
    tau = torch.sort(torch.rand(B, NM, generator=g) * 24.0, dim=1).values * keep
    # horizon
    t_len = torch.from_numpy(rng.integers(8, Tm + 1, size=B))
    tvalid = (torch.arange(Tm).view(1, -1) < t_len.view(-1, 1))
    t_hat = torch.sort(24.0 + 24.0 * torch.rand(B, Tm, generator=g), dim=1).values / 48.0 * tvalid
    truth = torch.randn(B, Tm, Cc, generator=g)
    tmask = (torch.rand(B, Tm, Cc, generator=g) < 0.7).float()
    tmask[:, 0, :] = torch.maximum(tmask[:, 0, :], (tmask.sum(1) == 0).float())     # >= 1 observation per row
    tmask = tmask * tvalid.unsqueeze(-1)
    if c["backbone"] != "tPatchGNN":
        L = c["L"]
        obs_mask = (torch.rand(B, L, Cc, generator=g) < 0.7).float()
        out["observed_data"] = torch.randn(B, L, Cc, generator=g) * obs_mask
        out["observed_tp"] = torch.sort(torch.rand(B, L, generator=g), dim=1).values * 0.5
        out["observed_mask"] = obs_mask
    out.update(tp_to_predict=t_hat, notes_embeddings=notes, tau=tau, data_to_predict=truth * tmask, mask_predicted_data=tmask)
    if device is not None:
        out = {k: v.to(device) for k, v in out.items()}
    return out, int(n_notes.sum())


def fusion_flops_per_window(sum_n, B, cfg="cfg2"):
    """SURVEY 8d algorithmic FLOPs (fwd+bwd = 3x fwd for the GEMM terms), per window."""
    c = CONFIGS[cfg]
    d, dt, T, nbar, d_m, Cc = D_TXT, D_TXT // 2, c["T"], sum_n / B, c["d_m"], c["C"]
    f_t2v = sum_n * (2 * d_m * d + 2 * (d + dt) * d + 4 * d * d) + B * T * (4 * nbar * d + 2 * d * d) + B * T * 2 * d * d
    f_rec = sum_n * 2 * d_m * d + B * T * (2 * nbar * d + 2 * d * d)
    f_xadd = B * T * (12 * d * d + 4 * T * d + 4 * Cc * d)
    f_gr = B * T * (8 * Cc * (Cc + d) + 8 * Cc * Cc)
    f = (f_t2v if c["ttf"] == "TTF_T2V_XAttn" else f_rec) + (f_xadd if c["mmf"] == "MMF_XAttn_Add" else f_gr)
    return 3.0 * f / B


def fusion_executed_flops_per_window(sum_n, B, cfg="cfg2"):
    """What the build EXECUTES for the same function: MMF_XAttn_Add runs in its low-rank form (csrc/xrank.hip: the text side projected
    onto (2C+1) H columns, the T x T attention on those), so its 12 d^2 term becomes 2 pw d + a few hundred FMAs per row; TTF and
    MMF_GR_Add as in the algorithmic count.  Reported next to the algorithmic figure so that nobody reads the latter as MFMA work."""
    c = CONFIGS[cfg]
    d, dt, T, nbar, d_m, Cc = D_TXT, D_TXT // 2, c["T"], sum_n / B, c["d_m"], c["C"]
    f_t2v = sum_n * (2 * d_m * d + 2 * (d + dt) * d + 4 * d * d) + B * T * (4 * nbar * d + 2 * d * d) + B * T * 2 * d * d
    f_rec = sum_n * 2 * d_m * d + B * T * (2 * nbar * d + 2 * d * d)
    pw = (2 * Cc + 1 + 7) // 8 * 8
    f_xadd = B * T * (2 * pw * d + 2 * T * (2 * Cc + 1))
    f_gr = B * T * (8 * Cc * (Cc + d) + 8 * Cc * Cc)
    f = (f_t2v if c["ttf"] == "TTF_T2V_XAttn" else f_rec) + (f_xadd if c["mmf"] == "MMF_XAttn_Add" else f_gr)
    return 3.0 * f / B


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(batch, warmup=3, steps=10, budget_s=45.0):
    """SURVEY 8d protocol: the oracle (CPU restatement, op-for-op incl. the T-fold K/V expansion; backbone =
    oracle/tpatchgnn_ref.py, the eager formulation pinned against the reference's goldens) timed on this box's host
    cores: same cfg2 batch, same region (backbone fwd -> fusion fwd -> masked MSE -> backward -> clip -> Adam), dropout
    masks drawn on the CPU each step like torch's dropout does; >= 3 warm-up and >= 10 timed steps, median; once with
    torch.set_num_threads(os.cpu_count()) (the protocol's number) and once with the thread count a short calibration
    finds best for this op mix.  The timed steps are cut short only if a setting would exceed `budget_s`."""
    from oracle import fusion_ref as R
    from oracle import tpatchgnn_ref as TP
    from fusions.FusionModel import FusionModel
    ncpu = os.cpu_count() or 1
    torch.manual_seed(0)
    a = model_args("cpu")
    model = TP.build(a).train()
    fus = FusionModel(a)          # parameter container only; the arithmetic below is the oracle's
    params = {k: v.detach().clone().requires_grad_(True) for k, v in fus.state_dict().items()}
    opt = torch.optim.Adam(list(model.parameters()) + list(params.values()), lr=1e-3)
    B, T = batch["tp_to_predict"].shape
    keep = 1.0 - P_DROP

    def step():
        B = batch["tp_to_predict"].shape[0]
        opt.zero_grad(set_to_none=True)
        pred = model.forecasting(batch["tp_to_predict"], batch["observed_data"], batch["observed_tp"], batch["observed_mask"])
        drop = {"ttf": {"attn": torch.bernoulli(torch.full((B, T, H, N_MAX), keep)),
                        "out": torch.bernoulli(torch.full((B, T, D_TXT), keep))},
                "mmf": {"attn": torch.bernoulli(torch.full((B, H, T, T), keep)),
                        "out": torch.bernoulli(torch.full((B, T, C), keep))}}
        out = R.fusion_forward("TTF_T2V_XAttn", "MMF_XAttn_Add", params, batch["notes_embeddings"], batch["tau"],
                               batch["tp_to_predict"], pred, H=H, kappa=KAPPA, drop=drop, p_drop=P_DROP, expand_T=True)
        loss = R.masked_mse(batch["data_to_predict"], out, batch["mask_predicted_data"])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(model.parameters()) + list(params.values()), 1.0)
        opt.step()

    def timed(nt):
        torch.set_num_threads(nt)
        t0 = time.perf_counter()
        for _ in range(warmup):
            step()
        per = (time.perf_counter() - t0) / warmup
        n = steps if per * steps <= budget_s else max(3, int(budget_s / per))
        ts = []
        for _ in range(n):
            t1 = time.perf_counter()
            step()
            ts.append(time.perf_counter() - t1)
        return float(np.median(ts)), n

    # calibration: one step per candidate thread count (ascending; stop once a setting is 3x off the best -- more threads
    # only get worse from there on this op mix)
    best = None
    for nt in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(nt)
        step()
        t0 = time.perf_counter()
        step()
        dt = time.perf_counter() - t0
        if best is None or dt < best[1]:
            best = (nt, dt)
        elif dt > 3 * best[1]:
            break
    med_best, n_best = timed(best[0])
    # the protocol's thread count, os.cpu_count(): with hundreds of hardware threads the many small ops of this step
    # oversubscribe badly (tens of seconds per step), so it is first probed on one eighth of the batch; the full
    # 3 + 10 protocol only runs if that projects to under 3 s per step, otherwise the projection is what is reported
    all_note = ""
    if best[0] == ncpu:
        med_all, n_all = med_best, n_best
    else:
        sub = {k: v[:max(1, B // 8)].contiguous() for k, v in batch.items()}
        full, batch = batch, sub
        Bs = sub["tp_to_predict"].shape[0]
        B_saved, B = B, Bs
        torch.set_num_threads(ncpu)
        step()
        t0 = time.perf_counter()
        step()
        proj = (time.perf_counter() - t0) * (B_saved / Bs)
        batch, B = full, B_saved
        if proj <= 3.0:
            med_all, n_all = timed(ncpu)
        else:
            med_all, n_all = proj, 1
            all_note = f" (projected from one step on {Bs} of the {B} windows: the full step would take ~{proj:.0f} s)"
    torch.set_num_threads(best[0])
    return {"value": round(B / med_best, 2), "unit": "windows/s", "cores": best[0], "kind": "port",
            "value_all_cores": round(B / med_all, 2), "all_cores": ncpu, "cpu_model": cpu_model_name(),
            "sample": f"{n_best} timed steps of the same {B}-window cfg2 batch after {warmup} warm-up steps, median "
                      f"{med_best*1e3:.0f} ms/step on {best[0]} torch threads (calibrated best); with torch.set_num_threads("
                      f"os.cpu_count()={ncpu}): {med_all*1e3:.0f} ms/step{all_note}; oracle/fusion_ref.py with the T-expanded K/V + "
                      f"oracle/tpatchgnn_ref.py, fp32, dropout {P_DROP}"}


def cpu_baseline_fusion(cfg, warmup=2, steps=6, budget_s=30.0):
    """cfg3 / cfg4 / cfg5: the fusion blocks' CPU restatement (oracle/fusion_ref.py, op-for-op incl. the T-expanded K/V; kind "port")
    timed on this box's host cores on the configuration's own synthetic batch, the backbone's forecast replaced by a fixed random
    Y_ts -- no CPU restatement of PatchTST / TimesNet / TimeLLM travels to the GPU box, so the region is
    fusion forward + masked MSE + backward + clip + Adam on the fusion parameters.  cfg5 is timed at B = 2 and scaled linearly (the
    expanded K/V of 64 windows of up to 4096 notes does not fit), as BASELINE.md section 3 prescribes."""
    from oracle import fusion_ref as R
    from fusions.FusionModel import FusionModel
    from fusions.load_llm import register_d_model
    register_d_model("SYN4096", 4096)
    c = CONFIGS[cfg]
    Bs = 2 if cfg == "cfg5" else B_PER_GPU
    ncpu = os.cpu_count() or 1
    nt = min(ncpu, 32)
    torch.set_num_threads(nt)
    torch.manual_seed(0)
    a = model_args("cpu", cfg, Bs)
    fus = FusionModel(a)
    params = {k: v.detach().clone().requires_grad_(True) for k, v in fus.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3)
    batch, _ = synth_batch(100, Bs, cfg)
    T, Cc, NM = c["T"], c["C"], c["N_MAX"]
    Y = torch.randn(Bs, T, Cc)
    keep = 1.0 - P_DROP

    def step():
        opt.zero_grad(set_to_none=True)
        drop = {"ttf": {"attn": torch.bernoulli(torch.full((Bs, T, H, NM), keep)), "out": torch.bernoulli(torch.full((Bs, T, D_TXT), keep))},
                "mmf": {"attn": torch.bernoulli(torch.full((Bs, H, T, T), keep)), "out": torch.bernoulli(torch.full((Bs, T, Cc), keep))}}
        out = R.fusion_forward(c["ttf"], c["mmf"], params, batch["notes_embeddings"], batch["tau"], batch["tp_to_predict"], Y, H=H,
                               kappa=KAPPA, drop=drop, p_drop=P_DROP, expand_T=True)
        loss = R.masked_mse(batch["data_to_predict"], out, batch["mask_predicted_data"])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()

    t0 = time.perf_counter()
    for _ in range(warmup):
        step()
    per = (time.perf_counter() - t0) / warmup
    n = steps if per * steps <= budget_s else max(2, int(budget_s / per))
    ts = []
    for _ in range(n):
        t1 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t1)
    med = float(np.median(ts))
    return {"value": round(Bs / med, 3), "unit": "windows/s", "cores": nt, "kind": "port", "all_cores": ncpu, "cpu_model": cpu_model_name(),
            "sample": f"{n} timed steps after {warmup} warm-up steps of the {cfg} synthetic batch at B = {Bs}"
                      f"{' (scaled linearly in B: BASELINE.md section 3)' if cfg == 'cfg5' else ''}, median {med*1e3:.0f} ms/step on {nt} "
                      f"torch threads; region: fusion forward ({c['ttf']} + {c['mmf']}, oracle/fusion_ref.py with the T-expanded K/V) + "
                      f"masked MSE + backward + clip + Adam -- the backbone is NOT in this figure (no CPU restatement of "
                      f"{c['backbone']} travels to the GPU box)"}


# ================================================================================================ workload on the GPU
class Workload:
    """one BASELINE configuration on one device: models, trainer, batch, the loss closure of a step"""

    def __init__(self, cfg, dev, windows, precision, group=None, wire="fp32", device_step=True, seed_off=0, overlap=True,
                 shard_optimizer=False, param_wire="fp32", packed_notes=False, fusion_only=False):
        from fusions.FusionModel import FusionModel
        from fusions.load_llm import register_d_model
        from immtsf import config
        from immtsf.train import FlatTrainer
        import importlib
        self.cfg, self.dev, self.B = cfg, dev, windows
        c = CONFIGS[cfg]
        register_d_model("SYN4096", 4096)
        config.precision = precision
        torch.manual_seed(0)                # identical initial weights on every rank
        a = model_args(str(dev), cfg, windows)
        self.model = getattr(importlib.import_module("models." + c["backbone"]), c["backbone"])(a).to(dev).train()
        self.fusion = FusionModel(a).to(dev).train()
        # host syncs inside the backbone (data-dependent shapes / prompt strings) rule out graph capture
        self.graphable = bool(getattr(self.model, "immtsf_graphable", False)) or fusion_only
        self.fusion_only = bool(fusion_only)
        excl = []      # tPatchGNN's time-embedding parameters: used by the patch encoder AND the decoder, both accumulate
        if c["backbone"] == "tPatchGNN":
            m = self.model
            excl = [m.te_scale.weight, m.te_scale.bias, m.te_periodic.weight, m.te_periodic.bias]
        backbone_params = [p for p in self.model.parameters() if p.requires_grad]
        # buckets = the groups whose gradients complete together.  Order in the flat buffers: MMF (+ the proj_out it folds), the
        # backbone, then TTF's backward phases with the LAST-completing ones at the end (C, then A and B, whose weight gradients FlagStep
        # moves to the parameter branch behind MMF's chain): a data-parallel FlagStep appends the ranks' guard word to the last range
        fb, fnames = self.fusion.grad_buckets(c["T"])
        ttf = [i for i, n in enumerate(fnames) if n.startswith("ttf")]
        ttf = [i for i in ttf if fnames[i] == "ttf_c"] + [i for i in ttf if fnames[i] != "ttf_c"]
        order = [i for i, n in enumerate(fnames) if not n.startswith("ttf")]
        buckets = [fb[i] for i in order] + [backbone_params] + [fb[i] for i in ttf]
        self.bucket_names = [fnames[i] for i in order] + ["backbone"] + [fnames[i] for i in ttf]
        bb = self.bucket_names.index("backbone")
        # the backbone's bucket on gradient sinks: all of tPatchGNN; of another backbone the parameters it names (PatchTST: the large
        # linear layers, whose weight gradients FlagStep moves to the parameter branch) -- the rest stays with autograd
        named = getattr(self.model, "immtsf_sink_params", None)
        keep_sink = {id(p) for p in named()} if named is not None else set()
        sinks = tuple(i for i in range(len(buckets)) if i != bb or c["backbone"] == "tPatchGNN" or keep_sink)
        not_sunk = [p for p in backbone_params if id(p) not in keep_sink] if (keep_sink and c["backbone"] != "tPatchGNN") else []
        self.trainer = FlatTrainer(buckets,
                                   lr=1e-3, weight_decay=0.0, max_norm=1.0, group=group, sink_buckets=sinks, sink_shared=excl, sink_exclude=not_sunk,
                                   overlap=True, device_step=device_step and self.graphable, grad_wire=wire,
                                   shard_optimizer=shard_optimizer, param_wire=param_wire)
        self.trainer.watch(self.model, self.fusion)
        big = c["N_MAX"] * c["d_m"] * windows > (1 << 28)
        if big:
            self.batch, self.sum_n = synth_batch(100 + seed_off, windows, cfg, device=dev)
            self.cpu_batch = None
        else:
            self.cpu_batch, self.sum_n = synth_batch(100 + seed_off, windows, cfg)
            self.batch = {k: v.to(dev) for k, v in self.cpu_batch.items()}
        self.packed = bool(packed_notes) and c["ttf"] == "TTF_T2V_XAttn"
        self.padded_notes = self.batch["notes_embeddings"]          # (the zero-padded form: hbm_roofline times its scan either way)
        if self.packed:
            # the notes as the device collate hands them over (immtsf.data.ResidentStore.collate): the embedding
            # rows stay in one resident matrix, the batch carries a row index per note and the per-window counts -- no zero-padded
            # (B, N, d_m) tensor, no |V| > 0 scan (note_mask) to re-derive the index from
            from immtsf.ops import PackedNotes
            notes = self.batch["notes_embeddings"]
            Bn, Nn, dm = notes.shape
            keep = notes.abs().sum(2) > 0
            lengths = keep.sum(1).to(torch.int32)
            rows = torch.arange(Bn * Nn, device=dev, dtype=torch.int32).view(Bn, Nn)[keep].contiguous()
            self.batch["notes_embeddings"] = PackedNotes(notes.reshape(Bn * Nn, dm).contiguous(), rows, lengths, Nn)
        self.global_cnt = self.batch["mask_predicted_data"].reshape(-1, c["C"]).sum(0)
        self.side = torch.cuda.Stream(device=dev) if overlap else None
        if self.fusion_only:
            # --fusion-only: the backbone's forecast is a fixed random tensor (a leaf that takes a gradient), so the step is the
            # fusion blocks + loss + their backward + the optimizer over the fusion's parameters -- what cfg5's 100 ms of frozen
            # GPT-2 body otherwise hides
            g = torch.Generator().manual_seed(4242 + seed_off)
            self.fixed_pred = torch.randn(windows, c["T"], c["C"], generator=g).to(dev).requires_grad_(True)

    def loss_fn(self):
        from immtsf.ops import masked_mse
        from lib.evaluation import forecast_and_fuse
        b = self.batch
        if self.fusion_only:
            self.fixed_pred.grad = None
            out = self.fusion(b["notes_embeddings"], b["tau"], b["tp_to_predict"], self.fixed_pred)
            return masked_mse(out, b["data_to_predict"], b["mask_predicted_data"], None, self.global_cnt)
        # (where the fusion's last block can run its head, the loss and their backward as one launch -- MMF_XAttn_Add's low-rank
        # form -- forecast_and_fuse returns the loss itself)
        return forecast_and_fuse(self.model, self.fusion, b, self.side, loss=(b["data_to_predict"], b["mask_predicted_data"], self.global_cnt))

    def eager_step(self):
        from immtsf.ops import backward_unit
        t = self.trainer
        t.zero_grad()
        loss = self.loss_fn()
        backward_unit(loss)
        t.sync_grads()
        t.step()
        return loss

    def flops_per_window(self):
        return fusion_flops_per_window(self.sum_n, self.B, self.cfg)

    def close(self):
        self.trainer.close()


FLAGS_MAX_WINDOWS = 4096     # FlagStep (three branches, device flags) against GraphedStep (graph edges), round 4: 256 windows 0.873 / 0.976 ms,
#                              512: 1.169 / 1.220, 1024: 1.601 / 1.688, 2048: 2.640 / 2.698, 4096: 4.638 / 4.682; beyond: not measured
FLAGS_GATE_MIN_WINDOWS = 4096    # FlagStep's scheduling hint (sched_gate), with / without: 512 windows 1.165 / 1.157, 1024: 1.626 / 1.603, 2048: 2.58 / 2.51,
#                                  3072: 3.53 / 3.55, 4096: 4.638 / 4.726


def flag_fns(w):
    """(text_fn, backbone_fn, head_fn) of a cfg2-style workload (text side | backbone | head), or None when it does not decompose"""
    from immtsf.ops import masked_mse
    fusion = w.fusion
    if w.side is None or not hasattr(fusion, "ttf") or not hasattr(fusion.mmf, "project_kv") or not w.graphable or w.fusion_only:
        return None
    b = w.batch
    fc_args = (b["tp_to_predict"], b["observed_data"], b["observed_tp"], b["observed_mask"])

    def text_fn():
        E, M, kv = fusion.text_side(b["notes_embeddings"], b["tau"], b["tp_to_predict"])
        return (E, M) + tuple(kv)

    def head_fn(pred, E, M, kv, fold):
        if hasattr(fusion.mmf, "forward_loss"):      # head + loss (+ their backward) in one launch where the block can
            return fusion.mmf.forward_loss(pred, E, M, b["data_to_predict"], b["mask_predicted_data"], w.global_cnt, kv=(kv, fold))
        out = fusion.mmf(pred, E, M, kv=(kv, fold))
        return masked_mse(out, b["data_to_predict"], b["mask_predicted_data"], None, w.global_cnt)

    return text_fn, (lambda: w.model.forecasting(*fc_args)), head_fn


def flag_step(w):
    """immtsf.train.FlagStep for a cfg2-style workload -- single process, or data parallel with the bucketed all-reduce beside the
    backward -- or None when the workload does not decompose that way or a spin timed out (on any rank) in three trial replays; the
    trial steps are undone (parameters, moments, counters restored), so the caller's first step is training step 1 either way."""
    from immtsf.train import FlagStep
    fns = flag_fns(w)
    if fns is None or w.trainer.sharded:
        return None
    names = w.bucket_names
    kw = {"sched_gate": w.B >= FLAGS_GATE_MIN_WINDOWS,
          # clip + Adam of a bucket at the head of the branch that reads its parameters first: TTF on the text side, the backbone on its
          # own branch, MMF_XAttn_Add (+ the proj_out it folds) on the parameter branch
          "adam_split": ([i for i, n in enumerate(names) if n.startswith("ttf")], [i for i, n in enumerate(names) if n == "backbone"],
                         [i for i, n in enumerate(names) if n == "mmf"]),
          "backbone_buckets": [i for i, n in enumerate(names) if n == "backbone"]}
    kw.update(json.loads(os.environ.get("IMMTSF_BENCH_FLAG_KW", "{}")))      # (A/B measurements only)
    st = FlagStep(w.trainer, *fns, **kw)
    snap = w.trainer.snapshot()
    for _ in range(3):
        st()
    if st.dist:
        st.calibrate_comm_order(3)  # (three more trial replays, traced: the collectives in the order in which the buckets really complete)
    torch.cuda.synchronize()
    try:
        st.check()                 # (a collective when the trainer has a process group: every rank takes the same branch)
        ok = True
    except Exception as e:         # noqa: BLE001
        print(f"# FlagStep rejected: {e}", file=sys.stderr)
        ok = False
    st.reset()                     # (the third trial's gradient still waits for its optimizer step: dropped with the trial)
    w.trainer.restore(snap)
    torch.cuda.synchronize()
    if not ok:
        st.clear_error()
        w.trainer._flush_cb = None
    return st if ok else None


def build_step(w, mode="auto", dist_on=False, captured_comm=False):
    """the step engine bench.py times for workload `w` -- also what tests/test_gpu_train.py::test_cfg2_step_vs_oracle runs, so that the
    oracle comparison covers the timed composition.  mode: "auto" (FlagStep up to FLAGS_MAX_WINDOWS windows per GPU where the
    workload decomposes, GraphedStep otherwise), "flags", "graphed", "phased", "eager".  Returns (step, info)."""
    from immtsf.train import GraphedStep, PhasedStep
    trainer = w.trainer
    info = {"engine": None, "flag_step_rejected": False}
    if mode == "eager" or not w.graphable:
        info["engine"] = "eager"
        return w.eager_step, info
    step = None
    if dist_on and captured_comm:
        # RCCL all-reduces captured inside graph A, bucket by bucket on the communication stream while the backward of the later
        # buckets still runs.  A failed capture leaves the HIP context unusable (seen with gloo, which cannot be captured): no fallback
        step = GraphedStep(trainer, w.loss_fn, capture_collectives=True)
        info["engine"] = "graphed+captured-comm"
        return step, info
    if mode == "phased":
        fns = flag_fns(w)
        if fns is not None:
            info["engine"] = "phased"
            return PhasedStep(trainer, *fns), info
    if mode == "flags" or (mode == "auto" and w.B <= FLAGS_MAX_WINDOWS):
        step = flag_step(w)
        if step is not None:
            info["engine"] = "flags"
            return step, info
        info["flag_step_rejected"] = flag_fns(w) is not None and not trainer.sharded
    if dist_on:
        trainer.overlap = False
    gkw = {"sched_gate": w.B >= FLAGS_GATE_MIN_WINDOWS}      # (the scheduling hint pays from 4096 windows on: 1 - 3 % slower below)
    gkw.update(json.loads(os.environ.get("IMMTSF_BENCH_GRAPH_KW", "{}")))      # (A/B measurements only)
    step = GraphedStep(trainer, w.loss_fn, **gkw)
    info["engine"] = "graphed"
    return step, info


def time_steps(step, steps, warmup, barrier):
    for _ in range(warmup):
        loss = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    host = time.perf_counter() - t0
    barrier()
    return time.perf_counter() - t0, host, loss


DUMP_MAX_ELEMS = 1 << 21     # --dump-outputs: elements per array (three float32 arrays + the float64 sample index: 42 MB, under 64 MB)


def dump_outputs(w, step, snap, out_dir):
    """--dump-outputs: what one step of the timed path computes from the benchmark's fixed inputs, as out_dir/<name>.npy.  The timed
    steps train, and a run of them is chaotic in rounding: the weight gradients are summed with atomics, in no fixed order, and Adam's
    normalised update turns those last-bit differences into visible ones within a few steps (two runs of 5 + 20 cfg2 steps: losses
    0.4 % apart; of one step: the same loss, parameters within 1e-9).  So after the timed region the engine's own step is replayed once
    more, untimed, from `snap` -- the trainer's state before the warm-up: seeded weights, zero moments, the first step's dropout and
    Adam counters -- on the same batch, and what that step hands its caller is written: `loss` (float64) and the updated state,
    `params`, `exp_avg`, `exp_avg_sq` (float32; after one step exp_avg is 0.1 x the clipped gradient), each the concatenation of the
    backbone's then the fusion's named trainable parameters (a layout independent of the flat buffers').  Arrays longer than
    DUMP_MAX_ELEMS hold the same fixed sample of positions, sorted, from a seeded generator (`sample_index`, float64).  Call on every
    rank (the step may hold collectives; a sharded optimizer gathers its moments); out_dir None: take part without writing."""
    t = w.trainer
    if hasattr(step, "reset"):
        step.reset()               # FlagStep: drop the optimizer step the last timed replay left pending (it is undone below)
    t.restore(snap)
    loss = step()
    sd = t.state_dict()            # (applies the step's held-back optimizer update; full flat moments on every rank)
    if out_dir is None:
        return
    flat = t.flat_param.detach().cpu().numpy()
    n_flat = flat.shape[0]
    owned = {id(p) for b in t.buckets for p in b}
    seen, runs = set(), []
    base = t.flat_param.data_ptr()
    for mod in (w.model, w.fusion):
        for name, p in mod.named_parameters():
            if id(p) not in owned or id(p) in seen:
                continue
            seen.add(id(p))
            off = (p.data_ptr() - base) // t.flat_param.element_size()
            if off < 0 or off + p.numel() > n_flat:
                raise RuntimeError(f"--dump-outputs: parameter {name} does not live in the trainer's flat buffer")
            runs.append(np.arange(off, off + p.numel(), dtype=np.int64))
    pos = np.concatenate(runs)
    os.makedirs(out_dir, exist_ok=True)
    if pos.shape[0] > DUMP_MAX_ELEMS:
        sel = np.sort(np.random.default_rng(0).choice(pos.shape[0], DUMP_MAX_ELEMS, replace=False))
        pos = pos[sel]
        np.save(os.path.join(out_dir, "sample_index.npy"), sel.astype(np.float64))
    np.save(os.path.join(out_dir, "loss.npy"), np.asarray(float(loss.detach().float().item()), dtype=np.float64))
    np.save(os.path.join(out_dir, "params.npy"), flat[pos].astype(np.float32))
    for k in ("exp_avg", "exp_avg_sq"):
        np.save(os.path.join(out_dir, f"{k}.npy"), sd[k].detach().cpu().numpy()[pos].astype(np.float32))


def graph_kernel_us(fn, reps=50, replays=10):
    """mean device time of one `fn()` (which enqueues kernels on the current stream): `reps` calls captured in one hipGraph,
    HIP events around replays -- launch latency excluded, the figure rocprofv3 reports as the kernels' duration"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * replays) * 1e3


def csrc_sha():
    """content hash of the kernel sources (imm-tsf_amd/csrc/*.hip, *.hpp, include/immtsf.h): a PMC profile under profiles/ counts as a
    measurement of THIS build only when it carries the same hash (tools/pmc_summary.py stamps it on the GPU box; there is no .git there)"""
    import glob
    import hashlib
    h = hashlib.sha1()
    files = sorted(glob.glob(os.path.join(ROOT, "imm-tsf_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "imm-tsf_amd", "csrc", "*.hpp")))
    for f in files + [os.path.join(ROOT, "include", "immtsf.h")]:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def gemm_roofline(w, lib, args, k2=20):
    """dominant kernel = the MFMA GEMM LAUNCH with the largest in-graph time per step.  HIP events bracket every GEMM launch on its
    launch stream over a block of eagerly launched steps (the library's timing tap; a grouped weight-gradient launch is ONE record with
    the sum of its members' flops and bytes) to find the candidates; each candidate -- the same kernel path, operand types and, for a
    grouped launch, member list -- is then re-timed as back-to-back launches inside one hipGraph (kernel time without launch latency:
    what rocprofv3 reports as the kernel's duration) and the candidates are ranked by that time x launches per step."""
    from immtsf import _lib
    dev = w.dev
    lib.immtsf_timing_enable(1)
    was_collective, w.trainer.collective = w.trainer.collective, False      # rank 0 only: no collectives in this leg
    for _ in range(k2):
        w.eager_step()
    w.trainer.collective = was_collective
    torch.cuda.synchronize()
    cap = 16384
    meta = (ctypes.c_int32 * (10 * cap))()
    ms = (ctypes.c_float * cap)()
    mem = (ctypes.c_int32 * (24 * cap))()
    n = lib.immtsf_timing_collect(cap, meta, ms, mem)
    lib.immtsf_timing_enable(0)
    groups = {}
    for i in range(n):
        groups.setdefault((tuple(meta[10 * i:10 * i + 10]), tuple(mem[24 * i:24 * i + 24])), []).append(ms[i])
    rows = []
    for (key, members), v in groups.items():
        layout, prec, Mm, Nn, Kk, nprob, nbatch, dyn, grid_threads, path = key
        if layout == 3:         # grouped TN launch: members (M, N, K, K-is-a-device-value)
            mem_l = [(members[4 * j], members[4 * j + 1], w.sum_n if members[4 * j + 3] else members[4 * j + 2]) for j in range(nprob)]
            fl = sum(2.0 * a * b_ * c for a, b_, c in mem_l)
            byts = sum(2 * c * a + 2 * c * b_ + 4 * a * b_ for a, b_, c in mem_l)
        else:
            if dyn == 1:
                Mm = w.sum_n
            elif dyn == 2:
                Kk = w.sum_n
            mem_l = None
            fl = 2.0 * Mm * Nn * Kk * nprob * max(nbatch, 1)
            byts = None
        rows.append(dict(key=key, members=mem_l, M=Mm, N=Nn, K=Kk, launches=len(v), avg_us=1e3 * float(np.mean(v)), total_ms=float(np.sum(v)),
                         flops=fl, bytes=byts))
    rows.sort(key=lambda r: -r["total_ms"])
    if os.environ.get("IMMTSF_BENCH_GEMM_TABLE"):
        for r in rows:
            k = r["key"]
            print(f"# gemm {['NT','NN','TN','TNgroup'][k[0]]} M={r['M']:6d} N={r['N']:5d} K={r['K']:6d} prob={k[5]} batch={k[6]:4d} dyn={k[7]} "
                  f"path={k[9]} launches/step={r['launches']/k2:5.1f} avg_us={r['avg_us']:7.1f} "
                  f"us/step={r['total_ms']*1e3/k2:7.1f} TF={r['flops']/(r['avg_us']*1e-6)/1e12:7.2f}", file=sys.stderr)
    gemm_ms = sum(r["total_ms"] for r in rows) / k2
    bf16 = args.precision == "bf16"

    def retime(r):
        """(launcher closure = ONE launch of the step's kind, algorithmic bytes, operand description, rocprof kernel-name prefix, keep)"""
        lay_i, Mm, Nn, Kk, nprob, nbatch, path = r["key"][0], r["M"], r["N"], r["K"], r["key"][5], max(r["key"][6], 1), r["key"][9]
        if lay_i == 3:
            ms_ = r["members"]
            As = [torch.randn(c, a, device=dev).bfloat16() for a, b_, c in ms_]
            Bs = [torch.randn(c, b_, device=dev).bfloat16() for a, b_, c in ms_]
            Cs = [torch.empty(a, b_, device=dev) for a, b_, c in ms_]
            k_ = len(ms_)
            pa = (ctypes.c_void_p * k_)(*[t.data_ptr() for t in As])
            pb = (ctypes.c_void_p * k_)(*[t.data_ptr() for t in Bs])
            pc = (ctypes.c_void_p * k_)(*[t.data_ptr() for t in Cs])
            i32 = lambda xs: (ctypes.c_int32 * k_)(*xs)      # noqa: E731
            la, lb, lc = i32([a for a, b_, c in ms_]), i32([b_ for a, b_, c in ms_]), i32([b_ for a, b_, c in ms_])
            mm, nn, kk = i32([a for a, b_, c in ms_]), i32([b_ for a, b_, c in ms_]), i32([c for a, b_, c in ms_])

            def one():
                _lib.check(lib.immtsf_gemm_bf16_group_tn(k_, pa, la, pb, lb, pc, lc, mm, nn, kk, _lib.stream_ptr()), "gemm_bf16_group_tn")
            return (one, r["bytes"], f"{k_} weight gradients of different shapes in one launch; A, B bf16 in HBM (LDS-DMA), C fp32",
                    "gemm2_group_kernel<", (As, Bs, Cs, pa, pb, pc, la, lb, lc, mm, nn, kk))
        shapes = {0: ((Mm, Kk), (Nn, Kk)), 1: ((Mm, Kk), (Kk, Nn)), 2: ((Kk, Mm), (Kk, Nn))}[lay_i]
        Ab, Bb = torch.randn(*shapes[0], device=dev), torch.randn(*shapes[1], device=dev)
        Cb = torch.empty(Mm, Nn, device=dev)
        reps = nprob * nbatch          # the batched / multi-problem forms of one launch are re-timed as that many plain launches
        if path == 2:       # bf16 operands in memory (LDS-DMA kernels: gemm2, or gemm3 for many rows): both operand images are bf16
            Ah, Bh = Ab.bfloat16(), Bb.bfloat16()

            def one():
                for _ in range(reps):
                    _lib.check(lib.immtsf_gemm_bf16(lay_i, _lib.ptr(Ah), Ah.shape[1], _lib.ptr(Bh), Bh.shape[1], _lib.ptr(Cb), Nn, None, Nn,
                                                    None, None, Mm, Nn, Kk, 1.0, 0, 0, None, 0, None, _lib.stream_ptr()), "gemm_bf16")
            return one, reps * (2 * Mm * Kk + 2 * Nn * Kk + 4 * Mm * Nn), "A, B bf16 in HBM (LDS-DMA), C fp32", "gemm", (Ah, Bh, Cb)
        twin = None
        # in the step the weight operand of a forward / data-gradient GEMM is read from FlatTrainer's bf16 twin: same here
        if bf16 and lay_i != 2 and nbatch == 1 and w.trainer.flat_twin is not None:
            twin = Bb.to(torch.bfloat16).contiguous()
            _lib.check(lib.immtsf_bf16_twin_register(_lib.ptr(Bb), _lib.ptr(twin), Bb.numel()), "bf16_twin_register")

        def one():
            for _ in range(reps):
                _lib.check(lib.immtsf_gemm(lay_i, 1 if bf16 else 0, _lib.ptr(Ab), Ab.shape[1], _lib.ptr(Bb), Bb.shape[1], _lib.ptr(Cb),
                                           Nn, None, Mm, Nn, Kk, 1.0, 0, 0, _lib.stream_ptr()), "gemm")
        return (one, reps * (4 * Mm * Kk + (2 if twin is not None else 4) * Nn * Kk + 4 * Mm * Nn),
                "A fp32, B " + ("bf16 twin of the weights" if twin is not None else "fp32") + ", C fp32", "gemm_kernel<", (Ab, Bb, Cb, twin))

    # the eager tap's durations include launch latency, which ranks tiny batched launches far too high: the candidates (the six
    # largest tap totals among the launches carrying >= 3 % of the step's GEMM flops) are re-timed inside a hipGraph and ranked by
    # kernel time x launches per step
    best = None
    step_flops = sum(r["flops"] * r["launches"] for r in rows)
    cands = [r for r in rows if r["flops"] * r["launches"] >= 0.03 * step_flops][:6]
    for r in cands:
        one, alg_bytes, operands, kname, keep = retime(r)
        us = graph_kernel_us(one, reps=20, replays=5)
        if kname == "gemm_kernel<" and keep[3] is not None:
            lib.immtsf_bf16_twin_unregister(_lib.ptr(keep[1]))
        tot = us * r["launches"] / k2
        if best is None or tot > best[0]:
            best = (tot, r, us, alg_bytes, operands, kname)
        del keep
    _, top, kernel_us, alg_bytes, operands, kname = best
    lay_i, Mm, Nn, Kk, nprob, path, grid_threads = top["key"][0], top["M"], top["N"], top["K"], top["key"][5], top["key"][9], top["key"][8]
    peak = PEAK_BF16_TFLOPS if bf16 else PEAK_FP32_TFLOPS
    ach = top["flops"] / (kernel_us * 1e-6) / 1e12
    ach_tap = top["flops"] / (top["avg_us"] * 1e-6) / 1e12
    allfl = sum(r["flops"] * r["launches"] for r in rows) / sum(r["total_ms"] for r in rows) / 1e9
    lay = {0: "NT", 1: "NN", 2: "TN", 3: "TN group"}[lay_i]
    # HBM-side traffic of that launch from a committed rocprofv3 PMC pass (counters cannot be read from inside the process) -- only
    # from a profile of THIS build: its csrc hash must equal the one of the sources this run was built from
    sha = csrc_sha()
    traffic, prov, why = None, None, "no PMC profile under profiles/ for this build"
    import glob
    for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic*.json")), reverse=True):
        try:
            pmc = json.load(open(fn))
        except Exception:      # noqa: BLE001
            continue
        if pmc.get("csrc_sha") != sha or pmc.get("windows_per_gpu", 64) != w.B or pmc.get("config", "cfg2") != w.cfg:
            continue
        tag = {0: "<false, false", 1: "<false, true", 2: "<true, true", 3: ""}[lay_i]
        for kr in pmc["kernels"]:
            nm = kr["kernel"]
            hit = (kname in nm) if lay_i == 3 else (("gemm2_kernel" + tag in nm or "gemm3_kernel" + tag in nm or "gemm_kernel<true, " + tag[1:] in nm))
            if hit and kr["grid_threads"] == grid_threads:
                traffic = kr["fetch_bytes_per_launch"] + (kr["write_bytes_per_launch"] or 0)
                prov = {"file": "profiles/" + os.path.basename(fn), "commit": pmc.get("commit"), "csrc_sha": sha, "kernel": nm[:160],
                        "fetch_bytes_per_launch": kr["fetch_bytes_per_launch"], "write_bytes_per_launch": kr["write_bytes_per_launch"],
                        "launches_profiled": kr["launches"]}
                break
        if traffic is not None:
            break
        why = f"{os.path.basename(fn)} is a profile of this build but holds no record of this launch (grid {grid_threads} threads)"
    # ... and the MFMA pipes' busy fraction of that launch from a committed SQ-counter pass of THIS build (tools/sq_pass_r05.sh)
    mfma_busy, sq_prov = None, None
    for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_sq_w*.json")), reverse=True):
        try:
            sq = json.load(open(fn))
        except Exception:      # noqa: BLE001
            continue
        if sq.get("csrc_sha") != sha or sq.get("windows_per_gpu", 64) != w.B or sq.get("config", "cfg2") != w.cfg:
            continue
        tag = {0: "<false, false", 1: "<false, true", 2: "<true, true", 3: ""}[lay_i]
        for kr in sq["kernels"]:
            nm = kr["kernel"]
            hit = (kname in nm) if lay_i == 3 else (("gemm2_kernel" + tag in nm or "gemm3_kernel" + tag in nm or "gemm_kernel<true, " + tag[1:] in nm))
            if hit and kr["grid_threads"] == grid_threads and kr.get("mfma_busy") is not None:
                mfma_busy = round(kr["mfma_busy"], 4)
                sq_prov = {"file": "profiles/" + os.path.basename(fn), "csrc_sha": sha, "kernel": nm[:160], "launches_profiled": kr["launches"],
                           "mfma_flops_counted": kr.get("mfma_flops"), "wait_any_frac": round(kr.get("wait_any_frac", 0.0), 3),
                           "formula": "SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 256 CUs x 4 SIMDs)"}
                break
        if mfma_busy is not None:
            break
    if top["members"]:
        desc = (f"gemm2_group_kernel: {len(top['members'])} TN weight gradients in one launch, (M x N x K) = " +
                ", ".join(f"{a}x{b_}x{c}" for a, b_, c in top["members"]))
    else:
        desc = f"{'gemm2/gemm3 (bf16 operands in HBM)' if path == 2 else 'gemm_kernel'} {lay} M={Mm} N={Nn} K={Kk} x{nprob * max(top['key'][6], 1)} problems per launch"
    return {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 5),
            "batch": f"{w.B} windows per GPU", "achieved_in_step_tap": round(ach_tap, 2), "frac_in_step_tap": round(ach_tap / peak, 5),
            "traffic": traffic, "traffic_provenance": prov, "mfma_busy": mfma_busy, "mfma_busy_provenance": sq_prov,
            "traffic_unit": "bytes/launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, separate PMC passes of this build: a committed profile of "
                            "this launch, not a measurement of this run)" if traffic is not None else f"null: {why} (csrc hash {sha})",
            "algorithmic_bytes": alg_bytes, "operands": operands, "flops_per_launch": top["flops"],
            "kernel": desc, "kernel_name_prefix": kname if lay_i == 3 else None, "grid_threads": grid_threads,
            "avg_launch_us": round(kernel_us, 2), "avg_launch_us_eager_tap": round(top["avg_us"], 2),
            "launches_per_step": round(top["launches"] / k2, 2), "all_gemm_ms_per_step": round(gemm_ms, 4), "all_gemm_tflops": round(allfl, 2),
            "gemm_launches_per_step": round(sum(r["launches"] for r in rows) / k2, 1),
            "gather_gemm": next(({"M": r["M"], "N": r["N"], "K": r["K"], "avg_us_eager_tap": round(r["avg_us"], 2)} for r in rows
                                 if r["key"][7] == 1 and r["K"] == CONFIGS[w.cfg]["d_m"] and r["key"][0] == 0), None)}


def hbm_roofline(w, lib, roof):
    """the gather / mask path against the HBM roofline: each kernel timed as 20 launches inside one hipGraph on the batch
    of the step; bytes = what the kernel must read and write once (SURVEY 8d `gather-path GB/s`)."""
    from immtsf import _lib
    dev = w.dev
    notes = w.padded_notes
    B, N, d_m = notes.shape
    mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)      # noqa: E731
    lengths, offsets, rowmap, seg, mtxt = i32(B), i32(B + 1), i32(B * N), i32(B * N), torch.empty(B, dtype=torch.uint8, device=dev)

    def ragged():
        _lib.check(lib.immtsf_ragged_index(_lib.ptr(notes), B, N, d_m, _lib.ptr(mask), _lib.ptr(lengths), _lib.ptr(offsets),
                                           _lib.ptr(rowmap), _lib.ptr(seg), _lib.ptr(mtxt), None, _lib.stream_ptr()), "ragged_index")
    out = []
    # the gather that IS in the timed step (packed notes, bf16 mode): notes_stage_kernel -- a wave per packed note: d_m fp32 read from the
    # resident embedding matrix, d_m + d/2 bf16 written (the note and the Time2Vec of its time stamp: the fold's / the chain's X operand)
    pk = w.batch.get("notes_embeddings") if isinstance(getattr(w, "batch", None), dict) else None
    from immtsf.ops import PackedNotes
    if isinstance(pk, PackedNotes) and hasattr(w.fusion, "ttf") and hasattr(w.fusion.ttf, "time2vec"):
        ix = pk.index()[1]
        try:
            dt = w.fusion.ttf.time2vec.periodic.weight.numel() + 1           # (one linear + dt - 1 periodic features: d / 2)
            R, ldx = B * N, d_m + dt
            X = torch.empty(R, ldx, dtype=torch.bfloat16, device=dev)
            tau = w.batch["tau"].float().contiguous()
            lw, lb, pw_, pb = [p_.detach().float().contiguous() for p_ in w.fusion.ttf._params()[3:7]]
            total = ix["offsets"][B:B + 1]

            def stage():
                _lib.check(lib.immtsf_notes_stage(_lib.ptr(pk.emb), d_m, _lib.ptr(pk.src_rows), _lib.ptr(total), R, _lib.ptr(X), ldx, _lib.ptr(tau),
                                                  _lib.ptr(ix["rowmap"]), dt, _lib.ptr(lw), _lib.ptr(lb), _lib.ptr(pw_), _lib.ptr(pb),
                                                  _lib.stream_ptr()), "notes_stage")
            us = graph_kernel_us(stage, reps=20)
            n_rows = int(w.sum_n)
            byts = n_rows * (d_m * 4 + ldx * 2 + 12)
            out.append({"kernel": "notes_stage_kernel (IN the timed step: gather of the packed notes from the resident embedding matrix, cast to "
                                  "bf16, Time2Vec of their time stamps beside them -- one wave per note)",
                        "bytes": byts, "us": round(us, 2), "GB/s": round(byts / us / 1e3, 1), "frac": round(byts / us / 1e3 / PEAK_HBM_GBS, 4),
                        "rows": n_rows})
        except Exception as e:       # noqa: BLE001 -- a companion figure must not cost the line
            out.append({"kernel": "notes_stage_kernel", "error": str(e)[:200]})
    us = graph_kernel_us(ragged, reps=20)
    byts = B * N * d_m * 4 + B * N * 9 + 4 * (2 * B + 1)
    out.append({"kernel": "note_mask + ragged_index (a2: (sum|V| > 0) scan of the padded notes -> lengths/offsets/rowmap"
                          + ("; NOT in the timed step: the notes arrive packed, see config.notes)" if w.packed else ")"),
                "bytes": byts, "us": round(us, 2), "GB/s": round(byts / us / 1e3, 1), "frac": round(byts / us / 1e3 / PEAK_HBM_GBS, 4)})
    gg = roof.get("gather_gemm") if roof else None
    if gg:
        byts = gg["M"] * gg["K"] * 4 + gg["N"] * gg["K"] * 2 + gg["M"] * gg["N"] * 2
        us = gg["avg_us_eager_tap"]
        out.append({"kernel": f"input_proj GEMM with the gathered A operand (packed rows of V, {gg['M']} x {gg['K']} fp32 read once; "
                              "eager launch incl. launch latency)",
                    "bytes": byts, "us": us, "GB/s": round(byts / us / 1e3, 1), "frac": round(byts / us / 1e3 / PEAK_HBM_GBS, 4)})
    return {"bound": "hbm", "peak": PEAK_HBM_GBS, "unit": "GB/s", "kernels": out,
            "note": f"{B} windows x {N} padded notes x d_m {d_m}: {B * N * d_m * 4 / 1e6:.1f} MB of embeddings; "
                    f"sum of notes {w.sum_n}; HBM3E spec 8 TB/s, a streaming copy reaches ~6.3 TB/s on this part"}


def dropin_ms(dev, precision, steps=20, warmup=5, nan_check="sync"):
    """what an unmodified main.py gets through the drop-in seam: lib.evaluation.compute_all_losses + loss.backward() + clip_grad_norm_ +
    torch.optim.Adam.  nan_check "sync" (the default of the seam: the reference's NaN guards on, a host sync per check, eager
    launches) or "deferred" (IMMTSF_NAN_CHECK=deferred: no host syncs, forward + loss + backward of a repeated batch shape replayed
    from a hipGraph -- lib/evaluation.py _SeamGraph); no FlatTrainer either way"""
    from fusions.FusionModel import FusionModel
    from immtsf import config
    from lib.evaluation import compute_all_losses
    from models.tPatchGNN import tPatchGNN
    config.precision = precision
    old = config.nan_check
    config.nan_check = nan_check
    try:
        torch.manual_seed(0)
        a = model_args(str(dev))
        model, fusion = tPatchGNN(a).to(dev).train(), FusionModel(a).to(dev).train()
        params = list(model.parameters()) + list(fusion.parameters())
        opt = torch.optim.Adam(params, lr=1e-3)
        cpu_b, _ = synth_batch(100, B_PER_GPU)
        b = {k: v.to(dev) for k, v in cpu_b.items()}

        def step():
            opt.zero_grad()
            res = compute_all_losses(model, fusion, b)
            res["loss"].backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        per = []                       # median of five blocks: the eager path is host-bound and a busy host core shows up as 2x outliers
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(max(steps // 2, 1)):
                step()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / max(steps // 2, 1) * 1e3)
        return sorted(per)[2]
    finally:
        config.nan_check = old


def spawn_ranks(n):
    """run this script as n ranks on one node (python -m torch.distributed.run ...) in a child process group; stdout of the
    children is scanned for rank 0's JSON line, which is printed last; returns the launcher's exit code"""
    import socket
    import subprocess
    share = bool(os.environ.get("IMMTSF_BENCH_SHARE_GPU"))
    have = torch.cuda.device_count()             # (counting devices does not initialise the GPU)
    if have < n and not share:
        print(f"bench.py --gpus {n}: only {have} GPU(s) visible", file=sys.stderr)
        return 2
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout:
        t = ln.strip()
        if t.startswith("{") and '"metric"' in t:
            line = t
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    return rc if rc else (0 if line is not None else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS), help="BASELINE.json configuration (cfg2 = the headline metric)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, the companion measurements too: step_stats, roofline, roofline_hbm, the sweep / "
                         "padded / fp32 / drop-in legs, cpu_baseline (a plain run times the steps and prints the line, nothing else)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step left its caller (loss, updated parameters, Adam moments) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline legs")
    ap.add_argument("--no-extras", action="store_true", help="--full without step_stats and the sweep / fp32 / drop-in legs (cfg2, 1 GPU only anyway)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying hipGraphs")
    ap.add_argument("--gemm-config", type=lambda x: int(x, 0), default=0,
                    help="A/B measurements only: immtsf_debug_gemm_config bits (0x100 no XCD order, 0x2000 no specialised wgrad kernel)")
    ap.add_argument("--gemm2-variant", type=int, default=0, help="A/B measurements only: force one tile variant of the bf16-in-memory GEMM")
    ap.add_argument("--phased", action="store_true",
                    help="immtsf.train.PhasedStep: six single-stream hipGraphs on two HIP streams with events between them, instead "
                         "of the whole step as parallel branches of one hipGraph (DESIGN.md section 6 has both measured)")
    ap.add_argument("--flags", action="store_true",
                    help="immtsf.train.FlagStep at any batch size: one hipGraph whose branches synchronise through device flags "
                         f"(spin kernels) instead of graph edges (the default up to {FLAGS_MAX_WINDOWS} windows per GPU)")
    ap.add_argument("--no-flags", action="store_true", help="GraphedStep (graph edges between the branches) at every batch size")
    ap.add_argument("--captured-comm", action="store_true",
                    help="N>1 graph mode: capture the bucketed RCCL all-reduces inside graph A (overlapped with the backward). "
                         "Verified here only on a 1-rank group, so the default is one eager all-reduce between the two graphs")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (RCCL) even for one rank: exercises the N>1 code path on a 1-GPU box")
    ap.add_argument("--no-overlap", action="store_true", help="do not run the backbone on a second HIP stream beside TTF")
    ap.add_argument("--grad-wire", default="auto", choices=["auto", "fp32", "bf16"],
                    help="N>1: element type of the gradient all-reduce; auto = bf16 in bf16 mode (half the xGMI bytes), fp32 otherwise")
    ap.add_argument("--shard-optimizer", action="store_true",
                    help="N>1: reduce-scatter -> clip + Adam on the rank's 1/N shard -> all-gather (FlatTrainer(shard_optimizer=True)) instead "
                         "of the default: all-reduce of the flat gradient, clip + Adam replicated on every rank.  Opt-in: the native "
                         "reduce_scatter_tensor / all_gather_into_tensor branches have only run on gloo's fallbacks and a 1-rank RCCL group")
    ap.add_argument("--no-shard-optimizer", action="store_true", help="(accepted for compatibility: this is the default now)")
    ap.add_argument("--param-wire", default="auto", choices=["auto", "fp32", "bf16"],
                    help="sharded optimizer: what the all-gather moves; auto = bf16 in bf16 mode (with the bf16 gradient wire the step "
                         "then moves exactly the bytes of one bf16 all-reduce; the replicated fp32 parameters are the widened bf16 "
                         "image, the fp32 master stays with the owner), fp32 (exact) otherwise")
    ap.add_argument("--padded-notes", action="store_true",
                    help="hand the notes over as the reference's zero-padded (B, N, d_m) tensor; the default is the packed form of the "
                         "device collate (resident embedding matrix + row index + per-window counts: BASELINE's 'single ragged buffer "
                         "with an offset index'), whose step has no (sum |V| > 0) scan")
    ap.add_argument("--packed-notes", action="store_true", help="(accepted for compatibility: this is the default now)")
    ap.add_argument("--fusion-only", action="store_true",
                    help="time the fusion blocks + loss + backward + optimizer with the backbone's forecast replaced by a fixed random tensor "
                         "(cfg5: the 7 ms of fusion without the 97 ms frozen GPT-2 body of TimeLLM)")
    ap.add_argument("--fuse-tail", default="auto", choices=["auto", "on", "off"],
                    help="A/B measurements only: TTF_T2V_XAttn's proj_out composed into MMF_XAttn_Add's low-rank projection "
                         "(immtsf.config.fuse_tail; auto = on)")
    ap.add_argument("--t2v-form", default="auto", choices=["auto", "chain", "fold", "mix"],
                    help="A/B measurements only: TTF_T2V_XAttn in its folded form wherever its limits hold (auto, the default) or as the "
                         "reference's GEMM chain (immtsf.config.t2v_form)")
    ap.add_argument("--windows-per-gpu", type=int, default=B_PER_GPU,
                    help="exploration only (the `sweep` field covers 64..4096): the metric is quoted on 64 windows per GPU")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    W = args.windows_per_gpu
    # stdout carries exactly one line, the JSON result: everything else a module prints (the fusion registry announces
    # its choices like the reference does) goes to stderr
    json_out, sys.stdout = sys.stdout, sys.stderr

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start N FRESH rank processes (torch.distributed.run) before anything in
        # this one has touched the GPU, relay rank 0's JSON line and exit with the launcher's code.  (Never an exec: a process that
        # has initialised the GPU must not be replaced; this parent never initialises it.)
        sys.stdout = json_out
        raise SystemExit(spawn_ranks(args.gpus))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} with WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} (or without a launcher)")
    assert torch.cuda.is_available(), "bench.py needs the MI355X"
    # control-flow test of the N>1 path on a 1-GPU box: IMMTSF_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and uses gloo
    # (RCCL refuses two ranks on one device); numbers from such a run mean nothing
    share_gpu = bool(os.environ.get("IMMTSF_BENCH_SHARE_GPU"))
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    group = None
    dist_on = world > 1 or args.force_dist
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        group = dist.group.WORLD

    from immtsf import _lib, config
    from immtsf.ops import masked_mse
    from immtsf.train import GraphedStep
    lib = _lib.load()
    if args.gemm_config:
        lib.immtsf_debug_gemm_config(args.gemm_config, 0)
    if args.gemm2_variant:
        lib.immtsf_debug_gemm2_config(args.gemm2_variant, 0, -1)
    config.nan_check = "deferred"       # no host syncs inside the step; the flag is checked after the run
    config.t2v_form = args.t2v_form
    config.fuse_tail = {"auto": "auto", "on": True, "off": False}[args.fuse_tail]
    config.manual_seed(1234 + rank)

    wire = args.grad_wire if args.grad_wire != "auto" else ("bf16" if args.precision == "bf16" else "fp32")
    pwire = args.param_wire if args.param_wire != "auto" else ("bf16" if args.precision == "bf16" else "fp32")
    sharded = dist_on and args.shard_optimizer and not args.no_shard_optimizer
    w = Workload(args.config, dev, W, args.precision, group=group, wire=wire, device_step=not args.no_graph, seed_off=rank,
                 overlap=not args.no_overlap, shard_optimizer=sharded, param_wire=pwire, packed_notes=not args.padded_notes,
                 fusion_only=args.fusion_only)
    trainer, fusion = w.trainer, w.fusion
    use_graph = (not args.no_graph) and w.graphable
    comm_mode = "bucketed on a side stream" if dist_on else "none"
    # per-variable observation counts of the GLOBAL batch: a property of the data (mask), reduced once when the batch
    # is built, so the step itself has no collective besides the gradient all-reduce
    if dist_on:
        import torch.distributed as dist
        dist.all_reduce(w.global_cnt)

    # hipGraph replay.  ONE graph per step whose branches (text side | backbone | parameter-only work) synchronise through device flags
    # (immtsf.train.FlagStep) up to FLAGS_MAX_WINDOWS windows per GPU, beyond that graph edges (GraphedStep).  clip + Adam of step k sit
    # at the head of replay k + 1, each bucket on the branch that reads it first.  N > 1: the SAME single graph; every bucket is rounded
    # to the bf16 wire image where it completes and announced by a counting device flag, a communication stream runs the all-reduces
    # beside the backward, and Adam reads the reduced wire image
    mode = "eager" if not use_graph else "phased" if args.phased else "graphed" if (args.no_flags or args.no_overlap) else \
           "flags" if args.flags else "auto"
    if dist_on and sharded and mode in ("auto", "flags"):
        mode = "graphed"
    try:
        step, step_info = build_step(w, mode, dist_on=dist_on, captured_comm=bool(dist_on and args.captured_comm and use_graph))
    except Exception as e:      # noqa: BLE001
        if dist_on and args.captured_comm:
            raise SystemExit(f"--captured-comm: the collectives could not be captured ({type(e).__name__}); "
                             "re-run without the flag") from e
        raise
    eng = step_info["engine"]
    launch_mode = {"eager": "eager launches",
                   "flags": "hipGraph replay: 1 graph per step, three branches (text side | backbone | parameter-only work) synchronised by device "
                            "flags; clip + Adam of step k at the head of replay k + 1, each bucket on the branch that reads it first",
                   "phased": "hipGraph replay: 6 single-stream graphs per step on 2 HIP streams (text side | backbone), HIP events between them",
                   "graphed": "hipGraph replay (2 graphs/step)", "graphed+captured-comm": "hipGraph replay (2 graphs/step)"}[eng]
    if eng == "graphed" and getattr(step, "single", False):
        launch_mode = "hipGraph replay (1 graph/step: forward, backward, clip + Adam)"
    if eng in ("eager", "graphed", "graphed+captured-comm") and not args.no_overlap:
        launch_mode += ", backbone on a second HIP stream beside TTF"
    if dist_on:
        if eng == "flags":
            launch_mode += "; N > 1: the same single graph (clip + Adam of step k at the head of replay k + 1 read the reduced wire image)"
            comm_mode = (f"bucketed, beside the backward: {len(step.segments)} bucket(s) on a communication stream behind counting device "
                         "flags [" + ", ".join("+".join(w.bucket_names[b] for b in g["buckets"]) + f"@{g['branch']}:{(g['hi'] - g['lo']) * (2 if wire == 'bf16' else 4) / 1e6:.2f}MB"
                                               for g in step.segments) + "], the ranks' guard word summed by the last one" +
                         (f"; order = measured completion (us after the step's start: {step.completion_us})" if getattr(step, "completion_us", None) else ""))
        elif eng == "graphed+captured-comm":
            comm_mode = "captured, bucketed"
        elif eng == "eager":
            comm_mode = "bucketed on a side stream"
        else:
            comm_mode = (f"reduce-scatter ({wire}) -> clip + Adam on the rank's 1/{world} shard -> all-gather ({pwire}), eager, behind "
                         "graph A") if sharded else "all-reduce, eager, between the graphs"

    def barrier():
        if dist_on:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    if os.environ.get("IMMTSF_BENCH_STREAM"):      # (A/B measurements only: the step on a stream of its own instead of the default stream)
        _side = torch.cuda.Stream(device=dev)
        _side.wait_stream(torch.cuda.current_stream())
        torch.cuda.set_stream(_side)
    snap0 = trainer.snapshot() if args.dump_outputs else None      # (the state the dump's step starts from: dump_outputs)
    elapsed, host_enqueue_s, loss = time_steps(step, args.steps, args.warmup, barrier)
    if dist_on:
        import torch.distributed as dist
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if step_info["engine"] == "flags":
        # a spin that gave up (on any rank) dropped steps inside the timed region: the number is void -- fall back to graph edges,
        # say so in the line, and time again
        try:
            step.check()
        except Exception as e:      # noqa: BLE001
            print(f"# FlagStep rejected after the timed region: {e}", file=sys.stderr)
            step.clear_error()
            trainer.flat_grad.zero_()
            step, step_info = build_step(w, "graphed", dist_on=dist_on)
            step_info["flag_step_rejected"] = True
            launch_mode = "hipGraph replay (graph edges between the branches; the flag engine timed out and was rejected)"
            if dist_on:
                comm_mode = "all-reduce, eager, between the graphs"
            elapsed, host_enqueue_s, loss = time_steps(step, args.steps, args.warmup, barrier)
            if dist_on:
                t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                elapsed = float(t.item())
    fusion.check_nan()
    assert torch.isfinite(loss).all(), "loss is not finite"
    ms_per_step = elapsed / args.steps * 1e3
    windows_per_s = W * world * args.steps / elapsed
    if args.dump_outputs:
        dump_outputs(w, step, snap0, args.dump_outputs if rank == 0 else None)
    # the contract's K steps are a ~15 ms sample at cfg2: the same step is replayed in blocks of 20 (>= 200 replays, N = 1 only: no
    # extra collectives are spent on it) and the block means are reported next to `ms_per_step` -- median and spread, not `value`
    step_stats = None
    if args.full and world == 1 and use_graph and not args.no_extras:
        blocks = []
        for _ in range(12):
            el, _, _ = time_steps(step, 20, 0, torch.cuda.synchronize)
            blocks.append(el / 20 * 1e3)
        blocks.sort()
        step_stats = {"replays": 240, "block": 20, "median_ms": round(blocks[len(blocks) // 2], 4), "min_ms": round(blocks[0], 4),
                      "max_ms": round(blocks[-1], 4)}

    roofline = hbm = None
    if args.full and not args.no_roofline and rank == 0:
        roofline = gemm_roofline(w, lib, args)
        hbm = hbm_roofline(w, lib, roofline)

    extras = {}
    grad_bytes = trainer.grad_bytes()
    if args.full and rank == 0 and world == 1 and args.config == "cfg2" and not args.no_extras and W == B_PER_GPU and not args.no_graph:
        w.close()
        del step
        # windows per GPU: where the step leaves the launch-bound regime (the >= 40 % MFMA target presumes a batch size)
        sweep = []
        for nw in (64, 256, 1024, 4096):
            ww = Workload("cfg2", dev, nw, args.precision, packed_notes=not args.padded_notes)
            st, _ = build_step(ww, "graphed" if args.no_flags else "auto")
            k = 10 if nw <= 256 else 4            # median of three blocks (one block of 30 was once seen 2.7 x off: a transient of the box)
            blocks = sorted(time_steps(st, k, 3 if i == 0 else 0, torch.cuda.synchronize)[0] for i in range(3))
            ms = blocks[1] / k * 1e3
            tf = ww.flops_per_window() * nw / (ms * 1e-3) / 1e12
            sweep.append({"windows_per_gpu": nw, "ms_per_step": round(ms, 4), "windows_per_s": round(nw / ms * 1e3, 1),
                          "fusion_algorithmic_tflops": round(tf, 2), "frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4),
                          "fusion_executed_tflops": round(fusion_executed_flops_per_window(ww.sum_n, nw, "cfg2") * nw / (ms * 1e-3) / 1e12, 2)})
            if nw == 4096:      # the gather / mask path where it is not one launch latency long: the index scan over 403 MB of padded notes
                try:
                    extras["roofline_hbm_4096_windows"] = hbm_roofline(ww, lib, None)
                except Exception as e:           # noqa: BLE001 -- a companion figure must not cost the line
                    extras["roofline_hbm_4096_windows"] = {"error": str(e)[:200]}
            ww.close()
            del st, ww
        extras["sweep"] = sweep
        # the same step with the notes handed over in the other form (padded: the reference's collate; packed: immtsf.data's device collate)
        other = "packed" if args.padded_notes else "padded"
        wp = Workload("cfg2", dev, B_PER_GPU, args.precision, packed_notes=bool(args.padded_notes))
        st, _ = build_step(wp, "graphed" if args.no_flags else "auto")
        blocks = sorted(time_steps(st, 40, 5 if i == 0 else 0, torch.cuda.synchronize)[0] for i in range(5))
        el = blocks[2]             # median of five blocks of 40 replays (a single block right after the 4096-window leg was seen 25 % off)
        extras[other] = {"ms_per_step": round(el / 40 * 1e3, 4), "windows_per_s": round(B_PER_GPU / (el / 40), 1),
                         "blocks_ms": [round(b / 40 * 1e3, 4) for b in blocks],
                         "what": "the same step with the notes as " + (
                             "PackedNotes (resident embedding matrix + int32 row index + per-window counts, the device collate's output): "
                             "no note_mask scan in the step" if other == "packed" else
                             "the reference's zero-padded (B, N, d_m) tensor: note_mask + ragged_index re-derive the index in the step")}
        wp.close()
        del st, wp
        # the fp32 parity mode (1e-4 against the reference) on the same step
        wf = Workload("cfg2", dev, B_PER_GPU, "fp32")
        st = GraphedStep(wf.trainer, wf.loss_fn)
        el, _, _ = time_steps(st, 20, 5, torch.cuda.synchronize)
        extras["ms_per_step_fp32"] = round(el / 20 * 1e3, 4)
        wf.close()
        del st, wf
        extras["dropin"] = {"ms_per_step": round(dropin_ms(dev, args.precision, nan_check="deferred"), 4),
                            "ms_per_step_nan_guards_sync": round(dropin_ms(dev, args.precision), 4),
                            "what": "unmodified-main.py seam: lib.evaluation.compute_all_losses + loss.backward() + clip_grad_norm_ + "
                                    "torch.optim.Adam as main.py writes them, no FlatTrainer.  ms_per_step: the seam's default "
                                    "(IMMTSF_NAN_CHECK=deferred: no host syncs; forward + loss + backward replayed from a hipGraph per batch shape; "
                                    "importing lib.evaluation routes optim.Adam / clip_grad_norm_ to immtsf.optim's two fused launches); "
                                    "ms_per_step_nan_guards_sync: IMMTSF_NAN_CHECK=sync, the reference's NaN guards with their host syncs, "
                                    "every launch eager"}
        config.precision = args.precision

    cpu = None
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1 and args.config == "cfg2":
        cpu_b, _ = synth_batch(100, B_PER_GPU)
        cpu = cpu_baseline(cpu_b)
    elif args.full and not args.no_cpu_baseline and rank == 0 and world == 1:
        cpu = cpu_baseline_fusion(args.config)

    if rank == 0:
        fl_win = fusion_flops_per_window(w.sum_n, W, args.config)
        line = {
            "metric": "forecast windows/sec (train fwd+bwd) on ragged 64-entity batch", "value": round(windows_per_s, 1),
            "unit": "windows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic",
            "launch": launch_mode, "engine": step_info["engine"], "flag_step_rejected": step_info["flag_step_rejected"],
            "host_enqueue_ms_per_step": round(host_enqueue_s / args.steps * 1e3, 4),
            "config": {"workload": f"{args.config}: " + CONFIGS[args.config]["text"].format(B=W) +
                                   (" -- FUSION ONLY: the backbone's forecast is a fixed random tensor" if args.fusion_only else ""),
                       "step": "backbone fwd + fusion fwd + masked MSE + backward + grad all-reduce (N>1) + clip + Adam",
                       "notes": ("packed: one ragged buffer of embedding rows + int32 row index + per-window counts (the device collate's "
                                 "output; extras.padded = the same step on the reference's zero-padded tensor)") if w.packed else
                                "padded: the reference's zero-padded (B, N, d_m) tensor, index re-derived in the step",
                       "global_batch": W * world, "parallelism": f"dp{world}", "sum_notes_rank0": w.sum_n,
                       "fusion_algorithmic_gflop_per_window": round(fl_win / 1e9, 4),
                       "fusion_algorithmic_tflops_at_step_time": round(fl_win * W * world / (ms_per_step * 1e-3) / 1e12, 2),
                       "fusion_executed_gflop_per_window": round(fusion_executed_flops_per_window(w.sum_n, W, args.config) / 1e9, 4),
                       "grad_bytes": grad_bytes,
                       "grad_allreduce": comm_mode + (f", {wire} on the wire" if dist_on and not sharded else "")},
            "roofline": roofline, "roofline_hbm": hbm, "cpu_baseline": cpu,
            "roofline_fusion_step": {"bound": "mfma", "achieved": round(fl_win * W * world / (ms_per_step * 1e-3) / 1e12 / world, 2),
                                     "peak": PEAK_BF16_TFLOPS if args.precision == "bf16" else PEAK_FP32_TFLOPS, "unit": "TFLOP/s per GPU",
                                     "frac": round(fl_win * W / (ms_per_step * 1e-3) / 1e12 /
                                                   (PEAK_BF16_TFLOPS if args.precision == "bf16" else PEAK_FP32_TFLOPS), 5),
                                     "batch": f"{W} windows per GPU",
                                     "achieved_executed": round(fusion_executed_flops_per_window(w.sum_n, W, args.config) * W /
                                                                (ms_per_step * 1e-3) / 1e12, 2),
                                     "what": "SURVEY 8d algorithmic fusion flops of the timed region / its time (the whole step: backbone, "
                                             "loss, optimizer and launch gaps are in the denominator); achieved_executed: the flops this "
                                             "build executes for the same function (MMF_XAttn_Add in its low-rank form) / the same time"},
            "step_stats": step_stats}
        line.update(extras)
    if dist_on:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()      # RCCL may log on teardown: keep the JSON line the last thing rank 0 prints
    if rank == 0:
        sys.stderr.flush()
        print(json.dumps(line), file=json_out, flush=True)
    # native libraries (RCCL prints its path on unload) must not write to stdout behind the JSON line
    json_out.flush()
    os.dup2(os.open(os.devnull, os.O_WRONLY), 1)


if __name__ == "__main__":
    main()
