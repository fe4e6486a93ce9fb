"""immtsf.EvalStep -- the evaluation pass (lib.evaluation.evaluation(): validation after every epoch, test whenever validation improves)
as a device-resident engine: per batch the forward (backbone on a side stream, text side on the current one) and ONE metric kernel that
adds the five per-variable sums to an fp64 accumulator on the device -- fused into MMF_XAttn_Add's head in its low-rank form
(MMF_XAttn_Add.forward_metrics), immtsf.ops.eval_metrics_accum behind every other forecast.  A batch shape seen for the second time is
captured into a hipGraph over static copies of the batch and replayed from then on (the seam's policy and memory pool,
lib.evaluation._graph_cache_lookup): a validation loader is not shuffled, so from the second epoch every batch is one graph launch.
Nothing synchronises until result(), which makes the loader's ONE device -> host copy and finishes on the host in float64.

    ev = immtsf.EvalStep(model, fusion)
    for batch in loader: ev(batch)
    res = ev.result()           # {"loss", "mse", "mae", "rmse", "mape"}
    ev.reset()
"""
import weakref

import numpy as np
import torch

from . import config, ops, step_plan

KEYS = ("loss", "mse", "mae", "rmse", "mape")
_TS = ("tp_to_predict", "observed_data", "observed_tp", "observed_mask", "data_to_predict", "mask_predicted_data")
_TXT = ("notes_embeddings", "tau")


def finish_metrics(acc) -> dict:
    """[5, C] sums (se, ae, ape, cnt, cnt_ape; anything np.asarray takes) -> the reference's metrics (lib/evaluation.py:192-283) as python
    floats, in float64: sum / (count + 1e-8) per variable, mean over the variables with a non-zero count, rmse = sqrt(mse).  No
    observation at all gives what that formula gives (0 / 0 = nan), not an error."""
    a = np.asarray(acc, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != 5:
        raise ValueError(f"finish_metrics: expected a (5, C) array, got {a.shape}")
    se, ae, ape, cnt, cnt_ape = a
    with np.errstate(divide="ignore", invalid="ignore"):
        n_var, n_var_ape = np.float64(np.count_nonzero(cnt)), np.float64(np.count_nonzero(cnt_ape))
        mse = (se / (cnt + 1e-8)).sum() / n_var
        mae = (ae / (cnt + 1e-8)).sum() / n_var
        mape = (ape / (cnt_ape + 1e-8)).sum() / n_var_ape
        vals = (mse, mse, mae, np.sqrt(mse), mape)
    return dict(zip(KEYS, (float(v) for v in vals)))


class _EvalGraph:
    """forward + metric kernel of one batch shape, captured over static copies of the batch; adds to the engine's accumulator"""

    def __init__(self, step, batch, names):
        from lib.evaluation import _pool_acquire
        dev = batch["tp_to_predict"].device
        self.names = names
        self.static = {k: batch[k].detach().clone() for k in names}
        self.bytes = sum(v.numel() * v.element_size() for v in self.static.values())
        # one run outside the capture (allocations, lazily built workspaces) into a throw-away accumulator
        spare = torch.zeros_like(step.acc)
        warm = torch.cuda.Stream(device=dev)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            step._enqueue(self.static, spare)
        torch.cuda.current_stream().wait_stream(warm)
        torch.cuda.synchronize()
        pool = _pool_acquire(self, dev)
        self.graph = torch.cuda.CUDAGraph()
        step_plan.collect_before_capture()
        with torch.cuda.graph(self.graph, pool=pool):
            step._enqueue(self.static, step.acc)

    def __call__(self, batch):
        torch._foreach_copy_([self.static[k] for k in self.names], [batch[k] for k in self.names])
        self.graph.replay()


class EvalStep:
    """see the module docstring.  Counters: batches (fed since reset()), replays / captures / eager (since construction)."""
    instances = 0      # engines built in this process (tests: the default path builds none)

    def __init__(self, model, fusion=None, enable_text=True, graph=True):
        self._model = weakref.ref(model)
        fusion = fusion if enable_text else None
        self._fusion = None if fusion is None else weakref.ref(fusion)
        self.graph = bool(graph)
        self.acc = None
        self.batches = self.replays = self.captures = self.eager = 0
        self._graphs, self._seen, self._side = {}, {}, None
        self._scratch = None      # its own slab scratch + ticket word: engines on different streams do not meet in them
        EvalStep.instances += 1

    @property
    def model(self):
        return self._model()

    @property
    def fusion(self):
        return None if self._fusion is None else self._fusion()

    def _enqueue(self, b, acc):
        """forward + metric sums of one batch into acc; launches only"""
        model, fusion = self.model, self.fusion
        truth, mask = b["data_to_predict"], b["mask_predicted_data"]
        tp = b["tp_to_predict"]
        fc_args = (tp, b["observed_data"], b["observed_tp"], b["observed_mask"])
        if fusion is None:
            return ops.eval_metrics_accum(model.forecasting(*fc_args), truth, mask, acc, self._scratch)
        notes, tau = b["notes_embeddings"], b["tau"]
        if not hasattr(fusion, "text_side"):
            return ops.eval_metrics_accum(fusion(notes, tau, tp, model.forecasting(*fc_args)), truth, mask, acc, self._scratch)
        # the backbone beside the text side, joined before the modality block: ordinary stream edges (lib.evaluation.forecast_and_fuse)
        main = torch.cuda.current_stream()
        self._side.wait_stream(main)
        E_txt, M_txt, kv = fusion.text_side(notes, tau, tp)
        with torch.cuda.stream(self._side):
            pred_y = model.forecasting(*fc_args)
        main.wait_stream(self._side)
        pred_y.record_stream(main)
        if hasattr(fusion.mmf, "forward_metrics"):
            return fusion.mmf.forward_metrics(pred_y, E_txt, M_txt, truth, mask, acc, kv=kv, scratch=self._scratch)
        out = fusion.mmf(pred_y, E_txt, M_txt) if kv is None else fusion.mmf(pred_y, E_txt, M_txt, kv=kv)
        return ops.eval_metrics_accum(out, truth, mask, acc, self._scratch)

    def _key(self, b, names):
        """what a captured graph bakes in besides the batch's values (lib.evaluation._seam_key)"""
        mods = [m for m in (self.model, self.fusion) if m is not None]
        sig = tuple(p.data_ptr() for m in mods for p in m.parameters())
        return (config.precision, config.t2v_form, config.fuse_tail, config.xattn_rank, config.attn_mid, config.note_index, config.gr_split,
                config.dlinear_fused, config.timemixer_fused, config.ttm_fused, config.cru_fused, config.latentode_fused, config.neuralflow_fused, config.neuralflow_tanh_fused, config.timesnet_spectrum_fused, sig, tuple((k, tuple(b[k].shape), b[k].dtype) for k in names))

    def __call__(self, batch):
        model, fusion = self.model, self.fusion
        if model is None or (self._fusion is not None and fusion is None):
            raise RuntimeError("EvalStep: its model / fusion module no longer exists")
        if model.training or (fusion is not None and fusion.training):
            raise RuntimeError("EvalStep needs model.eval() and fusion.eval(): a graph captured with dropout on would replay one mask for ever")
        names = _TS + (_TXT if fusion is not None else ())
        dev = batch["tp_to_predict"].device
        Cc = batch["data_to_predict"].shape[-1]
        if self.acc is None:
            self.acc = torch.zeros(5, Cc, dtype=torch.float64, device=dev)      # captured graphs point at it: never reallocated
            self._side = torch.cuda.Stream(device=dev)
            self._scratch = ops.EvalScratch(dev)
        elif self.acc.shape[1] != Cc or self.acc.device != dev:
            raise ValueError(f"EvalStep: batches of {Cc} variables on {dev} after {self.acc.shape[1]} on {self.acc.device}")
        with torch.no_grad():
            g = None
            if (self.graph and getattr(model, "immtsf_graphable", False) and config.nan_check != "sync" and
                    all(torch.is_tensor(batch.get(k)) and batch[k].is_cuda for k in names)):
                from lib.evaluation import _graph_cache_lookup
                need = sum(batch[k].numel() * batch[k].element_size() for k in names)
                key = self._key(batch, names)
                known = key in self._graphs
                g = _graph_cache_lookup(self._graphs, self._seen, key, need, lambda: _EvalGraph(self, batch, names))
                if g is not None and not known:
                    self.captures += 1
            if g is not None:
                g(batch)
                self.replays += 1
            else:
                self._enqueue(batch, self.acc)
                self.eager += 1
        self.batches += 1

    def result(self) -> dict:
        """the metrics of the batches fed since reset(): ONE device -> host copy (which is the pass's only synchronisation)"""
        if config.nan_check == "deferred":
            from lib.evaluation import check_deferred_nan
            check_deferred_nan(self.fusion)
        if self.batches == 0:
            raise ValueError("evaluation(): empty dataloader")
        return finish_metrics(self.acc.cpu().numpy())

    def reset(self):
        """zero the accumulator; the captured graphs stay"""
        if self.acc is not None:
            self.acc.zero_()
        self.batches = 0
