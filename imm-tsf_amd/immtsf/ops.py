"""torch.autograd.Function wrappers around the block-level C ABI (include/immtsf.h).

Every Function enqueues on torch's current HIP stream; the forward workspace (which holds the saved-for-backward
state) is a torch uint8 tensor kept on `ctx`; gradients are written by the HIP backward into one flat buffer
and returned as views.  Inputs must be fp32, contiguous and on the GPU: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, config, step_plan
from ._lib import DecoderParams, FusionCfg, GCNParams, GRParams, NoteIndex, RecAvgParams, T2VParams, TTCNParams, XAddParams, check, ptr, stream_ptr


def _need_gpu(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.ImmtsfError("immtsf ops need tensors on the GPU (HIP); there is no CPU fallback")
        if t.dtype not in (torch.float32, torch.uint8, torch.bool, torch.int32):
            raise _lib.ImmtsfError(f"unsupported dtype {t.dtype}; the HIP path takes fp32 tensors")


def _c(t):
    return None if t is None else t.contiguous()


def _struct(cls, tensors):
    s = cls()
    for name, t in zip(cls.FIELDS, tensors):
        setattr(s, name, None if t is None else t.data_ptr())
    return s


def _sinks_of(params):
    """Gradient sinks registered by immtsf.train.FlatTrainer: a parameter carrying `_immtsf_grad_sink` (a view into
    the trainer's flat gradient buffer) gets its gradient written there directly by the HIP backward, and autograd
    is handed None for it (no AccumulateGrad add kernel, no per-parameter allocation)."""
    return [None if p is None else getattr(p, "_immtsf_grad_sink", None) for p in params]


def _shared(params, sinks):
    """True when every given parameter writes to a sink that several HIP backward ops ADD into (FlatTrainer sink_shared:
    the buffers are zero-filled once per step and every writer accumulates)."""
    return all(s is not None and getattr(p, "_immtsf_grad_shared", False) for p, s in zip(params, sinks))


def _claim_sinks(params, sinks, who):
    """two HIP ops that write the SAME parameters' sinks in one step (tPatchGNN's LearnableTE: the patch encoder and the decoder) must
    both accumulate -- which they do only when the trainer declared the parameters `sink_shared`.  Each op names itself here in its
    forward; a second writer of an undeclared sink raises instead of silently overwriting the first one's gradient."""
    for p, s in zip(params, sinks):
        if p is None or s is None or getattr(p, "_immtsf_grad_shared", False):
            continue
        seen = getattr(p, "_immtsf_sink_writers", None)
        if seen is None:
            p._immtsf_sink_writers = {who}
        elif who not in seen:
            raise _lib.ImmtsfError("a parameter's gradient sink has two writers (%s and %s) but was not declared shared: pass it in "
                                   "FlatTrainer(sink_shared=[...])" % (sorted(seen)[0], who))


def _prezeroed(params, sinks):
    """1 when every gradient of the block goes to a sink that its owner zero-fills each step (FlatTrainer)."""
    ok = all(p is None or (s is not None and getattr(p, "_immtsf_grad_prezeroed", False)) for p, s in zip(params, sinks))
    return 1 if ok else 0


def _grad_buffers(params, sinks=None):
    """(buffers the HIP backward writes, gradients to return to autograd).  One flat allocation for the
    parameters without a sink."""
    sinks = sinks or [None] * len(params)
    n = sum(p.numel() for p, s in zip(params, sinks) if p is not None and s is None)
    dev = next(p.device for p in params if p is not None)
    flat = torch.empty(n, dtype=torch.float32, device=dev) if n else None
    bufs, rets, off = [], [], 0
    for p, s in zip(params, sinks):
        if p is None:
            bufs.append(None)
            rets.append(None)
        elif s is not None:
            bufs.append(s)
            rets.append(None)
        else:
            v = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
            bufs.append(v)
            rets.append(v)
    return bufs, rets


def _zeroed_grad_buffers(params, sinks):
    """like _grad_buffers for backward kernels that ACCUMULATE parameter gradients by atomics: the buffers must read zero.
    Sinks whose owner zero-fills them every step (FlatTrainer) are used as they are; everything else comes out of one
    zero-filled allocation."""
    pre = [s is not None and getattr(p, "_immtsf_grad_prezeroed", False) for p, s in zip(params, sinks)]
    n = sum(p.numel() for p, ok in zip(params, pre) if not ok)
    flat = torch.zeros(n, dtype=torch.float32, device=params[0].device) if n else None
    bufs, rets, off = [], [], 0
    for p, s, ok in zip(params, sinks, pre):
        if ok:
            bufs.append(s)
            rets.append(None)
        else:
            v = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
            bufs.append(v)
            rets.append(v)
    return bufs, rets


def _fire(hook, burst=None):
    """run a bucket hook (immtsf.train.FlatTrainer); burst: (token, index, count) of hooks fired back to back -- buckets that complete at
    the same moment -- which lets a data-parallel step pack, announce and send neighbours in the flat buffer as one"""
    if hook is not None:
        if burst is not None and getattr(hook, "_immtsf_bucket_index", None) is not None:
            hook(burst)
        else:
            hook()


def _bytes(n, dev):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)


# ---- idioms of the fused backbones (one launch reads every parameter through a pointer table, one flat buffer takes every gradient)
_pointer_tables = {}      # owner: _pointer_table.  Never emptied: a captured graph keeps reading the table it was captured with
_grad_layouts = {}        # owner: _grad_layout.  (library entry, dims) -> (offsets, length): a few ints per shape ever seen


def _pointer_table(params, device):
    """the device array of parameter pointers a fused backbone kernel reads, in the order of `params`: one host -> device copy per
    distinct set of storages (so the first call with a new set has to be outside a stream capture, as every warm-up run is)"""
    key = (device.type, device.index) + tuple(p.data_ptr() for p in params)
    t = _pointer_tables.get(key)
    if t is None:
        t = _pointer_tables[key] = torch.tensor(key[2:], dtype=torch.int64, device=device)
    return t


def _grad_layout(lib_fn, dims, n_entries, what):
    """-> (float offset of each of the `n_entries` table entries in the flat gradient that the library entry named `lib_fn` lays out for
    `dims`, -1 = none; the flat gradient's length).  what: the error text for dimensions the library refuses."""
    got = _grad_layouts.get((lib_fn, dims))
    if got is None:
        offs = torch.full((n_entries,), -1, dtype=torch.int32)
        nv = int(getattr(_lib.load(), lib_fn)(*dims, offs.data_ptr(), n_entries))
        if nv < 0:
            raise _lib.ImmtsfError(what)
        got = _grad_layouts[(lib_fn, dims)] = (offs.tolist(), nv)
    return got


def _flat_views(flat, offs, shapes, needs):
    """the flat gradient cut into per-parameter views (None where autograd wants none, or the layout has none)"""
    rets = []
    for o, shape, need in zip(offs, shapes, needs):
        numel = 1
        for s in shape:
            numel *= s
        rets.append(flat[o:o + numel].view(shape) if need and o >= 0 else None)
    return rets


def _kernel_drop(p, site, device):
    """(p, seed, site, counter pointer) of a dropout drawn inside a fused kernel: one config.next_seed() when p > 0, none otherwise"""
    return (p, config.next_seed() if p > 0 else 0, site, config.dropout_counter_ptr(device) if p > 0 else None)


def _dims_supported(supported_fn, workspace_fn, dims_struct, call):
    """a dims-struct backbone's limits: the library's `supported` entry and, for a compute call, a positive workspace size"""
    if not supported_fn(C.byref(dims_struct)):
        return False
    return bool(workspace_fn(C.byref(dims_struct)) > 0) if call else True


# ---- bf16 images of activations that cross a block boundary (bf16 mode).  The producer registers (fp32 tensor, bf16
# image); a consumer that is handed the SAME, unmodified fp32 data finds the image and skips its cast kernel.  The registry
# holds the fp32 tensor's STORAGE (so the address cannot be recycled under a stale entry) but not the tensor: a gradient that a
# backward returns must stay un-referenced, or autograd's AccumulateGrad clones it instead of taking it (a copy launch on the
# serial section in front of the backbone's backward, and the clone then misses its image: a cast launch more).
# All three registries below are owned by the fusion blocks (TTF* / MMF* Functions), which reach them through _reg_put / _reg_take alone.
_shadows = []          # [(storage, data_ptr, shape, version, bf16 tensor)], newest last, at most _SHADOW_CAP entries
_SHADOW_CAP = 6


# ---- hand-over of the fused tail (config.z_handover).  Forward: the producer (TTFT2VXAttnFn) registers its output Z with the cfg of its
# call; the consumer (MMFXRankPFn) that is handed the same data finds it and may ask the library whether the producer's backward takes a
# low-rank gradient.  Backward: the consumer registers (dZ placeholder -> dP, Wc); the producer's backward looks its incoming gradient up.
_handover = []         # [(storage, data_ptr, shape, version, FusionCfg of the producer's call, half_only)]
_lowrank = []          # [(storage, data_ptr, shape, version, (LowRankGrad struct, tensors it points into))]


def _reg_put(reg, t, payload):
    reg.append((t.untyped_storage(), t.data_ptr(), tuple(t.shape), t._version, payload))
    if len(reg) > _SHADOW_CAP:
        del reg[0]


def _reg_take(reg, x, pop=False):
    if x is None or not x.is_contiguous():
        return None
    for i in range(len(reg) - 1, -1, -1):
        _st, p, shape, ver, payload = reg[i]
        if p == x.data_ptr() and shape == tuple(x.shape) and x._version == ver:
            if pop:
                del reg[i]
            return payload
    return None


def _bf16_dataflow(precision, d):
    return precision == 1 and d >= 16 and d % 16 == 0


def make_cfg(B, N, T, Cc, d_m, d, H, precision, training, p_drop, kappa, seed, device=None):
    return FusionCfg(B, N, T, Cc, d_m, d, H, precision, 1 if training else 0, float(p_drop), float(kappa),
                     int(seed) & 0xFFFFFFFFFFFFFFFF, None if device is None else config.dropout_counter_ptr(device))


# ------------------------------------------------------------------------------------------------ TTF_T2V_XAttn
class PackedNotes:
    """A batch's notes in packed-ragged form over a resident embedding matrix (immtsf.data.ResidentStore.collate):
    emb [rows, d_m] fp32, src_rows [sum_n] int32 (row of each note, window-major), lengths [B] int32, N = padded width
    of the accompanying tau (B,N).  Accepted by TTF_T2V_XAttn.forward in place of the zero-padded (B,N,d_m) tensor."""

    def __init__(self, emb, src_rows, lengths, N):
        if emb.numel() >= 2 ** 32:
            raise ValueError("resident embedding matrix must stay below 2^32 elements (32-bit gather offsets)")
        self.emb, self.src_rows, self.lengths, self.N = emb, src_rows, lengths, int(N)
        self.shape = (lengths.shape[0], self.N, emb.shape[1])
        self.device = emb.device
        self._index = None

    def index(self):
        """the batch's ragged index (immtsf_note_index: mask, M_txt, lengths, offsets, rowmap, seg), built ONCE per batch -- the batch
        builder knows every window's note count, so the index is part of the hand-over (offsets authoritative) instead
        of two launches at the head of every forward.  Returns (ctypes struct, tensors it points into)."""
        if self._index is None:
            B, N = self.lengths.shape[0], self.N
            dev = self.device
            u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)        # noqa: E731
            i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)       # noqa: E731
            t = {"mask": u8(B * N), "mtxt": u8(B), "lengths": i32(B), "offsets": i32(B + 1), "rowmap": i32(B * N), "seg": i32(B * N)}
            ix = NoteIndex(*[t[f].data_ptr() for f in NoteIndex.FIELDS])
            check(_lib.load().immtsf_note_index_build(ptr(self.lengths), B, N, C.byref(ix), stream_ptr()), "note_index_build")
            self._index = (ix, t)
        return self._index


class TTFT2VXAttnFn(torch.autograd.Function):
    """(notes (B,N,d_m) | resident emb + src_rows + lengths, tau (B,N)) -> (E_txt (B,T,d), M_txt uint8 (B)).
    params in immtsf_t2v_params order."""

    @staticmethod
    def forward(ctx, notes, tau, T, H, p_drop, training, precision, seed, nan_flag, src_rows, lengths, no_proj, *params):
        # no_proj: False | True | "handover" (True + config.z_handover's promises: the output's only consumer reads the bf16 image when there
        # is one, and may send its gradient back in low-rank form)
        lib = _lib.load()
        handover = no_proj == "handover" and config.z_handover
        no_proj = bool(no_proj)
        notes, tau = _c(notes), _c(tau)
        params = tuple(_c(p) for p in params)
        _need_gpu(notes, tau, *params)
        # (src_rows may come as the PackedNotes itself: then the batch's prebuilt ragged index is used instead of deriving it in the call)
        index = None
        if isinstance(src_rows, PackedNotes):
            index = src_rows.index() if config.note_index else None
            src_rows = src_rows.src_rows
        packed = src_rows is not None
        B, N = tau.shape
        d_m = notes.shape[-1]
        d = params[0].numel()
        cfg = make_cfg(B, N, T, 0, d_m, d, H, precision, training, p_drop, 0.0, seed, notes.device)
        cfg.form = {"auto": 0, "chain": 1, "fold": 2, "mix": 3}[config.t2v_form]        # (the backward reads the same cfg: one form per call pair)
        if no_proj:             # proj_out is left to the consumer (MMFXRankPFn's "_z" form): the output is Z, the LayerNorm + dropout result
            cfg.form |= _lib.FORM_NO_PROJ
        ctx.no_proj = bool(no_proj)
        ws = _bytes(lib.immtsf_ttf_t2v_xattn_workspace_bytes(C.byref(cfg)), notes.device)
        E = torch.empty(B, T, d, dtype=torch.float32, device=notes.device)
        M = torch.empty(B, dtype=torch.uint8, device=notes.device)
        ps = _struct(T2VParams, params)
        E_h = None
        if _bf16_dataflow(precision, d) and d_m % 8 == 0:
            E_h = torch.empty(B, T, d, dtype=torch.bfloat16, device=notes.device)
            cfg.out_h = E_h.data_ptr()
        if handover and E_h is not None and config.nan_check != "sync":
            cfg.form |= _lib.FORM_HALF_OUT        # (E stays unwritten: whoever reads it must take the image -- MMFXRankPFn checks)
        if index is not None:
            cfg.note_index = C.addressof(index[0])
            M = index[1]["mtxt"].view(-1)        # (a fresh tensor object over the batch's M_txt: no copy, no launch)
        ctx.index = index                        # (keeps the struct and its tensors alive for the backward)
        if packed:
            check(lib.immtsf_ttf_t2v_xattn_forward_packed(C.byref(cfg), C.byref(ps), ptr(notes), ptr(src_rows), ptr(lengths),
                                                          ptr(tau), ptr(E), ptr(M), ptr(ws), ws.numel(), stream_ptr()),
                  "ttf_t2v_xattn_forward_packed")
        else:
            check(lib.immtsf_ttf_t2v_xattn_forward(C.byref(cfg), C.byref(ps), ptr(notes), ptr(tau), ptr(E), ptr(M), ptr(ws),
                                                   ws.numel(), ptr(nan_flag), stream_ptr()), "ttf_t2v_xattn_forward")
        cfg.out_h = None
        if E_h is not None:
            _reg_put(_shadows, E, E_h)
        if handover:
            _reg_put(_handover, E, (cfg, bool(cfg.form & _lib.FORM_HALF_OUT)))
        ctx.cfg, ctx.ws, ctx.src_rows = cfg, ws, src_rows
        # scheduling hint of a two-stream captured step (immtsf.train.GraphedStep): this call's backward will set the gate behind its
        # row-bound kernels; the plan remembers who promised, so that nobody waits for a flag nobody sets
        ctx.gate = step_plan.current().arm_gate() if training else None
        ctx.save_for_backward(notes, tau, *[p if p is not None else notes.new_empty(0) for p in params])
        ctx.none_mask = [p is None for p in params]
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        # bucket hooks (immtsf.train.FlatTrainer): a hook fires behind the backward PHASE that completes its bucket -- out_proj /
        # LayerNorm (/ proj_out) gradients are final long before input_proj's, and a data-parallel step hands them to the all-reduce then
        ctx.folded = bool(lib.immtsf_ttf_t2v_xattn_folded(C.byref(cfg)))
        ctx.phase_hooks = _t2v_phase_hooks(params, no_proj, ctx.folded)
        ctx.mark_non_differentiable(M)
        ctx.set_materialize_grads(False)      # no zero-filled uint8 'gradient' of M (one fill kernel per backward)
        return E, M

    @staticmethod
    def backward(ctx, dE, _dM):
        lib = _lib.load()
        saved = ctx.saved_tensors
        notes, tau = saved[0], saved[1]
        params = [None if isnone else p for p, isnone in zip(saved[2:], ctx.none_mask)]
        if dE is None:       # E_txt unused downstream (grads are not materialised, see forward)
            dE = torch.zeros(ctx.cfg.B, ctx.cfg.T, ctx.cfg.d, dtype=torch.float32, device=notes.device)
        dE = dE.contiguous()
        grads, rets = _grad_buffers(params, ctx.sinks)
        sc = _bytes(lib.immtsf_ttf_t2v_xattn_scratch_bytes(C.byref(ctx.cfg)), notes.device)
        ps, gs = _struct(T2VParams, params), _struct(T2VParams, grads)
        ctx.cfg.sched_flag = ctx.gate
        dE_h = _reg_take(_shadows, dE) if _bf16_dataflow(ctx.cfg.precision, ctx.cfg.d) else None
        ctx.cfg.in_h = None if dE_h is None else dE_h.data_ptr()
        lowrank = _reg_take(_lowrank, dE, pop=True) if ctx.no_proj else None      # (dE is then an unwritten placeholder: dZ = coef basis)
        ctx.cfg.lr_grad = None if lowrank is None else C.addressof(lowrank[0])
        cfg, hooks = ctx.cfg, ctx.phase_hooks
        packed = ctx.src_rows is not None

        def call(mask, stream=None):
            cfg.bwd_phase = mask
            st = stream_ptr() if stream is None else stream
            if packed:
                check(lib.immtsf_ttf_t2v_xattn_backward_packed(C.byref(cfg), C.byref(ps), ptr(notes), ptr(ctx.src_rows), ptr(tau),
                                                               ptr(dE), ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(),
                                                               C.byref(gs), st), "ttf_t2v_xattn_backward_packed")
            else:
                check(lib.immtsf_ttf_t2v_xattn_backward(C.byref(cfg), C.byref(ps), ptr(notes), ptr(tau), ptr(dE), ptr(ctx.ws),
                                                        ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs), st),
                      "ttf_t2v_xattn_backward")
            cfg.bwd_phase = 0

        plan = step_plan.current()
        if plan.ttf_flag is not None and not ctx.folded and all(r is None for r in rets):
            # a step with a parameter-only branch (immtsf.train.FlagStep): this stream runs the data path and the LAST phase's weight
            # gradients; the weight gradients of phases A and B -- whose inputs exist long before the end -- leave as one grouped launch
            # on that branch, behind a flag that says phase B's data path has run.  Their buckets' hooks fire there.
            call(_lib.BWD_PHASE_A | _lib.BWD_PHASE_B)
            early = [h for ph, h in hooks if ph < 2]

            def wgrad(stream):
                call(_lib.BWD_WGRAD_A | _lib.BWD_WGRAD_B, stream)
                token = object()
                for i_, h in enumerate(early):
                    _fire(h, (token, i_, len(early)))
            plan.defer_wgrad(wgrad, keep=(notes, tau, dE, sc, ps, gs, params, grads, dE_h, lowrank), ttf=True)
            call(_lib.BWD_PHASE_C | _lib.BWD_WGRAD_C)
            for ph, h in hooks:
                if ph == 2:
                    _fire(h)
        else:
            # one call (every weight gradient in one grouped launch) unless a bucket completes before the last phase: then one call per
            # run of phases up to the next hook (immtsf_fusion_cfg.bwd_phase), data path and weight gradients together
            cuts = sorted({ph for ph, _ in hooks if ph < 2})
            lo = 0
            for c in cuts + [2]:
                call(sum(0x11 << i for i in range(lo, c + 1)) if cuts else 0)
                lo = c + 1
                for ph, h in hooks:
                    if ph == c:
                        _fire(h)
        cfg.lr_grad = None
        if ctx.no_proj:         # (proj_out's gradients come out of the consumer's backward)
            rets = list(rets)
            rets[15] = rets[16] = None
        return (None,) * 12 + tuple(rets)


_T2V_PHASE = (1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 0, 0, 0, 0, 0, 0)      # immtsf_t2v_params index -> backward phase that completes its gradient


def _t2v_phase_hooks(params, no_proj, folded):
    """[(phase, hook)] for TTFT2VXAttnFn.backward: every bucket hook found on the block's parameters, with the phase (0 A, 1 B, 2 C:
    include/immtsf.h IMMTSF_BWD_PHASE_*) behind which ALL of the block's parameters in that hook's bucket have their final gradient.  The
    folded form's gradients all leave its chain rule at the end (phase C); so does a hook whose parameter carries no bucket stamp."""
    own = [(i, p) for i, p in enumerate(params) if p is not None and not (no_proj and i >= 15)]
    out, seen = [], set()
    for i, p in own:
        hook = getattr(p, "_immtsf_bwd_hook", None)
        if hook is None or id(hook) in seen:
            continue
        seen.add(id(hook))
        bucket = getattr(p, "_immtsf_bucket", None)
        if folded or bucket is None:
            out.append((2, hook))
            continue
        out.append((max(_T2V_PHASE[j] for j, q in own if getattr(q, "_immtsf_bucket", None) == bucket), hook))
    return out


# ------------------------------------------------------------------------------------------------ TTF_RecAvg
class TTFRecAvgFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, notes, tau, t_hat, p_drop, training, precision, seed, nan_flag, *params):
        lib = _lib.load()
        notes, tau, t_hat = _c(notes), _c(tau), _c(t_hat)
        params = tuple(_c(p) for p in params)
        _need_gpu(notes, tau, t_hat, *params)
        B, N, d_m = notes.shape
        T = t_hat.shape[1]
        d = params[3].numel()      # ln_w
        cfg = make_cfg(B, N, T, 0, d_m, d, 1, precision, training, p_drop, 0.0, seed, notes.device)
        ws = _bytes(lib.immtsf_ttf_recavg_workspace_bytes(C.byref(cfg)), notes.device)
        E = torch.empty(B, T, d, dtype=torch.float32, device=notes.device)
        M = torch.empty(B, dtype=torch.uint8, device=notes.device)
        ps = _struct(RecAvgParams, params)
        check(lib.immtsf_ttf_recavg_forward(C.byref(cfg), C.byref(ps), ptr(notes), ptr(tau), ptr(t_hat), ptr(E), ptr(M),
                                            ptr(ws), ws.numel(), ptr(nan_flag), stream_ptr()), "ttf_recavg_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.save_for_backward(notes, tau, t_hat, *[p if p is not None else notes.new_empty(0) for p in params])
        ctx.none_mask = [p is None for p in params]
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        ctx.done_hook = getattr(params[0], "_immtsf_bwd_hook", None)
        ctx.mark_non_differentiable(M)
        ctx.set_materialize_grads(False)      # no zero-filled uint8 'gradient' of M (one fill kernel per backward)
        return E, M

    @staticmethod
    def backward(ctx, dE, _dM):
        lib = _lib.load()
        saved = ctx.saved_tensors
        notes, tau, t_hat = saved[:3]
        params = [None if isnone else p for p, isnone in zip(saved[3:], ctx.none_mask)]
        if dE is None:
            dE = torch.zeros(ctx.cfg.B, ctx.cfg.T, ctx.cfg.d, dtype=torch.float32, device=notes.device)
        dE = dE.contiguous()
        grads, rets = _grad_buffers(params, ctx.sinks)
        sc = _bytes(lib.immtsf_ttf_recavg_scratch_bytes(C.byref(ctx.cfg)), notes.device)
        ps, gs = _struct(RecAvgParams, params), _struct(RecAvgParams, grads)
        check(lib.immtsf_ttf_recavg_backward(C.byref(ctx.cfg), C.byref(ps), ptr(notes), ptr(tau), ptr(t_hat), ptr(dE),
                                             ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs), stream_ptr()),
              "ttf_recavg_backward")
        _fire(ctx.done_hook)
        return (None,) * 8 + tuple(rets)


# ------------------------------------------------------------------------------------------------ MMF_XAttn_Add
class MMFXAttnAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, E, M_u8, H, kappa, p_drop, training, precision, seed, *params):
        lib = _lib.load()
        Y, E, M_u8 = _c(Y), _c(E), _c(M_u8)
        params = tuple(_c(p) for p in params)
        _need_gpu(Y, E, M_u8, *params)
        B, T, Cc = Y.shape
        d = E.shape[2]
        cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, training, p_drop, kappa, seed, Y.device)
        ws = _bytes(lib.immtsf_mmf_xattn_add_workspace_bytes(C.byref(cfg)), Y.device)
        out = torch.empty_like(Y)
        ps = _struct(XAddParams, params)
        check(lib.immtsf_mmf_xattn_add_forward(C.byref(cfg), C.byref(ps), ptr(Y), ptr(E), ptr(M_u8), ptr(out), ptr(ws),
                                               ws.numel(), stream_ptr()), "mmf_xattn_add_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        ctx.done_hook = getattr(params[0], "_immtsf_bwd_hook", None)
        ctx.save_for_backward(Y, E, M_u8, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        Y, E, M_u8, *params = ctx.saved_tensors
        dout = dout.contiguous()
        grads, rets = _grad_buffers(params, ctx.sinks)
        dY, dE = torch.empty_like(Y), torch.empty_like(E)
        sc = _bytes(lib.immtsf_mmf_xattn_add_scratch_bytes(C.byref(ctx.cfg)), Y.device)
        ps, gs = _struct(XAddParams, params), _struct(XAddParams, grads)
        check(lib.immtsf_mmf_xattn_add_backward(C.byref(ctx.cfg), C.byref(ps), ptr(Y), ptr(E), ptr(M_u8), ptr(dout), ptr(dY),
                                                ptr(dE), ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs),
                                                stream_ptr()), "mmf_xattn_add_backward")
        _fire(ctx.done_hook)
        return (dY, dE, None, None, None, None, None, None, None) + tuple(rets)


def _half_grads(params, owned_full, owned_part, sinks):
    """gradient buffers for one half of MMF_XAttn_Add: `params` in XAddParams order with None for parameters the half
    does not touch.  owned_part = indices (attn.in_proj_weight / _bias) of which the half writes only some rows: without a
    sink the rest of such a buffer must read as zero, because autograd adds the two halves' tensors."""
    grads, rets = _grad_buffers(params, sinks)
    for i in owned_part:
        if params[i] is not None and sinks[i] is None:
            grads[i].zero_()
    return grads, rets


class MMFXAttnKVFn(torch.autograd.Function):
    """key/value half of MMF_XAttn_Add: E_txt -> KV (B,T,2d) = (k | v) = in_proj_{k,v}(proj_{k,v}(E_txt)), computed with the
    per-step product weights.  Depends only on the text side, so it can run beside the backbone; params: (proj_k_w,
    proj_v_w, attn_in_w, attn_in_b)."""

    @staticmethod
    def forward(ctx, E, H, precision, done_hook, proj_k_w, proj_v_w, attn_in_w, attn_in_b):
        lib = _lib.load()
        E = _c(E)
        params = (None, _c(proj_k_w), _c(proj_v_w), _c(attn_in_w), _c(attn_in_b), None, None, None, None, None, None)
        _need_gpu(E, *params)
        B, T, d = E.shape
        cfg = make_cfg(B, 0, T, 1, 0, d, H, precision, False, 0.0, 0.0, 0, E.device)
        ws = _bytes(lib.immtsf_mmf_xattn_kv_workspace_bytes(C.byref(cfg)), E.device)
        KV = torch.empty(B, T, 2 * d, dtype=torch.float32, device=E.device)
        ps = _struct(XAddParams, params)
        E_h = _reg_take(_shadows, E) if _bf16_dataflow(precision, d) else None
        cfg.in_h = None if E_h is None else E_h.data_ptr()
        ctx.E_h = E_h
        check(lib.immtsf_mmf_xattn_kv_forward(C.byref(cfg), C.byref(ps), ptr(E), ptr(KV), ptr(ws), ws.numel(), stream_ptr()),
              "mmf_xattn_kv_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        ctx.done_hook = done_hook          # the block's gradients are final once THIS half's backward has run
        ctx.save_for_backward(E, *params[1:5])
        return KV

    @staticmethod
    def backward(ctx, dKV):
        lib = _lib.load()
        E, wk, wv, win, bin_ = ctx.saved_tensors
        params = [None, wk, wv, win, bin_, None, None, None, None, None, None]
        grads, rets = _half_grads(params, (1, 2), (3, 4), ctx.sinks)
        dE = torch.empty_like(E)
        sc = _bytes(lib.immtsf_mmf_xattn_kv_scratch_bytes(C.byref(ctx.cfg)), E.device)
        ps, gs = _struct(XAddParams, params), _struct(XAddParams, grads)
        dKV = dKV.contiguous()
        cfg, dE_h = ctx.cfg, None
        if _bf16_dataflow(cfg.precision, cfg.d):
            dKV_h = _reg_take(_shadows, dKV)
            cfg.in_h = None if dKV_h is None else dKV_h.data_ptr()
            cfg.aux_h = None if ctx.E_h is None else ctx.E_h.data_ptr()
            dE_h = torch.empty(dE.shape, dtype=torch.bfloat16, device=dE.device)
            cfg.out_h = dE_h.data_ptr()
        check(lib.immtsf_mmf_xattn_kv_backward(C.byref(cfg), C.byref(ps), ptr(E), ptr(dKV), ptr(dE), ptr(ctx.ws),
                                               ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs), stream_ptr()),
              "mmf_xattn_kv_backward")
        if dE_h is not None:
            _reg_put(_shadows, dE, dE_h)
        _fire(ctx.done_hook)
        return (dE, None, None, None) + tuple(rets[1:5])


def mmf_xattn_q_fold(Y_C, d, H, precision, params):
    """the query half's per-step product weights (see immtsf_mmf_xattn_q_fold): a flat fp32 tensor; no autograd -- the
    parameters' gradients come out of MMFXAttnQFn.backward by the chain rule"""
    lib = _lib.load()
    dev = params[0].device
    cfg = make_cfg(1, 0, 1, Y_C, 0, d, H, precision, False, 0.0, 0.0, 0, dev)
    fold = torch.empty(lib.immtsf_mmf_xattn_q_fold_floats(C.byref(cfg)), dtype=torch.float32, device=dev)
    ps = _struct(XAddParams, tuple(None if p is None else _c(p.detach()) for p in params))
    check(lib.immtsf_mmf_xattn_q_fold(C.byref(cfg), C.byref(ps), ptr(fold), stream_ptr()), "mmf_xattn_q_fold")
    return fold


class MMFXAttnQFn(torch.autograd.Function):
    """query half of MMF_XAttn_Add: (Y_ts, KV, M_txt) -> Y_out.  params in XAddParams order without proj_k/proj_v.
    fold: the result of mmf_xattn_q_fold (or None: formed inside the forward)."""

    @staticmethod
    def forward(ctx, Y, KV, M_u8, fold, H, kappa, p_drop, training, precision, seed, proj_q_w, attn_in_w, attn_in_b, *rest):
        lib = _lib.load()
        Y, KV, M_u8 = _c(Y), _c(KV), _c(M_u8)
        params = (_c(proj_q_w), None, None, _c(attn_in_w), _c(attn_in_b)) + tuple(_c(p) for p in rest)
        _need_gpu(Y, KV, M_u8, *params)
        B, T, Cc = Y.shape
        d = KV.shape[2] // 2
        cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, training, p_drop, kappa, seed, Y.device)
        ws = _bytes(lib.immtsf_mmf_xattn_q_workspace_bytes(C.byref(cfg)), Y.device)
        out = torch.empty_like(Y)
        ps = _struct(XAddParams, params)
        check(lib.immtsf_mmf_xattn_q_forward(C.byref(cfg), C.byref(ps), ptr(Y), ptr(KV), ptr(M_u8), ptr(fold), ptr(out), ptr(ws),
                                             ws.numel(), stream_ptr()), "mmf_xattn_q_forward")
        ctx.cfg, ctx.ws, ctx.fold = cfg, ws, fold
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        ctx.save_for_backward(Y, KV, M_u8, params[0], *params[3:])
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        Y, KV, M_u8, wq, *rest = ctx.saved_tensors
        params = [wq, None, None] + list(rest)
        grads, rets = _half_grads(params, (0, 5, 6, 7, 8, 9, 10), (3, 4), ctx.sinks)
        dY, dKV = torch.empty_like(Y), torch.empty_like(KV)
        sc = _bytes(lib.immtsf_mmf_xattn_q_scratch_bytes(C.byref(ctx.cfg)), Y.device)
        ps, gs = _struct(XAddParams, params), _struct(XAddParams, grads)
        # the parameter gradients can only be postponed when they go to sinks (autograd gets None for them either way)
        defer = step_plan.current().hold_params and all(r is None for r in rets)
        cfg, ws, fold = ctx.cfg, ctx.ws, ctx.fold
        dKV_h = None
        if _bf16_dataflow(cfg.precision, cfg.d):
            dKV_h = torch.empty(dKV.shape, dtype=torch.bfloat16, device=dKV.device)
            cfg.out_h = dKV_h.data_ptr()
        check(lib.immtsf_mmf_xattn_q_backward(C.byref(cfg), C.byref(ps), ptr(Y), ptr(KV), ptr(M_u8), ptr(fold), ptr(dout.contiguous()),
                                              ptr(dY), ptr(dKV), ptr(ws), ws.numel(), ptr(sc), sc.numel(), C.byref(gs),
                                              1 if defer else 0, stream_ptr()), "mmf_xattn_q_backward")
        cfg.out_h = None
        if dKV_h is not None:
            _reg_put(_shadows, dKV, dKV_h)
        if defer:
            keep = (Y, M_u8, params, grads)         # the closure keeps every buffer it touches alive

            def finish():
                check(lib.immtsf_mmf_xattn_q_backward_params(C.byref(cfg), C.byref(ps), ptr(keep[0]), ptr(keep[1]), ptr(fold), ptr(ws),
                                                             ws.numel(), ptr(sc), sc.numel(), C.byref(gs), stream_ptr()),
                      "mmf_xattn_q_backward_params")
            step_plan.current().defer_params(finish)
        return (dY, dKV, None, None, None, None, None, None, None, None, rets[0]) + tuple(rets[3:])


# ---- MMF_XAttn_Add, low-rank form (csrc/xrank.hip): the text side is projected onto (2C+1) H columns, the attention + head is one
# kernel per direction on those columns
def mmf_xrank_pw(T, Cc, d, H):
    """row pitch of P for these dimensions, or 0 when the low-rank form does not take them (config.xattn_rank off, or limits)"""
    if not config.xattn_rank:
        return 0
    lib = _lib.load()
    cfg = make_cfg(1, 0, T, Cc, 0, d, H, 0, False, 0.0, 0.0, 0, None)
    return int(lib.immtsf_mmf_xrank_pw(C.byref(cfg)))


class MMFXRankPFn(torch.autograd.Function):
    """P half of MMF_XAttn_Add's low-rank form: E_txt -> (P (B,T,pw), b_HO (C)).  Depends only on the text side; its backward yields
    dE_txt and the gradients of every parameter except LayerNorm's.  params: XAddParams order without ln_w / ln_b."""

    @staticmethod
    def forward(ctx, E, Cc, H, precision, done_hook, *params9):
        lib = _lib.load()
        E = _c(E)
        # "_z" form: two more parameters, the producer's last linear map (proj_out.weight, .bias); E is then Z, its input
        proj = tuple(_c(p) for p in params9[9:11]) if len(params9) == 11 else None
        params9 = params9[:9]
        params = tuple(_c(p) for p in params9) + (None, None)
        _need_gpu(E, *params)
        B, T, d = E.shape
        cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, False, 0.0, 0.0, 0, E.device)
        pw = int(lib.immtsf_mmf_xrank_pw(C.byref(cfg)))
        if pw <= 0:
            raise _lib.ImmtsfError("MMF_XAttn_Add low-rank form: shape outside its limits")
        ws = _bytes(lib.immtsf_mmf_xrank_p_workspace_bytes(C.byref(cfg)), E.device)
        P = torch.empty(B, T, pw, dtype=torch.float32, device=E.device)
        bHO = torch.empty(Cc, dtype=torch.float32, device=E.device)
        ps = _struct(XAddParams, params)
        E_h = _reg_take(_shadows, E) if _bf16_dataflow(precision, d) else None
        cfg.in_h = None if E_h is None else E_h.data_ptr()
        ctx.E_h = E_h
        # the fused tail's hand-over (config.z_handover): did the producer promise to take a low-rank gradient for this Z?
        ho = _reg_take(_handover, E, pop=True) if proj is not None else None      # (one consumer: the entry has done its work)
        ctx.lowrank = False
        if ho is not None:
            if ho[1] and E_h is None:
                raise _lib.ImmtsfError("Z was handed over as its bf16 image alone (config.z_handover) but the image is gone")
            ctx.lowrank = bool(lib.immtsf_ttf_t2v_xattn_accepts_lowrank(C.byref(ho[0]), pw))
        # the fold depends on parameters only: in a step that offers a fold stream (immtsf.train.FlagStep) it runs there, beside the
        # text side's own forward, and this stream picks it up just before the projection
        def fold(stream):
            if proj is not None:
                check(lib.immtsf_mmf_xrank_fold_z(C.byref(cfg), C.byref(ps), ptr(proj[0]), ptr(proj[1]), ptr(bHO), ptr(ws), ws.numel(),
                                                  stream), "mmf_xrank_fold_z")
            else:
                check(lib.immtsf_mmf_xrank_fold(C.byref(cfg), C.byref(ps), ptr(bHO), ptr(ws), ws.numel(), stream), "mmf_xrank_fold")
        folded = 1 if step_plan.current().fold(fold, ws, bHO) else 0
        if proj is not None:
            _need_gpu(*proj)
            check(lib.immtsf_mmf_xrank_p_forward_z(C.byref(cfg), C.byref(ps), ptr(proj[0]), ptr(proj[1]), ptr(E), ptr(P), ptr(bHO), ptr(ws),
                                                   ws.numel(), folded, stream_ptr()), "mmf_xrank_p_forward_z")
        else:
            check(lib.immtsf_mmf_xrank_p_forward(C.byref(cfg), C.byref(ps), ptr(E), ptr(P), ptr(bHO), ptr(ws), ws.numel(),
                                                 folded, stream_ptr()), "mmf_xrank_p_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.sinks = _sinks_of(params)
        ctx.done_hook = done_hook          # the block's gradients are final once THIS half's backward has run
        ctx.has_proj = proj is not None
        ctx.proj_sinks = _sinks_of(proj) if proj is not None else None
        ctx.save_for_backward(E, *params[:9], *(proj or ()))
        return P, bHO

    @staticmethod
    def backward(ctx, dP, dbHO):
        lib = _lib.load()
        E, *params9 = ctx.saved_tensors
        proj = None
        if ctx.has_proj:
            proj, params9 = params9[9:11], params9[:9]
            pgrads, prets = _grad_buffers(proj, ctx.proj_sinks)
        params = list(params9) + [None, None]
        grads, rets = _grad_buffers(params, ctx.sinks)
        dE = torch.empty_like(E)          # (low-rank hand-over: an unwritten placeholder that carries the registration below)
        cfg = ctx.cfg
        lowrank = ctx.lowrank and proj is not None and config.z_handover
        cfg.form = (cfg.form | _lib.FORM_LOWRANK_OUT) if lowrank else (cfg.form & ~_lib.FORM_LOWRANK_OUT)
        sc = _bytes(lib.immtsf_mmf_xrank_p_scratch_bytes(C.byref(cfg)), E.device)
        ps, gs = _struct(XAddParams, params), _struct(XAddParams, grads)
        dP = dP.contiguous()
        dbHO = torch.zeros(cfg.C, dtype=torch.float32, device=E.device) if dbHO is None else dbHO.contiguous()
        dE_h = None
        if _bf16_dataflow(cfg.precision, cfg.d):
            dP_h = _reg_take(_shadows, dP)
            cfg.in_h = None if dP_h is None else dP_h.data_ptr()
            cfg.aux_h = None if ctx.E_h is None else ctx.E_h.data_ptr()
            if proj is None:        # ("_z" form: the producer's backward reads dZ as fp32 rows only)
                dE_h = torch.empty(dE.shape, dtype=torch.bfloat16, device=dE.device)
                cfg.out_h = dE_h.data_ptr()
            else:
                cfg.out_h = None

        ws0 = ctx.ws

        def params_chain(stream, first=0, last=3, keep=(params, grads)):
            # launches first..last of the parameter chain; "_z" form: the parameter-only step in front of it (dW_fold from dWc;
            # proj_out's gradients) with the first
            if proj is not None and first == 0:
                check(lib.immtsf_mmf_xrank_p_backward_pre_z(C.byref(cfg), ptr(proj[0]), ptr(proj[1]), ptr(ws0), ws0.numel(), ptr(sc), sc.numel(),
                                                            ptr(pgrads[0]), ptr(pgrads[1]), stream), "mmf_xrank_p_backward_pre_z")
            check(lib.immtsf_mmf_xrank_p_backward_params(C.byref(cfg), C.byref(ps), ptr(dbHO), ptr(ws0), ws0.numel(), ptr(sc), sc.numel(),
                                                         C.byref(gs), first, last, stream), "mmf_xrank_p_backward_params")

        def data_half(part=0, stream=None):
            # part 0: dZ and the chain's seeds; "_z" form only: BWD_PHASE_A = dZ alone, BWD_WGRAD_A = the seeds (dWc, dbc) alone
            if proj is not None:
                cfg.bwd_phase = part
                check(lib.immtsf_mmf_xrank_p_backward_data_z(C.byref(cfg), C.byref(ps), ptr(proj[0]), ptr(proj[1]), ptr(E), ptr(dP), ptr(dE),
                                                             ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(),
                                                             stream_ptr() if stream is None else stream),
                      "mmf_xrank_p_backward_data_z")
                cfg.bwd_phase = 0
            else:
                check(lib.immtsf_mmf_xrank_p_backward_data(C.byref(cfg), C.byref(ps), ptr(E), ptr(dP), ptr(dE), ptr(ctx.ws), ctx.ws.numel(), ptr(sc),
                                                           sc.numel(), stream_ptr()), "mmf_xrank_p_backward_data")
        plan = step_plan.current()
        if all(r is None for r in rets[:9]) and plan.defer > 0:
            # every gradient goes straight to its sink: the last `defer` launches of the parameter chain are left to the other branch
            k = 3 - min(3, int(plan.defer))
            # the "_z" form with the whole chain deferred: this stream (the text side's dependent chain) only forms dZ; the chain's
            # seeds dWc = dP^T Z -- parameter-gradient work too -- open the other branch's jobs
            seeds_later = proj is not None and k == 0
            data_half(_lib.BWD_PHASE_A if seeds_later else 0)
            if seeds_later:
                plan.jobs.append(lambda stream, keep=(E, dP): data_half(_lib.BWD_WGRAD_A, stream))
            if k > 0:
                params_chain(stream_ptr(), 0, k)
            plan.set_tail()
            plan.jobs.append(lambda stream: params_chain(stream, k, 3))
            # the block's gradients are final behind the LAST of those launches: its hook (data parallel: the bucket's announcement)
            # fires there, on the stream that runs them
            hook, ctx.done_hook = ctx.done_hook, None
            plan.jobs.append(lambda stream, hook=hook: _fire(hook))
        else:
            data_half()
            params_chain(stream_ptr())
        if dE_h is not None:
            _reg_put(_shadows, dE, dE_h)
        if lowrank:
            basis, rank = C.c_void_p(), C.c_int32()
            check(lib.immtsf_mmf_xrank_lowrank_basis(C.byref(cfg), ptr(ctx.ws), ctx.ws.numel(), C.byref(basis), C.byref(rank)),
                  "mmf_xrank_lowrank_basis")
            _reg_put(_lowrank, dE, (_lib.LowRankGrad(dP.data_ptr(), basis.value, rank.value, dP.shape[-1]), dP, ctx.ws))
        _fire(ctx.done_hook)
        return (dE, None, None, None, None) + tuple(rets[:9]) + (tuple(prets) if proj is not None else ())


class MMFXRankQFn(torch.autograd.Function):
    """Q half of the low-rank form: (Y_ts, P, b_HO, M_txt, ln_w, ln_b) -> Y_out; the serial section between the backbone's forward
    and backward (one kernel per direction)."""

    @staticmethod
    def forward(ctx, Y, P, bHO, M_u8, d, H, kappa, p_drop, training, precision, seed, ln_w, ln_b):
        lib = _lib.load()
        Y, P, bHO, M_u8, ln_w, ln_b = _c(Y), _c(P), _c(bHO), _c(M_u8), _c(ln_w), _c(ln_b)
        _need_gpu(Y, P, bHO, M_u8, ln_w, ln_b)
        B, T, Cc = Y.shape
        cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, training, p_drop, kappa, seed, Y.device)
        if int(lib.immtsf_mmf_xrank_pw(C.byref(cfg))) != P.shape[2]:
            raise _lib.ImmtsfError("MMF_XAttn_Add low-rank form: P does not have the row pitch of these dimensions")
        ws = _bytes(lib.immtsf_mmf_xrank_q_workspace_bytes(C.byref(cfg)), Y.device)
        out = torch.empty_like(Y)
        check(lib.immtsf_mmf_xrank_q_forward(C.byref(cfg), ptr(ln_w), ptr(ln_b), ptr(Y), ptr(P), ptr(bHO), ptr(M_u8), ptr(out), ptr(ws),
                                             ws.numel(), stream_ptr()), "mmf_xrank_q_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.sinks = _sinks_of((ln_w, ln_b))
        ctx.save_for_backward(Y, P, M_u8, ln_w, ln_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        Y, P, M_u8, ln_w, ln_b = ctx.saved_tensors
        grads, rets = _grad_buffers((ln_w, ln_b), ctx.sinks)
        dY, dP = torch.empty_like(Y), torch.empty_like(P)
        dbHO = torch.empty(Y.shape[2], dtype=torch.float32, device=Y.device)
        cfg, dP_h = ctx.cfg, None
        if _bf16_dataflow(cfg.precision, cfg.d):
            dP_h = torch.empty(dP.shape, dtype=torch.bfloat16, device=dP.device)
            cfg.out_h = dP_h.data_ptr()
        check(lib.immtsf_mmf_xrank_q_backward(C.byref(cfg), ptr(ln_w), ptr(Y), ptr(P), ptr(M_u8), ptr(dout.contiguous()), ptr(dY), ptr(dP),
                                              ptr(dbHO), ptr(grads[0]), ptr(grads[1]), ptr(ctx.ws), ctx.ws.numel(), stream_ptr()),
              "mmf_xrank_q_backward")
        cfg.out_h = None
        if dP_h is not None:
            _reg_put(_shadows, dP, dP_h)
        return (dY, dP, dbHO, None, None, None, None, None, None, None, None) + tuple(rets)


_xq_tickets = {}       # owner: _xq_ticket.  (device type, index) -> the ticket words of the two *_q_train kernels


def _xq_ticket(device) -> torch.Tensor:
    """the zero-initialised ticket word of immtsf_mmf_xrank_q_train: one per device for the life of the process (a captured graph keeps
    pointing at it; the call leaves it zero; one training step per device at a time)"""
    key = (device.type, device.index)
    t = _xq_tickets.get(key)
    if t is None:
        t = _xq_tickets[key] = torch.zeros(64, dtype=torch.int32, device=device)
    return t


class MMFXRankQLossFn(torch.autograd.Function):
    """Q half of the low-rank form + masked MSE (immtsf.ops.masked_mse with global_cnt) + the backward of both, ONE launch: the
    forward computes the loss and every gradient (seeded with 1); backward() hands them on (scaled unless the seed is
    backward_unit's).  (Y_ts, P, b_HO, M_txt, truth, mask, cnt, ln_w, ln_b) -> loss."""

    @staticmethod
    def forward(ctx, Y, P, bHO, M_u8, truth, mask, cnt, d, H, kappa, p_drop, training, precision, seed, ln_w, ln_b):
        lib = _lib.load()
        # the early "dY_ts is ready" flag is only sound when autograd hands THIS call's dY buffer on as Y's gradient: a
        # non-contiguous Y makes AccumulateGrad clone it into Y's layout (a copy kernel behind this one)
        y_dense = Y.is_contiguous()
        Y, P, bHO, M_u8, ln_w, ln_b = _c(Y), _c(P), _c(bHO), _c(M_u8), _c(ln_w), _c(ln_b)
        truth, mask, cnt = _c(truth), _c(mask), _c(cnt.to(torch.float32))
        _need_gpu(Y, P, bHO, M_u8, truth, mask, cnt, ln_w, ln_b)
        B, T, Cc = Y.shape
        cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, training, p_drop, kappa, seed, Y.device)
        if int(lib.immtsf_mmf_xrank_pw(C.byref(cfg))) != P.shape[2]:
            raise _lib.ImmtsfError("MMF_XAttn_Add low-rank form: P does not have the row pitch of these dimensions")
        sc = _bytes(lib.immtsf_mmf_xrank_q_train_scratch_bytes(C.byref(cfg)), Y.device)
        sinks = _sinks_of((ln_w, ln_b))
        grads, rets = _grad_buffers((ln_w, ln_b), sinks)
        dY, dP = torch.empty_like(Y), torch.empty_like(P)
        dbHO = torch.empty(Cc, dtype=torch.float32, device=Y.device)
        loss = torch.empty((), dtype=torch.float32, device=Y.device)
        dP_h = None
        if _bf16_dataflow(cfg.precision, cfg.d):
            dP_h = torch.empty(dP.shape, dtype=torch.bfloat16, device=dP.device)
            cfg.out_h = dP_h.data_ptr()
        # immtsf.train.FlagStep: the device flag the backbone's stream waits on before its backward is published by this kernel as
        # soon as dY_ts is complete (the step's head flag is taken: the caller skips its own flag_set)
        flag = step_plan.current().take_head_flag(dY) if y_dense else None
        check(lib.immtsf_mmf_xrank_q_train(C.byref(cfg), ptr(ln_w), ptr(ln_b), ptr(Y), ptr(P), ptr(bHO), ptr(M_u8), ptr(truth), ptr(mask),
                                           ptr(cnt), 1.0, None, ptr(loss), ptr(dY), ptr(dP), ptr(dbHO), ptr(grads[0]), ptr(grads[1]),
                                           ptr(sc), sc.numel(), ptr(_xq_ticket(Y.device)), flag, stream_ptr()), "mmf_xrank_q_train")
        if dP_h is not None:
            _reg_put(_shadows, dP, dP_h)
        ctx.grads = (dY, dP, dbHO) + tuple(rets)
        # LayerNorm's two gradients went straight to FlatTrainer's sinks (rets None): they were written with the unit seed, so a
        # backward with any other seed (loss scaling, loss * k) has to rescale them where they lie
        ctx.sunk = tuple(b for b, r in zip(grads, rets) if r is None)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        g = ctx.grads
        ctx.grads = None
        if not is_unit_grad(dloss):
            g = tuple(None if t is None else t * dloss for t in g)
            for b in ctx.sunk:           # (one writer per sink and step -- the sink contract -- so scaling in place is exact)
                b.mul_(dloss)
        ctx.sunk = ()
        return (g[0], g[1], g[2]) + (None,) * 11 + (g[3], g[4])


# ------------------------------------------------------------------------------------------------ MMF_GR_Add
class MMFGRAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, E, M_u8, hidden, p_drop, training, precision, seed, *params):
        lib = _lib.load()
        Y, E, M_u8 = _c(Y), _c(E), _c(M_u8)
        params = tuple(_c(p) for p in params)
        _need_gpu(Y, E, M_u8, *params)
        B, T, Cc = Y.shape
        d = E.shape[2]
        cfg = make_cfg(B, 0, T, Cc, 0, d, 1, precision, training, p_drop, 0.0, seed, Y.device)
        ws = _bytes(lib.immtsf_mmf_gr_add_workspace_bytes(C.byref(cfg), hidden), Y.device)
        out = torch.empty_like(Y)
        ps = _struct(GRParams, params)
        check(lib.immtsf_mmf_gr_add_forward(C.byref(cfg), hidden, C.byref(ps), ptr(Y), ptr(E), ptr(M_u8), ptr(out), ptr(ws),
                                            ws.numel(), stream_ptr()), "mmf_gr_add_forward")
        ctx.cfg, ctx.ws, ctx.hidden = cfg, ws, hidden
        ctx.sinks = _sinks_of(params)
        ctx.cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        ctx.done_hook = getattr(params[0], "_immtsf_bwd_hook", None)
        ctx.save_for_backward(Y, E, M_u8, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        Y, E, M_u8, *params = ctx.saved_tensors
        dout = dout.contiguous()
        grads, rets = _grad_buffers(params, ctx.sinks)
        dY, dE = torch.empty_like(Y), torch.empty_like(E)
        sc = _bytes(lib.immtsf_mmf_gr_add_scratch_bytes(C.byref(ctx.cfg), ctx.hidden), Y.device)
        ps, gs = _struct(GRParams, params), _struct(GRParams, grads)
        check(lib.immtsf_mmf_gr_add_backward(C.byref(ctx.cfg), ctx.hidden, C.byref(ps), ptr(Y), ptr(E), ptr(M_u8), ptr(dout),
                                             ptr(dY), ptr(dE), ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs),
                                             stream_ptr()), "mmf_gr_add_backward")
        _fire(ctx.done_hook)
        return (dY, dE, None, None, None, None, None, None) + tuple(rets)


def gr_split_pw(T, Cc, d, hidden):
    """row pitch of MMF_GR_Add's split-form P for these dimensions, 0 where the split form does not apply (immtsf_mmf_gr_pw)"""
    cfg = make_cfg(1, 0, int(T), int(Cc), 0, int(d), 1, 0, False, 0.0, 0.0, 0, None)
    return int(_lib.load().immtsf_mmf_gr_pw(C.byref(cfg), int(hidden)))


class MMFGRPFn(torch.autograd.Function):
    """P half of MMF_GR_Add's split form (csrc/gr_train.hip): E_txt -> P (B, T, pw), the text columns of the GRU's input map and of the
    gate net (+ both biases).  Depends on the text side only; its backward yields dE_txt and the text columns of d W_ih / d W_g, d b_ih,
    d b_g (the Y columns come out of MMFGRQLossFn).  params: GRParams order."""

    @staticmethod
    def forward(ctx, E, Cc, hidden, precision, *params):
        lib = _lib.load()
        E = _c(E)
        params = tuple(_c(p) for p in params)
        _need_gpu(E, *params)
        B, T, d = E.shape
        cfg = make_cfg(B, 0, T, Cc, 0, d, 1, precision, False, 0.0, 0.0, 0, E.device)
        pw = int(lib.immtsf_mmf_gr_pw(C.byref(cfg), hidden))
        if pw <= 0:
            raise _lib.ImmtsfError("MMF_GR_Add split form: shape outside its limits")
        ws = _bytes(lib.immtsf_mmf_gr_p_workspace_bytes(C.byref(cfg), hidden), E.device)
        P = torch.empty(B, T, pw, dtype=torch.float32, device=E.device)
        E_h = _reg_take(_shadows, E) if _bf16_dataflow(precision, d) else None
        cfg.in_h = None if E_h is None else E_h.data_ptr()
        ps = _struct(GRParams, params)
        check(lib.immtsf_mmf_gr_p_forward(C.byref(cfg), hidden, C.byref(ps), ptr(E), ptr(P), ptr(ws), ws.numel(), stream_ptr()),
              "mmf_gr_p_forward")
        cfg.in_h = None
        ctx.cfg, ctx.ws, ctx.hidden, ctx.E_h = cfg, ws, hidden, E_h
        ctx.sinks = _sinks_of(params)
        ctx.save_for_backward(E, *params)
        return P

    @staticmethod
    def backward(ctx, dP):
        lib = _lib.load()
        E, *params = ctx.saved_tensors
        cfg = ctx.cfg
        dP = dP.contiguous()
        # the four gradients this half owns: w_ih (0), b_ih (2), gate_w (6), gate_b (7) -- the text columns of the two matrices only: a
        # sink is written in place (the other half adds its columns to the same buffer), otherwise a zero-filled full-size tensor each
        own = (0, 2, 6, 7)
        bufs, rets = [None] * 10, [None] * 10
        for i in own:
            if ctx.sinks[i] is not None:
                bufs[i] = ctx.sinks[i]
            else:
                bufs[i] = rets[i] = torch.zeros_like(params[i])
        dE = torch.empty_like(E)
        sc = _bytes(lib.immtsf_mmf_gr_p_scratch_bytes(C.byref(cfg), ctx.hidden), E.device)
        ps, gs = _struct(GRParams, params), _struct(GRParams, bufs)
        dE_h = None
        if _bf16_dataflow(cfg.precision, cfg.d):
            cfg.aux_h = None if ctx.E_h is None else ctx.E_h.data_ptr()
            dE_h = torch.empty(dE.shape, dtype=torch.bfloat16, device=dE.device)
            cfg.out_h = dE_h.data_ptr()
        check(lib.immtsf_mmf_gr_p_backward(C.byref(cfg), ctx.hidden, C.byref(ps), ptr(E), ptr(dP), ptr(dE), ptr(ctx.ws), ctx.ws.numel(), ptr(sc),
                                           sc.numel(), C.byref(gs), stream_ptr()), "mmf_gr_p_backward")
        cfg.aux_h = cfg.out_h = None
        if dE_h is not None:
            _reg_put(_shadows, dE, dE_h)
        _fire(getattr(params[0], "_immtsf_bwd_hook", None))      # (the block's gradients are final once THIS half's backward has run)
        return (dE, None, None, None) + tuple(rets)


class MMFGRQLossFn(torch.autograd.Function):
    """the Y half of MMF_GR_Add's split form + masked MSE (immtsf.ops.masked_mse with global_cnt) + the backward of both, ONE launch
    (immtsf_mmf_gr_q_train): the forward computes the loss and every gradient (seeded with 1); backward() hands them on.
    (Y_ts, P, M_txt, truth, mask, cnt, params...) -> loss."""

    @staticmethod
    def forward(ctx, Y, P, M_u8, truth, mask, cnt, hidden, p_drop, training, precision, seed, *params):
        lib = _lib.load()
        y_dense = Y.is_contiguous()
        Y, P, M_u8 = _c(Y), _c(P), _c(M_u8)
        truth, mask, cnt = _c(truth), _c(mask), _c(cnt.to(torch.float32))
        params = tuple(_c(p) for p in params)
        _need_gpu(Y, P, M_u8, truth, mask, cnt, *params)
        B, T, Cc = Y.shape
        d = params[0].shape[1] - Cc
        cfg = make_cfg(B, 0, T, Cc, 0, d, 1, precision, training, p_drop, 0.0, seed, Y.device)
        if int(lib.immtsf_mmf_gr_pw(C.byref(cfg), hidden)) != P.shape[2]:
            raise _lib.ImmtsfError("MMF_GR_Add split form: P does not have the row pitch of these dimensions")
        sinks = _sinks_of(params)
        # the eight gradients this half owns (w_ih and gate_w: their Y columns), ADDED into zeroed buffers: pre-zeroed sinks as they are
        own = (0, 1, 3, 4, 5, 6, 8, 9)
        bufs, rets = [None] * 10, [None] * 10
        for i in own:
            if sinks[i] is not None and getattr(params[i], "_immtsf_grad_prezeroed", False):
                bufs[i] = sinks[i]
            else:
                bufs[i] = rets[i] = torch.zeros_like(params[i])
        dY, dP = torch.empty_like(Y), torch.empty_like(P)
        loss = torch.empty((), dtype=torch.float32, device=Y.device)
        scratch = torch.empty(B, dtype=torch.float32, device=Y.device)
        # immtsf.train.FlagStep: dY_ts is published by the kernel itself
        flag = step_plan.current().take_head_flag(dY) if y_dense else None
        ps, gs = _struct(GRParams, params), _struct(GRParams, bufs)
        check(lib.immtsf_mmf_gr_q_train(C.byref(cfg), hidden, C.byref(ps), ptr(Y), ptr(P), ptr(M_u8), ptr(truth), ptr(mask), ptr(cnt), 1.0, None,
                                        ptr(loss), ptr(dY), ptr(dP), C.byref(gs), ptr(scratch), ptr(_xq_ticket(Y.device)[8:]), flag, stream_ptr()),
              "mmf_gr_q_train")
        ctx.grads = (dY, dP) + tuple(rets)
        ctx.sunk = tuple(bufs[i] for i in own if rets[i] is None)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        g = ctx.grads
        ctx.grads = None
        if not is_unit_grad(dloss):
            g = tuple(None if t is None else t * dloss for t in g)
            for b in ctx.sunk:
                b.mul_(dloss)
        ctx.sunk = ()
        return (g[0], g[1]) + (None,) * 9 + tuple(g[2:])


class MMFGRQFn(torch.autograd.Function):
    """the Y half of the split form, output only (inference / no_grad: immtsf_mmf_gr_q_train with truth == NULL)."""

    @staticmethod
    def forward(ctx, Y, P, M_u8, hidden, precision, *params):
        lib = _lib.load()
        Y, P, M_u8 = _c(Y), _c(P), _c(M_u8)
        params = tuple(_c(p) for p in params)
        _need_gpu(Y, P, M_u8, *params)
        B, T, Cc = Y.shape
        cfg = make_cfg(B, 0, T, Cc, 0, params[0].shape[1] - Cc, 1, precision, False, 0.0, 0.0, 0, Y.device)
        out = torch.empty_like(Y)
        ps = _struct(GRParams, params)
        check(lib.immtsf_mmf_gr_q_train(C.byref(cfg), hidden, C.byref(ps), ptr(Y), ptr(P), ptr(M_u8), None, None, None, 0.0, ptr(out), None, None,
                                        None, None, None, None, None, stream_ptr()), "mmf_gr_q_train")
        return out

    @staticmethod
    def backward(ctx, dout):
        raise RuntimeError("MMFGRQFn is the inference form of MMF_GR_Add's split path: training goes through MMFGRQLossFn or MMFGRAddFn")


# ------------------------------------------------------------------------------------------------ tPatchGNN TE + TTCN
class TTCNPatchEncodeFn(torch.autograd.Function):
    """(x, tt, mask: (P,L)) -> (P, ttcn_dim) or, with_flag, (P, ttcn_dim + 1) whose last column is the patch-non-empty
    flag (any mask > 0; no gradient).  params in immtsf_ttcn_params order."""

    @staticmethod
    def forward(ctx, x, tt, mask, precision, with_flag, *params):
        lib = _lib.load()
        x, tt, mask = _c(x), _c(tt), _c(mask)
        params = tuple(_c(p) for p in params)
        _need_gpu(x, tt, mask, *params)
        P, L = x.shape
        te_dim = params[2].numel() + 1
        K = params[10].numel()
        ld = K + 1 if with_flag else K
        out = torch.empty(P, ld, dtype=torch.float32, device=x.device)
        ws = _bytes(lib.immtsf_ttcn_workspace_bytes(P, L, te_dim, K), x.device)
        ps = _struct(TTCNParams, params)
        check(lib.immtsf_ttcn_forward(P, L, te_dim, K, precision, ptr(x), ptr(tt), ptr(mask), C.byref(ps), ptr(out), ld,
                                      K if with_flag else -1, ptr(ws), ws.numel(), stream_ptr()), "ttcn_forward")
        ctx.dims = (P, L, te_dim, K, precision, ld)
        ctx.ws = ws
        ctx.sinks = _sinks_of(params)
        _claim_sinks(params[:4], ctx.sinks[:4], "ttcn_patch_encode")
        ctx.save_for_backward(x, tt, mask, out, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, tt, mask, out, *params = ctx.saved_tensors
        P, L, te_dim, K, precision, ld = ctx.dims
        dout = dout.contiguous()
        te_acc = _shared(params[:4], ctx.sinks[:4])       # time-embedding parameters shared with the decoder's LearnableTE
        grads, rets = _grad_buffers(params, ctx.sinks)
        sc = _bytes(lib.immtsf_ttcn_scratch_bytes(P, L, te_dim, K), x.device)
        ps, gs = _struct(TTCNParams, params), _struct(TTCNParams, grads)
        # parameter gradients only, chip-filling, nothing but the optimizer waits for them: go behind the text side's row-bound
        # backward kernels (a hint: the spin gives up after 50 ms and the call proceeds)
        step_plan.current().wait_gate()
        check(lib.immtsf_ttcn_backward(P, L, te_dim, K, precision, ptr(x), ptr(tt), ptr(mask), C.byref(ps), ptr(out), ptr(dout), ld,
                                       ptr(ctx.ws), ctx.ws.numel(), ptr(sc), sc.numel(), C.byref(gs), 1 if te_acc else 0, stream_ptr()),
              "ttcn_backward")
        return (None, None, None, None, None) + tuple(rets)


def ttcn_patch_encode(x, tt, mask, te_scale_w, te_scale_b, te_per_w, te_per_b, W1, b1, W2, b2, W3, b3, T_bias, precision=None,
                      with_flag=False):
    """Fused LearnableTE + TTCN of tPatchGNN (models/tPatchGNN.py:176-195) on (P, L) patch tensors; with_flag appends
    the patch-non-empty column of :268-270."""
    return TTCNPatchEncodeFn.apply(x.float(), tt.float(), mask.float(), config.precision_code(precision), bool(with_flag),
                                   te_scale_w, te_scale_b, te_per_w, te_per_b, W1, b1, W2, b2, W3, b3, T_bias)


def patch_flatten3(X, tt, mask):
    """X, tt, mask (B, M, L, N) data tensors (no gradient) -> three (B*N*M, L) tensors, the patch rows of tPatchGNN's encoder
    (models/tPatchGNN.py:271-275), in one launch instead of three permute copies."""
    lib = _lib.load()
    X, tt, mask = _c(X.float()), _c(tt.float()), _c(mask.float())
    _need_gpu(X, tt, mask)
    B, M, L, N = X.shape
    out = torch.empty(3, B * N * M, L, dtype=torch.float32, device=X.device)
    check(lib.immtsf_patch_flatten3(ptr(X), ptr(tt), ptr(mask), B, M, L, N, ptr(out[0]), ptr(out[1]), ptr(out[2]), stream_ptr()),
          "patch_flatten3")
    return out[0], out[1], out[2]


class GCNAdaptiveFn(torch.autograd.Function):
    """tPatchGNN's adaptive-graph stage on (B,N,M,D): one workgroup per (window, patch) cell, params in
    immtsf_gcn_params order.  Backward recomputes the cell in LDS; parameter gradients accumulate by atomics into one
    zeroed flat buffer whose slices are returned."""

    @staticmethod
    def forward(ctx, x, order, *params):
        lib = _lib.load()
        x = _c(x)
        params = tuple(_c(p) for p in params)
        _need_gpu(x, *params)
        B, N, M, D = x.shape
        nd = params[0].shape[1]
        out = torch.empty_like(x)
        ps = _struct(GCNParams, params)
        ctx.dims = (B, N, M, D, nd, order)
        ctx.sinks = _sinks_of(params)
        if any(ctx.needs_input_grad):
            # a training forward leaves every cell's intermediates for the backward (5 KB per cell) instead of having it recompute them
            saved = torch.empty(lib.immtsf_tpatchgnn_gcn_saved_floats(B, N, M, D, nd, order), dtype=torch.float32, device=x.device)
            check(lib.immtsf_tpatchgnn_gcn_forward_saved(B, N, M, D, nd, order, ptr(x), C.byref(ps), ptr(out), ptr(saved), stream_ptr()),
                  "tpatchgnn_gcn_forward_saved")
            ctx.save_for_backward(saved, *params)
        else:
            check(lib.immtsf_tpatchgnn_gcn_forward(B, N, M, D, nd, order, ptr(x), C.byref(ps), ptr(out), stream_ptr()),
                  "tpatchgnn_gcn_forward")
            ctx.save_for_backward(x, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        saved, *params = ctx.saved_tensors
        B, N, M, D, nd, order = ctx.dims
        dout = dout.contiguous()
        dx = torch.empty_like(dout)
        grads, rets = _zeroed_grad_buffers(params, ctx.sinks)
        ps, gs = _struct(GCNParams, params), _struct(GCNParams, grads)
        check(lib.immtsf_tpatchgnn_gcn_backward_saved(B, N, M, D, nd, order, ptr(saved), C.byref(ps), ptr(dout), ptr(dx), C.byref(gs),
                                                      stream_ptr()), "tpatchgnn_gcn_backward_saved")
        return (dx, None) + tuple(rets)


def gcn_adaptive_supported(N, D, nd, order):
    return _lib.load().immtsf_tpatchgnn_gcn_lds_bytes(N, D, nd, order) > 0


def gcn_adaptive(x, order, nodevec1, nodevec2, gate1, gate2, lin1, lin2, mlp_conv):
    """x (B,N,M,D) -> (B,N,M,D); gate*: nn.Linear(D+nd,1), lin*: nn.Linear(D,nd), mlp_conv: the 1x1 nn.Conv2d."""
    return GCNAdaptiveFn.apply(x.float(), int(order), nodevec1, nodevec2, gate1.weight, gate1.bias, gate2.weight, gate2.bias,
                               lin1.weight, lin1.bias, lin2.weight, lin2.bias, mlp_conv.weight, mlp_conv.bias)


class EncoderLayerFn(torch.autograd.Function):
    """immtsf_encoder_layer_forward/backward: nn.TransformerEncoderLayer (post-norm, relu, batch_first) over short sequences,
    params in immtsf_encoder_layer_params order.  7 launches forward, 15 backward (csrc/encoder_layer.hip)."""

    @staticmethod
    def forward(ctx, x, H, p_attn, p_drop, eps, training, precision, seed, site_base, *params):
        lib = _lib.load()
        x = _c(x)
        params = tuple(_c(p) for p in params)
        _need_gpu(x, *params)
        Bs, S, D = x.shape
        F = params[6].shape[0]
        p_on = training and (p_attn > 0 or p_drop > 0)
        cfg = _lib.EncoderLayerCfg(Bs, S, D, int(H), F, precision, 1 if training else 0, float(p_attn), float(p_drop), float(eps),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, config.dropout_counter_ptr(x.device) if p_on else None,
                                   int(site_base), 0)
        ws = _bytes(lib.immtsf_encoder_layer_workspace_bytes(C.byref(cfg)), x.device)
        out = torch.empty_like(x)
        ps = _struct(_lib.EncoderLayerParams, params)
        check(lib.immtsf_encoder_layer_forward(C.byref(cfg), C.byref(ps), ptr(x), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "encoder_layer_forward")
        ctx.cfg, ctx.ws = cfg, ws
        ctx.sinks = _sinks_of(params)
        ctx.save_for_backward(x, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, *params = ctx.saved_tensors
        cfg = ctx.cfg
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        grads, rets = _grad_buffers(params, ctx.sinks)
        cfg.grads_prezeroed = _prezeroed(params, ctx.sinks)
        sc = _bytes(lib.immtsf_encoder_layer_scratch_bytes(C.byref(cfg)), x.device)
        ps, gs = _struct(_lib.EncoderLayerParams, params), _struct(_lib.EncoderLayerParams, grads)
        check(lib.immtsf_encoder_layer_backward(C.byref(cfg), C.byref(ps), ptr(x), ptr(dout), ptr(dx), ptr(ctx.ws), ctx.ws.numel(),
                                                ptr(sc), sc.numel(), C.byref(gs), stream_ptr()), "encoder_layer_backward")
        ctx.ws = None
        return (dx,) + (None,) * 8 + tuple(rets)


def encoder_layer_supported(S, D, H):
    return S <= 8 and D % 4 == 0 and D <= 1024 and D % H == 0 and (D // H) <= 64 and (D // H) % 4 == 0


def encoder_layer(lyr, x, training, site_base, precision=None):
    """lyr: an nn.TransformerEncoderLayer (post-norm, relu, batch_first); x (Bs, S, D)"""
    at = lyr.self_attn
    p_attn, p_drop = float(at.dropout), float(lyr.dropout.p)
    seed = config.next_seed() if training and (p_attn > 0 or p_drop > 0) else 0
    return EncoderLayerFn.apply(x.float(), at.num_heads, p_attn, p_drop, lyr.norm1.eps, bool(training), config.precision_code(precision),
                                seed, site_base, at.in_proj_weight, at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
                                lyr.norm1.weight, lyr.norm1.bias, lyr.linear1.weight, lyr.linear1.bias, lyr.linear2.weight,
                                lyr.linear2.bias, lyr.norm2.weight, lyr.norm2.bias)


class ResidualLayerNormFn(torch.autograd.Function):
    """out = LayerNorm(x + Dropout(branch)) in one kernel per direction (+ the two-parameter column sums backward)."""

    @staticmethod
    def forward(ctx, x, branch, gamma, beta, eps, p_drop, training, seed, site):
        lib = _lib.load()
        x2, b2 = _c(x).reshape(-1, x.shape[-1]), _c(branch).reshape(-1, x.shape[-1])
        _need_gpu(x2, b2, gamma, beta)
        rows, d = x2.shape
        p = float(p_drop) if training else 0.0
        cnt = config.dropout_counter_ptr(x.device) if p > 0 else None
        xhat = torch.empty_like(x2)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        check(lib.immtsf_residual_layernorm_forward(ptr(x2), ptr(b2), rows, d, ptr(gamma), ptr(beta), float(eps), 1 if training else 0, p,
                                                    seed, site, cnt, ptr(xhat), ptr(rstd), ptr(out), stream_ptr()), "residual_layernorm_forward")
        ctx.save_for_backward(xhat, rstd, gamma)
        ctx.cfg = (rows, d, 1 if training else 0, p, seed, site, cnt, x.shape)
        ctx.sinks = _sinks_of((gamma, beta))
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        xhat, rstd, gamma = ctx.saved_tensors
        rows, d, tr, p, seed, site, cnt, shape = ctx.cfg
        g = dout.contiguous()
        dx, db = torch.empty_like(xhat), torch.empty_like(xhat)
        (dgamma, dbeta), rets = _grad_buffers((gamma, gamma), ctx.sinks)
        scratch = torch.empty(64 * (d + 8), dtype=torch.float32, device=g.device)
        check(lib.immtsf_residual_layernorm_backward(ptr(g), rows, d, ptr(gamma), ptr(xhat), ptr(rstd), tr, p, seed, site, cnt, ptr(dx),
                                                     ptr(db), ptr(dgamma), ptr(dbeta), ptr(scratch), stream_ptr()), "residual_layernorm_backward")
        return dx.view(shape), db.view(shape), rets[0], rets[1], None, None, None, None, None


def residual_layernorm_supported(d):
    return d % 4 == 0 and d <= 1024


def residual_layer_norm(x, branch, norm, p_drop, training, site):
    """norm: an nn.LayerNorm; x, branch (..., d)"""
    seed = config.next_seed() if training and p_drop > 0 else 0
    return ResidualLayerNormFn.apply(x.float(), branch.float(), norm.weight, norm.bias, norm.eps, float(p_drop), bool(training), seed, site)


class FFNBlockFn(torch.autograd.Function):
    """immtsf_ffn_block_forward/backward: out = LayerNorm(x + Dropout(W2 Dropout(act(W1 x + b1)) + b2)); W1 / W2 may be the
    (out, in, 1) weights of kernel-size-1 nn.Conv1d modules (same memory as (out, in))."""

    @staticmethod
    def forward(ctx, x, act, p_drop, eps, training, precision, seed, site_base, *params):
        lib = _lib.load()
        x2 = _c(x).reshape(-1, x.shape[-1])
        params = tuple(_c(p) for p in params)
        _need_gpu(x2, *params)
        R, D = x2.shape
        F = params[0].shape[0]
        p = float(p_drop) if training else 0.0
        cfg = _lib.FFNBlockCfg(R, D, F, int(act), precision, 1 if training else 0, p, float(eps), int(seed) & 0xFFFFFFFFFFFFFFFF,
                               config.dropout_counter_ptr(x.device) if p > 0 else None, int(site_base), 0)
        ws = _bytes(lib.immtsf_ffn_block_workspace_bytes(C.byref(cfg)), x.device)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ps = _struct(_lib.FFNBlockParams, params)
        check(lib.immtsf_ffn_block_forward(C.byref(cfg), C.byref(ps), ptr(x2), ptr(out), ptr(ws), ws.numel(), stream_ptr()), "ffn_block_forward")
        ctx.cfg, ctx.ws, ctx.shape = cfg, ws, x.shape
        ctx.sinks = _sinks_of(params)
        ctx.save_for_backward(x2, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x2, *params = ctx.saved_tensors
        cfg = ctx.cfg
        dout = dout.contiguous()
        dx = torch.empty_like(x2)
        grads, rets = _grad_buffers(params, ctx.sinks)
        pz = _prezeroed(params, ctx.sinks)
        cfg.grads_prezeroed = pz
        sc = _bytes(lib.immtsf_ffn_block_scratch_bytes(C.byref(cfg)), x2.device)
        ps, gs = _struct(_lib.FFNBlockParams, params), _struct(_lib.FFNBlockParams, grads)
        ws = ctx.ws
        ctx.ws = None

        def call(bits, stream):
            cfg.grads_prezeroed = pz | bits
            rc = lib.immtsf_ffn_block_backward(C.byref(cfg), C.byref(ps), ptr(x2), ptr(dout), ptr(dx), ptr(ws), ws.numel(), ptr(sc), sc.numel(),
                                               C.byref(gs), stream)
            cfg.grads_prezeroed = pz
            return rc
        # a step with a parameter-only branch (immtsf.train.FlagStep): the two weight-gradient products leave this stream's dependent chain
        # (LinearBf16Fn.backward has the why); only when every gradient goes straight to a pre-zeroed sink and the library takes the phases
        plan = step_plan.current()
        if pz and plan.wgrad_open and all(r is None for r in rets):
            rc = call(2, stream_ptr())
            if rc == 0:
                plan.defer_wgrad(lambda stream: check(call(4, stream), "ffn_block_backward"),
                                 keep=(x2, dout, dx, ws, sc, params, grads, ps, gs))
                return (dx.view(ctx.shape),) + (None,) * 7 + tuple(rets)
            if rc != -3:          # (IMMTSF_EUNSUPPORTED: nothing was launched -- the one-call form below)
                check(rc, "ffn_block_backward")
        check(call(0, stream_ptr()), "ffn_block_backward")
        return (dx.view(ctx.shape),) + (None,) * 7 + tuple(rets)


def ffn_block(x, conv1, conv2, norm, act, p_drop, training, site_base, precision=None):
    """conv1 / conv2: nn.Conv1d(kernel_size=1) or nn.Linear; norm: nn.LayerNorm; act: "relu" | "gelu"."""
    seed = config.next_seed() if training and p_drop > 0 else 0
    return FFNBlockFn.apply(x.float(), 1 if act == "relu" else 2, float(p_drop), norm.eps, bool(training), config.precision_code(precision),
                            seed, site_base, conv1.weight, conv1.bias, conv2.weight, conv2.bias, norm.weight, norm.bias)


def _ptr_array(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


class InceptionMergeFn(torch.autograd.Function):
    """(W_0 .. W_{n-1}, b_0 .. b_{n-1}) of an Inception_Block_V1 (kernel sizes 1, 3, .., 2n-1) -> the ONE averaged kernel as a
    GEMM weight W_eff (Cout, KS*KS*Cin) and bias b_eff (immtsf_inception_merge / _unmerge)."""

    @staticmethod
    def forward(ctx, n, *wb):
        lib = _lib.load()
        ws, bs = [_c(t) for t in wb[:n]], [_c(t) for t in wb[n:]]
        _need_gpu(*ws, *bs)
        Cout, Cin = ws[0].shape[0], ws[0].shape[1]
        KS = 2 * n - 1
        Weff = torch.empty(Cout, KS * KS * Cin, dtype=torch.float32, device=ws[0].device)
        beff = torch.empty(Cout, dtype=torch.float32, device=ws[0].device)
        check(lib.immtsf_inception_merge(n, Cin, Cout, _ptr_array(ws), _ptr_array(bs), ptr(Weff), ptr(beff), stream_ptr()), "inception_merge")
        ctx.dims = (n, Cin, Cout)
        ctx.shapes = [w.shape for w in ws] + [b.shape for b in bs]
        ctx.sinks = _sinks_of(wb)
        ctx.params = wb            # parameters (not saved tensors: only their sinks / shapes are needed)
        return Weff, beff

    @staticmethod
    def backward(ctx, dW, db):
        lib = _lib.load()
        n, Cin, Cout = ctx.dims
        grads, rets = _grad_buffers(ctx.params, ctx.sinks)
        ctx.params = None
        check(lib.immtsf_inception_unmerge(n, Cin, Cout, ptr(dW.contiguous()), ptr(db.contiguous()), _ptr_array(grads[:n]), _ptr_array(grads[n:]),
                                           stream_ptr()), "inception_unmerge")
        return (None,) + tuple(rets)


class Conv2dSameCLFn(torch.autograd.Function):
    """y (B,H,W,Cout) = act(conv2d_same(x (B,H,W,Cin), W_eff) + b_eff) on channels-last images: im2col + MFMA GEMM
    (immtsf_conv2d_same_cl_forward/backward); act 0 none, 2 GELU."""

    @staticmethod
    def forward(ctx, x, Weff, beff, KS, act, precision):
        lib = _lib.load()
        x, Weff, beff = _c(x), _c(Weff), _c(beff)
        _need_gpu(x, Weff, beff)
        B, H, W, Cin = x.shape
        Cout = Weff.shape[0]
        rows, K = B * H * W, KS * KS * Cin
        col = torch.empty(rows, K, dtype=torch.float32, device=x.device)
        z = torch.empty(rows, Cout, dtype=torch.float32, device=x.device) if act == 2 else None
        y = torch.empty(B, H, W, Cout, dtype=torch.float32, device=x.device)
        check(lib.immtsf_conv2d_same_cl_forward(precision, ptr(x), B, H, W, Cin, KS, ptr(Weff), ptr(beff), Cout, act, ptr(col), ptr(z), ptr(y),
                                                stream_ptr()), "conv2d_same_cl_forward")
        ctx.save_for_backward(col, z, Weff)
        ctx.dims = (B, H, W, Cin, KS, Cout, act, precision)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        col, z, Weff = ctx.saved_tensors
        B, H, W, Cin, KS, Cout, act, precision = ctx.dims
        rows, K = B * H * W, KS * KS * Cin
        dy = dy.contiguous()
        dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(Weff)
        db = torch.empty(Cout, dtype=torch.float32, device=dy.device)
        scratch = torch.empty(lib.immtsf_conv2d_same_cl_scratch_floats(B, H, W, Cin, KS, Cout), dtype=torch.float32, device=dy.device)
        check(lib.immtsf_conv2d_same_cl_backward(precision, ptr(col), ptr(z), None, ptr(dy), B, H, W, Cin, KS, ptr(Weff), Cout, act, ptr(dx),
                                                 ptr(dW), ptr(db), ptr(scratch), stream_ptr()), "conv2d_same_cl_backward")
        return dx, dW, db, None, None, None


class Conv2dPeriodFn(torch.autograd.Function):
    """Conv2dSameCLFn on a TimesNet period image whose period lives ON THE DEVICE (immtsf_conv2d_period_forward / _backward): x, y are
    position-major (Lmax * B, C) matrices (row l * B + b), `period` / `rows` one device int32 each (ops.period_rows).  Every shape on the
    host is static, so the step can be captured into a hipGraph; rows beyond `rows` are neither read nor written."""

    @staticmethod
    def forward(ctx, x, period, rows, Weff, beff, KS, act, precision, B, Lmax, w16):
        lib = _lib.load()
        x, Weff, beff = _c(x), _c(Weff), _c(beff)
        _need_gpu(x, Weff, beff)
        Cin, Cout = x.shape[1], Weff.shape[0]
        R, K = B * Lmax, KS * KS * Cin
        hf = precision == 1 and Cin % 8 == 0 and Cout % 8 == 0      # bf16 mode: the im2col image as bf16, the products on the bf16-in-HBM kernels
        col = torch.empty(R, K, dtype=torch.bfloat16 if hf else torch.float32, device=x.device)
        ready = 1 if (hf and w16 is not None) else 0                # (the kernel's bf16 image, cast once by the caller for all periods)
        if hf and w16 is None:
            w16 = torch.empty(Cout, K, dtype=torch.bfloat16, device=x.device)
        if not hf:
            w16 = None
        z = torch.empty(R, Cout, dtype=torch.float32, device=x.device) if act == 2 else None
        y = torch.empty(R, Cout, dtype=torch.float32, device=x.device)
        check(lib.immtsf_conv2d_period_forward(precision, ptr(x), B, Lmax, ptr(period), ptr(rows), Cin, KS, ptr(Weff), ptr(beff), Cout, act,
                                               ptr(col), ptr(z), ptr(y), ptr(w16), ready, stream_ptr()), "conv2d_period_forward")
        ctx.hf = hf
        ctx.save_for_backward(col, z, Weff, period, rows)
        ctx.dims = (B, Lmax, Cin, KS, Cout, act, precision)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        col, z, Weff, period, rows = ctx.saved_tensors
        B, Lmax, Cin, KS, Cout, act, precision = ctx.dims
        dy = dy.contiguous()
        # (rows beyond the image are never written: whoever consumes dx -- the previous period convolution, the slice that crops the
        # series -- never reads them either)
        dx = torch.empty(B * Lmax, Cin, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(Weff)
        db = torch.empty(Cout, dtype=torch.float32, device=dy.device)
        scratch = torch.empty(lib.immtsf_conv2d_period_scratch_floats(B, Lmax, Cin, KS, Cout), dtype=torch.float32, device=dy.device)
        w16 = torch.empty(1, dtype=torch.bfloat16, device=dy.device) if ctx.hf else None       # (only says "the bf16 path": images live in scratch)
        check(lib.immtsf_conv2d_period_backward(precision, ptr(col), ptr(z), ptr(dy), B, Lmax, ptr(period), ptr(rows), Cin, KS, ptr(Weff), Cout,
                                                act, ptr(dx), ptr(dW), ptr(db), ptr(scratch), ptr(w16), stream_ptr()), "conv2d_period_backward")
        return dx, None, None, dW, db, None, None, None, None, None, None


class Conv2dPeriodsFn(torch.autograd.Function):
    """Conv2dPeriodFn for the k period images of a TimesBlock in ONE call (immtsf_conv2d_periods_forward / _backward): x is one input shared
    by every image, (R, Cin), or one per image, (k, R, Cin); y (k, R, Cout).  In bf16 mode the images ride along grid.z of one im2col and
    one product launch per direction; the kernel's gradient is the sum over the images, accumulated in place."""

    @staticmethod
    def forward(ctx, x, period, rows, Weff, beff, KS, act, precision, B, Lmax):
        lib = _lib.load()
        x, Weff, beff = _c(x), _c(Weff), _c(beff)
        _need_gpu(x, Weff, beff)
        k = period.numel()
        shared = x.dim() == 2
        Cin, Cout = x.shape[-1], Weff.shape[0]
        R, K = B * Lmax, KS * KS * Cin
        hf = precision == 1 and Cin % 8 == 0 and Cout % 8 == 0
        col = torch.empty(k, R, K, dtype=torch.bfloat16 if hf else torch.float32, device=x.device)
        w16 = torch.empty(Cout, K, dtype=torch.bfloat16, device=x.device) if hf else None
        z = torch.empty(k, R, Cout, dtype=torch.float32, device=x.device) if act == 2 else None
        y = torch.empty(k, R, Cout, dtype=torch.float32, device=x.device)
        check(lib.immtsf_conv2d_periods_forward(precision, ptr(x), 0 if shared else R * Cin, B, Lmax, k, ptr(period), ptr(rows), Cin, KS, ptr(Weff),
                                                ptr(beff), Cout, act, ptr(col), ptr(z), ptr(y), ptr(w16), 0, stream_ptr()), "conv2d_periods_forward")
        ctx.hf, ctx.shared = hf, shared
        ctx.save_for_backward(col, z, Weff, period, rows)
        ctx.dims = (B, Lmax, Cin, KS, Cout, act, precision, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        col, z, Weff, period, rows = ctx.saved_tensors
        B, Lmax, Cin, KS, Cout, act, precision, k = ctx.dims
        dy = dy.contiguous()
        R = B * Lmax
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((R, Cin) if ctx.shared else (k, R, Cin), dtype=torch.float32, device=dy.device)
        acc = torch.zeros(Weff.numel() + Cout, dtype=torch.float32, device=dy.device)      # dW | db: the images add into it
        dW, db = acc[:Weff.numel()].view_as(Weff), acc[Weff.numel():]
        scratch = torch.empty(lib.immtsf_conv2d_periods_scratch_floats(B, Lmax, k, Cin, KS, Cout), dtype=torch.float32, device=dy.device)
        w16 = torch.empty(1, dtype=torch.bfloat16, device=dy.device) if ctx.hf else None
        check(lib.immtsf_conv2d_periods_backward(precision, ptr(col), ptr(z), ptr(dy), B, Lmax, k, ptr(period), ptr(rows), Cin, KS, ptr(Weff), Cout,
                                                 act, ptr(dx), 1 if ctx.shared else 0, ptr(dW), ptr(db), ptr(scratch), ptr(w16), stream_ptr()),
              "conv2d_periods_backward")
        return dx, None, None, dW, db, None, None, None, None, None


class InceptionPeriodsFn(torch.autograd.Function):
    """An Inception_Block_V1 (layers/Conv_Blocks.py:8-31: the mean of n same-padded convolutions, kernel sizes 1, 3, .., 2n-1) over the k
    period images of a TimesBlock in the IMPLICIT form (csrc/conv.hip conv_period_mfma_kernel: no im2col image, a workgroup holds a
    (window, period) image in LDS): merge of the n kernels, the convolution (+ GELU), and backward the data gradient through the same
    kernel, the merged kernel's gradient from an im2col image of the INPUT formed only for that product, and the un-merge into the n
    kernels' gradients.  With a parameter branch (immtsf.train.FlagStep) and gradient sinks the kernel-gradient half runs there.
    args: x (R, Cin) shared or (k, R, Cin), period, rows, act, precision, B, Lmax, n, W_0..W_{n-1}, b_0..b_{n-1}."""

    @staticmethod
    def forward(ctx, x, period, rows, act, precision, B, Lmax, n, *wb):
        lib = _lib.load()
        x = _c(x)
        ws, bs = [_c(t) for t in wb[:n]], [_c(t) for t in wb[n:]]
        _need_gpu(x, *ws, *bs)
        k = period.numel()
        shared = x.dim() == 2
        Cout, Cin = ws[0].shape[0], ws[0].shape[1]
        KS = 2 * n - 1
        R, K = B * Lmax, KS * KS * Cin
        dev = x.device
        Weff = torch.empty(Cout, K, dtype=torch.float32, device=dev)
        beff = torch.empty(Cout, dtype=torch.float32, device=dev)
        check(lib.immtsf_inception_merge(n, Cin, Cout, _ptr_array(ws), _ptr_array(bs), ptr(Weff), ptr(beff), stream_ptr()), "inception_merge")
        w16 = torch.empty(Cout, K, dtype=torch.bfloat16, device=dev)
        z = torch.empty(k, R, Cout, dtype=torch.float32, device=dev) if act == 2 else None
        y = torch.empty(k, R, Cout, dtype=torch.float32, device=dev)
        check(lib.immtsf_conv2d_periods_forward(precision, ptr(x), 0 if shared else R * Cin, B, Lmax, k, ptr(period), ptr(rows), Cin, KS, ptr(Weff),
                                                ptr(beff), Cout, act, None, ptr(z), ptr(y), ptr(w16), 0, stream_ptr()), "conv2d_periods_forward")
        ctx.shared = shared
        ctx.save_for_backward(x, z, Weff, period, rows)
        ctx.dims = (B, Lmax, Cin, KS, Cout, act, precision, k, n)
        ctx.sinks = _sinks_of(wb)
        ctx.params = wb
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, z, Weff, period, rows = ctx.saved_tensors
        B, Lmax, Cin, KS, Cout, act, precision, k, n = ctx.dims
        dy = dy.contiguous()
        R = B * Lmax
        dev = dy.device
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((R, Cin) if ctx.shared else (k, R, Cin), dtype=torch.float32, device=dev)
        acc = torch.zeros(Weff.numel() + Cout, dtype=torch.float32, device=dev)      # d W_eff | d b_eff: the images add into it
        dW, db = acc[:Weff.numel()].view_as(Weff), acc[Weff.numel():]
        scratch = torch.empty(lib.immtsf_conv2d_periods_backward_x_scratch_floats(B, Lmax, k, Cin, KS, Cout), dtype=torch.float32, device=dev)
        grads, rets = _grad_buffers(ctx.params, ctx.sinks)
        ctx.params = None
        xs = 0 if ctx.shared else R * Cin

        def call(phase, stream):
            check(lib.immtsf_conv2d_periods_backward_x(precision, ptr(x), xs, ptr(z), ptr(dy), B, Lmax, k, ptr(period), ptr(rows), Cin, KS, ptr(Weff),
                                                       Cout, act, ptr(dx), 1 if ctx.shared else 0, ptr(dW), ptr(db), ptr(scratch), phase, stream),
                  "conv2d_periods_backward_x")

        def wgrad(stream, keep=(x, z, dy, Weff, acc, scratch, grads)):
            call(2, stream)
            check(lib.immtsf_inception_unmerge(n, Cin, Cout, ptr(dW), ptr(db), _ptr_array(grads[:n]), _ptr_array(grads[n:]), stream),
                  "inception_unmerge")
        call(1, stream_ptr())
        # a step with a parameter-only branch: the kernels' gradients -- an im2col image, the summed product, the un-merge; nothing in the
        # backward waits for them -- leave this stream's dependent chain (needs every kernel on a gradient sink: nothing is returned)
        plan = step_plan.current()
        if plan.wgrad_open and all(r is None for r in rets):
            plan.defer_wgrad(wgrad)
        else:
            wgrad(stream_ptr())
        return (dx,) + (None,) * 7 + tuple(rets)


def inception_periods_ok(block, Lmax, precision=None):
    """True where InceptionPeriodsFn applies to this Inception_Block_V1 (immtsf_conv2d_periods_implicit_ok: bf16 mode, channel counts
    multiples of 8 up to 64, Lmax <= 128)"""
    n = len(block.kernels)
    if n > INCEPTION_MAX or not block.kernels[0].weight.is_cuda:
        return False
    Cout, Cin = block.kernels[0].weight.shape[:2]
    return bool(_lib.load().immtsf_conv2d_periods_implicit_ok(config.precision_code(precision), int(Lmax), int(Cin), 2 * n - 1, int(Cout)))


def inception_periods(x, period, rows, block, B, Lmax, act=None, precision=None):
    ks = block.kernels
    return InceptionPeriodsFn.apply(x.float(), period, rows, 2 if act == "gelu" else 0, config.precision_code(precision), int(B), int(Lmax),
                                    len(ks), *[c.weight for c in ks], *[c.bias for c in ks])


class PeriodAggregateFn(torch.autograd.Function):
    """TimesBlock's aggregation of the k period images and its residual as one launch (immtsf_period_aggregate_forward / _backward):
    (Y (k, Lmax*B, N) position-major, w (B, k) softmax weights, x (B, total, N)) -> x + sum_j w[:, j] Y_j cropped to `total` steps."""

    @staticmethod
    def forward(ctx, Y, w, x, B, total, Lmax):
        lib = _lib.load()
        Y, w, x = _c(Y), _c(w), _c(x)
        _need_gpu(Y, w, x)
        k, N = Y.shape[0], Y.shape[2]
        out = torch.empty_like(x)
        check(lib.immtsf_period_aggregate_forward(ptr(Y), ptr(w), ptr(x), B, total, Lmax, N, k, ptr(out), stream_ptr()), "period_aggregate_forward")
        ctx.save_for_backward(Y, w)
        ctx.dims = (B, total, Lmax, N, k)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        Y, w = ctx.saved_tensors
        B, total, Lmax, N, k = ctx.dims
        dout = dout.contiguous()
        dY, dw = torch.empty_like(Y), torch.empty_like(w)
        check(lib.immtsf_period_aggregate_backward(ptr(Y), ptr(w), ptr(dout), B, total, Lmax, N, k, ptr(dY), ptr(dw), stream_ptr()),
              "period_aggregate_backward")
        return dY, dw, dout, None, None, None


def conv2d_periods(x, period, rows, Weff, beff, KS, B, Lmax, act=None, precision=None):
    return Conv2dPeriodsFn.apply(x.float(), period, rows, Weff, beff, int(KS), 2 if act == "gelu" else 0, config.precision_code(precision),
                                 int(B), int(Lmax))


def period_aggregate(Y, w, x, B, total, Lmax):
    return PeriodAggregateFn.apply(Y, w.float(), x.float(), int(B), int(total), int(Lmax))


def period_rows(top, total, B):
    """top (k int64 device values: TimesNet's selected frequency indices) -> (period int32 (k), rows int32 (k)) on the device: period =
    total // top, rows = B * (total rounded up to a multiple of the period) -- models/TimesNet.py:17-18, 50-56 without the host read"""
    k = top.numel()
    period = torch.empty(k, dtype=torch.int32, device=top.device)
    rows = torch.empty(k, dtype=torch.int32, device=top.device)
    check(_lib.load().immtsf_period_rows(ptr(_c(top)), k, int(total), int(B), ptr(period), ptr(rows), stream_ptr()), "period_rows")
    return period, rows


# ---- TimesNet's period selection without an FFT library (csrc/timesnet_spectrum.hip) ----------------------------------------------------
def timesnet_spectrum_ok(T, N, k):
    """the shapes the spectrum kernels take (immtsf_timesnet_spectrum_ok): 2 <= T <= 512, 1 <= N <= 256, T N <= 16384, 1 <= k <=
    min(16, T // 2)"""
    return bool(_lib.load().immtsf_timesnet_spectrum_ok(int(T), int(N), int(k)))


def _spectrum_forward(x, k):
    """the two forward launches on x (B, T, N): -> (amp_mean (B, F), freq (F), top (k) int64, period (k) int32, rows (k) int32, weight (B, k),
    w (B, k), xl (2T B, N))"""
    if x.dim() != 3:
        raise _lib.ImmtsfError(f"timesnet_spectrum: x (B, T, N), got {tuple(x.shape)}")
    _need_gpu(x)
    if x.dtype != torch.float32:
        raise _lib.ImmtsfError(f"timesnet_spectrum: x is {x.dtype}; the kernels are fp32 in every precision mode")
    B, T, N = x.shape
    k = int(k)
    if B < 1 or not timesnet_spectrum_ok(T, N, k):
        raise _lib.ImmtsfError(f"timesnet_spectrum: B {B}, T {T}, N {N}, k {k} is outside timesnet_spectrum_ok")
    lib = _lib.load()
    dev, F = x.device, T // 2 + 1
    amp_mean = torch.empty(B, F, dtype=torch.float32, device=dev)
    freq = torch.empty(F, dtype=torch.float32, device=dev)
    xl = torch.empty(2 * T * B, N, dtype=torch.float32, device=dev)
    top = torch.empty(k, dtype=torch.int64, device=dev)
    period = torch.empty(k, dtype=torch.int32, device=dev)
    rows = torch.empty(k, dtype=torch.int32, device=dev)
    weight = torch.empty(B, k, dtype=torch.float32, device=dev)
    w = torch.empty(B, k, dtype=torch.float32, device=dev)
    check(lib.immtsf_timesnet_spectrum_fwd(ptr(x), B, T, N, ptr(amp_mean), ptr(xl), stream_ptr()), "timesnet_spectrum_fwd")
    check(lib.immtsf_timesnet_spectrum_select(ptr(amp_mean), B, T, k, ptr(freq), ptr(top), ptr(period), ptr(rows), ptr(weight), ptr(w),
                                              stream_ptr()), "timesnet_spectrum_select")
    return amp_mean, freq, top, period, rows, weight, w, xl


class TimesNetSpectrumFn(torch.autograd.Function):
    """TimesBlock's period selection as two launches forward, one backward: x (B, T, N) -> (top, period, rows, w, xl) -- the k selected
    frequency indices (int64), their periods and image row counts (int32; ops.period_rows' values), the softmaxed per-window weights (B, k)
    and the position-major image (2T B, N).  Differentiable in x through w and xl; top / period / rows carry no gradient."""

    @staticmethod
    def forward(ctx, x, k):
        x = _c(x)
        _, _, top, period, rows, _, w, xl = _spectrum_forward(x, k)
        ctx.save_for_backward(x, top, w)
        ctx.mark_non_differentiable(top, period, rows)
        ctx.set_materialize_grads(False)
        return top, period, rows, w, xl

    @staticmethod
    def backward(ctx, g_top, g_period, g_rows, g_w, g_xl):
        x, top, w = ctx.saved_tensors
        B, T, N = x.shape
        g_w = None if g_w is None else _c(g_w.float())
        g_xl = None if g_xl is None else _c(g_xl.float())
        dx = torch.empty_like(x)
        check(_lib.load().immtsf_timesnet_spectrum_bwd(ptr(x), ptr(top), ptr(w), ptr(g_w), ptr(g_xl), B, T, N, top.numel(), ptr(dx), stream_ptr()),
              "timesnet_spectrum_bwd")
        return dx, None


def timesnet_spectrum(x, k):
    """x (B, T, N) fp32 -> (top (k) int64, period (k) int32, rows (k) int32, w (B, k), xl (2T B, N)), everything on the device: what
    fft_for_period_device + period_rows + softmax + the padded transpose of models/TimesNet.py TimesBlock.forward compute, by a direct DFT
    (include/immtsf.h immtsf_timesnet_spectrum_*).  Outside timesnet_spectrum_ok this raises: callers check."""
    return TimesNetSpectrumFn.apply(x, int(k))


def timesnet_spectrum_stats(x, k):
    """the forward's intermediate values, for tests and tools: (amp_mean (B, F) the per-window mean amplitude over the channels, freq (F) its
    mean over the windows with freq[0] = 0, weight (B, k) = amp_mean[:, top] before the softmax).  No gradient."""
    amp_mean, freq, _, _, _, weight, _, _ = _spectrum_forward(_c(x.detach()), k)
    return amp_mean, freq, weight


def conv2d_period(x, period, rows, Weff, beff, KS, B, Lmax, act=None, precision=None, w16=None):
    return Conv2dPeriodFn.apply(x.float(), period, rows, Weff, beff, int(KS), 2 if act == "gelu" else 0, config.precision_code(precision),
                                int(B), int(Lmax), w16)


INCEPTION_MAX = 8


def inception_merge(block):
    """block: layers.Conv_Blocks.Inception_Block_V1 -> (W_eff, b_eff, KS)"""
    ks = block.kernels
    n = len(ks)
    Weff, beff = InceptionMergeFn.apply(n, *[k.weight for k in ks], *[k.bias for k in ks])
    return Weff, beff, 2 * n - 1


def conv2d_same_cl(x, Weff, beff, KS, act=None, precision=None):
    return Conv2dSameCLFn.apply(x.float(), Weff, beff, int(KS), 2 if act == "gelu" else 0, config.precision_code(precision))


class TPatchDecoderFn(torch.autograd.Function):
    """tPatchGNN's forecast decoder on (h (B,N,D), te (B,Lp,E)) -> (B,Lp,N): one kernel per direction -- exact fp32, or in bf16
    mode the second layer and its gradients on MFMA tiles (csrc/decoder.hip).  Backward recomputes the forward; parameter
    gradients accumulate by atomics into one zeroed flat buffer."""

    @staticmethod
    def forward(ctx, h, te, precision, *params):
        lib = _lib.load()
        h, te = _c(h), _c(te)
        params = tuple(_c(p) for p in params)
        _need_gpu(h, te, *params)
        B, N, D = h.shape
        Lp, E = te.shape[1], te.shape[2]
        H = params[2].shape[0]
        out = torch.empty(B, Lp, N, dtype=torch.float32, device=h.device)
        ps = _struct(DecoderParams, params)
        check(lib.immtsf_tpatchgnn_decoder_forward_p(B, N, Lp, D, E, H, precision, ptr(h), ptr(te), C.byref(ps), ptr(out), stream_ptr()),
              "tpatchgnn_decoder_forward")
        ctx.dims = (B, N, Lp, D, E, H, precision)
        ctx.sinks = _sinks_of(params)
        ctx.save_for_backward(h, te, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        h, te, *params = ctx.saved_tensors
        B, N, Lp, D, E, H, precision = ctx.dims
        dout = dout.contiguous()
        dh, dte = torch.empty_like(h), torch.empty_like(te)
        grads, rets = _zeroed_grad_buffers(params, ctx.sinks)
        ps, gs = _struct(DecoderParams, params), _struct(DecoderParams, grads)
        check(lib.immtsf_tpatchgnn_decoder_backward_p(B, N, Lp, D, E, H, precision, ptr(h), ptr(te), C.byref(ps), ptr(dout), ptr(dh),
                                                      ptr(dte), C.byref(gs), stream_ptr()), "tpatchgnn_decoder_backward")
        return (dh, dte, None) + tuple(rets)


class TPatchDecoderTEFn(torch.autograd.Function):
    """The decoder with LearnableTE of the prediction times inside: (h (B,N,D), t (B,Lp)) -> (B,Lp,N).  te = [w0 t + b0 ; sin(w t + b)]
    is built while a window is staged and its gradient is reduced to the four parameter gradients in the backward kernel: no
    (B,Lp,E) tensor, no separate Time2Vec launches (models/tPatchGNN.py:176-180, 283-291).  t is data (no gradient)."""

    @staticmethod
    def forward(ctx, h, t, precision, w0, b0, w, b, *params):
        lib = _lib.load()
        h, t = _c(h), _c(t)
        tparams = tuple(_c(q) for q in (w0, b0, w, b))
        params = tuple(_c(q) for q in params)
        _need_gpu(h, t, *tparams, *params)
        B, N, D = h.shape
        Lp, E = t.shape[1], 1 + tparams[2].numel()
        H = params[2].shape[0]
        out = torch.empty(B, Lp, N, dtype=torch.float32, device=h.device)
        ps, ts = _struct(DecoderParams, params), _struct(_lib.Time2VecParams, tparams)
        check(lib.immtsf_tpatchgnn_decoder_forward_te(B, N, Lp, D, E, H, precision, ptr(h), ptr(t), C.byref(ts), C.byref(ps), ptr(out),
                                                      stream_ptr()), "tpatchgnn_decoder_forward_te")
        ctx.dims = (B, N, Lp, D, E, H, precision)
        ctx.sinks, ctx.tsinks = _sinks_of(params), _sinks_of(tparams)
        _claim_sinks(tparams, ctx.tsinks, "tpatch_decoder_te")
        ctx.save_for_backward(h, t, *tparams, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        h, t, w0, b0, w, b, *params = ctx.saved_tensors
        tparams = (w0, b0, w, b)
        B, N, Lp, D, E, H, precision = ctx.dims
        dout = dout.contiguous()
        dh = torch.empty_like(h)
        grads, rets = _zeroed_grad_buffers(params, ctx.sinks)
        tgrads, trets = _zeroed_grad_buffers(tparams, ctx.tsinks)       # (shared sinks -- the patch encoder adds into them too -- are zero-filled by their owner)
        ps, gs = _struct(DecoderParams, params), _struct(DecoderParams, grads)
        ts, tg = _struct(_lib.Time2VecParams, tparams), _struct(_lib.Time2VecParams, tgrads)
        check(lib.immtsf_tpatchgnn_decoder_backward_te(B, N, Lp, D, E, H, precision, ptr(h), ptr(t), C.byref(ts), C.byref(ps), ptr(dout),
                                                       ptr(dh), C.byref(gs), C.byref(tg), stream_ptr()), "tpatchgnn_decoder_backward_te")
        return (dh, None, None) + tuple(trets) + tuple(rets)


def tpatch_decoder_supported(seq, N, Lp, D, E):
    """seq: the reference's decoder nn.Sequential (Linear, ReLU, Linear, ReLU, Linear(H, 1))"""
    mods = list(seq)
    if len(mods) != 5 or not all(isinstance(m, torch.nn.Linear) for m in mods[0::2]) \
            or not all(isinstance(m, torch.nn.ReLU) for m in mods[1::2]):
        return False
    l1, l2, l3 = mods[0], mods[2], mods[4]
    H = l1.out_features
    if l1.in_features != D + E or l2.in_features != H or l2.out_features != H or l3.in_features != H or l3.out_features != 1:
        return False
    if any(m.bias is None for m in (l1, l2, l3)):
        return False
    return _lib.load().immtsf_tpatchgnn_decoder_lds_bytes(N, Lp, D, E, H) > 0


def tpatch_decoder(seq, h, te, precision=None):
    """decoder(cat[h broadcast over Lp ; te broadcast over N]).squeeze(-1).permute(0, 2, 1) of models/tPatchGNN.py:283-291
    without materialising the (B, N, Lp, D+E) tensor: h (B,N,D), te (B,Lp,E) -> (B,Lp,N)."""
    l1, l2, l3 = seq[0], seq[2], seq[4]
    return TPatchDecoderFn.apply(h.float(), te.float(), config.precision_code(precision), l1.weight, l1.bias, l2.weight, l2.bias,
                                 l3.weight, l3.bias)


def tpatch_decoder_te(seq, h, t, w0, b0, w, b, precision=None):
    """tpatch_decoder with the time embedding of the prediction times t (B, Lp) computed inside (w0 / b0: te_scale, w / b: te_periodic)"""
    if t.requires_grad:
        raise RuntimeError("immtsf.tpatch_decoder_te: timestamps are data; no gradient is produced for them")
    l1, l2, l3 = seq[0], seq[2], seq[4]
    return TPatchDecoderTEFn.apply(h.float(), t.float(), config.precision_code(precision), w0, b0, w, b, l1.weight, l1.bias, l2.weight,
                                   l2.bias, l3.weight, l3.bias)


# ------------------------------------------------------------------------------------------------ layer primitives
_ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2}


def _gemm(layout, prec, A, lda, B, ldb, Cm, ldc, bias, M, N, K, alpha=1.0, accumulate=0, act=0):
    lib = _lib.load()
    check(lib.immtsf_gemm(layout, prec, ptr(A), lda, ptr(B), ldb, ptr(Cm), ldc, ptr(bias), M, N, K, alpha, accumulate, act,
                          stream_ptr()), "gemm")


class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b) on the MFMA GEMM (NT forward with the bias / ReLU epilogue; backward = one
    immtsf_linear_backward call: NN data gradient, TN weight gradient with the bias gradient folded in)."""

    @staticmethod
    def forward(ctx, x, W, b, precision, relu):
        x2 = _c(x).reshape(-1, x.shape[-1])
        W = _c(W)
        _need_gpu(x2, W, b)
        M, K = x2.shape
        N = W.shape[0]
        y = torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=x.device)   # not a view: callers may relu_ it
        _gemm(0, precision, x2, K, W, K, y, N, b, M, N, K, act=1 if relu else 0)
        ctx.save_for_backward(x2, W, y if relu else None)
        ctx.has_bias, ctx.precision, ctx.shape = b is not None, precision, x.shape
        ctx.sinks = _sinks_of((W, b))
        ctx.pre = all(s is not None and getattr(p, "_immtsf_grad_prezeroed", False) for p, s in zip((W, b), ctx.sinks) if p is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x2, W, y = ctx.saved_tensors
        M, K = x2.shape
        N = W.shape[0]
        dy2 = dy.contiguous().reshape(M, N)
        if y is not None:
            dy2 = torch.ops.aten.threshold_backward(dy2, y.reshape(M, N), 0.0)
        need_w = ctx.needs_input_grad[1]
        dx = torch.empty(M, K, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
        dW = db = rW = rb = None
        if need_w and ctx.pre:  # gradient sinks that their owner zero-fills every step: written in place, nothing returned
            dW, db = ctx.sinks
        elif need_w:            # ONE zero fill for dW|db: the split-K weight gradient then needs no memsets of its own
            flat = torch.zeros(N * K + (N if ctx.has_bias else 0), dtype=torch.float32, device=dy.device)
            dW = rW = flat[:N * K].view(N, K)
            db = rb = flat[N * K:] if ctx.has_bias else None
        check(lib.immtsf_linear_backward(ctx.precision, ptr(x2), ptr(W), ptr(dy2), M, N, K, ptr(dx), None, ptr(dW), ptr(db),
                                         1, stream_ptr()), "linear_backward")
        return (dx.view(ctx.shape) if dx is not None else None), rW, rb, None, None


class LinearBf16Fn(torch.autograd.Function):
    """nl (1..3) linear layers y_i = act(x W_i^T + b_i) that share ONE input, in the bf16 dataflow (immtsf_linear_bf16_forward /
    _backward): the input is cast once and kept as bf16 for the weight gradients, the weights are read from FlatTrainer's bf16 twins
    (else cast into a scratch image), the forward is ONE launch, the backward one cast per upstream gradient, nl accumulating
    data-gradient launches and ONE grouped weight-gradient launch.  args: x, relu, nl, W_1..W_nl, b_1..b_nl (None allowed)."""

    @staticmethod
    def forward(ctx, x, relu, nl, *wb):
        lib = _lib.load()
        Ws, bs = [_c(w) for w in wb[:nl]], list(wb[nl:])
        x2 = _c(x).reshape(-1, x.shape[-1])
        _need_gpu(x2, *Ws)
        M, K = x2.shape
        N = Ws[0].shape[0]
        dev = x.device
        x16 = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
        w16 = [torch.empty(N, K, dtype=torch.bfloat16, device=dev) for _ in range(nl)]       # (unused when a twin is registered)
        ys = [torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=dev) for _ in range(nl)]
        arr = lambda ts: (C.c_void_p * nl)(*[None if t is None else t.data_ptr() for t in ts])      # noqa: E731
        check(lib.immtsf_linear_bf16_forward(nl, ptr(x2), ptr(x16), arr(Ws), arr(w16), arr(bs), arr(ys), M, N, K, 1 if relu else 0,
                                             stream_ptr()), "linear_bf16_forward")
        ctx.save_for_backward(x16, *Ws, *([ys[0]] if relu else []))
        ctx.nl, ctx.relu, ctx.shape, ctx.w16 = nl, relu, x.shape, w16
        ctx.has_bias = [b is not None for b in bs]
        ctx.wsinks, ctx.bsinks = _sinks_of(Ws), _sinks_of(bs)
        ctx.pre = all(s is not None and getattr(p, "_immtsf_grad_prezeroed", False)
                      for p, s in zip(list(Ws) + bs, ctx.wsinks + ctx.bsinks) if p is not None)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        lib = _lib.load()
        nl = ctx.nl
        saved = ctx.saved_tensors
        x16, Ws = saved[0], saved[1:1 + nl]
        M, K = x16.shape
        N = Ws[0].shape[0]
        dev = x16.device
        dys = [torch.zeros(M, N, dtype=torch.float32, device=dev) if d is None else d.contiguous().reshape(M, N) for d in dys]
        if ctx.relu:
            dys[0] = torch.ops.aten.threshold_backward(dys[0], saved[1 + nl].reshape(M, N), 0.0)
        need_w = any(ctx.needs_input_grad[3 + i] for i in range(nl))
        dx = torch.empty(M, K, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        rW, rb = [None] * nl, [None] * nl
        dW, db = [None] * nl, [None] * nl
        if need_w and ctx.pre:          # gradient sinks that their owner zero-fills every step: written in place, nothing returned
            dW, db = list(ctx.wsinks), list(ctx.bsinks)
        elif need_w:                    # ONE zero fill for every dW | db
            per = N * K + N
            flat = torch.zeros(nl * per, dtype=torch.float32, device=dev)
            for i in range(nl):
                dW[i] = rW[i] = flat[i * per:i * per + N * K].view(N, K)
                if ctx.has_bias[i]:
                    db[i] = rb[i] = flat[i * per + N * K:(i + 1) * per]
        dy16 = torch.empty(nl * M * N, dtype=torch.bfloat16, device=dev)
        arr = lambda ts: (C.c_void_p * nl)(*[None if t is None else t.data_ptr() for t in ts])      # noqa: E731
        w16 = ctx.w16

        def launch(stream, dx_, wgrads, mode):          # wgrads: (dW, db) or None  (the closure keeps every buffer it reads alive)
            dW_, db_ = (arr(wgrads[0]), arr(wgrads[1])) if wgrads else (None, None)
            check(lib.immtsf_linear_bf16_backward(nl, ptr(x16), arr(Ws), arr(w16), arr(dys), ptr(dy16), ptr(dx_), dW_, db_, M, N, K, mode, stream),
                  "linear_bf16_backward")
        # a step with a parameter-only branch (immtsf.train.FlagStep): the weight gradients -- nothing in the backward waits for them --
        # leave this stream's dependent chain (the data gradient and the casts stay).  Only when every gradient goes straight to a
        # pre-zeroed sink (nothing is returned).
        plan = step_plan.current()
        if need_w and ctx.pre and plan.wgrad_open and dx is not None:
            launch(stream_ptr(), dx, None, 1)
            plan.defer_wgrad(lambda stream: launch(stream, None, (dW, db), 3))
            return (dx.view(ctx.shape), None, None) + tuple(rW) + tuple(rb)
        launch(stream_ptr(), dx, (dW, db) if need_w else None, 1)
        return ((dx.view(ctx.shape) if dx is not None else None), None, None) + tuple(rW) + tuple(rb)


def _bf16_linear_ok(x, W, precision):
    # (small layers -- tPatchGNN's 64 -> 32 temporal aggregation -- keep their exact-fp32 one-launch kernels)
    return (config.precision_code(precision) == 1 and x.is_cuda and W.shape[1] % 8 == 0 and W.shape[0] % 8 == 0 and W.shape[1] >= 128 and
            W.shape[0] >= 64 and x.numel() // x.shape[-1] >= 256)


def linear(x, W, b=None, precision=None, relu=False):
    if _bf16_linear_ok(x, W, precision):      # bf16 mode, enough rows: the bf16-in-HBM kernels (operands cast once, weights from their twins)
        return LinearBf16Fn.apply(x.float(), relu, 1, W, b)[0]
    return LinearFn.apply(x.float(), W, b, config.precision_code(precision), relu)


def linear_multi(x, weights, biases, precision=None):
    """[x W_i^T + b_i] for layers sharing one input (a self-attention's q | k | v projections) -- one launch forward, one grouped
    weight-gradient launch backward in bf16 mode; one linear() each otherwise"""
    nl = len(weights)
    same = all(w.shape == weights[0].shape for w in weights)
    if 1 <= nl <= 3 and same and _bf16_linear_ok(x, weights[0], precision):
        return list(LinearBf16Fn.apply(x.float(), False, nl, *weights, *biases))
    return [linear(x, w, b, precision) for w, b in zip(weights, biases)]


class MLPFn(torch.autograd.Function):
    """Linear (ReLU Linear)* chain, e.g. tPatchGNN's decoder (models/tPatchGNN.py:158-163): one GEMM per layer forward
    (bias + ReLU in the epilogue), two per layer backward -- the ReLU mask is applied in the epilogue of the NEXT
    layer's data-gradient GEMM and the bias gradient rides the weight-gradient GEMM as a ones column."""

    @staticmethod
    def forward(ctx, x, precision, has_bias, *params):
        nl = len(has_bias)
        Ws = [_c(w) for w in params[:nl]]
        bs = list(params[nl:])
        acts = [_c(x).reshape(-1, x.shape[-1])]
        _need_gpu(acts[0], *Ws)
        for i, W in enumerate(Ws):
            M, K = acts[-1].shape
            N = W.shape[0]
            shape = (M, N) if i + 1 < nl else (*x.shape[:-1], N)
            y = torch.empty(shape, dtype=torch.float32, device=x.device)
            _gemm(0, precision, acts[-1], K, W, K, y, N, bs[i], M, N, K, act=1 if i + 1 < nl else 0)
            acts.append(y)
        ctx.save_for_backward(*acts[:-1], *Ws)
        ctx.nl, ctx.has_bias, ctx.precision, ctx.shape = nl, has_bias, precision, x.shape
        ctx.wsinks, ctx.bsinks = _sinks_of(params[:nl]), _sinks_of(bs)
        ctx.pre = all(s is not None and getattr(p, "_immtsf_grad_prezeroed", False)
                      for p, s in zip(list(params[:nl]) + bs, ctx.wsinks + ctx.bsinks) if p is not None)
        return acts[-1]

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        nl = ctx.nl
        acts, Ws = ctx.saved_tensors[:nl], ctx.saved_tensors[nl:]
        dWs, dbs = [None] * nl, [None] * nl
        g = dy.contiguous().reshape(-1, Ws[-1].shape[0])
        dev = dy.device
        if ctx.pre:             # FlatTrainer sinks (zero-filled by their owner every step): written in place
            dWs, dbs = list(ctx.wsinks), list(ctx.bsinks)
            rWs, rbs = [None] * nl, [None] * nl
        else:
            # ONE zero-filled buffer for every layer's dW|db (32-byte aligned slices): no per-GEMM memsets
            sizes = [((W.numel() + 7) // 8 * 8, (W.shape[0] + 7) // 8 * 8) if ctx.needs_input_grad[3 + i] else (0, 0)
                     for i, W in enumerate(Ws)]
            flat = torch.zeros(max(1, sum(a + b for a, b in sizes)), dtype=torch.float32, device=dev)
            off = 0
            for i, W in enumerate(Ws):
                if ctx.needs_input_grad[3 + i]:
                    dWs[i] = flat[off:off + W.numel()].view(W.shape)
                    off += sizes[i][0]
                    if ctx.has_bias[i]:
                        dbs[i] = flat[off:off + W.shape[0]]
                    off += sizes[i][1]
            rWs, rbs = dWs, dbs
        for i in reversed(range(nl)):
            x, W = acts[i], Ws[i]
            M, K = x.shape
            N = W.shape[0]
            need_x = i > 0 or ctx.needs_input_grad[0]
            dx = torch.empty(M, K, dtype=torch.float32, device=dev) if need_x else None
            check(lib.immtsf_linear_backward(ctx.precision, ptr(x), ptr(W), ptr(g), M, N, K, ptr(dx),
                                             ptr(x) if i > 0 else None, ptr(dWs[i]), ptr(dbs[i]), 1, stream_ptr()),
                  "linear_backward")
            g = dx
        return (g.view(ctx.shape) if g is not None else None), None, None, *rWs, *rbs


def mlp(x, weights, biases, precision=None):
    """weights[i] (N_i, K_i), biases[i] (N_i) or None; ReLU between layers, none after the last."""
    return MLPFn.apply(x.float(), config.precision_code(precision), tuple(b is not None for b in biases), *weights, *biases)


class Time2VecFn(torch.autograd.Function):
    """[w0 t + b0, sin(w t + b)] rows (Time2Vec / tPatchGNN.LearnableTE); t is data (no gradient)."""

    @staticmethod
    def forward(ctx, t, w0, b0, w, b):
        lib = _lib.load()
        t1 = _c(t).reshape(-1)
        _need_gpu(t1, w0, b0)
        d = 1 + (w.numel() if w is not None else 0)
        out = torch.empty(*t.shape, d, dtype=torch.float32, device=t.device)
        check(lib.immtsf_time2vec_forward(ptr(t1), t1.numel(), d, ptr(w0), ptr(b0), ptr(w), ptr(b), ptr(out), stream_ptr()),
              "time2vec_forward")
        _claim_sinks((w0, b0, w, b), _sinks_of((w0, b0, w, b)), "time2vec")
        ctx.save_for_backward(t1, w0, b0, w, b)
        ctx.d = d
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        t1, w0, b0, w, b = ctx.saved_tensors
        d = ctx.d
        g = dout.contiguous().reshape(-1, d)
        params = (w0, b0, w, b)
        sinks = _sinks_of(params)
        acc = w is not None and _shared(params, sinks)      # parameters shared with another HIP op (tPatchGNN: the TTCN encoder)
        if acc:
            (dw0, db0, dw, db), rets = sinks, (None,) * 4
        else:
            dw0, db0 = torch.empty_like(w0), torch.empty_like(b0)
            dw = torch.empty_like(w) if w is not None else None
            db = torch.empty_like(b) if b is not None else None
            rets = (dw0, db0, dw, db)
        scratch = torch.empty(2 * 64 * d, dtype=torch.float32, device=g.device)
        check(lib.immtsf_time2vec_backward(ptr(t1), t1.numel(), d, ptr(w), ptr(b), ptr(g), ptr(dw0), ptr(db0), ptr(dw), ptr(db),
                                           ptr(scratch), 1 if acc else 0, stream_ptr()), "time2vec_backward")
        return (None,) + tuple(rets)


def time2vec(t, w0, b0, w, b):
    """t (...,) -> (..., 1 + len(w)); w0/b0 = Linear(1,1) weight/bias, w/b = Linear(1,d-1) weight (d-1,1) / bias."""
    if t.requires_grad:
        raise RuntimeError("immtsf.time2vec: timestamps are data; no gradient is produced for them")
    return Time2VecFn.apply(t.float(), _c(w0), _c(b0), None if w is None else _c(w), None if b is None else _c(b))


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        lib = _lib.load()
        x2 = _c(x).reshape(-1, x.shape[-1])
        _need_gpu(x2, gamma, beta)
        rows, d = x2.shape
        xhat = torch.empty_like(x2)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        z = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        check(lib.immtsf_layernorm_forward(ptr(x2), rows, d, ptr(gamma), ptr(beta), float(eps), ptr(xhat), ptr(rstd), ptr(z),
                                           0.0, 0, 0, stream_ptr()), "layernorm_forward")
        ctx.save_for_backward(xhat, rstd, gamma)
        ctx.shape = x.shape
        ctx.sinks = _sinks_of((gamma, beta))
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = _lib.load()
        xhat, rstd, gamma = ctx.saved_tensors
        rows, d = xhat.shape
        g = dz.contiguous().reshape(rows, d).clone()
        dx = torch.empty_like(xhat)
        (dgamma, dbeta), rets = _grad_buffers((gamma, gamma), ctx.sinks)        # overwritten by the kernel
        scratch = torch.empty(64 * d, dtype=torch.float32, device=dz.device)
        check(lib.immtsf_layernorm_backward(ptr(g), rows, d, ptr(gamma), ptr(xhat), ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta),
                                            ptr(scratch), 0.0, 0, 0, stream_ptr()), "layernorm_backward")
        return dx.view(ctx.shape), rets[0], rets[1], None


def layer_norm(x, gamma, beta, eps=1e-5):
    return LayerNormFn.apply(x.float(), gamma, beta, eps)


class FullAttentionFn(torch.autograd.Function):
    """softmax(scale * Q K^T) V per (batch, head) for (B,L,H,E)/(B,S,H,E)/(B,S,H,D) tensors
    (layers/SelfAttention_Family.py:50-77): batched MFMA GEMMs + fused softmax/dropout rows."""

    @staticmethod
    def forward(ctx, q, k, v, scale, p_drop, training, seed, site, causal, precision):
        lib = _lib.load()
        q, k, v = _c(q), _c(k), _c(v)
        _need_gpu(q, k, v)
        B, L, H, E = q.shape
        S, D = k.shape[1], v.shape[3]
        dev = q.device
        P = torch.empty(B, H, L, S, dtype=torch.float32, device=dev)
        p = float(p_drop) if training else 0.0
        if config.attn_mid and lib.immtsf_attn_mid_supported(L, S, E, D):
            # few positions, wide heads (PatchTST: 10 x 10 scores with E = 256): one kernel per direction (csrc/attn_mid.hip)
            cnt = config.dropout_counter_ptr(dev) if p > 0 else None
            out = torch.empty(B, L, H, D, dtype=torch.float32, device=dev)
            check(lib.immtsf_attn_mid_forward(ptr(q), ptr(k), ptr(v), B, L, S, H, E, D, float(scale), 1 if causal else 0, p, seed, site, cnt,
                                              ptr(P), ptr(out), stream_ptr()), "attn_mid_forward")
            ctx.save_for_backward(q, k, v, P)
            ctx.cfg = (scale, p, seed, site, precision, cnt)
            ctx.mid = True
            return out
        ctx.mid = False
        check(lib.immtsf_gemm_batched(0, precision, ptr(q), H * E, L * H * E, E, ptr(k), H * E, S * H * E, E, ptr(P), S,
                                      H * L * S, L * S, B, H, L, S, E, float(scale), stream_ptr()), "qk^T")
        A = torch.empty_like(P) if p > 0 else P
        cnt = config.dropout_counter_ptr(dev) if p > 0 else None
        check(lib.immtsf_softmax_rows_forward(ptr(P), ptr(A), B, H, L, S, None, p, seed, site, 1 if causal else 0, cnt,
                                              stream_ptr()), "softmax")
        out = torch.empty(B, L, H, D, dtype=torch.float32, device=dev)
        check(lib.immtsf_gemm_batched(1, precision, ptr(A), S, H * L * S, L * S, ptr(v), H * D, S * H * D, D, ptr(out), H * D,
                                      L * H * D, D, B, H, L, D, S, 1.0, stream_ptr()), "a.v")
        ctx.save_for_backward(q, k, v, P, A)
        ctx.cfg = (scale, p, seed, site, precision, cnt)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        if ctx.mid:
            q, k, v, P = ctx.saved_tensors
            A = None
        else:
            q, k, v, P, A = ctx.saved_tensors
        scale, p, seed, site, precision, cnt = ctx.cfg
        B, L, H, E = q.shape
        S, D = k.shape[1], v.shape[3]
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        st = stream_ptr()
        if ctx.mid:
            check(lib.immtsf_attn_mid_backward(ptr(q), ptr(k), ptr(v), ptr(P), ptr(dout), B, L, S, H, E, D, float(scale), p, seed, site, cnt,
                                               ptr(dq), ptr(dk), ptr(dv), st), "attn_mid_backward")
            return dq, dk, dv, None, None, None, None, None, None, None
        dA = torch.empty_like(P)
        # dA = dO V^T ; dV = A^T dO
        check(lib.immtsf_gemm_batched(0, precision, ptr(dout), H * D, L * H * D, D, ptr(v), H * D, S * H * D, D, ptr(dA), S,
                                      H * L * S, L * S, B, H, L, S, D, 1.0, st), "dA")
        check(lib.immtsf_gemm_batched(2, precision, ptr(A), S, H * L * S, L * S, ptr(dout), H * D, L * H * D, D, ptr(dv), H * D,
                                      S * H * D, D, B, H, S, D, L, 1.0, st), "dV")
        check(lib.immtsf_softmax_rows_backward(ptr(dA), ptr(P), B, H, L, S, p, seed, site, cnt, st), "softmax_bwd")
        # dQ = scale dS K ; dK = scale dS^T Q
        check(lib.immtsf_gemm_batched(1, precision, ptr(dA), S, H * L * S, L * S, ptr(k), H * E, S * H * E, E, ptr(dq), H * E,
                                      L * H * E, E, B, H, L, E, S, float(scale), st), "dQ")
        check(lib.immtsf_gemm_batched(2, precision, ptr(dA), S, H * L * S, L * S, ptr(q), H * E, L * H * E, E, ptr(dk), H * E,
                                      S * H * E, E, B, H, S, E, L, float(scale), st), "dK")
        return dq, dk, dv, None, None, None, None, None, None, None


class FullAttentionQKVFn(torch.autograd.Function):
    """self-attention on a PACKED in-projection output qkv (B, L, 3, H, E) (what `x @ in_proj_weight^T` yields): the
    batched GEMMs read q / k / v through strides and the backward writes dq / dk / dv straight into one (B,L,3,H,E)
    tensor -- no slice copies forward, no zero-fill + copy + add per slice backward."""

    @staticmethod
    def forward(ctx, qkv, scale, p_drop, training, seed, site, causal, precision):
        lib = _lib.load()
        qkv = _c(qkv)
        _need_gpu(qkv)
        B, L, three, H, E = qkv.shape
        assert three == 3
        dev = qkv.device
        ld, so = 3 * H * E, L * 3 * H * E
        q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * H * E, qkv.data_ptr() + 8 * H * E
        P = torch.empty(B, H, L, L, dtype=torch.float32, device=dev)
        check(lib.immtsf_gemm_batched(0, precision, C.c_void_p(q), ld, so, E, C.c_void_p(k), ld, so, E, ptr(P), L, H * L * L, L * L,
                                      B, H, L, L, E, float(scale), stream_ptr()), "qk^T")
        p = float(p_drop) if training else 0.0
        A = torch.empty_like(P) if p > 0 else P
        cnt = config.dropout_counter_ptr(dev) if p > 0 else None
        check(lib.immtsf_softmax_rows_forward(ptr(P), ptr(A), B, H, L, L, None, p, seed, site, 1 if causal else 0, cnt,
                                              stream_ptr()), "softmax")
        out = torch.empty(B, L, H, E, dtype=torch.float32, device=dev)
        check(lib.immtsf_gemm_batched(1, precision, ptr(A), L, H * L * L, L * L, C.c_void_p(v), ld, so, E, ptr(out), H * E,
                                      L * H * E, E, B, H, L, E, L, 1.0, stream_ptr()), "a.v")
        ctx.save_for_backward(qkv, P, A)
        ctx.cfg = (scale, p, seed, site, precision, cnt)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        qkv, P, A = ctx.saved_tensors
        scale, p, seed, site, precision, cnt = ctx.cfg
        B, L, _, H, E = qkv.shape
        ld, so = 3 * H * E, L * 3 * H * E
        q, k, v = qkv.data_ptr(), qkv.data_ptr() + 4 * H * E, qkv.data_ptr() + 8 * H * E
        dout = dout.contiguous()
        dA = torch.empty_like(P)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv.data_ptr(), dqkv.data_ptr() + 4 * H * E, dqkv.data_ptr() + 8 * H * E
        st = stream_ptr()
        check(lib.immtsf_gemm_batched(0, precision, ptr(dout), H * E, L * H * E, E, C.c_void_p(v), ld, so, E, ptr(dA), L,
                                      H * L * L, L * L, B, H, L, L, E, 1.0, st), "dA")
        check(lib.immtsf_gemm_batched(2, precision, ptr(A), L, H * L * L, L * L, ptr(dout), H * E, L * H * E, E, C.c_void_p(dv), ld,
                                      so, E, B, H, L, E, L, 1.0, st), "dV")
        check(lib.immtsf_softmax_rows_backward(ptr(dA), ptr(P), B, H, L, L, p, seed, site, cnt, st), "softmax_bwd")
        check(lib.immtsf_gemm_batched(1, precision, ptr(dA), L, H * L * L, L * L, C.c_void_p(k), ld, so, E, C.c_void_p(dq), ld, so, E,
                                      B, H, L, E, L, float(scale), st), "dQ")
        check(lib.immtsf_gemm_batched(2, precision, ptr(dA), L, H * L * L, L * L, C.c_void_p(q), ld, so, E, C.c_void_p(dk), ld, so, E,
                                      B, H, L, E, L, float(scale), st), "dK")
        return dqkv, None, None, None, None, None, None, None


class SharedKVAttentionFn(torch.autograd.Function):
    """softmax(scale * q k^T) v where the keys / values are ONE set shared by the whole batch (TimeLLM's ReprogrammingLayer,
    models/TimeLLM.py:43-61: the mapped word prototypes): q (B,L,H,E), k (S,H,E), v (S,H,E) -> (B,L,H,E).  Per head one MFMA
    GEMM over all B*L query rows (batched over the heads through strides), the fused softmax + dropout row kernel, and one
    GEMM back; the scores live as (H, B*L, S)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, p_drop, training, seed, site, precision):
        lib = _lib.load()
        q, k, v = _c(q), _c(k), _c(v)
        _need_gpu(q, k, v)
        B, L, H, E = q.shape
        S = k.shape[0]
        R = B * L
        dev = q.device
        P = torch.empty(H, R, S, dtype=torch.float32, device=dev)
        st = stream_ptr()
        check(lib.immtsf_gemm_batched(0, precision, ptr(q), H * E, 0, E, ptr(k), H * E, 0, E, ptr(P), S, 0, R * S, 1, H, R, S, E,
                                      float(scale), st), "q k^T")
        p = float(p_drop) if training else 0.0
        A = torch.empty_like(P) if p > 0 else P
        cnt = config.dropout_counter_ptr(dev) if p > 0 else None
        check(lib.immtsf_softmax_rows_forward(ptr(P), ptr(A), 1, H, R, S, None, p, seed, site, 0, cnt, st), "softmax")
        out = torch.empty(B, L, H, E, dtype=torch.float32, device=dev)
        check(lib.immtsf_gemm_batched(1, precision, ptr(A), S, 0, R * S, ptr(v), H * E, 0, E, ptr(out), H * E, 0, E, 1, H, R, E, S,
                                      1.0, st), "a v")
        ctx.save_for_backward(q, k, v, P, A)
        ctx.cfg = (scale, p, seed, site, precision, cnt)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        q, k, v, P, A = ctx.saved_tensors
        scale, p, seed, site, precision, cnt = ctx.cfg
        B, L, H, E = q.shape
        S, R = k.shape[0], B * L
        dout = dout.contiguous()
        dA = torch.empty_like(P)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        st = stream_ptr()
        check(lib.immtsf_gemm_batched(0, precision, ptr(dout), H * E, 0, E, ptr(v), H * E, 0, E, ptr(dA), S, 0, R * S, 1, H, R, S, E,
                                      1.0, st), "dA")
        check(lib.immtsf_gemm_batched(2, precision, ptr(A), S, 0, R * S, ptr(dout), H * E, 0, E, ptr(dv), H * E, 0, E, 1, H, S, E, R,
                                      1.0, st), "dV")
        check(lib.immtsf_softmax_rows_backward(ptr(dA), ptr(P), 1, H, R, S, p, seed, site, cnt, st), "softmax_bwd")
        check(lib.immtsf_gemm_batched(1, precision, ptr(dA), S, 0, R * S, ptr(k), H * E, 0, E, ptr(dq), H * E, 0, E, 1, H, R, E, S,
                                      float(scale), st), "dQ")
        check(lib.immtsf_gemm_batched(2, precision, ptr(dA), S, 0, R * S, ptr(q), H * E, 0, E, ptr(dk), H * E, 0, E, 1, H, S, E, R,
                                      float(scale), st), "dK")
        return dq, dk, dv, None, None, None, None, None, None


def shared_kv_attention(q, k, v, scale, p_drop=0.0, training=False, seed=0, site=16, precision=None):
    return SharedKVAttentionFn.apply(q.float(), k.float(), v.float(), scale, p_drop, training, seed, site,
                                     config.precision_code(precision))


ATTN_SHORT_MAX = 8      # IMMTSF_ATTN_SHORT_MAX


class ShortAttentionQKVFn(torch.autograd.Function):
    """FullAttentionQKVFn for sequences of at most ATTN_SHORT_MAX positions: one thread per (sequence, head, position), one
    launch per direction, exact fp32, same dropout stream; the backward recomputes the softmax (nothing but qkv is saved)."""

    @staticmethod
    def forward(ctx, qkv, scale, p_drop, training, seed, site, causal):
        lib = _lib.load()
        qkv = _c(qkv)
        _need_gpu(qkv)
        B, L, three, H, E = qkv.shape
        assert three == 3 and L <= ATTN_SHORT_MAX
        p = float(p_drop) if training else 0.0
        cnt = config.dropout_counter_ptr(qkv.device) if p > 0 else None
        out = torch.empty(B, L, H, E, dtype=torch.float32, device=qkv.device)
        check(lib.immtsf_attention_short_forward(ptr(qkv), B, L, H, E, float(scale), 1 if causal else 0, p, seed, site, cnt,
                                                 ptr(out), stream_ptr()), "attention_short_forward")
        ctx.save_for_backward(qkv)
        ctx.cfg = (float(scale), p, seed, site, 1 if causal else 0, cnt)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (qkv,) = ctx.saved_tensors
        scale, p, seed, site, causal, cnt = ctx.cfg
        B, L, _, H, E = qkv.shape
        dqkv = torch.empty_like(qkv)
        check(lib.immtsf_attention_short_backward(ptr(qkv), ptr(dout.contiguous()), B, L, H, E, scale, causal, p, seed, site, cnt,
                                                  ptr(dqkv), stream_ptr()), "attention_short_backward")
        return dqkv, None, None, None, None, None, None


def full_attention_qkv(qkv, scale, p_drop=0.0, training=False, seed=0, site=16, causal=False, precision=None):
    """qkv (B, L, 3, H, E) -> (B, L, H, E)"""
    if qkv.shape[1] <= ATTN_SHORT_MAX and qkv.shape[4] <= 64 and qkv.shape[4] % 4 == 0:
        return ShortAttentionQKVFn.apply(qkv.float(), scale, p_drop, training, seed, site, causal)
    return FullAttentionQKVFn.apply(qkv.float(), scale, p_drop, training, seed, site, causal, config.precision_code(precision))


def full_attention(q, k, v, scale, p_drop=0.0, training=False, seed=0, site=16, causal=False, precision=None):
    return FullAttentionFn.apply(q.float(), k.float(), v.float(), scale, p_drop, training, seed, site, causal,
                                 config.precision_code(precision))


# ------------------------------------------------------------------------------------------------ embeddings (a12 / a13)
EMBED_KMAX, EMBED_DMAX = 64, 512      # csrc/embed.hip limits
SITE_LAYER_BASE = 16                  # csrc/common.hpp: dropout sites of the layers/ modules


class EmbedFn(torch.autograd.Function):
    """immtsf_embed_forward/backward: mode 0 = replication pad + unfold + Linear(patch_len -> D) + pe + dropout on (R, L)
    rows, mode 1 = circular 3-tap token convolution + pe + dropout on (B, L, c_in); W (D, K) resp. (D, c_in, 3)."""

    @staticmethod
    def forward(ctx, x, W, pe, mode, P, K, stride, p_drop, training, seed, site):
        lib = _lib.load()
        x, W, pe = _c(x), _c(W), _c(pe)
        _need_gpu(x, W, pe)
        if mode == 0:
            R, L, c_in = x.shape[0], x.shape[1], 1
        else:
            R, L, c_in = x.shape
        D = W.shape[0]
        p = float(p_drop) if training else 0.0
        cnt = config.dropout_counter_ptr(x.device) if p > 0 else None
        out = torch.empty(R, P, D, dtype=torch.float32, device=x.device)
        check(lib.immtsf_embed_forward(mode, ptr(x), R, L, c_in, P, K, stride, D, ptr(W), ptr(pe), ptr(out), p, seed, site, cnt,
                                       stream_ptr()), "embed_forward")
        ctx.save_for_backward(x, W)
        ctx.cfg = (mode, R, L, c_in, P, K, stride, D, p, seed, site, cnt)
        ctx.sink = getattr(W, "_immtsf_grad_sink", None) if getattr(W, "_immtsf_grad_prezeroed", False) else None
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, W = ctx.saved_tensors
        mode, R, L, c_in, P, K, stride, D, p, seed, site, cnt = ctx.cfg
        dW = ctx.sink if ctx.sink is not None else torch.empty_like(W)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        check(lib.immtsf_embed_backward(mode, ptr(x), R, L, c_in, P, K, stride, D, ptr(W), ptr(dout.contiguous()), ptr(dW),
                                        1 if ctx.sink is not None else 0, ptr(dx), p, seed, site, cnt, stream_ptr()), "embed_backward")
        return (dx, None if ctx.sink is not None else dW) + (None,) * 9


def embed_supported(K, D):
    return K <= EMBED_KMAX and D <= EMBED_DMAX


def patch_embed(x, W, pe, patch_len, stride, pad, p_drop=0.0, training=False, site=None):
    """x (B, n_vars, L) -> (B * n_vars, P, D): PatchEmbedding (layers/Embed.py:165-190) in one kernel"""
    B, n_vars, L = x.shape
    P = (L + pad - patch_len) // stride + 1
    p = float(p_drop) if training else 0.0
    return EmbedFn.apply(x.float().reshape(B * n_vars, L), W, pe.reshape(-1, pe.shape[-1]), 0, P, patch_len, stride, p, training,
                         config.next_seed() if p > 0 else 0, SITE_LAYER_BASE + 40 if site is None else site)


def token_embed(x, W, pe, p_drop=0.0, training=False, site=None):
    """x (B, L, c_in) -> (B, L, D): TokenEmbedding + PositionalEmbedding + dropout of DataEmbedding in one kernel"""
    B, L, c_in = x.shape
    p = float(p_drop) if training else 0.0
    return EmbedFn.apply(x.float(), W, pe.reshape(-1, pe.shape[-1]), 1, L, 3 * c_in, 1, p, training,
                         config.next_seed() if p > 0 else 0, SITE_LAYER_BASE + 41 if site is None else site)


# ------------------------------------------------------------------------------------------------ loss
class MaskedMSEFn(torch.autograd.Function):
    """compute_error(truth, pred, mask, "MSE", "mean") (lib/evaluation.py:17-62) with a fused backward.

    With `group` (a torch.distributed process group) the per-variable (sum, count) pair is all-reduced before the
    divide, so every rank sees the loss of the global batch and sum-reduced gradients equal the single-process ones."""

    @staticmethod
    def forward(ctx, pred, truth, mask, group, global_cnt):
        lib = _lib.load()
        pred, truth, mask = _c(pred), _c(truth), _c(mask)
        _need_gpu(pred, truth, mask)
        Cc = pred.shape[-1]
        rows = pred.numel() // Cc
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        dpred = torch.empty_like(pred)
        if group is None and global_cnt is not None and Cc <= 64:
            # counts known beforehand: nothing waits for a reduction, several workgroups, one launch
            cnt = _c(global_cnt.to(torch.float32))
            check(lib.immtsf_masked_mse_counted(ptr(truth), ptr(pred), ptr(mask), rows, Cc, ptr(cnt), ptr(_mse_scratch(pred.device)),
                                                ptr(loss), ptr(dpred), 1.0, stream_ptr()), "masked_mse_counted")
            ctx.save_for_backward(dpred)
            return loss
        if group is None and rows * Cc <= _MSE_SMALL_MAX and Cc <= 4096:
            # one single-workgroup kernel instead of three launches (they sit between the forward and the backward)
            cnt = _c(global_cnt.to(torch.float32)) if global_cnt is not None else None
            check(lib.immtsf_masked_mse(ptr(truth), ptr(pred), ptr(mask), rows, Cc, ptr(cnt) if cnt is not None else None, None,
                                        None, ptr(loss), ptr(dpred), 1.0, stream_ptr()), "masked_mse")
            ctx.save_for_backward(dpred)
            return loss
        buf = torch.empty(2 + 128, Cc, dtype=torch.float32, device=pred.device)
        sums = buf[:2]
        check(lib.immtsf_masked_mse_sums(ptr(truth), ptr(pred), ptr(mask), rows, Cc, ptr(sums[0]), ptr(sums[1]),
                                         ptr(buf[2]), stream_ptr()), "masked_mse_sums")
        cnt = sums[1]
        if global_cnt is not None:
            cnt = _c(global_cnt.to(torch.float32))
        elif group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        check(lib.immtsf_masked_mse_finish(ptr(truth), ptr(pred), ptr(mask), rows, Cc, ptr(sums[0]), ptr(cnt), ptr(loss),
                                           ptr(dpred), 1.0, stream_ptr()), "masked_mse_finish")
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (dpred,) = ctx.saved_tensors
        if is_unit_grad(dloss):      # d(loss)/d(loss) = 1 from backward_unit(): the saved gradient is the answer
            return dpred, None, None, None, None
        return dpred * dloss, None, None, None, None


_MSE_SMALL_MAX = 1 << 17        # IMMTSF_MSE_SMALL_MAX
_mse_scratch_cache = {}         # owner: _mse_scratch.  (device type, index) -> the device's ticket + partial-loss buffer


def _mse_scratch(device) -> torch.Tensor:
    """Ticket word + partial losses of immtsf_masked_mse_counted: one zero-initialised buffer per device, kept for the life of
    the process (a captured graph keeps pointing at it).  One loss per step and process: calls are ordered on their stream; two
    concurrent calls on different streams of one device would need their own buffers (the C entry point takes any)."""
    key = (device.type, device.index)
    t = _mse_scratch_cache.get(key)
    if t is None:
        t = _mse_scratch_cache[key] = torch.zeros(65, dtype=torch.float32, device=device)
    return t


_unit_grads = {}                # owner: unit_grad / is_unit_grad.  (device type, index) -> the device's constant 1.0


def unit_grad(device) -> torch.Tensor:
    """The constant scalar 1.0 that `backward_unit` seeds the backward pass with (one per device, never written)."""
    key = (device.type, device.index)
    t = _unit_grads.get(key)
    if t is None:
        t = _unit_grads[key] = torch.ones((), dtype=torch.float32, device=device)
    return t


def is_unit_grad(t: torch.Tensor) -> bool:
    u = _unit_grads.get((t.device.type, t.device.index))
    return u is not None and t.data_ptr() == u.data_ptr() and t.dim() == 0


def backward_unit(loss: torch.Tensor):
    """loss.backward() seeded with the cached constant 1.0: no fill kernel for the seed, and loss functions that saved
    their input gradient (masked_mse) hand it on without a multiply -- two launches less between forward and backward."""
    loss.backward(gradient=unit_grad(loss.device))


def masked_mse(pred, truth, mask, group=None, global_cnt=None):
    """Data parallel, two ways to get single-process-equivalent gradients:
      group=...       all-reduce the per-variable (sum, count) inside the call (loss = global loss on every rank);
      global_cnt=...  per-variable observation counts of the GLOBAL batch, reduced once when the batch is built
                      (they depend on the mask only): no collective inside the step, the returned value is this
                      rank's share of the global loss (the shares add up to it)."""
    return MaskedMSEFn.apply(pred, truth, mask, group, global_cnt)


def dropout_keep_mask(seed: int, site: int, n: int, p: float, device) -> torch.Tensor:
    """uint8 keep-mask of `n` consecutive elements of a dropout site (for tests / mask export)."""
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.uint8, device=device)
    check(lib.immtsf_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, site, n, float(p), ptr(out), stream_ptr()), "dropout_mask")
    return out


# ------------------------------------------------------------------------------------------------ evaluation metrics
class EvalScratch:
    """slab scratch (one buffer per size, kept: a captured graph keeps pointing at it) and the ticket word of the evaluation-metric
    kernels.  The calls that share one must be ordered on their streams (the ticket is zero between calls): an immtsf.EvalStep owns
    its own; callers that pass none share the device's default and are on their own stream at their own risk."""

    def __init__(self, device):
        self.device = device
        self.ticket = torch.zeros(16, dtype=torch.int32, device=device)
        self._bufs = {}

    def take(self, nbytes):
        b = self._bufs.get(int(nbytes))
        if b is None:
            b = self._bufs[int(nbytes)] = _bytes(nbytes, self.device)
        return b, self.ticket


_eval_default = {}              # owner: _eval_scratch.  (device type, index) -> the EvalScratch of callers that pass none


def _eval_scratch(device, nbytes, scratch=None):
    if scratch is None:
        key = (device.type, device.index)
        scratch = _eval_default.get(key)
        if scratch is None:
            scratch = _eval_default[key] = EvalScratch(device)
    elif scratch.device != device:
        raise _lib.ImmtsfError(f"EvalScratch of {scratch.device} used on {device}")
    return scratch.take(nbytes)


def _eval_acc_ok(acc, Cc):
    if acc.dtype != torch.float64 or tuple(acc.shape) != (5, Cc) or not acc.is_contiguous() or not acc.is_cuda:
        raise _lib.ImmtsfError(f"evaluation accumulator must be a contiguous float64 (5, {Cc}) tensor on the GPU")


def eval_metrics_accum(pred, truth, mask, acc, scratch=None):
    """acc (5, C) float64 += per-variable sums of [(t-p)^2 m, |t-p| m, |t-p| / t (t != 0) m, m, (t != 0) m] over (..., C) tensors: ONE
    launch (immtsf_eval_metrics_accum), each tensor read once, deterministic.  Enqueues only.  scratch: an EvalScratch (None: the
    device's shared default)."""
    lib = _lib.load()
    Cc = pred.shape[-1]
    if tuple(truth.shape) != tuple(pred.shape) or tuple(mask.shape) != tuple(pred.shape):
        raise _lib.ImmtsfError("eval_metrics_accum: pred, truth and mask must have one shape")
    pred, truth, mask = (_c(t.detach().to(torch.float32)) for t in (pred, truth, mask))
    _need_gpu(pred, truth, mask)
    _eval_acc_ok(acc, Cc)
    rows = pred.numel() // Cc
    sc, tk = _eval_scratch(pred.device, lib.immtsf_eval_metrics_scratch_bytes(rows, Cc), scratch)
    check(lib.immtsf_eval_metrics_accum(ptr(truth), ptr(pred), ptr(mask), rows, Cc, ptr(acc), ptr(sc), sc.numel(), ptr(tk), stream_ptr()),
          "eval_metrics_accum")
    return acc


def mmf_xrank_q_eval(Y, P, bHO, M_u8, truth, mask, acc, d, H, kappa, precision, ln_w, ln_b, want_out=False, scratch=None):
    """Q half of MMF_XAttn_Add's low-rank form in evaluation mode + eval_metrics_accum over its result: ONE launch
    (immtsf_mmf_xrank_q_eval).  Returns the fused forecast when want_out, else None (it is then never written)."""
    lib = _lib.load()
    Y, P, bHO, M_u8, ln_w, ln_b = (_c(t.detach()) for t in (Y, P, bHO, M_u8, ln_w, ln_b))
    truth, mask = _c(truth.detach().to(torch.float32)), _c(mask.detach().to(torch.float32))
    _need_gpu(Y, P, bHO, M_u8, truth, mask, ln_w, ln_b)
    B, T, Cc = Y.shape
    if tuple(truth.shape) != (B, T, Cc) or tuple(mask.shape) != (B, T, Cc):
        raise _lib.ImmtsfError("mmf_xrank_q_eval: truth and mask must have the forecast's shape")
    _eval_acc_ok(acc, Cc)
    cfg = make_cfg(B, 0, T, Cc, 0, d, H, precision, False, 0.0, kappa, 0, Y.device)
    if int(lib.immtsf_mmf_xrank_pw(C.byref(cfg))) != P.shape[2]:
        raise _lib.ImmtsfError("MMF_XAttn_Add low-rank form: P does not have the row pitch of these dimensions")
    sc, tk = _eval_scratch(Y.device, lib.immtsf_mmf_xrank_q_eval_scratch_bytes(C.byref(cfg)), scratch)
    out = torch.empty_like(Y) if want_out else None
    check(lib.immtsf_mmf_xrank_q_eval(C.byref(cfg), ptr(ln_w), ptr(ln_b), ptr(Y), ptr(P), ptr(bHO), ptr(M_u8), ptr(out), None, 0, ptr(truth),
                                      ptr(mask), ptr(acc), ptr(sc), sc.numel(), ptr(tk), stream_ptr()), "mmf_xrank_q_eval")
    return out


# ------------------------------------------------------------------------------------------------ DLinear backbone
def dlinear_supported(S, P, Cc, k, individual):
    """the limits of the fused DLinear path (immtsf_dlinear_supported): 1 <= S, P <= 128, odd k >= 1, any C >= 1"""
    return bool(_lib.load().immtsf_dlinear_supported(int(S), int(P), int(Cc), int(k), 1 if individual else 0))


class DLinearFn(torch.autograd.Function):
    """DLinear.forecasting() (masked instance norm, moving-average decomposition, three Linear(S -> P) maps, de-normalisation) as ONE
    launch; backward = the parameter gradients in TWO (immtsf_dlinear_forward / _backward, csrc/dlinear.hip).  data / mask (B, L, C) and
    tp (B, L) are data: no gradient.  dims = (S, P, Lp, k, individual); params in the table's order, G = C (individual) or 1 tensors per
    kind.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, data, mask, tp, dims, table, *params):
        lib = _lib.load()
        S, P, Lp, k, individual = dims
        data, mask, tp = _c(data), _c(mask), _c(tp)
        _need_gpu(data, mask, tp, *params)
        B, L, Cc = data.shape
        y = torch.empty(B, Lp, Cc, dtype=torch.float32, device=data.device)
        stats = torch.empty(2, B, Cc, dtype=torch.float32, device=data.device)      # mean, std: what the backward restages the rows with
        check(lib.immtsf_dlinear_forward(B, L, Cc, S, P, Lp, k, individual, ptr(data), ptr(mask), ptr(tp), ptr(table), ptr(y),
                                         ptr(stats[0]), ptr(stats[1]), stream_ptr()), "dlinear_forward")
        ctx.dims = (B, L, Cc) + tuple(dims)
        ctx.save_for_backward(data, mask, tp, stats)
        return y

    @staticmethod
    def backward(ctx, dY):
        lib = _lib.load()
        data, mask, tp, stats = ctx.saved_tensors
        B, L, Cc, S, P, Lp, k, individual = ctx.dims
        G = Cc if individual else 1
        dY = dY.contiguous()
        flat = torch.empty(3 * G * P * (S + 1), dtype=torch.float32, device=dY.device)      # every entry is written: no zero fill
        dW = [flat[i * G * P * S:(i + 1) * G * P * S].view(G, P, S) for i in range(3)]
        db = [flat[3 * G * P * S + i * G * P:3 * G * P * S + (i + 1) * G * P].view(G, P) for i in range(3)]
        ws = _bytes(lib.immtsf_dlinear_workspace_bytes(B, S, P, Cc, individual), dY.device)
        check(lib.immtsf_dlinear_backward(B, L, Cc, S, P, Lp, k, individual, ptr(data), ptr(mask), ptr(tp), ptr(stats[0]), ptr(stats[1]),
                                          ptr(dY), ptr(dW[0]), ptr(dW[1]), ptr(dW[2]), ptr(db[0]), ptr(db[1]), ptr(db[2]), ptr(ws),
                                          ws.numel(), stream_ptr()), "dlinear_backward")
        rets = [t[g] for t in dW + db for g in range(G)]
        return (None,) * 5 + tuple(r if need else None for r, need in zip(rets, ctx.needs_input_grad[5:]))


def dlinear_forecast(data, mask, tp, Lp, S, P, k, seasonal, trend, time):
    """data, mask (B, L <= S, C), tp (B, L) -> the de-normalised forecast (B, Lp <= P, C) of DLinear.  seasonal / trend / time: the
    module's nn.Linear(S, P), or -- individual mode -- its nn.ModuleList of C of them."""
    individual = not hasattr(seasonal, "weight")
    B, L, Cc = data.shape
    mods = [list(m) if individual else [m] for m in (seasonal, trend, time)]
    params = [l.weight for m in mods for l in m] + [l.bias for m in mods for l in m]
    G = Cc if individual else 1
    if len(params) != 6 * G or any(not p.is_contiguous() or p.dtype != torch.float32 for p in params) or \
            any(tuple(p.shape) != (P, S) for p in params[:3 * G]) or any(tuple(p.shape) != (P,) for p in params[3 * G:]):
        raise _lib.ImmtsfError(f"dlinear_forecast: expected {G} contiguous fp32 Linear({S}, {P}) per map")
    if not dlinear_supported(S, P, Cc, k, individual) or not (0 <= L <= S and 0 <= Lp <= P) or B < 1 or \
            tuple(mask.shape) != (B, L, Cc) or tuple(tp.shape) != (B, L):
        raise _lib.ImmtsfError(f"dlinear_forecast: shapes outside the fused kernel (B {B}, L {L}, C {Cc}, S {S}, P {P}, Lp {Lp}, k {k})")
    # (the table immtsf_dlinear_forward reads: [Ws | Wt | Wtau | bs | bt | btau][channel])
    return DLinearFn.apply(data, mask, tp, (int(S), int(P), int(Lp), int(k), 1 if individual else 0), _pointer_table(params, data.device),
                           *params)


# ------------------------------------------------------------------------------------------------ TimeMixer backbone
SITE_TIMEMIXER_EMBED = SITE_LAYER_BASE + 42      # the embedding's dropout inside csrc/timemixer.hip: element ((off_i B + b T_i + t) d + f)


def timemixer_supported(S, P, Cc, d_model, d_ff, e_layers, down_layers, moving_avg):
    """the limits of the fused TimeMixer path (immtsf_timemixer_supported): 2 <= S <= 64, P <= 64, d_model <= 32, d_ff <= 64,
    e_layers <= 4, down_layers <= 6, 2C+1 <= 64, odd moving_avg"""
    return bool(_lib.load().immtsf_timemixer_supported(int(S), int(P), int(Cc), int(d_model), int(d_ff), int(e_layers), int(down_layers),
                                                       int(moving_avg)))


def timemixer_params(model):
    """the module's tensors in the order of immtsf_timemixer_forward's pointer table (the last block's trend mixers included: the
    kernels never read them and they get no gradient)"""
    n = model.down_layers
    ps = [model.enc_embedding.value_embedding.tokenConv.weight, model.enc_embedding.position_embedding.pe]
    for blk in model.pdm_blocks:
        seqs = list(blk.mix_season.down_sampling_layers) + [blk.mix_trend.up_sampling_layers[n - 1 - i] for i in range(n)] + [blk.out_layer]
        for seq in seqs:
            ps += [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias]
    head = model.predict_layers[n]
    return ps + [head.weight, head.bias, model.projection.weight, model.projection.bias]


def _timemixer_layout(dims):
    """-> (float offset of every table entry in the flat gradient, -1 = none; the flat gradient's length)"""
    E, n = dims[5], dims[6]
    return _grad_layout("immtsf_timemixer_grad_layout", dims[:7], 2 + E * (8 * n + 4) + 4,
                        f"timemixer: dimensions outside the fused kernel {dims}")


class TimeMixerFn(torch.autograd.Function):
    """TimeMixer.forecasting() as ONE launch; backward = the parameter gradients in TWO (immtsf_timemixer_forward / _backward,
    csrc/timemixer.hip), written into one flat buffer whose slices are handed to autograd (a parameter's FlatTrainer sink receives its
    slice through AccumulateGrad, as with DLinearFn).  data / mask (B, L, C) and tp (B, L) are data: no gradient.  dims = (S, P, C, d,
    d_ff, e_layers, n, k); drop = (p, seed, site, device counter).  params in the table's order.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, data, mask, tp, Lp, dims, drop, table, *params):
        lib = _lib.load()
        S, P, Cc, d, dff, E, n, k = dims
        data, mask, tp = _c(data), _c(mask), _c(tp)
        _need_gpu(data, mask, tp, *params)
        B, L, _ = data.shape
        p, seed, site, cnt = drop
        y = torch.empty(B, Lp, Cc, dtype=torch.float32, device=data.device)
        check(lib.immtsf_timemixer_forward(B, L, Cc, S, P, Lp, d, dff, E, n, k, ptr(data), ptr(mask), ptr(tp), ptr(table), ptr(y), p, seed,
                                           site, cnt, stream_ptr()), "timemixer_forward")
        ctx.cfg = (B, L, Lp, dims, drop)
        ctx.table = table
        ctx.shapes = [tuple(q.shape) for q in params]
        # the backward recomputes the forward from the parameters: saved (no copy), so that autograd's version check covers them
        ctx.save_for_backward(data, mask, tp, *params)
        return y

    @staticmethod
    def backward(ctx, dY):
        lib = _lib.load()
        data, mask, tp = ctx.saved_tensors[:3]
        B, L, Lp, dims, (p, seed, site, cnt) = ctx.cfg
        S, P, Cc, d, dff, E, n, k = dims
        offs, nv = _timemixer_layout(dims)
        flat = torch.empty(nv, dtype=torch.float32, device=dY.device)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_timemixer_workspace_bytes(B, S, P, Cc, d, dff, E, n), dY.device)
        check(lib.immtsf_timemixer_backward(B, L, Cc, S, P, Lp, d, dff, E, n, k, ptr(data), ptr(mask), ptr(tp), ptr(ctx.table),
                                            ptr(dY.contiguous()), ptr(flat), p, seed, site, cnt, ptr(ws), ws.numel(), stream_ptr()),
              "timemixer_backward")
        return (None,) * 7 + tuple(_flat_views(flat, offs, ctx.shapes, ctx.needs_input_grad[7:]))


def timemixer_forecast(model, data, mask, tp, Lp):
    """data, mask (B, L <= input_len, C), tp (B, L) -> the de-normalised forecast (B, Lp <= pred_len, C) of a models.TimeMixer.TimeMixer
    at the reference's default options.  In training mode with dropout > 0 the embedding's dropout is drawn inside the kernel: one
    config.next_seed() per call, site SITE_TIMEMIXER_EMBED, the device counter of config.enable_device_counters honoured."""
    c = model.configs
    n = model.down_layers
    dims = (int(model.input_len), int(model.pred_len), int(model.C), int(c.d_model), int(c.d_ff), int(model.layers), int(n),
            int(c.moving_avg))
    S, P, Cc, d, dff, E, _, k = dims
    B, L, _ = data.shape
    params = timemixer_params(model)
    if not timemixer_supported(*dims) or not (0 <= L <= S and 0 <= Lp <= P) or B < 1 or tuple(data.shape) != (B, L, Cc) or \
            tuple(mask.shape) != (B, L, Cc) or tuple(tp.shape) != (B, L):
        raise _lib.ImmtsfError(f"timemixer_forecast: shapes outside the fused kernel (B {B}, L {L}, Lp {Lp}, dims {dims})")
    T = [S >> i for i in range(n + 1)]
    want = [(d, 2 * Cc + 1, 3), None]
    for j in range(E):
        for i in range(n):
            want += [(T[i + 1], T[i]), (T[i + 1],), (T[i + 1], T[i + 1]), (T[i + 1],)]
        for i in range(n):
            want += [(T[i], T[i + 1]), (T[i],), (T[i], T[i]), (T[i],)]
        want += [(dff, d), (dff,), (d, dff), (d,)]
    want += [(P, T[n]), (P,), (Cc, d), (Cc,)]
    pe = params[1]
    if any(not q.is_contiguous() or q.dtype != torch.float32 for q in params) or pe.dim() != 3 or pe.shape[1] < S or pe.shape[2] != d or \
            any(w is not None and tuple(q.shape) != w for q, w in zip(params, want)):
        raise _lib.ImmtsfError("timemixer_forecast: the module's parameters are not the contiguous fp32 tensors of these dimensions")
    table = _pointer_table(params, data.device)
    p = float(model.enc_embedding.dropout.p) if model.training else 0.0
    drop = _kernel_drop(p, SITE_TIMEMIXER_EMBED, data.device)
    model._last_drop = drop      # (p, seed, site, counter pointer) of this module's latest fused call: what dropout_keep_mask reproduces
    return TimeMixerFn.apply(data, mask, tp, int(Lp), dims, drop, table, *params)


# ------------------------------------------------------------------------------------------------ TTM backbone
SITE_TTM_MIXER = SITE_LAYER_BASE + 43      # drop1 of a narrow mixer block inside csrc/ttm.hip; its drop2 is SITE_TTM_MIXER + 1
_TTM_MODES = {"patch": 0, "channel": 1}


def _ttm_view(mode, shape):
    """x (B, M, N, D) -> (mode code, outer, inner, F, D) of immtsf_ttm_mixer_*: the block mixes F at every (outer, inner, column)"""
    B, M, N, D = shape
    return (0, B * M, 1, N, D) if mode == "patch" else (1, B, N, M, D)


def ttm_mixer_supported(mode, shape):
    """the limits of the narrow mixer kernel (immtsf_ttm_mixer_supported) for x of `shape` (B, M, N, D): mode patch / channel,
    mixed axis F <= 32, D <= 65536, fewer than 2^31 elements"""
    if mode not in _TTM_MODES or len(shape) != 4 or min(shape) < 1:
        return False
    return bool(_lib.load().immtsf_ttm_mixer_supported(*[int(v) for v in _ttm_view(mode, shape)]))


def ttm_mixer_params(block):
    """a layers.MLP.TTMMixerBlock's tensors in the kernel's order: gamma, beta, W1, b1, W2, b2, Wg, bg"""
    return (block.norm.weight, block.norm.bias, block.mlp.fc1.weight, block.mlp.fc1.bias, block.mlp.fc2.weight, block.mlp.fc2.bias,
            block.gating_block.attn_layer.weight, block.gating_block.attn_layer.bias)


class TTMMixerFn(torch.autograd.Function):
    """One TTMMixerBlock in mode patch / channel on a contiguous x (B, M, N, D) as ONE launch; backward = dx and the eight parameter
    gradients in TWO (immtsf_ttm_mixer_forward / _backward, csrc/ttm.hip), recomputed from x: nothing else is saved.  drop = (p, seed,
    site, device counter).  The kernel OVERWRITES its gradient buffers, so they are a fresh allocation whose slices are handed to
    autograd: a parameter's FlatTrainer sink (pre-zeroed, shared or not) receives its slice through AccumulateGrad, as with DLinearFn
    and TimeMixerFn, and a block called twice before one backward accumulates.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, x, mode, drop, eps, *params):
        lib = _lib.load()
        x = _c(x)
        _need_gpu(x, *params)
        view = _ttm_view(mode, x.shape)
        p, seed, site, cnt = drop
        out = torch.empty_like(x)
        check(lib.immtsf_ttm_mixer_forward(*view, ptr(x), *[ptr(q) for q in params], eps, ptr(out), p, seed, site, cnt, stream_ptr()),
              "ttm_mixer_forward")
        ctx.cfg = (view, drop, eps)
        ctx.save_for_backward(x, *params)      # the parameters: saved (no copy), so that autograd's version check covers them
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, params = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        view, (p, seed, site, cnt), eps = ctx.cfg
        dout = dout.contiguous()
        dx = torch.empty_like(x)
        need = ctx.needs_input_grad[4:]
        bufs, rets = [None] * 8, [None] * 8
        if any(need):
            bufs, rets = _grad_buffers([q if n else None for q, n in zip(params, need)])      # overwritten by the fold
        g = dict(zip(("gamma", "beta", "W1", "b1", "W2", "b2", "Wg", "bg"), bufs))
        ws = _bytes(lib.immtsf_ttm_mixer_workspace_bytes(*view), dout.device)
        check(lib.immtsf_ttm_mixer_backward(*view, ptr(x), *[ptr(q) for q in params], eps, ptr(dout), ptr(dx), ptr(g["gamma"]), ptr(g["beta"]),
                                            ptr(g["W1"]), ptr(g["b1"]), ptr(g["W2"]), ptr(g["b2"]), ptr(g["Wg"]), ptr(g["bg"]), p, seed, site,
                                            cnt, ptr(ws), ws.numel(), stream_ptr()), "ttm_mixer_backward")
        return (dx if ctx.needs_input_grad[0] else None, None, None, None) + tuple(rets)


class TTMGateFn(torch.autograd.Function):
    """out = res + u softmax(g) over the last axis, one launch; backward = du, dg in one (immtsf_ttm_gate_forward / _backward); the
    residual's gradient is the upstream gradient itself"""

    @staticmethod
    def forward(ctx, res, u, g):
        lib = _lib.load()
        res, u, g = _c(res), _c(u), _c(g)
        _need_gpu(res, u, g)
        d = u.shape[-1]
        out = torch.empty_like(u)
        check(lib.immtsf_ttm_gate_forward(u.numel() // d, d, ptr(res), ptr(u), ptr(g), ptr(out), stream_ptr()), "ttm_gate_forward")
        ctx.save_for_backward(u, g)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        u, g = ctx.saved_tensors
        d = u.shape[-1]
        dout = dout.contiguous()
        du, dg = torch.empty_like(u), torch.empty_like(u)
        check(lib.immtsf_ttm_gate_backward(u.numel() // d, d, ptr(u), ptr(g), ptr(dout), ptr(du), ptr(dg), stream_ptr()), "ttm_gate_backward")
        return dout, du, dg


def ttm_mixer(block, x, mode, training):
    """a layers.MLP.TTMMixerBlock in mode "patch" / "channel" on a contiguous fp32 x (B, M, N, D) -> x + gate(mlp(norm(x) along the mixed
    axis)).  In training mode with dropout > 0 both dropouts are drawn inside the kernel: one config.next_seed() per call, sites
    SITE_TTM_MIXER / + 1, the device counter of config.enable_device_counters honoured; block._last_drop keeps what dropout_keep_mask
    reproduces them from."""
    params = ttm_mixer_params(block)
    F_ = x.shape[2] if mode == "patch" else x.shape[1]
    want = [(x.shape[3],), (x.shape[3],), (2 * F_, F_), (2 * F_,), (F_, 2 * F_), (F_,), (F_, F_), (F_,)]
    if not ttm_mixer_supported(mode, tuple(x.shape)) or not x.is_contiguous() or x.dtype != torch.float32:
        raise _lib.ImmtsfError(f"ttm_mixer: x {tuple(x.shape)} in mode {mode} is outside the kernel")
    if any(not q.is_contiguous() or q.dtype != torch.float32 or tuple(q.shape) != w for q, w in zip(params, want)):
        raise _lib.ImmtsfError("ttm_mixer: the block's parameters are not the contiguous fp32 tensors of these dimensions")
    p = float(block.mlp.dropout1.p) if training else 0.0
    if p > 0 and float(block.mlp.dropout2.p) != p:
        raise _lib.ImmtsfError("ttm_mixer: the two dropouts of a block share one probability")
    drop = _kernel_drop(p, SITE_TTM_MIXER, x.device)
    block._last_drop = drop
    return TTMMixerFn.apply(x, mode, drop, float(block.norm.eps), *params)


def ttm_gate(res, u, g):
    """res + u * softmax(g, -1), fp32 tensors of one shape on the GPU"""
    if not (res.shape == u.shape == g.shape) or u.dim() < 1 or u.shape[-1] < 1:
        raise _lib.ImmtsfError(f"ttm_gate: shapes {tuple(res.shape)}, {tuple(u.shape)}, {tuple(g.shape)}")
    return TTMGateFn.apply(res.float(), u.float(), g.float())


# ---- Informer's layers (csrc/prob_attn.hip, csrc/conv_distil.hip) ----------------------------------------------------------------------
def prob_attention_supported(L_Q, L_K, D, u):
    """the limits of the ProbAttention kernels (immtsf_prob_attention_supported): lengths <= 1024 in both roles, head width <= 512,
    1 <= u <= L_Q"""
    return bool(_lib.load().immtsf_prob_attention_supported(int(L_Q), int(L_K), int(D), int(u)))


class ProbAttentionFn(torch.autograd.Function):
    """immtsf_prob_attention_forward / _backward: two launches each.  q (B, L_Q, H, D), k / v (B, L_K, H, D), index_sample (L_Q, U)
    int32 -> (B, H, L_Q, D); P (B, H, u, L_K) and the selected indices (B, H, u), ascending, are saved (ctx.sel is also left on the
    Function's output as `.prob_sel` for the tests)."""

    @staticmethod
    def forward(ctx, q, k, v, index_sample, n_top, scale, causal):
        lib = _lib.load()
        q, k, v, index_sample = _c(q), _c(k), _c(v), _c(index_sample)
        _need_gpu(q, k, v, index_sample)
        B, LQ, H, D = q.shape
        LK, U = k.shape[1], index_sample.shape[1]
        dev = q.device
        M = torch.empty(B, H, LQ, dtype=torch.float32, device=dev)
        out = torch.empty(B, H, LQ, D, dtype=torch.float32, device=dev)
        P = torch.empty(B, H, n_top, LK, dtype=torch.float32, device=dev)
        sel = torch.empty(B, H, n_top, dtype=torch.int32, device=dev)
        check(lib.immtsf_prob_attention_forward(B, H, LQ, LK, D, U, n_top, 1 if causal else 0, scale, ptr(q), ptr(k), ptr(v), ptr(index_sample),
                                                ptr(M), ptr(out), ptr(P), ptr(sel), stream_ptr()), "prob_attention_forward")
        ctx.save_for_backward(q, k, v, P, sel)
        ctx.cfg = (B, H, LQ, LK, D, n_top, 1 if causal else 0, scale)
        ctx.mark_non_differentiable(sel, M)
        return out, sel, M

    @staticmethod
    def backward(ctx, dout, _dsel, _dM):
        lib = _lib.load()
        q, k, v, P, sel = ctx.saved_tensors
        B, H, LQ, LK, D, u, causal, scale = ctx.cfg
        dout = dout.contiguous()
        dq, dk, dv, dS = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(P)
        check(lib.immtsf_prob_attention_backward(B, H, LQ, LK, D, u, causal, scale, ptr(q), ptr(k), ptr(v), ptr(dout), ptr(P), ptr(sel), ptr(dS),
                                                 ptr(dq), ptr(dk), ptr(dv), stream_ptr()), "prob_attention_backward")
        return dq, dk, dv, None, None, None, None


def prob_attention_composed(q, k, v, index_sample, n_top, scale, causal, want_sel=False):
    """the same function from torch ops (the cross-check, and the path outside the kernels' limits): the un-squeezed measure, ties in it
    to the lower query index (a stable descending sort), the selected set ascending.  No gradient flows through the measure."""
    _need_gpu(q, k, v, index_sample)
    B, LQ, H, D = q.shape
    LK = k.shape[1]
    Q, K, V = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)      # (B, H, L, D)
    idx = index_sample.long().clamp(0, LK - 1)
    with torch.no_grad():
        Ks = K[:, :, idx, :]                                                # (B, H, L_Q, U, D)
        QK = torch.einsum("bhld,bhlud->bhlu", Q, Ks)
        M = QK.max(-1).values - QK.sum(-1) / LK
        M = torch.where(torch.isnan(M), torch.full_like(M, float("-inf")), M)
        top = torch.sort(M, dim=-1, descending=True, stable=True).indices[..., :n_top]
        top = torch.sort(top, dim=-1).values                                # (B, H, u) ascending
    gather = top.unsqueeze(-1).expand(B, H, n_top, D)
    scores = torch.matmul(torch.gather(Q, 2, gather), K.transpose(-2, -1)) * scale
    if causal:
        assert LQ == LK
        keys = torch.arange(LK, device=q.device)
        scores = scores.masked_fill(keys[None, None, None, :] > top.unsqueeze(-1), float("-inf"))
        ctxt = V.cumsum(dim=-2)
    else:
        ctxt = V.mean(dim=-2, keepdim=True).expand(B, H, LQ, D)
    upd = torch.matmul(torch.softmax(scores, dim=-1), V)
    out = torch.scatter(ctxt.contiguous(), 2, gather, upd)
    return (out, top.int()) if want_sel else out


def prob_attention(q, k, v, index_sample, n_top, scale, causal, want_sel=False):
    """Informer's ProbAttention core on q (B, L_Q, H, D), k / v (B, L_K, H, D) with an explicit (L_Q, U_part) integer sample of key indices:
    -> (B, H, L_Q, D) contiguous (want_sel: also the selected query indices (B, H, n_top), ascending).  The kernels wherever
    prob_attention_supported allows and config.informer_fused is on, else prob_attention_composed.  fp32 in either precision mode."""
    if q.dim() != 4 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2:] != q.shape[2:] or index_sample.dim() != 2:
        raise _lib.ImmtsfError(f"prob_attention: shapes {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}, {tuple(index_sample.shape)}")
    q, k, v, index_sample = q.float(), k.float(), v.float(), index_sample.to(torch.int32)
    _need_gpu(q, k, v, index_sample)
    B, LQ, H, D = q.shape
    LK, U = k.shape[1], index_sample.shape[1]
    n_top = int(n_top)
    if index_sample.shape[0] != LQ or not 1 <= U or not 1 <= n_top <= LQ or (causal and LQ != LK):
        raise _lib.ImmtsfError(f"prob_attention: sample {tuple(index_sample.shape)}, n_top {n_top}, causal {causal} for L_Q {LQ}, L_K {LK}")
    if config.informer_fused and U <= LK and prob_attention_supported(LQ, LK, D, n_top):
        out, sel, _ = ProbAttentionFn.apply(q, k, v, index_sample, n_top, float(scale), bool(causal))
        return (out, sel) if want_sel else out
    return prob_attention_composed(q, k, v, index_sample, n_top, float(scale), bool(causal), want_sel)


def conv_distil_supported(d):
    """the widths the ConvLayer row kernels take (immtsf_conv_distil_supported; as residual_layernorm_supported): d % 4 == 0, d <= 1024"""
    return d % 4 == 0 and 4 <= d <= 1024


class ConvDistilFn(torch.autograd.Function):
    """BatchNorm1d + ELU + MaxPool1d(3, 2, 1) on the rows y (B, L + 2, d) of ConvLayer's product (immtsf_conv_distil_forward / _backward):
    two launches per direction, one for an evaluation forward.  The running buffers are updated in place by the kernel."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, batches, eps, momentum, training):
        lib = _lib.load()
        y = _c(y)
        _need_gpu(y, gamma, beta, running_mean, running_var)
        B, T, d = y.shape
        L = T - 2
        mean, rstd = torch.empty(d, dtype=torch.float32, device=y.device), torch.empty(d, dtype=torch.float32, device=y.device)
        out = torch.empty(B, (L + 1) // 2 + 1, d, dtype=torch.float32, device=y.device)
        ws = _bytes(lib.immtsf_conv_distil_workspace_bytes(B, L, d), y.device)
        check(lib.immtsf_conv_distil_forward(B, L, d, 1 if training else 0, ptr(y), ptr(gamma), ptr(beta), eps, momentum, ptr(running_mean),
                                             ptr(running_var), ptr(batches), ptr(mean), ptr(rstd), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "conv_distil_forward")
        ctx.save_for_backward(y, gamma, beta, mean, rstd)
        ctx.cfg = (B, L, d, 1 if training else 0)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        y, gamma, beta, mean, rstd = ctx.saved_tensors
        B, L, d, training = ctx.cfg
        dout = dout.contiguous()
        dn, dy = torch.empty_like(y), torch.empty_like(y)
        (dgamma, dbeta), rets = _grad_buffers((gamma, beta))
        ws = _bytes(lib.immtsf_conv_distil_workspace_bytes(B, L, d), y.device)
        check(lib.immtsf_conv_distil_backward(B, L, d, training, ptr(y), ptr(gamma), ptr(beta), ptr(mean), ptr(rstd), ptr(dout), ptr(dn), ptr(dy),
                                              ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream_ptr()), "conv_distil_backward")
        return dy, rets[0], rets[1], None, None, None, None, None, None


def conv_distil(x, conv, norm, training, precision=None):
    """Informer's ConvLayer on x (B, L, d), L >= 2: conv = nn.Conv1d(d, d, 3, padding=2, padding_mode="circular"), norm = nn.BatchNorm1d(d)
    with affine parameters, running statistics and a float momentum -> (B, (L + 1) // 2 + 1, d).  The three taps are ONE product of the
    GEMM family over the gathered image [x[t-2], x[t-1], x[t]] (indices mod L) of L + 2 rows; everything behind it is ConvDistilFn."""
    _need_gpu(x)
    B, L, d = x.shape
    if L < 2 or not conv_distil_supported(d) or tuple(conv.weight.shape) != (d, d, 3):
        raise _lib.ImmtsfError(f"conv_distil: x {tuple(x.shape)}, weight {tuple(conv.weight.shape)} is outside the kernel")
    x = x.float()
    xw = torch.cat([x[:, L - 2:], x, x[:, :2]], dim=1)                                      # xw[m] = x[(m - 2) mod L], L + 4 rows
    img = torch.cat([xw[:, 0:L + 2], xw[:, 1:L + 3], xw[:, 2:L + 4]], dim=-1)               # (B, L + 2, 3 d): tap k at columns k d ..
    W3 = conv.weight.permute(0, 2, 1).reshape(d, 3 * d)
    y = linear(img, W3, conv.bias, precision)
    return ConvDistilFn.apply(y, norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.num_batches_tracked, float(norm.eps),
                              float(norm.momentum), bool(training))


# ---- Informer's model stages (csrc/informer.hip): everything of models/Informer.py that is not a layer
SITE_INFORMER_ENC = SITE_LAYER_BASE + 46      # enc_embedding's dropout: element (b input_len + l) d_model + f
SITE_INFORMER_DEC = SITE_LAYER_BASE + 47      # dec_embedding's dropout: element (b pred_len + t) d_model + f


def informer_model_supported(input_len, pred_len, Cc, d_model):
    """the limits of the fused Informer stages (immtsf_informer_model_supported): 1 <= input_len, pred_len <= 512, 1 <= C <= 32,
    d_model % 4 == 0, 4 <= d_model <= 512 or a multiple of 64 up to 1024"""
    return bool(_lib.load().immtsf_informer_model_supported(int(input_len), int(pred_len), int(Cc), int(d_model)))


class InformerFrontFn(torch.autograd.Function):
    """padding, masked instance norm, the two input concatenations and both DataEmbeddings as ONE launch; backward = the two token
    weights' gradients in TWO (immtsf_informer_front_forward / _backward).  data / mask (B, L, C), tp (B, L), tpp (B, Lp) are data: no
    gradient.  dims = (input_len, pred_len); drop = (p, seed, counter pointer).  -> enc (B, input_len, D), dec (B, pred_len, D), means,
    stdev (B, 1, C)."""

    @staticmethod
    def forward(ctx, data, mask, tp, tpp, W_enc, W_dec, pe_enc, pe_dec, dims, drop):
        lib = _lib.load()
        data, mask, tp, tpp, W_enc, W_dec, pe_enc, pe_dec = (_c(t) for t in (data, mask, tp, tpp, W_enc, W_dec, pe_enc, pe_dec))
        _need_gpu(data, mask, tp, tpp, W_enc, W_dec, pe_enc, pe_dec)
        (B, L, Cc), Lp, (S, P), D = data.shape, tpp.shape[1], dims, W_enc.shape[0]
        p, seed, cnt = drop
        dev = data.device
        stats = torch.empty(2, B, 1, Cc, dtype=torch.float32, device=dev)
        enc = torch.empty(B, S, D, dtype=torch.float32, device=dev)
        dec = torch.empty(B, P, D, dtype=torch.float32, device=dev)
        check(lib.immtsf_informer_front_forward(B, L, S, Lp, P, Cc, D, ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(W_enc), ptr(W_dec),
                                                ptr(pe_enc), ptr(pe_dec), ptr(stats[0]), ptr(stats[1]), ptr(enc), ptr(dec), p, seed,
                                                SITE_INFORMER_ENC, SITE_INFORMER_DEC, cnt, stream_ptr()), "informer_front_forward")
        ctx.cfg = (B, L, S, Lp, P, Cc, D, p, seed, cnt)
        ctx.save_for_backward(data, mask, tp, tpp, stats)
        ctx.mark_non_differentiable(stats)
        return enc, dec, stats

    @staticmethod
    def backward(ctx, d_enc, d_dec, _d_stats):
        lib = _lib.load()
        data, mask, tp, tpp, stats = ctx.saved_tensors
        B, L, S, Lp, P, Cc, D, p, seed, cnt = ctx.cfg
        dev = data.device
        d_enc = torch.zeros(B, S, D, dtype=torch.float32, device=dev) if d_enc is None else d_enc.contiguous()
        d_dec = torch.zeros(B, P, D, dtype=torch.float32, device=dev) if d_dec is None else d_dec.contiguous()
        dW = torch.empty(2, D, 2 * Cc + 1, 3, dtype=torch.float32, device=dev)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_informer_front_workspace_bytes(B, S, P, Cc, D), dev)
        check(lib.immtsf_informer_front_backward(B, L, S, Lp, P, Cc, D, ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(stats[0]), ptr(stats[1]),
                                                 ptr(d_enc), ptr(d_dec), ptr(dW[0]), ptr(dW[1]), p, seed, SITE_INFORMER_ENC,
                                                 SITE_INFORMER_DEC, cnt, ptr(ws), ws.numel(), stream_ptr()), "informer_front_backward")
        return (None,) * 4 + (dW[0] if ctx.needs_input_grad[4] else None, dW[1] if ctx.needs_input_grad[5] else None) + (None,) * 4


def informer_front(data, mask, tp, tpp, input_len, pred_len, W_enc, W_dec, pe_enc, pe_dec, p_drop=0.0, training=False, seed=None):
    """data, mask (B, L <= input_len, C), tp (B, L), tpp (B, Lp <= pred_len) -> (enc (B, input_len, D), dec (B, pred_len, D), means,
    stdev (B, 1, C)) of Informer's front end.  W_enc / W_dec: the two tokenConv weights (D, 2C + 1, 3); pe_enc / pe_dec: the positional
    tables (1, n, D) or (n, D).  The dropout masks are those of SITE_INFORMER_ENC / SITE_INFORMER_DEC under `seed` (None: a fresh
    config.next_seed())."""
    B, L, Cc = data.shape
    D, Lp = W_enc.shape[0], tpp.shape[1]
    pe_enc, pe_dec = pe_enc.reshape(-1, pe_enc.shape[-1]), pe_dec.reshape(-1, pe_dec.shape[-1])
    if not (informer_model_supported(input_len, pred_len, Cc, D) and B >= 1 and 1 <= L <= input_len and 1 <= Lp <= pred_len) or \
            tuple(mask.shape) != (B, L, Cc) or tuple(tp.shape) != (B, L) or tpp.shape[0] != B or \
            tuple(W_enc.shape) != (D, 2 * Cc + 1, 3) or tuple(W_dec.shape) != (D, 2 * Cc + 1, 3) or \
            any(t.shape[0] < max(input_len, pred_len) or t.shape[1] != D for t in (pe_enc, pe_dec)):
        raise _lib.ImmtsfError(f"informer_front: shapes outside the fused kernel (B {B}, L {L}, input_len {input_len}, Lp {Lp}, pred_len "
                               f"{pred_len}, C {Cc}, d_model {D})")
    p = float(p_drop) if training else 0.0
    drop = (p, (config.next_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF) if p > 0 else 0,
            config.dropout_counter_ptr(data.device) if p > 0 else None)
    enc, dec, stats = InformerFrontFn.apply(data, mask, tp, tpp, W_enc, W_dec, pe_enc, pe_dec, (int(input_len), int(pred_len)), drop)
    return enc, dec, stats[0], stats[1]


class InformerTailFn(torch.autograd.Function):
    """decoder.norm -> decoder.projection -> * stdev + means on the rows t < Lp of x (B, pred_len, D) as ONE launch -> (B, Lp, C); backward =
    dx (exact zeros in rows t >= Lp), d gamma, d beta, dW, d bias in TWO (immtsf_informer_tail_forward / _backward).  means / stdev
    (B, 1, C) are data: no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, W, bias, means, stdev, Lp, eps):
        lib = _lib.load()
        x, gamma, beta, W, bias, means, stdev = (_c(t) for t in (x, gamma, beta, W, bias, means, stdev))
        _need_gpu(x, gamma, beta, W, bias, means, stdev)
        B, P, D = x.shape
        Cc = W.shape[0]
        y = torch.empty(B, Lp, Cc, dtype=torch.float32, device=x.device)
        rows = torch.empty(2, B * Lp, dtype=torch.float32, device=x.device)      # mean, rstd of every normalised row
        check(lib.immtsf_informer_tail_forward(B, Lp, P, Cc, D, ptr(x), ptr(gamma), ptr(beta), eps, ptr(W), ptr(bias), ptr(means), ptr(stdev),
                                               ptr(y), ptr(rows[0]), ptr(rows[1]), stream_ptr()), "informer_tail_forward")
        ctx.cfg = (B, Lp, P, Cc, D)
        ctx.save_for_backward(x, gamma, beta, W, stdev, rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, beta, W, stdev, rows = ctx.saved_tensors
        B, Lp, P, Cc, D = ctx.cfg
        dx = torch.empty_like(x)
        flat = torch.empty(2 * D + Cc * D + Cc, dtype=torch.float32, device=x.device)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_informer_tail_workspace_bytes(B, Lp, Cc, D), x.device)
        check(lib.immtsf_informer_tail_backward(B, Lp, P, Cc, D, ptr(x), ptr(gamma), ptr(beta), ptr(W), ptr(stdev), ptr(rows[0]), ptr(rows[1]),
                                                ptr(dy.contiguous()), ptr(dx), ptr(flat), ptr(ws), ws.numel(), stream_ptr()),
              "informer_tail_backward")
        rets = (dx, flat[:D], flat[D:2 * D], flat[2 * D:2 * D + Cc * D].view(Cc, D), flat[2 * D + Cc * D:])
        return tuple(r if need else None for r, need in zip(rets, ctx.needs_input_grad[:5])) + (None,) * 4


def informer_tail(x, norm, projection, means, stdev, Lp):
    """x (B, pred_len, D) the last decoder layer's output, norm = nn.LayerNorm(D), projection = nn.Linear(D, C) with bias, means / stdev
    (B, 1, C) of the front end -> the de-normalised forecast (B, Lp <= pred_len, C), contiguous"""
    B, P, D = x.shape
    Cc = projection.weight.shape[0]
    if not (informer_model_supported(1, P, Cc, D) and 1 <= Lp <= P) or projection.bias is None or tuple(projection.weight.shape) != (Cc, D) or \
            tuple(norm.weight.shape) != (D,) or norm.bias is None or means.numel() != B * Cc or stdev.numel() != B * Cc:
        raise _lib.ImmtsfError(f"informer_tail: shapes outside the fused kernel (B {B}, Lp {Lp}, pred_len {P}, C {Cc}, d_model {D})")
    return InformerTailFn.apply(x.float(), norm.weight, norm.bias, projection.weight, projection.bias, means, stdev, int(Lp), float(norm.eps))


# ---- TimesNet's model stages (csrc/timesnet_model.hip, csrc/informer.hip's tail): everything of models/TimesNet.py around the TimesBlocks
SITE_TIMESNET_EMBED = SITE_LAYER_BASE + 41      # token_embed's site and element (b input_len + s) d_model + f: either route, one mask


def timesnet_model_supported(input_len, pred_len, Cc, d_model):
    """the limits of the fused TimesNet stages (immtsf_timesnet_model_supported): input_len + pred_len <= 256, 1 <= C <= 10,
    d_model % 4 == 0, 4 <= d_model <= 512"""
    return bool(_lib.load().immtsf_timesnet_model_supported(int(input_len), int(pred_len), int(Cc), int(d_model)))


class TimesNetFrontFn(torch.autograd.Function):
    """padding, plain instance norm, the input concatenation, DataEmbedding, the horizon rows and predict_linear as ONE launch; backward =
    d predict_linear.weight / .bias and d tokenConv.weight in TWO (immtsf_timesnet_front_forward / _backward).  data / mask (B, L, C),
    tp (B, L), tpp (B, Lp) are data: no gradient.  dims = (input_len, pred_len); drop = (p, seed, counter pointer, site); save_e: keep
    the embedded rows for the backward instead of forming them again.  -> enc (B, input_len + pred_len, D), stats (2, B, 1, C)."""

    @staticmethod
    def forward(ctx, data, mask, tp, tpp, W_tok, pe, W_pred, b_pred, dims, drop, save_e):
        lib = _lib.load()
        data, mask, tp, tpp, W_tok, pe, W_pred, b_pred = (_c(t) for t in (data, mask, tp, tpp, W_tok, pe, W_pred, b_pred))
        _need_gpu(data, mask, tp, tpp, W_tok, pe, W_pred, b_pred)
        (B, L, Cc), Lp, (S, P), D = data.shape, tpp.shape[1], dims, W_tok.shape[0]
        p, seed, cnt, site = drop
        dev = data.device
        stats = torch.empty(2, B, 1, Cc, dtype=torch.float32, device=dev)
        enc = torch.empty(B, S + P, D, dtype=torch.float32, device=dev)
        E = torch.empty(B, S, D, dtype=torch.float32, device=dev) if save_e else None
        check(lib.immtsf_timesnet_front_forward(B, L, S, Lp, P, Cc, D, ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(W_tok), ptr(pe), ptr(W_pred),
                                                ptr(b_pred), ptr(stats[0]), ptr(stats[1]), ptr(enc), ptr(E), p, seed, site, cnt, stream_ptr()),
              "timesnet_front_forward")
        ctx.cfg = (B, L, S, Lp, P, Cc, D, p, seed, cnt, site)
        ctx.save_for_backward(data, mask, tp, tpp, W_tok, pe, W_pred, stats, E)
        ctx.mark_non_differentiable(stats)
        return enc, stats

    @staticmethod
    def backward(ctx, d_enc, _d_stats):
        lib = _lib.load()
        data, mask, tp, tpp, W_tok, pe, W_pred, stats, E = ctx.saved_tensors
        B, L, S, Lp, P, Cc, D, p, seed, cnt, site = ctx.cfg
        dev, T, Kc = data.device, S + P, 2 * Cc + 1
        flat = torch.empty(T * T + T + D * Kc * 3, dtype=torch.float32, device=dev)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_timesnet_front_workspace_bytes(B, S, P, Cc, D), dev)
        check(lib.immtsf_timesnet_front_backward(B, L, S, Lp, P, Cc, D, ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(W_tok), ptr(pe), ptr(W_pred),
                                                 ptr(stats[0]), ptr(stats[1]), ptr(E), ptr(d_enc.contiguous()), ptr(flat), p, seed, site, cnt,
                                                 ptr(ws), ws.numel(), stream_ptr()), "timesnet_front_backward")
        need = ctx.needs_input_grad
        return (None,) * 4 + (flat[T * T + T:].view(D, Kc, 3) if need[4] else None, None, flat[:T * T].view(T, T) if need[6] else None,
                              flat[T * T:T * T + T] if need[7] else None) + (None,) * 3


def timesnet_front(data, mask, tp, tpp, input_len, pred_len, W_token, pe, W_predict, b_predict, p_drop=0.0, training=False, seed=None,
                   save_e=None):
    """data, mask (B, L <= input_len, C), tp (B, L), tpp (B, Lp <= pred_len) -> (enc (B, input_len + pred_len, D), means, stdev (B, 1, C)) of
    TimesNet's front end.  W_token: enc_embedding's tokenConv weight (D, 2C + 1, 3); pe: its positional table (1, n, D) or (n, D);
    W_predict (T, T), b_predict (T): predict_linear.  The dropout mask is token_embed's: one config.next_seed() when p > 0 in training
    (`seed` overrides it), SITE_TIMESNET_EMBED.  save_e None: config.timesnet_model_save_e."""
    B, L, Cc = data.shape
    D, Lp, T = W_token.shape[0], tpp.shape[1], input_len + pred_len
    pe = pe.reshape(-1, pe.shape[-1])
    if not (timesnet_model_supported(input_len, pred_len, Cc, D) and B >= 1 and 1 <= L <= input_len and 1 <= Lp <= pred_len) or \
            tuple(mask.shape) != (B, L, Cc) or tuple(tp.shape) != (B, L) or tpp.shape[0] != B or tuple(W_token.shape) != (D, 2 * Cc + 1, 3) or \
            pe.shape[0] < input_len or pe.shape[1] != D or tuple(W_predict.shape) != (T, T) or b_predict is None or \
            tuple(b_predict.shape) != (T,):
        raise _lib.ImmtsfError(f"timesnet_front: shapes outside the fused kernel (B {B}, L {L}, input_len {input_len}, Lp {Lp}, pred_len "
                               f"{pred_len}, C {Cc}, d_model {D})")
    p = float(p_drop) if training else 0.0
    drop = (p, (config.next_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF) if p > 0 else 0,
            config.dropout_counter_ptr(data.device) if p > 0 else None, SITE_TIMESNET_EMBED)
    enc, stats = TimesNetFrontFn.apply(data, mask, tp, tpp, W_token, pe, W_predict, b_predict, (int(input_len), int(pred_len)), drop,
                                       bool(config.timesnet_model_save_e if save_e is None else save_e))
    return enc, stats[0], stats[1]


class TimesNetTailFn(torch.autograd.Function):
    """layer_norm -> projection -> * stdev + means on the rows off .. off + Lp - 1 of x (B, T, D) as ONE launch -> (B, Lp, C); backward = dx
    (exact zeros on every other row), d gamma, d beta, dW, d bias in TWO (immtsf_timesnet_tail_forward / _backward: InformerTailFn's
    kernels with a row offset).  means / stdev (B, 1, C) are data: no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, W, bias, means, stdev, off, Lp, eps):
        lib = _lib.load()
        x, gamma, beta, W, bias, means, stdev = (_c(t) for t in (x, gamma, beta, W, bias, means, stdev))
        _need_gpu(x, gamma, beta, W, bias, means, stdev)
        B, T, D = x.shape
        Cc = W.shape[0]
        y = torch.empty(B, Lp, Cc, dtype=torch.float32, device=x.device)
        rows = torch.empty(2, B * Lp, dtype=torch.float32, device=x.device)      # mean, rstd of every normalised row
        check(lib.immtsf_timesnet_tail_forward(B, Lp, T, off, Cc, D, ptr(x), ptr(gamma), ptr(beta), eps, ptr(W), ptr(bias), ptr(means),
                                               ptr(stdev), ptr(y), ptr(rows[0]), ptr(rows[1]), stream_ptr()), "timesnet_tail_forward")
        ctx.cfg = (B, Lp, T, off, Cc, D)
        ctx.save_for_backward(x, gamma, beta, W, stdev, rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, beta, W, stdev, rows = ctx.saved_tensors
        B, Lp, T, off, Cc, D = ctx.cfg
        dx = torch.empty_like(x)
        flat = torch.empty(2 * D + Cc * D + Cc, dtype=torch.float32, device=x.device)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_informer_tail_workspace_bytes(B, Lp, Cc, D), x.device)
        check(lib.immtsf_timesnet_tail_backward(B, Lp, T, off, Cc, D, ptr(x), ptr(gamma), ptr(beta), ptr(W), ptr(stdev), ptr(rows[0]),
                                                ptr(rows[1]), ptr(dy.contiguous()), ptr(dx), ptr(flat), ptr(ws), ws.numel(), stream_ptr()),
              "timesnet_tail_backward")
        rets = (dx, flat[:D], flat[D:2 * D], flat[2 * D:2 * D + Cc * D].view(Cc, D), flat[2 * D + Cc * D:])
        return tuple(r if need else None for r, need in zip(rets, ctx.needs_input_grad[:5])) + (None,) * 5


def timesnet_tail(x, norm, projection, means, stdev, input_len, Lp):
    """x (B, T, D) the last TimesBlock's output (before the last layer_norm), norm = nn.LayerNorm(D), projection = nn.Linear(D, C) with
    bias, means / stdev (B, 1, C) of the front end -> the de-normalised forecast of rows input_len .. input_len + Lp - 1: (B, Lp, C)"""
    B, T, D = x.shape
    Cc = projection.weight.shape[0]
    if not (informer_model_supported(1, T, Cc, D) and Lp >= 1 and input_len >= 0 and input_len + Lp <= T) or projection.bias is None or \
            tuple(projection.weight.shape) != (Cc, D) or tuple(norm.weight.shape) != (D,) or norm.bias is None or \
            means.numel() != B * Cc or stdev.numel() != B * Cc:
        raise _lib.ImmtsfError(f"timesnet_tail: shapes outside the fused kernel (B {B}, rows {input_len} + {Lp} of {T}, C {Cc}, d_model {D})")
    return TimesNetTailFn.apply(x.float(), norm.weight, norm.bias, projection.weight, projection.bias, means, stdev, int(input_len), int(Lp),
                                float(norm.eps))


# ------------------------------------------------------------------------------------------------ CRU backbone
def cru_supported(lsd, num_basis, bandwidth, T):
    """the limits of the fused CRU recurrence (immtsf_cru_supported): lsd even, 2 <= lsd <= 32, num_basis <= 256, bandwidth <= lsd / 2,
    1 <= T <= 2^20"""
    return bool(_lib.load().immtsf_cru_supported(int(lsd), int(num_basis), int(bandwidth), int(T)))


def _cru_layout(lsd, K, bw):
    """-> (the nine float offsets of [tm11 | tm12 | tm21 | tm22 | coef_w | coef_b | trans_var | icu | icl] in the flat gradient, its length)"""
    return _grad_layout("immtsf_cru_grad_layout", (lsd, K, bw), 9,
                        f"cru_scan: dimensions outside the fused kernel (lsd {lsd}, num_basis {K}, bandwidth {bw})")


class CRUScanFn(torch.autograd.Function):
    """The Kalman recurrence of a CRU layer (masked update, coefficient softmax, basis mix, matrix exponential, prior mean and covariance
    diagonals over all T time points) as ONE launch; backward = TWO (immtsf_cru_forward / _backward, csrc/cru.hip).  The posterior
    covariances are returned for their readers but carry no gradient (forecasting() never reads the variance decoder); the times and
    the validity flags are data.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, y, y_var, valid, t, bandwidth, *params):
        lib = _lib.load()
        y, y_var, valid, t = _c(y), _c(y_var), _c(valid), _c(t)
        params = tuple(_c(q) for q in params)
        _need_gpu(y, y_var, valid, t, *params)
        B, T, lod = y.shape
        lsd, K = 2 * lod, params[0].shape[0]
        pm = torch.empty(B, T, lsd, dtype=torch.float32, device=y.device)
        cov = torch.empty(3, B, T, lod, dtype=torch.float32, device=y.device)
        if B > 0:
            check(lib.immtsf_cru_forward(B, T, lsd, K, bandwidth, ptr(y), ptr(y_var), ptr(valid), ptr(t), *(ptr(q) for q in params), ptr(pm),
                                         ptr(cov[0]), ptr(cov[1]), ptr(cov[2]), stream_ptr()), "cru_forward")
        ctx.dims = (B, T, lsd, K, bandwidth)
        ctx.shapes = [tuple(q.shape) for q in params]
        ctx.save_for_backward(y, y_var, valid, t, pm, cov, *params)
        cu, cl, cs = cov[0], cov[1], cov[2]
        ctx.mark_non_differentiable(cu, cl, cs)
        return pm, cu, cl, cs

    @staticmethod
    def backward(ctx, dpm, *_):
        lib = _lib.load()
        y, y_var, valid, t, pm, cov = ctx.saved_tensors[:6]
        params = ctx.saved_tensors[6:]
        B, T, lsd, K, bw = ctx.dims
        offs, nv = _cru_layout(lsd, K, bw)
        flat = torch.empty(nv, dtype=torch.float32, device=y.device)      # every entry is written: no zero fill
        dy = torch.empty(2, B, T, lsd // 2, dtype=torch.float32, device=y.device)
        ws = _bytes(lib.immtsf_cru_workspace_bytes(B, T, lsd, K, bw), y.device)
        check(lib.immtsf_cru_backward(B, T, lsd, K, bw, ptr(y), ptr(y_var), ptr(valid), ptr(t), *(ptr(q) for q in params), ptr(pm), ptr(cov[0]),
                                      ptr(cov[1]), ptr(cov[2]), ptr(dpm.contiguous()), ptr(dy[0]), ptr(dy[1]), ptr(flat), ptr(ws), ws.numel(),
                                      stream_ptr()), "cru_backward")
        rets = _flat_views(flat, offs, ctx.shapes, ctx.needs_input_grad[5:])
        return (dy[0] if ctx.needs_input_grad[0] else None, dy[1] if ctx.needs_input_grad[1] else None, None, None, None) + tuple(rets)


def cru_scan(y, y_var, valid, t, bandwidth, tm11, tm12, tm21, tm22, coef_w, coef_b, trans_var, icu, icl):
    """y, y_var (B, T, lod) latent observations and variances, valid (B, T) bool / uint8, t (B, T) time stamps; tm** (K, E) the flat banded
    bases, coef_w (K, 2 lod), coef_b (K), trans_var (2 lod values) / icu / icl (lod values) the ACTIVATED variances -> post_mean (B, T, 2 lod)
    and the posterior covariance vectors cu, cl, cs (B, T, lod) of the continuous CRU cell.  Gradients reach y, y_var and the parameters."""
    B, T, lod = y.shape
    lsd, K = 2 * lod, tm11.shape[0]
    if valid.dtype == torch.bool:
        valid = valid.view(torch.uint8)
    if B < 1 or not cru_supported(lsd, K, bandwidth, T) or B * T * lsd >= 1 << 31:
        raise _lib.ImmtsfError(f"cru_scan: shapes outside the fused kernel (B {B}, T {T}, lsd {lsd}, num_basis {K}, bandwidth {bandwidth})")
    E = _cru_layout(lsd, K, int(bandwidth))[0][1] // K
    want = [(K, E)] * 4 + [(K, lsd), (K,), lsd, lod, lod]
    params = (tm11, tm12, tm21, tm22, coef_w, coef_b, trans_var, icu, icl)
    if tuple(y_var.shape) != (B, T, lod) or tuple(valid.shape) != (B, T) or tuple(t.shape) != (B, T) or valid.dtype != torch.uint8 or \
            any(q.dtype != torch.float32 for q in (y, y_var, t) + params) or \
            any((q.numel() != w) if isinstance(w, int) else (tuple(q.shape) != w) for q, w in zip(params, want)):
        raise _lib.ImmtsfError("cru_scan: the tensors are not the fp32 tensors of these dimensions")
    return CRUScanFn.apply(y, y_var, valid, t, int(bandwidth), *params)


# ------------------------------------------------------------------------------------------------ TimeLLM's frozen GPT-2 body
GPT2_SITE_EMBD = 65536           # include/immtsf.h IMMTSF_SITE_GPT2_*


def gpt2_sites(layer):
    """(attention, first residual, second residual) dropout sites of block `layer`; the embedding dropout is GPT2_SITE_EMBD"""
    return 65537 + 3 * layer, 65538 + 3 * layer, 65539 + 3 * layer


def _gpt2_inner(cfg):
    return cfg.n_inner if cfg.n_inner is not None else 4 * cfg.n_embd


def _gpt2_model_ok(llm_model):
    """what gpt2_body_supported and gpt2_embed_notes_supported ask of the model alone"""
    from transformers import GPT2Model
    if not isinstance(llm_model, GPT2Model):
        return False
    cfg = llm_model.config
    if (cfg.activation_function != "gelu_new" or not cfg.scale_attn_weights or cfg.scale_attn_by_inverse_layer_idx or
            cfg.reorder_and_upcast_attn or getattr(cfg, "add_cross_attention", False) or len(llm_model.h) < 1):
        return False
    return not (int(cfg.n_embd) % 8 or _gpt2_inner(cfg) % 8 or any(p.dtype != torch.float32 for p in llm_model.parameters()))


def gpt2_body_supported(llm_model, S_p, S_t):
    """the limits of gpt2_body: a transformers GPT2Model with head_dim 64, gelu_new, scaled attention weights, neither the inverse-layer
    scale nor the reordered up-cast attention, no cross attention, fp32 parameters, S = S_p + S_t <= n_positions and <= 1024"""
    if S_p < 0 or S_t < 1 or not _gpt2_model_ok(llm_model):
        return False
    cfg = llm_model.config
    return bool(_lib.load().immtsf_gpt2_supported(int(cfg.n_embd), int(cfg.n_head), int(S_p + S_t), int(cfg.n_positions)))


split_product_calls = 0          # products of the frozen bodies / note-embedding operators that ran on immtsf_gemm_split
asplit_product_calls = 0         # ... and, for a Llama stored in bf16 in fp32 mode, on immtsf_gemm_asplit


def _split_images(W):
    """(hi, lo) bf16 images of a contiguous fp32 tensor: hi = bf16(W), lo = bf16(W - hi), the operands of csrc/gemm_split.hip"""
    hi = torch.empty(W.shape, dtype=torch.bfloat16, device=W.device)
    lo = torch.empty_like(hi)
    check(_lib.load().immtsf_split_bf16(ptr(W), W.numel(), ptr(hi), ptr(lo), stream_ptr()), "split_bf16")
    return hi, lo


# ---- host helpers of the frozen-LLM drivers (the three TimeLLM bodies and the three note embedders below) --------------------------------
class _FrozenEntry:
    """what _frozen_cached keeps: the fp32 items `build` made (w: the first, the weight) and, made when first asked for, w's bf16 image
    and its (hi, lo) pair"""
    __slots__ = ("key", "items", "w", "w16", "split")

    def __init__(self, key, items):
        self.key, self.items, self.w, self.w16, self.split = key, items, items[0], None, None

    def image(self, bf, sp):
        if bf:
            if self.w16 is None:
                self.w16 = torch.empty(self.w.shape, dtype=torch.bfloat16, device=self.w.device)
                check(_lib.load().immtsf_f32_to_bf16(ptr(self.w), ptr(self.w16), self.w.numel(), stream_ptr()), "f32_to_bf16")
            return self.w16
        if sp:
            if self.split is None:
                self.split = _split_images(self.w)
            return self.split
        return None


def _frozen_cached(model, owner, slot, params, build):
    """the _FrozenEntry of (owner, slot), cached on the model and keyed by the storage address, version and shape of every parameter in
    `params`: load_state_dict(), .to() or any in-place write makes a new one, by build() -> the tuple of contiguous fp32 items"""
    cache = model.__dict__.setdefault("_immtsf_frozen", {})
    key = tuple([(p.data_ptr(), p._version, tuple(p.shape)) for p in params])
    hit = cache.get((id(owner), slot))
    if hit is None or hit.key != key:
        hit = cache[(id(owner), slot)] = _FrozenEntry(key, build())
    return hit


def _gpt2_w(model, W):
    return _frozen_cached(model, W, "w", (W,), lambda: (W.detach().contiguous(),))


def _gpt2_w16(model, W):
    """bf16 image of a frozen Conv1D weight, same (in, out) layout, cached and remade as _frozen_cached says"""
    return _gpt2_w(model, W).image(True, False)


def _gpt2_w_split(model, W):
    """(hi, lo) bf16 images of a frozen weight, same layout, in the entry that holds _gpt2_w16's image"""
    return _gpt2_w(model, W).image(False, True)


def _w_img(model, W, bf, sp):
    """what a frozen product reads beside the fp32 weight: its bf16 image in bf16 mode, its (hi, lo) pair under
    config.frozen_products == "split" in fp32 mode, else nothing"""
    return _gpt2_w(model, W).image(bf, sp) if (bf or sp) else None


_IN_PLACE = "in place"           # the `img` of a weight that is stored in bf16: the parameter is the image (a stored-bf16 Llama)


def _adr(t, off=0):
    """device pointer of element `off` of a tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


def _allocators(dev, bf=True):
    """(f32, b16): torch.empty(*shape) in that dtype on dev; with bf false, b16 gives None (no bf16 copy is kept in fp32 mode)"""
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)       # noqa: E731
    b16 = (lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)) if bf else (lambda *s: None)      # noqa: E731
    return f32, b16


def _tail_rows(t, B, rows_per_b, S_t):
    """the last S_t rows of every sequence of a (B rows_per_b, ...) tensor, compact"""
    if rows_per_b == S_t:
        return t
    return t.view(B, rows_per_b, -1)[:, rows_per_b - S_t:].contiguous().view(B * S_t, -1)


class _Carver:
    """carve(rows, cols, dt): the next matrix of a byte workspace, every start rounded up to 256 bytes -- the layout include/immtsf.h
    documents for the *_workspace_bytes functions; done() checks the bound, once"""

    def __init__(self, ws):
        self.ws, self.off = ws, 0

    def __call__(self, rows, cols, dt=torch.float32):
        nbytes = rows * cols * (2 if dt == torch.bfloat16 else 4)
        t = self.ws[self.off:self.off + nbytes].view(dt).view(rows, cols)
        self.off += (nbytes + 255) & ~255
        return t

    def done(self):
        assert self.off <= self.ws.numel()


def _frozen_gemm(lib, layout, precision, pa32, pa16, lda, W, img, w_off, ldb, out, c_off, ldc, bias, M, N, K, st, what="gpt2_gemm"):
    """out[.. c_off ..] (M, N; pitch ldc) = a (M, K; pitch lda) op(W[.. w_off ..]) + bias: one product of a frozen body.  pa32 / pa16
    and bias: pointers as the caller made them (bias already at its offset, or None); W the fp32 weight and `img` what _w_img gave for
    it, both read from element offset w_off at pitch ldb; out written from element offset c_off.  An (hi, lo) pair goes to
    immtsf_gemm_split when that supports the shape; anything else is immtsf_gpt2_gemm's call as it always was.  img _IN_PLACE: W is
    stored in bf16 and there is no fp32 weight -- bf16 mode hands its storage to immtsf_gpt2_gemm as the image (no route of that call
    reads a null fp32 operand: a shape the bf16-in-memory kernels refuse comes back as an error), fp32 mode is immtsf_gemm_asplit."""
    global split_product_calls, asplit_product_calls
    if img is _IN_PLACE:
        if precision == 1:
            check(lib.immtsf_gpt2_gemm(layout, 1, None, pa16, lda, None, _adr(W, w_off), ldb, _adr(out, c_off), ldc, bias, M, N, K, st),
                  what + " (stored bf16)")
        else:
            check(lib.immtsf_gemm_asplit(layout, pa32, lda, _adr(W, w_off), ldb, _adr(out, c_off), ldc, bias, M, N, K, st), what + " (asplit)")
            asplit_product_calls += 1
        return
    if isinstance(img, tuple):
        if lib.immtsf_gemm_split_supported(layout, M, N, K, lda, ldb, ldc):
            check(lib.immtsf_gemm_split(layout, pa32, lda, _adr(img[0], w_off), _adr(img[1], w_off), ldb, _adr(out, c_off), ldc, bias, M, N, K, st),
                  what + " (split)")
            split_product_calls += 1
            return
        img = None
    check(lib.immtsf_gpt2_gemm(layout, precision, pa32, pa16, lda, _adr(W, w_off), _adr(img, w_off), ldb, _adr(out, c_off), ldc, bias, M, N, K, st),
          what)


class _FrozenProducts:
    """the weight products of one pass over a frozen model in one precision mode: bf (bf16 mode), sp (fp32 mode under
    config.frozen_products == "split") and _frozen_gemm's calls for nn.Linear weights (N, K) and GPT-2's Conv1D weights (in, out), each
    read as it is stored.  stored: the model is a Llama stored in bf16 (_llama_model_kind) -- every weight is its own image, nothing is
    cached, and fp32 mode runs immtsf_gemm_asplit whatever config.frozen_products says"""

    def __init__(self, lib, model, precision, st):
        self.lib, self.model, self.precision, self.st = lib, model, precision, st
        self.bf = precision == 1
        self.stored = config.llama_stored_bf16 and _llama_model_kind(model) == "bf16"
        self.sp = config.frozen_split(precision) and not self.stored

    def pair(self, t32, t16):
        """(fp32 pointer, bf16 pointer) of an operand or a result kept in the mode's format: the other one is None"""
        return (None, ptr(t16)) if self.bf else (ptr(t32), None)

    def img(self, W):
        return _IN_PLACE if self.stored else _w_img(self.model, W, self.bf, self.sp)

    def mm(self, a32, a16, W, img, bias, rows, out, ldc, w_row=0, n_out=None, c_off=0):
        """out[:, c_off:c_off + n_out] = a (rows, K) W[w_row:w_row + n_out]^T + bias[w_row:..] (layout 0); img: W's image as _w_img gives it"""
        K = W.shape[1]
        n_out = W.shape[0] if n_out is None else n_out
        p32, p16 = self.pair(a32, a16)
        _frozen_gemm(self.lib, 0, self.precision, p32, p16, K, W, img, w_row * K, K, out, c_off, ldc, _adr(bias, w_row), rows, n_out, K, self.st)

    def lin(self, a32, a16, dense, rows, out):
        """out (rows, N) = a dense.weight^T + dense.bias"""
        self.mm(a32, a16, dense.weight, self.img(dense.weight), dense.bias, rows, out, dense.weight.shape[0])

    def mm_t(self, g32, g16, W, img, rows, g_off=0, ldg=None):
        """g (rows, N) W -> (rows, K) fp32: the backward of mm (layout 1); g_off, ldg: g is the columns g_off .. g_off + N - 1 of a buffer
        of pitch ldg"""
        N, K = W.shape
        o = torch.empty(rows, K, dtype=torch.float32, device=W.device)
        p32, p16 = (None, _adr(g16, g_off)) if self.bf else (_adr(g32, g_off), None)
        _frozen_gemm(self.lib, 1, self.precision, p32, p16, N if ldg is None else ldg, W, img, 0, K, o, 0, K, None, rows, K, N, self.st,
                     "gpt2_gemm (backward)")
        return o

    def lin_t(self, g32, g16, dense, rows):
        return self.mm_t(g32, g16, dense.weight, self.img(dense.weight), rows)

    def conv(self, pa, conv, M, N, K, out, ldc, w_off=0, c_off=0):
        """out[:, c_off:c_off + N] = a (M, K) W[:, w_off:w_off + N] + bias[w_off:..]: W (in, out) a Conv1D's weight (layout 1); pa: a's
        (fp32, bf16) pointers"""
        W = conv.weight
        _frozen_gemm(self.lib, 1, self.precision, pa[0], pa[1], K, W, self.img(W), w_off, W.shape[1], out, c_off, ldc,
                     _adr(conv.bias, w_off), M, N, K, self.st)

    def conv_t(self, g, conv, N, K):
        """g (M, K) fp32 W^T -> (M, N) fp32: the backward of conv (layout 0; the fp32 operand in either mode)"""
        W = conv.weight
        o = torch.empty(g.shape[0], N, dtype=torch.float32, device=g.device)
        _frozen_gemm(self.lib, 0, self.precision, ptr(g), None, K, W, _w_img(self.model, W, False, self.sp), 0, K, o, 0, N, None,
                     g.shape[0], N, K, self.st, "gpt2_gemm (backward)")
        return o


def _body_inputs(name, llm_model, prefix_embeds, tail_embeds, supported):
    """(tail, prefix or None, need_bwd) as the body Functions take them; raises outside `supported`"""
    tail = _c(tail_embeds.float())
    prefix = None if prefix_embeds is None or prefix_embeds.shape[1] == 0 else _c(prefix_embeds.detach().float())
    _need_gpu(tail, prefix)
    if not supported(llm_model, 0 if prefix is None else prefix.shape[1], tail.shape[1]):
        raise _lib.ImmtsfError(f"{name}: this body / sequence length is outside {name}_supported")
    return tail, prefix, torch.is_grad_enabled() and tail.requires_grad


def _body_drops(probs, training, seed):
    """(the dropout probabilities, zeros outside training; the Philox key: `seed`, or config.next_seed() when a dropout is on)"""
    drops = tuple(float(p) if training else 0.0 for p in probs)
    if seed is None:
        seed = config.next_seed() if any(p > 0.0 for p in drops) else 0
    return drops, int(seed) & 0xFFFFFFFFFFFFFFFF


def _notes_prologue(name, llm_model, ids, cu, precision, max_len, supported, d_of, widest_of, empty_first=False):
    """what the three *_embed_notes do before their first launch: the checks in their order, max_len (read from cu when not given: one
    device -> host copy), the pass's _FrozenProducts and the result buffer -> (pooled, done, ids, cu, max_len, products); done: pooled is
    the result already (no note, or no token at all).  d_of(cfg): the width, read before `supported` is asked; widest_of(cfg): the
    widest workspace row, read after it; empty_first: no note returns before the model is looked at"""
    _need_gpu(ids, cu)
    if ids.dtype != torch.int32 or cu.dtype != torch.int32 or ids.dim() != 1 or cu.dim() != 1 or cu.numel() < 1:
        raise _lib.ImmtsfError(f"{name}: ids (sum L) and cu (N + 1) are int32 vectors")
    ids, cu = _c(ids), _c(cu)
    N, T = cu.numel() - 1, ids.numel()
    d = d_of(llm_model.config)
    if N == 0 and empty_first:
        return torch.zeros(0, d, dtype=torch.float32, device=ids.device), True, ids, cu, max_len, None
    if max_len is None:
        max_len = int((cu[1:] - cu[:-1]).max()) if T and N else 1
    max_len = max(int(max_len), 1)
    if not supported(llm_model, max_len):
        raise _lib.ImmtsfError(f"{name}: this model / note length is outside {name}_supported")
    if N == 0:
        return torch.zeros(0, d, dtype=torch.float32, device=ids.device), True, ids, cu, max_len, None
    if T >= 2 ** 31 // (4 * widest_of(llm_model.config)):
        raise _lib.ImmtsfError(f"{name}: too many tokens for one call (split the batch)")
    products = _FrozenProducts(_lib.load(), llm_model, config.precision_code(precision), stream_ptr())
    pooled = torch.empty(N, d, dtype=torch.float32, device=ids.device)
    return (pooled.zero_() if T == 0 else pooled), T == 0, ids, cu, max_len, products


class GPT2BodyFn(torch.autograd.Function):
    """transformers' GPT2Model(inputs_embeds=cat([prefix, tail], 1)).last_hidden_state[:, -S_t:] on csrc/gpt2.hip + the GEMM family.  The
    body is frozen and only `tail` takes a gradient; attention is causal without a padding mask, so no prefix row depends on a tail row
    and the backward runs over the B S_t tail rows alone (exactly).  The last block computes queries, projections and the MLP for the tail
    rows only.  Saved per block: the c_attn output (K and V of all rows) and, for the tail rows, the block inputs, LayerNorm statistics,
    q, attention output, log-sum-exp and the MLP pre-activation."""

    @staticmethod
    def forward(ctx, tail, prefix, model, p_drops, precision, seed, need_bwd):
        lib = _lib.load()
        st = stream_ptr()
        cfg = model.config
        B, S_t, d = tail.shape
        S_p = 0 if prefix is None else prefix.shape[1]
        S, H, inner, L = S_p + S_t, int(cfg.n_head), _gpt2_inner(cfg), len(model.h)
        P = _FrozenProducts(lib, model, precision, st)
        bf = P.bf
        p_e, p_a, p_r = p_drops
        eps = float(cfg.layer_norm_epsilon)
        scale = 1.0 / float(d // H) ** 0.5
        f32, b16 = _allocators(tail.device)

        def mm(a32, a16, conv, M, N, K, out, ldc, w_off=0, c_off=0):      # (both pointers as they are: the attention output has both)
            P.conv((ptr(a32), ptr(a16)), conv, M, N, K, out, ldc, w_off, c_off)

        def ln(x, rows_per_b, s_from, norm, stats):
            n = B * (rows_per_b - s_from)
            y32, y16 = (None, b16(n, d)) if bf else (f32(n, d), None)
            mean, rstd = (f32(n), f32(n)) if stats else (None, None)
            check(lib.immtsf_gpt2_layernorm(ptr(x), B, rows_per_b, s_from, d, ptr(norm.weight), ptr(norm.bias), eps, ptr(y32), ptr(y16),
                                            ptr(mean), ptr(rstd), st), "gpt2_layernorm")
            return y32, y16, mean, rstd

        tl = lambda t, rows_per_b: _tail_rows(t, B, rows_per_b, S_t)      # noqa: E731

        x = f32(B * S, d)
        check(lib.immtsf_gpt2_embed(ptr(prefix), ptr(tail), ptr(model.wpe.weight), B, S_p, S_t, d, p_e, seed, GPT2_SITE_EMBD, ptr(x), st),
              "gpt2_embed")
        saved = []
        for li, blk in enumerate(model.h):
            qf = S_p if li == L - 1 else 0
            Sq = S - qf
            s_attn, s_r1, s_r2 = gpt2_sites(li)
            ca, cp, fc, mp = blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj
            h32, h16, mean1, rstd1 = ln(x, S, 0, blk.ln_1, need_bwd)
            qkv = f32(B * S, 3 * d)
            if qf == 0:
                mm(h32, h16, ca, B * S, 3 * d, d, qkv, 3 * d)
                q, ldq = qkv, 3 * d
            else:           # the last block: K and V of all rows, queries of the tail rows
                mm(h32, h16, ca, B * S, 2 * d, d, qkv, 3 * d, w_off=d, c_off=d)
                t32, t16, _, _ = ln(x, S, qf, blk.ln_1, False)
                q, ldq = f32(B * Sq, d), d
                mm(t32, t16, ca, B * Sq, d, d, q, d)
            ao32 = f32(B * Sq, d) if (need_bwd or not bf) else None
            ao16 = b16(B * Sq, d) if bf else None
            lse = f32(B, H, Sq) if need_bwd else None
            check(lib.immtsf_gpt2_attention_forward(ptr(q), ldq, _adr(qkv, d), _adr(qkv, 2 * d), 3 * d, B, S, H, qf, scale, p_a, seed, s_attn,
                                                    ptr(ao32), ptr(ao16), ptr(lse), st), "gpt2_attention_forward")
            pr = f32(B * Sq, d)
            mm(ao32, ao16, cp, B * Sq, d, d, pr, d)
            x1 = f32(B * Sq, d)
            check(lib.immtsf_gpt2_residual(ptr(x), B, S, qf, Sq, S, qf, d, ptr(pr), p_r, seed, s_r1, ptr(x1), st), "gpt2_residual")
            g32, g16, mean2, rstd2 = ln(x1, Sq, 0, blk.ln_2, need_bwd)
            pre = f32(B * Sq, inner)
            mm(g32, g16, fc, B * Sq, inner, d, pre, inner)
            a32, a16 = (None, b16(B * Sq, inner)) if bf else (f32(B * Sq, inner), None)
            check(lib.immtsf_gpt2_gelu(ptr(pre), pre.numel(), ptr(a32), ptr(a16), st), "gpt2_gelu")
            mo = f32(B * Sq, d)
            mm(a32, a16, mp, B * Sq, d, inner, mo, d)
            x2 = f32(B * Sq, d)
            check(lib.immtsf_gpt2_residual(ptr(x1), B, Sq, 0, Sq, S, qf, d, ptr(mo), p_r, seed, s_r2, ptr(x2), st), "gpt2_residual")
            if need_bwd:
                q_t = q if qf else qkv.view(B, S, 3 * d)[:, S_p:, :d].contiguous().view(B * S_t, d)
                lse_t = lse if Sq == S_t else lse[:, :, S_p:].contiguous()
                saved.append((tl(x, S), tl(mean1.view(-1, 1), S).view(-1), tl(rstd1.view(-1, 1), S).view(-1), q_t, qkv, tl(ao32, Sq), lse_t,
                              tl(x1, Sq), tl(mean2.view(-1, 1), Sq).view(-1), tl(rstd2.view(-1, 1), Sq).view(-1), tl(pre, Sq)))
            x = x2
        out = f32(B, S_t, d)
        mean_f, rstd_f = (f32(B * S_t), f32(B * S_t)) if need_bwd else (None, None)
        check(lib.immtsf_gpt2_layernorm(ptr(x), B, S_t, 0, d, ptr(model.ln_f.weight), ptr(model.ln_f.bias), eps, ptr(out), None, ptr(mean_f),
                                        ptr(rstd_f), st), "gpt2_layernorm")
        if need_bwd:
            ctx.saved, ctx.final = saved, (x, mean_f, rstd_f)
            ctx.model, ctx.dims, ctx.drops, ctx.seed, ctx.precision = model, (B, S_p, S_t, d, H, inner), p_drops, seed, precision
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        st = stream_ptr()
        model = ctx.model
        B, S_p, S_t, d, H, inner = ctx.dims
        S, M = S_p + S_t, B * S_t
        p_e, p_a, p_r = ctx.drops
        seed = ctx.seed
        mm_t = _FrozenProducts(lib, model, ctx.precision, st).conv_t
        scale = 1.0 / float(d // H) ** 0.5
        f32, _ = _allocators(dout.device)

        def ln_bwd(g, x, mean, rstd, norm, resid):
            o = f32(M, d)
            check(lib.immtsf_gpt2_layernorm_backward(ptr(g), ptr(x), ptr(mean), ptr(rstd), ptr(norm.weight), ptr(resid), M, d, ptr(o), st),
                  "gpt2_layernorm_backward")
            return o

        def undrop(g, p, site):        # the dropout's backward: the same mask, redrawn
            if p <= 0.0:
                return g
            o = f32(M, d)
            check(lib.immtsf_gpt2_residual(None, B, 0, 0, S_t, S, S_p, d, ptr(g), p, seed, site, ptr(o), st), "gpt2_residual (backward)")
            return o

        xf, mean_f, rstd_f = ctx.final
        dx = ln_bwd(dout.contiguous().view(M, d), xf, mean_f, rstd_f, model.ln_f, None)
        for li in reversed(range(len(model.h))):
            blk = model.h[li]
            x_t, mean1, rstd1, q_t, qkv, ao_t, lse_t, x1_t, mean2, rstd2, pre_t = ctx.saved[li]
            s_attn, s_r1, s_r2 = gpt2_sites(li)
            dact = mm_t(undrop(dx, p_r, s_r2), blk.mlp.c_proj, inner, d)
            dpre = f32(M, inner)
            check(lib.immtsf_gpt2_gelu_backward(ptr(pre_t), ptr(dact), dpre.numel(), ptr(dpre), st), "gpt2_gelu_backward")
            dx1 = ln_bwd(mm_t(dpre, blk.mlp.c_fc, d, inner), x1_t, mean2, rstd2, blk.ln_2, dx)
            dao = mm_t(undrop(dx1, p_r, s_r1), blk.attn.c_proj, d, d)
            dqkv = f32(M, 3 * d)
            check(lib.immtsf_gpt2_attention_backward(ptr(q_t), d, _adr(qkv, d), _adr(qkv, 2 * d), 3 * d, ptr(dao), ptr(ao_t), ptr(lse_t), B, S, H,
                                                     S_p, scale, p_a, seed, s_attn, ptr(dqkv), _adr(dqkv, d), _adr(dqkv, 2 * d), 3 * d, st),
                  "gpt2_attention_backward")
            dx = ln_bwd(mm_t(dqkv, blk.attn.c_attn, d, 3 * d), x_t, mean1, rstd1, blk.ln_1, dx1)
        dtail = undrop(dx, p_e, GPT2_SITE_EMBD)
        return dtail.view(B, S_t, d), None, None, None, None, None, None


def gpt2_body(llm_model, prefix_embeds, tail_embeds, training, precision=None, seed=None):
    """hidden_tail (B, S_t, d) = ln_f output of the last S_t rows of the frozen GPT-2 body over [prefix_embeds | tail_embeds].  Only
    tail_embeds takes a gradient (prefix_embeds may require one; it gets none).  training: the body's three dropouts (embd / attn / resid
    pdrop of its config) are drawn from immtsf's generator -- ops.dropout_keep_mask(seed, site, ...) reproduces them (GPT2_SITE_EMBD,
    gpt2_sites(layer)); seed: the Philox key, config.next_seed() by default.  Outside gpt2_body_supported this raises: callers check."""
    tail, prefix, need_bwd = _body_inputs("gpt2_body", llm_model, prefix_embeds, tail_embeds, gpt2_body_supported)
    cfg = llm_model.config
    drops, seed = _body_drops((cfg.embd_pdrop, cfg.attn_pdrop, cfg.resid_pdrop), training, seed)
    return GPT2BodyFn.apply(tail, prefix, llm_model, drops, config.precision_code(precision), seed, need_bwd)


# ------------------------------------------------------------------------------------------------ raw-text mode: notes through a frozen GPT-2
def gpt2_embed_notes_supported(llm_model, max_len):
    """the limits of gpt2_embed_notes: gpt2_body_supported's conditions on the model (a transformers GPT2Model with head_dim 64, gelu_new,
    scaled attention weights, neither the inverse-layer scale nor the reordered up-cast attention, no cross attention, fp32 parameters,
    d and the MLP width multiples of 8) and 1 <= max_len <= n_positions, <= 1024"""
    if max_len < 1 or not _gpt2_model_ok(llm_model):
        return False
    cfg = llm_model.config
    return bool(_lib.load().immtsf_note_embed_supported(int(cfg.n_embd), int(cfg.n_head), int(max_len), int(cfg.n_positions)))


def gpt2_embed_notes(llm_model, ids, cu, precision=None, max_len=None):
    """pooled (N, d) fp32: the mean over each note's tokens of the frozen GPT2Model's last hidden state -- reference
    fusions/load_llm.py embed_notes without the padding (csrc/note_embed.hip + the GEMM family + the row kernels of csrc/gpt2.hip over the
    packed rows).  ids (sum L) int32: the notes' real tokens back to back; cu (N + 1) int32: prefix sums of the token counts; both on the
    model's device.  A note of no tokens gives an exact zero row.  max_len: an upper bound of the token counts (read from cu when not
    given: one device -> host copy).  The model's parameters are read in place (the bf16 weight images of bf16 mode are gpt2_body's
    cache); runs under no_grad and saves nothing.  Outside gpt2_embed_notes_supported this raises: callers check."""
    with torch.no_grad():
        pooled, done, ids, cu, max_len, P = _notes_prologue(
            "gpt2_embed_notes", llm_model, ids, cu, precision, max_len, gpt2_embed_notes_supported, lambda cfg: int(cfg.n_embd),
            lambda cfg: max(int(cfg.n_embd), _gpt2_inner(cfg)), empty_first=True)
        if done:
            return pooled
        lib, st, precision, bf = P.lib, P.st, P.precision, P.bf
        cfg = llm_model.config
        (N, d), T = pooled.shape, ids.numel()
        H, inner = int(cfg.n_head), _gpt2_inner(cfg)
        eps = float(cfg.layer_norm_epsilon)
        scale = 1.0 / float(d // H) ** 0.5
        # one workspace for the whole pass, carved as include/immtsf.h lists it
        carve = _Carver(_bytes(lib.immtsf_note_embed_workspace_bytes(T, d, inner, precision), ids.device))
        op = torch.bfloat16 if bf else torch.float32
        x, x1, h, qkv, ao, pr, pre, act = (carve(T, d), carve(T, d), carve(T, d, op), carve(T, 3 * d), carve(T, d, op), carve(T, d),
                                           carve(T, inner), carve(T, inner, op))
        carve.done()

        def mm(a, conv, N_out, K, out):
            P.conv(P.pair(a, a), conv, T, N_out, K, out, N_out)

        def ln(src, norm, dst):
            check(lib.immtsf_gpt2_layernorm(ptr(src), 1, T, 0, d, ptr(norm.weight), ptr(norm.bias), eps, *P.pair(dst, dst), None, None, st),
                  "gpt2_layernorm")

        def add(base, y, dst):
            check(lib.immtsf_gpt2_residual(ptr(base), 1, T, 0, T, T, 0, d, ptr(y), 0.0, 0, 0, ptr(dst), st), "gpt2_residual")

        check(lib.immtsf_note_embed_tokens(ptr(ids), ptr(cu), N, T, ptr(llm_model.wte.weight), int(llm_model.wte.weight.shape[0]),
                                           ptr(llm_model.wpe.weight), int(llm_model.wpe.weight.shape[0]), d, ptr(x), st), "note_embed_tokens")
        for blk in llm_model.h:
            ln(x, blk.ln_1, h)
            mm(h, blk.attn.c_attn, 3 * d, d, qkv)
            check(lib.immtsf_note_embed_attention(ptr(qkv), 3 * d, ptr(cu), N, T, H, max_len, scale, precision, *P.pair(ao, ao), st),
                  "note_embed_attention")
            mm(ao, blk.attn.c_proj, d, d, pr)
            add(x, pr, x1)
            ln(x1, blk.ln_2, h)
            mm(h, blk.mlp.c_fc, inner, d, pre)
            check(lib.immtsf_gpt2_gelu(ptr(pre), pre.numel(), *P.pair(act, act), st), "gpt2_gelu")
            mm(act, blk.mlp.c_proj, d, inner, pr)
            add(x1, pr, x)
        check(lib.immtsf_note_embed_pool(ptr(x), ptr(cu), N, T, d, ptr(llm_model.ln_f.weight), ptr(llm_model.ln_f.bias), eps, ptr(pooled), st),
              "note_embed_pool")
        return pooled


# ------------------------------------------------------------------------------------------------ raw-text mode: notes through a frozen BERT
def bert_embed_notes_supported(llm_model, max_len):
    """the limits of bert_embed_notes: a transformers BertModel (the class itself; its pooler is ignored) with head_dim 64, hidden_act
    "gelu" (the erf form), absolute position embeddings, neither a decoder nor cross attention, at least one layer left after
    llm_layers_fusion has cut the stack, fp32 parameters, hidden_size and intermediate_size multiples of 8, and
    1 <= max_len <= max_position_embeddings, <= 1024"""
    from transformers import BertModel
    if type(llm_model) is not BertModel or max_len < 1:
        return False
    cfg = llm_model.config
    d, H = int(cfg.hidden_size), int(cfg.num_attention_heads)
    if (cfg.hidden_act != "gelu" or getattr(cfg, "position_embedding_type", None) not in (None, "absolute") or
            getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False) or len(llm_model.encoder.layer) < 1):
        return False
    if d % 8 or int(cfg.intermediate_size) % 8 or any(p.dtype != torch.float32 for p in llm_model.parameters()):
        return False
    return bool(_lib.load().immtsf_bert_embed_supported(d, H, int(max_len), int(cfg.max_position_embeddings)))


def _bert_qkv(model, att, bf, sp=False):
    """(W (3d, d), bias (3d), bf16 image of W or None) of one layer's query | key | value Linears, concatenated once and cached on the model,
    keyed by the six parameters' storage address and version: load_state_dict(), .to() or any in-place write makes a new one.  sp (fp32
    mode under config.frozen_products == "split"): the third item is W's (hi, lo) pair, cached in the same entry"""
    params = (att.query.weight, att.key.weight, att.value.weight, att.query.bias, att.key.bias, att.value.bias)
    hit = _frozen_cached(model, att, "qkv", params, lambda: (torch.cat([p.detach() for p in params[:3]], 0).contiguous(),
                                                             torch.cat([p.detach() for p in params[3:]], 0).contiguous()))
    return hit.w, hit.items[1], hit.image(bf, sp)


def bert_embed_notes(llm_model, ids, cu, precision=None, max_len=None):
    """pooled (N, d) fp32: the mean over each note's tokens of the frozen BertModel's last hidden state -- reference fusions/load_llm.py
    embed_notes without the padding (csrc/bert_embed.hip, the non-causal ragged attention of csrc/note_embed.hip and the GEMM family over
    the packed rows; 8 launches a layer + 2).  ids (sum L) int32: the notes' real tokens back to back; cu (N + 1) int32: prefix sums of the
    token counts; both on the model's device.  Token type 0 everywhere, as the reference calls the model.  A note of no tokens gives an
    exact zero row.  max_len: an upper bound of the token counts (read from cu when not given: one device -> host copy).  The model's
    parameters are read in place, but for the cached query | key | value concatenation and, in bf16 mode, the cached bf16 weight images;
    runs under no_grad and saves nothing.  Outside bert_embed_notes_supported this raises: callers check."""
    with torch.no_grad():
        pooled, done, ids, cu, max_len, P = _notes_prologue(
            "bert_embed_notes", llm_model, ids, cu, precision, max_len, bert_embed_notes_supported,
            lambda cfg: int(getattr(cfg, "hidden_size", 0)), lambda cfg: max(3 * int(cfg.hidden_size), int(cfg.intermediate_size)))
        if done:
            return pooled
        lib, st, precision, bf = P.lib, P.st, P.precision, P.bf
        cfg = llm_model.config
        (N, d), T = pooled.shape, ids.numel()
        H, inner = int(cfg.num_attention_heads), int(cfg.intermediate_size)
        eps = float(cfg.layer_norm_eps)
        scale = 1.0 / float(d // H) ** 0.5
        # one workspace for the whole pass, carved as include/immtsf.h lists it
        carve = _Carver(_bytes(lib.immtsf_bert_embed_workspace_bytes(T, d, inner, precision), ids.device))
        op = torch.bfloat16 if bf else torch.float32
        x, x1 = carve(T, d), carve(T, d)
        h = carve(T, d, torch.bfloat16) if bf else None
        qkv, ao, pr, pre, act = carve(T, 3 * d), carve(T, d, op), carve(T, d), carve(T, inner), carve(T, inner, op)
        carve.done()

        def add_ln(y, base, norm, dst):
            check(lib.immtsf_bert_embed_add_layernorm(ptr(y), ptr(base), T, d, ptr(norm.weight), ptr(norm.bias), eps, ptr(dst), ptr(h), st),
                  "bert_embed_add_layernorm")

        emb = llm_model.embeddings
        word, pos = emb.word_embeddings.weight, emb.position_embeddings.weight
        check(lib.immtsf_bert_embed_rows(ptr(ids), ptr(cu), N, T, ptr(word), int(word.shape[0]), ptr(pos), int(pos.shape[0]),
                                         ptr(emb.token_type_embeddings.weight), d, ptr(emb.LayerNorm.weight), ptr(emb.LayerNorm.bias), eps,
                                         ptr(x), ptr(h), st), "bert_embed_rows")
        for layer in llm_model.encoder.layer:
            att = layer.attention
            Wqkv, bqkv, Wqkv16 = _bert_qkv(llm_model, att.self, bf, P.sp)
            P.mm(x, h, Wqkv, Wqkv16, bqkv, T, qkv, 3 * d)
            check(lib.immtsf_bert_embed_attention(ptr(qkv), 3 * d, ptr(cu), N, T, H, max_len, scale, precision, *P.pair(ao, ao), st),
                  "bert_embed_attention")
            P.lin(ao, ao, att.output.dense, T, pr)
            add_ln(pr, x, att.output.LayerNorm, x1)
            P.lin(x1, h, layer.intermediate.dense, T, pre)
            check(lib.immtsf_bert_embed_gelu(ptr(pre), pre.numel(), *P.pair(act, act), st), "bert_embed_gelu")
            P.lin(act, act, layer.output.dense, T, pr)
            add_ln(pr, x1, layer.output.LayerNorm, x)
        check(lib.immtsf_bert_embed_pool(ptr(x), ptr(cu), N, T, d, ptr(pooled), st), "bert_embed_pool")
        return pooled


# ------------------------------------------------------------------------------------------------ raw-text mode: notes through a frozen Llama
_LLAMA_ROPE_TYPES = ("default", "linear", "llama3")      # inv_freq is fixed at construction: the module's buffer is the whole of it


def _llama_dims(cfg):
    """(d, H, H_kv, head_dim, inner) of a LlamaConfig"""
    d, H = int(cfg.hidden_size), int(cfg.num_attention_heads)
    return d, H, int(getattr(cfg, "num_key_value_heads", None) or H), int(getattr(cfg, "head_dim", None) or d // H), int(cfg.intermediate_size)


def _llama_model_kind(llm_model):
    """what llama_embed_notes_supported and llama_body_supported ask of the model alone, short of the library's answer on its widths and
    lengths: None outside the limits; "fp32" when every parameter is fp32; "bf16" when config.llama_stored_bf16 is on and every
    parameter is bf16 (a checkpoint stored in bf16, read in place: DESIGN 4v).  Mixed dtypes, fp16 and anything else: None"""
    from transformers import LlamaModel
    if type(llm_model) is not LlamaModel:
        return None
    cfg = llm_model.config
    _, _, _, hd, _ = _llama_dims(cfg)
    rope = getattr(llm_model, "rotary_emb", None)
    if (hd != 128 or cfg.hidden_act != "silu" or getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False) or
            len(llm_model.layers) < 1 or getattr(rope, "rope_type", None) not in _LLAMA_ROPE_TYPES or
            tuple(getattr(rope, "inv_freq", torch.zeros(0)).shape) != (64,)):
        return None
    dtypes = {p.dtype for p in llm_model.parameters()}
    if dtypes == {torch.float32}:
        return "fp32"
    if dtypes == {torch.bfloat16} and config.llama_stored_bf16:
        return "bf16"
    return None


def llama_embed_notes_supported(llm_model, max_len):
    """the limits of llama_embed_notes: a transformers LlamaModel (the class itself) with head_dim 128, H query heads over H_kv K/V heads
    with H / H_kv in {1, 2, 4, 8}, hidden_act "silu", neither attention nor MLP bias, rope_type default / linear / llama3 (those whose
    inv_freq does not depend on the call: dynamic, yarn and longrope keep the stock path), at least one layer, fp32 parameters -- or,
    with config.llama_stored_bf16 on, every parameter bf16 on one CUDA device --, hidden_size and intermediate_size multiples of 8, and
    1 <= max_len <= max_position_embeddings, <= 1024"""
    if max_len < 1:
        return False
    kind = _llama_model_kind(llm_model)
    if kind is None:
        return False
    if kind == "bf16":
        devices = {p.device for p in llm_model.parameters()}
        if len(devices) != 1 or next(iter(devices)).type != "cuda":
            return False
    cfg = llm_model.config
    d, H, H_kv, hd, inner = _llama_dims(cfg)
    return bool(_lib.load().immtsf_llama_embed_supported(d, H, H_kv, inner, int(max_len), int(cfg.max_position_embeddings)))


def _llama_cat(model, owner, slot, linears, bf, sp=False):
    """(W, bf16 image of W or None): the weights of `linears` concatenated along the output axis, once, cached on the model under
    (owner, slot) and keyed by the parameters' storage address and version: load_state_dict(), .to() or any in-place write makes a new one.
    sp (fp32 mode under config.frozen_products == "split"): the second item is W's (hi, lo) pair, cached in the same entry"""
    params = tuple(lin.weight for lin in linears)
    hit = _frozen_cached(model, owner, slot, params, lambda: (torch.cat([p.detach() for p in params], 0).contiguous(),))
    return hit.w, hit.image(bf, sp)


class _LlamaCat:
    """the weights of `linears` (q | k | v of an attention, gate | up of an MLP) as ONE weight along the output axis.  An fp32 model: the
    cached concatenation of _llama_cat, one product per call.  A model stored in bf16 (P.stored): nothing is concatenated or cached --
    mm is one product per member into the shared buffer at the member's column offset, and mm_t one layout-1 product per member over
    its columns of g, summed in a fixed order, the members' order (q, then k, then v; gate, then up): (g_q W_q + g_k W_k) + g_v W_v."""

    def __init__(self, P, model, owner, slot, linears):
        self.P, self.linears = P, linears
        self.cat = None if P.stored else _llama_cat(model, owner, slot, linears, P.bf, P.sp)
        self.widths = [int(lin.weight.shape[0]) for lin in linears]

    def mm(self, a32, a16, rows, out, ldc, first=0, count=None):
        """out[:, :n] = a (rows, K) [W_first | .. | W_(first + count - 1)]^T, n the members' widths together"""
        last = len(self.linears) if count is None else first + count
        if self.cat is not None:
            self.P.mm(a32, a16, *self.cat, None, rows, out, ldc, w_row=sum(self.widths[:first]), n_out=sum(self.widths[first:last]))
            return
        c = 0
        for lin, n in zip(self.linears[first:last], self.widths[first:last]):
            self.P.mm(a32, a16, lin.weight, _IN_PLACE, None, rows, out, ldc, c_off=c)
            c += n

    def mm_t(self, g32, g16, rows):
        """g (rows, sum of the widths) [W_0 ; W_1 ; ..] -> (rows, K) fp32"""
        if self.cat is not None:
            return self.P.mm_t(g32, g16, *self.cat, rows)
        o, off, ldg = None, 0, sum(self.widths)
        for lin, n in zip(self.linears, self.widths):
            part = self.P.mm_t(g32, g16, lin.weight, _IN_PLACE, rows, g_off=off, ldg=ldg)
            o = part if o is None else o.add_(part)
            off += n
        return o


def _llama_qkv_cat(model, att, P):
    return _LlamaCat(P, model, att, "qkv", (att.q_proj, att.k_proj, att.v_proj))


def _llama_gu_cat(model, mlp, P):
    return _LlamaCat(P, model, mlp, "gu", (mlp.gate_proj, mlp.up_proj))


def _llama_rows(lib, P):
    """the row kernels that read a parameter, by the model's storage: name -> the entry point (the _p16 one for a stored-bf16 model)"""
    sfx = "_p16" if P.stored else ""
    return {n: getattr(lib, f"immtsf_llama_{n}{sfx}") for n in ("embed_tokens", "embed_rmsnorm", "embed_add_rmsnorm", "embed_pool",
                                                                "body_rmsnorm", "body_rmsnorm_backward")}


def llama_embed_notes(llm_model, ids, cu, precision=None, max_len=None):
    """pooled (N, d) fp32: the mean over each note's tokens of the frozen LlamaModel's last hidden state -- reference fusions/load_llm.py
    embed_notes without the padding (csrc/llama_embed.hip and the GEMM family over the packed rows; 9 launches a layer + 5).  ids (sum L)
    int32: the notes' real tokens back to back; cu (N + 1) int32: prefix sums of the token counts; both on the model's device.  Positions
    are 0 .. L - 1 inside each note, the cos / sin table is built per call from the model's own rotary_emb.inv_freq and
    attention_scaling.  A note of no tokens gives an exact zero row.  max_len: an upper bound of the token counts (read from cu when not
    given: one device -> host copy).  The model's parameters are read in place, but for the cached q | k | v and gate | up concatenations
    and, in bf16 mode, the cached bf16 weight images; runs under no_grad and saves nothing.  A model stored in bf16
    (config.llama_stored_bf16) is read in place altogether: no concatenation, no image, nothing cached (_LlamaCat, _frozen_gemm); the
    result is fp32 all the same.  Outside llama_embed_notes_supported this raises: callers check."""
    def widest(cfg):
        d, H, H_kv, hd, inner = _llama_dims(cfg)
        return max(d, (H + 2 * H_kv) * hd, 2 * inner)

    with torch.no_grad():
        pooled, done, ids, cu, max_len, P = _notes_prologue(
            "llama_embed_notes", llm_model, ids, cu, precision, max_len, llama_embed_notes_supported,
            lambda cfg: int(getattr(cfg, "hidden_size", 0)), widest)
        if done:
            return pooled
        lib, st, precision, bf = P.lib, P.st, P.precision, P.bf
        cfg = llm_model.config
        N, T, dev = pooled.shape[0], ids.numel(), ids.device
        d, H, H_kv, hd, inner = _llama_dims(cfg)
        dq, dqkv = H * hd, (H + 2 * H_kv) * hd
        eps = float(cfg.rms_norm_eps)
        scale = 1.0 / float(hd) ** 0.5
        # one workspace for the whole pass, carved as include/immtsf.h lists it
        carve = _Carver(_bytes(lib.immtsf_llama_embed_workspace_bytes(T, d, H, H_kv, inner, max_len, precision), dev))
        op = torch.bfloat16 if bf else torch.float32
        x, h, qkv, ao, pr, gu, act = (carve(T, d), carve(T, d, op), carve(T, dqkv), carve(T, dq, op), carve(T, d), carve(T, 2 * inner),
                                      carve(T, inner, op))
        cos_t, sin_t, rstd = carve(max_len, 64), carve(max_len, 64), carve(T, 1)
        carve.done()

        rope = llm_model.rotary_emb
        inv_freq = rope.inv_freq.detach().to(device=dev, dtype=torch.float32).contiguous()
        check(lib.immtsf_llama_embed_rope_table(ptr(inv_freq), float(rope.attention_scaling), max_len, ptr(cos_t), ptr(sin_t), st),
              "llama_embed_rope_table")
        emb = llm_model.embed_tokens.weight
        rows = _llama_rows(lib, P)
        check(rows["embed_tokens"](ptr(ids), T, ptr(emb), int(emb.shape[0]), d, ptr(x), st), "llama_embed_tokens")
        for i, layer in enumerate(llm_model.layers):
            att, mlp = layer.self_attn, layer.mlp
            w_in = layer.input_layernorm.weight
            if i == 0:
                check(rows["embed_rmsnorm"](ptr(x), T, d, ptr(w_in), eps, *P.pair(h, h), st), "llama_embed_rmsnorm")
            else:      # the residual add of the layer before rides on this norm
                check(rows["embed_add_rmsnorm"](ptr(x), ptr(pr), T, d, ptr(w_in), eps, *P.pair(h, h), st), "llama_embed_add_rmsnorm")
            _llama_qkv_cat(llm_model, att, P).mm(h, h, T, qkv, dqkv)
            check(lib.immtsf_llama_embed_rope(ptr(qkv), dqkv, ptr(cu), N, T, H, H_kv, max_len, ptr(cos_t), ptr(sin_t), st), "llama_embed_rope")
            check(lib.immtsf_llama_embed_attention(ptr(qkv), dqkv, ptr(cu), N, T, H, H_kv, max_len, scale, precision, *P.pair(ao, ao), st),
                  "llama_embed_attention")
            P.lin(ao, ao, att.o_proj, T, pr)
            check(rows["embed_add_rmsnorm"](ptr(x), ptr(pr), T, d, ptr(layer.post_attention_layernorm.weight), eps, *P.pair(h, h), st),
                  "llama_embed_add_rmsnorm")
            _llama_gu_cat(llm_model, mlp, P).mm(h, h, T, gu, 2 * inner)
            check(lib.immtsf_llama_embed_swiglu(ptr(gu), T, inner, *P.pair(act, act), st), "llama_embed_swiglu")
            P.lin(act, act, mlp.down_proj, T, pr)
        check(rows["embed_pool"](ptr(x), ptr(pr), ptr(cu), N, T, d, ptr(llm_model.norm.weight), eps, ptr(rstd), ptr(pooled), st),
              "llama_embed_pool")
        return pooled


# ------------------------------------------------------------------------------------------------ TimeLLM: the frozen Llama body
def llama_body_supported(llm_model, S_p, S_t):
    """the limits of llama_body: llama_embed_notes_supported's conditions on the model (the LlamaModel class itself, head_dim 128,
    H / H_kv in {1, 2, 4, 8}, silu, no attention or MLP bias, rope_type default / linear / llama3, fp32 parameters or -- with
    config.llama_stored_bf16 on -- all bf16 on one CUDA device, widths multiples of 8), S_p >= 0, S_t >= 1 and
    S = S_p + S_t <= max_position_embeddings, <= 1024"""
    if S_p < 0 or S_t < 1 or not llama_embed_notes_supported(llm_model, 1):
        return False
    cfg = llm_model.config
    d, H, H_kv, _, inner = _llama_dims(cfg)
    return bool(_lib.load().immtsf_llama_body_supported(d, H, H_kv, inner, int(S_p + S_t), int(cfg.max_position_embeddings)))


class LlamaBodyFn(torch.autograd.Function):
    """transformers' LlamaModel(inputs_embeds=cat([prefix, tail], 1)).last_hidden_state[:, -S_t:] on csrc/llama_body.hip, the forward row
    kernels of csrc/llama_embed.hip and the GEMM family.  The body is frozen and only `tail` takes a gradient; there is no
    attention mask, so positions are arange(S), attention is plain causal, no prefix row depends on a tail row and the backward runs
    over the B S_t tail rows alone (exactly).  The last layer computes queries, o_proj and the MLP for the tail rows only.  Saved per
    layer: the roped K and V of all rows and, for the tail rows, the block input, both rstd, the roped q, the attention output, the
    log-sum-exp, the post-attention residual and the gate | up product."""

    @staticmethod
    def forward(ctx, tail, prefix, model, precision, need_bwd):
        lib = _lib.load()
        st = stream_ptr()
        cfg = model.config
        B, S_t, d = tail.shape
        S_p = 0 if prefix is None else prefix.shape[1]
        S, L = S_p + S_t, len(model.layers)
        _, H, H_kv, hd, inner = _llama_dims(cfg)
        dq, dkv = H * hd, H_kv * hd
        dqkv = dq + 2 * dkv
        dev = tail.device
        P = _FrozenProducts(lib, model, precision, st)
        rows_k = _llama_rows(lib, P)
        bf = P.bf
        eps = float(cfg.rms_norm_eps)
        scale = 1.0 / float(hd) ** 0.5
        f32, b16 = _allocators(dev)

        def rms(xin, S_in, s_from, y, w, stats):
            """(row sums xin + y or xin itself, normed operand, rstd) of the rows s_from .. S_in - 1, compact"""
            n = B * (S_in - s_from)
            xo = f32(n, d) if y is not None else None
            h = b16(n, d) if bf else f32(n, d)
            rstd = f32(n) if stats else None
            check(rows_k["body_rmsnorm"](ptr(xin), B, S_in, s_from, d, ptr(y), ptr(xo), ptr(w), eps, *P.pair(h, h), ptr(rstd), st),
                  "llama_body_rmsnorm")
            return (xin if xo is None else xo), h, rstd

        def rope(buf, off, ld, rows, rows_per_b, pos0, heads):
            check(lib.immtsf_llama_body_rope(_adr(buf, off), ld, rows, rows_per_b, pos0, heads, S, ptr(cos_t), ptr(sin_t), 0, None, st),
                  "llama_body_rope")

        tl = lambda t, rows_per_b: _tail_rows(t, B, rows_per_b, S_t)      # noqa: E731

        rot = model.rotary_emb
        inv_freq = rot.inv_freq.detach().to(device=dev, dtype=torch.float32).contiguous()
        cos_t, sin_t = f32(S, 64), f32(S, 64)
        check(lib.immtsf_llama_embed_rope_table(ptr(inv_freq), float(rot.attention_scaling), S, ptr(cos_t), ptr(sin_t), st),
              "llama_embed_rope_table")
        x = tail.view(B * S_t, d) if prefix is None else torch.cat([prefix, tail], 1).view(B * S, d)
        y, Sx = None, S               # y: the MLP output of the layer before, added behind the next norm; Sx: rows per sequence of x
        saved = []
        for li, layer in enumerate(model.layers):
            att, mlp = layer.self_attn, layer.mlp
            qf = S_p if li == L - 1 else 0
            Sq = S - qf
            x, h, rstd1 = rms(x, Sx, 0, y, layer.input_layernorm.weight, need_bwd)
            Wqkv = _llama_qkv_cat(model, att, P)
            if qf == 0:
                qkv = f32(B * S, dqkv)
                Wqkv.mm(h, h, B * S, qkv, dqkv)
                rope(qkv, 0, dqkv, B * S, S, 0, H + H_kv)
                q, ldq, kv, ldkv, k_off = qkv, dqkv, qkv, dqkv, dq
            else:           # the last layer: K and V of all rows, queries of the tail rows
                kv = f32(B * S, 2 * dkv)
                Wqkv.mm(h, h, B * S, kv, 2 * dkv, first=1)
                rope(kv, 0, 2 * dkv, B * S, S, 0, H_kv)
                _, ht, _ = rms(x, S, qf, None, layer.input_layernorm.weight, False)
                q = f32(B * Sq, dq)
                Wqkv.mm(ht, ht, B * Sq, q, dq, count=1)
                rope(q, 0, dq, B * Sq, Sq, qf, H)
                ldq, ldkv, k_off = dq, 2 * dkv, 0
            ao32 = f32(B * Sq, dq) if (need_bwd or not bf) else None
            ao16 = b16(B * Sq, dq) if bf else None
            lse = f32(B * Sq, H) if need_bwd else None
            check(lib.immtsf_llama_body_attention_forward(ptr(q), ldq, _adr(kv, k_off), _adr(kv, k_off + dkv), ldkv, B, S, H, H_kv, qf, scale,
                                                          precision, ptr(ao32), ptr(ao16), ptr(lse), st), "llama_body_attention_forward")
            pr = f32(B * Sq, d)
            P.lin(ao32, ao16, att.o_proj, B * Sq, pr)
            x1, g, rstd2 = rms(x, S, qf, pr, layer.post_attention_layernorm.weight, need_bwd)
            gu = f32(B * Sq, 2 * inner)
            _llama_gu_cat(model, mlp, P).mm(g, g, B * Sq, gu, 2 * inner)
            act = b16(B * Sq, inner) if bf else f32(B * Sq, inner)
            check(lib.immtsf_llama_embed_swiglu(ptr(gu), B * Sq, inner, *P.pair(act, act), st), "llama_embed_swiglu")
            mo = f32(B * Sq, d)
            P.lin(act, act, mlp.down_proj, B * Sq, mo)
            if need_bwd:
                if qf == 0:
                    q_t = tl(qkv[:, :dq], S)
                    kv_all = qkv[:, dq:] if S_p == 0 else qkv[:, dq:].contiguous()      # (with no prefix the tail is the whole buffer)
                    kv_ld = dqkv if S_p == 0 else 2 * dkv
                else:
                    q_t, kv_all, kv_ld = q, kv, 2 * dkv
                saved.append((tl(x, S), tl(rstd1.view(-1, 1), S).view(-1), q_t if q_t.is_contiguous() else q_t.contiguous(), kv_all, kv_ld,
                              tl(ao32, Sq), tl(lse, Sq), tl(x1, Sq), tl(rstd2.view(-1, 1), Sq).view(-1), tl(gu, Sq)))
            x, y, Sx = x1, mo, Sq
        out = f32(B, S_t, d)
        xf = f32(B * S_t, d)
        rstd_f = f32(B * S_t) if need_bwd else None
        check(rows_k["body_rmsnorm"](ptr(x), B, Sx, Sx - S_t, d, ptr(tl(y, Sx)), ptr(xf), ptr(model.norm.weight), eps, ptr(out), None,
                                     ptr(rstd_f), st), "llama_body_rmsnorm")
        if need_bwd:
            ctx.saved, ctx.final = saved, (xf, rstd_f)
            ctx.model, ctx.dims, ctx.precision, ctx.rope = model, (B, S_p, S_t, d, H, H_kv, hd, inner), precision, (cos_t, sin_t)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        st = stream_ptr()
        model = ctx.model
        B, S_p, S_t, d, H, H_kv, hd, inner = ctx.dims
        S, M = S_p + S_t, B * S_t
        dq, dkv = H * hd, H_kv * hd
        dqkv = dq + 2 * dkv
        P = _FrozenProducts(lib, model, ctx.precision, st)
        rms_backward = _llama_rows(lib, P)["body_rmsnorm_backward"]
        bf = P.bf
        scale = 1.0 / float(hd) ** 0.5
        cos_t, sin_t = ctx.rope
        f32, b16 = _allocators(dout.device, bf)

        def rms_bwd(g, x, rstd, w, resid):
            o, o16 = f32(M, d), b16(M, d)
            check(rms_backward(ptr(g), ptr(x), ptr(rstd), ptr(w), ptr(resid), M, d, ptr(o), ptr(o16), st),
                  "llama_body_rmsnorm_backward")
            return o, o16

        xf, rstd_f = ctx.final
        dx, dx16 = rms_bwd(dout.contiguous().view(M, d), xf, rstd_f, model.norm.weight, None)
        for li in reversed(range(len(model.layers))):
            layer = model.layers[li]
            att, mlp = layer.self_attn, layer.mlp
            x_t, rstd1, q_t, kv, kv_ld, ao_t, lse_t, x1_t, rstd2, gu_t = ctx.saved[li]
            dact = P.lin_t(dx, dx16, mlp.down_proj, M)
            dgu, dgu16 = (None, b16(M, 2 * inner)) if bf else (f32(M, 2 * inner), None)
            check(lib.immtsf_llama_body_swiglu_backward(ptr(gu_t), ptr(dact), M, inner, ptr(dgu), ptr(dgu16), st),
                  "llama_body_swiglu_backward")
            dg = _llama_gu_cat(model, mlp, P).mm_t(dgu, dgu16, M)
            dx1, dx1_16 = rms_bwd(dg, x1_t, rstd2, layer.post_attention_layernorm.weight, dx)
            dao = P.lin_t(dx1, dx1_16, att.o_proj, M)
            dbuf, dbuf16 = f32(M, dqkv), b16(M, dqkv)
            kp = C.c_void_p(kv.data_ptr())            # (a view into the q | k | v buffer starts at its K columns)
            check(lib.immtsf_llama_body_attention_backward(ptr(q_t), dq, kp, C.c_void_p(kv.data_ptr() + 4 * dkv), kv_ld, ptr(dao), ptr(ao_t),
                                                           ptr(lse_t), B, S, H, H_kv, S_p, scale, ptr(dbuf), _adr(dbuf, dq),
                                                           _adr(dbuf, dq + dkv), dqkv, st), "llama_body_attention_backward")
            check(lib.immtsf_llama_body_rope(ptr(dbuf), dqkv, M, S_t, S_p, H + H_kv, S, ptr(cos_t), ptr(sin_t), 1, ptr(dbuf16), st),
                  "llama_body_rope (backward)")
            dh = _llama_qkv_cat(model, att, P).mm_t(dbuf, dbuf16, M)
            dx, dx16 = rms_bwd(dh, x_t, rstd1, layer.input_layernorm.weight, dx1)
        return dx.view(B, S_t, d), None, None, None, None


def llama_body(llm_model, prefix_embeds, tail_embeds, training, precision=None):
    """hidden_tail (B, S_t, d) = the final norm's output for the last S_t rows of the frozen Llama body over [prefix_embeds | tail_embeds].
    Only tail_embeds takes a gradient (prefix_embeds may require one; it gets none).  Llama's only dropout is attention_dropout:
    `training` with config.attention_dropout > 0 is not supported (callers take the stock path).  The model's parameters are read in
    place, but for the cached q | k | v and gate | up concatenations and, in bf16 mode, the cached bf16 weight images (shared with
    llama_embed_notes).  A model stored in bf16 (config.llama_stored_bf16) is read in place altogether, as llama_embed_notes says; inputs,
    result, gradient and saved tensors stay fp32, and a data gradient through q | k | v (gate | up) is its members' layout-1 products
    summed in the order q, k, v (gate, up).  Outside llama_body_supported this raises: callers check."""
    tail, prefix, need_bwd = _body_inputs("llama_body", llm_model, prefix_embeds, tail_embeds, llama_body_supported)
    if training and float(getattr(llm_model.config, "attention_dropout", 0.0) or 0.0) > 0.0:
        raise _lib.ImmtsfError("llama_body: attention dropout in training mode is not supported (take the stock path)")
    return LlamaBodyFn.apply(tail, prefix, llm_model, config.precision_code(precision), need_bwd)


# ------------------------------------------------------------------------------------------------ TimeLLM's frozen BERT body
BERT_SITE_EMBD = 131072          # include/immtsf.h IMMTSF_SITE_BERT_*


def bert_sites(layer):
    """(attention probabilities, attention-output dropout, feed-forward-output dropout) sites of layer `layer`; the embedding dropout is
    BERT_SITE_EMBD"""
    return 131073 + 3 * layer, 131074 + 3 * layer, 131075 + 3 * layer


def bert_body_supported(llm_model, S_p, S_t):
    """the limits of bert_body: bert_embed_notes_supported's conditions on the model (the BertModel class itself, head_dim 64, hidden_act
    "gelu", absolute positions, neither a decoder nor cross attention, fp32 parameters, hidden_size and intermediate_size multiples of 8,
    at least one layer), S_p >= 0, S_t >= 1 and S = S_p + S_t <= max_position_embeddings, <= 1024"""
    if S_p < 0 or S_t < 1 or not bert_embed_notes_supported(llm_model, 1):
        return False
    cfg = llm_model.config
    return bool(_lib.load().immtsf_bert_body_supported(int(cfg.hidden_size), int(cfg.num_attention_heads), int(S_p + S_t),
                                                       int(cfg.max_position_embeddings)))


class BertBodyFn(torch.autograd.Function):
    """transformers' BertModel(inputs_embeds=cat([prefix, tail], 1)).last_hidden_state[:, -S_t:] on csrc/bert_body.hip, the erf GELU of
    csrc/bert_embed.hip and the GEMM family.  The body is frozen and only `tail` takes a gradient.  BERT is bidirectional and
    there is no attention mask: every row of every layer depends on every tail row, so a middle layer runs forward and backward over all
    B S rows.  Two exact reductions.  Last layer, forward: only the tail rows leave the body, so K and V are computed for all rows but the
    queries, the output dense, both add + LayerNorms and the feed-forward for the S_t tail rows only.  First layer, backward: the embedding
    LayerNorm is row-wise and the prefix takes no gradient, so layer 0's dq and the dqkv -> dx0 product run over the tail rows only (its
    dk / dv of the tail keys still sum over all of the layer's queries).  With one layer both hold in the same layer.  Saved per layer,
    for the layer's rows: the q | k | v product (all rows), the attention output, the log-sum-exp, both pre-norm sums with their
    statistics and the feed-forward pre-activation; for the embedding, the tail rows' pre-norm sum and statistics."""

    @staticmethod
    def forward(ctx, tail, prefix, model, p_drops, precision, seed, need_bwd):
        lib = _lib.load()
        st = stream_ptr()
        cfg = model.config
        B, S_t, d = tail.shape
        S_p = 0 if prefix is None else prefix.shape[1]
        S, H, inner, L = S_p + S_t, int(cfg.num_attention_heads), int(cfg.intermediate_size), len(model.encoder.layer)
        M = B * S_t
        P = _FrozenProducts(lib, model, precision, st)
        bf, mm, lin = P.bf, P.mm, P.lin
        p_h, p_a = p_drops
        eps = float(cfg.layer_norm_eps)
        scale = 1.0 / float(d // H) ** 0.5
        f32, b16 = _allocators(tail.device, bf)

        def add_ln(xin, S_in, s_from, y, q_from, norm, site, out32, keep16):
            """LayerNorm(xin rows + dropout(y)) -> (out32, bf16 image or None, pre-norm sum, mean, rstd)"""
            n = B * (S_in - s_from)
            o16 = b16(n, d) if keep16 else None
            sm, mean, rstd = (f32(n, d), f32(n), f32(n)) if need_bwd else (None, None, None)
            check(lib.immtsf_bert_body_add_layernorm(ptr(xin), B, S_in, s_from, ptr(y), S, q_from, d, ptr(norm.weight), ptr(norm.bias), eps, p_h,
                                                     seed, site, ptr(out32), ptr(o16), ptr(sm), ptr(mean), ptr(rstd), st),
                  "bert_body_add_layernorm")
            return o16, sm, mean, rstd

        def tl(t):        # the tail rows of a (B S, ...) tensor, compact
            if t is None or S_p == 0:
                return t
            return t.view(B, S, -1)[:, S_p:].contiguous().view(M, -1)

        emb = model.embeddings
        x, x16 = f32(B * S, d), b16(B * S, d)
        sum0, mean0, rstd0 = (f32(M, d), f32(M), f32(M)) if need_bwd else (None, None, None)
        check(lib.immtsf_bert_body_embed(ptr(prefix), ptr(tail), ptr(emb.position_embeddings.weight), ptr(emb.token_type_embeddings.weight), B,
                                         S_p, S_t, d, ptr(emb.LayerNorm.weight), ptr(emb.LayerNorm.bias), eps, p_h, seed, BERT_SITE_EMBD, ptr(x),
                                         ptr(x16), ptr(sum0), ptr(mean0), ptr(rstd0), st), "bert_body_embed")
        out = f32(B, S_t, d)
        saved = []
        for li, layer in enumerate(model.encoder.layer):
            last = li == L - 1
            qf = S_p if last else 0
            Sq = S - qf
            Mq = B * Sq
            s_attn, s_h1, s_h2 = bert_sites(li)
            att = layer.attention
            W, bias, W16 = _bert_qkv(model, att.self, bf, P.sp)
            qkv = f32(B * S, 3 * d)
            if qf == 0:
                mm(x, x16, W, W16, bias, B * S, qkv, 3 * d)
                q, ldq = qkv, 3 * d
            else:           # the last layer: K and V of all rows, queries of the tail rows
                mm(x, x16, W, W16, bias, B * S, qkv, 3 * d, w_row=d, n_out=2 * d, c_off=d)
                q, ldq = f32(Mq, d), d
                mm(None if bf else tl(x), tl(x16), W, W16, bias, Mq, q, d, n_out=d)
            ao32 = f32(Mq, d) if (need_bwd or not bf) else None
            ao16 = b16(Mq, d)
            lse = f32(B, H, Sq) if need_bwd else None
            check(lib.immtsf_bert_body_attention_forward(ptr(q), ldq, _adr(qkv, d), _adr(qkv, 2 * d), 3 * d, B, S, H, qf, scale, precision, p_a,
                                                         seed, s_attn, ptr(ao32), ptr(ao16), ptr(lse), st), "bert_body_attention_forward")
            pr = f32(Mq, d)
            lin(ao32, ao16, att.output.dense, Mq, pr)
            x1 = f32(Mq, d)
            x1_16, sum1, mean1, rstd1 = add_ln(x, S, qf, pr, qf, att.output.LayerNorm, s_h1, x1, bf)
            pre = f32(Mq, inner)
            lin(x1, x1_16, layer.intermediate.dense, Mq, pre)
            a32, a16 = (None, b16(Mq, inner)) if bf else (f32(Mq, inner), None)
            check(lib.immtsf_bert_embed_gelu(ptr(pre), pre.numel(), ptr(a32), ptr(a16), st), "bert_embed_gelu")
            mo = f32(Mq, d)
            lin(a32, a16, layer.output.dense, Mq, mo)
            x2 = out.view(M, d) if last else f32(Mq, d)
            x2_16, sum2, mean2, rstd2 = add_ln(x1, Sq, 0, mo, qf, layer.output.LayerNorm, s_h2, x2, bf and not last)
            if need_bwd:
                saved.append((q, ldq, qkv, ao32, lse, sum1, mean1, rstd1, pre, sum2, mean2, rstd2))
            x, x16 = x2, x2_16
        if need_bwd:
            ctx.saved, ctx.embed = saved, (sum0, mean0, rstd0)
            ctx.model, ctx.dims, ctx.drops, ctx.seed, ctx.precision = model, (B, S_p, S_t, d, H, inner), p_drops, seed, precision
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        st = stream_ptr()
        model, prec, seed = ctx.model, ctx.precision, ctx.seed
        B, S_p, S_t, d, H, inner = ctx.dims
        S, M, L = S_p + S_t, B * S_t, len(model.encoder.layer)
        p_h, p_a = ctx.drops
        P = _FrozenProducts(lib, model, prec, st)
        bf, mm_t, lin_t = P.bf, P.mm_t, P.lin_t
        scale = 1.0 / float(d // H) ** 0.5
        f32, b16 = _allocators(dout.device, bf)

        def ln_bwd(dy, Sn, sm, mean, rstd, norm, q_from, site):
            """dy = (dy_a, Sa, sa_from, dy_b, tb_from) -> (d_sum fp32, the branch's gradient as the next product reads it: fp32, bf16)"""
            dy_a, Sa, sa_from, dy_b, tb_from = dy
            n = B * Sn
            dsum = f32(n, d)
            br32 = f32(n, d) if (not bf and p_h > 0.0) else None
            br16 = b16(n, d)
            check(lib.immtsf_bert_body_layernorm_backward(ptr(dy_a), B, Sa, sa_from, Sn, ptr(dy_b), tb_from, ptr(sm), ptr(mean), ptr(rstd),
                                                          ptr(norm.weight), d, S, q_from, p_h, seed, site, 0, ptr(dsum), ptr(br32), ptr(br16),
                                                          st), "bert_body_layernorm_backward")
            return dsum, (None if bf else (dsum if br32 is None else br32)), br16

        dy = (dout.contiguous().view(M, d), S_t, 0, None, 0)
        for li in reversed(range(L)):
            layer = model.encoder.layer[li]
            att = layer.attention
            first, last = li == 0, li == L - 1
            qf = S_p if last else 0
            Sq = S - qf
            Mq = B * Sq
            q, ldq, qkv, ao32, lse, sum1, mean1, rstd1, pre, sum2, mean2, rstd2 = ctx.saved[li]
            s_attn, s_h1, s_h2 = bert_sites(li)
            dsum2, dmo32, dmo16 = ln_bwd(dy, Sq, sum2, mean2, rstd2, layer.output.LayerNorm, qf, s_h2)
            dact = lin_t(dmo32, dmo16, layer.output.dense, Mq)
            dpre32, dpre16 = (None, b16(Mq, inner)) if bf else (f32(Mq, inner), None)
            check(lib.immtsf_bert_body_gelu_backward(ptr(pre), ptr(dact), dact.numel(), ptr(dpre32), ptr(dpre16), st), "bert_body_gelu_backward")
            g1 = lin_t(dpre32, dpre16, layer.intermediate.dense, Mq)
            dsum1, dpr32, dpr16 = ln_bwd((dsum2, Sq, 0, g1, 0), Sq, sum1, mean1, rstd1, att.output.LayerNorm, qf, s_h1)
            dao = lin_t(dpr32, dpr16, att.output.dense, Mq)
            # dq for the queries whose rows take a gradient through q, dk / dv for the keys whose rows do, each summed over all Sq queries
            dq_from = S_p if (first or last) else 0
            k_from = S_p if first else 0
            if first:           # the dqkv -> dx0 product over the tail rows only
                rows_b, dq_off = S_t, 0
            else:
                rows_b, dq_off = S, dq_from * 3 * d
            dqkv = f32(B * rows_b, 3 * d)
            if dq_off:          # the last layer of several: the prefix rows have keys and values but no query
                dqkv.view(B, S, 3 * d)[:, :S_p, :d].zero_()
            dsum = f32(Mq, H) if bf else None
            check(lib.immtsf_bert_body_attention_backward(ptr(q), ldq, _adr(qkv, d), _adr(qkv, 2 * d), 3 * d, ptr(dao), ptr(ao32), ptr(lse), B, S, H,
                                                          qf, dq_from, k_from, scale, prec, p_a, seed, s_attn, _adr(dqkv, dq_off), rows_b,
                                                          _adr(dqkv, d), _adr(dqkv, 2 * d), rows_b, 3 * d, ptr(dsum), st),
                  "bert_body_attention_backward")
            dqkv16 = b16(B * rows_b, 3 * d)
            if bf:
                check(lib.immtsf_f32_to_bf16(ptr(dqkv), ptr(dqkv16), dqkv.numel(), st), "f32_to_bf16")
            W, _, W16 = _bert_qkv(model, att.self, bf, P.sp)
            gq = mm_t(dqkv, dqkv16, W, W16, B * rows_b)
            if first:
                dy = (dsum1, Sq, S_p - qf, gq, 0)
            elif last:
                dy = (gq, S, 0, dsum1, S_p)
            else:
                dy = (dsum1, S, 0, gq, 0)
        sum0, mean0, rstd0 = ctx.embed
        dy_a, Sa, sa_from, dy_b, tb_from = dy
        dtail = f32(M, d)
        norm = model.embeddings.LayerNorm
        check(lib.immtsf_bert_body_layernorm_backward(ptr(dy_a), B, Sa, sa_from, S_t, ptr(dy_b), tb_from, ptr(sum0), ptr(mean0), ptr(rstd0),
                                                      ptr(norm.weight), d, S, S_p, p_h, seed, BERT_SITE_EMBD, 1, ptr(dtail), None, None, st),
              "bert_body_layernorm_backward (embedding)")
        return dtail.view(B, S_t, d), None, None, None, None, None, None


def bert_body(llm_model, prefix_embeds, tail_embeds, training, precision=None, seed=None):
    """hidden_tail (B, S_t, d) fp32 = the last S_t rows of the frozen BertModel's last hidden state over [prefix_embeds | tail_embeds]
    (token type 0, absolute positions, no attention mask: the padded prompt tokens are attended, as the reference calls the model).  Only
    tail_embeds takes a gradient (prefix_embeds may require one; it gets none); under no_grad, or with a tail that needs no gradient,
    nothing is saved.  Two exact reductions: the last layer computes K and V for all rows but queries, the output dense, both add +
    LayerNorms and the feed-forward for the tail rows only; the backward of the first layer computes dq and the dqkv -> dx0 product for
    the tail rows only (the embedding LayerNorm is row-wise and the prefix takes no gradient).  Every other layer runs over all B S rows
    in both directions: attention is bidirectional.  training: the body's four dropouts (embedding, attention probabilities and the two
    hidden dropouts of each layer; hidden_dropout_prob / attention_probs_dropout_prob of its config) are drawn from immtsf's generator --
    ops.dropout_keep_mask(seed, site, ...) reproduces them (BERT_SITE_EMBD, bert_sites(layer)); seed: the Philox key, config.next_seed()
    by default.  The model's parameters are read in place, but for the cached query | key | value concatenation and, in bf16 mode, the
    cached bf16 weight images (shared with bert_embed_notes).  Outside bert_body_supported this raises: callers check."""
    tail, prefix, need_bwd = _body_inputs("bert_body", llm_model, prefix_embeds, tail_embeds, bert_body_supported)
    if tail.dim() != 3 or tail.shape[2] != llm_model.config.hidden_size or \
            (prefix is not None and (prefix.shape[0] != tail.shape[0] or prefix.shape[2] != tail.shape[2])):
        raise _lib.ImmtsfError("bert_body: prefix (B, S_p, d) and tail (B, S_t, d) with d the body's hidden_size")
    cfg = llm_model.config
    drops, seed = _body_drops((cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob), training, seed)
    return BertBodyFn.apply(tail, prefix, llm_model, drops, config.precision_code(precision), seed, need_bwd)


# ---- TimeLLM's prompt statistics (csrc/timellm_prompt.hip) -------------------------------------------------------------------------------
def timellm_prompt_supported(L, C, top_k):
    """the limits of the prompt-statistics kernel (immtsf_timellm_prompt_supported): 1 <= L <= 2048, 1 <= C <= 64, 1 <= top_k <= 64 and the
    (L, C) tile within 64 KB of LDS (L C <= 16384)"""
    return bool(_lib.load().immtsf_timellm_prompt_supported(int(L), int(C), int(top_k)))


def timellm_prompt_split(packed, C):
    """the (B, 3 C + 1) float32 and (B, top_k) int32 views of a packed (B, 3 C + 1 + top_k) buffer, on whichever device it lies"""
    n = 3 * int(C) + 1
    return packed[:, :n], packed[:, n:].view(torch.int32)


def timellm_prompt_packed(x, top_k):
    """one launch for the batch: x (B, L, C) -> the packed (B, 3 C + 1 + top_k) buffer of four-byte words timellm_prompt_split reads
    (a float32 tensor whose last top_k columns hold int32 bits), so that ONE copy brings every statistic to the host.  No autograd (the
    prompt carries no gradient), no host sync.  Outside timellm_prompt_supported this raises: callers check."""
    if x.dim() != 3:
        raise _lib.ImmtsfError(f"timellm_prompt_stats: x (B, L, C), got {tuple(x.shape)}")
    x = _c(x.detach().float())
    _need_gpu(x)
    B, L, Cc = x.shape
    top_k = int(top_k)
    if L < 1 or Cc < 1 or top_k < 1 or not timellm_prompt_supported(L, Cc, top_k):
        raise _lib.ImmtsfError(f"timellm_prompt_stats: L {L}, C {Cc}, top_k {top_k} is outside timellm_prompt_supported")
    packed = torch.empty(B, 3 * Cc + 1 + top_k, dtype=torch.float32, device=x.device)
    check(_lib.load().immtsf_timellm_prompt_stats(ptr(x), B, L, Cc, top_k, ptr(packed), stream_ptr()), "timellm_prompt_stats")
    return packed


def timellm_prompt_stats(x, top_k):
    """TimeLLM's five prompt statistics of x (B, L, C) in one launch: (stats, lags), a (B, 3 C + 1) float32 view -- min, max and lower
    median per channel, then the trend value x.diff(1).sum(1).mean(1), whose sign the prompt spells -- and a (B, top_k) int32 view -- the
    lags of the min(top_k, L) largest circular autocorrelations, descending, ties to the lower lag, padded with the last -- of ONE device
    buffer (timellm_prompt_packed's).  Semantics: include/immtsf.h."""
    return timellm_prompt_split(timellm_prompt_packed(x, top_k), x.shape[2])


# ---- TimeLLM's word prototypes in folded form (csrc/timellm_reprogram.hip) -----------------------------------------------------------------
def timellm_prototypes_supported(E, W_map, Wk, Wv):
    """the limits of the folded prototype operator: fp32 contiguous tensors on the GPU, E (V, d_llm) WITHOUT a gradient (the operator
    returns none for it), W_map (S, V), Wk / Wv (D, d_llm) with 2 D <= 128 a multiple of 16 and d_llm a multiple of 8; any S, V >= 1"""
    ts = (E, W_map, Wk, Wv)
    if any(t is None or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() for t in ts):
        return False
    if E.requires_grad or Wk.shape != Wv.shape or W_map.shape[1] != E.shape[0] or Wk.shape[1] != E.shape[1]:
        return False
    return bool(_lib.load().immtsf_timellm_prototypes_supported(W_map.shape[0], E.shape[0], E.shape[1], Wk.shape[0]))


def timellm_prototypes_pays(S, d_llm, D):
    """the fold's flop count 2 D2 V (d_llm + S) against the as-written 2 S V d_llm (+ the two projections): it wins when
    S d_llm > D2 (d_llm + S), D2 = 2 D"""
    return S * d_llm > 2 * D * (d_llm + S)


class TimeLLMPrototypesFn(torch.autograd.Function):
    """(k, v) = key / value projection of mapping_layer(E^T)^T without the (S, d_llm) table: P = E [Wk^T | Wv^T], [k|v] = W_map P +
    b_map (x) r + [bk|bv] (immtsf_timellm_prototypes_forward, 3 launches); backward 3 launches, W_map read once (include/immtsf.h).
    Saved: P (V, 2 D) and r (2 D); nothing is kept across calls."""

    @staticmethod
    def forward(ctx, E, W_map, b_map, Wk, bk, Wv, bv, precision, cache_on):
        lib = _lib.load()
        S, V = W_map.shape
        D, d = Wk.shape
        dev = W_map.device
        bf = precision == 1
        E16 = _gpt2_w16(cache_on, E) if bf else None
        P = torch.empty(V, 2 * D, dtype=torch.float32, device=dev)
        r = torch.empty(2 * D, dtype=torch.float32, device=dev)
        kv = torch.empty(2, S, D, dtype=torch.float32, device=dev)
        nb = int(lib.immtsf_timellm_prototypes_scratch_bytes(S, V, d, D, 0))
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        check(lib.immtsf_timellm_prototypes_forward(precision, ptr(E), ptr(E16), ptr(W_map), ptr(b_map), ptr(Wk), ptr(bk), ptr(Wv), ptr(bv),
                                                    S, V, d, D, ptr(P), ptr(r), ptr(kv[0]), ptr(kv[1]), ptr(scratch), nb, stream_ptr()),
              "timellm_prototypes_forward")
        ctx.save_for_backward(E, W_map, b_map, P, r)
        ctx.E16, ctx.precision, ctx.dims = E16, precision, (S, V, d, D)
        params = (W_map, b_map, Wk, bk, Wv, bv)
        ctx.sinks = _sinks_of(params)
        ctx.pre = all(s is not None and getattr(p, "_immtsf_grad_prezeroed", False) for p, s in zip(params, ctx.sinks))
        return kv[0], kv[1]

    @staticmethod
    def backward(ctx, dk, dv):
        lib = _lib.load()
        E, W_map, b_map, P, r = ctx.saved_tensors
        S, V, d, D = ctx.dims
        dev = W_map.device
        dk = torch.zeros(S, D, dtype=torch.float32, device=dev) if dk is None else dk.contiguous()
        dv = torch.zeros(S, D, dtype=torch.float32, device=dev) if dv is None else dv.contiguous()
        dk, dv = (g.clone() if g.data_ptr() % 16 else g for g in (dk, dv))      # (a view at an odd offset of a larger gradient buffer)
        if ctx.pre:      # gradient sinks that their owner zero-fills every step: every word is written once, nothing returned
            dW_map, db_map, dWk, dbk, dWv, dbv = ctx.sinks
            ret = (None,) * 6
        else:
            dW_map = torch.empty(S, V, dtype=torch.float32, device=dev)
            up8 = lambda n: (n + 7) // 8 * 8      # noqa: E731
            flat = torch.empty(up8(S) + 2 * (up8(D * d) + up8(D)), dtype=torch.float32, device=dev)
            off, small = 0, []
            for n, shape in ((S, (S,)), (D * d, (D, d)), (D, (D,)), (D * d, (D, d)), (D, (D,))):
                small.append(flat[off:off + n].view(shape))
                off += up8(n)
            db_map, dWk, dbk, dWv, dbv = small
            ret = (dW_map, db_map, dWk, dbk, dWv, dbv)
            del small
        nb = int(lib.immtsf_timellm_prototypes_scratch_bytes(S, V, d, D, 1))
        scratch = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        check(lib.immtsf_timellm_prototypes_backward(ctx.precision, ptr(E), ptr(ctx.E16), ptr(W_map), ptr(b_map), ptr(P), ptr(r), ptr(dk),
                                                     ptr(dv), S, V, d, D, ptr(dW_map), ptr(db_map), ptr(dWk), ptr(dbk), ptr(dWv), ptr(dbv),
                                                     ptr(scratch), nb, stream_ptr()), "timellm_prototypes_backward")
        need = ctx.needs_input_grad
        return (None,) + tuple(g if need[1 + i] else None for i, g in enumerate(ret)) + (None, None)


def timellm_prototypes(E, W_map, b_map, Wk, bk, Wv, bv, precision=None, cache_on=None):
    """TimeLLM's word prototypes, the keys and values of its reprogramming layer, in folded form: (k, v), each (S, D) fp32, equal to
    key_projection(src), value_projection(src) with src = mapping_layer(E^T)^T -- computed as W_map (E [Wk^T | Wv^T]) + ..., so the
    (S, d_llm) table src is never formed and W_map is read once per direction.  Gradients for the six parameters, none for the frozen E.
    In bf16 mode E is read through a bf16 image cached on `cache_on` (the model whose frozen weights the GPT-2 body caches; default: on
    E itself), keyed by E's address and version.  Outside timellm_prototypes_supported this raises: callers check."""
    if not timellm_prototypes_supported(E, W_map, Wk, Wv):
        raise _lib.ImmtsfError("timellm_prototypes: outside timellm_prototypes_supported")
    S, D = W_map.shape[0], Wk.shape[0]
    b_map, bk, bv = _c(b_map), _c(bk), _c(bv)
    _need_gpu(b_map, bk, bv)
    if tuple(b_map.shape) != (S,) or tuple(bk.shape) != (D,) or tuple(bv.shape) != (D,):
        raise _lib.ImmtsfError("timellm_prototypes: b_map (S), bk, bv (D)")
    return TimeLLMPrototypesFn.apply(E, W_map, b_map, Wk, bk, Wv, bv, config.precision_code(precision), E if cache_on is None else cache_on)


# ------------------------------------------------------------------------------------------------ LatentODE backbone
def _latent_ode_dims(B, L, Lp, C, rec_dims, units, gru_units, latents):
    return _lib.LatentODEDims(int(B), int(L), int(Lp), int(C), int(rec_dims), int(units), int(gru_units), int(latents))


def latent_ode_supported(B, L, Lp, C, rec_dims, units, gru_units, latents, call=False):
    """the limits of the fused LatentODE kernels (immtsf_latent_ode_supported: rec_dims, latents <= 64, units, gru_units <= 128, C <= 64,
    L, Lp <= 2^20, the weights and a tile's state within 160 KB of LDS), from the dims alone; call: also what a compute call needs
    (B >= 1 and the saved state's index range, immtsf_latent_ode_workspace_bytes > 0)"""
    lib = _lib.load()
    return _dims_supported(lib.immtsf_latent_ode_supported, lib.immtsf_latent_ode_workspace_bytes,
                           _latent_ode_dims(B, L, Lp, C, rec_dims, units, gru_units, latents), call)


class LatentODEFn(torch.autograd.Function):
    """LatentODE's forecasting() (ODE-RNN encoder over the observed points, transform_z0, z0 = mu + eps |sigma|, the generative ODE over
    the forecast times, the decoder) as ONE launch; backward = TWO (immtsf_latent_ode_forward / _backward, csrc/latent_ode.hip).  The
    flat parameter buffer is the only input with a gradient.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, data, mask, steps, step_len, tpp, flat, eps, widths):
        lib = _lib.load()
        data, mask, steps, step_len, tpp, flat, eps = (_c(t) for t in (data, mask, steps, step_len, tpp, flat, eps))
        _need_gpu(data, mask, steps, step_len, tpp, flat, eps)
        B, L, Cc = data.shape
        Lp = tpp.shape[0]
        R, U, G, Z = widths
        d = _latent_ode_dims(B, L, Lp, Cc, R, U, G, Z)
        out = torch.empty(B, Lp, Cc, dtype=torch.float32, device=data.device)
        states = torch.empty(B, L + 1, 2 * R, dtype=torch.float32, device=data.device)
        traj = torch.empty(B, Lp, Z, dtype=torch.float32, device=data.device)
        check(lib.immtsf_latent_ode_forward(C.byref(d), ptr(data), ptr(mask), ptr(steps), ptr(step_len), ptr(tpp), ptr(flat), ptr(eps),
                                            ptr(out), ptr(states), ptr(traj), stream_ptr()), "latent_ode_forward")
        ctx.dims = (B, L, Lp, Cc, R, U, G, Z)
        ctx.save_for_backward(data, mask, steps, step_len, tpp, flat, eps, states, traj)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        data, mask, steps, step_len, tpp, flat, eps, states, traj = ctx.saved_tensors
        d = _latent_ode_dims(*ctx.dims)
        grads = torch.empty_like(flat)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_latent_ode_workspace_bytes(C.byref(d)), data.device)
        check(lib.immtsf_latent_ode_backward(C.byref(d), ptr(data), ptr(mask), ptr(steps), ptr(step_len), ptr(tpp), ptr(flat), ptr(eps),
                                             ptr(states), ptr(traj), ptr(dout.contiguous()), ptr(grads), ptr(ws), ws.numel(), stream_ptr()),
              "latent_ode_backward")
        return None, None, None, None, None, grads, None, None


def latent_ode(data, mask, steps, step_len, tp_pred, flat_params, eps, widths):
    """data, mask (B, L, C); steps (L) int32 / step_len (L): the step plan of the shared time axis (-1: Euler, n >= 1: n RK4 steps, 0:
    none); tp_pred (Lp); flat_params: every parameter in state_dict order, flattened; eps (B, latents); widths = (rec_dims, units,
    gru_units, latents) -> the forecast (B, Lp, C).  Gradients reach flat_params only."""
    B, L, Cc = data.shape
    Lp = tp_pred.shape[0]
    R, U, G, Z = (int(w) for w in widths)
    if not latent_ode_supported(B, L, Lp, Cc, R, U, G, Z, call=True):
        raise _lib.ImmtsfError(f"latent_ode: shapes outside the fused kernel (B {B}, L {L}, Lp {Lp}, C {Cc}, widths {(R, U, G, Z)})")
    d = _latent_ode_dims(B, L, Lp, Cc, R, U, G, Z)
    nv = int(_lib.load().immtsf_latent_ode_param_count(C.byref(d)))
    if tuple(mask.shape) != (B, L, Cc) or tuple(steps.shape) != (L,) or tuple(step_len.shape) != (L,) or tp_pred.dim() != 1 or \
            tuple(eps.shape) != (B, Z) or flat_params.numel() != nv or steps.dtype != torch.int32 or \
            any(q.dtype != torch.float32 for q in (data, mask, step_len, tp_pred, flat_params, eps)):
        raise _lib.ImmtsfError("latent_ode: the tensors are not the fp32 tensors of these dimensions")
    return LatentODEFn.apply(data, mask, steps, step_len, tp_pred, flat_params, eps, (R, U, G, Z))


# ------------------------------------------------------------------------------------------------ NeuralFlow backbone
def _neural_flow_dims(B, L, Lp, C, rec_dims, latents, hidden_dim, hidden_layers, flow_layers):
    return _lib.NeuralFlowDims(int(B), int(L), int(Lp), int(C), int(rec_dims), int(latents), int(hidden_dim), int(hidden_layers),
                               int(flow_layers))


NEURAL_FLOW_TIME_NETS = {"TimeLinear": 0, "TimeTanh": 1}      # IMMTSF_NF_TIME_LINEAR / IMMTSF_NF_TIME_TANH
neural_flow_launches = {name: 0 for name in NEURAL_FLOW_TIME_NETS}      # forward calls per kernel instance (tests assert which one ran)


def _neural_flow_kind(time_net):
    """the library's number of a time net; -1 (which the library refuses) for a name it has no instance of"""
    return NEURAL_FLOW_TIME_NETS.get(time_net, -1)


def neural_flow_supported(B, L, Lp, C, rec_dims, latents, hidden_dim, hidden_layers, flow_layers, call=False, time_net="TimeLinear"):
    """the limits of the fused NeuralFlow kernels (immtsf_neural_flow_tn_supported: time_net TimeLinear or TimeTanh, rec_dims, latents <= 64,
    hidden_dim <= 128, hidden_layers, flow_layers <= 4, C <= 64, L, Lp <= 2^20, W_hh, the flow's nets and a tile's state within 160 KB of
    LDS), from the dims alone; call: also what a compute call needs (B >= 1 and the saved state's index range,
    immtsf_neural_flow_tn_workspace_bytes > 0)"""
    lib = _lib.load()
    kind = _neural_flow_kind(time_net)
    return _dims_supported(lambda d: lib.immtsf_neural_flow_tn_supported(d, kind), lambda d: lib.immtsf_neural_flow_tn_workspace_bytes(d, kind),
                           _neural_flow_dims(B, L, Lp, C, rec_dims, latents, hidden_dim, hidden_layers, flow_layers), call)


class NeuralFlowFn(torch.autograd.Function):
    """NeuralFlow's forecasting() (the encoder's reversed walk of coupling-flow step + LSTM cell, transform_z0, z0 = mu + eps sigma, the
    coupling flow at every forecast time, the decoder) as TWO launches; backward = THREE (immtsf_neural_flow_tn_forward / _tn_backward,
    csrc/neural_flow.hip), on the kernel instance of `time_net` (kept on the node as .time_net).  The flat parameter buffer is the only
    input with a gradient.  fp32 in either precision mode."""

    @staticmethod
    def forward(ctx, data, mask, tp, tpp, flat, eps, widths, time_net="TimeLinear"):
        lib = _lib.load()
        data, mask, tp, tpp, flat, eps = (_c(t) for t in (data, mask, tp, tpp, flat, eps))
        _need_gpu(data, mask, tp, tpp, flat, eps)
        B, L, Cc = data.shape
        Lp = tpp.shape[1]
        R, Z = widths[0], widths[1]
        d = _neural_flow_dims(B, L, Lp, Cc, *widths)
        out = torch.empty(B, Lp, Cc, dtype=torch.float32, device=data.device)
        xg = torch.empty(B, L, 4 * R, dtype=torch.float32, device=data.device)
        states = torch.empty(B, L + 1, 2 * R, dtype=torch.float32, device=data.device)
        zs = torch.empty(B, 3, Z, dtype=torch.float32, device=data.device)
        check(lib.immtsf_neural_flow_tn_forward(C.byref(d), _neural_flow_kind(time_net), ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(flat),
                                                ptr(eps), ptr(out), ptr(xg), ptr(states), ptr(zs), stream_ptr()), "neural_flow_forward")
        neural_flow_launches[time_net] += 1
        ctx.dims = (B, L, Lp, Cc) + tuple(widths)
        ctx.time_net = time_net
        ctx.save_for_backward(data, mask, tp, tpp, flat, eps, xg, states, zs)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        data, mask, tp, tpp, flat, eps, xg, states, zs = ctx.saved_tensors
        d = _neural_flow_dims(*ctx.dims)
        kind = _neural_flow_kind(ctx.time_net)
        grads = torch.empty_like(flat)      # every entry is written: no zero fill
        ws = _bytes(lib.immtsf_neural_flow_tn_workspace_bytes(C.byref(d), kind), data.device)
        check(lib.immtsf_neural_flow_tn_backward(C.byref(d), kind, ptr(data), ptr(mask), ptr(tp), ptr(tpp), ptr(flat), ptr(eps), ptr(xg),
                                                 ptr(states), ptr(zs), ptr(dout.contiguous()), ptr(grads), ptr(ws), ws.numel(),
                                                 stream_ptr()), "neural_flow_backward")
        return None, None, None, None, grads, None, None, None


def neural_flow(data, mask, tp, tp_pred, flat_params, eps, widths, time_net="TimeLinear"):
    """data, mask (B, L, C); tp (B, L), tp_pred (B, Lp): every window's own times; flat_params: every parameter in state_dict order,
    flattened; eps (B, latents); widths = (rec_dims, latents, hidden_dim, hidden_layers, flow_layers); time_net 'TimeLinear' or
    'TimeTanh' -> the forecast (B, Lp, C).  Gradients reach flat_params only."""
    B, L, Cc = data.shape
    widths = tuple(int(w) for w in widths)
    if tp_pred.dim() != 2:
        raise _lib.ImmtsfError("neural_flow: tp_pred is (B, Lp)")
    Lp = tp_pred.shape[1]
    if not neural_flow_supported(B, L, Lp, Cc, *widths, call=True, time_net=time_net):
        raise _lib.ImmtsfError(f"neural_flow: shapes outside the fused kernel (B {B}, L {L}, Lp {Lp}, C {Cc}, widths {widths}, "
                               f"time_net {time_net!r})")
    d = _neural_flow_dims(B, L, Lp, Cc, *widths)
    nv = int(_lib.load().immtsf_neural_flow_tn_param_count(C.byref(d), _neural_flow_kind(time_net)))
    if tuple(mask.shape) != (B, L, Cc) or tuple(tp.shape) != (B, L) or tuple(tp_pred.shape) != (B, Lp) or tuple(eps.shape) != (B, widths[1]) or \
            flat_params.numel() != nv or any(q.dtype != torch.float32 for q in (data, mask, tp, tp_pred, flat_params, eps)):
        raise _lib.ImmtsfError("neural_flow: the tensors are not the fp32 tensors of these dimensions")
    return NeuralFlowFn.apply(data, mask, tp, tp_pred, flat_params, eps, widths, time_net)
