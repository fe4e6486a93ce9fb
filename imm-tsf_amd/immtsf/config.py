"""Process-wide knobs of the HIP path."""
import os
import threading

_PRECISIONS = {"fp32": 0, "bf16": 1}

# "fp32": exact-fp32 MFMA (parity with the reference's fp32 CPU path); "bf16": bf16 MFMA operands, fp32 accumulate.
precision = os.environ.get("IMMTSF_PRECISION", "fp32")

# How the reference's `torch.isnan(x).any()` guards (fusions/FusionModel.py:103-112, TTF_*.py:116/75) are honoured:
#   "sync"     -- like the reference: check (and host-sync) inside forward, raise ValueError immediately (5 host syncs per step: the
#                 seam then runs every launch eagerly, 3.2 ms per step at the benchmark configuration)
#   "deferred" -- (default since round 5; a documented deviation) the same ValueError, raised at the NEXT host-visible point: the kernels
#                 OR a device flag, lib.evaluation leaves "loss is NaN / notes held NaN" in pinned memory by an asynchronous copy, and the
#                 next compute_all_losses() / evaluation() call -- or FusionModel.check_nan() -- raises; no host sync inside the step
#   "off"      -- no checks
nan_check = os.environ.get("IMMTSF_NAN_CHECK", "deferred")


def precision_code(p=None) -> int:
    p = precision if p is None else p
    if p not in _PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {p!r}")
    return _PRECISIONS[p]


# dropout seeds: (base seed, call counter) -> one 64-bit Philox key per forward call
_lock = threading.Lock()
_base_seed = None
_counter = 0


def manual_seed(seed: int):
    global _base_seed, _counter
    with _lock:
        _base_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        _counter = 0


def next_seed() -> int:
    """A fresh Philox key; deterministic after torch.manual_seed()/immtsf.config.manual_seed()."""
    global _base_seed, _counter
    with _lock:
        if _base_seed is None:
            import torch
            _base_seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
        _counter += 1
        x = (_base_seed + 0x9E3779B97F4A7C15 * _counter) & 0xFFFFFFFFFFFFFFFF
        # splitmix64 finaliser
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 31
        return x


# ---- device-side step counters (hipGraph replay) -----------------------------------------------------------
# When a training step is captured into a hipGraph every host-side scalar is frozen into the graph.  Two scalars
# must still change per replay: the dropout key and Adam's step number.  With device counters enabled the fusion
# kernels add *dropout_step to their Philox key and the fused Adam kernel reads/increments *adam_step.
_device_counters = {}


def enable_device_counters(device):
    """-> (adam_step int64[1], dropout_step int64[1]) tensors on `device`; from now on every fusion forward on that
    device passes the dropout counter to the kernels."""
    import torch
    key = str(device)
    if key not in _device_counters:
        _device_counters[key] = (torch.zeros(1, dtype=torch.int64, device=device),
                                 torch.zeros(1, dtype=torch.int64, device=device))
    return _device_counters[key]


def disable_device_counters(device=None):
    if device is None:
        _device_counters.clear()
    else:
        _device_counters.pop(str(device), None)


def dropout_counter_ptr(device):
    c = _device_counters.get(str(device))
    return None if c is None else c[1].data_ptr()

# Alternative formulations kept as cross-checks of the default ones (tests flip these attributes; no environment variables):
# MMF_XAttn_Add in its low-rank form (csrc/xrank.hip) wherever its limits allow; False: the full-rank key/value + query halves
xattn_rank = True
# ... and, for a training step whose loss is the masked MSE with known observation counts, the Q half + loss + their backward as ONE
# launch (MMF_XAttn_Add.forward_loss); False: the Q half and the loss as separate ops
xattn_fused_loss = True
# FusionModel: TTF_T2V_XAttn's proj_out composed into MMF_XAttn_Add's low-rank projection: "auto" / True = wherever the pair of blocks
# allows it, False = the two blocks as written (tests run both)
fuse_tail = "auto"
# the zero-edit seam (lib.evaluation.compute_all_losses) serves a repeated (model, fusion, batch shape) from a replayed hipGraph when
# nan_check is "deferred" (no host syncs inside the step); False: every call is launched eagerly
seam_graph = True
# TTF_T2V_XAttn: "auto" = the library chooses by batch size (the folded form, csrc/t2v_fold.hip, from IMMTSF_T2V_FOLD_MIN_ROWS padded note
# rows on -- its parameter-only chains are a fixed cost; its mix-first variant, csrc/t2v_premix.hip, for windows of more than 64 padded
# notes in bf16 mode), "fold" = the folded form wherever its limits hold, "mix" = the mix-first variant wherever ITS limits hold (bf16
# mode, one head, T <= 32), "chain" = the reference's GEMM chain as written
t2v_form = "auto"
# TTF_T2V_XAttn on PackedNotes: use the batch's prebuilt ragged index (PackedNotes.index(), built once per batch) instead of deriving
# it inside every forward; False: the call derives it (two launches at its head) -- the cross-check
note_index = True
# the fused TTF_T2V_XAttn -> MMF_XAttn_Add tail (FusionModel.fused_tail) hands Z over as its bf16 image ALONE (no fp32 Z: it has no reader
# in the bf16 dataflow) and takes the gradient back in LOW-RANK form (dP, Wc) -- dZ = dP Wc is formed inside the LayerNorm backward
# instead of being written and re-read (0.8 GB per step at 4096 windows, one launch on the text chain at 64).  False: the dense hand-over
# in both directions -- the cross-check
# MMF_GR_Add in split form (csrc/gr_train.hip: the text columns of its two linear maps ahead of the backbone, the Y half + loss + backward as
# one launch); False: the block as written -- the cross-check
gr_split = True
z_handover = os.environ.get("IMMTSF_Z_HANDOVER", "1") != "0"
# FullAttention over <= 32 positions with heads up to 256 wide as one kernel per direction (csrc/attn_mid.hip); False: batched GEMMs +
# row softmax
attn_mid = True
# lib.evaluation.evaluation() on immtsf.EvalStep (forward + fused metric kernel per batch shape as a replayed hipGraph, one device -> host
# copy per loader); False (the default): the eager forward and the metrics as torch ops
eval_engine = os.environ.get("IMMTSF_EVAL_ENGINE", "0") == "1"
# DLinear.forecasting() as one HIP launch per direction (csrc/dlinear.hip) wherever immtsf_dlinear_supported allows; IMMTSF_DLINEAR_FUSED=0:
# the composed path (torch element-wise ops around three immtsf.ops.linear calls) -- the cross-check.  fp32 in either precision mode
dlinear_fused = os.environ.get("IMMTSF_DLINEAR_FUSED", "1") != "0"
# TimeMixer.forecasting() as one HIP launch forward and two backward (csrc/timemixer.hip) wherever the options are the reference's defaults
# and immtsf_timemixer_supported allows; IMMTSF_TIMEMIXER_FUSED=0: the composed path (one embedding kernel per scale, torch element-wise
# ops around immtsf.ops.linear calls) -- the cross-check.  fp32 in either precision mode
timemixer_fused = os.environ.get("IMMTSF_TIMEMIXER_FUSED", "1") != "0"
# TTM's narrow mixer blocks (patch / channel) as one HIP launch forward and two backward, and the feature mixer's gate + residual as one
# launch per direction (csrc/ttm.hip), block by block wherever immtsf_ttm_mixer_supported allows; IMMTSF_TTM_FUSED=0: the composed path
# (torch element-wise ops and permutes around immtsf.ops.linear / layer_norm calls) -- the cross-check.  The kernels are fp32 in either mode
ttm_fused = os.environ.get("IMMTSF_TTM_FUSED", "1") != "0"
# Informer's layers: ProbAttention as two HIP launches per direction (csrc/prob_attn.hip) wherever immtsf_prob_attention_supported allows,
# and ConvLayer's BatchNorm + ELU + MaxPool on rows (csrc/conv_distil.hip) wherever immtsf_conv_distil_supported allows;
# IMMTSF_INFORMER_FUSED=0: the composed path (torch gather / sort / scatter, nn.BatchNorm1d, nn.MaxPool1d) with the same tie rule -- the
# cross-check.  The kernels are fp32 in either precision mode
informer_fused = os.environ.get("IMMTSF_INFORMER_FUSED", "1") != "0"
# Informer's model (models.Informer): everything around the layers -- padding, masked instance norm, the input concatenations and both
# DataEmbeddings as one HIP launch forward and two backward, decoder.norm + decoder.projection + de-normalisation + the slice to the horizon
# as one forward and two backward (csrc/informer.hip) -- wherever immtsf_informer_model_supported allows, c_out == C, the batch fits the
# model lengths and wants no gradient; IMMTSF_INFORMER_MODEL_FUSED=0: the composed path (the reference's sequence on torch ops,
# immtsf.ops.token_embed, layer_norm and linear) -- the cross-check.  Independent of informer_fused, which steers the layers.  fp32 in
# either precision mode
informer_model_fused = os.environ.get("IMMTSF_INFORMER_MODEL_FUSED", "1") != "0"
# TimesNet's model (models.TimesNet): everything around the TimesBlock loop -- padding, plain instance norm, the input concatenation,
# DataEmbedding, the horizon rows and predict_linear as one HIP launch forward and two backward (csrc/timesnet_model.hip), the last
# layer_norm + projection + de-normalisation + the slice to the horizon as one forward and two backward (csrc/informer.hip's tail kernels
# with a row offset) -- wherever immtsf_timesnet_model_supported allows, c_out == enc_in, the batch fits the model lengths and wants no
# gradient; IMMTSF_TIMESNET_MODEL_FUSED=0: the composed path (torch cats and permutes around immtsf.ops.token_embed, linear and layer_norm),
# bit for bit what it was -- the cross-check.  fp32 in either precision mode
timesnet_model_fused = os.environ.get("IMMTSF_TIMESNET_MODEL_FUSED", "1") != "0"
# ... and only up to the largest size at which the route measured not slower than the composed one: (input_len + pred_len)^2 * d_model <=
# this (cfg4's 64^2 * 16; at 192^2 * 64 the fused step measured 1.7 % slower).  None: no bound (tools/timesnet_bench.py --model
# measures the kernels on both sides of it)
timesnet_model_max_work = 64 * 64 * 16
# whether that front end keeps its embedded rows E (B, input_len, d_model) for the backward (1) or forms them again there (0, the
# default: DESIGN 4e has the measurement)
timesnet_model_save_e = os.environ.get("IMMTSF_TIMESNET_MODEL_SAVE_E", "0") == "1"
# CRU's Kalman recurrence as one HIP launch forward and two backward (csrc/cru.hip) wherever the cell is the continuous CRUCell with the
# single Linear + softmax coefficient net and immtsf_cru_supported allows; IMMTSF_CRU_FUSED=0: the composed path (a Python loop over the
# time points around torch.matrix_exp) -- the cross-check.  The kernels are fp32 in either precision mode
cru_fused = os.environ.get("IMMTSF_CRU_FUSED", "1") != "0"
# TimeLLM's frozen GPT-2 body on csrc/gpt2.hip + the GEMM family (immtsf.ops.gpt2_body: causal attention with a prefix, the last block and
# the whole backward over the reprogrammed patch rows only, bf16 weight images in bf16 mode) wherever gpt2_body_supported allows;
# IMMTSF_TIMELLM_FUSED=0: transformers' GPT2Model on stock PyTorch in fp32 -- the cross-check.  Follows config.precision
timellm_fused = os.environ.get("IMMTSF_TIMELLM_FUSED", "1") != "0"
# A BERT body (immtsf.ops.bert_body, csrc/bert_body.hip) takes the fused path in bf16 mode only: in fp32 mode it measured slower than the
# stock call (178 vs 72 ms), so fp32 mode keeps the stock call unless IMMTSF_TIMELLM_BERT_FP32=1 asks for the operator (the
# cross-check of the two paths at fp32 accuracy; less saved memory).  Under timellm_fused either way
timellm_bert_fp32 = os.environ.get("IMMTSF_TIMELLM_BERT_FP32", "0") == "1"
# How the frozen GPT-2 / Llama / BERT bodies and the three note-embedding operators form their weight products in fp32 mode (bf16 mode
# never reads this).  "fp32": fp32 operands on the f32 MFMA, as ever.  "split": every product that immtsf_gemm_split_supported allows
# runs on the bf16 MFMA over two cached bf16 images of the frozen weight and the activation cut in registers (csrc/gemm_split.hip,
# 16 - 17 significant bits per operand, three MFMA passes); the rest of the body stays the fp32-mode one
frozen_products = os.environ.get("IMMTSF_FROZEN_PRODUCTS", "fp32")
_FROZEN_PRODUCTS = ("fp32", "split")


def frozen_split(precision_code_: int) -> bool:
    """whether a frozen body at this precision code forms its products on the split-bf16 kernel"""
    if frozen_products not in _FROZEN_PRODUCTS:
        raise ValueError(f"frozen_products must be one of {sorted(_FROZEN_PRODUCTS)}, got {frozen_products!r}")
    return precision_code_ == 0 and frozen_products == "split"
# TimeLLM's prompt statistics (min, max, median, trend, top lags of every window) in ONE launch and ONE device-to-host copy per
# forecasting() call (immtsf.ops.timellm_prompt_stats, csrc/timellm_prompt.hip) wherever timellm_prompt_supported allows;
# IMMTSF_TIMELLM_PROMPT_FUSED=0: the torch expressions with rfft / irfft and five host reads per window -- the cross-check.  The text is
# formatted and tokenised on the host either way
timellm_prompt_fused = os.environ.get("IMMTSF_TIMELLM_PROMPT_FUSED", "1") != "0"
# TimeLLM's word prototypes (the reprogramming layer's keys and values) in folded form: W_map (E [Wk^T | Wv^T]) instead of
# (W_map E) Wk^T, (W_map E) Wv^T, so the (ts_vocab_size, d_llm) table is never formed and the mapping weight is read once per direction
# (immtsf.ops.timellm_prototypes, csrc/timellm_reprogram.hip) wherever timellm_prototypes_supported allows and the fold has
# fewer flops (ts_vocab_size d_llm > 2 D (d_llm + ts_vocab_size)); IMMTSF_TIMELLM_REPROGRAM_FUSED=0: the three linear() calls as the
# reference writes them -- the cross-check
timellm_reprogram_fused = os.environ.get("IMMTSF_TIMELLM_REPROGRAM_FUSED", "1") != "0"
# Raw-text mode (fusions.load_llm.embed_notes, immtsf.text.embed_corpus): a frozen GPT2Model over the notes' REAL tokens only, packed
# back to back (immtsf.ops.gpt2_embed_notes: csrc/note_embed.hip + the GEMM family + the row kernels of csrc/gpt2.hip), wherever
# gpt2_embed_notes_supported allows and the tokenizer pads on the right; IMMTSF_NOTE_EMBED_FUSED=0: the reference's formulation (every
# note padded to max_length, transformers' model on stock PyTorch, masked mean) -- the cross-check.  Follows config.precision
note_embed_fused = os.environ.get("IMMTSF_NOTE_EMBED_FUSED", "1") != "0"
# ... in fp32 mode only for calls of at least this many notes: a single note per call measured 0.88x of the padded call there (the
# small-row fp32 GEMMs), several notes 2.4x.  bf16 mode takes the fused path at any count (2.6x / 7.0x)
note_embed_fp32_min_notes = int(os.environ.get("IMMTSF_NOTE_EMBED_FP32_MIN_NOTES", "2"))
# The same switch covers a frozen BertModel (immtsf.ops.bert_embed_notes: csrc/bert_embed.hip, the non-causal ragged attention of
# csrc/note_embed.hip, the GEMM family).  Its fp32 threshold is its own knob, measured on its own: a single note per call
# 0.95x of the padded call (within the passes' spread of it: no win), 32 notes 1.8x.  bf16 mode takes the fused path at any count
# (1.9x / 4.7x)
bert_embed_fp32_min_notes = int(os.environ.get("IMMTSF_BERT_EMBED_FP32_MIN_NOTES", "2"))
# ... and a frozen LlamaModel (immtsf.ops.llama_embed_notes: csrc/llama_embed.hip, the GEMM family), again with its own fp32 threshold.
# Measured at Llama-3.1-8B's widths a single note per call is 3.0x the padded call in fp32 and 32 notes 2.0x (bf16: 8.5x /
# 20x), so nothing is gated off: the threshold is 1
llama_embed_fp32_min_notes = int(os.environ.get("IMMTSF_LLAMA_EMBED_FP32_MIN_NOTES", "1"))
# A frozen LlamaModel STORED in bf16 (every parameter torch.bfloat16: what from_pretrained returns for Llama-3.1 / deepseek-llm under
# dtype="auto") on the same two operators, read in place: in bf16 mode the GEMM family takes the parameter's own storage as the
# bf16 image, in fp32 mode every product is immtsf_gemm_asplit (fp32 activations cut in registers against the stored weight, whatever
# frozen_products says), the row kernels read bf16 parameters (the _p16 entry points), and q | k | v and gate | up are products side by
# side instead of one product on a concatenated copy -- no second image of any weight.  OFF unless IMMTSF_LLAMA_STORED_BF16=1:
# tests/test_gpu_llama_embed.py and test_gpu_llama_body.py pin that a bf16 model with nothing set is refused (the padded stock call)
llama_stored_bf16 = os.environ.get("IMMTSF_LLAMA_STORED_BF16", "0") == "1"
# LatentODE's forecasting() as one HIP launch forward and two backward (csrc/latent_ode.hip) wherever the encoder is the ODE-RNN with
# rec_layers = gen_layers = 1, one trajectory sample, and immtsf_latent_ode_supported allows; IMMTSF_LATENTODE_FUSED=0: the composed path
# (the reference's loop over the observed points on torch ops, the step plan copied to the host once) -- the cross-check.  fp32 in
# either precision mode
latentode_fused = os.environ.get("IMMTSF_LATENTODE_FUSED", "1") != "0"
# NeuralFlow's forecasting() as two HIP launches forward and three backward (csrc/neural_flow.hip) wherever the flow is the coupling flow
# with the TimeLinear time net and immtsf_neural_flow_supported allows; IMMTSF_NEURALFLOW_FUSED=0: the composed path (the reference's
# loop over the observed points on torch ops) -- the cross-check.  fp32 in either precision mode
neuralflow_fused = os.environ.get("IMMTSF_NEURALFLOW_FUSED", "1") != "0"
# ... and the same launches for nf_time_net='TimeTanh' (the TimeTanh instance of those kernels), under every condition above.  OFF unless
# IMMTSF_NEURALFLOW_TANH_FUSED=1: tests/test_gpu_neuralflow.py pins that a TimeTanh model with nothing set takes the composed path, and
# what ran before this instance existed keeps running as it did.  neuralflow_fused off turns both off
neuralflow_tanh_fused = os.environ.get("IMMTSF_NEURALFLOW_TANH_FUSED", "0") == "1"
# lib.parse_datasets.parse_datasets() returns immtsf.data.ResidentLoader objects over a ResidentStore (the dataset in HBM, every batch
# built on the device, one id upload per epoch); IMMTSF_RESIDENT_LOADER=0: the reference module's own host loaders, when a
# reference tree is on the path (NotImplementedError otherwise)
resident_loader = os.environ.get("IMMTSF_RESIDENT_LOADER", "1") != "0"
# immtsf.optim.FusedAdam under torch.amp.GradScaler takes the loss scale inside its two launches (the clip on the gradient as stored, the
# unscale and the skip decision on the device: no foreach unscale, no host read of found_inf); IMMTSF_OPTIM_AMP=0: GradScaler's generic
# route (it unscales every .grad, reads found_inf on the host, then calls step()) -- read when the optimizer is built
optim_amp = os.environ.get("IMMTSF_OPTIM_AMP", "1") != "0"
# TimesBlock's period selection (the amplitude spectrum, the top-k, the periods and image row counts, the softmaxed weights, the
# position-major copy of the series) as two HIP launches forward and one backward (immtsf.ops.timesnet_spectrum: csrc/timesnet_spectrum.hip,
# a direct DFT -- no FFT library in the step) on the device-period branch wherever immtsf_timesnet_spectrum_ok allows;
# IMMTSF_TIMESNET_SPECTRUM_FUSED=0: torch.fft.rfft / topk / softmax / pad as before -- the cross-check.  fp32 in either precision mode
timesnet_spectrum_fused = os.environ.get("IMMTSF_TIMESNET_SPECTRUM_FUSED", "1") != "0"
