"""Shapes, seeded inputs and the error measure shared by tests/test_attention_ref.py (CPU) and tests/test_gpu_attention.py (GPU).  Plain torch
on the CPU; imports nothing of immtsf."""
import torch

# ---- the short kernels (csrc/attn.hip: launch_attn_short_fwd / _bwd), shapes (B, L, H, E) of the packed (B, L, 3, H, E) tensor with the
# instance each direction is meant to reach.  `short_instance` below restates the launcher's rule; test_attention_ref.py holds this table
# to it, so that a shape edited here cannot silently stop reaching its instance (a rule edited in the launcher has to be edited there too).
SHORT = [
    ((37, 2, 1, 32), "staged<2,8>", "staged<2,8>"),       # 16 sequences per workgroup: groups 16 + 16 + 5
    ((5, 1, 3, 4), "staged<2,8>", "staged<2,8>"),         # L = 1, one partial group
    ((19, 3, 2, 20), "staged<4,8>", "staged<4,8>"),       # groups 16 + 3
    ((6, 4, 1, 32), "staged<4,8>", "staged<4,8>"),        # the instance's limits on both L and E, one partial group
    ((9, 4, 1, 36), "staged<8,16>", "staged<8,16>"),      # L <= 4 but E > 32
    ((21, 7, 2, 12), "staged<8,16>", "staged<8,16>"),     # groups 16 + 5
    ((7, 8, 2, 64), "staged<8,16>", "unstaged<8,16>"),    # three rows of LDS per sequence fit four sequences, four rows only three
    ((6, 8, 4, 64), "unstaged<8,16>", "unstaged<8,16>"),  # by the LDS cap
    ((5, 8, 9, 8), "unstaged<8,16>", "unstaged<8,16>"),   # by H L = 72 > 64; 360 threads: the second workgroup is partial
]


def short_stage_seqs(L, H, E, rows_per):
    """sequences per workgroup of the staged kernels (csrc/attn.hip: short_stage_seqs)"""
    return min(256 // (H * L), (48 * 1024) // (rows_per * L * H * E * 4), 16)


def short_instance(L, H, E, rows_per):
    """rows_per 3 = forward, 4 = backward -> the kernel instance launch_attn_short_fwd / _bwd picks"""
    if short_stage_seqs(L, H, E, rows_per) < 4:
        return "unstaged<8,16>"
    return "staged<2,8>" if L <= 2 and E <= 32 else "staged<4,8>" if L <= 4 and E <= 32 else "staged<8,16>"


# ---- csrc/attn_mid.hip (config.attn_mid), shapes (B, L, S, H, E, D)
MID = [
    (1, 32, 32, 1, 256, 256),      # 97.5 KB / 130 KB of dynamic LDS: the opt-in above 64 KB in both directions; L S = 1024: the fourth ds_mine slot
    (2, 5, 9, 3, 252, 8),          # L % 4 != 0 (idle waves in the last round), S % 8 = 1, the last lane idle, D << E
    (2, 32, 17, 2, 4, 4),          # the narrowest heads: one lane of 64 at work
    (3, 9, 12, 2, 8, 200),         # D >> E
    (1, 1, 1, 1, 4, 4),
]


def mid_supported(L, S, E, D):
    """csrc/attn_mid.hip: am_ok"""
    return 1 <= L <= 32 and 1 <= S <= 32 and 4 <= E <= 256 and 4 <= D <= 256 and E % 4 == 0 and D % 4 == 0


def mid_lds_bytes(L, S, E, D, backward):
    return ((L + S) * (E + 4) + (S + (L if backward else 0)) * (D + 4)) * 4


# ---- batched GEMMs + softmax_rows: shapes attn_mid refuses (the last one it would take: run with config.attn_mid = False)
GEMM = [
    (2, 37, 37, 2, 24, 24),        # L, S > 32; L == S: the causal variants
    (2, 33, 70, 3, 10, 6),         # S > 64: the per-lane loop of softmax_rows runs twice; E % 4 != 0
    (1, 1, 1, 1, 1, 1),
    (2, 10, 10, 2, 64, 32),        # supported by attn_mid: the knob switched off
]
GEMM_BF16 = GEMM[:2]
QKV_GEMM = [(5, 19, 3, 8), (3, 2, 1, 5)]      # (B, L, H, E): L > 8; E % 4 != 0 (not routed to the short kernel)
SHARED = [(3, 5, 2, 12, 70), (2, 1, 1, 8, 1)]      # (B, L, H, E, S)
LIVE = (3, 2, 5, 70)      # B, H, L, S with live = [1, 0, 1]

VARIANTS = [("plain", False, 0.0), ("causal", True, 0.0), ("dropout", False, 0.3), ("causal_dropout", True, 0.3)]


def variants(L, S):
    return [v for v in VARIANTS if L == S or not v[1]]


_AMP = (1.0, 0.03, 8.0)      # loud and quiet (b, h) slices side by side: a wrong quiet slice must not hide under a loud one's maximum


def _amp(B, H):
    return torch.tensor([_AMP[i % 3] for i in range(B * H)]).view(B, 1, H, 1)


def dense_inputs(shape, seed=0):
    """(B, L, S, H, E, D) -> q (B, L, H, E), k (B, S, H, E), v (B, S, H, D), upstream (B, L, H, D), float32"""
    B, L, S, H, E, D = shape
    g = torch.Generator().manual_seed(1000 + seed + 7 * B + 11 * L + 13 * S + 17 * H + 19 * E + 23 * D)
    q = torch.randn(B, L, H, E, generator=g)
    k = torch.randn(B, S, H, E, generator=g)
    v = torch.randn(B, S, H, D, generator=g) * _amp(B, H)
    up = torch.randn(B, L, H, D, generator=g) * _amp(B, H).flip(0)
    return q, k, v, up


def packed_inputs(shape, seed=0):
    """(B, L, H, E) -> qkv (B, L, 3, H, E), upstream (B, L, H, E)"""
    B, L, H, E = shape
    q, k, v, up = dense_inputs((B, L, L, H, E, E), seed)
    return torch.stack([q, k, v], dim=2).contiguous(), up


def shared_inputs(shape, seed=0):
    """(B, L, H, E, S) -> q (B, L, H, E), k (S, H, E), v (S, H, E), upstream (B, L, H, E)"""
    B, L, H, E, S = shape
    q, _, _, up = dense_inputs((B, L, S, H, E, E), seed)
    _, k, v, _ = dense_inputs((1, L, S, H, E, E), seed + 1)
    return q, k[0].contiguous(), v[0].contiguous(), up


# ---- extreme logits: E = 16, so scale = 16 ** -0.5 = 0.25 is exact, q and k hold integers in [-6, 6], so every q.k is an integer of at
# most 16 * 36 = 576 in size and every score a multiple of 0.25 up to +-144: exact in float32 whatever the order of the sum
EXTREME_E = 16
EXTREME_SCALE = 0.25


def extreme_inputs(B, L, S, H, D=16, seed=0):
    """needs L >= 4, S >= 3 and more than one (b, h) slice.  Slice (b, h) = (0, 0): every key holds 5s and 6s; query row 0 is all +6 (every
    score >= 120), query row 1 all -6 (every score <= -120: without the max subtraction every exp underflows and the row is 0 / 0).  The
    last slice: key 2 and query 3 share one +-6 pattern and its other keys stay within [-2, 2] (score 144 next to scores of at most 48:
    every other exp of that row underflows after the subtraction).  Elsewhere integers in [-6, 6]."""
    assert L >= 4 and S >= 3 and B * H >= 2
    g = torch.Generator().manual_seed(77 + seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()      # noqa: E731
    q, k = ri(-6, 6, B, L, H, EXTREME_E), ri(-6, 6, B, S, H, EXTREME_E)
    k[0, :, 0] = ri(5, 6, S, EXTREME_E)
    q[0, 0, 0] = 6.0
    q[0, 1, 0] = -6.0
    pattern = 12.0 * ri(0, 1, EXTREME_E) - 6.0
    k[-1, :, -1] = ri(-2, 2, S, EXTREME_E)
    k[-1, 2, -1] = pattern
    q[-1, 3, -1] = pattern
    v = torch.randn(B, S, H, D, generator=g)
    up = torch.randn(B, L, H, D, generator=g)
    return q, k, v, up


# ---- the error measure
def slice_error(got, want, dims=(0, 2)):
    """per slice over `dims` (the batch and head axes of the layout: (0, 2) for (B, L, H, E), (0, 1) for (B, H, L, S), (1,) for the shared
    (S, H, E)): max |got - want| over the slice / max(max |want| over the slice, 1e-6 of the largest |want| of the tensor).  A slice whose
    bound is 0 (an all-zero tensor) must be matched exactly.  -> (worst error, index of that slice among the flattened `dims`)"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    n = 1
    for d in dims:
        n *= want.shape[d]
    if want.numel() == 0:
        return 0.0, 0
    front = tuple(range(len(dims)))
    g2, w2 = got.movedim(dims, front).reshape(n, -1), want.movedim(dims, front).reshape(n, -1)
    diff = (g2 - w2).abs().amax(dim=1)
    bound = torch.clamp(w2.abs().amax(dim=1), min=1e-6 * float(w2.abs().max()))
    err = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)       # 0 / 0 = 0; x / 0 = inf
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(err.argmax())
    return float(err[i]), i


def l2_error(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    den = float(want.norm())
    num = float((got - want).norm())
    return 0.0 if num == 0.0 else num / den if den > 0 else float("inf")
