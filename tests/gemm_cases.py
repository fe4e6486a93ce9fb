"""The case table of tests/test_gpu_gemm_paths.py: one row per route of csrc/gemm.hip, gemm2.hip, gemm3.hip and linear_small.hip.

A row names the entry point, the layout (0 NT, 1 NN, 2 TN), M, N, K, the options, and the ROUTE the launcher must take for it: the
kernel code of immtsf_debug_last_gemm_launch (include/immtsf.h), the threads of the grid, and -- for the entries that pass through
immtsf_launch_gemm -- the kernel path of the timing tap's record (1 csrc/gemm.hip, 2 csrc/gemm2.hip / gemm3.hip).  `why` restates the
launcher's rule with the case's numbers filled in; tests/test_gemm_ref.py recomputes every grid from (tile, splits, block) below, so a
row cannot drift from its own reasoning, and the GPU test fails naming both routes when the launcher disagrees.

grid threads = tiles(BM, BN) * splits * block (gemm.hip / gemm2.hip); 512 * workgroups for gemm3.hip's persistent kernels.

Options (all optional): prec (immtsf_gemm's precision), alpha, bias, act (1 relu, 2 erf GELU), acc (accumulate onto an integer C),
add_vec, flag_div (int32 row flags, one per flag_div rows), dyn (a device-side M for NT / NN, K for TN), rowmap (a_rowmap with repeats),
no_c (C NULL, Ch only), ch (bf16 copy), pad = (lda, ldb, ldc, ldch) extra elements per row, twin (B registered as a bf16 twin), bgrad
(TN column sums), g3cfg (immtsf_debug_gemm3_config's first argument), real (also run a real-operand instance against gemm_ref.bound),
f32 (the kernel multiplies fp32 values whatever the precision)."""


def cdiv(a, b):
    return (a + b - 1) // b


CASES = []


def case(id, entry, layout, M, N, K, code, tile, splits, block, why, path=None, grid=None, **opt):
    g = grid if grid is not None else cdiv(M, tile[0]) * cdiv(N, tile[1]) * splits * block
    CASES.append(dict(id=id, entry=entry, layout=layout, M=M, N=N, K=K, code=code, tile=tile, splits=splits, block=block, grid=g, path=path,
                      why=why, opt=opt))


L = ("nt", "nn", "tn")

# ---------------------------------------------------------------------------------------------- immtsf_gemm, precision 0 (fp32 MFMA)
for lay in (0, 1, 2):
    case(f"f32-64-scalar-{L[lay]}", "gemm", lay, 37, 50, 19, 1900, (64, 64), 1, 256,
         "tiles128 = 1 < 512 -> 64x64x16; lda / ldb / ldc not multiples of 4 -> scalar loaders; ldc != N -> no split", path=1, prec=0,
         pad=(2, 3, 1, 0), real=True)
    case(f"f32-64-{L[lay]}", "gemm", lay, 100, 72, 136, 1900, (64, 64), 1, 256,
         "tiles128 = 1 < 512 -> 64x64x16; tiles = 4, ksteps = cdiv(136, 64) = 3 < 8 -> no split", path=1, prec=0, real=True)
    case(f"f32-128-{L[lay]}", "gemm", lay, 2881, 2881, 24, 1901, (128, 128), 1, 256,
         "tiles128 = 23 * 23 = 529 >= 512 -> 128x128x16; tiles = 2116 >= 256 -> no split", path=1, prec=0, real=True)
    case(f"f32-splitk-{L[lay]}", "gemm", lay, 128, 16, 2048, 1900, (64, 64), 16, 256,
         "tiles = 2 < 192, ksteps = 32 >= 8 -> splits = min(512 / 2, 32 / 2) = 16, zero-fill + atomics", path=1, prec=0)
    case(f"f32-splitk-acc-{L[lay]}", "gemm", lay, 128, 16, 2048, 1900, (64, 64), 16, 256,
         "as f32-splitk; accumulate: no zero-fill, the atomics add onto the old C", path=1, prec=0, acc=1)
    case(f"f32-epi-{L[lay]}", "gemm", lay, 100, 72, 136, 1900, (64, 64), 1, 256,
         "as f32-64; relu keeps split-K off whatever K", path=1, prec=0, bias=1, alpha=0.5, act=1, real=True)

# ---------------------------------------------------------------------------------------------- immtsf_gemm, precision 1 (bf16 staged)
case("bf-v11-nt", "gemm", 0, 100, 72, 136, 1011, (64, 64), 1, 512, "tiles128 = 1; K % 128 = 8 -> v11; K % 32 = 8 -> not v7", path=1, prec=1, real=True)
case("bf-v11-tn", "gemm", 2, 100, 72, 136, 1011, (64, 64), 1, 512, "TN -> v11; tiles = 4 < 96 -> not the specialised v15", path=1, prec=1, real=True)
for lay in (0, 1):
    case(f"bf-v14-{L[lay]}", "gemm", lay, 96, 80, 256, 1014, (64, 64), 1, 512, "tiles128 = 1; K % 128 = 0, not TN -> v14; ksteps = 4 < 8 -> no split",
         path=1, prec=1)
    case(f"bf-v7-{L[lay]}", "gemm", lay, 70, 90, 96, 1007, (64, 64), 1, 256, "K % 64 = 32, K % 32 = 0, K <= 512 -> v7 (64x64x32)", path=1, prec=1, real=True)
    case(f"bf-v4-{L[lay]}", "gemm", lay, 2881, 2881, 72, 1004, (128, 128), 1, 256, "tiles128 = 529 >= 512 -> v4 (128x128x64)", path=1, prec=1, real=True)
case("bf-v15-tn", "gemm", 2, 704, 704, 264, 1015, (64, 64), 1, 512,
     "TN, tiles = 11 * 11 = 121 in 96..230, K = 264 >= 256, aligned -> tn_spec v15 (2 x 256 threads), unsplit; K % 64 = 8", path=1, prec=1)
case("bf-v11-twin", "gemm", 0, 100, 72, 136, 1111, (64, 64), 1, 512, "as bf-v11-nt; B inside a registered twin, ldb % 8 = 0 -> BBF instance",
     path=1, prec=1, twin=1, real=True)
case("bf-v14-twin", "gemm", 1, 96, 80, 256, 1114, (64, 64), 1, 512, "as bf-v14-nn; B from its twin", path=1, prec=1, twin=1)
case("bf-v7-twin", "gemm", 0, 70, 90, 96, 1107, (64, 64), 1, 256, "as bf-v7-nt; B from its twin", path=1, prec=1, twin=1, real=True)
case("bf-v4-twin", "gemm", 1, 2881, 2888, 72, 1104, (128, 128), 1, 256,
     "as bf-v4-nn (N = 2888: an NN twin needs ldb = N % 8 = 0); tiles128 = 23 * 23 = 529; B from its twin", path=1, prec=1, twin=1, real=True)
case("bf-splitk-nt", "gemm", 0, 128, 16, 2048, 1014, (64, 64), 16, 512, "K % 128 = 0 -> v14; tiles = 2, ksteps = 32 -> 16 splits", path=1, prec=1)
case("bf-splitk-tn", "gemm", 2, 128, 16, 2048, 1011, (64, 64), 16, 512, "TN -> v11; tiles = 2, ksteps = 32 -> 16 splits", path=1, prec=1, acc=1)

# ---------------------------------------------------------------------------------------------- the skinny kernels of gemm.hip
# (exact fp32 FMAs in BOTH precision modes -- f32: the real-operand reference multiplies the fp32 values, not bf16 images; they take no MFMA tile: grid = cdiv(M * N / 4, 256) * 256 threads for skinny_k, cdiv(M, 4) * 256 for skinny_n)
for prec in (0, 1):
    for K in (8, 16):
        for lay in (0, 1):
            case(f"skinny-k{K}-{L[lay]}-p{prec}", "gemm", lay, 259, 68, K, 1800, None, 1, 256,
                 f"M = 259 >= 256, K = {K}, N = 68 >= 64, N % 4 = 0, aligned, no accumulate -> skinny_k", path=1, grid=cdiv(259 * 17, 256) * 256,
                 prec=prec, bias=1, real=True, f32=1)
    for N in (8, 16):
        for acc in (0, 1):
            case(f"skinny-n{N}-acc{acc}-p{prec}", "gemm", 1, 259, N, 70, 1801, None, 1, 256,
                 f"NN, M = 259 >= 256, N = {N}, K = 70 >= 64, no bias; lda = 72 (K = 70 is no multiple of 4: the rule needs lda % 4 = 0) -> skinny_n",
                 path=1, grid=cdiv(259, 4) * 256, prec=prec, acc=acc, pad=(2, 0, 0, 0), real=True, f32=1)
case("skinny-not-m255", "gemm", 0, 255, 68, 8, 1900, (64, 64), 1, 256, "M = 255 < 256 -> MFMA tile", path=1, prec=0, bias=1, real=True)
case("skinny-not-k12", "gemm", 0, 259, 68, 12, 1900, (64, 64), 1, 256, "K = 12 is neither 8 nor 16 -> MFMA tile", path=1, prec=0, bias=1, real=True)
case("skinny-not-n12", "gemm", 1, 259, 12, 70, 1900, (64, 64), 1, 256, "N = 12 is neither 8 nor 16 -> MFMA tile", path=1, prec=0, pad=(2, 0, 0, 0), real=True)

# ---------------------------------------------------------------------------------------------- erf GELU (bar 8 * 2^-24 * max(|z|, 1))
case("gelu-p0", "gemm", 0, 100, 72, 136, 1900, (64, 64), 1, 256, "as f32-64-nt", path=1, prec=0, bias=1, act=2)
case("gelu-p1", "gemm", 0, 100, 72, 136, 1011, (64, 64), 1, 512, "as bf-v11-nt", path=1, prec=1, bias=1, act=2)

# ---------------------------------------------------------------------------------------------- immtsf_gemm_bf16 (gemm2.hip; no tap)
V17 = "n64 = 2 * 2 = 4 <= 272 -> v17 (64x64, 4 K groups, 1024 threads)"
for lay in (0, 1):
    for name, o in (("plain", {}), ("relu", dict(act=1)), ("alpha2", dict(alpha=2.0)), ("acc", dict(acc=1)), ("chonly", dict(no_c=1, ch=1)),
                    ("pitch", dict(ch=1, pad=(0, 0, 4, 8))), ("rowmap", dict(rowmap=1)), ("dynm", dict(dyn=37)),
                    ("all", dict(act=1, alpha=2.0, acc=1, ch=1, pad=(8, 8, 4, 8), rowmap=1, dyn=37, bias=1))):
        case(f"g2-v17-{name}-{L[lay]}", "gemm_bf16", lay, 100, 72, 136, 2017, (64, 64), 1, 1024,
             V17 + ("; device M 37 of 100: Meff = 57, the grid keeps the bound's 4 tiles" if "dyn" in o else ""), real=(name in ("plain", "all")), **o)
case("g2-v16", "gemm_bf16", 0, 1088, 1152, 72, 2016, (64, 96), 1, 1024, "n64 = 17 * 18 = 306 > 272; N % 96 = 0, n96 = 17 * 12 = 204 <= 272 -> v16", bias=1, ch=1, real=True)
case("g2-v9", "gemm_bf16", 0, 1800, 640, 72, 2009, (64, 64), 1, 512, "n64 = 29 * 10 = 290 > 272; N % 96 != 0 and N < 960 -> v9 (8 waves)", bias=1, ch=1, real=True)
case("g2-v7-tn", "gemm_bf16", 2, 2944, 2944, 72, 2007, (256, 128), 1, 512, "t128 = 23 * 23 = 529 >= 512, TN -> v7 (256x128)", bgrad=1, real=True)
case("g2-v7-nt", "gemm_bf16", 0, 4096, 2048, 72, 2007, (256, 128), 1, 512,
     "t128 = 32 * 16 = 512 < 1024 -> v7; relu keeps it off gemm3 (cdiv(M, 128) * cdiv(N, 256) = 256 >= 192)", bias=1, act=1, real=True)
case("g2-v13-nt", "gemm_bf16", 0, 4096, 4096, 72, 2013, (256, 256), 1, 512, "t128 = 32 * 32 = 1024, NT, N >= 1024 -> v13 (256x256); relu keeps it off gemm3",
     bias=1, act=1, real=True)
case("g2-skinny-tn", "gemm_bf16", 2, 32, 1032, 2056, 2017, (64, 64), 4, 1024, "TN, M = 32 <= 64, N = 1032 >= 1024, K = 2056 >= 2048 -> 4 atomic splits of v17", bgrad=1)
case("g2-v18-dynk", "gemm_bf16", 2, 256, 256, 16384, 2018, (128, 128), 8, 512,
     "TN, K >= 16384, t128 = 4 <= 72 -> long_k v18, splits = min(256 / 4, 8) = 8; device K 9000", bgrad=1, dyn=9000)

# ---------------------------------------------------------------------------------------------- immtsf_gemm3_bf16 (gemm3.hip; no tap)
# tile = argmin over {256x256, 128x256, 256x192 (NT / NN)} of rounds(tiles / 256) * area * (1.18 if 128 rows) * (1.06 if 192 wide);
# grid = tiles rounded up to 8 (<= 256) workgroups of 512 threads, 256 workgroups with a device-side row count
G3S = "(200, 264): 128x256 costs 1 * 32768 * 1.18 = 38666 < 256x192 52101 < 256x256 65536; 2 * 2 = 4 tiles -> 8 workgroups"
for lay in (0, 1):
    case(f"g3-128-{L[lay]}", "gemm3", lay, 200, 264, 72, 3000, None, 1, 512, G3S, grid=8 * 512, real=True)
    case(f"g3-128-epi-{L[lay]}", "gemm3", lay, 200, 264, 72, 3000, None, 1, 512, G3S + "; the flag group of rows 126..132 straddles the tile edge at 128",
         grid=8 * 512, bias=1, add_vec=1, flag_div=7, ch=1, pad=(0, 0, 4, 8), alpha=0.5, real=True)
    case(f"g3-128-dyn-{L[lay]}", "gemm3", lay, 200, 264, 72, 3000, None, 1, 512, G3S + "; device rows 131 -> the full 256 workgroups", grid=256 * 512,
         bias=1, add_vec=1, flag_div=7, dyn=131, no_c=1, ch=1)
    case(f"g3-f128-{L[lay]}", "gemm3", lay, 200, 264, 72, 3000, None, 1, 512, "forced 128 rows: 128x256 the only candidate", grid=8 * 512, g3cfg=128, bias=1)
    case(f"g3-f256-{L[lay]}", "gemm3", lay, 200, 264, 72, 3001, None, 1, 512, "forced 256 rows and 256 columns; 1 * 2 = 2 tiles -> 8 workgroups", grid=8 * 512,
         g3cfg=256 | (1 << 12), bias=1, flag_div=7, ch=1)
    case(f"g3-f192-{L[lay]}", "gemm3", lay, 200, 264, 72, 3002, None, 1, 512, "forced 192 columns (256 rows); device rows 131 -> the full 256 workgroups", grid=256 * 512,
         g3cfg=2 << 12, bias=1, add_vec=1, ch=1, dyn=131)
case("g3-192-own", "gemm3", 0, 4100, 2048, 72, 3002, None, 1, 512,
     "256x192: 17 * 11 = 187 tiles, 1 round, 52101 < 256x256 (136 tiles) 65536 < 128x256 (264 tiles, 2 rounds) 77332; 187 -> 192 workgroups", grid=192 * 512,
     bias=1, real=True)
case("g3-256-own", "gemm3", 1, 4100, 2888, 72, 3001, None, 1, 512,
     "256x256: 17 * 12 = 204 tiles, 1 round, 65536 < 128x256 (396 tiles, 2 rounds) 77332 < 256x192 (272 tiles, 2 rounds) 104202; 204 -> 208 workgroups",
     grid=208 * 512, bias=1, real=True)
case("g3-tn", "gemm3", 2, 264, 200, 72, 3000, None, 1, 512, "TN (no 192 tile): 128x256 3 tiles 38666 < 256x256 65536; 3 -> 8 workgroups", grid=8 * 512, real=True)
case("g3-tn-split", "gemm3_tn", 2, 64, 96, 8192, 3010, None, 21, 512,
     "1 tile, nk = 128: S = 256 shrinks until nk / S >= 6 -> 21 splits = 21 items -> 24 workgroups, then the reduce launch", grid=24 * 512, acc=1, alpha=0.5,
     bgrad=1)

BY_ID = {c["id"]: c for c in CASES}

# ---------------------------------------------------------------------------------------------- immtsf_linear_backward
# linear_small.hip is no GEMM launcher: its route is known from the timing tap recording NO launch for the call (every product of the
# GEMM route passes through immtsf_launch_gemm and is recorded).  With dW given it is taken only when grads_prezeroed != 0.
LINEAR_SMALL = [(1, 1, 1), (300, 5, 42), (4096, 32, 64)]
# (M, N, K) just outside -> per precision the records [dx (NN, M x K over N), dW (TN, N x K over M)] as (code, grid threads)
LINEAR_GEMM = {
    (4097, 32, 64): {0: [(1900, 65 * 256, "65 tiles, ksteps 1"), (1900, 32 * 256, "1 tile, ksteps = 65 -> min(512, 32) = 32 splits")],
                     1: [(1007, 65 * 256, "reduction 32: % 64 != 0, % 32 = 0 -> v7"), (1011, 32 * 512, "TN -> v11, 32 splits")]},
    (300, 33, 42): {0: [(1900, 5 * 256, "5 tiles"), (1900, 256, "1 tile, ksteps = 5 < 8")],
                    1: [(1011, 5 * 512, "reduction 33 -> v11"), (1011, 512, "TN -> v11, unsplit")]},
}

# ---------------------------------------------------------------------------------------------- immtsf_gemm_bf16_group_tn
# members (M, N, K); sum of 128-tiles < 192 -> 64x64 K-group tiles (code 2900), grid = sum of 64-tiles * 1024 threads
GROUPS = {2: [(8, 8, 40), (72, 136, 8)],
          6: [(8, 8, 40), (72, 136, 8), (64, 64, 264), (104, 40, 100), (136, 72, 72), (200, 8, 16)]}

# ---------------------------------------------------------------------------------------------- immtsf_linear_bf16_forward / _backward
LINEAR_BF16 = dict(M=70, N=24, K=40, why="every product is v17 of gemm2.hip (path 2): forward 2 * 1 tiles * nl problems * 1024 threads; dx 2 tiles; "
                                         "the nl weight gradients one grouped record (layout code 3, path 3) or, nl = 1, one TN launch of 1 tile")


def extras(opt):
    """largest magnitude of the integer addends of a case (bias, add_vec, old C: each <= 3)"""
    return 3.0 * (bool(opt.get("bias")) + bool(opt.get("add_vec")) + bool(opt.get("acc")))
