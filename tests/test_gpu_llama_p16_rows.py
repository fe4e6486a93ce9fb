"""GPU checks of the _p16 entry points of csrc/llama_embed.hip and csrc/llama_body.hip: the row kernels of a frozen Llama with the model's
parameter (the embedding table, an RMSNorm weight) read as bf16.  The kernels are the fp32 ones with the parameter type as a template
argument and the up-cast in registers, so each _p16 call on bf16 parameters must give, bit for bit (torch.equal on every output), what its
fp32 sibling gives on the parameters up-cast to fp32."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lib():
    from immtsf import _lib as L
    return L.load(), L.stream_ptr()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gain(d, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.3 * torch.randn(d, generator=g)).to(torch.bfloat16).to(dev)


def _rand(shape, dev, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def test_tokens():
    dev = _dev()
    lib, st = _lib()
    vocab, d = 50, 256
    table = _rand((vocab, d), dev, 1).to(torch.bfloat16)
    ids = torch.tensor([0, 49, 7, 7, 23, 49, 0, 31, 2], dtype=torch.int32, device=dev)
    got, want = torch.full((ids.numel(), d), -7.0, device=dev), torch.full((ids.numel(), d), -7.0, device=dev)
    assert lib.immtsf_llama_embed_tokens_p16(_p(ids), ids.numel(), _p(table), vocab, d, _p(got), st) == 0
    table32 = table.float()
    assert lib.immtsf_llama_embed_tokens(_p(ids), ids.numel(), _p(table32), vocab, d, _p(want), st) == 0
    assert torch.equal(got, want) and torch.equal(got, table32[ids.long()])


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("out_bf16", [False, True])
def test_rmsnorm_and_add_rmsnorm(rows, d, out_bf16):
    dev = _dev()
    lib, st = _lib()
    w16 = _gain(d, dev, d + rows)
    w32 = w16.float()
    x, y = _rand((rows, d), dev, 2), _rand((rows, d), dev, 3)
    dt = torch.bfloat16 if out_bf16 else torch.float32

    def outs():
        o = torch.zeros(rows, d, dtype=dt, device=dev)
        return o, ((None, _p(o)) if out_bf16 else (_p(o), None))

    a, pa = outs()
    b, pb = outs()
    assert lib.immtsf_llama_embed_rmsnorm_p16(_p(x), rows, d, _p(w16), EPS, *pa, st) == 0
    assert lib.immtsf_llama_embed_rmsnorm(_p(x), rows, d, _p(w32), EPS, *pb, st) == 0
    assert torch.equal(a, b) and bool(a.any())
    xa, xb = x.clone(), x.clone()
    a, pa = outs()
    b, pb = outs()
    assert lib.immtsf_llama_embed_add_rmsnorm_p16(_p(xa), _p(y), rows, d, _p(w16), EPS, *pa, st) == 0
    assert lib.immtsf_llama_embed_add_rmsnorm(_p(xb), _p(y), rows, d, _p(w32), EPS, *pb, st) == 0
    assert torch.equal(a, b) and torch.equal(xa, xb) and torch.equal(xa, x + y)


@pytest.mark.parametrize("with_y", [False, True])
def test_pool(with_y):
    dev = _dev()
    lib, st = _lib()
    counts, d = (0, 1, 33, 96), 256
    T, N = sum(counts), len(counts)
    cu = torch.tensor([0, 0, 1, 34, 130], dtype=torch.int32, device=dev)
    w16 = _gain(d, dev, 11)
    x, y = _rand((T, d), dev, 4), (_rand((T, d), dev, 5) if with_y else None)
    res = []
    for fn, w in ((lib.immtsf_llama_embed_pool_p16, w16), (lib.immtsf_llama_embed_pool, w16.float())):
        xc, rstd, pooled = x.clone(), torch.zeros(T, device=dev), torch.full((N, d), -7.0, device=dev)
        assert fn(_p(xc), _p(y), _p(cu), N, T, d, _p(w), EPS, _p(rstd), _p(pooled), st) == 0
        res.append((xc, rstd, pooled))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    pooled = res[0][2]
    assert not pooled[0].any() and bool(pooled[1:].any()) and bool(torch.isfinite(pooled).all())


@pytest.mark.parametrize("B,S_in,s_from", [(3, 42, 37), (1, 1, 0)])
@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("with_rstd", [False, True])
def test_body_rmsnorm_and_its_backward(B, S_in, s_from, with_y, with_rstd):
    dev = _dev()
    lib, st = _lib()
    d = 256
    n = B * (S_in - s_from)
    w16 = _gain(d, dev, 13 + S_in)
    xin = _rand((B * S_in, d), dev, 6)
    y = _rand((n, d), dev, 7) if with_y else None
    fwd = []
    for fn, w in ((lib.immtsf_llama_body_rmsnorm_p16, w16), (lib.immtsf_llama_body_rmsnorm, w16.float())):
        xo = torch.zeros(n, d, device=dev) if with_y else None
        o32, o16 = torch.zeros(n, d, device=dev), torch.zeros(n, d, dtype=torch.bfloat16, device=dev)
        rstd = torch.zeros(n, device=dev) if with_rstd else None
        assert fn(_p(xin), B, S_in, s_from, d, _p(y), _p(xo), _p(w), EPS, _p(o32), None, _p(rstd), st) == 0
        assert fn(_p(xin), B, S_in, s_from, d, _p(y), _p(xo), _p(w), EPS, None, _p(o16), _p(rstd), st) == 0
        fwd.append((xo, o32, o16, rstd))
    for a, b in zip(*fwd):
        assert (a is None and b is None) or torch.equal(a, b)
    assert bool(fwd[0][1].any()) and torch.equal(fwd[0][2], fwd[0][1].to(torch.bfloat16))
    # the backward over the same compact rows: dy, the rows' x and rstd; the residual gradient stands where y stood
    x = xin.view(B, S_in, d)[:, s_from:].reshape(n, d).contiguous()
    if with_y:
        x = x + y
    rstd = torch.rsqrt(x.pow(2).mean(-1) + EPS).contiguous()
    dy, resid = _rand((n, d), dev, 8), (_rand((n, d), dev, 9) if with_y else None)
    bwd = []
    for fn, w in ((lib.immtsf_llama_body_rmsnorm_backward_p16, w16), (lib.immtsf_llama_body_rmsnorm_backward, w16.float())):
        o32, o16 = torch.zeros(n, d, device=dev), torch.zeros(n, d, dtype=torch.bfloat16, device=dev)
        assert fn(_p(dy), _p(x), _p(rstd), _p(w), _p(resid), n, d, _p(o32), _p(o16), st) == 0
        bwd.append((o32, o16))
    for a, b in zip(*bwd):
        assert torch.equal(a, b)
    assert bool(bwd[0][0].any())
