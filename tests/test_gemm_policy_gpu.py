"""Which kernel gemm._linear / gemm._dgrad pick for a product, and how the row blocks of a shared
(3E, E) parameter get their weight / bias gradients, immediately and deferred.  The expected
launches follow the predicates and the *_supported functions (rowsgemm: N % 32, K % 64, K <= 1024,
M <= 2048; tilegemm: N % 128, K % 64, M > 2048; gemm256: N % 8, K % 8; rows256: 256 / 264 wide,
no bias, M >= GEMM256_MIN_M); results against the fp32 product of the same operands."""
import pytest
import torch

from helpers import ov3d  # noqa: F401
from test_rows_gemm_gpu import _check

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LONG = 4096   # GEMM256_MIN_M for the rows marked `long`: the routes of the longest row blocks


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, device=gen.device, generator=gen) * scale).to(BF)


def _census(fn):
    from ov3d_amd import _native
    _native.census_start()
    try:
        out = fn()
    finally:
        calls = _native.census_stop()
    return out, calls


# (M, N, K, extra, expected launches); extra: bias / strided / misaligned / float32 / long
LINEAR = [
    (64, 32, 64, "bias", {"ov3d_rows_gemm": 1}),
    (2048, 96, 192, "strided", {"ov3d_rows_gemm": 1}),
    (2049, 128, 64, "bias", {"ov3d_tile_gemm": 1}),
    (2049, 96, 64, "", {"ov3d_gemm256": 1}),
    (64, 32, 72, "", {"ov3d_gemm256": 1}),
    (64, 32, 2048, "", {"ov3d_gemm256": 1}),
    (64, 30, 64, "", {}),
    (64, 32, 64, "misaligned", {}),
    (64, 32, 64, "float32", {}),
    (LONG, 256, 256, "long", {"ov3d_rows256": 1}),
    (LONG, 256, 256, "long bias", {"ov3d_gemm256": 1}),
    (LONG, 128, 128, "long", {"ov3d_gemm256": 1}),
]


@pytest.mark.parametrize("M,N,K,extra,expected", LINEAR)
def test_linear_route(cuda, monkeypatch, M, N, K, extra, expected):
    from ov3d_amd import gemm
    if "long" in extra:
        monkeypatch.setattr(gemm, "GEMM256_MIN_M", LONG)
    gen = torch.Generator(device=cuda).manual_seed(M + N + K)
    if extra == "strided":
        x = _rand(gen, M, K + 64)[:, 32:32 + K]     # row stride K + 64
    elif extra == "misaligned":
        x = _rand(gen, M, K + 8)[:, 4:4 + K]        # base 8 bytes past a 16-byte boundary
        assert x.data_ptr() % 16 == 8
    else:
        x = _rand(gen, M, K)
    w = _rand(gen, N, K, scale=K ** -0.5)
    b = _rand(gen, N) if "bias" in extra else None
    if extra == "float32":
        x, w = x.float(), w.float()
    out, calls = _census(lambda: gemm._linear(x, w, b))
    assert calls == expected
    assert out.shape == (M, N) and out.dtype == x.dtype
    ref = x.float() @ w.float().t() + (b.float() if b is not None else 0)
    _check(out, ref, torch.nn.functional.linear(x, w, b))


DGRAD = [
    (64, 64, 32, False, {"ov3d_rows_gemm": 1}),
    (2049, 64, 128, False, {"ov3d_tile_gemm": 1}),
    (2049, 64, 96, False, {"ov3d_gemm256": 1}),
    (64, 72, 32, False, {}),     # no gemm256 route at M <= ROWS_GEMM_MAX_M: the library
    (LONG, 256, 256, True, {"ov3d_rows256": 1}),
    (LONG, 128, 128, True, {"ov3d_gemm256": 1}),
]


@pytest.mark.parametrize("M,N,K,long,expected", DGRAD)
def test_dgrad_route(cuda, monkeypatch, M, N, K, long, expected):
    from ov3d_amd import gemm
    if long:
        monkeypatch.setattr(gemm, "GEMM256_MIN_M", LONG)
    gen = torch.Generator(device=cuda).manual_seed(3 * M + N + K)
    dy = _rand(gen, M, N)
    w = _rand(gen, N, K, scale=N ** -0.5)
    out, calls = _census(lambda: gemm._dgrad(dy, w))
    assert calls == expected
    assert out.shape == (M, K) and out.dtype == BF
    _check(out, dy.float() @ w.float(), dy @ w)


def _relnorm(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("first", [1, 0])
def test_in_projection_row_blocks_immediate_and_deferred(cuda, first):
    """blocks first .. 2 of a (3E, E) in-projection: rows no block covers get exactly zero,
    every covered block is g^T x / sum g of its own bf16 rows, with gemm.DEFER_WGRAD off (one
    ov3d_wgrad launch per block) and on (one grouped launch at the end of the backward)"""
    from ov3d_amd import gemm
    E, R = 64, 300
    gen = torch.Generator(device=cuda).manual_seed(11 + first)
    blocks = list(range(first, 3))
    xs = [torch.randn(R, E, device=cuda, generator=gen) for _ in blocks]
    gs = [torch.randn(R, E, device=cuda, generator=gen) for _ in blocks]
    w0 = torch.randn(3 * E, E, device=cuda, generator=gen) / E ** 0.5
    b0 = torch.randn(3 * E, device=cuda, generator=gen)
    grads = {}
    for defer in (False, True):
        w, b = w0.clone().requires_grad_(), b0.clone().requires_grad_()
        gemm.DEFER_WGRAD = defer
        try:
            with torch.autocast("cuda", dtype=BF):
                ys = gemm.in_projection(w, b, [(x.clone().requires_grad_(), k * E, (k + 1) * E)
                                               for x, k in zip(xs, blocks)])
            loss = sum((y.float() * g).sum() for y, g in zip(ys, gs))
            _, calls = _census(loss.backward)
            assert not gemm._PENDING
        finally:
            gemm.DEFER_WGRAD = False
        if defer:
            assert calls.get("ov3d_wgrad_group") == 1 and "ov3d_wgrad" not in calls, calls
        else:
            assert calls.get("ov3d_wgrad") == len(blocks), calls
        assert torch.count_nonzero(w.grad[:first * E]) == 0
        assert torch.count_nonzero(b.grad[:first * E]) == 0
        for x, g, k in zip(xs, gs, blocks):
            gb, xb = g.to(BF).float(), x.to(BF).float()
            rows = slice(k * E, (k + 1) * E)
            assert _relnorm(w.grad[rows], gb.t() @ xb) <= 1e-5, (defer, k)
            assert _relnorm(b.grad[rows], gb.sum(0)) <= 1e-5, (defer, k)
        grads[defer] = (w.grad, b.grad)
    for a, ref in zip(grads[True], grads[False]):
        assert _relnorm(a, ref) <= 1e-4
