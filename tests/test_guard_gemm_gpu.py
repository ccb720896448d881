"""Guard-band cases of the GEMM families (tests/guard.py: G1 no stray writes, G2 no dependence
on memory outside the inputs, G3 fully written, G4 the family's own value bar, G5 workspaces
of exactly the reported size, G6 rejections write nothing) at the smallest ragged shapes of
each tile: csrc/tilegemm.hip (BN 128, BK 64), rowsgemm.hip (32-column tiles, K % 64),
gemm256.hip (256 x 256, BK 64), rows256.hip (TM 128) and wgrad.hip (128 / 256 tiles, 32- and
64-row stages).  Every operand has a row stride 8 elements past its width and a base that is
16-byte aligned and no more."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_gemm256_gpu import _check as check256
from test_tile_gemm_gpu import _check as check_lib

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ENTRIES = ("ov3d_tile_gemm", "ov3d_tile_gemm_act", "ov3d_tile_gemm2", "ov3d_tile_gemm_batched",
           "ov3d_rows_gemm", "ov3d_rows_gemm_act", "ov3d_rows_gemm_group", "ov3d_gemm256",
           "ov3d_gemm256_pair", "ov3d_gemm256_batched", "ov3d_conv3x3_gemm256", "ov3d_rows256",
           "ov3d_rows256_bn", "ov3d_wgrad", "ov3d_wgrad_bn", "ov3d_wgrad_group")


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _bf(g, *shape, s=1.0):
    return (torch.randn(*shape, generator=g) * s).to(BF)


def _seed():
    """the dropout seed word: an in-range value in the interior and in both bands"""
    return In(torch.tensor([20241], dtype=torch.int64), index=(3, 5))


# ---------------------------------------------------------------- tilegemm / rowsgemm

def _linear_case(cuda, entry, M, N, K, mode):
    """plain product, `mode` nt-bias / nt (trans_b = 1) / nn (trans_b = 0)"""
    trans_b = mode != "nn"
    g = _gen(M, N, K, len(mode))
    a = _bf(g, M, K)
    w = _bf(g, *((N, K) if trans_b else (K, N)), s=K ** -0.5)
    b = _bf(g, N) if mode == "nt-bias" else None
    lda, ldw, ldc = K + 8, w.shape[1] + 8, N + 8
    specs = {"A": In(a, ld=lda), "W": In(w, ld=ldw), "bias": In(b) if b is not None else None,
             "C": Out((M, N), BF, ld=ldc)}

    def call(t):
        guard.call(entry, M, N, K, t["A"], lda, t["W"], ldw, int(trans_b), t["bias"], t["C"], ldc,
                   like=t["A"])
    out = guard.run_case(cuda, specs, call)["C"]
    ad, wd = a.to(cuda), w.to(cuda)
    bd = b.to(cuda) if b is not None else None
    if trans_b:
        ref, lib = ad.float() @ wd.float().t() + (bd.float() if b is not None else 0), F.linear(ad, wd, bd)
    else:
        ref, lib = ad.float() @ wd.float(), ad @ wd
    check_lib(out, ref, lib)


def _act_case(cuda, entry, plain, M, N, K, epi, p):
    """the FFN epilogues: bit-equal to the plain product followed by the row kernel (the bar of
    test_tile_gemm_ffn_epilogues_match_row_kernels / test_fused_ffn_equals_unfused_bitwise)"""
    g = _gen(M, N, K, epi, int(p * 10))
    a = _bf(g, M, K)
    lda, ldc, ldh = K + 8, N + 8, N + 8
    site = 1234
    if epi == 1:
        w, b, trans_b, h = _bf(g, N, K, s=K ** -0.5), _bf(g, N), 1, None
    else:
        w, b, trans_b = _bf(g, K, N, s=K ** -0.5), None, 0
        h = torch.relu(_bf(g, M, N))                    # the activation output: about half zeros
    ldw = w.shape[1] + 8
    specs = {"A": In(a, ld=lda), "W": In(w, ld=ldw), "bias": In(b) if b is not None else None,
             "seed": _seed() if epi == 1 and p > 0 else None,
             "H": In(h, ld=ldh) if h is not None else None, "C": Out((M, N), BF, ld=ldc)}

    def call(t):
        guard.call(entry, M, N, K, t["A"], lda, t["W"], ldw, trans_b, t["bias"], epi, float(p),
                   t["seed"], site, t["H"], ldh if h is not None else 0, t["C"], ldc, like=t["A"])
    out = guard.run_case(cuda, specs, call)["C"]
    ad, wd = a.to(cuda), w.to(cuda)
    y = torch.empty((M, N), dtype=BF, device=cuda)
    guard.call(plain, M, N, K, ad, K, wd, wd.shape[1], trans_b, b.to(cuda) if b is not None else None,
               y, N, like=ad)
    ref = torch.empty_like(y)
    if epi == 1:
        seed = torch.tensor([20241], dtype=torch.int64, device=cuda) if p > 0 else None
        guard.call("ov3d_relu_dropout_fwd", y, M, N, float(p), seed, site, ref, like=y)
    else:
        guard.call("ov3d_relu_dropout_bwd", h.to(cuda), y, M * N, float(p), ref, like=y)
    assert torch.equal(out, ref)


TILE_M = [1, 127, 129, 300]
TILE_NK = [(128, 64), (256, 192)]


@pytest.mark.parametrize("mode", ["nt-bias", "nt", "nn"])
@pytest.mark.parametrize("N,K", TILE_NK)
@pytest.mark.parametrize("M", TILE_M)
def test_tile_gemm(cuda, M, N, K, mode):
    _linear_case(cuda, "ov3d_tile_gemm", M, N, K, mode)


@pytest.mark.parametrize("epi,p", [(1, 0.0), (1, 0.1), (2, 0.0), (2, 0.1)])
@pytest.mark.parametrize("N,K", TILE_NK)
@pytest.mark.parametrize("M", TILE_M)
def test_tile_gemm_act(cuda, M, N, K, epi, p):
    _act_case(cuda, "ov3d_tile_gemm_act", "ov3d_tile_gemm", M, N, K, epi, p)


def test_tile_gemm2(cuda):
    M, N, K1, K2 = 129, 128, 64, 128
    g = _gen(M, N, K1, K2)
    a1, a2 = _bf(g, M, K1), _bf(g, M, K2)
    w1, w2 = _bf(g, K1, N, s=K1 ** -0.5), _bf(g, K2, N, s=K2 ** -0.5)
    lda, ldw, ldc = K2 + 8, N + 8, N + 8                # lda2 == lda1, ldw2 == ldw1
    specs = {"A1": In(a1, ld=lda), "A2": In(a2, ld=lda), "W1": In(w1, ld=ldw), "W2": In(w2, ld=ldw),
             "C": Out((M, N), BF, ld=ldc)}

    def call(t):
        guard.call("ov3d_tile_gemm2", M, N, K1, t["A1"], lda, t["W1"], ldw, K2, t["A2"], lda,
                   t["W2"], ldw, 0, t["C"], ldc, like=t["A1"])
    out = guard.run_case(cuda, specs, call)["C"]
    a1, a2, w1, w2 = (x.to(cuda) for x in (a1, a2, w1, w2))
    check_lib(out, a1.float() @ w1.float() + a2.float() @ w2.float(), (a1 @ w1).addmm_(a2, w2))


@pytest.mark.parametrize("trans_b", [1, 0])
def test_tile_gemm_batched(cuda, trans_b):
    """3 problems whose batch strides skip a row of A and of C (the skipped C rows stay sentinel)"""
    nb, M, N, K = 3, 129, 128, 64
    g = _gen(nb, M, N, K, trans_b)
    a = _bf(g, nb, M + 1, K)
    w = _bf(g, nb, *((N, K) if trans_b else (K, N)), s=K ** -0.5)
    lda, ldw, ldc = K + 8, w.shape[2] + 8, N + 8
    written = torch.ones(nb, M + 1, N, dtype=torch.bool)
    written[:, M] = False
    specs = {"A": In(a, ld=lda), "W": In(w, ld=ldw), "C": Out((nb, M + 1, N), BF, ld=ldc, full=written)}

    def call(t):
        guard.call("ov3d_tile_gemm_batched", nb, M, N, K, t["A"], lda, (M + 1) * lda, t["W"], ldw,
                   w.shape[1] * ldw, trans_b, t["C"], ldc, (M + 1) * ldc, like=t["A"])
    out = guard.run_case(cuda, specs, call)["C"][:, :M]
    ad, wd = a.to(cuda)[:, :M], w.to(cuda)
    wt = wd.transpose(1, 2) if trans_b else wd
    check_lib(out, torch.bmm(ad.float(), wt.float()), torch.bmm(ad, wt))


ROWS_M = [1, 17, 33, 100]
ROWS_NK = [(32, 64), (96, 1024)]


@pytest.mark.parametrize("mode", ["nt-bias", "nt", "nn"])
@pytest.mark.parametrize("N,K", ROWS_NK)
@pytest.mark.parametrize("M", ROWS_M)
def test_rows_gemm(cuda, M, N, K, mode):
    _linear_case(cuda, "ov3d_rows_gemm", M, N, K, mode)


@pytest.mark.parametrize("epi,p", [(1, 0.0), (1, 0.1), (2, 0.0), (2, 0.1)])
@pytest.mark.parametrize("N,K", ROWS_NK)
@pytest.mark.parametrize("M", ROWS_M)
def test_rows_gemm_act(cuda, M, N, K, epi, p):
    _act_case(cuda, "ov3d_rows_gemm_act", "ov3d_rows_gemm", M, N, K, epi, p)


@pytest.mark.parametrize("trans_b", [1, 0])
def test_rows_gemm_group(cuda, trans_b):
    """3 problems of different N and K over the same 33 rows: each equals its single launch bit
    for bit (test_rows_gemm_group_equals_single_launches)"""
    from ov3d_amd import _native
    M, shapes = 33, [(32, 64), (96, 128), (64, 1024)]
    g = _gen(M, trans_b, 3)
    specs, data = {}, []
    for i, (N, K) in enumerate(shapes):
        a = _bf(g, M, K)
        w = _bf(g, *((N, K) if trans_b else (K, N)), s=K ** -0.5)
        b = _bf(g, N) if trans_b else None
        data.append((a, w, b))
        specs.update({f"A{i}": In(a, ld=K + 8), f"W{i}": In(w, ld=w.shape[1] + 8),
                      f"b{i}": In(b) if b is not None else None, f"C{i}": Out((M, N), BF, ld=N + 4)})
    P = _native.struct("ov3d_rows_gemm_problem")

    def call(t):
        arr = (P * 3)(*[P(t[f"A{i}"].data_ptr(), K + 8, t[f"W{i}"].data_ptr(), data[i][1].shape[1] + 8,
                          t[f"b{i}"].data_ptr() if trans_b else None, t[f"C{i}"].data_ptr(), N + 4, N, K)
                        for i, (N, K) in enumerate(shapes)])
        guard.call("ov3d_rows_gemm_group", M, 3, ctypes.addressof(arr), trans_b, like=t["A0"])
    out = guard.run_case(cuda, specs, call)
    for i, (N, K) in enumerate(shapes):
        a, w, b = (x.to(cuda) if x is not None else None for x in data[i])
        single = torch.empty((M, N), dtype=BF, device=cuda)
        guard.call("ov3d_rows_gemm", M, N, K, a, K, w, w.shape[1], trans_b, b, single, N, like=a)
        assert torch.equal(out[f"C{i}"], single), i
        wt = w.float().t() if trans_b else w.float()
        check_lib(single, a.float() @ wt + (b.float() if b is not None else 0),
                  F.linear(a, w, b) if trans_b else a @ w)


# ---------------------------------------------------------------- gemm256

def _ref256(a, w, b, r, relu):
    ref = a.float() @ w.float().t()
    lib = F.linear(a, w, b.to(BF) if b is not None else None)
    if b is not None:
        ref = ref + b.float()
    if r is not None:
        ref, lib = ref + r.float(), lib + r
    if relu:
        ref, lib = ref.clamp_min(0), lib.clamp_min(0)
    return ref, lib


@pytest.mark.parametrize("bias,res,relu", [(None, False, False), ("bf16", True, True),
                                           ("f32", False, True)])
@pytest.mark.parametrize("K", [8, 72, 264])
@pytest.mark.parametrize("N", [8, 264])
@pytest.mark.parametrize("M", [1, 255, 257])
def test_gemm256(cuda, M, N, K, bias, res, relu):
    g = _gen(M, N, K, relu, res)
    a, w = _bf(g, M, K), _bf(g, N, K, s=K ** -0.5)
    b = None if bias is None else (_bf(g, N) if bias == "bf16" else torch.randn(N, generator=g))
    r = _bf(g, M, N) if res else None
    lda, ldb, ldr, ldc = K + 8, K + 8, N + 8, N + 8
    specs = {"A": In(a, ld=lda), "B": In(w, ld=ldb), "bias": In(b) if b is not None else None,
             "R": In(r, ld=ldr) if res else None, "C": Out((M, N), BF, ld=ldc)}

    def call(t):
        guard.call("ov3d_gemm256", t["A"], lda, t["B"], ldb, t["bias"], int(bias == "f32"), t["R"],
                   ldr if res else 0, t["C"], ldc, M, N, K, int(relu), like=t["A"])
    out = guard.run_case(cuda, specs, call)["C"]
    ref, lib = _ref256(a.to(cuda), w.to(cuda), b.to(cuda) if b is not None else None,
                       r.to(cuda) if res else None, relu)
    check256(out, ref, lib)


def test_gemm256_pair(cuda):
    M, N, K = 257, 264, 72
    g = _gen(M, N, K, 2)
    a1, a2, w1, w2 = _bf(g, M, K), _bf(g, M, K), _bf(g, N, K, s=K ** -0.5), _bf(g, N, K, s=K ** -0.5)
    b1, b2 = _bf(g, N), _bf(g, N)
    lda, ldb, ldc = K + 8, K + 8, N + 8
    specs = {"A": In(a1, ld=lda), "A2": In(a2, ld=lda), "B": In(w1, ld=ldb), "B2": In(w2, ld=ldb),
             "b": In(b1), "b2": In(b2), "C": Out((M, N), BF, ld=ldc), "C2": Out((M, N), BF, ld=ldc)}

    def call(t):
        guard.call("ov3d_gemm256_pair", t["A"], t["A2"], lda, t["B"], t["B2"], ldb, t["b"], t["b2"], 0,
                   t["C"], t["C2"], ldc, M, N, K, like=t["A"])
    out = guard.run_case(cuda, specs, call)
    for o, a, w, b in ((out["C"], a1, w1, b1), (out["C2"], a2, w2, b2)):
        check256(o, *_ref256(a.to(cuda), w.to(cuda), b.to(cuda), None, False))


def test_gemm256_batched(cuda):
    """3 problems; A and C batch strides skip a row, the f32 bias rows are 4 elements apart"""
    nb, M, N, K = 3, 129, 40, 72
    g = _gen(nb, M, N, K)
    a, w, b = _bf(g, nb, M + 1, K), _bf(g, nb, N, K, s=K ** -0.5), torch.randn(nb, N, generator=g)
    lda, ldb, ldc, sbias = K + 8, K + 8, N + 8, N + 4
    written = torch.ones(nb, M + 1, N, dtype=torch.bool)
    written[:, M] = False
    specs = {"A": In(a, ld=lda), "B": In(w, ld=ldb), "bias": In(b, ld=sbias),
             "C": Out((nb, M + 1, N), BF, ld=ldc, full=written)}

    def call(t):
        guard.call("ov3d_gemm256_batched", t["A"], lda, (M + 1) * lda, t["B"], ldb, N * ldb, t["bias"],
                   sbias, 1, t["C"], ldc, (M + 1) * ldc, M, N, K, nb, 1, like=t["A"])
    out = guard.run_case(cuda, specs, call)["C"]
    for p in range(nb):
        check256(out[p, :M], *_ref256(a[p, :M].to(cuda), w[p].to(cuda), b[p].to(cuda), None, True))


@pytest.mark.parametrize("res", [False, True])
def test_conv3x3_gemm256(cuda, res):
    n, H, W, Cin, cout = 2, 3, 5, 64, 8
    g = _gen(n, H, W, Cin, cout, res)
    x = _bf(g, n, H, W, Cin)
    wt = _bf(g, cout, 3, 3, Cin, s=(9 * Cin) ** -0.5)
    b = _bf(g, cout)
    r = _bf(g, n * H * W, cout) if res else None
    ldb, ldr, ldc = 9 * Cin + 8, cout + 8, cout + 8
    specs = {"X": In(x.reshape(n * H * W, Cin)), "Wt": In(wt.reshape(cout, 9 * Cin), ld=ldb),
             "bias": In(b), "R": In(r, ld=ldr) if res else None, "Y": Out((n * H * W, cout), BF, ld=ldc)}

    def call(t):
        guard.call("ov3d_conv3x3_gemm256", t["X"], n, H, W, Cin, t["Wt"], ldb, t["bias"], 0, t["R"],
                   ldr if res else 0, t["Y"], ldc, cout, 1, like=t["X"])
    out = guard.run_case(cuda, specs, call)["Y"]
    ref = F.conv2d(x.to(cuda).permute(0, 3, 1, 2).float(), wt.to(cuda).permute(0, 3, 1, 2).float(),
                   b.to(cuda).float(), padding=1).permute(0, 2, 3, 1).reshape(n * H * W, cout)
    if res:
        ref = ref + r.to(cuda).float()
    check256(out, ref.clamp_min(0))


# ---------------------------------------------------------------- rows256

def _counters():
    return Out((2,), torch.int32, init=torch.zeros(2, dtype=torch.int32), full=False)


@pytest.mark.parametrize("K,N", [(256, 256), (264, 256), (256, 264)])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_rows256(cuda, M, K, N):
    """equals ov3d_gemm256 on the same operands bit for bit (test_rows256_equals_gemm256_bitwise);
    the claim counters are zero again after the launch"""
    from ov3d_amd import gemm
    g = _gen(M, K, N)
    x, w = _bf(g, M, K), _bf(g, N, K, s=0.06)
    ldx, ldw, ldy = K + 8, K + 8, N + 8
    specs = {"X": In(x, ld=ldx), "W": In(w, ld=ldw), "Y": Out((M, N), BF, ld=ldy), "counters": _counters()}

    def call(t):
        guard.call("ov3d_rows256", t["X"], ldx, K, N, t["W"], ldw, t["Y"], ldy, M, t["counters"],
                   like=t["X"])
    out = guard.run_case(cuda, specs, call)
    assert not bool(out["counters"].any())
    xd, wd = x.to(cuda), w.to(cuda)
    assert torch.equal(out["Y"], gemm.gemm256(xd, wd))
    check256(out["Y"], xd.float() @ wd.float().t())


def _bn_rows(x, scale, shift):
    """bf16(relu(x * scale + shift)) by ov3d_rows_bn_apply (no dropout), the arithmetic the
    fused entries are pinned to"""
    R, C = x.shape
    z = torch.empty_like(x)
    guard.call("ov3d_rows_bn_apply", x, 1, C, 0, C, R, C, scale, shift, 0.0, None, 0, z, C, 0, C, like=x)
    return z


@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_rows256_bn(cuda, M, with_z):
    from ov3d_amd import gemm
    g = _gen(M, with_z, 256)
    x, w = _bf(g, M, 256), _bf(g, 256, 256, s=0.06)
    scale, shift = torch.randn(256, generator=g), torch.randn(256, generator=g)
    ldx, ldw, ldy, ldz = 264, 264, 264, 264
    specs = {"X": In(x, ld=ldx), "W": In(w, ld=ldw), "scale": In(scale), "shift": In(shift),
             "Y": Out((M, 256), BF, ld=ldy), "Z": Out((M, 256), BF, ld=ldz) if with_z else None,
             "counters": _counters()}

    def call(t):
        guard.call("ov3d_rows256_bn", t["X"], ldx, t["scale"], t["shift"], t["W"], ldw, t["Y"], ldy,
                   t["Z"], ldz if with_z else 0, M, t["counters"], like=t["X"])
    out = guard.run_case(cuda, specs, call)
    assert not bool(out["counters"].any())
    z = _bn_rows(x.to(cuda), scale.to(cuda), shift.to(cuda))
    if with_z:
        assert torch.equal(out["Z"], z)
    assert torch.equal(out["Y"], gemm.gemm256(z, w.to(cuda)))


# ---------------------------------------------------------------- wgrad

def _wgrad_err(got, ref):
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("nsplit,bias", [(1, True), (4, False), (4, True)])
@pytest.mark.parametrize("N,K", [(16, 24), (128, 128), (136, 264)])
@pytest.mark.parametrize("R", [1, 31, 33, 65, 130])
def test_wgrad(cuda, R, N, K, nsplit, bias, bn):
    """dW = dy^T x and db = column sums within 1e-5 relative (summation order only,
    test_wgrad_gpu.py's bound); the workspace has exactly ov3d_wgrad_workspace floats (G5)"""
    from ov3d_amd import _native
    g = _gen(R, N, K, nsplit, bias, bn)
    dy, x = _bf(g, R, N), _bf(g, R, K)
    scale, shift = torch.randn(K, generator=g), torch.randn(K, generator=g)
    ldy, ldx, ldw = N + 8, K + 8, K + 8
    nws = _native.load().ov3d_wgrad_workspace(R, N, K, nsplit)
    assert nws == (0 if nsplit == 1 else nsplit * (N * K + N))
    specs = {"dy": In(dy, ld=ldy), "x": In(x, ld=ldx), "dW": Out((N, K), torch.float32, ld=ldw),
             "db": Out((N,), torch.float32) if bias else None,
             "ws": Out((nws,), torch.float32, full=False, compare=False, finite=False) if nws else None,
             "scale": In(scale) if bn else None, "shift": In(shift) if bn else None}

    def call(t):
        if bn:
            guard.call("ov3d_wgrad_bn", t["dy"], ldy, t["x"], ldx, R, N, K, t["scale"], t["shift"],
                       t["dW"], ldw, t["db"], t["ws"], None, nsplit, like=t["dy"])
        else:
            guard.call("ov3d_wgrad", t["dy"], ldy, t["x"], ldx, R, N, K, t["dW"], ldw, t["db"], t["ws"],
                       None, nsplit, like=t["dy"])
    out = guard.run_case(cuda, specs, call)
    dyd, xd = dy.to(cuda), x.to(cuda)
    if bn:
        xd = _bn_rows(xd, scale.to(cuda), shift.to(cuda))
    assert _wgrad_err(out["dW"], dyd.float().t() @ xd.float()) < 1e-5
    if bias:
        assert _wgrad_err(out["db"], dyd.float().sum(0)) < 1e-5


def test_wgrad_group(cuda):
    """3 problems mixing the shapes above in one stream-K launch; dW and db banded, the
    workspace exactly ov3d_wgrad_group_workspace floats"""
    from ov3d_amd import _native
    shapes = [(33, 16, 24, True), (130, 136, 264, True), (65, 128, 128, False)]
    g = _gen(3, 33, 130, 65)
    data = [(_bf(g, R, N), _bf(g, R, K)) for R, N, K, _ in shapes]
    P = _native.struct("ov3d_wgrad_problem")

    def table(ptr):
        return (P * 3)(*[P(ptr(f"dy{i}"), N + 8, ptr(f"x{i}"), K + 8, R, N, K, 1, ptr(f"dW{i}"), K + 8,
                           ptr(f"db{i}") if b else None) for i, (R, N, K, b) in enumerate(shapes)])
    # the size function never dereferences the operands: size the workspace from placeholder
    # pointers of the bands' alignment, and check it again with the real ones in the call
    sizing = table(lambda name: 512 + 16)
    nws = _native.load().ov3d_wgrad_group_workspace(ctypes.addressof(sizing), 3)
    assert nws > 0
    specs = {"ws": Out((nws,), torch.float32, full=False, compare=False, finite=False)}
    for i, (R, N, K, b) in enumerate(shapes):
        specs.update({f"dy{i}": In(data[i][0], ld=N + 8), f"x{i}": In(data[i][1], ld=K + 8),
                      f"dW{i}": Out((N, K), torch.float32, ld=K + 8),
                      f"db{i}": Out((N,), torch.float32) if b else None})

    def call(t):
        arr = table(lambda name: t[name].data_ptr())
        assert _native.load().ov3d_wgrad_group_workspace(ctypes.addressof(arr), 3) == nws
        guard.call("ov3d_wgrad_group", ctypes.addressof(arr), 3, t["ws"], like=t["ws"])
    out = guard.run_case(cuda, specs, call)
    for i, (R, N, K, b) in enumerate(shapes):
        dyd, xd = data[i][0].to(cuda), data[i][1].to(cuda)
        assert _wgrad_err(out[f"dW{i}"], dyd.float().t() @ xd.float()) <= 1e-5, i
        if b:
            assert _wgrad_err(out[f"db{i}"], dyd.float().sum(0)) <= 1e-5, i
