"""Guard-band cases of the row kernels (csrc/resnorm.hip, lngemm.hip, encpost.hip, bnrows.hip,
pool.hip, headsout.hip and the small reductions) at the smallest ragged row counts, every
operand between guard bands (tests/guard.py).  Values: the family's own references and bars
(restated or imported from its test file); where a family has no unit test of its raw entry,
the bound is derived in the case from the number formats involved."""
import ctypes

import pytest
import torch

import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_resnorm_gpu import row_keep

pytestmark = pytest.mark.gpu

BF, F32, F64, I32, U8 = torch.bfloat16, torch.float32, torch.float64, torch.int32, torch.uint8
ENTRIES = ("ov3d_relu_dropout_fwd", "ov3d_relu_dropout_bwd", "ov3d_add_cast_bf16", "ov3d_colsum_f32",
           "ov3d_colsum_group", "ov3d_reduce_partials", "ov3d_reduce_partials_f32", "ov3d_nbr_max_fwd",
           "ov3d_nbr_max_bwd", "ov3d_nbr_max_bnrelu_fwd", "ov3d_rows_bn_stats", "ov3d_rows_bn_apply",
           "ov3d_rows_bn_bwd", "ov3d_rows_bn_bwd_pooled", "ov3d_resnorm_fwd", "ov3d_resnorm_bwd",
           "ov3d_lngemm_fwd", "ov3d_lngemm_bwd", "ov3d_enc_post_fwd", "ov3d_enc_post_bwd",
           "ov3d_heads_out_fwd", "ov3d_heads_out_bwd")
SEED, SITE = 20241, 11
EINVAL = -1


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 32452843 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _seed():
    return In(torch.tensor([SEED], dtype=torch.int64), index=(3, 5))


def _lib():
    from ov3d_amd import _native
    return _native.load()


def _one_bf16_rounding(out, ref):
    """|out - ref| within one bf16 rounding of the fp32 reference (2^-8 relative: the format's
    half-ulp bound is 2^-9; one more for an fp32 operation order that differs), plus a float
    epsilon of the scale"""
    d = (out.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-6 * ref.abs().max().clamp_min(1e-30)
    assert int((d > bound).sum()) == 0, (d.max().item(), ref.abs().max().item())


# ---------------------------------------------------------------- element-wise rows

@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R", [1, 7, 1003])
def test_relu_dropout_fwd(cuda, R, p):
    """h = dropout(relu(y)) over (R, 8) rows, exact against the documented hash
    (test_relu_dropout_matches_torch)"""
    C = 8
    y = torch.randn(R, C, generator=_gen(R, int(p * 10))).to(BF)
    specs = {"y": In(y), "seed": _seed() if p > 0 else None, "h": Out((R, C), BF)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_relu_dropout_fwd", t["y"], R, C, float(p), t["seed"], SITE, t["h"], like=t["y"]))["h"]
    a = torch.relu(y.to(cuda).float())
    keep = row_keep(SEED, SITE, R, C, p, cuda)
    ref = torch.where(keep, (a * (1 / (1 - p))).bfloat16().float(), torch.zeros_like(a)) if p > 0 \
        else a.bfloat16().float()
    assert torch.equal(out.float(), ref)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 1003])
def test_relu_dropout_bwd(cuda, n, p):
    """dy = dh / (1 - p) where h > 0; n % 8 != 0 is rejected and writes nothing (G6), the nearest
    accepted lengths 8 and 1000 run"""
    g = _gen(n, int(p * 10))
    h, dh = torch.relu(torch.randn(n, generator=g)).to(BF), torch.randn(n, generator=g).to(BF)
    specs = {"h": In(h), "dh": In(dh), "dy": Out((n,), BF)}
    if n % 8:
        rc = guard.run_case(cuda, specs, lambda t: guard.raw_call(
            "ov3d_relu_dropout_bwd", t["h"], t["dh"], n, float(p), t["dy"], like=t["h"]), expect_reject=True)
        assert rc == (EINVAL, EINVAL)
        return
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_relu_dropout_bwd", t["h"], t["dh"], n, float(p), t["dy"], like=t["h"]))["dy"]
    ref = torch.where(h.float() > 0, dh.float() * (1 / (1 - p)), torch.zeros(n)).bfloat16()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("a_bf16", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 1003])
def test_add_cast_bf16(cuda, n, a_bf16):
    """sum = bf16(a + b) in fp32, ac = bf16(a) (fp32 a only), bit for bit
    (test_add_cast_bf16_equals_torch); n % 8 != 0 is rejected and writes nothing"""
    g = _gen(n, a_bf16)
    a, b = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    if a_bf16:
        a = a.to(BF)
    specs = {"a": In(a), "b": In(b), "sum": Out((n,), BF), "ac": None if a_bf16 else Out((n,), BF)}
    if n % 8:
        rc = guard.run_case(cuda, specs, lambda t: guard.raw_call(
            "ov3d_add_cast_bf16", t["a"], a_bf16, t["b"], n, t["sum"], t["ac"], like=t["a"]),
            expect_reject=True)
        assert rc == (EINVAL, EINVAL)
        return
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_add_cast_bf16", t["a"], a_bf16, t["b"], n, t["sum"], t["ac"], like=t["a"]))
    assert torch.equal(out["sum"].cpu(), (a.float() + b).to(BF))
    if not a_bf16:
        assert torch.equal(out["ac"].cpu(), a.to(BF))


# ---------------------------------------------------------------- small reductions

@pytest.mark.parametrize("width", [1, 7, 1003])
@pytest.mark.parametrize("nparts", [1, 7, 1003])
def test_colsum_f32(cuda, nparts, width):
    """column sums of (nparts, width) fp32 partials in a fixed order: part.sum(0) up to the
    summation order (test_colsum_f32_equals_torch_sum's bound)"""
    part = torch.randn(nparts, width, generator=_gen(nparts, width))
    specs = {"parts": In(part), "out": Out((width,), F32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_colsum_f32", t["parts"], nparts, width, t["out"], like=t["parts"]))["out"]
    torch.testing.assert_close(out.cpu(), part.double().sum(0).float(), rtol=1e-5,
                               atol=1e-5 * nparts ** 0.5)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("width", [1, 7, 1003])
@pytest.mark.parametrize("nparts", [1, 7, 1003])
def test_reduce_partials(cuda, nparts, width, f32):
    """(nparts, width) fp64 partials -> fp64 sums (summation order only: 1e-12 of the absolute
    sum, fp64's 2^-53 times the term count with room), or those sums rounded once to fp32"""
    part = torch.randn(nparts, width, generator=_gen(nparts, width, 1), dtype=F64)
    specs = {"parts": In(part), "tot": Out((width,), F32 if f32 else F64)}
    entry = "ov3d_reduce_partials_f32" if f32 else "ov3d_reduce_partials"
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        entry, t["parts"], nparts, width, t["tot"], like=t["parts"]))["tot"].cpu()
    ref, mag = part.sum(0), part.abs().sum(0)
    if f32:
        assert bool(((out.double() - ref).abs() <= mag * 2.0 ** -23).all())
    else:
        assert bool(((out - ref).abs() <= mag * 1e-12).all())


@pytest.mark.parametrize("nparts", [1, 7, 1003])
def test_colsum_group(cuda, nparts):
    """two outputs over three segments of (nparts, 4, C) resnorm partials: each output the
    ordered sum of its segments' column totals (fp32 summation order: colsum_f32's bound)"""
    from ov3d_amd import _native
    C = 64
    g = _gen(nparts, C)
    parts = [torch.randn(n, 4, C, generator=g) for n in (nparts, 3, nparts)]
    ks = (0, 3, 1)
    specs = {f"p{i}": In(p.view(-1, C)) for i, p in enumerate(parts)}
    specs.update({"d0": Out((C,), F32), "d1": Out((C,), F32)})
    Seg, Dst = _native.struct("ov3d_colsum_seg"), _native.struct("ov3d_colsum_out")

    def call(t):
        segs = (Seg * 3)(*[Seg(t[f"p{i}"].data_ptr(), parts[i].shape[0], ks[i]) for i in range(3)])
        outs = (Dst * 2)(Dst(t["d0"].data_ptr(), 0, 2), Dst(t["d1"].data_ptr(), 2, 1))
        guard.call("ov3d_colsum_group", ctypes.addressof(segs), 3, ctypes.addressof(outs), 2, C,
                   like=t["d0"])
    out = guard.run_case(cuda, specs, call)
    tot = [p[:, k].double().sum(0) for p, k in zip(parts, ks)]
    atol = 1e-5 * (2 * nparts + 3) ** 0.5
    torch.testing.assert_close(out["d0"].cpu(), (tot[0] + tot[1]).float(), rtol=1e-5, atol=atol)
    torch.testing.assert_close(out["d1"].cpu(), tot[2].float(), rtol=1e-5, atol=atol)


# ---------------------------------------------------------------- neighbour max pool

def _pool_ref(z, P, S, C):
    """max over the S rows of each centroid and the FIRST row holding it"""
    v = z.view(P, S, C)
    m = v.max(1).values
    first = (v == m[:, None]).to(torch.uint8).argmax(1).to(U8)
    return m, first


@pytest.mark.parametrize("bnrelu", [False, True])
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("S", [1, 5, 64, 256])
@pytest.mark.parametrize("P", [1, 3])
def test_nbr_max_fwd(cuda, P, S, C, bnrelu):
    """out (P, C) and arg (P, C) exact; with BN + ReLU fused, of z = bf16(relu(y * scale + shift))
    as ov3d_rows_bn_apply writes it (test_bn_relu_pool_equals_two_passes: bit for bit)"""
    g = _gen(P, S, C, bnrelu)
    y = torch.randn(P * S, C, generator=g).to(BF)
    y[0] = y[S - 1]                                      # a tie: the first row wins
    scale, shift = torch.randn(C, generator=g), torch.randn(C, generator=g)
    specs = {"y": In(y), "scale": In(scale) if bnrelu else None, "shift": In(shift) if bnrelu else None,
             "out": Out((P, C), BF),
             # a row index of 0x5A is a value, not a leftover sentinel: G3 on arg only where no
             # row has that index (the exact comparison below covers the rest)
             "arg": Out((P, C), U8, full=S <= 0x5A)}

    def call(t):
        if bnrelu:
            guard.call("ov3d_nbr_max_bnrelu_fwd", t["y"], P, S, C, t["scale"], t["shift"], t["out"],
                       t["arg"], like=t["y"])
        else:
            guard.call("ov3d_nbr_max_fwd", t["y"], P, S, C, t["out"], t["arg"], like=t["y"])
    out = guard.run_case(cuda, specs, call)
    z = y.to(cuda)
    if bnrelu:
        zz = torch.empty_like(z)
        guard.call("ov3d_rows_bn_apply", z, 1, C, 0, C, P * S, C, scale.to(cuda), shift.to(cuda), 0.0,
                   None, 0, zz, C, 0, C, like=z)
        z = zz
    m, first = _pool_ref(z, P, S, C)
    assert torch.equal(out["out"], m) and torch.equal(out["arg"], first)


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("S", [1, 5, 64, 256])
@pytest.mark.parametrize("P", [1, 3])
def test_nbr_max_bwd(cuda, P, S, C):
    """dy (P*S, C): g on the arg rows, zero elsewhere, every element written"""
    g = _gen(P, S, C, 7)
    gr = torch.randn(P, C, generator=g).to(BF)
    arg = torch.randint(0, S, (P, C), generator=g).to(U8)
    specs = {"g": In(gr), "arg": In(arg, index=(0, S - 1)), "dy": Out((P * S, C), BF)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_nbr_max_bwd", t["g"], t["arg"], P, S, C, t["dy"], like=t["g"]))["dy"]
    ref = torch.zeros(P, S, C, dtype=BF)
    ref.scatter_(1, arg.long()[:, None], gr[:, None])
    assert torch.equal(out.cpu(), ref.view(P * S, C))


# ---------------------------------------------------------------- BatchNorm rows

NPARTS = 5


def _layout(R, C, blocks):
    """(buffer shape, (ld, bstride, cb), logical (R, C) view of a buffer) of a rows operand:
    row-major with a stride 8 past C, or 256-channel blocks of (R, 256) rows"""
    if blocks:
        nb = C // 256
        return (nb * R, 256), (256, R * 256, 256), lambda t: t.view(nb, R, 256).permute(1, 0, 2).reshape(R, C)
    return (R, C), (C + 8, 0, C), lambda t: t


BN_SHAPES = [(R, C, False) for R in (1, 3, 5, 131) for C in (8, 40)] + [(R, 512, True) for R in (1, 3, 5, 131)]


def _to_layout(x, R, C, blocks):
    return x.view(R, C // 256, 256).permute(1, 0, 2).reshape(-1, 256).contiguous() if blocks else x


@pytest.mark.parametrize("x_bf16", [1, 0])
@pytest.mark.parametrize("R,C,blocks", BN_SHAPES)
def test_rows_bn_stats(cuda, R, C, blocks, x_bf16):
    """(nparts, 2, C) fp64 partials of sum x and sum x^2, every element written; summed over the
    parts they equal the fp64 sums up to each lane's fp32 accumulation over its rows
    (R 2^-24 of the absolute sum, with room: 1e-5)"""
    x = torch.randn(R, C, generator=_gen(R, C, x_bf16))
    x = x.to(BF) if x_bf16 else x
    shape, lay, _ = _layout(R, C, blocks)
    specs = {"x": In(_to_layout(x, R, C, blocks), ld=lay[0]), "parts": Out((NPARTS * 2, C), F64)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_rows_bn_stats", t["x"], x_bf16, *lay, R, C, t["parts"], NPARTS, like=t["x"]))["parts"]
    got = out.cpu().view(NPARTS, 2, C).sum(0)
    xd = x.double()
    for v, ref, mag in ((0, xd.sum(0), xd.abs().sum(0)), (1, (xd * xd).sum(0), (xd * xd).sum(0))):
        assert bool(((got[v] - ref).abs() <= 1e-5 * mag + 1e-30).all()), v


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("x_bf16", [1, 0])
@pytest.mark.parametrize("R,C,blocks", BN_SHAPES)
def test_rows_bn_apply(cuda, R, C, blocks, x_bf16, p):
    """out = bf16(dropout(relu(x * scale + shift))) with the documented keep hash, within one
    bf16 rounding of the fp32 expression; the output in the other layout family (row-major in,
    row-major out with ldo > C; block in, block out)"""
    g = _gen(R, C, x_bf16, int(p * 10))
    x = torch.randn(R, C, generator=g)
    x = x.to(BF) if x_bf16 else x
    scale, shift = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    shape, lay, view = _layout(R, C, blocks)
    specs = {"x": In(_to_layout(x, R, C, blocks), ld=lay[0]), "scale": In(scale), "shift": In(shift),
             "seed": _seed() if p > 0 else None, "out": Out(shape, BF, ld=lay[0])}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_rows_bn_apply", t["x"], x_bf16, *lay, R, C, t["scale"], t["shift"], float(p), t["seed"],
        SITE, t["out"], *lay, like=t["x"]))["out"]
    z = torch.relu(x.float() * scale + shift).to(cuda)
    if p > 0:
        z = torch.where(row_keep(SEED, SITE, R, C, p, cuda), z * (1 / (1 - p)), torch.zeros_like(z))
    _one_bf16_rounding(view(out), z)


def _bn_bwd_ref(dz, x, scale, shift, mean, invstd, cA, cB, cC):
    dt = torch.where(x * scale + shift > 0, dz, torch.zeros_like(dz))
    return dt, (dt * (x - mean) * invstd), cA * dt + cB * x + cC


@pytest.mark.parametrize("x_bf16", [1, 0])
@pytest.mark.parametrize("R,C,blocks", BN_SHAPES)
def test_rows_bn_bwd(cuda, R, C, blocks, x_bf16):
    _bn_bwd_case(cuda, R, C, blocks, False, x_bf16)


@pytest.mark.parametrize("R,C,blocks", [s for s in BN_SHAPES if not s[2]])
def test_rows_bn_bwd_pooled(cuda, R, C, blocks):
    _bn_bwd_case(cuda, R, C, blocks, True)


def _bn_bwd_case(cuda, R, C, blocks, pooled, x_bf16=1):
    """pass 0: (nparts, 2, C) fp64 partials of sum dt and sum dt xhat (lane sums in fp32: 1e-5 of
    the absolute sums); pass 1: dx = bf16(cA dt + cB x + cC) within one bf16 rounding.  pooled:
    ov3d_rows_bn_bwd_pooled, dz rebuilt from the pooled gradient and its arg rows (row-major
    only), S = R rows per centroid"""
    g = _gen(R, C, pooled, x_bf16)
    x = torch.randn(R, C, generator=g)
    x = x.to(BF) if x_bf16 else x
    scale, shift = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    mean, invstd = 0.2 * torch.randn(C, generator=g), 1 + 0.2 * torch.rand(C, generator=g)
    cA, cB, cC = (torch.randn(C, generator=g) for _ in range(3))
    shape, lay, view = _layout(R, C, blocks)
    if pooled:
        S = R
        gp = torch.randn(1, C, generator=g).to(BF)
        arg = torch.randint(0, S, (1, C), generator=g).to(U8)
        dz = torch.zeros(R, C, dtype=BF).scatter_(0, arg.long(), gp)
        lay, xin = (C, 0, C), In(x)
    else:
        dz = torch.randn(R, C, generator=g).to(BF)
        xin = In(_to_layout(x, R, C, blocks), ld=lay[0])
    vec = {k: In(v) for k, v in dict(scale=scale, shift=shift, mean=mean, invstd=invstd, cA=cA, cB=cB,
                                     cC=cC).items()}
    src = {"g": In(gp), "arg": In(arg, index=(0, S - 1))} if pooled else \
        {"dz": In(_to_layout(dz, R, C, blocks), ld=lay[0])}
    dt, dtx, dx = _bn_bwd_ref(dz.float(), x.float(), scale, shift, mean, invstd, cA, cB, cC)

    def call(t, ps):
        coef = (t["scale"], t["shift"], t["mean"], t["invstd"], t["cA"], t["cB"], t["cC"])
        parts, dxo = (t["parts"], None) if ps == 0 else (None, t["dx"])
        if pooled:
            guard.call("ov3d_rows_bn_bwd_pooled", ps, t["g"], t["arg"], S, t["x"], R, C, *coef, parts,
                       NPARTS if ps == 0 else 0, dxo, like=t["x"])
        else:
            guard.call("ov3d_rows_bn_bwd", ps, t["dz"], *lay, t["x"], x_bf16, *lay, R, C, *coef, 0.0, None, 0,
                       parts, NPARTS if ps == 0 else 0, dxo, *lay, like=t["x"])
    specs = {"x": xin, **src, **vec, "parts": Out((NPARTS * 2, C), F64)}
    got = guard.run_case(cuda, specs, lambda t: call(t, 0))["parts"].cpu().view(NPARTS, 2, C).sum(0)
    for v, term in ((0, dt.double()), (1, dtx.double())):
        assert bool(((got[v] - term.sum(0)).abs() <= 1e-5 * term.abs().sum(0) + 1e-30).all()), v
    oshape = (R, C) if pooled else shape
    specs = {"x": xin, **src, **vec, "dx": Out(oshape, BF, ld=lay[0])}
    out = guard.run_case(cuda, specs, lambda t: call(t, 1))["dx"]
    _one_bf16_rounding((out if pooled else view(out)).cpu(), dx)


# ---------------------------------------------------------------- residual + LayerNorm rows

def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()


RESNORM_C = [8, 16, 32, 64, 128, 256, 512]             # every C with ov3d_resnorm_supported(C)


def _resnorm_data(R, C, p, full):
    g = _gen(R, C, int(p * 10), full)
    d = dict(src=torch.randn(R, C, generator=g), ga=1 + 0.1 * torch.randn(C, generator=g),
             ba=0.1 * torch.randn(C, generator=g), gb=1 + 0.1 * torch.randn(C, generator=g),
             bb=0.1 * torch.randn(C, generator=g))
    d["y"] = torch.randn(R, C, generator=g).to(BF) if full else None
    d["pos"] = torch.randn(R, C, generator=g) if full else None
    return d


def _resnorm_ref(d, R, C, p, cuda):
    """test_resnorm_matches_torch's fp32 restatement with the keep mask of the documented hash"""
    src = d["src"].to(cuda).requires_grad_()
    s = src
    if d["y"] is not None:
        y = d["y"].to(cuda).float()
        if p > 0:
            dr = (y * (1 / (1 - p))).bfloat16().float()
            y = torch.where(row_keep(SEED, SITE, R, C, p, cuda), dr, torch.zeros_like(dr))
        s = src + y
    ga, ba, gb, bb = (d[k].to(cuda).requires_grad_() for k in ("ga", "ba", "gb", "bb"))
    ln_a = torch.nn.functional.layer_norm(s, (C,), ga, ba, 1e-5)
    xb = torch.nn.functional.layer_norm(s, (C,), gb, bb, 1e-5)
    xap = ln_a + d["pos"].to(cuda) if d["pos"] is not None else None
    return dict(src=src, s=s, xa=ln_a, xap=xap, xb=xb, ga=ga, ba=ba, gb=gb, bb=bb)


def _resnorm_fwd_plain(d, R, C, p, cuda):
    """(s, mean, rstd) of an unguarded forward, the inputs of the backward cases"""
    s, mean, rstd = torch.empty(R, C, device=cuda), torch.empty(R, device=cuda), torch.empty(R, device=cuda)
    xa = torch.empty(R, C, device=cuda, dtype=BF)
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda)
    guard.call("ov3d_resnorm_fwd", R, C, d["src"].to(cuda), 0, d["y"].to(cuda) if d["y"] is not None else None,
               1, float(p), seed, SITE, d["ga"].to(cuda), d["ba"].to(cuda), None, 0, None, None, 1e-5, s,
               mean, rstd, xa, None, None, 0, 0, 0, 0, like=s)
    return s.cpu(), mean.cpu(), rstd.cpu()


@pytest.mark.parametrize("full,p", [(True, 0.0), (True, 0.1), (False, 0.0)])
@pytest.mark.parametrize("C", RESNORM_C)
@pytest.mark.parametrize("R", [1, 7, 9, 33])
def test_resnorm_fwd(cuda, R, C, full, p):
    """s, mean, rstd, xa, xap, xb with (full) and without the branch y and pos; bars of
    test_resnorm_matches_torch: s 1e-6, the bf16 rows 8e-3, xb 1e-5 (relative Frobenius)"""
    assert _lib().ov3d_resnorm_supported(C) == 1
    d = _resnorm_data(R, C, p, full)
    specs = {k: In(d[k]) if d[k] is not None else None for k in ("src", "y", "pos", "ga", "ba", "gb", "bb")}
    specs.update({"seed": _seed() if p > 0 else None, "s": Out((R, C), F32), "mean": Out((R,), F32),
                  "rstd": Out((R,), F32), "xa": Out((R, C), BF), "xap": Out((R, C), BF) if full else None,
                  "xb": Out((R, C), F32)})
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_resnorm_fwd", R, C, t["src"], 0, t["y"], 1, float(p), t["seed"], SITE, t["ga"], t["ba"],
        t["pos"], 0, t["gb"], t["bb"], 1e-5, t["s"], t["mean"], t["rstd"], t["xa"], t["xap"], t["xb"], 0,
        0, 0, 0, like=t["src"]))
    with torch.no_grad():
        ref = _resnorm_ref(d, R, C, p, cuda)
    assert _rel(out["s"], ref["s"]) < 1e-6
    assert _rel(out["xa"], ref["xa"].bfloat16()) < 8e-3
    if full:
        assert _rel(out["xap"], ref["xap"].bfloat16()) < 8e-3
    assert _rel(out["xb"], ref["xb"]) < 1e-5
    assert _rel(out["mean"], ref["s"].mean(1)) < 1e-5 or float(ref["s"].mean(1).norm()) < 1e-3
    assert _rel(out["rstd"], (ref["s"].var(1, unbiased=False) + 1e-5).rsqrt()) < 1e-5


@pytest.mark.parametrize("full,p", [(True, 0.0), (True, 0.1), (False, 0.0)])
@pytest.mark.parametrize("C", RESNORM_C)
@pytest.mark.parametrize("R", [1, 7, 9, 33])
def test_resnorm_bwd(cuda, R, C, full, p):
    """dsrc, dy, dpos, the (nparts, 4, C) partials at exactly ov3d_resnorm_bwd_parts rows and the
    four LayerNorm weight gradients against fp32 autograd of the restatement; bars of
    test_resnorm_matches_torch: 1e-4, and 1e-2 for the bf16 dy"""
    d = _resnorm_data(R, C, p, full)
    s, mean, rstd = _resnorm_fwd_plain(d, R, C, p, cuda)
    g = _gen(R, C, 99)
    ds, dxb = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    dxa = torch.randn(R, C, generator=g).to(BF)
    dxap = torch.randn(R, C, generator=g).to(BF) if full else None
    nparts = _lib().ov3d_resnorm_bwd_parts(R, C)
    assert nparts > 0
    specs = {"s": In(s), "mean": In(mean), "rstd": In(rstd), "ds": In(ds), "dxa": In(dxa),
             "dxap": In(dxap) if full else None, "dxb": In(dxb), "ga": In(d["ga"]), "gb": In(d["gb"]),
             "seed": _seed() if p > 0 else None, "dsrc": Out((R, C), F32),
             "dy": Out((R, C), BF) if full else None, "dpos": Out((R, C), F32) if full else None,
             "parts": Out((nparts * 4, C), F32, compare=True),
             **{k: Out((C,), F32) for k in ("dga", "dba", "dgb", "dbb")}}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_resnorm_bwd", R, C, t["s"], t["mean"], t["rstd"], t["ds"], t["dxa"], t["dxap"], t["dxb"], 0,
        0, 0, 0, t["ga"], t["gb"], float(p), t["seed"], SITE, t["dsrc"], t["dy"], 1, t["dpos"], 0,
        t["parts"], nparts, t["dga"], t["dba"], t["dgb"], t["dbb"], 0, like=t["s"]))
    ref = _resnorm_ref(d, R, C, p, cuda)
    loss = (ref["s"] * ds.to(cuda)).sum() + (ref["xa"] * dxa.to(cuda).float()).sum() \
        + (ref["xb"] * dxb.to(cuda)).sum()
    if full:
        loss = loss + (ref["xap"] * dxap.to(cuda).float()).sum()
    loss.backward()
    dsrc = ref["src"].grad
    assert _rel(out["dsrc"], dsrc) < 1e-4
    for k in ("ga", "ba", "gb", "bb"):
        assert _rel(out["d" + k], ref[k].grad) < 1e-4, k
    if full:
        dy = dsrc
        if p > 0:
            dy = torch.where(row_keep(SEED, SITE, R, C, p, cuda), dsrc * (1 / (1 - p)), torch.zeros_like(dsrc))
        assert _rel(out["dy"], dy) < 1e-2
        assert torch.equal(out["dpos"], dxap.to(cuda).float())


# ---------------------------------------------------------------- LayerNorm + row GEMM, one launch

LN_C = 256


def _ln_problem_struct():
    from ov3d_amd import _native
    return _native.struct("ov3d_lngemm_problem")


@pytest.mark.parametrize("nprob,epi,p", [(1, 0, 0.0), (1, 1, 0.1), (2, 0, 0.1), (2, 1, 0.0)])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("R", [32, 96])
def test_lngemm_fwd(cuda, R, N, nprob, epi, p):
    """every output equals the two-launch path (ov3d_resnorm_fwd, then ov3d_rows_gemm_act per
    problem) bit for bit (test_lngemm_kernels_equal_two_launch_path); out rows 8 past N"""
    C = LN_C
    d = _resnorm_data(R, C, p, True)
    g = _gen(R, N, nprob, epi)
    Ns, sels = [N, 128][:nprob], [1, 0][:nprob]
    Ws = [(0.05 * torch.randn(n, C, generator=g)).to(BF) for n in Ns]
    bs = [(0.1 * torch.randn(n, generator=g)).to(BF) for n in Ns]
    site2, ldw = 12, C + 8
    specs = {k: In(d[k]) for k in ("src", "y", "pos", "ga", "ba", "gb", "bb")}
    specs.update({"seed": _seed() if p > 0 else None, "s": Out((R, C), F32), "mean": Out((R,), F32),
                  "rstd": Out((R,), F32), "xa": Out((R, C), BF), "xap": Out((R, C), BF),
                  "xb": Out((R, C), F32)})
    for i, n in enumerate(Ns):
        specs.update({f"W{i}": In(Ws[i], ld=ldw), f"b{i}": In(bs[i]), f"o{i}": Out((R, n), BF, ld=n + 8)})
    P = _ln_problem_struct()

    def call(t):
        arr = (P * nprob)(*[P(t[f"W{i}"].data_ptr(), ldw, t[f"b{i}"].data_ptr(), t[f"o{i}"].data_ptr(),
                              Ns[i] + 8, Ns[i], sels[i]) for i in range(nprob)])
        guard.call("ov3d_lngemm_fwd", R, t["src"], 0, t["y"], float(p), t["seed"], SITE, t["ga"], t["ba"],
                   t["pos"], 0, t["gb"], t["bb"], 1e-5, t["s"], t["mean"], t["rstd"], t["xa"], t["xap"],
                   t["xb"], 0, 0, 0, 0, nprob, ctypes.addressof(arr), epi, float(p), t["seed"], site2,
                   like=t["src"])
    out = guard.run_case(cuda, specs, call)
    dev = {k: v.to(cuda) for k, v in d.items()}
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda) if p > 0 else None
    ref = dict(s=torch.empty(R, C, device=cuda), mean=torch.empty(R, device=cuda),
               rstd=torch.empty(R, device=cuda), xa=torch.empty(R, C, device=cuda, dtype=BF),
               xap=torch.empty(R, C, device=cuda, dtype=BF), xb=torch.empty(R, C, device=cuda))
    guard.call("ov3d_resnorm_fwd", R, C, dev["src"], 0, dev["y"], 1, float(p), seed, SITE, dev["ga"],
               dev["ba"], dev["pos"], 0, dev["gb"], dev["bb"], 1e-5, ref["s"], ref["mean"], ref["rstd"],
               ref["xa"], ref["xap"], ref["xb"], 0, 0, 0, 0, like=ref["s"])
    for i, n in enumerate(Ns):
        o = torch.empty(R, n, device=cuda, dtype=BF)
        guard.call("ov3d_rows_gemm_act", R, n, C, ref["xap"] if sels[i] else ref["xa"], C, Ws[i].to(cuda), C,
                   1, bs[i].to(cuda), epi, float(p), seed, site2, None, 0, o, n, like=o)
        ref[f"o{i}"] = o
    for k, v in ref.items():
        assert torch.equal(out[k], v), (k, (out[k].float() - v.float()).abs().max().item())


@pytest.mark.parametrize("epi,p", [(0, 0.0), (0, 0.1), (2, 0.1)])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("R", [32, 96])
def test_lngemm_bwd(cuda, R, N, epi, p):
    """dsrc, dy, dpos, dx and the partials (exactly ov3d_lngemm_bwd_parts(R) rows) equal
    ov3d_resnorm_bwd followed by ov3d_rows_gemm_act bit for bit; W, H and dx rows 8 past N"""
    C = LN_C
    d = _resnorm_data(R, C, p, True)
    s, mean, rstd = _resnorm_fwd_plain(d, R, C, p, cuda)
    g = _gen(R, N, epi, 5)
    ds = torch.randn(R, C, generator=g)
    dxa, dxap = torch.randn(R, C, generator=g).to(BF), torch.randn(R, C, generator=g).to(BF)
    Wy = (0.05 * torch.randn(C, N, generator=g)).to(BF)
    Hh = torch.relu(torch.randn(R, N, generator=g)).to(BF)
    nparts = _lib().ov3d_lngemm_bwd_parts(R)
    assert nparts == _lib().ov3d_resnorm_bwd_parts(R, C)
    ld = N + 8
    specs = {"s": In(s), "mean": In(mean), "rstd": In(rstd), "ds": In(ds), "dxa": In(dxa), "dxap": In(dxap),
             "ga": In(d["ga"]), "seed": _seed() if p > 0 else None, "W": In(Wy, ld=ld),
             "H": In(Hh, ld=ld) if epi else None, "dsrc": Out((R, C), F32), "dy": Out((R, C), BF),
             "dpos": Out((R, C), F32), "parts": Out((nparts * 4, C), F32, full=False),
             "dx": Out((R, N), BF, ld=ld)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_lngemm_bwd", R, t["s"], t["mean"], t["rstd"], t["ds"], t["dxa"], t["dxap"], None, 0, 0, 0, 0,
        t["ga"], None, float(p), t["seed"], SITE, t["dsrc"], t["dy"], t["dpos"], 0, t["parts"], 0, t["W"],
        ld, N, epi, float(p), t["H"], ld if epi else 0, t["dx"], ld, like=t["s"]))
    seed = torch.tensor([SEED], dtype=torch.int64, device=cuda) if p > 0 else None
    ref = dict(dsrc=torch.empty(R, C, device=cuda), dy=torch.empty(R, C, device=cuda, dtype=BF),
               dpos=torch.empty(R, C, device=cuda), dx=torch.empty(R, N, device=cuda, dtype=BF))
    part = torch.full((nparts, 4, C), float("nan"), device=cuda)
    guard.call("ov3d_resnorm_bwd", R, C, s.to(cuda), mean.to(cuda), rstd.to(cuda), ds.to(cuda), dxa.to(cuda),
               dxap.to(cuda), None, 0, 0, 0, 0, d["ga"].to(cuda), None, float(p), seed, SITE, ref["dsrc"],
               ref["dy"], 1, ref["dpos"], 0, part, nparts, None, None, None, None, 0, like=part)
    guard.call("ov3d_rows_gemm_act", R, N, C, ref["dy"], C, Wy.to(cuda), N, 0, None, epi, float(p), None, 0,
               Hh.to(cuda) if epi else None, N if epi else 0, ref["dx"], N, like=part)
    for k, v in ref.items():
        assert torch.equal(out[k], v), (k, (out[k].float() - v.float()).abs().max().item())
    # the column blocks the row pass owns (k = 0 dga, 1 dba): written in full, equal to resnorm's
    got = out["parts"].view(nparts, 4, C)
    assert torch.equal(got[:, :2], part[:, :2])


# ---------------------------------------------------------------- encoder post-attention chain

@pytest.mark.parametrize("kq", [1, 0])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R", [64, 192])
def test_enc_post(cuda, monkeypatch, R, p, kq):
    """forward and backward equal the four launches they replace bit for bit (test_encpost_gpu.py),
    on the short row-block kernels (k_quarters = 1) and the long ones (0); weight rows 8 past
    their width; the partials at exactly ov3d_resnorm_bwd_parts(R, 256) rows"""
    import test_encpost_gpu as EP
    from ov3d_amd import gemm
    monkeypatch.setattr(gemm, "ROWS_GEMM", bool(kq))
    monkeypatch.setattr(gemm, "TILE_GEMM", True)
    assert EP._kq(R) == kq
    C, F = EP.C, EP.F
    d = EP._inputs(cuda, R, p)
    seed_in = In(d["seed"].cpu(), index=(3, 5)) if p > 0 else None
    ref = EP._unfused_fwd(d, R, p)
    cpu = {k: v.cpu() for k, v in d.items() if k != "seed"}
    w = {"wo": C + 8, "w1": C + 8, "w2": F + 8}
    specs = {k: In(cpu[k], ld=w.get(k)) for k in ("s", "o", "wo", "bo", "g2", "be2", "w1", "b1", "w2", "b2")}
    specs.update({"seed": seed_in, "s1": Out((R, C), F32), "mean": Out((R,), F32), "rstd": Out((R,), F32),
                  "x2": Out((R, C), BF), "h": Out((R, F), BF), "y2": Out((R, C), BF)})
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_enc_post_fwd", R, t["s"], t["o"], t["wo"], w["wo"], t["bo"], float(p), t["seed"], EP.SITE1,
        t["g2"], t["be2"], 1e-5, t["w1"], w["w1"], t["b1"], float(p), EP.SITE_FFN, t["w2"], w["w2"], t["b2"],
        kq, t["s1"], t["mean"], t["rstd"], t["x2"], t["h"], t["y2"], like=t["s"]))
    for k in ("s1", "mean", "rstd", "x2", "h", "y2"):
        assert torch.equal(out[k], ref[k]), (k, (out[k].float() - ref[k].float()).abs().max().item())
    # backward, from the unfused forward's saved tensors
    nparts = _lib().ov3d_resnorm_bwd_parts(R, C)
    d1 = gemm.act_gemm(d["dy2"], d["w2"], None, False, 2, p, h=ref["h"])
    dx2 = gemm.act_gemm(d1, d["w1"], None, False)
    ds, dy1 = torch.empty(R, C, device=cuda), torch.empty(R, C, device=cuda, dtype=BF)
    part = torch.empty(nparts, 4, C, device=cuda)
    guard.call("ov3d_resnorm_bwd", R, C, ref["s1"], ref["mean"], ref["rstd"], d["ds1"], dx2, None, None, 0, 0,
               0, 0, d["g2"], None, float(p), d["seed"], EP.SITE1, ds, dy1, 1, None, 0, part, nparts, None,
               None, None, None, 0, like=ds)
    rb = dict(d1=d1, dy1=dy1, dout=gemm.act_gemm(dy1, d["wo"], None, False), ds=ds)
    specs = {k: In(cpu[k], ld=w.get(k)) for k in ("ds1", "dy2", "g2", "wo", "w1", "w2")}
    specs.update({k: In(ref[k].cpu()) for k in ("s1", "mean", "rstd", "h")})
    specs.update({"seed": seed_in, "ds": Out((R, C), F32), "dy1": Out((R, C), BF), "dout": Out((R, C), BF),
                  "d1": Out((R, F), BF), "parts": Out((nparts * 4, C), F32, full=False)})
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_enc_post_bwd", R, t["ds1"], t["dy2"], t["s1"], t["mean"], t["rstd"], t["h"], t["g2"], t["wo"],
        w["wo"], t["w1"], w["w1"], t["w2"], w["w2"], float(p), t["seed"], EP.SITE1, float(p), kq, t["ds"],
        t["dy1"], t["dout"], t["d1"], t["parts"], nparts, like=t["ds"]))
    for k, v in rb.items():
        assert torch.equal(out[k], v), (k, (out[k].float() - v.float()).abs().max().item())
    assert torch.equal(out["parts"].view(nparts, 4, C)[:, :2], part[:, :2])


# ---------------------------------------------------------------- heads' output layers

@pytest.mark.parametrize("T", [1, 32])
@pytest.mark.parametrize("R", [1, 31, 33])
def test_heads_out(cuda, R, T):
    """ov3d_heads_out_fwd / _bwd (row blocks of 32) with the fewest and the most text rows, the
    workspace at exactly ov3d_heads_out_workspace floats, z and dz rows 8 past 1280 and dz's
    visual columns left to the caller; bars of test_heads_out_fwd_bwd_match_fp32"""
    assert _lib().ov3d_heads_out_max_text() == 32
    Hd, Nv, nb = 256, 640, 12
    n = [3, 3, nb, nb]
    ocol = [0, 3, 6, 6 + nb]
    Ns = sum(n)
    g = _gen(R, T)
    z = torch.randn(R, 5 * Hd, generator=g).to(BF)
    wv, bv = (torch.randn(Nv, Hd, generator=g) * 0.06).to(BF), torch.randn(Nv, generator=g) * 0.1
    ws = [(torch.randn(k, Hd, generator=g) * 0.06).to(BF) for k in n]
    bs = [torch.randn(k, generator=g) * 0.1 for k in n]
    text = torch.randn(T, Nv, generator=g) * 0.05
    ldz = 5 * Hd + 8
    nwork = _lib().ov3d_heads_out_workspace(R, T)
    ints = dict(n=(ctypes.c_int * 4)(*n), kcol=(ctypes.c_int * 4)(*[Hd * (1 + i) for i in range(4)]),
                ocol=(ctypes.c_int * 4)(*ocol))
    specs = {"z": In(z, ld=ldz), "wv": In(wv), "bv": In(bv), "text": In(text),
             **{f"ws{i}": In(ws[i]) for i in range(4)}, **{f"bs{i}": In(bs[i]) for i in range(4)},
             "out_v": Out((R, Nv), F32), "logits": Out((R, T), F32), "out_s": Out((R, Ns), F32),
             "work": Out((nwork,), F32, full=False, compare=False, finite=False) if nwork else None}

    def fwd(t):
        wp = (ctypes.c_void_p * 4)(*[t[f"ws{i}"].data_ptr() for i in range(4)])
        bp = (ctypes.c_void_p * 4)(*[t[f"bs{i}"].data_ptr() for i in range(4)])
        guard.call("ov3d_heads_out_fwd", t["z"], ldz, R, t["wv"], t["bv"], Nv, t["text"], T, 0, t["out_v"],
                   t["logits"], 4, ctypes.addressof(wp), ctypes.addressof(bp), ctypes.addressof(ints["n"]),
                   ctypes.addressof(ints["kcol"]), ctypes.addressof(ints["ocol"]), t["out_s"], Ns, t["work"],
                   like=t["z"])
    out = guard.run_case(cuda, specs, fwd)
    zf = z.to(cuda).float()
    ref_v = zf[:, :Hd] @ wv.to(cuda).float().t() + bv.to(cuda)
    ref_s = torch.cat([zf[:, Hd * (1 + i):Hd * (2 + i)] @ ws[i].to(cuda).float().t() + bs[i].to(cuda)
                       for i in range(4)], 1)
    torch.testing.assert_close(out["out_v"], ref_v, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out["out_s"], ref_s, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out["logits"], ref_v @ text.to(cuda).t(), rtol=1e-4, atol=1e-4)
    # backward
    gv, gl, gs = (torch.randn(R, k, generator=g) for k in (Nv, T, Ns))
    theirs = torch.zeros(R, 5 * Hd, dtype=torch.bool)
    theirs[:, Hd:] = True                                # the visual columns are the caller's
    specs = {"gv": In(gv), "gl": In(gl), "text": In(text), "gs": In(gs),
             **{f"ws{i}": In(ws[i]) for i in range(4)}, "gvb": Out((R, Nv), BF), "gsb": Out((R, Ns), BF),
             "dz": Out((R, 5 * Hd), BF, ld=ldz, full=theirs)}

    def bwd(t):
        wp = (ctypes.c_void_p * 4)(*[t[f"ws{i}"].data_ptr() for i in range(4)])
        guard.call("ov3d_heads_out_bwd", t["gv"], t["gl"], t["text"], R, Nv, T, 0, t["gs"], Ns, 4,
                   ctypes.addressof(wp), ctypes.addressof(ints["n"]), ctypes.addressof(ints["kcol"]),
                   ctypes.addressof(ints["ocol"]), t["gvb"], t["gsb"], t["dz"], ldz, like=t["gv"])
    out = guard.run_case(cuda, specs, bwd)
    torch.testing.assert_close(out["gvb"].float(), gv.to(cuda) + gl.to(cuda) @ text.to(cuda), rtol=8e-3,
                               atol=1e-3)
    assert torch.equal(out["gsb"], gs.to(cuda).to(BF))
    gsr = out["gsb"].float()
    for i in range(4):
        ref = gsr[:, ocol[i]:ocol[i] + n[i]] @ ws[i].to(cuda).float()
        torch.testing.assert_close(out["dz"][:, Hd * (1 + i):Hd * (2 + i)].float(), ref, rtol=8e-3, atol=1e-3)
