"""The encoder layer's chain after its self-attention in one launch each way (csrc/encpost.hip,
resnorm._EncPost) against the four launches it replaces each way: every output bit for bit, at
row counts that run the unfused path on the short row-block kernel (one tile, three tiles) and
on the long one (4096 rows), with and without dropout, LayerNorm weights away from 1 / 0."""
import ctypes

import pytest
import torch

from helpers import ov3d  # noqa: F401

pytestmark = pytest.mark.gpu

C, F = 256, 128
SITE1, SITE_FFN = 11, 12
ROWS = [64, 192, 4096]


def _inputs(cuda, R, p):
    from ov3d_amd import attention as flash
    g = torch.Generator(device=cuda).manual_seed(1000 * R + int(100 * p))
    rn = lambda *s: torch.randn(*s, device=cuda, generator=g)   # noqa: E731
    bf = torch.bfloat16
    d = dict(
        s=rn(R, C), o=rn(R, C).to(bf),
        wo=(rn(C, C) / C ** 0.5).to(bf), bo=(0.1 * rn(C)).to(bf),
        g2=1.0 + 0.3 * rn(C), be2=0.2 * rn(C),
        w1=(rn(F, C) / C ** 0.5).to(bf), b1=(0.1 * rn(F)).to(bf),
        w2=(rn(C, F) / F ** 0.5).to(bf), b2=(0.1 * rn(C)).to(bf),
        ds1=rn(R, C), dy2=rn(R, C).to(bf))
    d["seed"] = flash._seed(cuda) if p > 0 else None
    return d


def _kq(R):
    from ov3d_amd import gemm
    return int(gemm.ROWS_GEMM and R <= gemm.ROWS_GEMM_MAX_M)


def _unfused_fwd(d, R, p):
    """out-projection, resnorm, linear1 + ReLU + dropout, linear2: the launches of the old path"""
    from ov3d_amd import _native, gemm
    dev = d["s"].device
    y1 = gemm.act_gemm(d["o"], d["wo"], d["bo"], True)
    s1 = torch.empty((R, C), dtype=torch.float32, device=dev)
    mean = torch.empty(R, dtype=torch.float32, device=dev)
    rstd = torch.empty(R, dtype=torch.float32, device=dev)
    x2 = torch.empty((R, C), dtype=torch.bfloat16, device=dev)
    _native.call("ov3d_resnorm_fwd", R, C, d["s"], 0, y1, 1, float(p), d["seed"], SITE1, d["g2"],
                 d["be2"], None, 0, None, None, 1e-5, s1, mean, rstd, x2, None, None, 0, 0, 0, 0,
                 like=s1)
    h = gemm.act_gemm(x2, d["w1"], d["b1"], True, 1, p, d["seed"], SITE_FFN)
    y2 = gemm.act_gemm(h, d["w2"], d["b2"], True)
    return dict(s1=s1, mean=mean, rstd=rstd, x2=x2, h=h, y2=y2)


def _fused_fwd(d, R, p):
    from ov3d_amd import _native
    dev = d["s"].device
    bf = torch.bfloat16
    out = dict(s1=torch.empty((R, C), dtype=torch.float32, device=dev),
               mean=torch.empty(R, dtype=torch.float32, device=dev),
               rstd=torch.empty(R, dtype=torch.float32, device=dev),
               x2=torch.empty((R, C), dtype=bf, device=dev),
               h=torch.empty((R, F), dtype=bf, device=dev),
               y2=torch.empty((R, C), dtype=bf, device=dev))
    _native.call("ov3d_enc_post_fwd", R, d["s"], d["o"], d["wo"], C, d["bo"], float(p), d["seed"],
                 SITE1, d["g2"], d["be2"], 1e-5, d["w1"], C, d["b1"], float(p), SITE_FFN, d["w2"],
                 F, d["b2"], _kq(R), out["s1"], out["mean"], out["rstd"], out["x2"], out["h"],
                 out["y2"], like=d["s"])
    return out


def _colsum(partials, nparts):
    from ov3d_amd import resnorm
    dev = partials.device
    dg = torch.empty(C, dtype=torch.float32, device=dev)
    db = torch.empty(C, dtype=torch.float32, device=dev)
    resnorm._colsums(partials, nparts, C, (dg, db, None, None), 0)
    return dg, db


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R", ROWS)
def test_forward_kernel_equals_the_four_launches(cuda, R, p):
    from ov3d_amd import _native
    assert _native.load().ov3d_enc_post_supported(R, C, F) == 1
    d = _inputs(cuda, R, p)
    ref = _unfused_fwd(d, R, p)
    out = _fused_fwd(d, R, p)
    for k in ("s1", "mean", "rstd", "x2", "h", "y2"):
        assert torch.equal(out[k], ref[k]), (k, (out[k].float() - ref[k].float()).abs().max().item())
    zeros = (out["h"] == 0).float().mean().item()
    if p > 0:   # relu's half plus a tenth of the rest: an all-kept mask would give ~0.5
        assert 0.5 < zeros < 0.65, zeros


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("R", ROWS)
def test_backward_kernel_equals_the_four_launches(cuda, R, p):
    from ov3d_amd import _native, gemm
    lib = _native.load()
    d = _inputs(cuda, R, p)
    f = _unfused_fwd(d, R, p)
    dev = d["s"].device
    bf = torch.bfloat16
    nparts = lib.ov3d_resnorm_bwd_parts(R, C)
    # linear2's masked input gradient, linear1's, the resnorm backward, the out-projection's
    d1 = gemm.act_gemm(d["dy2"], d["w2"], None, False, 2, p, h=f["h"])
    dx2 = gemm.act_gemm(d1, d["w1"], None, False)
    ds = torch.empty((R, C), dtype=torch.float32, device=dev)
    dy1 = torch.empty((R, C), dtype=bf, device=dev)
    part = torch.empty((nparts, 4, C), dtype=torch.float32, device=dev)
    _native.call("ov3d_resnorm_bwd", R, C, f["s1"], f["mean"], f["rstd"], d["ds1"], dx2, None, None,
                 0, 0, 0, 0, d["g2"], None, float(p), d["seed"], SITE1, ds, dy1, 1, None, 0, part,
                 nparts, None, None, None, None, 0, like=ds)
    do = gemm.act_gemm(dy1, d["wo"], None, False)
    ref = dict(d1=d1, dy1=dy1, do=do, ds=ds)
    ref["dg2"], ref["db2"] = _colsum(part, nparts)

    out = dict(ds=torch.empty_like(ds), dy1=torch.empty_like(dy1), do=torch.empty_like(do),
               d1=torch.empty_like(d1))
    part2 = torch.full((nparts, 4, C), float("nan"), dtype=torch.float32, device=dev)
    _native.call("ov3d_enc_post_bwd", R, d["ds1"], d["dy2"], f["s1"], f["mean"], f["rstd"], f["h"],
                 d["g2"], d["wo"], C, d["w1"], C, d["w2"], F, float(p), d["seed"], SITE1, float(p),
                 _kq(R), out["ds"], out["dy1"], out["do"], out["d1"], part2, nparts, like=ds)
    out["dg2"], out["db2"] = _colsum(part2, nparts)
    for k in ("d1", "dy1", "do", "ds", "dg2", "db2"):
        assert torch.equal(out[k], ref[k]), (k, (out[k].float() - ref[k].float()).abs().max().item())
    assert torch.equal(part2[:, :2], part[:, :2]) and not part2.isnan().any()
    if p > 0:
        zeros = (out["dy1"] == 0).float().mean().item()
        assert 0.07 < zeros < 0.13, zeros   # the keep mask of dropout_p1, regenerated


def _encoder(cuda, ffn=128):
    from ov3d_amd.transformer import TransformerEncoder, TransformerEncoderLayer
    torch.manual_seed(3)
    enc = TransformerEncoder(TransformerEncoderLayer(256, 4, ffn, dropout=0.1), 2).to(cuda).train()
    with torch.no_grad():
        for l in enc.layers:   # LayerNorm weights away from 1 / 0, biases away from 0
            for n in (l.norm1, l.norm2):
                n.weight.add_(0.3 * torch.randn_like(n.weight))
                n.bias.add_(0.2 * torch.randn_like(n.bias))
            for b in (l.self_attn.out_proj.bias, l.linear1.bias, l.linear2.bias):
                b.add_(0.1 * torch.randn_like(b))
    return enc


def _run_encoder(enc, x0, pos, on, defer, monkeypatch):
    """-> (output, input gradient, parameter gradients, census) of one training step"""
    from ov3d_amd import _native, gemm, resnorm
    monkeypatch.setattr(resnorm, "enc_post", on)
    monkeypatch.setattr(resnorm, "enc_post_fwd", True)
    monkeypatch.setattr(resnorm, "enc_post_bwd", True)
    monkeypatch.setattr(gemm, "DEFER_WGRAD", defer)
    enc.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_()
    _native.census_start()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, out, _ = enc(x, pos=pos)
    out.float().square().sum().backward()
    census = _native.census_stop()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters()}
    assert all(g is not None for g in grads.values())
    return out.detach().clone(), x.grad.clone(), grads, census


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("L,B", [(256, 2), (2048, 1)])
def test_encoder_switch_on_equals_off(cuda, monkeypatch, L, B, defer):
    enc = _encoder(cuda)
    g = torch.Generator(device=cuda).manual_seed(L + B)
    x0 = torch.randn(L, B, 256, device=cuda, generator=g)
    pos = torch.randn(L, B, 256, device=cuda, generator=g)
    off = _run_encoder(enc, x0, pos, False, defer, monkeypatch)
    on = _run_encoder(enc, x0, pos, True, defer, monkeypatch)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for n in off[2]:
        assert torch.equal(on[2][n], off[2][n]), n
    nl = len(enc.layers)
    assert on[3].get("ov3d_enc_post_fwd", 0) == nl and on[3].get("ov3d_enc_post_bwd", 0) == nl
    assert "ov3d_enc_post_fwd" not in off[3] and "ov3d_enc_post_bwd" not in off[3]
    # norm1 and the encoder's last residual add stay on the resnorm launches
    assert on[3]["ov3d_resnorm_fwd"] == nl + 1 and off[3]["ov3d_resnorm_fwd"] == 2 * nl + 1


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_one_direction_fused_equals_off(cuda, monkeypatch, direction):
    """either direction alone on the fused kernel (OV3D_ENC_POST=fwd / bwd) gives the same step"""
    from ov3d_amd import resnorm
    enc = _encoder(cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    x0 = torch.randn(256, 2, 256, device=cuda, generator=g)
    off = _run_encoder(enc, x0, None, False, False, monkeypatch)
    monkeypatch.setattr(resnorm, "enc_post", True)
    from ov3d_amd import _native
    enc.zero_grad(set_to_none=True)
    monkeypatch.setattr(resnorm, "enc_post_fwd", direction == "fwd")
    monkeypatch.setattr(resnorm, "enc_post_bwd", direction == "bwd")
    x = x0.clone().requires_grad_()
    _native.census_start()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, out, _ = enc(x)
    out.float().square().sum().backward()
    census = _native.census_stop()
    assert ("ov3d_enc_post_fwd" in census) == (direction == "fwd")
    assert ("ov3d_enc_post_bwd" in census) == (direction == "bwd")
    assert torch.equal(out, off[0]) and torch.equal(x.grad, off[1])
    for n, p in enc.named_parameters():
        assert torch.equal(p.grad, off[2][n]), n


@pytest.mark.parametrize("ffn,L", [(256, 256), (128, 224)])
def test_unsupported_shapes_keep_the_old_path(cuda, monkeypatch, ffn, L):
    """dim_feedforward 256, or a row count that is no multiple of the 64-row tile"""
    from ov3d_amd import _native
    assert _native.load().ov3d_enc_post_supported(L, 256, ffn) == 0
    enc = _encoder(cuda, ffn)
    g = torch.Generator(device=cuda).manual_seed(L)
    x0 = torch.randn(L, 1, 256, device=cuda, generator=g)
    off = _run_encoder(enc, x0, None, False, False, monkeypatch)
    on = _run_encoder(enc, x0, None, True, False, monkeypatch)
    assert "ov3d_enc_post_fwd" not in on[3] and "ov3d_enc_post_bwd" not in on[3]
    assert on[3]["ov3d_resnorm_fwd"] == off[3]["ov3d_resnorm_fwd"] == 2 * len(enc.layers) + 1
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for n in off[2]:
        assert torch.equal(on[2][n], off[2][n]), n


def test_entries_reject_bad_arguments():
    """null pointers, misaligned operands and short or misaligned strides return the error code
    before any launch (host-side checks only: the pointers are never dereferenced)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # 16-byte aligned
    odd = ctypes.c_void_p(264)    # 8-byte aligned only
    assert lib.ov3d_enc_post_supported(64, 256, 128) == 1
    assert lib.ov3d_enc_post_supported(16384, 256, 128) == 1
    assert lib.ov3d_enc_post_supported(96, 256, 128) == 0
    assert lib.ov3d_enc_post_supported(64, 128, 128) == 0
    assert lib.ov3d_enc_post_supported(64, 256, 256) == 0
    assert lib.ov3d_enc_post_supported(0, 256, 128) == 0
    fwd_ok = dict(R=64, s=p, o=p, Wo=p, ldwo=256, bo=p, p1=0.1, seed=p, site1=1, g2=p, be2=p,
                  eps=1e-5, W1=p, ldw1=256, b1=p, pf=0.1, site_ffn=2, W2=p, ldw2=128, b2=p, kq=0,
                  s1=p, mean=p, rstd=p, x2=p, h=p, y2=p)

    def fwd(**kw):
        a = dict(fwd_ok, **kw)
        assert set(a) == set(fwd_ok)
        return lib.ov3d_enc_post_fwd(*[a[k] for k in fwd_ok], None)
    for k in ("s", "o", "Wo", "bo", "g2", "be2", "W1", "b1", "W2", "b2", "s1", "mean", "rstd", "x2",
              "h", "y2", "seed"):
        assert fwd(**{k: None}) == -1, k
    for k in ("s", "o", "Wo", "W1", "W2", "bo", "b1", "b2", "g2", "be2", "s1", "x2", "h", "y2"):
        assert fwd(**{k: odd}) == -1, k
    assert fwd(R=96) == -1 and fwd(R=0) == -1
    assert fwd(ldwo=248) == -1 and fwd(ldw1=260) == -1 and fwd(ldw2=120) == -1   # short, % 8, short
    assert fwd(p1=1.0) == -1 and fwd(pf=-0.1) == -1

    bwd_ok = dict(R=64, ds1=p, dy2=p, s1=p, mean=p, rstd=p, h=p, g2=p, Wo=p, ldwo=256, W1=p,
                  ldw1=256, W2=p, ldw2=128, p1=0.1, seed=p, site1=1, pf=0.1, kq=0, ds=p, dy1=p,
                  dout=p, d1=p, partials=p, nparts=8)

    def bwd(**kw):
        a = dict(bwd_ok, **kw)
        assert set(a) == set(bwd_ok)
        return lib.ov3d_enc_post_bwd(*[a[k] for k in bwd_ok], None)
    for k in ("ds1", "dy2", "s1", "mean", "rstd", "h", "g2", "Wo", "W1", "W2", "ds", "dy1", "dout",
              "d1", "partials", "seed"):
        assert bwd(**{k: None}) == -1, k
    for k in ("ds1", "dy2", "s1", "h", "g2", "Wo", "W1", "W2", "ds", "dy1", "dout", "d1", "partials"):
        assert bwd(**{k: odd}) == -1, k
    assert bwd(R=96) == -1 and bwd(nparts=2) == -1 and bwd(R=4096, nparts=512) == -1
    assert bwd(ldwo=248) == -1 and bwd(ldw1=260) == -1 and bwd(ldw2=120) == -1
    assert bwd(p1=1.0) == -1 and bwd(pf=1.5) == -1
