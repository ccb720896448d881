"""Guard-band cases of the point operations (csrc/fps.hip, csrc/group.hip): sampling, ball
query, grouping and gathering at the smallest shapes, every operand between guard bands
(tests/guard.py).  Index inputs carry valid indices in their bands (0 under fill A, the largest
valid index under fill B), so an over-read that is dereferenced changes the output instead of
the address space.  Values: the C oracle / exact torch expressions the family's tests in
test_kernels_gpu.py use (bit-exact)."""
import numpy as np
import pytest
import torch

import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32, I32, BF = torch.float32, torch.int32, torch.bfloat16
ENTRIES = ("ov3d_fps", "ov3d_fps_pair_status", "ov3d_ball_query", "ov3d_ball_query_cells",
           "ov3d_group_fwd", "ov3d_group_rows_bf16", "ov3d_group_bwd", "ov3d_group_inverse",
           "ov3d_group_bwd_csr", "ov3d_group_bwd_csr_bf16", "ov3d_gather_fwd", "ov3d_gather_bwd")


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 104729 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _scratch(n, dtype=F32):
    """a workspace of exactly n elements whose final contents are unspecified"""
    return Out((n,), dtype, full=False, compare=False, finite=False)


# ---------------------------------------------------------------- FPS

def _fps_case(cuda, B, N, M, gather, status=False):
    from ov3d_amd import _native
    xyz = torch.rand(B, N, 3, generator=_gen(B, N, M)) * 4
    nws = _native.load().ov3d_fps_workspace(B, N)
    specs = {"xyz": In(xyz), "idx": Out((B, M), I32), "new": Out((B, M, 3), F32) if gather else None,
             "ws": _scratch(nws) if nws else None, "status": Out((B,), I32) if status else None}

    def call(t):
        guard.call("ov3d_fps", t["xyz"], B, N, M, t["idx"], t["new"], t["ws"], like=t["xyz"])
        if status:
            guard.call("ov3d_fps_pair_status", t["ws"], B, N, M, t["status"], like=t["xyz"])
    out = guard.run_case(cuda, specs, call)
    ref = O.fps(xyz.numpy(), M)
    assert np.array_equal(out["idx"].cpu().numpy(), ref)
    if gather:
        exp = np.take_along_axis(xyz.numpy(), ref.astype(np.int64)[..., None], axis=1)
        assert np.array_equal(out["new"].cpu().numpy(), exp)
    if status:
        assert out["status"].cpu().tolist() == [0] * B
    return nws


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("N,M", [(1, 1), (63, 1), (63, 33), (65, 1), (65, 33), (1000, 1), (1000, 33)])
def test_fps(cuda, N, M, gather):
    assert _fps_case(cuda, 2, N, M, gather) == 0        # no workspace up to 20480 points


@pytest.mark.parametrize("N", [20481, 40961])
def test_fps_workspace_regimes(cuda, N):
    """the two regimes of ov3d_fps_workspace (half of each wave's points up to 40960, the running
    distances beyond) with the workspace at exactly the reported size, and the pair status"""
    assert _fps_case(cuda, 2, N, 8, True, status=True) > 0


# ---------------------------------------------------------------- ball query

def _ball_case(cuda, entry, B, N, M, S, r, seed):
    from ov3d_amd import _native
    g = _gen(N, M, S, seed)
    xyz = torch.rand(B, N, 3, generator=g)
    cen = xyz[:, torch.randperm(N, generator=g)[:M]].contiguous()
    cells = entry == "ov3d_ball_query_cells"
    nbytes = int(_native.load().ov3d_ball_query_ws_bytes(B, N)) if cells else 0
    specs = {"xyz": In(xyz), "cen": In(cen), "idx": Out((B, M, S), I32),
             "ws": _scratch(nbytes, torch.uint8) if cells else None}

    def call(t):
        if cells:
            guard.call(entry, t["xyz"], t["cen"], B, N, M, float(r), S, t["idx"], t["ws"], nbytes,
                       like=t["xyz"])
        else:
            guard.call(entry, t["xyz"], t["cen"], B, N, M, float(r), S, t["idx"], like=t["xyz"])
    out = guard.run_case(cuda, specs, call)
    ref = O.ball_query(xyz.numpy(), cen.numpy(), r, S)
    assert np.array_equal(out["idx"].cpu().numpy(), ref)
    return nbytes


@pytest.mark.parametrize("S", [1, 16, 65])
def test_ball_query(cuda, S):
    _ball_case(cuda, "ov3d_ball_query", 2, 100, 7, S, 0.3, 0)


@pytest.mark.parametrize("r", [0.05, 10.0])
def test_ball_query_cells(cuda, r):
    """8192 points: the smallest scene on the cell path, the index of exactly
    ov3d_ball_query_ws_bytes bytes; r = 10 puts every point in every ball, past the per-wave hit
    cap (the fallback scan)"""
    assert _ball_case(cuda, "ov3d_ball_query_cells", 2, 8192, 5, 16, r, 1) > 0


# ---------------------------------------------------------------- grouping

B, N, M, S, R = 2, 50, 3, 4, 0.4


def _scene(C, layout, seed):
    """points, centroids, an index in which no point is read more than twice (two addends: the
    atomic backward's sums do not depend on their order) and the features in `layout`"""
    g = _gen(C, len(layout), seed)
    xyz = torch.rand(B, N, 3, generator=g) * 2
    cen = xyz[:, :M].contiguous()
    idx = torch.stack([torch.randperm(N, generator=g)[:M * S] for _ in range(B)]).view(B, M, S).int()
    idx[:, 1, 0] = idx[:, 0, 0]                          # one point read twice per scene
    if layout == "bcn":
        store = torch.randn(B, C, N, generator=g)
        strides, feats = (C * N, 1, N), store
    else:                                                # seq-first (N, B, C)
        store = torch.randn(N, B, C, generator=g)
        strides, feats = (C, B * C, 1), store.permute(1, 2, 0)
    return xyz, cen, idx, store, strides, feats          # feats: the (B, C, N) view


def _group_ref(xyz, cen, idx, feats, C):
    il = idx.long().view(B, -1)
    gx = np.take_along_axis(xyz.numpy(), il.numpy()[..., None], axis=1).reshape(B, M, S, 3)
    ref = np.zeros((B, M, S, 3 + C), dtype=np.float32)
    ref[..., :3] = (gx - cen.numpy()[:, :, None, :]) / np.float32(R)
    if C:
        ft = feats.transpose(1, 2).contiguous().numpy()                      # (B, N, C)
        ref[..., 3:] = np.take_along_axis(ft, il.numpy()[..., None], axis=1).reshape(B, M, S, C)
    return torch.from_numpy(ref)


def _idx_in(idx):
    return In(idx, index=(0, N - 1))


@pytest.mark.parametrize("layout", ["bcn", "nbc"])
@pytest.mark.parametrize("C", [0, 5])
def test_group_fwd(cuda, C, layout):
    xyz, cen, idx, store, st, feats = _scene(C, layout, 1)
    specs = {"xyz": In(xyz), "cen": In(cen), "f": In(store) if C else None, "idx": _idx_in(idx),
             "out": Out((B * M * S, 3 + C), F32)}

    def call(t):
        guard.call("ov3d_group_fwd", t["xyz"], t["cen"], t["f"], *st, t["idx"], B, C, N, M, S, R, 1,
                   t["out"], like=t["xyz"])
    out = guard.run_case(cuda, specs, call)["out"]
    assert torch.equal(out.cpu().view(B, M, S, 3 + C), _group_ref(xyz, cen, idx, feats, C))


@pytest.mark.parametrize("ldo", [8, 16])
@pytest.mark.parametrize("layout", ["bcn", "nbc"])
@pytest.mark.parametrize("C", [0, 5])
def test_group_rows_bf16(cuda, C, layout, ldo):
    """every column of the ldo-wide rows is written: columns 3 + C .. ldo - 1 as zeros"""
    xyz, cen, idx, store, st, feats = _scene(C, layout, 2)
    specs = {"xyz": In(xyz), "cen": In(cen), "f": In(store) if C else None, "idx": _idx_in(idx),
             "out": Out((B * M * S, ldo), BF)}

    def call(t):
        guard.call("ov3d_group_rows_bf16", t["xyz"], t["cen"], t["f"], *st, t["idx"], B, C, N, M, S, R,
                   1, ldo, t["out"], like=t["xyz"])
    out = guard.run_case(cuda, specs, call)["out"]
    ref = torch.zeros(B * M * S, ldo)
    ref[:, :3 + C] = _group_ref(xyz, cen, idx, feats, C).view(-1, 3 + C)
    assert torch.equal(out.cpu(), ref.to(BF))


def _feature_grad_ref(g, idx, C):
    """(B, C, N) scatter-add of the feature columns of g (B*M*S, >= 3 + C); at most two addends"""
    ref = torch.zeros(B, C, N)
    gi = idx.long().view(B, 1, M * S).expand(B, C, M * S)
    return ref.scatter_add_(2, gi, g[:, 3:3 + C].float().view(B, M * S, C).transpose(1, 2))


def _as_bcn(flat, layout, C):
    return flat.view(B, C, N) if layout == "bcn" else flat.view(N, B, C).permute(1, 2, 0)


def _grad_out(C):
    """the feature-gradient buffer; C = 0: one element that must stay untouched"""
    return Out((B * C * N,), F32) if C else Out((1,), F32, full=False)


@pytest.mark.parametrize("layout", ["bcn", "nbc"])
@pytest.mark.parametrize("C", [0, 5])
def test_group_bwd(cuda, C, layout):
    _, _, idx, _, st, _ = _scene(C, layout, 3)
    g = torch.randn(B * M * S, 3 + C, generator=_gen(C, 3))
    specs = {"g": In(g), "idx": _idx_in(idx), "gf": _grad_out(C)}

    def call(t):
        guard.call("ov3d_group_bwd", t["g"], t["idx"], B, C, N, M, S, *st, t["gf"], like=t["g"])
    out = guard.run_case(cuda, specs, call)["gf"]
    if C:
        assert torch.equal(_as_bcn(out.cpu(), layout, C), _feature_grad_ref(g, idx, C))
    else:
        assert bool(torch.isnan(out).all())


def _inverse(cuda, idx):
    from ov3d_amd import pointnet2_utils as pu
    off, rows = pu.group_inverse(idx.to(cuda), N)
    return off.cpu(), rows.cpu()


def test_group_inverse(cuda):
    """offsets and rows are exactly a stable argsort by point (test_group_inverse_index); cnt and
    cursor are B*N-word scratch"""
    _, _, idx, _, _, _ = _scene(5, "bcn", 4)
    idx[1] = 7                                           # one point read by every row of a scene
    specs = {"idx": _idx_in(idx), "cnt": _scratch(B * N, I32), "off": Out((B * N + 1,), I32),
             "cur": _scratch(B * N, I32), "rows": Out((B * M * S,), I32)}

    def call(t):
        guard.call("ov3d_group_inverse", t["idx"], B, N, M, S, t["cnt"], t["off"], t["cur"], t["rows"],
                   like=t["idx"])
    out = guard.run_case(cuda, specs, call)
    key = np.repeat(np.arange(B), M * S) * N + idx.numpy().reshape(-1)
    assert np.array_equal(out["rows"].cpu().numpy(), np.argsort(key, kind="stable"))
    counts = np.bincount(key, minlength=B * N)
    assert np.array_equal(out["off"].cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))


@pytest.mark.parametrize("layout", ["bcn", "nbc"])
@pytest.mark.parametrize("C", [0, 5])
@pytest.mark.parametrize("bf16", [False, True])
def test_group_bwd_csr(cuda, C, layout, bf16):
    """the gather-form backward through the inverse index, fp32 rows (3 + C wide) and bf16 rows
    of stride 8 past their width; every feature gradient element written"""
    _, _, idx, _, st, _ = _scene(C, layout, 5)
    off, rows = _inverse(cuda, idx)
    g = torch.randn(B * M * S, 3 + C, generator=_gen(C, 5))
    ldg = 3 + C + (8 - (3 + C) % 8) % 8 + 8              # a multiple of 8 (the 16-byte chunk kernel)
    specs = {"g": In(g.to(BF), ld=ldg) if bf16 else In(g), "off": In(off, index=(0, B * M * S)),
             "rows": In(rows, index=(0, B * M * S - 1)), "gf": _grad_out(C)}

    def call(t):
        if bf16:
            guard.call("ov3d_group_bwd_csr_bf16", t["g"], ldg, t["off"], t["rows"], B, C, N, *st,
                       t["gf"], like=t["g"])
        else:
            guard.call("ov3d_group_bwd_csr", t["g"], t["off"], t["rows"], B, C, N, *st, t["gf"],
                       like=t["g"])
    out = guard.run_case(cuda, specs, call)["gf"]
    if C:
        gr = g.to(BF).float() if bf16 else g
        assert torch.equal(_as_bcn(out.cpu(), layout, C), _feature_grad_ref(gr, idx, C))
    else:
        assert bool(torch.isnan(out).all())


def test_gather_fwd_bwd(cuda):
    Bg, C, Ng, Mg = 2, 3, 10, 4
    g = _gen(Bg, C, Ng, Mg)
    f = torch.randn(Bg, C, Ng, generator=g)
    idx = torch.stack([torch.randperm(Ng, generator=g)[:Mg] for _ in range(Bg)]).int()
    gout = torch.randn(Bg, C, Mg, generator=g)
    gi = idx.long()[:, None].expand(Bg, C, Mg)
    specs = {"f": In(f), "idx": In(idx, index=(0, Ng - 1)), "out": Out((Bg, C, Mg), F32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_gather_fwd", t["f"], t["idx"], Bg, C, Ng, Mg, t["out"], like=t["f"]))["out"]
    assert torch.equal(out.cpu(), torch.gather(f, 2, gi))
    specs = {"g": In(gout), "idx": In(idx, index=(0, Ng - 1)), "gf": Out((Bg, C, Ng), F32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_gather_bwd", t["g"], t["idx"], Bg, C, Ng, Mg, t["gf"], like=t["g"]))["gf"]
    assert torch.equal(out.cpu(), torch.zeros(Bg, C, Ng).scatter_add_(2, gi, gout))
