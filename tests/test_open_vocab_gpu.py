"""Open-vocabulary classification on the GPU (csrc/openvocab.hip behind
include/ov3d_openvocab.h) against the float64 restatement (tests/open_vocab_ref.py): exact
integer cases at the shapes where the tiling can go wrong, in every dtype and both layouts;
rounded cases inside the derived bar; the special rows; layout independence bit for bit; the
back-projected route against classify_rows over compose_features; the guard-band cases
(tests/guard.py); the launch census and a hipGraph capture (a synchronisation raises there)."""
import functools

import numpy as np
import pytest
import torch

import backproj_cases as BC
import guard
import open_vocab_ref as R
from guard import In, Out
from helpers import ov3d  # noqa: F401

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_openvocab_classify",)

F_PLANES, P_PLANES = 3, 32 * 41
DT = list(R.DTYPES)


def host(t):
    return t.cpu().numpy()


def run(OV, cuda, feat, text, layout, **kw):
    """feat (R, C) tensor on the host, as rows or as (F, C, 32, 41) planes -> host arrays"""
    if layout == "planes":
        planes = feat.view(F_PLANES, P_PLANES, -1).transpose(1, 2).contiguous().view(F_PLANES, -1, 32, 41)
        out = OV.classify_frames(planes.to(cuda), text.to(cuda), **kw)
        assert all(o.shape == (F_PLANES, 32, 41) for o in out)
    else:
        out = OV.classify_rows(feat.to(cuda), text.to(cuda), **kw)
    label, score, norm = (host(o).reshape(-1) for o in out)
    assert label.dtype == np.int32 and score.dtype == np.float32 and norm.dtype == np.float32
    return label, score, norm


@pytest.fixture(scope="module")
def OV(ov3d):
    from ov3d_amd import open_vocab
    return open_vocab


# ---------------------------------------------------------------- exact cases

@functools.lru_cache(maxsize=None)
def exact_ref(Rr, C, T):
    feat, text = R.exact_case(Rr, C, T)
    return feat, text, R.classify(feat, text)


# R around the 16-row wave tile and the 64-row workgroup, C around the 128-byte chunk of either
# element size (and 520 = 16 * 32 + 8), T in every accumulator count (1, 2, 16 tiles) and ragged
EXACT = [(1, 1, 1), (63, 8, 5), (64, 96, 19), (65, 512, 200), (1000, 96, 256), (1000, 520, 19), (65, 13, 3),
         (1000, 512, 40)]


@pytest.mark.parametrize("layout", ["rows", "planes"])
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("Rr,C,T", EXACT)
def test_exact_cases_equal_float64(cuda, OV, Rr, C, T, name, layout):
    Rr = F_PLANES * P_PLANES if layout == "planes" else Rr
    feat, text, ref = exact_ref(Rr, C, T)
    dtype = R.DTYPES[name]
    label, score, norm = run(OV, cuda, torch.from_numpy(feat).to(dtype),
                             OV.prepare_text(text, dtype, normalize=False), layout)
    assert np.array_equal(label, ref["label"])
    assert np.array_equal(score.astype(np.float64), ref["score"])
    # the float32 sum of squares is exact and the root correctly rounded
    assert np.array_equal(norm, np.sqrt(ref["n2"]).astype(np.float32))
    assert np.array_equal(np.rint(norm.astype(np.float64) ** 2), ref["n2"])
    if T >= 200 and Rr >= 1000:
        s = ref["s"]
        assert ((s == s.max(1, keepdims=True)).sum(1) > 1).any()       # ties were there to be broken


# ---------------------------------------------------------------- rounded cases

@functools.lru_cache(maxsize=None)
def rounded_ref(family, name, T):
    from ov3d_amd import open_vocab as OV
    dtype = R.DTYPES[name]
    feat, text = getattr(R, family + "_case")(4096, 512, T)
    ft, fv = R.rounded(feat, dtype)
    tt = OV.prepare_text(text, dtype)
    return ft, tt, R.classify(fv, tt.to(torch.float64).numpy())


@pytest.mark.parametrize("T", [19, 200])
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("family", ["normal", "prototype"])
def test_rounded_cases_stay_inside_the_derived_bar(cuda, OV, family, name, T):
    C = 512
    ft, tt, ref = rounded_ref(family, name, T)
    label, score, norm = run(OV, cuda, ft, tt, "rows")
    rows = np.arange(len(label))
    assert ((label >= 0) & (label < T)).all()
    err = np.abs(score.astype(np.float64) - ref["s"][rows, label])
    bar = R.eps(C) * ref["absdot"][rows, label]
    n2 = norm.astype(np.float64) ** 2
    skip = R.excluded(ref, C)
    print(f"{family} {name} T={T}: score error / bar max {np.max(err / bar):.3g}, norm^2 rel error "
          f"{np.max(np.abs(n2 - ref['n2']) / ref['n2']):.3g} (bar {R.eps(C):.3g}), excluded {100 * skip.mean():.2f} %, "
          f"labels differing outside {(label != ref['label'])[~skip].sum()}")
    assert (err <= bar).all()
    assert (np.abs(n2 - ref["n2"]) <= R.eps(C) * ref["n2"]).all()
    assert skip.mean() <= R.EXCLUDED_CAP and (family == "normal" or not skip.any())
    assert np.array_equal(label[~skip], ref["label"][~skip])


# ---------------------------------------------------------------- special rows

@pytest.mark.parametrize("layout", ["rows", "planes"])
@pytest.mark.parametrize("name", DT)
def test_special_rows(cuda, OV, name, layout):
    dtype = R.DTYPES[name]
    Rr, C, T = F_PLANES * P_PLANES, 40, 5
    feat, text = R.exact_case(Rr, C, T, seed=1)
    text[:, :2] = np.abs(text[:, :2]) + 1.0            # positive in channels 0 and 1
    zero, nan, inf, neg = [3, 64, 1311, 1312, Rr - 1], [10, 70], [11, 2000], [12, 130]
    feat[zero] = 0.0
    feat[3, 5] = -0.0
    feat[nan, 7] = np.nan
    feat[inf, 0], feat[inf, 1] = np.inf, -np.inf       # inf - inf in every product
    feat[neg] = 0.0
    feat[neg, 0] = -np.inf                             # every product -inf: the first one wins
    ft = torch.from_numpy(feat).to(dtype)
    ref = R.classify(feat, text)
    assert (ref["label"][zero + nan + inf] == T).all() and (ref["label"][neg] == 0).all()
    label, score, norm = run(OV, cuda, ft, OV.prepare_text(text, dtype, normalize=False), layout)
    assert np.array_equal(label, ref["label"])
    assert np.array_equal(score.astype(np.float64), ref["score"])
    assert not score[zero + nan + inf].any() and not np.signbit(score[zero + nan + inf]).any()
    assert not norm[zero].any() and np.isnan(norm[nan]).all() and np.isinf(norm[inf + neg]).all()
    # another unseen value; the other rows do not change
    label7, score7, _ = run(OV, cuda, ft, OV.prepare_text(text, dtype, normalize=False), layout, unseen=-7)
    assert (label7[zero + nan + inf] == -7).all() and np.array_equal(label7 == -7, label == T)
    assert np.array_equal(score7, score)
    # one NaN product among finite ones never wins: class 2 would have won most rows
    big = text.copy()
    big[2] = 3.0 * np.sign(feat[100])
    big[2, :2] = 3.0
    assert (R.classify(feat, big)["label"] == 2).sum() > Rr // 10
    big[2, 9] = np.nan
    ref = R.classify(feat, big)
    label, score, _ = run(OV, cuda, ft, OV.prepare_text(big, dtype, normalize=False), layout)
    assert (label != 2).all() and np.array_equal(label, ref["label"])
    assert np.array_equal(score.astype(np.float64), ref["score"])


@pytest.mark.parametrize("name", DT)
def test_min_sim_flips_the_rows_below_the_cosine(cuda, OV, name):
    C, T = 512, 19
    ft, tt, ref = rounded_ref("prototype", name, T)
    rows = np.arange(len(ft))
    plain = run(OV, cuda, ft, tt, "rows")
    cos = ref["score"] / np.sqrt(ref["n2"])
    tau = float(np.float32(np.median(cos)))
    label, score, norm = run(OV, cuda, ft, tt, "rows", min_sim=tau)
    assert np.array_equal(score, plain[1]) and np.array_equal(norm, plain[2])
    # score < tau * norm is decided on float32 values inside the bar of each side
    slack = R.eps(C) * (ref["absdot"][rows, ref["label"]] + 2 * tau * np.sqrt(ref["n2"]))
    clear = np.abs(ref["score"] - tau * np.sqrt(ref["n2"])) > slack
    below = cos < tau
    assert clear.mean() > 0.95 and below[clear].sum() > 100 and (~below[clear]).sum() > 100
    assert (label[clear & below] == T).all()
    assert np.array_equal(label[clear & ~below], plain[0][clear & ~below])
    assert np.array_equal(label[~(label == T)], plain[0][~(label == T)])
    low = run(OV, cuda, ft, tt, "rows", min_sim=-1.0, unseen=-1)
    assert np.array_equal(low[0], plain[0])


# ---------------------------------------------------------------- layout independence

@pytest.mark.parametrize("C,T", [(200, 19), (13, 3), (64, 200)])
@pytest.mark.parametrize("name", DT)
def test_a_row_depends_on_its_values_alone(cuda, OV, name, C, T):
    """the same vectors as rows, as planes, as rows in another order, and as rows at an address
    that rules out 16-byte loads: label, score and norm bit for bit"""
    dtype = R.DTYPES[name]
    Rr = F_PLANES * P_PLANES
    feat, text = R.normal_case(Rr, C, T, seed=7)
    feat[::97] = 0.0
    feat[5::211, 3] = np.nan
    ft, tt = R.rounded(feat, dtype)[0], OV.prepare_text(text, dtype)
    base = run(OV, cuda, ft, tt, "rows")
    bits = lambda out: [o.view(np.int32) for o in out]                     # noqa: E731
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))   # noqa: E731
    assert same(run(OV, cuda, ft, tt, "planes"), base)
    perm = np.random.default_rng(1).permutation(Rr)
    moved = run(OV, cuda, ft[torch.from_numpy(perm)], tt, "rows")
    assert same(moved, [o[perm] for o in base])
    shifted = torch.empty(Rr * C + 1, dtype=dtype, device=cuda)
    shifted[1:] = ft.to(cuda).view(-1)
    tshift = torch.empty(T * C + 1, dtype=dtype, device=cuda)
    tshift[1:] = tt.to(cuda).view(-1)
    out = OV.classify_rows(shifted[1:].view(Rr, C), tshift[1:].view(T, C))
    assert same([host(o) for o in out], base)
    # and a few of them alone, one row per launch
    for r in (0, 97, 216, Rr - 1):
        one = OV.classify_rows(ft[r:r + 1].to(cuda), tt.to(cuda))
        assert same([host(o) for o in one], [o[r:r + 1] for o in base])
    assert (base[0] == T).sum() >= Rr // 97 and len(np.unique(base[0])) >= min(T, 3)


# ---------------------------------------------------------------- the back-projected route

@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_vertex_labels_equal_classified_composed_features(cuda, OV, name):
    from ov3d_amd import _native, projection
    dtype = R.DTYPES[name]
    case = BC.case("edges")
    F, C, T = len(case["poses"]), 24, 7
    rng = np.random.default_rng(11)
    feats = R.rounded(rng.standard_normal((F, C, 32, 41)), dtype)[0].to(cuda)
    text = OV.prepare_text(rng.standard_normal((T, C)), dtype, device=cuda)
    geo = [torch.from_numpy(case[k]).to(cuda) for k in ("points", "depth", "poses")]
    composed, frame = projection.compose_features(*geo, feats, rows=True)
    want = OV.classify_rows(composed, text)[0]
    _native.census_start()
    label, got_frame = OV.vertex_labels_from_frames(*geo, feats, text)
    census = _native.census_stop()
    assert census == {"ov3d_openvocab_classify": 1, "ov3d_backproj_compose": 1}
    assert label.dtype == torch.int32 and got_frame.dtype == torch.int32
    assert torch.equal(label, want) and torch.equal(got_frame, frame)
    none = host(frame) < 0
    assert 0 < none.sum() < len(none) and (host(label)[none] == T).all() and (host(label)[~none] < T).all()
    assert len(np.unique(host(label)[~none])) == T
    # another unseen, and a cosine floor, go the same way
    want = OV.classify_rows(composed, text, unseen=-100, min_sim=0.3)[0]
    label, _ = OV.vertex_labels_from_frames(*geo, feats, text, unseen=-100, min_sim=0.3)
    assert torch.equal(label, want) and 0 < (host(label)[~none] == -100).sum() < (~none).sum()


# ---------------------------------------------------------------- guard bands

# ragged R, C and T; 16-byte rows that take the vector loads; P not a multiple of 64
GUARD = [("rows", 65, 13, 3, 0), ("rows", 1, 1, 1, 0), ("rows", 130, 40, 17, 0), ("rows", 65, 72, 33, 0),
         ("planes", 3 * 37, 13, 3, 37), ("planes", 2 * 100, 5, 19, 100), ("planes", 1, 3, 2, 1)]


@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("layout,Rr,C,T,P", GUARD)
def test_guard_classify(cuda, ov3d, layout, Rr, C, T, P, name):
    dtype = R.DTYPES[name]
    feat, text = R.exact_case(Rr, C, T, seed=2)
    ref = R.classify(feat, text)
    data = R.to_planes(feat, Rr // P, P) if P else feat
    specs = {"feat": In(torch.from_numpy(data).to(dtype)), "text": In(torch.from_numpy(text).to(dtype)),
             "label": Out((Rr,), torch.int32), "score": Out((Rr,), torch.float32), "norm": Out((Rr,), torch.float32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_openvocab_classify", t["feat"], {"f32": 0, "bf16": 1, "f16": 2}[name], int(P > 0), Rr, C, P, t["text"],
        T, T, t["label"], t["score"], t["norm"], like=t["feat"]))
    assert np.array_equal(host(out["label"]), ref["label"])
    assert np.array_equal(host(out["score"]).astype(np.float64), ref["score"])
    assert np.array_equal(host(out["norm"]), np.sqrt(ref["n2"]).astype(np.float32))


@pytest.mark.parametrize("bad", [dict(R=0), dict(C=0), dict(C=4097), dict(T=0), dict(T=257), dict(dtype=3),
                                 dict(planes=2), dict(planes=1, P=64), dict(planes=1, P=0)])
def test_guard_rejected_calls_write_nothing(cuda, ov3d, bad):
    Rr, C, T = 65, 13, 3
    feat, text = R.exact_case(Rr, C, T)
    a = dict(R=Rr, C=C, T=T, dtype=0, planes=0, P=0)
    a.update(bad)
    specs = {"feat": In(torch.from_numpy(feat).float()), "text": In(torch.from_numpy(text).float()),
             "label": Out((Rr,), torch.int32), "score": Out((Rr,), torch.float32), "norm": Out((Rr,), torch.float32)}
    guard.run_case(cuda, specs, lambda t: guard.raw_call(
        "ov3d_openvocab_classify", t["feat"], a["dtype"], a["planes"], a["R"], a["C"], a["P"], t["text"], a["T"], 0,
        t["label"], t["score"], t["norm"], like=t["feat"]), expect_reject=True)


# ---------------------------------------------------------------- launches

def test_one_launch_each_and_nothing_synchronises(cuda, OV):
    """the census of entry calls, and all three drivers inside a hipGraph capture, where a
    synchronisation or a read-back raises; the replay gives the eager results"""
    from ov3d_amd import _native
    case = BC.case("edges")
    F, C, T = len(case["poses"]), 24, 7
    rng = np.random.default_rng(12)
    feats = torch.from_numpy(rng.standard_normal((F, C, 32, 41))).to(torch.bfloat16).to(cuda)
    rows = torch.from_numpy(rng.standard_normal((333, C))).to(torch.bfloat16).to(cuda)
    text = OV.prepare_text(rng.standard_normal((T, C)), torch.bfloat16, device=cuda)
    geo = [torch.from_numpy(case[k]).to(cuda) for k in ("points", "depth", "poses")]

    def all_three():
        return (OV.classify_rows(rows, text, min_sim=0.1) + OV.classify_frames(feats, text, unseen=-1)
                + OV.vertex_labels_from_frames(*geo, feats, text, min_sim=0.1))

    _native.census_start()
    OV.classify_rows(rows, text, min_sim=0.1)
    assert _native.census_stop() == {"ov3d_openvocab_classify": 1}
    _native.census_start()
    OV.classify_frames(feats, text)
    assert _native.census_stop() == {"ov3d_openvocab_classify": 1}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture
        eager = [t.clone() for t in all_three()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = all_three()
    for t in got:
        t.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert len(got) == 8
    for g, e in zip(got, eager):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                           e.view(torch.int32) if e.dtype == torch.float32 else e)
