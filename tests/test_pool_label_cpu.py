"""Pool labelling and pseudo-label assessment without a GPU: the numpy restatement of the two
entries (tests/pool_label_ref.py) against what the reference's own `labeling` and `match`
recorded (tests/golden/pool_label.npz), through the product's host side (ov3d_amd.pool_label,
ov3d_amd.label_assess) with the restatement standing in for the launches: the files byte for
byte, the three result shapes, replace=False, the (count, total) pairs; every ValueError; the
export set of include/ov3d_poollabel.h; and the argument validation of both entries, which
happens before any launch."""
import ctypes
import os

import numpy as np
import pytest

import pool_label_cases as PC
import pool_label_ref as R
from helpers import ROOT, ov3d  # noqa: F401

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pool_label.npz"))
SCAN = "scene0000_00"


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture
def host(monkeypatch):
    """the two modules with the restatement in place of the device"""
    from ov3d_amd import label_assess as LA, pool_label as PL
    monkeypatch.setattr(PL, "vote_group", R.vote_group)
    monkeypatch.setattr(LA, "_group", R.group)
    return PL, LA


@pytest.mark.parametrize("name", PC.LABEL_CASES + PC.SHAPE_CASES)
def test_restatement_equals_the_recorded_files(host, name, tmp_path):
    PL, _ = host
    case = PC.label_case(name)
    want = GOLD["label/" + name]
    assert same(PL.label_pool(case["points"], case["labels"], case["pool"]), want)
    vert_dir, label_dir, pool_dir = PC.write_label_tree(case, str(tmp_path), SCAN)
    out_dir = str(tmp_path / "out")
    labeler = PL.PoolLabeler(vert_dir, label_dir, pool_dir, out_dir)
    assert labeler.labeling(SCAN) == len(want)
    assert same(np.load(os.path.join(out_dir, SCAN + "_bbox.npy")), want)
    # the pool, the vertices and the labels are left as they were
    again = PC.label_case(name)
    assert all(same(case[k], again[k]) for k in case)


def test_the_recording_is_not_trivial():
    assert GOLD["label/none"].shape == (0, 7) and GOLD["label/one"].shape == (1, 7)
    for name in PC.LABEL_CASES:
        got = GOLD["label/" + name]
        assert len(got) >= 2 and np.isin(got[:, 6], PC.NYU40).all() and len(np.unique(got[:, 6])) >= 3
        assert (got[:, 6] == 4).any()                      # the tie of 4 and 5
    for name in PC.ASSESS_CASES:
        count, total = GOLD["assess/" + name]
        assert 0 < count < total


def test_a_float32_comparison_would_write_another_file(host):
    """the bound one float64 ulp from a float32 vertex: rounding the bounds to float32 keeps two
    more boxes"""
    PL, _ = host
    case = PC.label_case("f32")
    scan = PL._scan(case["points"], case["labels"], case["pool"], "f32")
    rounded = scan[2].copy()
    rounded[:, :6] = rounded[:, :6].astype(np.float32)
    kept = lambda b: int(np.isin(R.vote_group([(scan[0], scan[1], b)])[0], PC.NYU40).sum())     # noqa: E731
    assert kept(scan[2]) == len(GOLD["label/f32"]) and kept(rounded) == len(GOLD["label/f32"]) + 2


def test_run_groups_scans_and_respects_replace(host, tmp_path, monkeypatch):
    PL, _ = host
    names = []
    for i, name in enumerate(("f32", "none", "f64", "one", "f32")):
        scan = f"scene{i:04d}_00"
        dirs = PC.write_label_tree(PC.label_case(name), str(tmp_path), scan)
        names.append((scan, name))
    out_dir = str(tmp_path / "out")
    groups = []
    monkeypatch.setattr(PL, "vote_group", lambda scans, device="cuda": (groups.append(len(scans)),
                                                                      R.vote_group(scans))[1])
    labeler = PL.PoolLabeler(*dirs, out_dir, group=2)
    counts = labeler.run([s for s, _ in names])
    assert counts == [len(GOLD["label/" + n]) for _, n in names] and groups == [2, 2, 1]
    for scan, name in names:
        assert same(np.load(os.path.join(out_dir, scan + "_bbox.npy")), GOLD["label/" + name])
    # replace=False: an existing file is counted, not recomputed, whatever it holds
    np.save(os.path.join(out_dir, names[0][0] + "_bbox.npy"), np.zeros((5, 7)))
    del groups[:]
    assert labeler.labeling(names[0][0], replace=False) == 5 and groups == []
    os.remove(os.path.join(out_dir, names[2][0] + "_bbox.npy"))
    assert labeler.run([s for s, _ in names], replace=False) == [5] + counts[1:] and groups == [1]
    assert labeler.labeling(names[0][0]) == counts[0]


def test_label_pool_refusals(host, tmp_path):
    PL, _ = host
    case = PC.label_case("one")
    pts, lab, pool = case["points"], case["labels"], case["pool"]
    for bad in (-1, 64, 2.5, np.nan):
        labels = lab.astype(np.float64)
        labels[1] = bad
        with pytest.raises(ValueError, match="label_pool: per-vertex label"):
            PL.label_pool(pts, labels, pool)
    for bad in (np.nan, np.inf):
        boxes = pool.copy()
        boxes[2, 4] = bad
        with pytest.raises(ValueError, match="pool box 2 is not finite"):
            PL.label_pool(pts, lab, boxes)
    with pytest.raises(ValueError, match=r"\(P, 7\)"):
        PL.label_pool(pts, lab, pool[:, :6])
    with pytest.raises(ValueError, match="vertices"):
        PL.label_pool(pts.astype(np.float16), lab, pool)
    with pytest.raises(ValueError, match="one numeric label per vertex"):
        PL.label_pool(pts, lab[:-1], pool)
    # the file driver names the scan
    dirs = PC.write_label_tree(dict(case, labels=np.array([7, 7, 99])), str(tmp_path), SCAN)
    with pytest.raises(ValueError, match=SCAN + ": per-vertex label 99"):
        PL.PoolLabeler(*dirs, str(tmp_path / "out")).labeling(SCAN)
    # labels 41 .. 63 are accepted and vote, as in the reference (no detection class: dropped)
    assert PL.label_pool(pts, np.array([63, 63, 13]), pool).shape == (0, 7)
    with pytest.raises(ValueError, match="group"):
        PL.PoolLabeler(*dirs, str(tmp_path / "out"), group=0)


@pytest.mark.parametrize("name", PC.ASSESS_CASES)
def test_restatement_equals_the_recorded_agreement(host, name):
    _, LA = host
    case = PC.assess_case(name)
    want = tuple(GOLD["assess/" + name].tolist())
    assert LA.match(case["gt"], case["pseudo"]) == want
    conf = LA.frame_confusion(case["gt"].astype(np.uint8), case["pseudo"].astype(np.int64))
    assert conf.shape == (19, 19) and conf.dtype == np.int64 and conf.sum() == want[1]
    assert np.trace(conf) == want[0] and conf[18, 18] > 0
    assert (conf[:18].sum(1) > 0).all() and (conf[:, :18].sum(0) > 0).all()
    # the map is project_label(., False): nyu40ids[i] -> i, the rest ignored
    assert LA.GT_MAP[PC.NYU40].tolist() == list(range(18)) and (np.delete(LA.GT_MAP, PC.NYU40) == 18).all()


def test_assess_sums_the_scans(host, monkeypatch):
    _, LA = host
    cases = [PC.assess_case(n) for n in ("a", "b", "a", "a")]
    groups = []
    monkeypatch.setattr(LA, "_group", lambda frames, device: (groups.append(len(frames)), R.group(frames))[1])
    empty = (np.zeros((0, 24, 32), np.float32), np.zeros((0, 24, 32), np.int64))
    scans = [(f"s{i}", c["gt"], c["pseudo"]) for i, c in enumerate(cases)] + [("empty",) + empty]
    pairs, count, total, conf = LA.assess(iter(scans), group=2)
    want = [tuple(GOLD["assess/" + n].tolist()) for n in ("a", "b", "a", "a")] + [(0, 0)]
    assert pairs == want and groups == [1, 1, 2, 1]        # the frame size changes after "a" and after "b"
    assert (count, total) == (sum(c for c, _ in want), sum(t for _, t in want))
    assert isinstance(count, int) and isinstance(total, int)
    assert conf.dtype == np.int64 and conf.sum() == total and np.trace(conf) == count
    none = LA.assess([])
    assert none[:3] == ([], 0, 0) and not none[3].any()


def test_frame_refusals(host):
    _, LA = host
    case = PC.assess_case("b")
    gt, ps = case["gt"], case["pseudo"]
    for bad in (-1.0, 256.0, 3.5, np.nan):
        g = gt.copy()
        g[1, 2, 3] = bad
        with pytest.raises(ValueError, match="frame_confusion: ground-truth label"):
            LA.frame_confusion(g, ps)
    for bad in (-1, -99, 2.5, np.nan):
        p = ps.astype(np.float64)
        p[0, 4, 4] = bad
        with pytest.raises(ValueError, match="pseudo label"):
            LA.frame_confusion(gt, p)
    with pytest.raises(ValueError, match="s7: pseudo label"):
        LA.assess([("s7", gt, np.full(ps.shape, -5))])
    with pytest.raises(ValueError, match="one shape"):
        LA.frame_confusion(gt, ps[:, :-1])
    # ignored either way: >= 18 (as large as it likes) and -100
    p = ps.astype(np.int64)
    p[ps >= 18] = 1000
    assert np.array_equal(LA.frame_confusion(gt, p), LA.frame_confusion(gt, ps))


def test_exports_are_the_header():
    from ov3d_amd import _native
    with open(os.path.join(ROOT, "include", "ov3d_poollabel.h")) as f:
        protos = _native.read_header(f.read())[1]
    assert set(_native.HEADER_EXPORTS["ov3d_poollabel.h"]) == set(protos) == {
        "ov3d_poollabel_vote", "ov3d_poollabel_confusion"}
    lib = _native.load()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_entries_reject_invalid_arguments():
    """every entry of include/ov3d_poollabel.h validates before any launch (no device needed)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok = dict(pts=p, f64=0, ld=3, labels=p, pt_off=p, N=9, boxes=p, box_off=p, P=4, S=2, min_label=3, C=41,
              counts=p, mode=p)

    def vote(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_poollabel_vote(a["pts"], a["f64"], a["ld"], a["labels"], a["pt_off"], a["N"], a["boxes"],
                                       a["box_off"], a["P"], a["S"], a["min_label"], a["C"], a["counts"],
                                       a["mode"], None)
    for name in ("pts", "labels", "pt_off", "boxes", "box_off", "counts", "mode"):
        assert vote(**{name: None}) == -1, name
    assert vote(S=0) == -1 and vote(C=0) == -1 and vote(C=65) == -1 and vote(ld=2) == -1 and vote(f64=2) == -1
    assert vote(min_label=-1) == -1 and vote(min_label=42) == -1 and vote(N=-1) == -1 and vote(P=-1) == -1
    assert vote(N=1 << 31) == -1 and vote(P=1 << 31) == -1
    # N == 0 / P == 0 excuse their own pointers only
    assert vote(N=0, pts=None, labels=None, boxes=None) == -1 and vote(P=0, boxes=None, pt_off=None) == -1
    assert vote(P=0, boxes=None, counts=None, mode=None) == 0          # nothing to launch

    ok = dict(gt=p, pseudo=p, frame_off=p, F=3, HW=63, S=2, gt_map=p, K=18, conf=p)

    def confusion(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_poollabel_confusion(a["gt"], a["pseudo"], a["frame_off"], a["F"], a["HW"], a["S"],
                                            a["gt_map"], a["K"], a["conf"], None)
    for name in ("gt", "pseudo", "frame_off", "gt_map", "conf"):
        assert confusion(**{name: None}) == -1, name
    assert confusion(S=0) == -1 and confusion(K=0) == -1 and confusion(K=32) == -1 and confusion(HW=0) == -1
    assert confusion(F=-1) == -1 and confusion(F=1 << 31) == -1 and confusion(HW=1 << 31) == -1
    assert confusion(F=0, gt=None, pseudo=None, conf=None) == -1
