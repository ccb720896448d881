"""Pseudo-box lifting without a GPU: the numpy restatement (tests/lift_ref.py) against what the
reference's lift_boxes.py scripts recorded (tests/golden/lift_boxes.npz): the saved arrays bit
for bit, the lifted boxes within the bound derived below; the closed form of the pool match
against the sequential loop; the product's host side (planes, edge filter, label conversion,
limits, to_training_format); and the argument validation of every entry of
include/ov3d_lift.h, which happens before any launch.

The bound on a lifted coordinate.  The reference forms each coordinate as a dot product of at
most 4 terms through BLAS (summation order and fusing unspecified), ScanNet chains two such
maps; the restatement and the device sum in a fixed order.  To first order both differ from
the exact value by at most 4 * 2^-53 * s per map, s = max_i(sum_j |M_ij| max|p_j| + |t_i|), so
two results differ by at most 8 * 2^-53 * s; the bar is 4 times that, computed from each
case's own matrices and points."""
import ctypes
import os

import numpy as np
import pytest

import lift_cases as LC
import lift_ref as R
from helpers import ROOT, ov3d  # noqa: F401

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lift_boxes.npz"))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def map_scale(M, t, p):
    return float(np.max(np.abs(M) @ np.abs(p).max(0) + np.abs(t)))


def scannet_bar(case):
    A = case["axis_align_matrix"]
    Ainv = np.linalg.inv(A)
    orig = R.affine(Ainv, case["points"])
    s = max(map_scale(Ainv[:3, :3], Ainv[:3, 3], case["points"]), map_scale(A[:3, :3], A[:3, 3], orig))
    return 4 * 8 * 2.0 ** -53 * s


def sun_bar(case):
    H, W = case["depth"].shape
    v, u = np.indices((H, W))
    d = case["depth"].astype(np.float64)
    K = case["K"]
    p = np.stack([(u - K[0, 2]) * d / K[0, 0], d, (v - K[1, 2]) * d / K[1, 1]], -1).reshape(-1, 3)
    return 4 * 8 * 2.0 ** -53 * map_scale(case["Rtilt"], np.zeros(3), p)


def check_lifted(got, want, bar):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    if len(want):
        assert same(got[:, 6:], want[:, 6:])
        err = np.abs(got[:, :6] - want[:, :6]).max()
        print("lifted boxes: max error %.3e, bar %.3e" % (err, bar))
        assert err <= bar


@pytest.fixture(scope="module")
def scannet_results():
    """every ScanNet case through the restatement, once"""
    return {n: R.scannet_scan(**LC.scannet_case(n)) for n in LC.SCANNET_CASES}


@pytest.mark.parametrize("name", LC.SCANNET_CASES)
def test_restatement_equals_the_scannet_recording(scannet_results, name):
    final, lifted = scannet_results[name]
    assert same(final, GOLD[f"scannet/{name}/final"]), name
    check_lifted(lifted, GOLD[f"scannet/{name}/lifted"], scannet_bar(LC.scannet_case(name)))


@pytest.mark.parametrize("name", LC.SUN_CASES)
def test_restatement_equals_the_sun_recording(name):
    case = LC.sun_case(name)
    final, lifted = R.sun_scan(**case)
    assert same(final, GOLD[f"sun/{name}/final"]), name
    check_lifted(lifted, GOLD[f"sun/{name}/lifted"], sun_bar(case))


def test_the_recording_is_not_trivial():
    main = GOLD["scannet/main/final"]
    assert main.shape[1] == 10 and main.shape[0] >= 2
    assert GOLD["scannet/main/lifted"].shape[0] > main.shape[0]
    assert GOLD["scannet/nothing_lifted/final"].shape == (0, 7)
    assert GOLD["scannet/nothing_matched/final"].shape == (0, 10)
    assert GOLD["sun/nothing_lifted/final"].shape == (0, 8) and GOLD["sun/main/final"].shape[0] >= 2


def random_match_case(seed, M, P):
    """boxes around a few shared centres so that several lifted boxes share an argmax; scores
    with ties, zeros and negatives"""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.uniform(-2, 2, (max(2, P // 3), 3))
    c = centres[rng.integers(0, len(centres), M)] + rng.normal(0, 0.05, (M, 3))
    half = rng.uniform(0.2, 0.5, (M, 3))
    score = rng.choice([-0.5, 0.0, 0.25, 0.5, 0.5, 0.75, 0.9], M) if seed % 2 else rng.random(M) - 0.2
    boxes = np.concatenate([c - half, c + half, score[:, None],
                            rng.integers(0, 3, (M, 1)).astype(float)], 1)
    pc = np.concatenate([centres[rng.integers(0, len(centres), P - P // 4)] + rng.normal(0, 0.08, (P - P // 4, 3)),
                         rng.uniform(5, 9, (P // 4, 3))])
    pool = np.concatenate([pc, rng.uniform(0.4, 1.1, (P, 3)), np.zeros((P, 1))], 1)
    return boxes, pool


@pytest.mark.parametrize("seed", range(8))
def test_closed_form_of_the_match_equals_the_sequential_loop(seed):
    M, P = (5, 3) if seed == 0 else (40 + 7 * seed, 12 + 5 * seed)
    boxes, pool = random_match_case(seed, M, P)
    vv = R.pool_vv(pool)
    picks = R.nms(boxes, 0.7)
    assert (np.diff(boxes[picks, 6]) <= 0).all()           # pick order is score-descending
    for match in (0.3, 0.0, 0.05):
        label, score = R.match_loop(boxes, picks, vv, match)
        amax, maxiou, owner = R.match_closed(boxes, picks, vv, match)
        got_label = np.where(owner >= 0, boxes[np.maximum(owner, 0), 7], -100.0)
        got_score = np.where(owner >= 0, boxes[np.maximum(owner, 0), 6], 0.0)
        assert same(got_label, label) and same(got_score, score), (seed, match)
        if seed % 2:                                       # ties and non-positive scores took part
            assert (owner >= 0).any() and (label == -100).any()
            assert (boxes[picks, 6] <= 0).any() and len(set(boxes[picks, 6])) < len(picks)


def test_product_planes_and_edge_filter_equal_the_restatement():
    from ov3d_amd import lift_boxes as LB
    case = LC.scannet_case("main")
    planes, sl, plabel = LB.scannet_host_plan(case["intrinsic"], case["poses"], case["boxes2d"])
    rp, rsl, rlab = R.scannet_plan(case["intrinsic"], case["poses"], case["boxes2d"])
    assert planes.shape == (sum(len(b) for b in case["boxes2d"]) - 2, 24)
    assert np.array_equal(planes, rp, equal_nan=True) and same(sl, rsl)
    assert np.array_equal(plabel, rlab) and plabel.dtype == np.int32
    assert np.isnan(planes).any()                          # the -inf pose and the zero-width box
    assert case["intrinsic"][0, 0] == np.float32(LC.FX)    # the caller's intrinsic is not halved in place
    boxes = np.array([[0, 1, 5, 5, 1, 0], [1, 0, 5, 5, 1, 0], [1, 1, 319, 5, 1, 0], [1, 1, 5, 239, 1, 0],
                      [1, 1, 5, 5, 1, 0]], dtype=np.float64)
    assert same(LB.edge_filter(boxes, (240, 320)), boxes[4:])
    assert same(R.not_on_edge(boxes, (240, 320)), boxes[4:])


def test_label_conversion_and_limits():
    from ov3d_amd import lift_boxes as LB
    lab = LB._int_labels(np.array([0.0, 17.0, -100.0, 2.5, np.nan, np.inf, 1e12]), LB._NEVER_POINT)
    assert lab.tolist() == [0, 17, -100] + [LB._NEVER_POINT] * 4
    assert LB._int_labels(np.array([3, -100], np.int64), LB._NEVER_POINT).tolist() == [3, -100]
    b = np.zeros((4, 6))
    b[:, 5] = [2.0, 2.9, -0.5, np.nan]
    assert LB._box_labels(b).tolist() == [2, 2, 0, LB._NEVER_BOX]
    many = np.tile([[5.5, 5.5, 10.0, 10.0, 0.5, 3.0]], (LB.MAX_PER_CLASS + 1, 1))
    many[:, 4] = np.linspace(0.1, 0.9, len(many))
    with pytest.raises(ValueError, match="one class"):
        LB._check_counts(LB._box_labels(many))
    with pytest.raises(ValueError, match="at most"):
        LB._check_counts(np.arange(LB.MAX_BOXES + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="finite"):
        LB._check_boxes(np.array([[1, 1, 2, 2, np.nan, 0.0]]))
    with pytest.raises(ValueError, match="float"):
        LB._check_boxes(np.zeros((2, 6), np.int64))
    with pytest.raises(ValueError, match="gss_pool"):
        LB._pool(np.zeros((0, 7)))


def test_to_training_format():
    from ov3d_amd import lift_boxes as LB
    final = GOLD["scannet/main/final"]
    out = LB.to_training_format(final)
    assert out.shape == (len(final), 7) and same(out[:, :6], final[:, :6])
    assert out[:, 6].tolist() == [float(R.NYU40[int(c)]) for c in final[:, 6]]
    assert same(out, R.training_format(final))
    assert same(final, GOLD["scannet/main/final"])         # the input is left alone
    assert LB.to_training_format(np.zeros((0, 10))).shape == (0, 7)
    with pytest.raises(ValueError):
        LB.to_training_format(np.zeros((2, 6)))


def test_module_needs_no_image_decoder():
    """importing the module pulls in neither PIL nor imageio"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import ov3d_import; ov3d_import.load(); "
            "import ov3d_amd.lift_boxes; assert 'PIL' not in sys.modules and 'imageio' not in sys.modules" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_entries_reject_invalid_arguments():
    """every entry of include/ov3d_lift.h validates before any launch (no device needed)"""
    from ov3d_amd import _native
    lib = _native.load()
    with open(os.path.join(ROOT, "include", "ov3d_lift.h")) as f:
        protos = _native.read_header(f.read())[1]
    assert set(_native.HEADER_EXPORTS["ov3d_lift.h"]) == set(protos) == {
        "ov3d_lift_frustum", "ov3d_lift_image", "ov3d_lift_nms", "ov3d_lift_match"}
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first

    ok = dict(pts=p, f64=1, N=4, labels=p, A=p, Ainv=p, planes=p, plabel=p, M=2, ws=p, lohi=p, ld=8, count=p)

    def frustum(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_lift_frustum(a["pts"], a["f64"], a["N"], a["labels"], a["A"], a["Ainv"], a["planes"],
                                     a["plabel"], a["M"], a["ws"], a["lohi"], a["ld"], a["count"], None)
    for name in ("pts", "labels", "A", "Ainv", "planes", "plabel", "ws", "lohi", "count"):
        assert frustum(**{name: None}) == -1, name
    assert frustum(f64=2) == -1 and frustum(N=0) == -1 and frustum(M=0) == -1 and frustum(ld=5) == -1

    ok = dict(depth=p, f64=0, seg=p, lut=p, lut_n=37, H=4, W=5, boxes=p, plabel=p, k=1, calib=p, lohi=p,
              ld=6, count=p)

    def image(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_lift_image(a["depth"], a["f64"], a["seg"], a["lut"], a["lut_n"], a["H"], a["W"],
                                   a["boxes"], a["plabel"], a["k"], a["calib"], a["lohi"], a["ld"],
                                   a["count"], None)
    for name in ("depth", "seg", "boxes", "plabel", "calib", "lohi", "count"):
        assert image(**{name: None}) == -1, name
    assert image(f64=-1) == -1 and image(H=0) == -1 and image(W=0) == -1 and image(k=0) == -1
    assert image(ld=5) == -1 and image(lut_n=0) == -1 and image(lut=None) == -1    # lut_n without a table
    assert image(H=1 << 16, W=1 << 16) == -1

    def nms(boxes=p, ld=8, K=3, valid=None, size=0, thresh=0.7, rank=p, keep=p):
        return lib.ov3d_lift_nms(boxes, ld, K, valid, size, thresh, rank, keep, None)
    assert nms(boxes=None) == -1 and nms(rank=None) == -1 and nms(keep=None) == -1
    assert nms(K=-1) == -1 and nms(K=8193) == -1 and nms(ld=7) == -1 and nms(size=1) == -1   # ld 8 < 9
    assert nms(size=2) == -1 and nms(thresh=float("nan")) == -1
    assert nms(K=0) == 0                                   # nothing to do, nothing launched

    ok = dict(boxes=p, ld=8, rank=p, M=2, pool=p, P=3, match=0.3, owner=p, amax=p, maxiou=p, win=p, rows=p,
              out=p)

    def match(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_lift_match(a["boxes"], a["ld"], a["rank"], a["M"], a["pool"], a["P"], a["match"],
                                   a["owner"], a["amax"], a["maxiou"], a["win"], a["rows"], a["out"], None)
    for name in ("boxes", "rank", "pool", "owner", "amax", "maxiou", "win", "rows", "out"):
        assert match(**{name: None}) == -1, name
    assert match(ld=7) == -1 and match(M=0) == -1 and match(P=0) == -1 and match(match=float("nan")) == -1
