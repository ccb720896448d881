"""Multiview back-projection without a GPU: the numpy restatement (tests/backproj_ref.py) against
the reference's recorded tables and features (tests/golden/backproj.npz), the compose
definition over it, the export set of include/ov3d_backproj.h, and the margins of the stored
inputs."""
import os
import re

import numpy as np
import pytest

import backproj_cases as BC
import backproj_ref as R
from helpers import ROOT, ov3d  # noqa: F401

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "backproj.npz"))
PAR = R.params()


def gold(name):
    return {k: GOLD[name + "/" + k] for k in ("points", "depth", "poses", "features", "idx3d", "idx2d",
                                              "projected", "composed")}


def same(a, b):
    """same dtype, shape and bits"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name in BC.CASES:
        g = gold(name)
        out[name] = R.tables(g["points"], g["depth"], g["poses"], PAR)
    return out


def test_stored_inputs_are_the_cases():
    for name in BC.CASES:
        case, g = BC.case(name), gold(name)
        for k in ("points", "depth", "poses", "features"):
            assert same(case[k], g[k]), (name, k)


@pytest.mark.parametrize("name", BC.CASES)
def test_restatement_equals_the_recorded_tables(restated, name):
    g = gold(name)
    i3, i2 = restated[name]
    assert i3.dtype == np.int64 and i3.shape == (len(g["poses"]), len(g["points"]) + 1)
    assert np.array_equal(i3, g["idx3d"]) and np.array_equal(i2, g["idx2d"])
    if name == "main":
        assert (i3[:, 0] > 100).all()
    else:
        assert i3[0].sum() == 0 and i3[1].sum() == 0 and i2[:2].sum() == 0    # the reference's None
        both = np.intersect1d(i3[2, 1:1 + i3[2, 0]], i3[3, 1:1 + i3[3, 0]])
        assert len(both) > 0                                                   # two frames, one vertex


@pytest.mark.parametrize("name", BC.CASES)
def test_restatement_equals_the_recorded_features(restated, name):
    g = gold(name)
    i3, i2 = restated[name]
    N = len(g["points"])
    for f in range(len(g["poses"])):
        assert same(R.project(g["features"][f], i3[f], i2[f], N), g["projected"][f]), (name, f)
    assert R.project(g["features"][0][0], i3[0], i2[0], N).shape == (1, N)   # a 2-D label is C = 1


@pytest.mark.parametrize("name", BC.CASES)
def test_compose_definition_equals_the_recorded_composition(restated, name):
    g = gold(name)
    i3, i2 = restated[name]
    out, frame = R.compose_loop(g["features"], i3, i2, len(g["points"]))
    assert same(out, g["composed"])
    assert frame.dtype == np.int32
    mapped = np.zeros(len(g["points"]), bool)
    for f in range(len(i3)):
        idx = i3[f, 1:1 + i3[f, 0]]
        mapped[idx] = True
        later = np.zeros(len(mapped), bool)
        for h in range(f + 1, len(i3)):
            later[i3[h, 1:1 + i3[h, 0]]] = True
        assert (frame[idx][~later[idx]] == f).all()
    assert np.array_equal(frame >= 0, mapped) and not out[:, ~mapped].any()
    out2, frame2 = R.compose(g["points"], g["depth"], g["poses"], g["features"], PAR)
    assert same(out2, out) and same(frame2, frame)


@pytest.mark.parametrize("name", BC.CASES)
def test_margins_hold_on_the_stored_inputs(restated, name):
    g = gold(name)
    ev = BC.evaluate(g["points"], g["depth"], g["poses"], PAR)
    assert not ev["near"].any()
    i3, i2 = restated[name]
    for f in range(len(i3)):
        idx = np.nonzero(ev["keep"][f])[0]
        assert np.array_equal(i3[f, 1:1 + i3[f, 0]], idx) and np.array_equal(i2[f, 1:1 + i2[f, 0]], ev["pixel"][f][idx])
    if name == "main":
        for filt, (yes, no) in ev["stats"].items():
            assert yes > 0 and no > 0, filt


def test_evaluate_flags_a_point_on_a_threshold():
    """a vertex whose x lands on a pixel boundary is inside the margin, and only that one"""
    g = gold("main")
    table = R.frame_table(g["poses"][:1], PAR)
    keep, _ = R.decide(table[0], PAR, BC.IMAGE_DIMS, g["depth"][0], g["points"])
    P = g["poses"][0].astype(np.float64)
    cam = np.array([(10.5 - 20.0) / 37.01983 * 2.0, 0.1, 2.0])
    on_edge = (P[:3, :3] @ cam + P[:3, 3]).astype(np.float32)
    pts = np.concatenate([g["points"][keep][:3], on_edge[None]])
    near = BC.evaluate(pts, g["depth"][:1], g["poses"][:1], PAR)["near"]
    assert near.tolist() == [False, False, False, True]


def test_frame_table_of_unusable_poses():
    poses = np.stack([np.eye(4, dtype=np.float32), np.full((4, 4), -np.inf, np.float32),
                      np.zeros((4, 4), np.float32), np.diag([1, 1, 0, 1]).astype(np.float32)])
    table = R.frame_table(poses, PAR)
    assert table[:, 36].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert same(table[0, :12], np.eye(4, dtype=np.float32)[:3].reshape(-1))
    keep, _ = R.decide(table[1], PAR, BC.IMAGE_DIMS, np.ones((32, 41), np.float32), np.zeros((5, 3), np.float32))
    assert not keep.any()


def test_rounding_quirks_of_the_decision():
    """identity pose: the camera looks along +z.  A product of exactly -0.005 rounds to -0 and
    is outside; a pixel coordinate of .5 rounds to the even pixel"""
    table = R.frame_table(np.eye(4, dtype=np.float32)[None], PAR)[0]
    depth = np.full((32, 41), 2.0, np.float32)
    x_even = np.float32((10.5 - 20.0) / 37.01983 * 2.0)
    pts = np.array([[0.0, 0.0, 2.0], [x_even, 0.0, 2.0], [np.nan, 0.0, 2.0], [0.0, 0.0, 5.0]], np.float32)
    keep, pix = R.decide(table, PAR, BC.IMAGE_DIMS, depth, pts)
    assert keep.tolist() == [True, True, False, False]
    x = (np.float32(pts[1, 0]) * PAR[0]) / np.float32(2.0) + PAR[2]
    assert pix[1] % 41 == int(np.rint(x)) and pix[0] == 16 * 41 + 20   # 15.5 rounds to 16 (even)
    assert np.rint(np.float32(-0.5)) / np.float32(100) == 0 and not (np.rint(np.float32(-0.5)) / np.float32(100) < 0)


def test_backproj_exports_are_the_header(ov3d):
    from ov3d_amd import _native, projection
    src = open(os.path.join(ROOT, "include", "ov3d_backproj.h")).read()
    protos = re.findall(r"^int\s+(ov3d_\w+)\(", src, flags=re.M)
    assert set(_native.HEADER_EXPORTS["ov3d_backproj.h"]) == set(protos) == {
        "ov3d_backproj_frames", "ov3d_backproj_tables", "ov3d_backproj_gather", "ov3d_backproj_compose"}
    assert len(protos) == len(_native.HEADER_EXPORTS["ov3d_backproj.h"])
    defines = dict(re.findall(r"^#define\s+(OV3D_BACKPROJ_\w+)\s+(\d+)", src, flags=re.M))
    assert (int(defines["OV3D_BACKPROJ_ROW"]), int(defines["OV3D_BACKPROJ_PARAMS"]),
            int(defines["OV3D_BACKPROJ_BLOCK"])) == (projection.ROW, projection.NPARAMS, projection.BLOCK) \
        == (R.ROW, R.NPARAMS, R.BLOCK)
    lib = _native.load()
    for name in protos:
        assert hasattr(lib, name), name


def test_helper_constants_are_the_restatement(ov3d):
    from ov3d_amd import image_util, projection
    proc = image_util.image_processor()
    assert image_util.INTRINSICS == R.INTRINSICS == projection.INTRINSICS
    assert same(proc.PROJECTOR.host_params().numpy(), PAR)
    assert (proc.PROJECTOR.depth_min, proc.PROJECTOR.depth_max, proc.PROJECTOR.image_dims,
            proc.PROJECTOR.accuracy) == (0.1, 4.0, [41, 32], 0.05)
    other = projection.ProjectionHelper(R.INTRINSICS, 0.3, 6.0, [128, 80], 0.1)
    assert same(other.host_params().numpy(), R.params(R.INTRINSICS, 0.3, 6.0, (128, 80), 0.1))
    with pytest.raises(_native_error()):
        projection.ProjectionHelper(R.INTRINSICS, 0.1, 4.0, [41, 32], 0.05, cuda=False)


def _native_error():
    from ov3d_amd import _native
    return _native.NativeError
