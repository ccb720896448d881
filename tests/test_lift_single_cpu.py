"""Single-view pseudo-box lifting without a GPU: the numpy restatement (tests/lift_single_ref.py)
against what the reference's scannet/lift_boxes.py recorded with VIEW = 'single'
(tests/golden/lift_single.npz): the saved arrays bit for bit (their geometry is the pool's),
the lifted boxes within the bound derived below; the product's host side (slots, edge filter,
the intrinsic left alone, refusals); the export set of include/ov3d_liftview.h; the argument
validation of its entry, which happens before any launch; and that PIL loads lazily.

The bound on a lifted coordinate.  The reference forms a lifted point through three chained
maps, each a dot product of at most 4 terms through BLAS (summation order and fusing
unspecified): the ray r = Kinv [u, v, 1] times d, the pose w = R c + t, the alignment
a = A [w, 1].  The restatement and the device sum in a fixed order.  With eps = 2^-53, to first
order a map whose results are bounded by s = max_i(sum_j |M_ij| max|p_j| + |t_i|) adds at most
4 eps s to an exact evaluation and passes the error e of its input on as at most |M|_inf e
(largest absolute row sum).  Hence, from each case's own matrices, depths and pixel range,
    s1 = max_i(|Kinv| [W-1, H-1, 1])_i max d,          e1 = 4 eps s1
    s2 = max_i(|R| [s1, s1, s1] + |t|)_i over frames,  e2 = |R|_inf e1 + 4 eps s2
    s3 = max_i(|A3| [s2, s2, s2] + |A_i3|)_i,          e3 = |A3|_inf e2 + 4 eps s3
and two evaluations differ by at most 2 e3; the bar is 4 times that."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import lift_ref as R
import lift_single_cases as SC
import lift_single_ref as SR
from helpers import ROOT, ov3d  # noqa: F401
from test_lift_ref_cpu import check_lifted, same

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lift_single.npz"))


def single_bar(case):
    eps = 2.0 ** -53
    K = np.array(case["intrinsic"], dtype=np.float32)
    K[:2] /= 2.0
    kinv = np.abs(np.linalg.inv(K[:3, :3]).astype(np.float64))
    _, H, W = case["depths"].shape
    s1 = float((kinv @ np.array([W - 1.0, H - 1.0, 1.0])).max() * SR.metres(case["depths"]).max())
    e1 = 4 * eps * s1
    P = np.abs(np.asarray(case["poses"], np.float64))
    s2 = float((P[:, :3, :3].sum(2) * s1 + P[:, :3, 3]).max())
    e2 = float(P[:, :3, :3].sum(2).max()) * e1 + 4 * eps * s2
    A = np.abs(np.asarray(case["axis_align_matrix"], np.float64))
    s3 = float((A[:3, :3].sum(1) * s2 + A[:3, 3]).max())
    e3 = float(A[:3, :3].sum(1).max()) * e2 + 4 * eps * s3
    return 4 * 2 * e3


@pytest.fixture(scope="module")
def results():
    """every case through the restatement, once"""
    return {n: SR.scan(**SC.case(n)) for n in SC.CASES}


@pytest.mark.parametrize("name", SC.CASES)
def test_restatement_equals_the_recording(results, name):
    final, lifted = results[name]
    assert same(final, GOLD[f"single/{name}/final"]), name
    bar = single_bar(SC.case(name))
    assert 1e-15 < bar < 1e-12                             # metre-scale points: a few dozen ulps
    check_lifted(lifted, GOLD[f"single/{name}/lifted"], bar)


def test_the_recording_is_not_trivial():
    main, lifted = GOLD["single/main/final"], GOLD["single/main/lifted"]
    assert main.shape == (2, 10) and lifted.shape == (8, 8)
    assert (lifted[:, 7] == -100.0).sum() == 1
    assert same(lifted[0, :6], lifted[1, :6]) and lifted[0, 6] != lifted[1, 6]   # one (frame, label)
    assert same(GOLD["single/gt_labels/final"], main)       # the same scene as nyu40 ids
    assert GOLD["single/nothing_lifted/final"].shape == (0, 7)
    assert GOLD["single/nothing_matched/final"].shape == (0, 10)
    assert GOLD["single/nothing_matched/lifted"].shape == (8, 8)


def test_classes_of_the_restatement():
    seg = np.array([[-100, -3, 0, 17, 18, 40, 2 ** 31 - 1]])
    assert SR.classes(seg, ignore_from=18).tolist() == [[-100, -3, 0, 17, -100, -100, -100]]
    assert SR.classes(seg, ignore_from=None).tolist() == seg.tolist()
    lut = SR.nyu40_lut()
    assert SR.classes(np.array([0, 3, 4, 13, 39, 40, 41, -1]), lut=lut).tolist() == [-100, 0, 1, -100, 17,
                                                                                   -100, -100, -100]


def test_host_plan_slots_and_edge_filter():
    from ov3d_amd import lift_boxes as LB
    case = SC.case("main")
    K = case["intrinsic"].copy()
    plan = LB.single_host_plan(K, case["poses"], case["boxes2d"])
    assert same(K, case["intrinsic"]) and K[0, 0] == np.float32(SC.LC.FX)     # not halved in place
    kinv, pose, sl, frame, label = SR.plan(case["intrinsic"], case["poses"], case["boxes2d"], (240, 320))
    assert same(plan["kinv"], kinv) and same(plan["pose"], pose) and same(plan["score_label"], sl)
    assert plan["plabel"].dtype == np.int32 and np.array_equal(plan["plabel"], label)
    M = sum(len(b) for b in case["boxes2d"]) - 2             # two boxes touch the border
    assert len(sl) == M == 9
    # slots: distinct (frame, label) pairs; the two class-2 boxes of frame 0 share one
    sf, slab, bs = plan["slot_frame"], plan["slot_label"], plan["box_slot"]
    assert sf.dtype == slab.dtype == bs.dtype == np.int32 and len(sf) == len(slab) == M - 1
    assert len({(int(f), int(c)) for f, c in zip(sf, slab)}) == len(sf)
    assert np.array_equal(sf[bs], frame) and np.array_equal(slab[bs], label)
    assert bs[0] == bs[1] and 1 not in sf.tolist()           # frame 1 has no boxes
    assert (slab == -100).sum() == 1
    # the edge filter goes by the frames' own size
    boxes = [np.array([[1.0, 1.0, 6.0, 4.0, 0.5, 1.0], [1.0, 1.0, 5.0, 4.0, 0.4, 1.0]])]
    small = LB.single_host_plan(K, case["poses"][:1], boxes, (9, 7))
    assert small["score_label"].tolist() == [[0.4, 1.0]]
    none = LB.single_host_plan(K, case["poses"][:1], [np.zeros((0, 6))], (9, 7))
    assert len(none["box_slot"]) == 0 and len(none["slot_frame"]) == 0


def test_nyu40_table():
    from ov3d_amd import lift_boxes as LB
    lut = LB.nyu40_lut()
    assert lut.dtype == np.int32 and np.array_equal(lut, SR.nyu40_lut())


def test_refusals_come_before_any_launch():
    """every refusal is a ValueError on the host; device="meta" would fail at the first upload"""
    from ov3d_amd import lift_boxes as LB
    case = SC.case("main")
    del case["pseudo"]

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            LB.lift_scannet_scan_single(**dict(case, **kw), device="meta")
    poses = case["poses"].copy()
    poses[1, 0, 3] = np.inf                                  # a frame without boxes: refused all the same
    refused("finite", poses=poses)
    K = case["intrinsic"].copy()
    K[0, 0] = np.nan
    refused("finite", intrinsic=K)
    A = case["axis_align_matrix"].copy()
    A[2, 3] = -np.inf
    refused("finite", axis_align_matrix=A)
    d = case["depths"].astype(np.float32)
    d[3, 7, 9] = np.nan
    refused("finite", depths=d)
    refused("F,H,W", depths=case["depths"][:, :-1])
    refused("F,H,W", labels=case["labels"][:3])
    refused("F,H,W", depths=case["depths"].astype(np.float64))
    refused("poses", poses=case["poses"][:3])
    refused("gss_pool", gss_pool=np.zeros((0, 7)))
    bad = [b.copy() for b in case["boxes2d"]]
    bad[0][0, 4] = np.nan
    refused("finite", boxes2d=bad)
    many = [np.tile([[5.5, 5.5, 10.0, 10.0, 0.5, 3.0]], (LB.MAX_PER_CLASS + 1, 1))] + case["boxes2d"][1:]
    refused("one class", boxes2d=many)
    with pytest.raises(ValueError, match="view"):
        LB.ScannetBoxLifter(*"abcdef", view="both")


def test_nothing_to_lift_needs_no_device():
    from ov3d_amd import lift_boxes as LB
    case = SC.case("main")
    del case["pseudo"]
    case["boxes2d"] = [b[:0] for b in case["boxes2d"]]
    final, lifted = LB.lift_scannet_scan_single(**case, device="meta", return_lifted=True)
    assert final.shape == (0, 7) and lifted.shape == (0, 8)


def test_exports_of_the_header():
    from ov3d_amd import _native
    with open(os.path.join(ROOT, "include", "ov3d_liftview.h")) as f:
        protos = _native.read_header(f.read())[1]
    assert set(_native.HEADER_EXPORTS["ov3d_liftview.h"]) == set(protos) == {"ov3d_liftview_frames"}
    assert hasattr(_native.load(), "ov3d_liftview_frames")


def test_entry_rejects_invalid_arguments():
    """the entry validates before any launch (no device needed)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok = dict(depth=p, u16=0, seg=p, lut=None, lut_n=0, ignore=18, F=2, H=4, W=5, kinv=p, pose=p, align=p,
              sf=p, sl=p, S=3, bs=p, M=4, slohi=p, scount=p, lohi=p, ld=8, count=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_liftview_frames(a["depth"], a["u16"], a["seg"], a["lut"], a["lut_n"], a["ignore"],
                                        a["F"], a["H"], a["W"], a["kinv"], a["pose"], a["align"], a["sf"],
                                        a["sl"], a["S"], a["bs"], a["M"], a["slohi"], a["scount"], a["lohi"],
                                        a["ld"], a["count"], None)
    for name in ("depth", "seg", "kinv", "pose", "align", "sf", "sl", "bs", "slohi", "scount", "lohi", "count"):
        assert call(**{name: None}) == -1, name
    for name in ("F", "H", "W", "S", "M"):
        assert call(**{name: 0}) == -1 and call(**{name: -3}) == -1, name
    assert call(u16=2) == -1 and call(u16=-1) == -1          # a depth kind other than the two
    assert call(ld=5) == -1
    assert call(lut_n=40) == -1                              # lut_n without a table
    assert call(lut=p, lut_n=0) == -1
    assert call(H=1 << 16, W=1 << 15) == -1                  # H * W = 2^31
    assert call(H=1 << 16, W=1 << 16) == -1


def test_pil_loads_lazily():
    """importing the module and building the single-view driver pull in no image decoder"""
    code = ("import sys; sys.path.insert(0, %r); import ov3d_import; ov3d_import.load(); "
            "import ov3d_amd.lift_boxes as LB; LB.ScannetBoxLifter(*'abcdef', view='single'); "
            "assert 'PIL' not in sys.modules and 'imageio' not in sys.modules" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True)
