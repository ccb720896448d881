"""Pseudo-label generation on the host: the numpy restatement (tests/pseudo_label_ref.py) and
the product's LabelFormatter (device="cpu", the vote replaced by the restatement's) reproduce
every array the reference recorded in tests/golden/pseudo_label.npz exactly (values, dtype,
shape, order); label validation; and the entry's rejections, which need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pseudo_label_cases as PC
import pseudo_label_ref as R
from helpers import fixture, ov3d  # noqa: F401

GOLD = fixture("pseudo_label.npz")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def product_formatter(name, tmp_path, device, monkeypatch=None):
    from ov3d_amd import label_formatter as LF
    if monkeypatch is not None:
        monkeypatch.setattr(LF, "box_label_votes", R.vote_torch)
    scans, steps = PC.make(name)
    names = [PC.scan_name(i) for i in range(len(scans))]
    lf = LF.LabelFormatter("", str(tmp_path), None, names, device=device, scans=scans)
    for outputs, scan_idx in steps:
        lf.step({k: torch.from_numpy(v).to(device) for k, v in outputs.items()},
                {"scan_idx": torch.from_numpy(scan_idx).to(device)})
    return lf, names


def check_files(name, tmp_path, names):
    for i, n in enumerate(names):
        got = np.load(os.path.join(str(tmp_path), n + "_bbox.npy"))
        assert same(got, GOLD[f"{name}/bbox/{i}"]), (name, i)
        assert got.dtype == np.float64 and got.shape[1] == 7


@pytest.mark.parametrize("name", PC.CASES)
def test_golden_cases_are_not_trivial(name):
    past = GOLD[f"{name}/pseudo_boxes"].shape[0]
    kept = sum(GOLD[f"{name}/bbox/{i}"].shape[0] for i in range(len(PC.CASES[name]["scans"])))
    assert 4 * kept >= past and 4 * (past - kept) >= past
    if name == "mixed":
        sizes = [GOLD[f"mixed/bbox/{i}"].shape[0] for i in range(6)]
        assert sizes[3] == 0 and sizes[5] == 0          # all boxes fail the vote; no box at all
        assert all(sizes[i] > 0 for i in (0, 1, 2, 4))
        # the hand-made queries (pseudo_label_cases._specials), by their centre's x
        for i, copies in ((0, 2), (4, 1)):               # scan 0 was stepped twice: both copies
            x = GOLD[f"mixed/bbox/{i}"][:, 0].tolist()
            assert x.count(10.0) == 0                    # tie with a smaller label: dropped
            assert x.count(12.0) == copies               # tie with a larger label: kept
            assert x.count(14.0) == copies               # zero-size box on a grid plane
            assert x.count(18.0) == copies               # two equal maxima: the first, class 5
        box = GOLD["mixed/bbox/4"]
        assert box[box[:, 0] == 18.0][0, 6] == 5
        assert (box[:, 0] == 16.0).sum() == 1            # the vertex at lo - 2^-40 is outside
        assert (GOLD["mixed/pseudo_boxes"][:, 7] == np.float32(0.9)).any()


@pytest.mark.parametrize("name", PC.CASES)
def test_restatement_reproduces_the_reference(name):
    cs = PC.CASES[name]
    scans, steps = PC.make(name)
    pb = R.compute([R.step_rows(o, s) for o, s in steps], cs["th_s"], cs["th_o"])
    assert same(pb, GOLD[f"{name}/pseudo_boxes"]) and pb.dtype == np.float32
    for i, raw in enumerate(scans):
        assert same(R.gen_pseudo(pb, i, raw), GOLD[f"{name}/bbox/{i}"]), (name, i)
    # the vote form of the same rule: mode == class <=> kept
    for i, raw in enumerate(scans):
        cand = pb[pb[:, -1] == i]
        if not cand.shape[0]:
            continue
        lo, hi = R.bounds(cand)
        lab = np.where((raw[:, 3] >= 0) & (raw[:, 3] < 18), raw[:, 3], 255).astype(np.uint8)
        _, mode = R.vote(raw[None, :, :3], lab[None], lo[None], hi[None], 18)
        assert same(cand[mode[0] == cand[:, 6]][:, :7].astype(np.float64), GOLD[f"{name}/bbox/{i}"])


@pytest.mark.parametrize("name", PC.CASES)
def test_product_formatter_host_logic(name, tmp_path, monkeypatch):
    cs = PC.CASES[name]
    lf, names = product_formatter(name, tmp_path, "cpu", monkeypatch)
    lf.compute(0, cs["th_s"], cs["th_o"])
    assert same(lf.pseudo_boxes, GOLD[f"{name}/pseudo_boxes"])
    total = lf.save()
    check_files(name, tmp_path, names)
    assert total == sum(GOLD[f"{name}/bbox/{i}"].shape[0] for i in range(len(names)))
    # gen_pseudo: one scan, the same file and its count
    for i in range(len(names)):
        assert lf.gen_pseudo(i) == GOLD[f"{name}/bbox/{i}"].shape[0]
    check_files(name, tmp_path, names)


def test_float32_thresholds_and_first_maximum(tmp_path, monkeypatch):
    """np.float32(0.9) >= 0.9 holds in float32 and not in double; equal maxima give the first"""
    from ov3d_amd import label_formatter as LF
    assert not float(np.float32(0.9)) >= 0.9
    prob = np.zeros((1, 2, 18), np.float32)
    prob[0, 0, [4, 9]] = np.float32(0.9)
    prob[0, 1, 3] = np.nextafter(np.float32(0.9), np.float32(0))
    out = {"sem_cls_prob": prob, "objectness_prob": np.full((1, 2), 0.5, np.float32),
           "center_unnormalized": np.zeros((1, 2, 3), np.float32),
           "size_unnormalized": np.ones((1, 2, 3), np.float32)}
    lf = LF.LabelFormatter("", str(tmp_path), None, ["s"], device="cpu",
                           scans=[np.zeros((1, 4), np.float32)])
    lf.step({k: torch.from_numpy(v) for k, v in out.items()}, {"scan_idx": torch.zeros(1, dtype=torch.int64)})
    lf.compute(0, 0.9, 0.5)
    assert lf.pseudo_boxes.shape == (1, 10) and lf.pseudo_boxes[0, 6] == 4


def test_label_validation(tmp_path):
    from ov3d_amd import label_formatter as LF
    for bad in (-1.0, 2.5, float("nan")):
        raw = np.zeros((5, 4), np.float64)
        raw[3, 3] = bad
        with pytest.raises(ValueError, match="scene0042_00"):
            LF.LabelFormatter("", str(tmp_path), None, ["scene0042_00"], device="cpu", scans=[raw])
        # read from a file: raised when the scan is read
        np.save(os.path.join(str(tmp_path), "scene0042_00.npy"), raw)
        lf = LF.LabelFormatter("", str(tmp_path), str(tmp_path), ["scene0042_00"], device="cpu")
        lf.pseudo_boxes = np.zeros((0, 10), np.float32)
        with pytest.raises(ValueError, match="scene0042_00"):
            lf.gen_pseudo(0)
    raw = np.zeros((6, 4), np.float32)
    raw[:, 3] = [0, 17, 18, 40, -100, 5]
    assert LF.scan_labels(raw[:, 3], 18, "s").tolist() == [0, 17, 255, 255, 255, 5]


def test_wrapper_needs_the_device():
    from ov3d_amd import _native
    from ov3d_amd.label_formatter import box_label_votes
    with pytest.raises(_native.NativeError):
        box_label_votes(torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.uint8),
                        torch.zeros(1, 2, 3), torch.ones(1, 2, 3), 18)


def test_entry_rejects_invalid_combinations():
    """ov3d_box_points_count validates before any launch (host-side checks, no device)"""
    from ov3d_amd import _native
    f = _native.load().ov3d_box_points_count
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok0 = dict(pts=p, f64=0, sb=12, sn=3, N=4, boxes=p, kind=0, labels=None, C=0, B=1, K=2, counts=p, mode=None)
    ok1 = dict(ok0, kind=1, labels=p, C=18, mode=p)

    def rc(base, **kw):
        a = dict(base, **kw)
        return f(a["pts"], a["f64"], a["sb"], a["sn"], a["N"], a["boxes"], a["kind"], a["labels"],
                 a["C"], a["B"], a["K"], a["counts"], a["mode"], None)
    for kind in (-1, 2, 7):
        assert rc(ok1, kind=kind) == -1 and rc(ok0, kind=kind) == -1
    # kind 0 takes none of the vote's arguments
    assert rc(ok0, labels=p) == -1 and rc(ok0, C=18) == -1 and rc(ok0, f64=1) == -1
    assert rc(ok0, mode=p) == -1
    for base in (ok0, ok1):
        assert rc(base, pts=None) == -1 and rc(base, boxes=None) == -1 and rc(base, counts=None) == -1
        assert rc(base, sn=2) == -1
        assert rc(base, B=-1) == -1 and rc(base, K=-1) == -1 and rc(base, N=-1) == -1
    assert rc(ok1, labels=None) == -1
    for C in (0, -1, 33):
        assert rc(ok1, C=C) == -1
    assert rc(ok1, f64=2) == -1
    assert rc(ok1, B=0) == -1 and rc(ok1, K=0) == -1 and rc(ok1, N=0) == -1
