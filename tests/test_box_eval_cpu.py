"""Pseudo-box evaluation without a GPU: the numpy restatement of the two kernels
(tests/box_eval_ref.py) against what the reference's PRCalculator recorded
(tests/golden/box_eval.npz): every metric dict exactly, key order included, the per-class true
positive totals, and for the "curve" cases rec, prec and ap exactly; the product's host side
(ov3d_amd.box_eval) with the restatement standing in for the two launches, through step,
step_arrays and the file driver; the refusals; and the argument validation of every entry of
include/ov3d_boxeval.h, which happens before any launch."""
import ctypes
import os

import numpy as np
import pytest

import box_eval_cases as BC
import box_eval_ref as R
from helpers import ROOT, ov3d  # noqa: F401

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "box_eval.npz"))
MODES = ("step", "loop")
C = 32


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def used_scans(scans, mode):
    return [s for s in scans if not (mode == "loop" and len(s[0]) == 0)]


def pack_of(scans):
    """the scans in the CSR form of include/ov3d_boxeval.h, scores as np.prod gives them"""
    off = lambda i: np.concatenate([[0], np.cumsum([len(s[i]) for s in scans])]).astype(np.int32)   # noqa: E731
    return dict(pred=np.concatenate([p[:, :6].astype(np.float64) for p, _ in scans]).reshape(-1, 6),
                pred_cls=np.concatenate([p[:, 6] for p, _ in scans]).astype(np.int32),
                score=np.concatenate([np.prod(p[:, 3:6], 1).astype(np.float64) for p, _ in scans]),
                pred_off=off(0),
                gt=np.concatenate([g[:, :6].astype(np.float64) for _, g in scans]).reshape(-1, 6),
                gt_cls=np.concatenate([np.searchsorted(BC.NYU40, g[:, 6]) for _, g in scans]).astype(np.int32),
                gt_off=off(1))


def check_metrics(got, tag):
    """a metric dict against the recording: keys in order, values bit for bit (nan as nan),
    and Python ints where the reference reports ints"""
    assert list(got.keys()) == GOLD[tag + "/keys"].tolist(), tag
    vals = np.array([float(v) for v in got.values()], np.float64)
    assert np.array_equal(vals.view(np.int64), GOLD[tag + "/values"].view(np.int64)) or \
        np.array_equal(vals, GOLD[tag + "/values"], equal_nan=True), (tag, vals, GOLD[tag + "/values"])
    assert [isinstance(v, int) for v in got.values()] == GOLD[tag + "/is_int"].astype(bool).tolist(), tag
    assert all(isinstance(v, (int, np.float64)) for v in got.values()), tag


@pytest.fixture(scope="module")
def restated():
    """every case and mode through the restatement, once"""
    out = {}
    for name in BC.CASES:
        scans = BC.case(name)[0]
        for mode in MODES:
            used = used_scans(scans, mode)
            if used:
                pack = pack_of(used)
                out[name, mode] = (pack, R.match(**pack, thr=BC.THRESHOLDS))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", BC.CASES)
def test_restatement_equals_the_recorded_totals_and_curves(restated, name, mode):
    if (name, mode) not in restated:                       # every scan skipped: nothing to match
        assert name == "no_predictions" and mode == "loop"
        assert not GOLD[f"{name}/{mode}/0.25/tp"].any()
        return
    pack, m = restated[name, mode]
    nd, npos, ntp = R.tally(pack["pred_cls"], pack["gt_cls"], m["best"], BC.THRESHOLDS, C)
    for ti, thr in enumerate(BC.THRESHOLDS):
        tag = f"{name}/{mode}/{thr}"
        assert np.array_equal(nd, GOLD[tag + "/nd"]) and np.array_equal(npos, GOLD[tag + "/npos"])
        assert np.array_equal(ntp[ti], GOLD[tag + "/tp"]), tag
        assert np.array_equal(np.bincount(pack["pred_cls"], weights=m["tp"][ti], minlength=C), ntp[ti])
        if BC.case(name)[2] != "curve":
            assert not any(k.startswith(tag + "/rec/") for k in GOLD.files)
            continue
        curves = 0
        for c in np.nonzero(nd)[0]:
            sel = pack["pred_cls"] == c
            rec, prec, ap = R.curve(pack["score"][sel], m["tp"][ti][sel], npos[c])
            assert same(rec, GOLD[f"{tag}/rec/{c}"]) and same(prec, GOLD[f"{tag}/prec/{c}"]), (tag, c)
            assert same(np.float64(ap), GOLD[f"{tag}/ap/{c}"]), (tag, c)
            curves += 1
        assert curves >= 3


def test_the_recording_is_not_trivial():
    tp25, tp50 = GOLD["quirks/step/0.25/tp"], GOLD["quirks/step/0.5/tp"]
    assert tp25.sum() > tp50.sum() > 0                     # the thresholds decide differently
    assert GOLD["quirks/step/0.25/npos"].sum() > GOLD["quirks/loop/0.25/npos"].sum()   # the skipped scan's GT
    keys = GOLD["quirks/step/0.25/keys"].tolist()
    assert "2.0 Precision" in keys and "7 Precision" in keys and "10.0 Recall" in keys
    assert GOLD["quirks/step/0.25/is_int"].sum() == 2      # the GT-only class: Precision 0 and Recall 0
    assert "chair Precision" in GOLD["quirks_named/step/0.25/keys"].tolist()
    none = dict(zip(GOLD["no_predictions/step/0.25/keys"].tolist(), GOLD["no_predictions/step/0.25/values"]))
    assert np.isnan(none["mPrecision"]) and none["AR"] == 0.0 and none["2 Recall"] == 0.0
    assert GOLD["no_predictions/loop/0.25/keys"].tolist() == ["mPrecision", "AR"]


def host_calculator(monkeypatch, *args, **kw):
    """a PRCalculator whose two launches are the restatement"""
    from ov3d_amd import box_eval as BE
    monkeypatch.setattr(BE, "run_device", lambda pack, thr, C, device, flags=False: R.run(pack, thr, C, flags))
    return BE.PRCalculator(*args, **kw)


@pytest.mark.parametrize("name", BC.CASES)
def test_host_logic_reproduces_the_metric_dicts(monkeypatch, name):
    scans, class2type, kind = BC.case(name)
    for thr in BC.THRESHOLDS:
        calc = host_calculator(monkeypatch, thr, class2type)
        for pred, gt in scans:
            p, g = BC.lists(pred, gt)
            calc.step([p], [g])
        assert calc.scan_cnt == len(scans)
        check_metrics(calc.compute_metrics(), f"{name}/step/{thr}")
    both = host_calculator(monkeypatch, list(BC.THRESHOLDS), class2type)   # arrays, all thresholds at once
    for pred, gt in scans:
        both.step_arrays(pred, gt[:, :6], np.searchsorted(BC.NYU40, gt[:, 6]))
    got = both.compute_metrics()
    assert list(got.keys()) == list(BC.THRESHOLDS)
    for thr in BC.THRESHOLDS:
        check_metrics(got[thr], f"{name}/step/{thr}")
    if kind == "curve":
        curves = both.compute_curves()
        for thr in BC.THRESHOLDS:
            rec, prec, ap = curves[thr]
            tag = f"{name}/step/{thr}"
            for c in np.nonzero(GOLD[tag + "/nd"])[0]:
                assert same(rec[c], GOLD[f"{tag}/rec/{c}"]) and same(prec[c], GOLD[f"{tag}/prec/{c}"])
                assert same(np.float64(ap[c]), GOLD[f"{tag}/ap/{c}"])
            gt_only = np.nonzero((GOLD[tag + "/nd"] == 0) & (GOLD[tag + "/npos"] > 0))[0]
            assert all(rec[c] == 0 and isinstance(ap[c], int) for c in gt_only)
            assert len(ap) == len(np.nonzero(GOLD[tag + "/nd"] + GOLD[tag + "/npos"])[0])
    both.reset()
    assert both.scan_cnt == 0


@pytest.mark.parametrize("name", BC.CASES)
def test_file_driver_reproduces_the_script(monkeypatch, tmp_path, name, capsys):
    from ov3d_amd import box_eval as BE
    scans, class2type, _ = BC.case(name)
    monkeypatch.setattr(BE, "run_device", lambda pack, thr, C, device, flags=False: R.run(pack, thr, C, flags))
    names, box_dir, gt_dir = BC.write_tree(scans, str(tmp_path))
    for thr in BC.THRESHOLDS:
        tag = f"{name}/loop/{thr}"
        metrics, avg, total = BE.compute_precision_recall(names, box_dir, gt_dir, thr, class2type)
        check_metrics(metrics, tag)
        assert np.array_equal(np.array([avg, total], np.float64), GOLD[tag + "/avg_total"], equal_nan=True)
    if name == "quirks_named":                             # the default table is the tools' own
        assert BE.SCANNET_CLASS2TYPE == BC.CLASS2TYPE
        check_metrics(BE.compute_precision_recall(names, box_dir, gt_dir, 0.5)[0], tag)
        BE.print_metrics(metrics, avg, total, 0.5)
        lines = capsys.readouterr().out.splitlines()
        assert lines[0] == "-" * 10 + " prop: iou_thresh: 0.5 " + "-" * 10
        assert lines[1] == "avg num: %.2f total number: %d" % (avg, total)
        assert lines[2:] == ["eval %s: %f" % (k, v) for k, v in metrics.items()]
        # the training format: nyu40 ids in column 6 of the pseudo boxes
        for i, (pred, _) in enumerate(scans):
            t = np.array(pred)
            t[:, 6] = BC.NYU40[pred[:, 6].astype(int)]
            np.save(os.path.join(box_dir, BC.scan_name(i) + "_bbox.npy"), t)
        check_metrics(BE.compute_precision_recall(names, box_dir, gt_dir, 0.5, pred_ids="nyu40")[0], tag)


def test_refusals(monkeypatch, tmp_path):
    from ov3d_amd import box_eval as BE
    with pytest.raises(NotImplementedError, match="bb\\[7\\]"):
        BE.PRCalculator(0.25, obb=True)
    with pytest.raises(ValueError, match="thresholds"):
        BE.PRCalculator([0.1] * 17)
    with pytest.raises(ValueError, match="thresholds"):
        BE.PRCalculator([])
    calc = host_calculator(monkeypatch, 0.25)
    pred, gt = BC.quirks()[0]
    cls = np.searchsorted(BC.NYU40, gt[:, 6])
    bad = pred.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        calc.step_arrays(bad, gt, cls)
    bad = gt.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        calc.step_arrays(pred, bad, cls)
    bad = pred.copy()
    bad[2, 6] = 2.5
    with pytest.raises(ValueError, match="integers"):
        calc.step_arrays(bad, gt, cls)
    for c in (-1, 4096):
        with pytest.raises(ValueError, match="integers"):
            calc.step_arrays(pred, gt, np.full(len(gt), c))
    with pytest.raises(ValueError, match="integers"):
        calc.step([[(2.5, pred[0, :6], 1.0)]], [[]])
    with pytest.raises(ValueError, match="finite"):
        calc.step([[(2, pred[0, :6], np.nan)]], [[]])
    assert calc.scan_cnt == 0                              # nothing refused was kept
    names, box_dir, gt_dir = BC.write_tree([(pred, gt)], str(tmp_path))
    gt[1, 6] = 13                                          # no detection class
    np.save(os.path.join(gt_dir, names[0] + "_bbox.npy"), gt)
    with pytest.raises(ValueError, match=names[0]):
        BE.compute_precision_recall(names, box_dir, gt_dir)
    with pytest.raises(ValueError, match=names[0]):
        BE.compute_precision_recall(names, box_dir, gt_dir, pred_ids="nyu40")   # class indices 2, 4, 10 as ids


def test_exports_are_the_header():
    from ov3d_amd import _native
    with open(os.path.join(ROOT, "include", "ov3d_boxeval.h")) as f:
        protos = _native.read_header(f.read())[1]
    assert set(_native.HEADER_EXPORTS["ov3d_boxeval.h"]) == set(protos) == {
        "ov3d_boxeval_match", "ov3d_boxeval_tally"}
    lib = _native.load()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_entries_reject_invalid_arguments():
    """every entry of include/ov3d_boxeval.h validates before any launch (no device needed)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok = dict(pred=p, ldp=6, pred_cls=p, score=p, pred_off=p, P=5, gt=p, ldg=7, gt_cls=p, gt_off=p, G=4, S=2,
              thr=p, T=2, rank=p, jmax=p, ovmax=p, best=p, owner=p, tp=p)

    def match(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_boxeval_match(a["pred"], a["ldp"], a["pred_cls"], a["score"], a["pred_off"], a["P"],
                                      a["gt"], a["ldg"], a["gt_cls"], a["gt_off"], a["G"], a["S"], a["thr"],
                                      a["T"], a["rank"], a["jmax"], a["ovmax"], a["best"], a["owner"], a["tp"],
                                      None)
    for name in ("pred", "pred_cls", "score", "pred_off", "gt", "gt_cls", "gt_off", "thr", "rank", "jmax",
                 "ovmax", "best", "owner", "tp"):
        assert match(**{name: None}) == -1, name
    assert match(S=0) == -1 and match(T=0) == -1 and match(T=17) == -1
    assert match(ldp=5) == -1 and match(ldg=5) == -1 and match(P=-1) == -1 and match(G=-1) == -1
    assert match(P=1 << 31) == -1 and match(G=1 << 31) == -1
    # P == 0 / G == 0 excuse their own pointers only
    assert match(P=0, pred=None, thr=None) == -1 and match(G=0, gt=None, pred_off=None) == -1

    ok = dict(pred_cls=p, P=5, gt_cls=p, best=p, G=4, thr=p, T=2, C=18, nd=p, npos=p, ntp=p)

    def tally(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_boxeval_tally(a["pred_cls"], a["P"], a["gt_cls"], a["best"], a["G"], a["thr"], a["T"],
                                      a["C"], a["nd"], a["npos"], a["ntp"], None)
    for name in ("pred_cls", "gt_cls", "best", "thr", "nd", "npos", "ntp"):
        assert tally(**{name: None}) == -1, name
    assert tally(C=0) == -1 and tally(T=0) == -1 and tally(T=17) == -1 and tally(P=-1) == -1
    assert tally(G=-1) == -1 and tally(P=1 << 31) == -1
    assert tally(P=0, pred_cls=None, nd=None) == -1 and tally(G=0, gt_cls=None, best=None, thr=None) == -1
