"""Pseudo-box evaluation on the GPU (csrc/boxeval.hip behind include/ov3d_boxeval.h): both
kernels against the numpy restatement (tests/box_eval_ref.py), bit for bit on every output, at
the shapes where they can go wrong (scans of 0, 1, 63, 64, 65, 257 predictions and 0, 1, 255,
256, 257 GT boxes mixed within one call: an empty scan, one element, the wave, the workgroup
and the LDS chunk of 256 each missed and passed by one); the same calls between guard bands
(tests/guard.py); the product end to end against the reference's recorded dicts
(tests/golden/box_eval.npz) through step, step_arrays with device tensors and the file driver;
a threshold list against single-threshold runs; the two launches inside a hipGraph capture (a
synchronisation or a device -> host copy raises there); and the launch census."""
import numpy as np
import pytest
import torch

import box_eval_cases as BC
import box_eval_ref as R
import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_box_eval_cpu import GOLD, check_metrics, same

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_boxeval_match", "ov3d_boxeval_tally")

SCAN_P = (257, 0, 65, 1, 63, 64, 257, 65, 1)
SCAN_G = (257, 256, 0, 255, 1, 257, 256, 255, 0)
# S, T, C, ldp, ldg
SHAPES = [(1, 1, 1, 6, 6), (3, 3, 18, 7, 10), (9, 16, 37, 10, 7)]
THRESHOLDS = {1: [0.25], 3: [0.25, 0.5, 0.0], 16: [k / 16.0 for k in range(16)]}


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def kernel_case(S, T, C, ldp, ldg):
    """everything on a 1/8 grid, so that equal scores, equal IoUs and IoUs equal to a threshold
    occur; predictions are jittered copies of their scan's GT boxes where it has any; the
    columns past the sixth hold numbers nobody may read"""
    rng = np.random.Generator(np.random.PCG64(1000 * S + T))
    pred, gt, pcls, gcls = [], [], [], []
    for s in range(S):
        k, g = SCAN_P[s], SCAN_G[s]
        gc = rng.integers(-24, 25, (g, 3)) / 8.0
        gs = rng.integers(4, 13, (g, 3)) / 8.0
        gl = rng.integers(0, C, g)
        if g:
            src = rng.integers(0, g, k)
            pc = gc[src] + rng.integers(-2, 3, (k, 3)) / 8.0
            ps = gs[src] + rng.integers(-1, 2, (k, 3)) / 8.0
            pl = np.where(rng.random(k) < 0.7, gl[src], rng.integers(0, C, k))
        else:
            pc, ps, pl = rng.integers(-24, 25, (k, 3)) / 8.0, rng.integers(4, 13, (k, 3)) / 8.0, rng.integers(0, C, k)
        pred.append(np.concatenate([pc, ps, rng.uniform(-9, 9, (k, ldp - 6))], 1))
        gt.append(np.concatenate([gc, gs, rng.uniform(-9, 9, (g, ldg - 6))], 1))
        pcls.append(pl)
        gcls.append(gl)
    off = lambda rows: np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)   # noqa: E731
    pred, gt = np.concatenate(pred), np.concatenate(gt)
    return dict(pred=pred, pred_cls=np.concatenate(pcls).astype(np.int32),
                score=(pred[:, 3] * pred[:, 4]) * pred[:, 5], pred_off=off(pcls), gt=gt,
                gt_cls=np.concatenate(gcls).astype(np.int32), gt_off=off(gcls))


@pytest.fixture(scope="module")
def kernel_refs():
    """case and restated outputs per shape, computed once and left alone"""
    out = {}
    for S, T, C, ldp, ldg in SHAPES:
        case = kernel_case(S, T, C, ldp, ldg)
        m = R.match(**case, thr=THRESHOLDS[T])
        nd, npos, ntp = R.tally(case["pred_cls"], case["gt_cls"], m["best"], THRESHOLDS[T], C)
        out[S] = (case, dict(m, nd=nd, npos=npos, ntp=ntp))
    return out


def check_outputs(got, want, case, T, C):
    for name in ("rank", "jmax", "ovmax", "best", "owner", "tp", "nd", "npos", "ntp"):
        assert same(got[name], want[name]), name
    for t in range(T):                                     # the closed form: totals = sums of the flags
        assert np.array_equal(np.bincount(case["pred_cls"], weights=got["tp"][t], minlength=C), got["ntp"][t])


@pytest.mark.parametrize("S,T,C,ldp,ldg", SHAPES)
def test_kernels_equal_the_restatement(cuda, kernel_refs, S, T, C, ldp, ldg):
    from ov3d_amd import box_eval as BE
    case, want = kernel_refs[S]
    thr = THRESHOLDS[T]
    r = BE.launch(*(dev(case[k], cuda) for k in ("pred", "pred_cls", "score", "pred_off", "gt", "gt_cls",
                                                 "gt_off")), dev(np.array(thr), cuda), C)
    got = {k: v.cpu().numpy() for k, v in r.items()}
    check_outputs(got, want, case, T, C)
    # the case decides something: ties in the scores, shared GT boxes, exact thresholds, both flags
    assert len(np.unique(case["score"])) < len(case["score"])
    assert (np.bincount(want["jmax"][want["jmax"] >= 0]) > 1).any()
    assert any((want["ovmax"] == t).any() for t in thr) or T == 1
    assert want["tp"].any() and not want["tp"].all() and (want["jmax"] < 0).any() == (C > 1)
    assert (want["best"] == -np.inf).any() and (want["owner"] == R.FREE).any()


@pytest.mark.parametrize("S,T,C,ldp,ldg", SHAPES)
def test_guard_bands(cuda, kernel_refs, S, T, C, ldp, ldg):
    """both entries between guard bands, both fills: no write outside the outputs, no result
    that depends on bytes outside the inputs, every output element written"""
    case, want = kernel_refs[S]
    thr = THRESHOLDS[T]
    P, G = len(case["pred"]), len(case["gt"])
    specs = {"pred": In(torch.from_numpy(case["pred"][:, :6].copy()), ld=ldp),      # the gap columns hold sentinels
             "gt": In(torch.from_numpy(case["gt"][:, :6].copy()), ld=ldg),
             "pred_cls": In(torch.from_numpy(case["pred_cls"]), index=(0, C - 1)),
             "gt_cls": In(torch.from_numpy(case["gt_cls"]), index=(0, C - 1)),
             "score": In(torch.from_numpy(case["score"])),
             "pred_off": In(torch.from_numpy(case["pred_off"]), index=(0, 0)),
             "gt_off": In(torch.from_numpy(case["gt_off"]), index=(0, 0)),
             "thr": In(torch.tensor(thr, dtype=torch.float64)),
             "rank": Out((P,), torch.int32), "jmax": Out((P,), torch.int32),
             "ovmax": Out((P,), torch.float64, finite=False), "best": Out((G,), torch.float64, finite=False),
             "owner": Out((T, G), torch.int32), "tp": Out((T, P), torch.uint8),
             "nd": Out((C,), torch.int32), "npos": Out((C,), torch.int32), "ntp": Out((T, C), torch.int32)}

    def both(t):
        guard.call("ov3d_boxeval_match", t["pred"], ldp, t["pred_cls"], t["score"], t["pred_off"], P, t["gt"],
                   ldg, t["gt_cls"], t["gt_off"], G, S, t["thr"], T, t["rank"], t["jmax"], t["ovmax"],
                   t["best"], t["owner"], t["tp"], like=t["thr"])
        guard.call("ov3d_boxeval_tally", t["pred_cls"], P, t["gt_cls"], t["best"], G, t["thr"], T, C, t["nd"],
                   t["npos"], t["ntp"], like=t["thr"])
    out = guard.run_case(cuda, specs, both)
    check_outputs({k: v.cpu().numpy() for k, v in out.items()}, want, case, T, C)


@pytest.mark.parametrize("bad", [dict(S=0), dict(T=17), dict(ldp=5)])
def test_guard_rejected_match_writes_nothing(cuda, kernel_refs, bad):
    case, _ = kernel_refs[1]
    a = dict(S=1, T=1, ldp=6)
    a.update(bad)
    P, G = len(case["pred"]), len(case["gt"])
    specs = {k: In(torch.from_numpy(case[k])) for k in ("pred", "pred_cls", "score", "pred_off", "gt", "gt_cls",
                                                        "gt_off")}
    specs.update(thr=In(torch.tensor([0.25] * 17, dtype=torch.float64)), rank=Out((P,), torch.int32),
                 jmax=Out((P,), torch.int32), ovmax=Out((P,), torch.float64), best=Out((G,), torch.float64),
                 owner=Out((1, G), torch.int32), tp=Out((1, P), torch.uint8))
    assert guard.run_case(cuda, specs, lambda t: guard.raw_call(
        "ov3d_boxeval_match", t["pred"], a["ldp"], t["pred_cls"], t["score"], t["pred_off"], P, t["gt"], 6,
        t["gt_cls"], t["gt_off"], G, a["S"], t["thr"], a["T"], t["rank"], t["jmax"], t["ovmax"], t["best"],
        t["owner"], t["tp"], like=t["thr"]), expect_reject=True) == (-1, -1)


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("name", BC.CASES)
def test_product_equals_the_reference(cuda, name, tmp_path):
    from ov3d_amd import box_eval as BE
    scans, class2type, kind = BC.case(name)
    names, box_dir, gt_dir = BC.write_tree(scans, str(tmp_path))
    singles = {}
    for thr in BC.THRESHOLDS:
        calc = BE.PRCalculator(thr, class2type, device=cuda)
        for pred, gt in scans:
            p, g = BC.lists(pred, gt)
            calc.step([p], [g])
        singles[thr] = calc.compute_metrics()
        check_metrics(singles[thr], f"{name}/step/{thr}")
        metrics, avg, total = BE.compute_precision_recall(names, box_dir, gt_dir, thr, class2type, device=cuda)
        check_metrics(metrics, f"{name}/loop/{thr}")
        assert np.array_equal(np.array([avg, total], np.float64), GOLD[f"{name}/loop/{thr}/avg_total"],
                              equal_nan=True)
    # a threshold list equals the single-threshold runs; device tensors equal the lists
    both = BE.PRCalculator(list(BC.THRESHOLDS), class2type, device=cuda)
    for pred, gt in scans:
        both.step_arrays(dev(pred, cuda), dev(gt, cuda), dev(np.searchsorted(BC.NYU40, gt[:, 6]), cuda))
    got = both.compute_metrics()
    for thr in BC.THRESHOLDS:
        assert list(got[thr].items()) == list(singles[thr].items()) or name == "no_predictions"
        check_metrics(got[thr], f"{name}/step/{thr}")
    if kind == "curve":
        curves = both.compute_curves()
        for thr in BC.THRESHOLDS:
            rec, prec, ap = curves[thr]
            tag = f"{name}/step/{thr}"
            for c in np.nonzero(GOLD[tag + "/nd"])[0]:
                assert same(rec[c], GOLD[f"{tag}/rec/{c}"]) and same(prec[c], GOLD[f"{tag}/prec/{c}"])
                assert same(np.float64(ap[c]), GOLD[f"{tag}/ap/{c}"])


def test_device_tensors_are_refused_like_arrays(cuda):
    from ov3d_amd import box_eval as BE
    pred, gt = BC.quirks()[0]
    cls = np.searchsorted(BC.NYU40, gt[:, 6])
    calc = BE.PRCalculator(0.25, device=cuda)
    bad = pred.copy()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        calc.step_arrays(dev(bad, cuda), dev(gt, cuda), dev(cls, cuda))
    bad = pred.copy()
    bad[2, 6] = 2.5
    with pytest.raises(ValueError, match="integers"):
        calc.step_arrays(dev(bad, cuda), dev(gt, cuda), dev(cls, cuda))
    assert calc.scan_cnt == 0


def test_launches_are_capturable_and_counted(cuda, kernel_refs, monkeypatch):
    """the two launches inside a hipGraph capture replay to the same result; one
    compute_metrics is exactly the two entries and one device -> host copy"""
    from ov3d_amd import _native, box_eval as BE
    S, T, C = 3, 3, 18
    case, want = kernel_refs[S]
    t = [dev(case[k], cuda) for k in ("pred", "pred_cls", "score", "pred_off", "gt", "gt_cls", "gt_off")]
    t.append(dev(np.array(THRESHOLDS[T]), cuda))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        BE.launch(*t, C)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = BE.launch(*t, C)
    for v in r.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check_outputs({k: v.cpu().numpy() for k, v in r.items()}, want, case, T, C)

    calc = BE.PRCalculator([0.25, 0.5], device=cuda)
    for pred, gt in BC.quirks():
        calc.step_arrays(pred, gt, np.searchsorted(BC.NYU40, gt[:, 6]))
    copies = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.shape), cpu(self, *a, **k))[1])
    _native.census_start()
    got = calc.compute_metrics()
    census = _native.census_stop()
    monkeypatch.undo()
    assert census == {"ov3d_boxeval_match": 1, "ov3d_boxeval_tally": 1}
    assert len(copies) == 1
    check_metrics(got[0.5], "quirks/step/0.5")
