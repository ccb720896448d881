"""Pseudo-label generation on the GPU: ov3d_box_points_count kind 1 (csrc/evaldet.hip
box_label_vote_kernel) through box_label_votes against the numpy restatement
(tests/pseudo_label_ref.py), exactly; the product's LabelFormatter end to end against the
reference's recorded files (tests/golden/pseudo_label.npz); `step` inside a hipGraph capture
(a synchronisation or a device -> host copy raises there); `generate` on the reduced model;
and the kind-1 guard-band cases (tests/guard.py) at the ragged shapes."""
import os

import numpy as np
import pytest
import torch

import guard
import pseudo_label_cases as PC
import pseudo_label_ref as R
from guard import In, Out
from helpers import build_model_from_fixture, fixture, ov3d  # noqa: F401
from test_pseudo_label_cpu import GOLD, check_files, product_formatter, same

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_box_points_count",)

NS = (1, 63, 64, 65, 257, 1000)
KS = (1, 7, 8, 9, 33)
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def vote_case(N, K, C, dtype, B=3):
    """points on a 1/8 grid in [0, 2]^3 and bounds on the same grid (faces through vertices);
    scene 1 all ignored, scene 2's second half padding (label 255); empty boxes, NaN
    coordinates, and with float64 a vertex at lo - 2^-40 of box 0"""
    rng = np.random.Generator(np.random.PCG64(1000 * N + 10 * K + C + (dtype == np.float64)))
    pts = (rng.integers(0, 17, (B, N, 3)) / 8.0).astype(dtype)
    lab = rng.integers(0, C + 2, (B, N)).astype(np.uint8)       # C, C + 1: ignored values
    lab[1] = 200
    lab[2, N // 2 + 1:] = 255
    a = rng.integers(0, 17, (B, K, 3)) / 8.0
    w = rng.integers(0, 9, (B, K, 3)) / 8.0                       # 0: a zero-size box
    lo, hi = a.astype(np.float32), (a + w).astype(np.float32)
    lo[0, 0], hi[0, 0] = 0.25, 1.0
    if K > 2:
        lo[:, 2], hi[:, 2] = hi[:, 2] + 1, lo[:, 2].copy()        # lo > hi: empty
    nan = rng.random((B, N)) < 0.05
    pts[nan, rng.integers(0, 3, int(nan.sum()))] = np.nan
    if dtype == np.float64:
        pts[0, 0] = lo[0, 0].astype(np.float64) + [-2.0 ** -40, 0, 0]
        lab[0, 0] = 0
    return pts, lab, lo, hi


@pytest.fixture(scope="module")
def vote_refs():
    """every case's inputs and restatement answer, computed once"""
    out = {}
    for dt in (np.float32, np.float64):
        for N in NS:
            for K in KS:
                C = (1, 18, 32)[(NS.index(N) + KS.index(K)) % 3]
                case = vote_case(N, K, C, dt)
                out[dt, N, K] = (C, case, R.vote(*case, C))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", NS)
def test_box_label_votes_match_the_restatement(cuda, vote_refs, N, dtype):
    from ov3d_amd.label_formatter import box_label_votes
    seen = set()
    for K in KS:
        C, case, (counts, mode) = vote_refs[dtype, N, K]
        seen.add(C)
        c, m = box_label_votes(*(torch.from_numpy(x).to(cuda) for x in case), C)
        assert c.dtype == torch.int32 and m.dtype == torch.int32
        assert np.array_equal(c.cpu().numpy(), counts), (N, K, C)
        assert np.array_equal(m.cpu().numpy(), mode), (N, K, C)
        if dtype is np.float64:       # the vertex at lo - 2^-40 is outside box 0 in double
            pts, lab, lo, hi = case
            inside32 = np.all(pts[0, 0].astype(np.float32) >= lo[0, 0]) and np.all(pts[0, 0].astype(np.float32) <= hi[0, 0])
            assert inside32 and not np.all(pts[0, 0] >= lo[0, 0])
    assert seen == {1, 18, 32}


def test_votes_with_a_point_stride_and_every_class_count(cuda, vote_refs):
    """points as the xyz columns of wider rows (stride 6), and C = 1, 18, 32 at one shape"""
    from ov3d_amd.label_formatter import box_label_votes
    for C in (1, 18, 32):
        pts, lab, lo, hi = vote_case(257, 9, C, np.float32)
        wide = torch.full((3, 257, 6), float("nan"))
        wide[..., :3] = torch.from_numpy(pts)
        c, m = box_label_votes(wide.to(cuda)[..., :3], *(torch.from_numpy(x).to(cuda) for x in (lab, lo, hi)), C)
        counts, mode = R.vote(pts, lab, lo, hi, C)
        assert np.array_equal(c.cpu().numpy(), counts) and np.array_equal(m.cpu().numpy(), mode)


@pytest.mark.parametrize("name", PC.CASES)
def test_formatter_end_to_end_matches_the_reference_files(cuda, name, tmp_path):
    cs = PC.CASES[name]
    lf, names = product_formatter(name, tmp_path, cuda)
    assert all(b.is_cuda for b in lf.boxes)
    lf.compute(0, cs["th_s"], cs["th_o"])
    assert same(lf.pseudo_boxes, GOLD[f"{name}/pseudo_boxes"])
    total = lf.save()
    check_files(name, tmp_path, names)
    assert total == sum(GOLD[f"{name}/bbox/{i}"].shape[0] for i in range(len(names)))
    for i in range(len(names)):
        assert lf.gen_pseudo(i) == GOLD[f"{name}/bbox/{i}"].shape[0]
    check_files(name, tmp_path, names)


def test_step_is_capturable(cuda, tmp_path):
    """`step` inside a hipGraph capture: a host synchronisation or a device -> host copy raises
    during capture.  (Capture is the check used here, not torch's sync debug mode.)"""
    from ov3d_amd import label_formatter as LF
    scans, steps = PC.make("small")
    outputs, scan_idx = steps[0]
    dev_out = {k: torch.from_numpy(v).to(cuda) for k, v in outputs.items()}
    batch = {"scan_idx": torch.from_numpy(scan_idx).to(cuda)}
    lf = LF.LabelFormatter("", str(tmp_path), None, ["a", "b"], device=cuda, scans=scans)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lf.step(dev_out, batch)                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    lf.boxes.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lf.step(dev_out, batch)
    graph.replay()
    torch.cuda.synchronize()
    assert same(lf.boxes[0].cpu().numpy(), R.step_rows(outputs, scan_idx))


def test_generate_on_the_reduced_model(cuda, tmp_path):
    """generate -> process on synthetic scans: the files equal what the restatement makes from
    the same model outputs read back"""
    import scannet_aug_cases as SC
    from ov3d_amd import label_formatter as LF, scannet
    fx = fixture("model_scannet.npz")
    model, cfg, args = build_model_from_fixture(fx, cuda, "scannet")
    raw = SC.raw_scans()[:5]
    ds = scannet.ScannetDetectionDataset(cfg, split_set="val", num_points=2048, augment=False,
                                         use_color=args.use_color, device=cuda, scans=raw)
    rng = np.random.Generator(np.random.PCG64(9))
    # per-vertex labels: the class changes every 1.5 along x, a tenth ignored
    scans = []
    for i, (v, _) in enumerate(raw):
        lab = np.floor((v[:, 0] + 4.0) / 1.5 + i).astype(np.float64) % 18
        lab[rng.random(len(lab)) < 0.1] = -100
        scans.append(np.concatenate([v[:, :3].astype(np.float64 if i % 2 else np.float32),
                                     lab[:, None]], 1).astype(np.float64 if i % 2 else np.float32))
    lf = LF.LabelFormatter("", str(tmp_path), None, ds.scan_names, device=cuda, scans=scans, group=2)
    out = LF.generate(model, ds, lf, 2, np.random.RandomState(3))
    assert out is lf and len(lf.boxes) == 3 and all(b.is_cuda for b in lf.boxes)
    rows = [b.cpu().numpy() for b in lf.boxes]
    th_s = float(np.median(np.concatenate(rows)[:, 7]))
    lf.process(0, th_s, 0.0)
    pb = R.compute(rows, th_s, 0.0)
    assert same(lf.pseudo_boxes, pb) and pb.shape[0] >= 40
    kept = 0
    for i, n in enumerate(ds.scan_names):
        want = R.gen_pseudo(pb, i, scans[i])
        assert same(np.load(os.path.join(str(tmp_path), n + "_bbox.npy")), want), i
        kept += want.shape[0]
    print("generate: %d past the thresholds, %d kept" % (pb.shape[0], kept))
    with pytest.raises(ValueError, match="augment"):
        ds.augment = True
        LF.generate(model, ds, lf, 2)


# ---------------------------------------------------------------- guard bands, kind 1

def _guard_case(cuda, N, K, C, dtype, ld):
    pts, lab, lo, hi = vote_case(N, K, C, dtype)
    B = pts.shape[0]
    boxes = np.concatenate([lo, hi], -1)
    # label bands hold valid classes (0 / C - 1), so an over-read label would vote
    specs = {"pts": In(torch.from_numpy(pts), ld=ld), "boxes": In(torch.from_numpy(boxes)),
             "labels": In(torch.from_numpy(lab), index=(0, C - 1)),
             "counts": Out((B, K, C), torch.int32), "mode": Out((B, K), torch.int32)}

    def call(t):
        guard.call("ov3d_box_points_count", t["pts"], int(dtype == np.float64), N * ld, ld, N,
                   t["boxes"], 1, t["labels"], C, B, K, t["counts"], t["mode"], like=t["pts"])
    out = guard.run_case(cuda, specs, call)
    counts, mode = R.vote(pts, lab, lo, hi, C)
    assert np.array_equal(out["counts"].cpu().numpy(), counts)
    assert np.array_equal(out["mode"].cpu().numpy(), mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,C,ld", [(1, 1, 1, 3), (63, 7, 18, 3), (64, 8, 32, 4), (65, 9, 18, 3),
                                      (257, 33, 32, 6), (1000, 9, 18, 3)])
def test_guard_label_vote(cuda, N, K, C, ld, dtype):
    _guard_case(cuda, N, K, C, dtype, ld)


def test_guard_label_vote_without_mode(cuda):
    pts, lab, lo, hi = vote_case(65, 9, 18, np.float32)
    specs = {"pts": In(torch.from_numpy(pts)), "boxes": In(torch.from_numpy(np.concatenate([lo, hi], -1))),
             "labels": In(torch.from_numpy(lab), index=(0, 17)), "counts": Out((3, 9, 18), torch.int32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_box_points_count", t["pts"], 0, 65 * 3, 3, 65, t["boxes"], 1, t["labels"], 18, 3, 9,
        t["counts"], None, like=t["pts"]))
    assert np.array_equal(out["counts"].cpu().numpy(), R.vote(pts, lab, lo, hi, 18)[0])


@pytest.mark.parametrize("bad", [dict(kind=2), dict(C=33), dict(C=0), dict(f64=2), dict(N=0),
                                 dict(labels=None)])
def test_guard_rejected_vote_writes_nothing(cuda, bad):
    pts, lab, lo, hi = vote_case(65, 9, 18, np.float32)
    specs = {"pts": In(torch.from_numpy(pts)), "boxes": In(torch.from_numpy(np.concatenate([lo, hi], -1))),
             "labels": In(torch.from_numpy(lab), index=(0, 17)), "counts": Out((3, 9, 18), torch.int32),
             "mode": Out((3, 9), torch.int32)}
    a = dict(kind=1, C=18, f64=0, N=65, labels=True)
    a.update(bad)

    def call(t):
        return guard.raw_call("ov3d_box_points_count", t["pts"], a["f64"], 65 * 3, 3, a["N"],
                              t["boxes"], a["kind"], t["labels"] if a["labels"] else None, a["C"],
                              3, 9, t["counts"], t["mode"], like=t["pts"])
    assert guard.run_case(cuda, specs, call, expect_reject=True) == (-1, -1)
