"""Pool labelling and pseudo-label assessment on the GPU (csrc/poollabel.hip behind
include/ov3d_poollabel.h): the product against the reference's recorded files and counts
(tests/golden/pool_label.npz) byte for byte, through the array and the file drivers; both
kernels against the numpy restatement (tests/pool_label_ref.py) on ragged CSR groups at the
shapes where they can go wrong (scans of 0, 1, 3, 4, 5, 63, 65, 1023, 1025 and 4099 vertices
mixed so that the uint8 label rows start at every byte alignment; 0, 1, 7, 8, 9, 17 and 25
boxes around the tile of 8; 1, 41 and 64 bins; 0, 1 and 3 frames of 1, 63, 257 and 240 x 320
pixels); the same calls between guard bands (tests/guard.py); one group inside a hipGraph
capture; and the launch census."""
import os

import numpy as np
import pytest
import torch

import guard
import pool_label_cases as PC
import pool_label_ref as R
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_pool_label_cpu import GOLD, SCAN, same

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_poollabel_vote", "ov3d_poollabel_confusion")

BIG = np.finfo(np.float64).max
# vertices per scan, boxes per scan, vertex dtype, row stride, min_label, bins
VOTE_GROUPS = {
    "one": ((4099,), (17,), np.float32, 3, 3, 41),
    "five": ((1, 0, 3, 65, 1023), (1, 7, 0, 9, 8), np.float64, 4, 3, 64),
    "four": ((5, 4, 63, 1025), (25, 17, 1, 0), np.float32, 6, 0, 1),
    "three": ((3, 4099, 1), (8, 9, 7), np.float64, 3, 3, 41),
}
# frames per scan, pixels per frame
CONF_GROUPS = {
    "frame": ((3,), 240 * 320),
    "five": ((1, 0, 3, 1, 3), 63),
    "three": ((3, 1, 0), 257),
    "pixel": ((0, 1), 1),
    "pixels": ((1, 3, 1, 3), 1),
}


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def vote_case(name):
    """everything on a 1/8 grid, so that vertices sit on bounds; a NaN vertex per scan of 5 or
    more; labels 0 .. 69 (past every bin count); per scan with boxes one box that spans every
    finite number (an over-read vertex would be counted), one empty one (lo > hi) where there
    are three or more; the columns past the third hold numbers nobody may read"""
    n_pts, n_box, dtype, ld, min_label, C = VOTE_GROUPS[name]
    rng = np.random.Generator(np.random.PCG64(sum(n_pts) + 7 * sum(n_box)))
    pts, boxes = [], []
    for n, k in zip(n_pts, n_box):
        p = np.concatenate([rng.integers(0, 32, (n, 3)) / 8.0, rng.uniform(-9, 9, (n, ld - 3))], 1)
        if n >= 5:
            p[rng.integers(0, n), rng.integers(0, 3)] = np.nan
        lo = rng.integers(0, 24, (k, 3)) / 8.0
        b = np.concatenate([lo, lo + rng.integers(4, 17, (k, 3)) / 8.0], 1)
        if k >= 1:
            b[0] = [-BIG] * 3 + [BIG] * 3
        if k >= 3:
            b[2, [1, 4]] = b[2, [4, 1]]
        pts.append(p.astype(dtype))
        boxes.append(b)
    labels = rng.integers(0, 70, sum(n_pts)).astype(np.uint8)
    labels[rng.random(len(labels)) < 0.3] = min_label       # a majority to find
    return dict(pts=np.concatenate(pts), labels=labels, pt_off=offsets(n_pts), boxes=np.concatenate(boxes),
                box_off=offsets(n_box), min_label=min_label, C=C, ld=ld)


def conf_case(name):
    """runs of equal bytes and single ones, every byte value in both arrays where they fit"""
    frames, HW = CONF_GROUPS[name]
    F = sum(frames)
    rng = np.random.Generator(np.random.PCG64(F * HW))
    runs = lambda: np.repeat(rng.integers(0, 256, F * HW), rng.integers(1, 9, F * HW))[:F * HW]   # noqa: E731
    gt = runs().astype(np.uint8).reshape(F, HW)
    pseudo = np.where(rng.random(F * HW) < 0.5, runs() % 19, runs()).astype(np.uint8).reshape(F, HW)
    gt_map = rng.integers(0, 19, 256).astype(np.uint8)
    return dict(gt=gt, pseudo=pseudo, frame_off=offsets(frames), gt_map=gt_map)


@pytest.fixture(scope="module")
def refs():
    """case and restated outputs per group, computed once and left alone"""
    out = {}
    for name in VOTE_GROUPS:
        c = vote_case(name)
        out["vote", name] = (c, R.vote(c["pts"], c["labels"], c["pt_off"], c["boxes"], c["box_off"],
                                       c["min_label"], c["C"]))
    for name in CONF_GROUPS:
        c = conf_case(name)
        out["conf", name] = (c, R.confusion(c["gt"], c["pseudo"], c["frame_off"], c["gt_map"], 18))
    return out


# ---------------------------------------------------------------- kernels

@pytest.mark.parametrize("name", VOTE_GROUPS)
def test_vote_equals_the_restatement(cuda, refs, name):
    from ov3d_amd import pool_label as PL
    c, (counts, mode) = refs["vote", name]
    got_c, got_m = PL.vote(*(dev(c[k], cuda) for k in ("pts", "labels", "pt_off", "boxes", "box_off")),
                           c["min_label"], c["C"])
    assert same(got_c.cpu().numpy(), counts) and same(got_m.cpu().numpy(), mode)
    # the case decides something: hits, boxes without a vote, and the spanning box counts
    # every voting vertex of its scan that is not NaN
    assert (mode >= 0).any() and (mode == -1).any() and counts.sum() > 0
    lab, off = c["labels"].astype(np.int64), c["pt_off"]
    s = int(np.argmax(np.diff(c["box_off"]) > 0))
    votes = (lab[off[s]: off[s + 1]] >= c["min_label"]) & (lab[off[s]: off[s + 1]] < c["C"])
    finite = np.isfinite(c["pts"][off[s]: off[s + 1], :3]).all(1)
    assert counts[c["box_off"][s]].sum() == (votes & finite).sum()


@pytest.mark.parametrize("name", CONF_GROUPS)
def test_confusion_equals_the_restatement(cuda, refs, name):
    from ov3d_amd import label_assess as LA
    c, want = refs["conf", name]
    t = {k: dev(v, cuda) for k, v in c.items()}
    got = LA.confusion(t["gt"], t["pseudo"], t["frame_off"], t["gt_map"])
    assert same(got.cpu().numpy(), want)
    assert want.sum() == c["gt"].size and (name != "frame" or (want[0] > 0).all())
    # pseudo one byte off gt's alignment: the byte-by-byte path gives the same counts
    shifted = torch.empty(c["pseudo"].size + 1, dtype=torch.uint8, device=cuda)[1:].view(c["pseudo"].shape)
    shifted.copy_(t["pseudo"])
    assert (shifted.data_ptr() - t["gt"].data_ptr()) % 16 == 1
    assert same(LA.confusion(t["gt"], shifted, t["frame_off"], t["gt_map"]).cpu().numpy(), want)


@pytest.mark.parametrize("name", VOTE_GROUPS)
def test_vote_guard_bands(cuda, refs, name):
    """no write outside the outputs, no result that depends on bytes outside the inputs (the
    label bands hold a voting label, the spanning boxes would count an over-read vertex), every
    output element written"""
    c, (counts, mode) = refs["vote", name]
    N, P, S, ld, C = len(c["pts"]), len(c["boxes"]), len(c["pt_off"]) - 1, c["ld"], c["C"]
    specs = {"pts": In(torch.from_numpy(c["pts"][:, :3].copy()), ld=ld),
             "labels": In(torch.from_numpy(c["labels"]), index=(c["min_label"], C - 1)),
             "pt_off": In(torch.from_numpy(c["pt_off"]), index=(0, 0)),
             "boxes": In(torch.from_numpy(c["boxes"])),
             "box_off": In(torch.from_numpy(c["box_off"]), index=(0, 0)),
             "counts": Out((P, C), torch.int32), "mode": Out((P,), torch.int32)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_poollabel_vote", t["pts"], int(c["pts"].dtype == np.float64), ld, t["labels"], t["pt_off"], N,
        t["boxes"], t["box_off"], P, S, c["min_label"], C, t["counts"], t["mode"], like=t["boxes"]))
    assert same(out["counts"].cpu().numpy(), counts) and same(out["mode"].cpu().numpy(), mode)


@pytest.mark.parametrize("name", CONF_GROUPS)
def test_confusion_guard_bands(cuda, refs, name):
    c, want = refs["conf", name]
    F, HW = c["gt"].shape
    S = len(c["frame_off"]) - 1
    specs = {"gt": In(torch.from_numpy(c["gt"]), index=(3, 200)), "pseudo": In(torch.from_numpy(c["pseudo"]), index=(1, 40)),
             "frame_off": In(torch.from_numpy(c["frame_off"]), index=(0, 0)),
             "gt_map": In(torch.from_numpy(c["gt_map"]), index=(0, 18)), "conf": Out((S, 19, 19), torch.int64)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_poollabel_confusion", t["gt"], t["pseudo"], t["frame_off"], F, HW, S, t["gt_map"], 18, t["conf"],
        like=t["gt_map"]))
    assert same(out["conf"].cpu().numpy(), want)


@pytest.mark.parametrize("bad", [dict(S=0), dict(C=65), dict(ld=2), dict(K=32), dict(HW=0)])
def test_guard_rejected_calls_write_nothing(cuda, refs, bad):
    a = dict(S=5, C=64, ld=4, K=18, HW=63)
    a.update(bad)
    if set(bad) & {"K", "HW"}:
        c, _ = refs["conf", "five"]
        specs = {k: In(torch.from_numpy(c[k])) for k in ("gt", "pseudo", "frame_off", "gt_map")}
        specs["conf"] = Out((5, 33, 33), torch.int64)
        call = lambda t: guard.raw_call("ov3d_poollabel_confusion", t["gt"], t["pseudo"], t["frame_off"], 8,   # noqa: E731
                                        a["HW"], 5, t["gt_map"], a["K"], t["conf"], like=t["gt_map"])
    else:
        c, _ = refs["vote", "five"]
        specs = {k: In(torch.from_numpy(c[k])) for k in ("pts", "labels", "pt_off", "boxes", "box_off")}
        specs.update(counts=Out((len(c["boxes"]), 65), torch.int32), mode=Out((len(c["boxes"]),), torch.int32))
        call = lambda t: guard.raw_call("ov3d_poollabel_vote", t["pts"], 1, a["ld"], t["labels"], t["pt_off"],   # noqa: E731
                                        len(c["pts"]), t["boxes"], t["box_off"], len(c["boxes"]), a["S"], 3, a["C"],
                                        t["counts"], t["mode"], like=t["boxes"])
    assert guard.run_case(cuda, specs, call, expect_reject=True) == (-1, -1)


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("name", PC.LABEL_CASES + PC.SHAPE_CASES)
def test_label_pool_equals_the_reference(cuda, name, tmp_path):
    from ov3d_amd import pool_label as PL
    case = PC.label_case(name)
    want = GOLD["label/" + name]
    assert same(PL.label_pool(case["points"], case["labels"], case["pool"], device=cuda), want)
    dirs = PC.write_label_tree(case, str(tmp_path), SCAN)
    labeler = PL.PoolLabeler(*dirs, str(tmp_path / "out"), device=cuda)
    assert labeler.labeling(SCAN) == len(want)
    assert same(np.load(str(tmp_path / "out" / (SCAN + "_bbox.npy"))), want)


@pytest.mark.parametrize("name", PC.ASSESS_CASES)
def test_match_equals_the_reference(cuda, name):
    from ov3d_amd import label_assess as LA
    case = PC.assess_case(name)
    want = tuple(GOLD["assess/" + name].tolist())
    assert LA.match(case["gt"], case["pseudo"], device=cuda) == want
    conf = LA.frame_confusion(case["gt"], case["pseudo"], device=cuda)
    assert same(conf, R.group([LA._frames(case["gt"], case["pseudo"], name)])[0])
    assert (int(np.trace(conf)), int(conf.sum())) == want


def test_groups_are_one_launch_and_one_read_back(cuda, tmp_path, monkeypatch):
    """the file driver over mixed float32 / float64 scans and the assessment over several scans:
    one entry call and one device -> host copy per group, results equal to the recording"""
    from ov3d_amd import _native, label_assess as LA, pool_label as PL
    names = ("f32", "none", "f64", "one", "f32")
    scans = [f"scene{i:04d}_00" for i in range(len(names))]
    for scan, name in zip(scans, names):
        dirs = PC.write_label_tree(PC.label_case(name), str(tmp_path), scan)
    cases = [PC.assess_case(n) for n in ("a", "a", "a", "b")]
    copies = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.shape), cpu(self, *a, **k))[1])
    _native.census_start()
    counts = PL.PoolLabeler(*dirs, str(tmp_path / "out"), device=cuda, group=2).run(scans)
    pairs, count, total, conf = LA.assess(((f"s{i}", c["gt"], c["pseudo"]) for i, c in enumerate(cases)),
                                          device=cuda, group=2)
    census = _native.census_stop()
    monkeypatch.undo()
    assert census == {"ov3d_poollabel_vote": 3, "ov3d_poollabel_confusion": 3} and len(copies) == 6
    assert counts == [len(GOLD["label/" + n]) for n in names]
    for scan, name in zip(scans, names):
        assert same(np.load(os.path.join(str(tmp_path), "out", scan + "_bbox.npy")), GOLD["label/" + name])
    want = [tuple(GOLD["assess/" + n].tolist()) for n in ("a", "a", "a", "b")]
    assert pairs == want and (count, total) == (sum(c for c, _ in want), sum(t for _, t in want))
    assert conf.sum() == total and np.trace(conf) == count


def test_a_group_is_capturable(cuda, refs):
    """one vote and one confusion launch inside a hipGraph capture replay to the same result (a
    synchronisation or a device -> host copy would raise there)"""
    from ov3d_amd import label_assess as LA, pool_label as PL
    v, (counts, mode) = refs["vote", "five"]
    c, conf = refs["conf", "five"]
    tv = [dev(v[k], cuda) for k in ("pts", "labels", "pt_off", "boxes", "box_off")]
    tc = [dev(c[k], cuda) for k in ("gt", "pseudo", "frame_off", "gt_map")]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up outside the capture
        PL.vote(*tv, v["min_label"], v["C"])
        LA.confusion(*tc)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_c, got_m = PL.vote(*tv, v["min_label"], v["C"])
        got_conf = LA.confusion(*tc)
    for t in (got_c, got_m, got_conf):
        t.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert same(got_c.cpu().numpy(), counts) and same(got_m.cpu().numpy(), mode)
    assert same(got_conf.cpu().numpy(), conf)
