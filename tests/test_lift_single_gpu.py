"""Single-view pseudo-box lifting on the GPU (csrc/liftview.hip behind include/ov3d_liftview.h):
the entry against the numpy restatement (tests/lift_single_ref.py), bit for bit, at the
smallest shapes where it can go wrong; the uint16 depth conversion over all 65536 raw values;
the scan-level call and the file driver against the reference's recorded files
(tests/golden/lift_single.npz); device label tensors and uint16 depth against the host float
path; the chain inside a hipGraph capture; the guard-band cases (tests/guard.py) at the ragged
shapes; and the result, through to_training_format, loaded by
ScannetDetectionDataset(use_pbox=True)."""
import numpy as np
import pytest
import torch

import guard
import lift_single_cases as SC
import lift_single_ref as SR
from guard import In, Out
from helpers import ov3d  # noqa: F401
from test_lift_ref_cpu import check_lifted, same
from test_lift_single_cpu import GOLD, single_bar

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_liftview_frames",)

SHAPES = [(1, 1), (3, 5), (7, 259), (240, 320)]
SEG_VALUES = (0, 3, 17, 18, 25, -7, 39, 40, 4)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def entry_case(F, H, W):
    """random maps over SEG_VALUES; the last pixel of every frame is the only one of value 5;
    a non-trivial intrinsic, pose per frame and alignment"""
    rng = np.random.Generator(np.random.PCG64(1000 * F + 7 * H + W))
    seg = rng.choice(SEG_VALUES, (F, H, W)).astype(np.int32)
    seg[:, H - 1, W - 1] = 5
    raw = rng.integers(0, 6000, (F, H, W)).astype(np.uint16)
    raw[:, 0, 0] = 0                                        # depth 0 takes part
    K = SC.LC.intrinsic()
    K[:2] /= 2.0
    kinv = np.linalg.inv(K[:3, :3]).astype(np.float64)
    P = np.stack([SC.LC.look_at(rng.uniform(-3, -1, 3), rng.uniform(0, 1, 3)) for _ in range(F)]).astype(np.float64)
    pose = np.concatenate([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], 1)
    return seg, raw, kinv, pose, SC.LC.alignment()


def slots_for(F, labels):
    """every (frame, label) pair, then a slot of a frame past the end and one before the start"""
    sf = np.repeat(np.arange(F), len(labels)).astype(np.int32)
    sl = np.tile(np.asarray(labels, np.int32), F)
    return np.concatenate([sf, [F, -1]]).astype(np.int32), np.concatenate([sl, [labels[0]] * 2]).astype(np.int32)


def run_entry(cuda, depth, seg, lut, ignore_from, kinv, pose, A, sf, sl, bs):
    from ov3d_amd import lift_boxes as LB
    rows = torch.full((len(bs), 8), 7.0, dtype=torch.float64, device=cuda)
    count = LB.lift_views(dev(depth, cuda), dev(seg, cuda), None if lut is None else dev(lut, cuda), ignore_from,
                          dev(kinv, cuda), dev(pose, cuda), dev(A, cuda), dev(sf, cuda), dev(sl, cuda),
                          dev(bs, cuda), rows)
    rows = rows.cpu().numpy()
    assert (rows[:, 6:] == 7.0).all()                       # the caller's columns are left alone
    return rows[:, :6], count.cpu().numpy()


def want_entry(depth, cls, kinv, pose, A, sf, sl, bs):
    lohi, count = SR.lift_slots(SR.metres(depth), cls, kinv, pose, A, sf, sl)
    ok = (bs >= 0) & (bs < len(sf))
    at = np.where(ok, bs, 0)
    return np.where(ok[:, None], lohi[at], 0.0), np.where(ok, count[at], 0).astype(np.int32)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_entry_equals_the_restatement(cuda, H, W, F):
    seg, raw, kinv, pose, A = entry_case(F, H, W)
    lut = SR.nyu40_lut().astype(np.int32)
    variants = [  # lut, ignore_from, slot labels
        (None, 18, (0, 3, 17, -7, 5, 9, -100, 18)),         # 9: absent; 18: ignored, so empty
        (None, None, (0, 18, 25, 40, 5, -100)),             # nothing ignored: -100 is empty
        (lut, None, (0, 1, 17, -100, 2, 3)),                # nyu40 3, 4, 39, 5 -> 0, 1, 17, 2; 3: empty
    ]
    rng = np.random.Generator(np.random.PCG64(H + W + F))
    for lut_v, ign, labels in variants:
        sf, sl = slots_for(F, labels)
        S = len(sf)
        bs = np.concatenate([np.arange(S), rng.integers(0, S, 5), [-1, S]]).astype(np.int32)
        cls = SR.classes(seg, lut=lut_v) if lut_v is not None else SR.classes(seg, ignore_from=ign)
        for depth in (raw, SR.metres(raw)):
            want = want_entry(depth, cls, kinv, pose, A, sf, sl, bs)
            got = run_entry(cuda, depth, seg, lut_v, ign, kinv, pose, A, sf, sl, bs)
            assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), (H, W, F, ign, depth.dtype)
            assert same(got[0], want[0]), (H, W, F, ign, depth.dtype)
        count = want[1][:S].reshape(-1)
        assert (count[-2:] == 0).all() and (want[1][-2:] == 0).all()       # foreign frames and slots
        by = dict(zip(zip(sf[:-2].tolist(), sl[:-2].tolist()), count[:-2].tolist()))
        if lut_v is None:
            assert all(by[f, 5] == 1 for f in range(F))     # one pixel: min == max
            one = want[0][[i for i in range(S - 2) if sl[i] == 5]]
            assert same(one[:, :3], one[:, 3:])
        if lut_v is None and ign == 18:
            assert all(by[f, 9] == 0 and by[f, 18] == 0 for f in range(F))
        assert sum(by[0, c] for c in labels) == H * W or lut_v is None
    # a slot that holds the whole frame
    const = np.full_like(seg, 3)
    sf, sl = np.arange(F, dtype=np.int32), np.full(F, 3, np.int32)
    bs = np.arange(F, dtype=np.int32)
    want = want_entry(raw, SR.classes(const), kinv, pose, A, sf, sl, bs)
    got = run_entry(cuda, raw, const, None, 18, kinv, pose, A, sf, sl, bs)
    assert (want[1] == H * W).all() and np.array_equal(got[1], want[1]) and same(got[0], want[0])


def test_uint16_depth_is_the_float32_quotient_for_every_raw_value(cuda):
    """256 frames of 1 x 256 pixels, each pixel its own label and slot; identity intrinsic, pose
    and alignment, so the z column returns every converted depth"""
    raw = np.arange(65536, dtype=np.uint16).reshape(256, 1, 256)
    seg = np.tile(np.arange(256, dtype=np.int32), (256, 1)).reshape(256, 1, 256)
    sf = np.repeat(np.arange(256), 256).astype(np.int32)
    sl = np.tile(np.arange(256), 256).astype(np.int32)
    bs = np.arange(65536, dtype=np.int32)
    kinv, A = np.eye(3), np.eye(4)
    pose = np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]), (256, 1))
    metres = raw.astype(np.float32) / 1000
    got_u, n_u = run_entry(cuda, raw, seg, None, None, kinv, pose, A, sf, sl, bs)
    got_f, n_f = run_entry(cuda, metres, seg, None, None, kinv, pose, A, sf, sl, bs)
    assert (n_u == 1).all() and (n_f == 1).all()
    assert same(got_u[:, 2], metres.reshape(-1).astype(np.float64)) and same(got_u[:, 5], got_u[:, 2])
    assert same(got_u, got_f)


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("name", SC.CASES)
def test_scan_equals_the_reference_file(cuda, name):
    from ov3d_amd import lift_boxes as LB
    case = SC.case(name)
    final, lifted = LB.lift_scannet_scan_single(**case, device=cuda, return_lifted=True)
    assert same(final, GOLD[f"single/{name}/final"])
    check_lifted(lifted, GOLD[f"single/{name}/lifted"], single_bar(case))
    assert same(lifted, SR.scan(**case)[1])                 # and the restatement bit for bit
    # float32 metres for uint16 millimetres; a device label tensor for the host array
    as_float = dict(case, depths=SR.metres(case["depths"]))
    f2, l2 = LB.lift_scannet_scan_single(**as_float, device=cuda, return_lifted=True)
    assert same(f2, final) and same(l2, lifted)
    on_dev = dict(case, labels=dev(case["labels"].astype(np.int32), cuda))
    f3, l3 = LB.lift_scannet_scan_single(**on_dev, device=cuda, return_lifted=True)
    assert same(f3, final) and same(l3, lifted)
    both = dict(on_dev, depths=dev(SR.metres(case["depths"]), cuda))
    f4, l4 = LB.lift_scannet_scan_single(**both, device=cuda, return_lifted=True)
    assert same(f4, final) and same(l4, lifted)


@pytest.mark.parametrize("name", SC.CASES)
def test_file_driver_equals_the_reference_file(cuda, name, tmp_path):
    from ov3d_amd import lift_boxes as LB, open_vocab
    case, scan = SC.case(name), "scene0000_00"
    SC.write_tree(case, str(tmp_path), scan, with_labels=False)
    if case["pseudo"]:                                      # the label file as the product writes it
        open_vocab.save_frame_labels(str(tmp_path / "lseg" / (scan + ".npy")), range(len(case["labels"])),
                                     dev(case["labels"].astype(np.int32), cuda))
    lifter = LB.ScannetBoxLifter(*(str(tmp_path / d) for d in ("lseg", "frames", "boxes2d", "gss", "scans",
                                                               "written")), device=cuda, view="single",
                                 pseudo=case["pseudo"])
    want = GOLD[f"single/{name}/final"]
    assert lifter.lift([scan]) == [want.shape[0]]
    assert same(np.load(str(tmp_path / "written" / (scan + "_bbox.npy"))), want)


def test_chain_is_capturable(cuda):
    """single-view lift -> NMS -> match -> size NMS inside a hipGraph capture: a host
    synchronisation or a device -> host copy raises during capture; seven launches; the
    read-back comes after the replay"""
    from ov3d_amd import _native, lift_boxes as LB
    case = SC.case("main")
    plan = LB.single_host_plan(case["intrinsic"], case["poses"], case["boxes2d"])
    M = len(plan["box_slot"])
    rows_h = np.zeros((M, 8))
    rows_h[:, 6:] = plan["score_label"]
    t = [dev(x, cuda) for x in (case["depths"], case["labels"].astype(np.int32), plan["kinv"], plan["pose"],
                                case["axis_align_matrix"], plan["slot_frame"], plan["slot_label"],
                                plan["box_slot"], rows_h, case["gss_pool"])]
    packed, out, count, rank2 = LB.result_buffer(M, cuda)

    def chain():
        LB.lift_views(t[0], t[1], None, 18, *t[2:9], count)
        LB.chain_tail(t[8], count, t[9], out, rank2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _native.census_start()
        chain()                                            # warm-up outside the capture
        calls = _native.census_stop()
    torch.cuda.current_stream().wait_stream(side)
    assert calls == {"ov3d_liftview_frames": 1, "ov3d_lift_nms": 2, "ov3d_lift_match": 1}   # 2 + 1 + 3 + 1
    packed.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    graph.replay()
    torch.cuda.synchronize()
    assert same(LB._finish(packed, M, 7), GOLD["single/main/final"])


def test_result_loads_as_training_boxes(cuda, tmp_path):
    from ov3d_amd import lift_boxes as LB, scannet
    from ov3d_amd.dataset_config import ScannetDatasetConfig
    case, scan = SC.case("main"), "scene0000_00"
    final = LB.lift_scannet_scan_single(**case, device=cuda)
    root, meta, pbox = (tmp_path / d for d in ("det", "meta", "pbox"))
    for d in (root, meta, pbox):
        d.mkdir()
    rng = np.random.Generator(np.random.PCG64(3))
    vert = np.concatenate([rng.uniform(-3, 3, (400, 3)), np.full((400, 3), 128.0)], 1).astype(np.float32)
    np.save(str(root / (scan + "_vert.npy")), vert)
    (meta / "scannetv2_train.txt").write_text(scan + "\n")
    np.save(str(pbox / (scan + "_bbox.npy")), LB.to_training_format(final))
    cfg = ScannetDatasetConfig()
    ds = scannet.ScannetDetectionDataset(cfg, split_set="train", root_dir=str(root), meta_data_dir=str(meta),
                                         pseudo_box_dir=str(pbox), num_points=256, use_pbox=True, device=cuda)
    batch = ds.get_batch([0], rng=np.random.RandomState(0))
    k = final.shape[0]
    assert k >= 2 and int(batch["gt_box_present"].sum()) == k
    assert batch["gt_box_sem_cls_label"][0, :k].tolist() == [int(c) for c in final[:, 6]]
    assert np.allclose(batch["gt_box_centers"][0, :k].cpu().numpy(), final[:, :3].astype(np.float32))


# ---------------------------------------------------------------- guard bands

def guard_specs(F, H, W, u16, use_lut):
    seg, raw, kinv, pose, A = entry_case(F, H, W)
    labels = (0, 1, 17, -100, 2) if use_lut else (0, 3, 17, -7, 5, 9, -100)
    sf, sl = slots_for(F, labels)
    sf, sl = sf[:-2], sl[:-2]                               # slots of the call's own frames only
    S = len(sf)
    bs = np.concatenate([np.arange(S), [0, S - 1, S // 2]]).astype(np.int32)
    lut = SR.nyu40_lut().astype(np.int32)
    depth = raw.view(np.int16) if u16 else SR.metres(raw)   # uint16 bits; the entry takes a pointer
    specs = {"depth": In(torch.from_numpy(depth)), "seg": In(torch.from_numpy(seg), index=(3, 4)),
             "lut": In(torch.from_numpy(lut), index=(0, 1)) if use_lut else None,
             "kinv": In(torch.from_numpy(kinv)), "pose": In(torch.from_numpy(pose)), "A": In(torch.from_numpy(A)),
             "sf": In(torch.from_numpy(sf), index=(0, F - 1)), "sl": In(torch.from_numpy(sl), index=(0, 3)),
             "bs": In(torch.from_numpy(bs), index=(0, S - 1)),
             "slot_lohi": Out((S, 6), torch.float64), "slot_count": Out((S,), torch.int32),
             "lohi": Out((len(bs), 6), torch.float64, ld=9), "count": Out((len(bs),), torch.int32)}
    cls = SR.classes(seg, lut=lut) if use_lut else SR.classes(seg, ignore_from=18)
    return specs, (raw, cls, kinv, pose, A, sf, sl, bs), (F, H, W, S, len(bs))


def guard_call(t, dims, u16, use_lut, fn):
    F, H, W, S, M = dims
    return fn("ov3d_liftview_frames", t["depth"], int(u16), t["seg"], t["lut"], 40 if use_lut else 0, 18, F, H, W,
              t["kinv"], t["pose"], t["A"], t["sf"], t["sl"], S, t["bs"], M, t["slot_lohi"], t["slot_count"],
              t["lohi"], 9, t["count"], like=t["seg"])


@pytest.mark.parametrize("u16,use_lut", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("F,H,W", [(1, 1, 1), (3, 3, 5), (2, 7, 259), (3, 33, 31)])
def test_guard_liftview(cuda, F, H, W, u16, use_lut):
    specs, ref_args, dims = guard_specs(F, H, W, u16, use_lut)
    out = guard.run_case(cuda, specs, lambda t: guard_call(t, dims, u16, use_lut, guard.call))
    lohi, count = want_entry(*ref_args)
    assert np.array_equal(out["count"].cpu().numpy(), count) and same(out["lohi"].cpu().numpy(), lohi)
    assert count.sum() > 0


@pytest.mark.parametrize("bad", [dict(F=0), dict(S=0), dict(M=0), dict(u16=2), dict(H=1 << 16, W=1 << 15)])
def test_guard_rejected_call_writes_nothing(cuda, bad):
    specs, _, (F, H, W, S, M) = guard_specs(2, 7, 259, 0, False)
    a = dict(F=F, H=H, W=W, S=S, M=M, u16=0)
    a.update(bad)
    dims = (a["F"], a["H"], a["W"], a["S"], a["M"])
    assert guard.run_case(cuda, specs, lambda t: guard_call(t, dims, a["u16"], False, guard.raw_call),
                          expect_reject=True) == (-1, -1)
