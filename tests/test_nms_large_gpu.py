"""ov3d_nms3d past 512 boxes per scene (nms3d_big_kernel, csrc/nms.hip) and nms_2d_faster.

Against the REFERENCE's own pick lists (tests/golden/nms_large.npz, made by
make_eval_large_golden.py: K = 513 / 1100 / 2048 in 3D, K = 37 / 700 in 2D), against the C
oracle (oracle.nms3d, no K limit) with score ties and valid masks, against the small kernel
byte for byte at K <= 512 (ov3d_eval_large_kernels(1)), the refusal past 2048 and guard bands
around keep_out.  All comparisons are exact: the kernels evaluate the reference's float64
expressions in its order.
"""
import numpy as np
import pytest
import torch

import guard
from eval_large_cases import NMS2D_K, NMS3D_K, NMS_THRESHOLD
from guard import In, Out
from helpers import fixture
from ov3d_amd import nms

pytestmark = pytest.mark.gpu

# the entries this file's cases run between guard bands (tests/guard_cases.py)
ENTRIES = ("ov3d_nms3d",)


def _table(rs, B, K, levels=None):
    """(B, K, 8) boxes dense enough to suppress; scores from `levels` distinct values (ties)
    or tie-free"""
    lo = rs.uniform(-1.2, 1.2, (B, K, 3))
    boxes = np.zeros((B, K, 8))
    boxes[..., 0:3] = lo
    boxes[..., 3:6] = lo + rs.uniform(0.2, 1.5, (B, K, 3))
    boxes[..., 6] = rs.randint(0, levels, (B, K)) / levels if levels else rs.uniform(0, 1, (B, K))
    boxes[..., 7] = rs.randint(0, 4, (B, K))
    return boxes


def _oracle_keep(boxes, valid, old_type, samecls):
    from oracle import oracle as O
    B, K = boxes.shape[:2]
    keep = np.zeros((B, K), np.uint8)
    for b in range(B):
        sub = np.where(valid[b])[0] if valid is not None else np.arange(K)
        if sub.size:
            _, k = O.nms3d(boxes[b, sub], NMS_THRESHOLD, old_type=old_type, samecls=samecls)
            keep[b, sub] = k
    return keep


@pytest.mark.parametrize("old", [False, True])
@pytest.mark.parametrize("i", range(len(NMS3D_K)))
def test_nms3d_large_matches_reference(cuda, i, old):
    fx = fixture("nms_large.npz")
    boxes = fx[f"boxes{i}"]
    assert boxes.shape == (NMS3D_K[i], 8) and boxes.shape[0] > 512
    assert nms.nms_3d_faster_samecls(boxes, NMS_THRESHOLD, old) == fx[f"samecls{i}_{int(old)}"].tolist()
    assert nms.nms_3d_faster(boxes[:, :7], NMS_THRESHOLD, old) == fx[f"any{i}_{int(old)}"].tolist()


@pytest.mark.parametrize("old", [False, True])
@pytest.mark.parametrize("i", range(len(NMS2D_K)))
def test_nms2d_matches_reference(cuda, i, old):
    fx = fixture("nms_large.npz")
    boxes = fx[f"boxes2d{i}"]
    assert boxes.shape == (NMS2D_K[i], 5)
    assert nms.nms_2d_faster(boxes, NMS_THRESHOLD, old) == fx[f"nms2d{i}_{int(old)}"].tolist()


@pytest.mark.parametrize("samecls", [True, False])
@pytest.mark.parametrize("old", [False, True])
@pytest.mark.parametrize("K", [513, 576, 2048])
def test_nms3d_large_vs_oracle_with_ties(cuda, K, old, samecls):
    boxes = _table(np.random.RandomState(K), 3, K, levels=6)
    keep = nms.nms3d_batched(torch.from_numpy(boxes).to(cuda), NMS_THRESHOLD, old_type=old,
                             samecls=samecls).cpu().numpy()
    ref = _oracle_keep(boxes, None, old, samecls)
    assert 0 < ref.sum() < ref.size
    assert np.array_equal(keep, ref), np.argwhere(keep != ref)[:8]


@pytest.mark.parametrize("nvalid", [0, 1, 64, 65, 513])
def test_nms3d_large_valid_mask(cuda, nvalid):
    """B = 3 scenes of 576 rows of which nvalid take part (another subset per scene), ties"""
    K = 576
    rs = np.random.RandomState(100 + nvalid)
    boxes = _table(rs, 3, K, levels=6)
    valid = np.zeros((3, K), bool)
    for b in range(3):
        valid[b, rs.permutation(K)[:nvalid]] = True
    for samecls, old in ((True, False), (False, True)):
        keep = nms.nms3d_batched(torch.from_numpy(boxes).to(cuda), NMS_THRESHOLD, old_type=old,
                                 samecls=samecls, valid=torch.from_numpy(valid).to(cuda)).cpu().numpy()
        ref = _oracle_keep(boxes, valid, old, samecls)
        assert not keep[~valid].any()
        assert np.array_equal(keep, ref), np.argwhere(keep != ref)[:8]
        assert (ref.sum(1) >= min(nvalid, 1)).all()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130, 512])
def test_large_kernel_equals_small_kernel(cuda, K):
    """the same inputs through both kernels: keep equal byte for byte"""
    rs = np.random.RandomState(K)
    boxes = torch.from_numpy(_table(rs, 3, K, levels=6)).to(cuda)
    valid = torch.from_numpy(rs.rand(3, K) < 0.8).to(cuda)
    cases = [(old, same, v) for old in (False, True) for same in (True, False) for v in (None, valid)]
    prev = nms.large_kernels(-1)
    try:
        nms.large_kernels(0)
        small = [nms.nms3d_batched(boxes, NMS_THRESHOLD, o, s, v) for o, s, v in cases]
        assert nms.large_kernels(1) == 0
        large = [nms.nms3d_batched(boxes, NMS_THRESHOLD, o, s, v) for o, s, v in cases]
        assert nms.large_kernels(-1) == 1
    finally:
        nms.large_kernels(prev)
    for c, a, b in zip(cases, small, large):
        assert a.dtype == torch.uint8 and torch.equal(a, b), c[:2]
    if K >= 63:   # boxes were suppressed, so the comparison is not of all-ones masks
        assert cases[6] == (True, False, None) and int(small[6].sum()) < 3 * K


def test_more_than_2048_boxes_are_refused(cuda):
    assert nms.MAX_K == 2048
    boxes = torch.zeros((1, 2049, 8), dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        nms.nms3d_batched(boxes, NMS_THRESHOLD)
    # the entry itself: a status, and nothing written
    specs = {"boxes": In(torch.zeros((1, 2049, 8), dtype=torch.float64)),
             "keep": Out((1, 2049), torch.uint8)}
    rc = guard.run_case(cuda, specs, lambda t: guard.raw_call(
        "ov3d_nms3d", t["boxes"], None, 1, 2049, 8, NMS_THRESHOLD, 0, 1, t["keep"], like=t["keep"]),
        expect_reject=True)
    assert rc == (-1, -1)


def test_large_kernel_stays_inside_keep_out(cuda):
    """K = 513, B = 2 between guard bands: keep_out written completely and nothing beyond it,
    the result independent of the bytes around the inputs, and equal to the oracle's"""
    B, K = 2, 513
    rs = np.random.RandomState(5)
    boxes = _table(rs, B, K, levels=6)
    valid = rs.rand(B, K) < 0.9
    specs = {"boxes": In(torch.from_numpy(boxes)), "valid": In(torch.from_numpy(valid.astype(np.uint8))),
             "keep": Out((B, K), torch.uint8)}
    out = guard.run_case(cuda, specs, lambda t: guard.call(
        "ov3d_nms3d", t["boxes"], t["valid"], B, K, 8, NMS_THRESHOLD, 0, 1, t["keep"], like=t["keep"]))
    assert np.array_equal(out["keep"].cpu().numpy(), _oracle_keep(boxes, valid, False, True))
