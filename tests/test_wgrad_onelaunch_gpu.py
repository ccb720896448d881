"""Grouped weight gradients with the problem table in device memory (csrc/wgrad.hip
ov3d_wgrad_group): one stream-K launch takes every problem of a call, up to CAP; the table
(records, unit / tile prefixes, per-tile slot bases) is written into the head of the caller's
workspace by small writer launches that carry 46 problems each in their arguments.

All cases go through ov3d_wgrad_group on lists longer than one writer launch holds, at shapes
small enough to run in a blink yet large enough for tiles to be split across workgroups
(a 4096-row tile is 64 units; 48 mixed problems give each of the 256 workgroups ~ 15).
Reference: the fp32 product of the same bf16 rows, 1e-5 relative Frobenius (summation order
only, test_wgrad_gpu.py's bound)."""
import ctypes
import random

import pytest
import torch

from helpers import ov3d  # noqa: F401

pytestmark = pytest.mark.gpu

CAP = 512                      # kSKCap of csrc/wgrad.hip: problems per stream-K launch
SLOT = 256 * 256 + 256         # floats of one partial slot (tile + bias columns)
CUT = 48                       # kSKCut: problems per cut group (one workgroup per CU each)
RS = (64, 192, 1024, 4096)
DIMS = (3, 12, 64, 128, 256, 768)


def _problem(dev, g, R, N, K, bias):
    dy = torch.randn(R, N, device=dev, generator=g).to(torch.bfloat16)
    x = torch.randn(R, K, device=dev, generator=g).to(torch.bfloat16)
    return {"dy": dy, "x": x, "dw": torch.empty(N, K, device=dev),
            "db": torch.empty(N, device=dev) if bias else None}


def _reference(p):
    return p["dy"].float().t() @ p["x"].float(), (p["dy"].float().sum(0) if p["db"] is not None else None)


def _array(probs):
    from ov3d_amd import _native
    P = _native.struct("ov3d_wgrad_problem")
    return (P * len(probs))(*[
        P(p["dy"].data_ptr(), p["dy"].stride(0), p["x"].data_ptr(), p["x"].stride(0),
          p["dy"].shape[0], p["dy"].shape[1], p["x"].shape[1], 1, p["dw"].data_ptr(),
          p["dw"].stride(0), p["db"].data_ptr() if p["db"] is not None else None) for p in probs])


def _plan_slots(probs, cus):
    """-> (partial slots, tiles) of the one-launch plan of csrc/wgrad.hip: the problems form cut
    groups of CUT; a group's (tile, 64-row stage) units, in list order, are cut into one equal
    range per CU; a tile whose units fall to more than one workgroup has a slot per workgroup."""
    slots = ntiles = 0
    for c in range(0, len(probs), CUT):
        tiles = [(-(-p["dy"].shape[1] // 256) * -(-p["x"].shape[1] // 256), -(-p["dy"].shape[0] // 64))
                 for p in probs[c:c + CUT]]
        U = sum(nt * st for nt, st in tiles)
        G = min(cus, U)
        u = 0
        for nt, st in tiles:
            for _ in range(nt):
                wf, wl = ((u + 1) * G - 1) // U, ((u + st) * G - 1) // U
                slots += wl - wf + 1 if wl != wf else 0
                u += st
        ntiles += sum(nt for nt, _ in tiles)
    return slots, ntiles


def _workspace_floats(probs):
    from ov3d_amd import _native
    arr = _array(probs)
    return _native.load().ov3d_wgrad_group_workspace(ctypes.addressof(arr), len(probs))


def _run(probs, ws=None):
    from ov3d_amd import _native
    arr = _array(probs)
    if ws is None:
        n = _native.load().ov3d_wgrad_group_workspace(ctypes.addressof(arr), len(probs))
        ws = torch.empty(max(n, 1), dtype=torch.float32, device=probs[0]["dy"].device)
    _native.call("ov3d_wgrad_group", ctypes.addressof(arr), len(probs), ws, like=ws)
    return ws


def _outputs(probs):
    return [t.clone() for p in probs for t in (p["dw"], p["db"]) if t is not None]


def _poison(probs):
    for p in probs:
        p["dw"].fill_(float("nan"))
        if p["db"] is not None:
            p["db"].fill_(float("nan"))


def _check(probs, refs):
    for i, (p, (rw, rb)) in enumerate(zip(probs, refs)):
        shape = (i, tuple(p["dy"].shape), p["x"].shape[1])
        assert ((p["dw"] - rw).norm() / rw.norm()).item() <= 1e-5, shape
        if rb is not None:
            assert ((p["db"] - rb).norm() / rb.norm()).item() <= 1e-5, shape


@pytest.fixture(scope="module")
def mixed(cuda):
    """104 problems (the first 60 are the shorter list) and their references, computed once"""
    g = torch.Generator(device=cuda)
    g.manual_seed(11)
    rnd = random.Random(3)
    probs = []
    for i in range(104):
        if i == 7:
            probs.append(_problem(cuda, g, 4096, 768, 256, True))
            continue
        # every R, N and K value comes round; the pairing is shuffled
        probs.append(_problem(cuda, g, RS[i % 4], DIMS[(i // 4) % 6], rnd.choice(DIMS), i % 3 != 0))
    return probs, [_reference(p) for p in probs]


@pytest.mark.parametrize("n", [60, 104])
def test_mixed_lists_match_fp32_product(mixed, n):
    probs, refs = mixed[0][:n], mixed[1][:n]
    _poison(probs)
    _run(probs)
    _check(probs, refs)


def test_cap_plus_one_problems_chunk(cuda):
    """CAP + 1 problems: CAP in the first launch, one 256 x 256, 1024-row problem (16 units,
    16 workgroups, 16 slots) alone in the second"""
    g = torch.Generator(device=cuda)
    g.manual_seed(5)
    n = CAP + 1
    dy = torch.randn(n, 64, 16, device=cuda, generator=g).to(torch.bfloat16)
    x = torch.randn(n, 64, 24, device=cuda, generator=g).to(torch.bfloat16)
    dw = torch.full((n, 16, 24), float("nan"), device=cuda)
    db = torch.full((n, 16), float("nan"), device=cuda)
    probs = [{"dy": dy[i], "x": x[i], "dw": dw[i], "db": db[i]} for i in range(CAP)]
    probs.append(_problem(cuda, g, 1024, 256, 256, True))
    _poison(probs[-1:])
    _run(probs)
    rw = torch.bmm(dy[:CAP].float().transpose(1, 2), x[:CAP].float())
    rb = dy[:CAP].float().sum(1)
    err = (dw[:CAP] - rw).flatten(1).norm(dim=1) / rw.flatten(1).norm(dim=1)
    assert err.max().item() <= 1e-5
    assert ((db[:CAP] - rb).norm(dim=1) / rb.norm(dim=1)).max().item() <= 1e-5
    _check(probs[-1:], [_reference(probs[-1])])


@pytest.mark.parametrize("shapes", [
    [(4096, 256, 256)],                  # n = 1, 64 units: one workgroup per unit, 64 slots
    [(24576, 512, 256)],                 # n = 1, 768 units: three per workgroup
    [(192, 64, 64)] * 3,                 # 9 units, fewer than CUs: one workgroup per unit (G = U),
    [(192, 64, 64), (128, 12, 3)],       # 5 units: so every tile is split over its stages
], ids=["one-64u", "one-768u", "three-9u", "two-5u"])
def test_edge_lists(cuda, shapes):
    g = torch.Generator(device=cuda)
    g.manual_seed(len(shapes))
    probs = [_problem(cuda, g, R, N, K, True) for R, N, K in shapes]
    _poison(probs)
    _run(probs)
    _check(probs, [_reference(p) for p in probs])


def test_two_calls_are_bit_identical(mixed):
    probs = mixed[0]
    _poison(probs)
    _run(probs)
    first = _outputs(probs)
    _poison(probs)
    _run(probs)
    for a, b in zip(first, _outputs(probs)):
        assert torch.equal(a, b)


def test_captured_call_replays_on_rewritten_inputs(cuda, mixed):
    """The table must reach the device on every replay: the workspace is wiped and other
    memory allocated and freed between replays, the inputs are rewritten in place, and each
    replay must equal an eager call (its own fresh workspace) bit for bit."""
    src = mixed[0][:60]
    probs = [{"dy": p["dy"].clone(), "x": p["x"].clone(), "dw": torch.empty_like(p["dw"]),
              "db": torch.empty_like(p["db"]) if p["db"] is not None else None} for p in src]
    ws = torch.empty(_workspace_floats(probs), device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(probs, ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(probs, ws)
    g = torch.Generator(device=cuda)
    for rep in range(3):
        g.manual_seed(100 + rep)
        for p in probs:
            p["dy"].copy_(torch.randn(p["dy"].shape, device=cuda, generator=g))
            p["x"].copy_(torch.randn(p["x"].shape, device=cuda, generator=g))
        ws.zero_()
        scratch = torch.full((1 << 20,), float(rep), device=cuda)
        del scratch
        _poison(probs)
        graph.replay()
        replayed = _outputs(probs)
        _poison(probs)
        _run(probs)
        for a, b in zip(replayed, _outputs(probs)):
            assert torch.equal(a, b), rep


def test_workspace_holds_slots_and_table_and_is_enough(cuda, mixed):
    """the reported size covers the plan's partial slots plus the table, and a buffer of
    exactly that size is enough: NaN guards on both sides stay untouched"""
    probs, refs = mixed[0][:60], mixed[1][:60]
    n = _workspace_floats(probs)
    slots, ntiles = _plan_slots(probs, torch.cuda.get_device_properties(cuda).multi_processor_count)
    assert slots > 0
    k = len(probs)
    table = 64 * k + 8 * (k + 1) + 4 * (k + 1) + 4 * (ntiles + 1) + 4 * ntiles
    assert 4 * n >= 4 * SLOT * slots + table
    guard = 4096
    buf = torch.full((n + 2 * guard,), float("nan"), device=cuda)
    _poison(probs)
    _run(probs, buf[guard:guard + n])
    _check(probs, refs)
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
