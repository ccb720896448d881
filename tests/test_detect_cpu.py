"""Detecting with any vocabulary, without a GPU: the export set of include/ov3d_detect.h and the
entry's argument validation (before any launch), the float64 restatement
(tests/vocab_score_ref.py) against a direct softmax on hand cases, its NMS against the reference's
recorded picks (tests/golden/nms.npz), the committed seed of the synthetic chain case, and the
host refusals of ov3d_amd.detect (before any native call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vocab_score_ref as V
from helpers import ROOT, fixture, ov3d  # noqa: F401


@pytest.fixture
def D(monkeypatch):
    """the module with a native door that fails the test when anything goes through it"""
    from ov3d_amd import _native, detect

    def refuse(name, *a, **k):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_native, "call", refuse)
    return detect


def test_exports_are_the_header():
    from ov3d_amd import _native, detect
    with open(os.path.join(ROOT, "include", "ov3d_detect.h")) as f:
        text = f.read()
    protos = _native.read_header(text)[1]
    assert set(_native.HEADER_EXPORTS["ov3d_detect.h"]) == set(protos) == {"ov3d_vocab_score"}
    lib = _native.load()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    for name, value in (("MAX_T", detect.MAX_T), ("MAX_C", detect.MAX_C), ("MAX_K", detect.MAX_K),
                        ("TILE_T", detect.TILE_T)):
        assert f"#define OV3D_DETECT_{name} {value} " in text, name
    assert (detect.MAX_T, detect.MAX_C, detect.MAX_K) == (4096, 4096, 16)
    # the prototype lives in this header alone
    inc = os.path.join(ROOT, "include")
    assert [f for f in sorted(os.listdir(inc)) if "ov3d_vocab_score" in open(os.path.join(inc, f)).read()] == \
        ["ov3d_detect.h"]


def test_entry_rejects_invalid_arguments():
    """validation happens before any launch (no device needed)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok = dict(feat=p, dtype=0, R=65, C=13, ldf=16, text=p, T=3, bg=2, scale=1.0, K=5, obj=p, lse=p, cls=p, prob=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_vocab_score(a["feat"], a["dtype"], a["R"], a["C"], a["ldf"], a["text"], a["T"], a["bg"],
                                    a["scale"], a["K"], a["obj"], a["lse"], a["cls"], a["prob"], None)
    for name in ("feat", "text", "obj", "lse", "cls", "prob"):
        assert call(**{name: None}) == -1, name
    assert call(dtype=-1) == -1 and call(dtype=2) == -1          # float16 is not taken
    assert call(R=0) == -1 and call(R=-5) == -1 and call(R=1 << 31) == -1
    assert call(C=0) == -1 and call(C=4097) == -1 and call(ldf=12) == -1
    assert call(T=0) == -1 and call(T=4097) == -1
    assert call(bg=3) == -1 and call(bg=-2) == -1
    assert call(K=0) == -1 and call(K=17) == -1
    assert call(scale=float("nan")) == -1 and call(scale=float("inf")) == -1


def test_the_restatement_on_hand_cases():
    # T = 1: with the background the row has no foreground, without it the one class is certain
    f = np.array([[1.0, 2.0], [-3.0, 0.5]])
    r = V.score(f, np.array([[0.5, 0.25]]), 0, 1.0, 3)
    assert r["obj"].tolist() == [0.0, 0.0] and (r["top_cls"] == -1).all() and not r["top_prob"].any()
    assert r["lse"].tolist() == [1.0, -1.375]
    r = V.score(f, np.array([[0.5, 0.25]]), -1, 1.0, 3)
    assert r["obj"].tolist() == [1.0, 1.0] and r["top_cls"].tolist() == [[0, -1, -1]] * 2
    assert r["top_prob"].tolist() == [[1.0, 0.0, 0.0]] * 2 and r["lse"].tolist() == [1.0, -1.375]
    # a tie goes to the smaller index; K larger than the foreground pads with -1 and 0
    t = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [0.0, 0.0]])
    f = np.array([[2.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    for bg in (4, 1, -1):
        for scale in (1.0, 0.5):
            r = V.score(f, t, bg, scale, 6)
            for i in range(3):
                p, obj = V.softmax_direct(scale * (f[i] @ t.T), bg)
                fgs = [c for c in range(5) if c != bg]
                want = sorted(fgs, key=lambda c: (-p[c], c))
                n = len(fgs)
                assert r["top_cls"][i].tolist() == want + [-1] * (6 - n)
                assert np.allclose(r["top_prob"][i, :n], p[want], rtol=1e-14, atol=0) and not r["top_prob"][i, n:].any()
                assert abs(r["obj"][i] - obj) <= 1e-15 and (bg >= 0 or r["obj"][i] == 1.0)
                assert abs(r["lse"][i] - np.log(np.exp(scale * (f[i] @ t.T)).sum())) <= 1e-14
    r = V.score(f, t, 4, 1.0, 6)
    assert r["top_cls"][0].tolist() == [0, 2, 3, 1, -1, -1]       # 0 and 2 tie
    assert r["top_cls"][2].tolist() == [0, 1, 2, 3, -1, -1]       # an all-zero row: uniform, first indices
    assert np.allclose(r["top_prob"][2, :4], 0.2) and abs(r["obj"][2] - 0.8) < 1e-15
    # a non-finite score: never a detection
    f[1, 0] = np.nan
    f[2, 1] = np.inf
    r = V.score(f, t, 4, 1.0, 2)
    assert r["obj"].tolist()[1:] == [0.0, 0.0] and np.isnan(r["lse"][1:]).all() and np.isfinite(r["lse"][0])
    assert (r["top_cls"][1:] == -1).all() and not r["top_prob"][1:].any()
    # a background that dominates by more than A_CAP: obj underflows in float32, not here
    r = V.score(np.array([[200.0, 0.0]]), np.array([[0.0, 1.0], [1.0, 0.0]]), 1, 1.0, 1)
    assert 0 < r["obj"][0] < 1e-80 and r["top_cls"].tolist() == [[0]]


def test_the_exact_family_is_exact_and_has_ties():
    for C in (1, 8, 13, 96, 520, 640):
        feat, text = V.exact_case(65, C, 17)
        k = V.exact_shift(C)
        s = feat @ text.T
        assert np.array_equal(s * 2.0 ** k, np.rint(s * 2.0 ** k)) and np.abs(s * 2.0 ** k).max() < 2 ** 24
        for dt in (torch.float32, torch.bfloat16):
            assert np.array_equal(torch.from_numpy(feat).to(dt).double().numpy(), feat)
            assert np.array_equal(torch.from_numpy(text).to(dt).double().numpy(), text)
        if C >= 8:
            assert 0.5 < s.std() < 2.0, (C, s.std())
    feat, text = V.exact_case(1000, 96, 4096)
    r = V.score(feat, text, 4095, 1.0, 16)
    top = np.take_along_axis(r["s"], r["top_cls"].astype(np.int64), 1)
    assert (top[:, 1:] == top[:, :-1]).any(1).mean() > 0.5


def test_the_nms_restatement_against_the_recorded_picks():
    fx = fixture("nms.npz")
    for i in range(3):
        boxes = fx[f"boxes{i}"]
        for old in (0, 1):
            for name, same in (("samecls", True), ("any", False)):
                keep = V.nms(boxes, 0.25, bool(old), same)
                assert sorted(np.nonzero(keep)[0].tolist()) == sorted(fx[f"{name}{i}_{old}"].tolist()), (i, old, name)
    # the valid mask takes boxes out before the walk
    boxes = fx["boxes1"]
    valid = np.arange(len(boxes)) % 3 != 0
    keep = V.nms(boxes, 0.25, False, True, valid)
    sub = np.nonzero(valid)[0]
    assert not keep[~valid].any() and np.array_equal(keep[sub], V.nms(boxes[sub], 0.25, False, True))


def test_the_committed_chain_case_meets_its_preconditions():
    c = V.chain_case(V.CHAIN_SEED)
    ref = V.score(c["visual"].reshape(128, 64), c["text"], 10, 1.0, 10)
    ok, pairs, thr = V.separated_all(ref, 64, 0.05, 2, 64)
    assert ok and V.top1_clear(ref, 64).all(), (pairs, thr)
    assert (ref["obj"] < 0.05).any() and (ref["obj"] > 0.5).any()     # the threshold is exercised
    lo, hi = V.obj_interval(ref, 64)
    b = V.bars(ref, 64, rounded_dots=True)
    bar = b["obj_rel"] * ref["obj"] + b["obj_floor"]
    assert (lo <= ref["obj"]).all() and (ref["obj"] <= hi).all()
    assert (lo >= ref["obj"] - bar).all() and (hi <= ref["obj"] + bar).all()   # the interval is the tighter one


def test_vocabulary_refusals(D):
    good = np.random.default_rng(0).standard_normal((7, 16))
    v = D.Vocabulary(good, names=[f"n{i}" for i in range(7)])
    assert (v.T, v.C, v.bg, v.scale) == (7, 16, 6, 1.0) and v.text.dtype == torch.float32
    assert np.array_equal(v.text.double().numpy(), good.astype(np.float32).astype(np.float64)) and v.name(3) == "n3"
    assert D.Vocabulary(good, background=None).bg == -1 and D.Vocabulary(good, background=0).bg == 0
    assert D.Vocabulary(good, background=-7).bg == 0
    unit = D.Vocabulary(good, normalize=True, dtype=torch.bfloat16)
    assert unit.text.dtype == torch.bfloat16 and np.allclose((unit.text.double() ** 2).sum(1), 1.0, atol=2.0 ** -6)
    with pytest.raises(ValueError, match="background"):
        D.Vocabulary(good, background=7)
    with pytest.raises(ValueError, match="background"):
        D.Vocabulary(good, background=-8)
    bad = good.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        D.Vocabulary(bad)
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        D.Vocabulary(torch.from_numpy(bad))
    with pytest.raises(ValueError, match="T = 4097"):
        D.Vocabulary(np.zeros((4097, 4)))
    with pytest.raises(ValueError, match="T = 0"):
        D.Vocabulary(np.zeros((0, 4)))
    with pytest.raises(ValueError, match="C = 4097"):
        D.Vocabulary(np.zeros((2, 4097)))
    with pytest.raises(ValueError, match="names"):
        D.Vocabulary(good, names=["a", "b"])
    with pytest.raises(ValueError, match=r"\(T, C\)"):
        D.Vocabulary(good[0])
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        D.Vocabulary(good, dtype=torch.float16)
    with pytest.raises(ValueError, match="scale"):
        D.Vocabulary(good, scale=float("nan"))
    with pytest.raises(ValueError, match="not finite in"):
        with np.errstate(over="ignore"):
            D.Vocabulary(good * 1e39)                   # finite in float64, inf once rounded
    assert D.Vocabulary(np.zeros((4096, 2))).T == 4096


def test_scoring_refusals_come_before_any_native_call(D):
    from ov3d_amd import _native
    vocab = D.Vocabulary(np.ones((5, 16)))
    q = torch.zeros(2, 8, 16)
    with pytest.raises(TypeError, match="Vocabulary"):
        D.score_queries(q, vocab.text)
    with pytest.raises(TypeError, match="tensor"):
        D.score_queries(q.numpy(), vocab)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        D.score_queries(q.double(), vocab)
    with pytest.raises(TypeError, match="dtype="):         # wrong dtype pairing, both ways
        D.score_queries(q.bfloat16(), vocab)
    with pytest.raises(TypeError, match="dtype="):
        D.score_queries(q, D.Vocabulary(np.ones((5, 16)), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="16 channels"):   # channel mismatch
        D.score_queries(torch.zeros(2, 8, 15), vocab)
    with pytest.raises(ValueError, match="k = 17"):
        D.score_queries(q, vocab, topk=17)
    with pytest.raises(ValueError, match="k = 0"):
        D.score_queries(q, vocab, topk=0)
    with pytest.raises(ValueError, match="rows"):
        D.score_queries(torch.zeros(0, 16), vocab)
    with pytest.raises(ValueError, match="adjacent"):
        D.score_queries(torch.zeros(16, 8).t(), vocab)
    with pytest.raises(ValueError, match="evenly spaced"):
        D.score_queries(torch.zeros(4, 9, 16)[:, :8], vocab)
    # all in order, but on the host: there is no CPU fallback
    with pytest.raises(_native.NativeError, match="ROCm device only"):
        D.score_queries(q, vocab)
    stacked = torch.zeros(3, 2, 8, 16)
    assert D._rows(stacked[-1], 16) == (16, 16) and D._rows(stacked[:, :, :, :16][-1], 16) == (16, 16)
    assert D._rows(torch.zeros(2, 8, 24)[..., :16], 16) == (16, 24) and D._rows(torch.zeros(16), 16) == (1, 16)


def test_detect_refusals_come_before_any_native_call(D):
    from ov3d_amd import _native, nms
    vocab = D.Vocabulary(np.ones((5, 16)))
    out = {"visual_embeds": torch.zeros(2, 8, 16), "box_corners": torch.zeros(2, 8, 8, 3)}
    with pytest.raises(ValueError, match="box_corners"):
        D.detect(dict(out, box_corners=torch.zeros(2, 8, 7, 3)), vocab)
    with pytest.raises(ValueError, match="against box_corners"):
        D.detect(dict(out, visual_embeds=torch.zeros(2, 9, 16)), vocab)
    with pytest.raises(ValueError, match="16 channels"):
        D.detect(dict(out, visual_embeds=torch.zeros(2, 8, 15)), vocab)
    with pytest.raises(TypeError, match="dtype="):
        D.detect(dict(out, visual_embeds=torch.zeros(2, 8, 16).bfloat16()), vocab)
    with pytest.raises(ValueError, match="k = 17"):
        D.detect(out, vocab, topk=17)
    with pytest.raises(ValueError, match="point cloud"):
        D.detect(out, vocab, config=D.get_ap_config_dict(remove_empty_box=True))
    with pytest.raises(ValueError, match="per-class proposals"):
        D.detect(out, vocab, config=D.get_ap_config_dict(remove_empty_box=False, per_class_proposal=False))
    big = nms.MAX_K + 1
    with pytest.raises(ValueError, match="nms3d supports"):
        D.detect({"visual_embeds": torch.zeros(1, big, 16), "box_corners": torch.zeros(1, big, 8, 3)}, vocab)
    with pytest.raises(_native.NativeError, match="ROCm device only"):
        D.detect(out, vocab)
    with pytest.raises(TypeError, match="Vocabulary"):
        D.Detector(torch.nn.Linear(2, 2), vocab.text)
    det = D.Detector(torch.nn.Linear(2, 2), vocab, topk=3)
    assert det.vocab is vocab and det.topk == 3 and det.set_vocabulary(D.Vocabulary(np.ones((9, 16)))).vocab.T == 9


def test_to_list_orders_classes_outer_and_boxes_inner(D):
    neg = -float("inf")
    cls = torch.tensor([[[4, 1], [1, -1], [-1, -1], [1, 4]]], dtype=torch.int32)
    score = torch.tensor([[[0.5, 0.25], [0.75, neg], [neg, neg], [0.125, 0.0625]]])
    corners = torch.arange(4 * 24, dtype=torch.float32).view(1, 4, 8, 3)
    got = D.Detections(None, cls, score, None, corners, None).to_list()
    assert [(c, float(s)) for c, _, s in got[0]] == [(1, 0.25), (1, 0.75), (1, 0.125), (4, 0.5), (4, 0.0625)]
    assert [int(b[0, 0]) // 24 for _, b, _ in got[0]] == [0, 1, 3, 0, 3]
    assert got[0][0][1].shape == (8, 3) and got[0][0][1].dtype == np.float32 and got[0][0][2].dtype == np.float32
