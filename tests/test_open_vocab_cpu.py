"""Open-vocabulary classification without a GPU: the export set of include/ov3d_openvocab.h and
the entry's argument validation (before any launch), the host refusals of ov3d_amd.open_vocab
(before any native call), prepare_text against float64, the writers' files through their
consumers' own loading code, and the exclusion cap of the rounded GPU cases on the float64
restatement alone (tests/open_vocab_ref.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import open_vocab_ref as R
from helpers import ROOT, ov3d  # noqa: F401


@pytest.fixture
def OV(monkeypatch):
    """the module with a native door that fails the test when anything goes through it"""
    from ov3d_amd import _native, open_vocab

    def refuse(name, *a, **k):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_native, "call", refuse)
    return open_vocab


def test_exports_are_the_header():
    from ov3d_amd import _native
    with open(os.path.join(ROOT, "include", "ov3d_openvocab.h")) as f:
        protos = _native.read_header(f.read())[1]
    assert set(_native.HEADER_EXPORTS["ov3d_openvocab.h"]) == set(protos) == {"ov3d_openvocab_classify"}
    lib = _native.load()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_entry_rejects_invalid_arguments():
    """validation happens before any launch (no device needed)"""
    from ov3d_amd import _native, open_vocab
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    ok = dict(feat=p, dtype=1, planes=0, R=65, C=13, P=0, text=p, T=3, unseen=3, label=p, score=p, norm=p)

    def classify(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_openvocab_classify(a["feat"], a["dtype"], a["planes"], a["R"], a["C"], a["P"], a["text"],
                                           a["T"], a["unseen"], a["label"], a["score"], a["norm"], None)
    for name in ("feat", "text", "label", "score", "norm"):
        assert classify(**{name: None}) == -1, name
    assert classify(dtype=-1) == -1 and classify(dtype=3) == -1 and classify(planes=2) == -1 and classify(planes=-1) == -1
    assert classify(R=0) == -1 and classify(R=-5) == -1 and classify(R=1 << 31) == -1
    assert classify(C=0) == -1 and classify(C=open_vocab.MAX_C + 1) == -1
    assert classify(T=0) == -1 and classify(T=open_vocab.MAX_T + 1) == -1
    assert classify(planes=1, P=0) == -1 and classify(planes=1, P=-1) == -1 and classify(planes=1, P=64) == -1
    assert (open_vocab.MAX_T, open_vocab.MAX_C) == (256, 4096)


def test_host_refusals_come_before_any_native_call(OV):
    from ov3d_amd import _native
    f = torch.zeros(8, 16)
    t = torch.zeros(3, 16)
    with pytest.raises(TypeError, match="tensors"):
        OV.classify_rows(f.numpy(), t)
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        OV.classify_rows(f.double(), t.double())
    with pytest.raises(TypeError, match="prepare_text"):
        OV.classify_rows(f.bfloat16(), t)
    with pytest.raises(ValueError, match="2-d features"):
        OV.classify_rows(f[None], t)
    with pytest.raises(ValueError, match="4-d features"):
        OV.classify_frames(f, t)
    with pytest.raises(ValueError, match="text"):
        OV.classify_rows(f, t[0])
    with pytest.raises(ValueError, match="channels"):
        OV.classify_rows(f, torch.zeros(3, 15))
    with pytest.raises(ValueError, match="channels"):
        OV.classify_frames(torch.zeros(2, 15, 4, 4), t)
    with pytest.raises(ValueError, match="T = 257"):
        OV.classify_rows(f, torch.zeros(257, 16))
    with pytest.raises(ValueError, match="T = 0"):
        OV.classify_rows(f, torch.zeros(0, 16))
    with pytest.raises(ValueError, match="C = 4097"):
        OV.classify_rows(torch.zeros(2, 4097), torch.zeros(3, 4097))
    with pytest.raises(ValueError, match="rows"):
        OV.classify_rows(torch.zeros(0, 16), t)
    with pytest.raises(ValueError, match="text is on"):
        OV.classify_rows(torch.zeros(8, 16, device="meta"), t)
    with pytest.raises(ValueError, match="unseen"):
        OV.classify_rows(f, t, unseen=1 << 31)
    with pytest.raises(ValueError, match="min_sim"):
        OV.classify_rows(f, t, min_sim=float("nan"))
    # all in order, but on the host: there is no CPU fallback
    with pytest.raises(_native.NativeError, match="ROCm device only"):
        OV.classify_rows(f, t)
    with pytest.raises(_native.NativeError, match="ROCm device only"):
        OV.classify_frames(torch.zeros(2, 16, 4, 4), t)
    with pytest.raises(_native.NativeError, match="ROCm device only"):
        OV.vertex_labels_from_frames(np.zeros((5, 3)), np.zeros((2, 32, 41)), np.zeros((2, 4, 4)),
                                     torch.zeros(2, 16, 32, 41), t)


def _neighbours(v):
    """the representable values next to every element of the bfloat16 / float16 / float32 tensor"""
    ints = {2: torch.int16, 4: torch.int32}[v.element_size()]
    bits = v.view(ints).to(torch.int64)
    mag, sign = bits & (2 ** (8 * v.element_size() - 1) - 1), bits < 0
    out = []
    for step in (-1, 1):
        m = mag + step
        flip = m < 0                                  # below +-0: the smallest value of the other sign
        m = torch.where(flip, torch.ones_like(m), m)
        s = sign ^ flip
        full = torch.where(s, m - 2 ** (8 * v.element_size() - 1), m)
        out.append(full.to(ints).view(v.dtype).to(torch.float64).numpy())
    return out


@pytest.mark.parametrize("name", list(R.DTYPES))
def test_prepare_text_against_float64(OV, name):
    dtype = R.DTYPES[name]
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((19, 512)) * np.exp(rng.uniform(-3, 3, (19, 1)))
    raw[7] = 0.0
    got = OV.prepare_text(raw, dtype)
    assert got.dtype == dtype and got.shape == (19, 512) and got.device.type == "cpu"
    n = np.sqrt((raw * raw).sum(1, keepdims=True))
    want = np.divide(raw, n, out=np.zeros_like(raw), where=n > 0)
    v = got.to(torch.float64).numpy()
    # one rounding: no representable value is closer to the float64 quotient
    err = np.abs(v - want)
    for other in _neighbours(got):
        assert (err <= np.abs(other - want)).all()
    assert not v[7].any() and np.allclose((v * v).sum(1)[np.arange(19) != 7], 1.0, atol=2.0 ** -6)
    # a tensor input keeps its device; normalize=False is the cast alone
    again = OV.prepare_text(torch.from_numpy(raw), dtype)
    assert torch.equal(again, got)
    ints = rng.integers(-3, 4, (5, 8)).astype(np.float64)
    plain = OV.prepare_text(ints, dtype, normalize=False)
    assert plain.dtype == dtype and np.array_equal(plain.to(torch.float64).numpy(), ints)
    with pytest.raises(TypeError):
        OV.prepare_text(raw, torch.float64)
    with pytest.raises(ValueError):
        OV.prepare_text(raw[0], dtype)


def test_bfloat16_text_is_rounded_once(OV):
    """values a float32 stop on the way would round the wrong way: just above a bfloat16 tie by
    less than half a float32 ulp"""
    tie = 1.0 + 2.0 ** -8                              # halfway between bfloat16 1.0 and 1.0078125
    x = np.array([[tie + 2.0 ** -30, tie - 2.0 ** -30, -(tie + 2.0 ** -30), tie]])
    got = OV.prepare_text(x, torch.bfloat16, normalize=False).to(torch.float64).numpy()
    assert got.tolist() == [[1.0078125, 1.0, -1.0078125, 1.0]]


def test_vertex_file_loads_through_its_consumers(OV, tmp_path):
    from ov3d_amd import label_formatter as LF
    rng = np.random.default_rng(2)
    for dt in (np.float32, np.float64):
        xyz = rng.uniform(-3, 3, (50, 3)).astype(dt)
        label = rng.integers(0, 20, 50).astype(np.int32)
        path = str(tmp_path / f"scene_{np.dtype(dt).name}.npy")
        OV.save_vertex_labels(path, torch.from_numpy(xyz), torch.from_numpy(label))
        # ScannetBoxLifter.lift_one's read
        sem = np.load(path, allow_pickle=False)
        assert sem.dtype == dt and sem.shape == (50, 4)
        assert np.array_equal(sem[:, :3], xyz) and np.array_equal(sem[:, 3], label)
        # LabelFormatter's read
        fmt = LF.LabelFormatter(None, None, str(tmp_path), [f"scene_{np.dtype(dt).name}"], device="cpu")
        got_xyz, got_label = fmt._scan(0)
        assert got_xyz.dtype == dt and np.array_equal(got_xyz, xyz)
        assert got_label.dtype == np.uint8
        assert np.array_equal(got_label, LF.scan_labels(label.astype(dt), 18, "s"))
        assert np.array_equal(got_label[label < 18], label[label < 18])
    with pytest.raises(ValueError):
        OV.save_vertex_labels(str(tmp_path / "bad.npy"), xyz, label[:-1])
    with pytest.raises(TypeError):
        OV.save_vertex_labels(str(tmp_path / "bad.npy"), xyz, label.astype(np.float32))


def test_frame_file_loads_through_its_consumer(OV, tmp_path):
    from ov3d_amd import label_assess as LA
    rng = np.random.default_rng(3)
    ids = [0, 20, 40, 1000]
    maps = rng.integers(0, 20, (4, 32, 41)).astype(np.int32)
    maps[0, 0, 0] = 256                                # unseen at T = 256 still fits
    path = str(tmp_path / "scene0000_00.npy")
    OV.save_frame_labels(path, [f"{i}" for i in ids], torch.from_numpy(maps))
    # assess_pseudo_label.py:32-33, frame ids as the strings of the file names
    x = np.load(path, allow_pickle=True)
    pseudo = np.stack([x.item()[int(i)].astype(np.int64) for i in ("0", "20", "40", "1000")])
    assert pseudo.dtype == np.int64 and np.array_equal(pseudo, maps)
    assert all(x.item()[i].dtype == np.int16 and x.item()[i].shape == (32, 41) for i in ids)
    loaded = OV.load_frame_labels(path, ids)
    assert loaded.dtype == np.int64 and np.array_equal(loaded, pseudo)
    # what label_assess makes of it: classes 0..17, the rest ignored
    gt = np.zeros(maps.shape, np.float32)
    _, ps = LA._frames(gt, loaded, "scene0000_00")
    assert ps.dtype == np.uint8 and np.array_equal(ps.reshape(maps.shape)[maps < 18], maps[maps < 18])
    assert (ps.reshape(maps.shape)[maps >= 18] == LA.IGNORED_BYTE).all()
    with pytest.raises(ValueError):
        OV.save_frame_labels(path, ids[:-1], maps)
    with pytest.raises(ValueError):
        OV.save_frame_labels(path, [0, 0, 1, 2], maps)
    with pytest.raises(TypeError):
        OV.save_frame_labels(path, ids, maps.astype(np.float32))


@pytest.mark.parametrize("T", [19, 200])
@pytest.mark.parametrize("name", list(R.DTYPES))
def test_the_exclusion_rule_hides_little(OV, name, T):
    """the label comparison of the rounded GPU cases may skip near-ties: on the committed
    generators that is under 2 % of the normal rows and none of the prototype rows"""
    dtype = R.DTYPES[name]
    Rr, C = 4096, 512
    feat, text = R.normal_case(Rr, C, T)
    ref = R.classify(R.rounded(feat, dtype)[1], OV.prepare_text(text, dtype).to(torch.float64).numpy())
    share = R.excluded(ref, C).mean()
    print(f"normal {name} T={T}: {100 * share:.2f} % of the rows excluded")
    assert 0 < share <= R.EXCLUDED_CAP
    feat, text = R.prototype_case(Rr, C, T)
    ref = R.classify(R.rounded(feat, dtype)[1], OV.prepare_text(text, dtype).to(torch.float64).numpy())
    assert not R.excluded(ref, C).any()


def test_the_restatement_on_small_cases():
    f = np.array([[1.0, 2.0], [0.0, -0.0], [np.nan, 1.0], [1.0, 1.0], [np.inf, -np.inf]])
    t = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
    ref = R.classify(f, t)
    assert ref["label"].tolist() == [1, 3, 3, 0, 3] and ref["score"].tolist() == [2.0, 0.0, 0.0, 1.0, 0.0]
    t[0, 0] = np.nan                                   # s_0 is NaN everywhere: it never wins
    ref = R.classify(f[[0, 3]], t, unseen=-1)
    assert ref["label"].tolist() == [1, 1] and ref["score"].tolist() == [2.0, 1.0]
    rows = np.arange(24.0).reshape(6, 4)
    planes = R.to_planes(rows, 2, 3)
    assert planes.shape == (2, 4, 3) and planes[1, 2, 0] == rows[3, 2]
