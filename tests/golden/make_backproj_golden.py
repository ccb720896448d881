"""Writes tests/golden/backproj.npz: the REFERENCE's own image_processor.compute_projection
(utils/image_util.py) and ProjectionHelper.project (utils/projection.py), loaded by file path,
unchanged, run on the CPU over backproj_cases.py.

The two files ask for a CUDA device and for imageio and torchvision at import: torch.Tensor.cuda
is the identity while they run, and empty stand-in modules go into sys.modules (nothing of them
is called: the frame file decoding is not part of this).  The per-frame `print` is swallowed.

Recorded per case: the inputs, both (F, N+1) tables as int32, every frame's projected features
and the composition `out[:, idx] = project(...)[:, idx]` over the frames in order.  Asserted per
case, or the generator fails: no decision quantity is inside its margin (backproj_cases.evaluate),
the float64 decisions give the recorded tables, and in the main case each of the four filters
(frustum, pixel range, depth range, depth agreement) accepts something and rejects something.

The archive is written member by member with a fixed timestamp, so a re-run reproduces the file
byte for byte."""
import contextlib
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import backproj_cases as BC  # noqa: E402

REF = os.environ.get("OV3D_REFERENCE", "/root/reference")


def load_reference():
    """-> the reference's utils.image_util module (utils.projection loaded beside it)"""
    for name in ("imageio", "torchvision", "torchvision.transforms"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["imageio"].imread = None
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision.transforms"].InterpolationMode = None
    pkg = types.ModuleType("utils")
    pkg.__path__ = []
    sys.modules["utils"] = pkg
    mods = {}
    for name in ("projection", "image_util"):
        spec = importlib.util.spec_from_file_location("utils." + name, os.path.join(REF, "utils", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["utils." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["image_util"]


def write_archive(path, arrays):
    with zipfile.ZipFile(path, "w") as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        mod = load_reference()
        proc = mod.image_processor()
        par = BC.R.params()
        for name in BC.CASES:
            case = BC.case(name)
            pts, depth, poses, feats = (case[k] for k in ("points", "depth", "poses", "features"))
            N, F = len(pts), len(poses)
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                i3, i2 = proc.compute_projection(pts, depth, poses)
            i3, i2 = i3.numpy(), i2.numpy()
            assert i3.shape == i2.shape == (F, N + 1) and i3.dtype == np.int64
            ev = BC.evaluate(pts, depth, poses, par)
            assert not ev["near"].any(), (name, "points inside a margin", int(ev["near"].sum()))
            for f in range(F):
                idx = np.nonzero(ev["keep"][f])[0]
                assert i3[f, 0] == i2[f, 0] == len(idx), (name, f, int(i3[f, 0]), len(idx))
                assert np.array_equal(i3[f, 1:1 + len(idx)], idx) and not i3[f, 1 + len(idx):].any(), (name, f)
                assert np.array_equal(i2[f, 1:1 + len(idx)], ev["pixel"][f][idx]) and not i2[f, 1 + len(idx):].any()
            if name == "main":
                for filt, (yes, no) in ev["stats"].items():
                    assert yes > 0 and no > 0, (name, filt, yes, no)
            projected = np.stack([proc.PROJECTOR.project(torch.from_numpy(feats[f]), torch.from_numpy(i3[f]),
                                                         torch.from_numpy(i2[f]), N).numpy() for f in range(F)])
            composed = np.zeros((feats.shape[1], N), np.float32)
            for f in range(F):
                idx = i3[f, 1:1 + i3[f, 0]]
                composed[:, idx] = projected[f][:, idx]
            assert np.abs(i3).max() < 2 ** 31 and np.abs(i2).max() < 2 ** 31
            out.update({name + "/points": pts, name + "/depth": depth, name + "/poses": poses,
                        name + "/features": feats, name + "/idx3d": i3.astype(np.int32),
                        name + "/idx2d": i2.astype(np.int32), name + "/projected": projected,
                        name + "/composed": composed})
            mapped = int((i3[:, 0] > 0).sum())
            print(f"{name}: {N} vertices, {F} frames ({mapped} map something, "
                  f"{said.getvalue().count('found')} reported), per frame {i3[:, 0].tolist()}, "
                  f"{int((composed != 0).any(0).sum())} vertices with features, filters {ev['stats']}")
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "backproj.npz")
    write_archive(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
