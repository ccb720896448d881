"""The C-ABI library: loads, exports every entry point the headers (include/ov3d.h and the
include/ov3d_*.h beside it) declare, and the product refuses CPU tensors (no silent fallback).
No compute here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from helpers import ROOT, ov3d


def header_sources():
    """the text of every header the binding reads, include/ov3d.h first"""
    from ov3d_amd import _native
    assert _native.HEADER_PATHS[0] == _native.HEADER_PATH == os.path.join(ROOT, "include", "ov3d.h")
    assert len(_native.HEADER_PATHS) >= 8
    return [open(p).read() for p in _native.HEADER_PATHS]


def header_symbols():
    found = [name for src in header_sources()
             for name in re.findall(r"^(?:int|long long|const char\*)\s+(ov3d_\w+)\(", src, flags=re.M)]
    assert len(found) == len(set(found))
    return sorted(found)


def test_library_exports_every_header_symbol():
    from ov3d_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 11
    for s in syms:
        assert hasattr(lib, s), s
    assert set(syms) == set(_native.EXPORTS)


P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
# written out from the prototypes of include/ov3d.h: name -> (restype, argtypes)
EXPECTED = {
    "ov3d_version": (ctypes.c_char_p, []),
    "ov3d_wall_clock_khz": (L, []),
    "ov3d_fps": (I, [P, I, I, I, P, P, P, P]),
    "ov3d_bn_finalize": (I, [P, D, I, P, P, F, F, P, P, P, P, P, P, P, P]),
    "ov3d_nms3d": (I, [P, P, I, I, I, D, I, I, P, P]),
    "ov3d_multi_copy": (I, [I, P, P, P, P]),
    "ov3d_stream_create": (I, [P]),
    "ov3d_stamps_arm": (I, [P, L, L]),
    "ov3d_stamps_get": (I, [I, P, P, P, P]),
    "ov3d_wgrad_group_workspace": (L, [P, I]),
    "ov3d_resnorm_bwd_parts": (I, [L, I]),
    "ov3d_scan_labels": (I, [P, P]),
    "ov3d_attn_bwd_dkdv_batch": (I, [P, I, I, I, I, I, F, F, P]),
}


def test_derived_signatures_match_written_out_expectations():
    """argtypes / restype that _native derives from the header vs literals written from it by hand"""
    from ov3d_amd import _native
    lib = _native.load()
    for name, (restype, argtypes) in EXPECTED.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_every_header_symbol_is_bound():
    """every prototype this test's own regular expression finds resolves in the library and has
    argtypes of its parameter count; nothing is left to ctypes' int default"""
    from ov3d_amd import _native
    lib = _native.load()
    src = "\n".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S) for src in header_sources())
    protos = dict(re.findall(r"^(?:int|long long|const char\*)\s+(ov3d_\w+)\(([^)]*)\);", src, flags=re.M))
    assert sorted(protos) == header_symbols()
    assert set(protos) == set(_native.EXPORTS) and len(_native.EXPORTS) == len(protos)
    for name, params in protos.items():
        n = 0 if params.strip() == "void" else len(params.split(","))
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, (name, n)
        assert fn.restype in (ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p), name


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of each struct of the header, as the host C compiler lays it
    out, vs the ctypes.Structure _native derives"""
    from ov3d_amd import _native
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler (cc) on PATH")
    src = open(os.path.join(ROOT, "include", "ov3d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    structs = re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S)
    assert len(structs) >= 10
    # the other headers have to compile as C beside it
    lines = ["#include <stdio.h>", "#include <stddef.h>"]
    lines += [f'#include "{os.path.basename(p)}"' for p in _native.HEADER_PATHS] + ["int main(void) {"]
    for body, name in structs:
        cls = _native.struct(name)
        assert cls is _native.struct(name)           # cached
        # the field names, by this test's own reading: the last word of each declarator
        fields = [re.sub(r"\[.*", "", d).split()[-1].lstrip("*") for decl in body.split(";")
                  if decl.strip() for d in decl.split(",")]
        assert [f for f, _ in cls._fields_] == fields, name
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"),
                    str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    seen = 0
    for key, value in (ln.split() for ln in out.splitlines()):
        name, _, field = key.partition(".")
        cls = _native.struct(name)
        got = getattr(cls, field).offset if field else ctypes.sizeof(cls)
        assert got == int(value), (key, got, value)
        seen += 1
    assert seen == sum(1 + len(_native.struct(n)._fields_) for _, n in structs)
    desc = _native.struct("ov3d_set_loss_desc")
    assert desc.dict_w.size == 8 * 4 and desc.total_order.size == 8 * 4   # arrays sized by a #define


def test_reader_rejects_types_outside_the_closed_set():
    """nothing defaults to int: an unknown parameter, field or return type raises, naming the
    declaration"""
    from ov3d_amd import _native
    good = ("typedef struct { int a, b; float w[2]; const void* p; } ov3d_t;\n"
            "int ov3d_f(const ov3d_t* t, double x);\n")
    structs, protos = _native.read_header(good)
    assert structs == {"ov3d_t": [("a", I), ("b", I), ("w", F * 2), ("p", P)]}
    assert protos == {"ov3d_f": (I, [P, D])}
    with pytest.raises(_native.NativeError, match=r"ov3d_g\(int n, short k\)"):
        _native.read_header(good + "int ov3d_g(int n, short k);\n")
    with pytest.raises(_native.NativeError, match=r"short k"):
        _native.read_header("typedef struct { int n; short k; } ov3d_u;\n" + good)
    with pytest.raises(_native.NativeError, match=r"ov3d_h\(int n\)"):
        _native.read_header(good + "unsigned ov3d_h(int n);\n")
    with pytest.raises(_native.NativeError, match=r"w\[OV3D_UNKNOWN\]"):
        _native.read_header("typedef struct { float w[OV3D_UNKNOWN]; } ov3d_v;\n")


def test_missing_header_fails_loudly():
    from ov3d_amd import _native
    with pytest.raises(_native.NativeError, match="/nonexistent/ov3d.h"):
        _native.read_headers(("/nonexistent/ov3d.h",) + _native.HEADER_PATHS[1:])


def test_a_name_declared_in_two_headers_fails_loudly(tmp_path):
    """entries and structs are unique across the headers: a second declaration would shadow the
    first in the one binding table"""
    from ov3d_amd import _native
    a, b, c, d = (str(tmp_path / n) for n in ("ov3d.h", "ov3d_a.h", "ov3d_b.h", "ov3d_c.h"))
    (tmp_path / "ov3d.h").write_text("typedef struct { int n; } ov3d_t;\nint ov3d_f(const ov3d_t* t);\n")
    (tmp_path / "ov3d_a.h").write_text("int ov3d_g(int n);\nint ov3d_f(double x);\n")
    (tmp_path / "ov3d_b.h").write_text("typedef struct { float w; } ov3d_t;\nint ov3d_h(int n);\n")
    (tmp_path / "ov3d_c.h").write_text("typedef struct { float w; } ov3d_u;\nint ov3d_k(int n);\n")
    structs, protos, exports = _native.read_headers((a, d))
    assert set(structs) == {"ov3d_t", "ov3d_u"} and tuple(protos) == ("ov3d_f", "ov3d_k")
    assert exports == {"ov3d.h": ("ov3d_f",), "ov3d_c.h": ("ov3d_k",)}
    for other, name in ((b, "ov3d_f"), (c, "ov3d_t")):
        with pytest.raises(_native.NativeError) as e:
            _native.read_headers((a, other))
        assert f"`{name}`" in str(e.value) and a in str(e.value) and other in str(e.value)


def test_version_string():
    from ov3d_amd import _native
    assert "gfx950" in _native.version()


def test_no_cpu_fallback():
    from ov3d_amd import _native, pointnet2_utils
    with pytest.raises(_native.NativeError):
        pointnet2_utils.furthest_point_sample(torch.zeros(1, 16, 3), 4)
    from ov3d_amd.box_util import generalized_box3d_iou
    with pytest.raises(_native.NativeError):
        generalized_box3d_iou(torch.zeros(1, 2, 8, 3), torch.zeros(1, 2, 8, 3), torch.tensor([2]))


def test_missing_library_fails_loudly(monkeypatch):
    from ov3d_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libov3d_hip.so")
    with pytest.raises(_native.NativeError):
        _native.load()


def test_package_exports_drop_in_modules():
    import importlib
    for m in ("pointnet2_utils", "pointnet2_modules", "model_3detr", "criterion", "box_util", "nms",
              "dist", "transformer", "helpers", "position_embedding"):
        importlib.import_module("ov3d_amd." + m)
    assert callable(ov3d.build_model) and callable(ov3d.build_criterion)


def test_round4_entries_reject_bad_arguments():
    """The RegionCLIP close / pool / token entries and the squared-distance mask
    kind validate before touching the device (host-side checks; no GPU needed)."""
    from ov3d_amd import _native
    lib = _native.load()
    fake = ctypes.c_void_p(16)   # never dereferenced: every call below fails validation first
    assert lib.ov3d_bias_residual_act(None, 2, 4, 8, None, None, 1, None) == -1
    assert lib.ov3d_bias_residual_act(fake, 2, 4, 7, fake, fake, 1, None) == -1      # cols % 8
    assert lib.ov3d_avgpool2_nhwc(None, 2, 1, 4, 4, 8, None, None) == -1
    assert lib.ov3d_avgpool2_nhwc(fake, 3, 1, 4, 4, 8, fake, None) == -1            # elem bytes
    assert lib.ov3d_attnpool_tokens(None, 2, 1, 81, 64, None, None, None) == -1
    assert lib.ov3d_attn_mask_pack(fake, 3, 1.0, 1, 32, 64, fake, None) == -1        # kind 3


def test_round5_entries_reject_bad_arguments():
    """ov3d_gemm256 / ov3d_conv3x3_gemm256 validate shapes, strides and alignment before any
    launch; ov3d_sa_dy_fused keeps its argument checks (its > 2 GiB inputs route to the 64-bit
    kernel instead of failing).  Host-side checks only."""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(264)    # 8-byte aligned only
    ok = dict(A=p, lda=128, B=p, ldb=128, bias=None, bf=0, R=None, ldr=0, C=p, ldc=64, M=100,
              N=64, K=128, relu=0)

    def g(**kw):
        a = dict(ok, **kw)
        return lib.ov3d_gemm256(a["A"], a["lda"], a["B"], a["ldb"], a["bias"], a["bf"], a["R"],
                                a["ldr"], a["C"], a["ldc"], a["M"], a["N"], a["K"], a["relu"], None)
    assert g(A=None) == -1
    assert g(K=100) == -1             # K % 8
    assert g(N=60, ldc=64) == -1      # N % 8
    assert g(lda=100) == -1           # lda < K
    assert g(ldb=136 + 4) == -1       # ldb % 8
    assert g(C=odd) == -1             # 16-byte alignment
    assert g(R=p, ldr=32) == -1       # ldr < N
    assert g(M=0) == -1
    assert lib.ov3d_conv3x3_gemm256(p, 2, 9, 9, 96, p, 864, None, 0, None, 0, p, 64, 64, 1,
                                    None) == -1   # Cin % 64
    assert lib.ov3d_conv3x3_gemm256(p, 2, 9, 9, 64, p, 512, None, 0, None, 0, p, 64, 64, 1,
                                    None) == -1   # ldb < 9 Cin
    assert lib.ov3d_conv3x3_gemm256(None, 2, 9, 9, 64, p, 576, None, 0, None, 0, p, 64, 64, 1,
                                    None) == -1
    assert lib.ov3d_sa_dy_fused(None, None, None, None, 1 << 23, 128, 256, 64, None, None, None,
                                None, None, None, None, None, None, None, None, 1, None) == -1
    # the fused attention pool: shape limits, strides and alignment
    assert lib.ov3d_attnpool_fused_supported(81, 2560, 40) == 1
    assert lib.ov3d_attnpool_fused_supported(96, 2560, 40) == 0      # ntok + 1 > 96
    assert lib.ov3d_attnpool_fused_supported(81, 2560, 49) == 0      # H > 48
    assert lib.ov3d_attnpool_fused_supported(81, 2500, 40) == 0      # C % 64
    assert lib.ov3d_attnpool_fused(p, p, p, p, 40 * 2560, 2560, 4, 81, 2560, 49, p, None) == -1
    assert lib.ov3d_attnpool_fused(p, p, p, p, 40 * 2560, 2564, 4, 81, 2560, 40, p, None) == -1
    assert lib.ov3d_attnpool_fused(p, p, p, odd, 40 * 2560, 2560, 4, 81, 2560, 40, p, None) == -1
    assert lib.ov3d_attnpool_mean(p, 4, 81, 2564, p, p, None) == -1          # C % 8
    assert lib.ov3d_attnpool_mean(None, 4, 81, 2560, p, p, None) == -1
