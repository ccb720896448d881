"""ctypes binding of ``lib/libov3d_hip.so`` (the C ABI declared in include/ov3d.h and the
include/ov3d_*.h beside it).

This is the only door from Python to the hot-path kernels.  There is no CPU
fallback: if the library is missing, or a tensor is not on a ROCm device, the
call raises.  Pointers are ``tensor.data_ptr()``; the stream is torch's current
HIP stream on the tensor's device, so every op is stream-ordered with the
surrounding torch work and capturable into a hipGraph.
"""
import ctypes
import glob
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libov3d_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ov3d.h")

OV3D_GIOU_CYTHON = 0
OV3D_GIOU_TENSOR = 1

_lib = None


class NativeError(RuntimeError):
    pass


# The closed set of C types the headers use.  Any pointer is a c_void_p, so that
# data_ptr() ints, None and byref() all pass.
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float,
            "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char *": ctypes.c_char_p}


def _ctype(ctype, decl):
    if "*" in ctype:
        return ctypes.c_void_p
    if ctype.strip() not in _SCALARS:
        raise NativeError(f"include/ov3d.h: `{decl}` has a type the binding does not know "
                          f"({', '.join(_SCALARS)} or a pointer)")
    return _SCALARS[ctype.strip()]


def read_header(text):
    """C header text -> ({struct: [(field, ctype)]}, {function: (restype, [argtypes])}) for every
    `typedef struct { ... } name;` and every prototype; a declaration outside the closed set of
    types raises NativeError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = dict(re.findall(r"^#define\s+(\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M))
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{|^\}\s*$', "", text, flags=re.M)
    structs = {}

    def read_struct(m):
        fields = structs[m.group(2)] = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            # type, then one or more names, each with an optional [length]
            dm = re.fullmatch(r"(.*?[\s*])(\w+(?:\[\w+\])?(?:, ?\w+(?:\[\w+\])?)*)", decl)
            names = re.findall(r"(\w+)(?:\[(\w+)\])?", dm.group(2)) if dm else []
            lengths = [defines.get(length, length) for _, length in names]
            if dm is None or not all(n == "" or n.isdigit() for n in lengths):
                raise NativeError(f"include/ov3d.h: cannot read the field `{decl}` of {m.group(2)}")
            ct = _ctype(dm.group(1), decl)
            fields += [(name, ct * int(n) if n else ct) for (name, _), n in zip(names, lengths)]
        return ""

    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", read_struct, text, flags=re.S)
    protos = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.*?[\s*])(\w+) ?\((.*)\)", decl)
        ret = m and " ".join(m.group(1).replace("*", " * ").split())
        if m is None or ret not in _RETURNS:
            raise NativeError(f"include/ov3d.h: cannot read the declaration `{decl}`")
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        protos[m.group(2)] = (_RETURNS[ret], [_ctype(p if "*" in p else p.rpartition(" ")[0], decl)
                                              for p in params])
    return structs, protos


def read_headers(paths):
    """header files -> ({struct: fields}, {function: prototype}, {file name: its functions}); a
    missing file, or a function or struct name declared in two of them, raises NativeError"""
    structs, protos, exports, owner = {}, {}, {}, {}
    for path in paths:
        if not os.path.exists(path):
            raise NativeError(f"{path} not found: the ctypes binding is derived from it")
        with open(path) as f:
            s, p = read_header(f.read())
        for name in (*s, *p):
            if name in owner:
                raise NativeError(f"`{name}` is declared in both {owner[name]} and {path}")
            owner[name] = path
        structs.update(s)
        protos.update(p)
        exports[os.path.basename(path)] = tuple(p)
    return structs, protos, exports


# One reader for every header: include/ov3d.h, then each feature's include/ov3d_*.h as the
# directory lists them, so a header added later is bound without a change here.
HEADER_PATHS = (HEADER_PATH, *sorted(glob.glob(os.path.join(os.path.dirname(HEADER_PATH), "ov3d_*.h"))))
_STRUCT_FIELDS, _PROTOS, HEADER_EXPORTS = read_headers(HEADER_PATHS)
EXPORTS = tuple(_PROTOS)
_STRUCTS = {}


def struct(name):
    """the ctypes.Structure of a struct of the headers (fields in its header's order)"""
    if name not in _STRUCTS:
        _STRUCTS[name] = type(name, (ctypes.Structure,), {"_fields_": _STRUCT_FIELDS[name]})
    return _STRUCTS[name]


def load():
    """Load libov3d_hip.so (raises if it was not built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback); "
                "build it with `make -C open-vocabulary-3d-object-detection_amd/csrc`")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = lib
    return _lib


def version():
    return load().ov3d_version().decode()


def stream_create(device):
    """-> torch.cuda.ExternalStream over a new HIP stream of the caller's own (ov3d_stream_create):
    unlike torch.cuda.Stream() it never comes from (or returns to) PyTorch's recycled pool.  The
    stream lives for the process."""
    with torch.cuda.device(device):
        h = ctypes.c_void_p()
        rc = load().ov3d_stream_create(ctypes.byref(h))
        if rc != 0 or not h.value:
            raise NativeError(f"ov3d_stream_create failed with status {rc}")
        return torch.cuda.ExternalStream(h.value, device=device)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def check_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if t.device.type != "cuda":
        raise NativeError(f"{name}: ov3d kernels run on the ROCm device only (got {t.device})")
    return t


def check(t, name, dtype=None, ndim=None):
    check_device(t, name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim}-d tensor, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


# Optional per-launch timing (bench.py): HIP events recorded on the launch stream.
_TIMING = {}


def timing_enable(names):
    _TIMING.clear()
    for n in names:
        _TIMING[n] = []


def timing_collect():
    """-> {name: [{"ms": float, "shape": (int args...)}]}; synchronises the events."""
    out = {}
    for n, recs in _TIMING.items():
        out[n] = []
        for ev0, ev1, shape in recs:
            ev1.synchronize()
            out[n].append({"ms": ev0.elapsed_time(ev1), "shape": shape})
    _TIMING.clear()
    return out


# Optional launch census (tests): the set of entry points called while enabled.
_CALLED = None


STAMP_KINDS = ("fwd", "dq", "dkdv", "gemm256")


def stamps_arm(buf, min_work=1 << 20):
    """arm the attention kernels' in-kernel launch stamps into the int64 device tensor buf (None
    disarms; the launch table stays readable).  Launches captured into a graph while armed keep
    stamping on every replay."""
    lib = load()
    if buf is None:
        lib.ov3d_stamps_arm(None, 0, 0)
    else:
        lib.ov3d_stamps_arm(buf.data_ptr(), buf.numel(), int(min_work))


def stamps_read(buf):
    """-> [(kind, launch duration ms, Lq * Lk)] for every recorded launch whose slots hold
    stamps: max(exit) - min(entry) over its waves (wall clock, ov3d_wall_clock_khz)."""
    lib = load()
    khz = lib.ov3d_wall_clock_khz()
    host = buf.cpu()
    out = []
    for i in range(lib.ov3d_stamps_count()):
        kind, off, waves, work = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
        lib.ov3d_stamps_get(i, ctypes.byref(kind), ctypes.byref(off), ctypes.byref(waves), ctypes.byref(work))
        st = host[off.value: off.value + 2 * waves.value].view(-1, 2)
        if bool((st == 0).any()):
            continue
        out.append((STAMP_KINDS[kind.value], (st[:, 1].max() - st[:, 0].min()).item() / khz, work.value))
    return out


def census_start():
    global _CALLED
    _CALLED = {}


def census_stop():
    """-> {entry point: number of calls} since census_start()"""
    global _CALLED
    out, _CALLED = _CALLED or {}, None
    return out


def note(name):
    """count a launch made without call() (census)"""
    if _CALLED is not None:
        _CALLED[name] = _CALLED.get(name, 0) + 1


def call(name, *args, like):
    """Invoke `name` with args (+ the current stream of `like`); raise on nonzero status."""
    fn = getattr(load(), name)
    note(name)
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor) or a is None:
            conv.append(_ptr(a))
        else:
            conv.append(a)
    rec = _TIMING.get(name)
    if rec is not None:
        stream = torch.cuda.current_stream(like.device)
        ev0 = torch.cuda.Event(enable_timing=True)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
    rc = fn(*conv, _stream(like))
    if rec is not None:
        ev1.record(stream)
        rec.append((ev0, ev1, tuple(a for a in args if isinstance(a, int))[:3]))
    if rc != 0:
        raise NativeError(f"{name} failed with status {rc}")


SunLabelsArgs = struct("ov3d_sun_labels_args")
ScanLabelsArgs = struct("ov3d_scan_labels_args")


def byref(struct):
    """address of a ctypes structure, for a pointer argument (the caller keeps it alive)"""
    return ctypes.c_void_p(ctypes.addressof(struct))


def multi_copy(dsts, srcs):
    """copy every src tensor into the same-size dst tensor (contiguous, device) in one launch"""
    n = len(dsts)
    if n == 0:
        return
    for d, s in zip(dsts, srcs):
        if d.nbytes != s.nbytes or not (d.is_contiguous() and s.is_contiguous()) or d.dtype != s.dtype:
            raise ValueError("multi_copy: contiguous same-dtype, same-size tensors only")
        check_device(d, "multi_copy dst")
        check_device(s, "multi_copy src")
    sp = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
    dp = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts])
    nb = (ctypes.c_longlong * n)(*[d.nbytes for d in dsts])
    call("ov3d_multi_copy", n, ctypes.addressof(sp), ctypes.addressof(dp), ctypes.addressof(nb),
         like=dsts[0])
