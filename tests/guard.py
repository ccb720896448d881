"""Guard bands: does a kernel touch only the memory it was given?

Every operand of a guarded call lives inside one ordinary allocation laid out as
[front band | interior | back band].  The bands (and, with a row stride larger than the logical
width, the gap columns of every row) hold a fixed bit pattern, so that

  G1  a write outside the interior changes a sentinel and is reported with its byte offset;
  G2  a result that depends on bytes outside the inputs differs between a run whose input
      bands hold quiet NaNs (fill "A") and one whose bands hold the largest finite value
      (fill "B"), or is not finite;
  G3  an output element that was never written still holds the pre-fill sentinel.

Nothing here can fault: an overrun of up to a whole tile lands in a band of the same
allocation.  Index-typed inputs get bands of valid in-range values (different for A and B), so
an over-read that is dereferenced changes the output instead of forming a wild address.

The interior base is 16 bytes past a 512-byte boundary: 16-byte aligned and no more, which is
all include/ov3d.h asks of callers (pass align= where an entry documents more).
"""
import math

import torch

MIN_BAND = 64 * 1024
TILE_ROWS = 256

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# fill A: quiet NaN with a recognisable payload; fill B: the largest finite value
_FLOAT_SENTINEL = {
    torch.float32: {"A": 0x7FC0A5A5, "B": 0x7F7FFFFF},
    torch.bfloat16: {"A": 0x7FD5, "B": 0x7F7F},
    torch.float16: {"A": 0x7ED5, "B": 0x7BFF},
    torch.float64: {"A": 0x7FF8A5A5A5A5A5A5, "B": 0x7FEFFFFFFFFFFFFF},
}
# integer and byte buffers: 0x5A bytes (outputs, and inputs under fill A); inputs under fill B
# get 0xA5 bytes so that G2 sees a dependence on them
_BYTE_SENTINEL = {"A": 0x5A, "B": 0xA5}


def _signed(pattern, itemsize):
    bits = 8 * itemsize
    if itemsize == 1:
        return pattern
    return pattern - (1 << bits) if pattern >= 1 << (bits - 1) else pattern


def sentinel(dtype, fill):
    """the band bit pattern of `dtype` under `fill`, as a value of the same-width integer type"""
    itemsize = torch.empty((), dtype=dtype).element_size()
    if dtype in _FLOAT_SENTINEL:
        return _signed(_FLOAT_SENTINEL[dtype][fill], itemsize)
    b = _BYTE_SENTINEL[fill]
    return _signed(int.from_bytes(bytes([b]) * itemsize, "little"), itemsize)


class Banded:
    """handle of one banded buffer: .view is the interior (logical shape, row stride ld)"""

    def __init__(self, buf, front, shape, ld, dtype, pattern, name):
        self.buf, self.front, self.shape, self.ld, self.dtype = buf, front, tuple(shape), ld, dtype
        self.pattern, self.name = pattern, name
        self.itemsize = torch.empty((), dtype=dtype).element_size()
        self.int_dtype = _INT[self.itemsize]
        self.view = self._interior(buf).view(dtype)

    def _strides(self):
        strides, acc = [1], self.ld
        for d in reversed(self.shape[1:-1]):
            strides.insert(0, acc)
            acc *= d
        if len(self.shape) > 1:
            strides.insert(0, acc)
        return strides[-len(self.shape):]

    def _interior(self, buf):
        """the logical elements of `buf` (a flat uint8 buffer of this layout) as integers"""
        ints = buf.view(self.int_dtype)
        return ints.as_strided(self.shape, self._strides(), self.front // self.itemsize)

    def ints(self):
        """contiguous copy of the interior's bit patterns"""
        return self._interior(self.buf).clone()

    def set(self, data):
        self.view.copy_(data.to(self.view.device).reshape(self.shape))
        return self

    def assert_bands_intact(self):
        """G1: every guard byte (front band, gap columns, back band) still holds its sentinel"""
        copy = self.buf.clone()
        self._interior(copy).fill_(self.pattern)
        bad = (copy.view(self.int_dtype) != self.pattern).nonzero()
        if bad.numel():
            first = int(bad[0]) * self.itemsize - self.front
            last = int(bad[-1]) * self.itemsize + self.itemsize - 1 - self.front
            raise AssertionError(
                f"{self.name}: {bad.numel()} guard elements overwritten, byte offsets {first} .. "
                f"{last} relative to the interior base (interior spans "
                f"{self.interior_bytes()} bytes, row stride {self.ld * self.itemsize})")

    def interior_bytes(self):
        rows = math.prod(self.shape[:-1])
        return ((rows - 1) * self.ld + self.shape[-1]) * self.itemsize if rows else 0

    def assert_fully_written(self, expected=None):
        """G3: no interior element (of the boolean mask `expected`, default all) still holds the
        pre-fill sentinel"""
        left = self._interior(self.buf) == self.pattern
        if expected is not None:
            left = left & expected.to(left.device)
        n = int(left.sum())
        if n:
            where = left.nonzero()[0].tolist()
            raise AssertionError(f"{self.name}: {n} of {left.numel()} elements never written, "
                                 f"first at {where}")

    def assert_unwritten(self, where):
        """the interior elements of the boolean mask `where` still hold the pre-fill sentinel
        (columns or rows of the buffer that belong to somebody else)"""
        hit = (self._interior(self.buf) != self.pattern) & where.to(self.buf.device)
        n = int(hit.sum())
        if n:
            raise AssertionError(f"{self.name}: {n} interior elements outside the call's output "
                                 f"were written, first at {hit.nonzero()[0].tolist()}")

    def assert_untouched(self):
        """G6: bands intact and the whole interior still the pre-fill sentinel"""
        self.assert_bands_intact()
        assert bool((self._interior(self.buf) == self.pattern).all()), \
            f"{self.name}: a rejected call wrote into the interior"


def band_size(ld, itemsize, band_bytes=None):
    """at least one whole 256-row tile of overrun, never under 64 KiB, a multiple of 512"""
    need = max(MIN_BAND, TILE_ROWS * ld * itemsize, band_bytes or 0)
    return -(-need // 512) * 512


def banded(shape, dtype, device, *, ld=None, fill, band_bytes=None, index=None, align=16,
           name="buffer"):
    """-> Banded.  One flat allocation [front band | interior | back band]; the interior is a
    view of logical `shape` whose rows (last dimension) are `ld` elements apart, every other
    dimension dense over the rows.  fill "A" / "B" selects the sentinel; index = (a, b) fills
    bands and gaps with the valid value a (fill A) or b (fill B) instead (index-typed inputs)."""
    shape = tuple(int(d) for d in shape) or (1,)
    ld = int(ld) if ld is not None else shape[-1]
    assert ld >= shape[-1], (ld, shape)
    itemsize = torch.empty((), dtype=dtype).element_size()
    band = band_size(ld, itemsize, band_bytes)
    rows = math.prod(shape[:-1])
    interior = max(((rows - 1) * ld + shape[-1]) * itemsize, itemsize)
    total = -(-(band + 512 + interior + band + 512) // 512) * 512
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    want = 16 if align <= 16 else 0
    front = band + (want - buf.data_ptr() - band) % max(512, align)
    assert front % itemsize == 0 and front + interior + band <= total
    if index is not None:
        pattern = int(index[0] if fill == "A" else index[1])
    else:
        pattern = sentinel(dtype, fill)
    buf.view(_INT[itemsize]).fill_(pattern)
    h = Banded(buf, front, shape, ld, dtype, pattern, name)
    assert h.view.data_ptr() % max(512, align) == want
    return h


class In:
    """an input of a guarded call: `data` (logical shape) copied into a banded buffer of row
    stride ld; index = (a, b): an index-typed input whose bands hold the valid values a / b"""

    def __init__(self, data, ld=None, index=None, align=16):
        self.data, self.ld, self.index, self.align = data, ld, index, align


class Out:
    """an output, in/out tensor or workspace: pre-filled with the sentinel (or `init`); full:
    True = every element must be written (G3), False = no such promise, or a boolean mask:
    exactly its elements are written and every other one keeps its sentinel (a column range of
    somebody else's rows); compare: False leaves it out of the A/B bit comparison
    (scratch whose final contents are unspecified)"""

    def __init__(self, shape, dtype, ld=None, full=True, init=None, compare=True, finite=True,
                 align=16):
        self.shape, self.dtype, self.ld, self.full, self.init = shape, dtype, ld, full, init
        self.compare, self.finite, self.align = compare, finite, align


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def run_case(device, specs, call, *, expect_reject=False):
    """Run `call(t)` twice (t: name -> interior view; None specs pass through as None), all
    input bands in fill A, then in fill B, and assert G1 (all bands and gaps intact, inputs
    unchanged), G3 (outputs with full set hold no sentinel) and G2 (outputs bit-identical
    between the runs, floats finite).  -> {name: contiguous copy of the output} of run A, for
    the value check (G4).  expect_reject: `call` must return a nonzero status and leave every
    output untouched (G6); returns the statuses."""
    results = {}
    for fill in ("A", "B"):
        handles, views = {}, {}
        for name, s in specs.items():
            if s is None:
                views[name] = None
                continue
            if isinstance(s, In):
                h = banded(s.data.shape, s.data.dtype, device, ld=s.ld, fill=fill, index=s.index,
                           align=s.align, name=f"{name} (input, fill {fill})").set(s.data)
            else:
                h = banded(s.shape, s.dtype, device, ld=s.ld, fill=fill, align=s.align,
                           name=f"{name} (output, fill {fill})")
                if s.init is not None:
                    h.set(s.init)
            handles[name], views[name] = h, h.view
        before = {n: handles[n].ints() for n, s in specs.items() if isinstance(s, In)}
        rc = call(views)
        _sync(device)
        if expect_reject:
            assert rc not in (0, None), f"the call was accepted (status {rc})"
        for name, h in handles.items():
            s = specs[name]
            if isinstance(s, In):
                h.assert_bands_intact()
                assert torch.equal(h.ints(), before[name]), f"{h.name}: the call wrote its input"
            elif expect_reject and s.init is None:
                h.assert_untouched()
            else:
                h.assert_bands_intact()
                if expect_reject:
                    assert torch.equal(h.view, s.init.to(h.view.device).reshape(h.shape)), h.name
                elif s.full is True:
                    h.assert_fully_written()
                elif s.full is not False:
                    h.assert_fully_written(s.full)
                    h.assert_unwritten(~s.full)
        results[fill] = ({n: h.ints() for n, h in handles.items() if isinstance(specs[n], Out)},
                         {n: h.view.clone() for n, h in handles.items() if isinstance(specs[n], Out)},
                         rc)
    if expect_reject:
        return results["A"][2], results["B"][2]
    for name, a in results["A"][0].items():
        s = specs[name]
        if not s.compare:
            continue
        b = results["B"][0][name]
        if s.full is not True:
            # elements the call need not write hold the run's own pre-fill: compare the rest
            keep = (a != sentinel(s.dtype, "A")) | (b != sentinel(s.dtype, "B"))
            a, b = a[keep], b[keep]
        diff = a != b
        assert not bool(diff.any()), (f"{name}: {int(diff.sum())} output elements differ between "
                                      "input-band fills A and B: the result depends on memory "
                                      "outside the inputs")
        out = results["A"][1][name]
        if s.finite and out.is_floating_point():
            vals = out if s.full is True else out[keep]
            assert bool(torch.isfinite(vals.float()).all()), f"{name}: non-finite output"
    return results["A"][1]


def raw_call(name, *args, like):
    """the status of entry `name` (tensors and None as pointers, the current stream of `like`
    appended): for G6, where a nonzero status is the expected outcome"""
    from ov3d_amd import _native
    fn = getattr(_native.load(), name)
    conv = [_native._ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    return fn(*conv, _native._stream(like))


def call(name, *args, like):
    """the raw entry through _native.call (raises on a nonzero status)"""
    from ov3d_amd import _native
    _native.call(name, *args, like=like)
