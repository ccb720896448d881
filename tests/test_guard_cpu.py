"""tests/guard.py on CPU tensors with fake kernels written in Python: a well-behaved kernel
passes, and each of the six failure kinds (a write before the interior, after it, into a gap
column, a leftover sentinel, an A/B difference, a non-finite result) is flagged; and the closed
set: every entry of include/ov3d.h that can write device memory is either guarded by a case of
tests/test_guard_*_gpu.py or named, with a reason, in guard_cases.NOT_GUARDED."""
import re

import pytest
import torch

import guard
from guard import In, Out
from helpers import ov3d  # noqa: F401

CPU = torch.device("cpu")
R, C, LD = 5, 6, 14


def _specs():
    x = torch.arange(R * C, dtype=torch.float32).reshape(R, C) / 7
    return {"x": In(x.to(torch.bfloat16), ld=LD), "idx": In(torch.arange(R, dtype=torch.int32),
                                                             index=(0, R - 1)),
            "y": Out((R, C), torch.float32, ld=LD), "n": Out((R,), torch.int32)}


def _good(t):
    t["y"].copy_(t["x"].float()[t["idx"].long()] * 2)
    t["n"].copy_(t["idx"] + 1)


def _flat(view):
    """the whole allocation behind an interior view, and the interior's element offset in it"""
    whole = torch.empty(0, dtype=view.dtype).set_(view.untyped_storage())
    return whole, view.storage_offset()


def test_layout_alignment_and_band_size():
    for dtype, ld in ((torch.bfloat16, 1032), (torch.float32, 8), (torch.uint8, 3), (torch.float64, 5)):
        h = guard.banded((3, 2), dtype, CPU, ld=ld, fill="A")
        item = h.itemsize
        assert h.view.data_ptr() % 512 == 16                  # 16-byte aligned and no more
        assert h.view.shape == (3, 2) and h.view.stride() == (ld, 1)
        band = max(64 * 1024, 256 * ld * item)
        assert h.front >= band and h.buf.numel() - h.front - h.interior_bytes() >= band
        h.assert_bands_intact()
        with pytest.raises(AssertionError, match="never written"):
            h.assert_fully_written()
    h = guard.banded((4,), torch.float32, CPU, fill="A", align=256)
    assert h.view.data_ptr() % 512 == 0
    # sentinels are bit patterns: fp32 / bf16 quiet NaNs (A), largest finite (B), 0x5A bytes
    assert guard.sentinel(torch.float32, "B") == 0x7F7FFFFF and guard.sentinel(torch.bfloat16, "B") == 0x7F7F
    a = guard.banded((2,), torch.float32, CPU, fill="A").view
    b = guard.banded((2,), torch.bfloat16, CPU, fill="B").view
    assert bool(torch.isnan(a).all()) and bool((b == torch.finfo(torch.bfloat16).max).all())
    assert guard.sentinel(torch.int32, "A") == 0x5A5A5A5A and guard.sentinel(torch.uint8, "A") == 0x5A
    # index inputs: valid values, different per fill
    for fill, v in (("A", 0), ("B", 9)):
        h = guard.banded((3,), torch.int32, CPU, fill=fill, index=(0, 9))
        whole, off = _flat(h.view)
        assert int(whole[off - 1]) == v and int(whole[off + 3]) == v


def test_three_dimensional_view_rows_are_ld_apart():
    h = guard.banded((2, 3, 4), torch.float32, CPU, ld=12, fill="B")
    assert h.view.stride() == (36, 12, 1)
    h.view.fill_(1.0)
    h.assert_bands_intact()
    h.assert_fully_written()


def test_well_behaved_kernel_passes():
    out = guard.run_case(CPU, _specs(), _good)
    x = _specs()["x"].data.float()
    assert torch.equal(out["y"], x * 2) and out["y"].is_contiguous()
    assert torch.equal(out["n"], torch.arange(1, R + 1, dtype=torch.int32))


def test_write_one_element_before_the_interior_is_flagged():
    def bad(t):
        _good(t)
        whole, off = _flat(t["y"])
        whole[off - 1] = 1.0
    with pytest.raises(AssertionError, match=r"y \(output.*byte offsets -4 \.\. -1 "):
        guard.run_case(CPU, _specs(), bad)


def test_write_one_element_after_the_interior_is_flagged():
    def bad(t):
        _good(t)
        whole, off = _flat(t["y"])
        whole[off + (R - 1) * LD + C] = 1.0
    end = ((R - 1) * LD + C) * 4
    with pytest.raises(AssertionError, match=rf"byte offsets {end} \.\. {end + 3} "):
        guard.run_case(CPU, _specs(), bad)


def test_write_into_a_gap_column_is_flagged():
    def bad(t):
        _good(t)
        whole, off = _flat(t["y"])
        whole[off + 2 * LD + C] = 0.0        # row 2, first column past the logical width
    at = (2 * LD + C) * 4
    with pytest.raises(AssertionError, match=rf"byte offsets {at} \.\. {at + 3} "):
        guard.run_case(CPU, _specs(), bad)


def test_write_into_an_input_is_flagged():
    def bad(t):
        _good(t)
        t["x"][0, 0] = 3.0
    with pytest.raises(AssertionError, match="wrote its input"):
        guard.run_case(CPU, _specs(), bad)


def test_leftover_sentinel_is_flagged():
    def bad(t):
        _good(t)
        whole, off = _flat(t["y"])
        whole.view(torch.int32)[off + 3 * LD + 1] = guard.sentinel(torch.float32, "A")
    with pytest.raises(AssertionError, match=r"never written, first at \[3, 1\]"):
        guard.run_case(CPU, _specs(), bad)


def test_dependence_on_memory_outside_the_inputs_is_flagged():
    def over_read(t):                        # a row tile that also sums the first gap column
        _good(t)
        whole, off = _flat(t["x"])
        t["y"][0, 0] += 0.0 * whole[off + C].float()        # 0 x NaN under A, 0 x finite under B
    with pytest.raises(AssertionError, match="differ between input-band fills"):
        guard.run_case(CPU, _specs(), over_read)

    def over_read_index(t):                  # reads idx[R] and dereferences it: 0 under A, R-1 under B
        _good(t)
        whole, off = _flat(t["idx"])
        t["n"][0] = whole[off + R] + 100
    with pytest.raises(AssertionError, match="n: 1 output elements differ"):
        guard.run_case(CPU, _specs(), over_read_index)


def test_non_finite_output_is_flagged():
    def bad(t):
        _good(t)
        t["y"][1, 1] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        guard.run_case(CPU, _specs(), bad)


def test_partially_written_outputs_and_rejections():
    specs = _specs()
    mask = torch.ones(R, C, dtype=torch.bool)
    mask[:, C - 1] = False                   # documented: the last column is left alone
    specs["y"] = Out((R, C), torch.float32, ld=LD, full=mask)

    def partial(t):
        t["y"][:, :C - 1] = t["x"].float()[:, :C - 1]
        t["n"].zero_()
    guard.run_case(CPU, specs, partial)
    with pytest.raises(AssertionError, match="never written"):
        guard.run_case(CPU, specs, lambda t: t["n"].zero_())

    def trespass(t):                         # also writes the column that belongs to somebody else
        partial(t)
        t["y"][2, C - 1] = 1.0
    with pytest.raises(AssertionError, match=rf"outside the call's output were written, first at \[2, {C - 1}\]"):
        guard.run_case(CPU, specs, trespass)
    # G6: a rejected call returns a status and writes nothing
    assert guard.run_case(CPU, _specs(), lambda t: -1, expect_reject=True) == (-1, -1)
    with pytest.raises(AssertionError, match="wrote into the interior"):
        guard.run_case(CPU, _specs(), lambda t: (t["n"].zero_(), -1)[1], expect_reject=True)
    with pytest.raises(AssertionError, match="accepted"):
        guard.run_case(CPU, _specs(), lambda t: 0, expect_reject=True)


def _writers():
    """entries of the headers with a pointer parameter that is not const-qualified (or a
    pointer to a struct that carries such pointers): the ones that can write device memory"""
    from ov3d_amd import _native
    text = "\n".join(open(p).read() for p in _native.HEADER_PATHS)
    protos = _native.EXPORTS
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    structs = dict((name, body) for body, name in
                   re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S))

    def writes(decl):
        decl = " ".join(decl.split())
        if "*" not in decl:
            return False
        if not decl.startswith("const "):
            return True
        base = decl.split()[1].rstrip("*")
        return base in structs and any(writes(f) for f in structs[base].split(";"))
    out = set()
    for name in protos:
        params = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        if any(writes(p) for p in params.split(",")):
            out.add(name)
    return out


def test_every_writing_entry_is_guarded_or_listed():
    """a kernel added later cannot skip this suite silently"""
    import guard_cases
    writers = _writers()
    assert {"ov3d_fps", "ov3d_gemm256", "ov3d_wgrad_group", "ov3d_lngemm_fwd", "ov3d_multi_copy",
            "ov3d_sun_labels", "ov3d_attn_bwd_dkdv_batch"} <= writers
    assert {"ov3d_vocab_score", "ov3d_openvocab_classify", "ov3d_lift_nms", "ov3d_backproj_compose"} <= writers
    assert "ov3d_fps_workspace" not in writers and "ov3d_version" not in writers
    guarded = guard_cases.guarded()
    listed = set(guard_cases.NOT_GUARDED)
    assert not guarded & listed, sorted(guarded & listed)
    assert writers - guarded - listed == set(), sorted(writers - guarded - listed)
    assert (guarded | listed) - writers == set(), sorted((guarded | listed) - writers)
    for name, reason in guard_cases.NOT_GUARDED.items():
        assert isinstance(reason, str) and len(reason) > 10 and "\n" not in reason, name


def test_guarded_table_names_entries_the_case_files_call():
    """the table is read from the case files: each names the entries its cases run, and every
    such name appears in a call in that file's text"""
    import guard_cases
    for module, names in guard_cases.CASE_FILES.items():
        text = open(guard_cases.path(module)).read()
        assert names, module
        for name in names:                   # once in ENTRIES, and in at least one call
            assert text.count(f'"{name}"') >= 2, (module, name)
