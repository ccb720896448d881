"""The evaluation caps and the kernel switch, on the host: no device is touched."""
import ctypes

from helpers import ov3d  # noqa: F401


def test_caps():
    from ov3d_amd import ap_calculator, nms
    assert nms.MAX_K == 2048
    assert ap_calculator.AP_MAX_PROPOSALS == 2048 and ap_calculator.AP_MAX_GT == 1024
    assert callable(nms.nms_2d_faster) and callable(nms.large_kernels)


def test_large_kernels_switch_round_trips():
    from ov3d_amd import _native, nms
    lib = _native.load()
    assert lib.ov3d_eval_large_kernels(-1) == 0          # off by default
    try:
        assert lib.ov3d_eval_large_kernels(1) == 0       # returns the previous setting
        assert lib.ov3d_eval_large_kernels(-1) == 1
        assert nms.large_kernels() == 1                  # the Python face of the same switch
        assert lib.ov3d_eval_large_kernels(7) == 1       # any other positive value: on
        assert lib.ov3d_eval_large_kernels(0) == 1
        assert nms.large_kernels(1) == 0 and nms.large_kernels(0) == 1
    finally:
        lib.ov3d_eval_large_kernels(0)
    assert lib.ov3d_eval_large_kernels(-1) == 0


def test_entries_reject_shapes_past_the_caps():
    """ov3d_nms3d and ov3d_ap_match validate K and G before any launch (host-side checks)"""
    from ov3d_amd import _native
    lib = _native.load()
    p = ctypes.c_void_p(256)      # never dereferenced: every call below fails validation first
    assert lib.ov3d_nms3d(p, None, 1, 2049, 8, 0.25, 0, 1, p, None) == -1
    assert lib.ov3d_nms3d(p, p, 4, 2049, 7, 0.25, 1, 0, p, None) == -1
    assert lib.ov3d_ap_match(p, p, p, p, 1, 2049, 64, 20, 0.25, p, None) == -1
    assert lib.ov3d_ap_match(p, p, p, p, 1, 256, 1025, 20, 0.25, p, None) == -1
    for on in (0, 1):             # whichever kernel would have run
        prev = lib.ov3d_eval_large_kernels(on)
        try:
            assert lib.ov3d_nms3d(p, None, 1, 2049, 8, 0.25, 0, 1, p, None) == -1
            assert lib.ov3d_ap_match(p, p, p, p, 1, 2049, 1025, 20, 0.25, p, None) == -1
        finally:
            lib.ov3d_eval_large_kernels(prev)
