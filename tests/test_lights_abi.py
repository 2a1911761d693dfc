"""The C ABI of the bounded lights (include/soc_rt.h): symbols, the host struct's size, the upload's validation (before any
HIP call: these tests run without a GPU) and a bounded call without bounds."""
import ctypes as C

import numpy as np
import pytest

from soc_real_time_renderer_amd import _abi

SYMBOLS = ("soc_upload_light_bounds", "soc_composition_bounded", "soc_composition_luminance_histogram_bounded",
           "soc_renderer_set_light_bounds")


def test_symbols_exported(soc):
    for name in SYMBOLS:
        assert hasattr(soc.lib(), name), name
        assert name in _abi.FUNCTIONS


def test_abi_unchanged_and_sizes(soc):
    lib = soc.lib()
    assert lib.soc_abi_version() == 1
    assert lib.soc_abi_sizeof(b"soc_light_bounds") == 1024 == C.sizeof(_abi.LightBounds)
    assert _abi.LIGHT_BOUNDS_DEVICE_BYTES == 2048 and _abi.LIGHTS_CULL == 1


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("kind,index", [("point", 0), ("point", 127), ("spot", 5)])
def test_upload_refuses_bad_ranges(soc, bad, kind, index):
    b = soc.light_bounds([1.0] * 128, [2.0] * 128)
    (b.point_range if kind == "point" else b.spot_range)[index] = bad
    # validation comes first: the device pointer is never touched (a host buffer stands in for it)
    fake = np.zeros(_abi.LIGHT_BOUNDS_DEVICE_BYTES, np.uint8)
    rc = soc.lib().soc_upload_light_bounds(C.byref(b), fake.ctypes.data, None)
    assert rc == -1
    msg = soc.lib().soc_last_error_string().decode()
    assert f"{kind}_range[{index}]" in msg, msg
    assert not fake.any()


def test_upload_names_the_first_bad_index(soc):
    b = soc.light_bounds([0.0, 3.0, -2.0, float("nan")], [float("inf")])
    fake = np.zeros(_abi.LIGHT_BOUNDS_DEVICE_BYTES, np.uint8)
    assert soc.lib().soc_upload_light_bounds(C.byref(b), fake.ctypes.data, None) == -1
    assert "point_range[2]" in soc.lib().soc_last_error_string().decode()
    assert soc.lib().soc_upload_light_bounds(None, fake.ctypes.data, None) == -1
    assert soc.lib().soc_upload_light_bounds(C.byref(b), None, None) == -1


def test_light_bounds_helper(soc):
    b = soc.light_bounds([1.5, 0.0], [4.0])
    assert list(b.point_range[:3]) == [1.5, 0.0, 0.0] and b.spot_range[0] == 4.0 and b.spot_range[1] == 0.0
    with pytest.raises(ValueError):
        soc.light_bounds([1.0] * 129)


def _host_images(W, H):
    f16 = np.zeros((H, W, 4), np.float16)
    return dict(target=f16.copy(), albedo=f16.copy(), emissive=f16.copy(), normal=f16.copy(),
                depth=np.ones((H, W), np.float32), ssao=np.zeros((H // 2, W // 2), np.uint8),
                shadow=np.ones((16, 16), np.float32), clouds=np.zeros((H, W, 4), np.uint8))


def test_bounded_call_without_bounds_is_refused(soc):
    """NULL d_bounds: an error code and nothing launched (the images are host arrays no kernel could have read)."""
    W, H = 32, 16
    g = soc.globals_defaults(W, H)
    im = _host_images(W, H)
    args = [soc.img(im[k]) for k in ("target", "albedo", "emissive", "normal", "depth", "ssao", "shadow", "clouds")]
    lib = soc.lib()
    rc = lib.soc_composition_bounded(C.byref(g), None, *args, None, 1, None, None)
    assert rc == -1 and "bounds" in lib.soc_last_error_string().decode()
    ae = np.zeros(257, np.int32)
    scratch = np.zeros(_abi.HISTOGRAM_SCRATCH_WORDS, np.int32)
    rc = lib.soc_composition_luminance_histogram_bounded(C.byref(g), None, *args, ae.ctypes.data, scratch.ctypes.data,
                                                         None, 1, None, None)
    assert rc == -1 and "bounds" in lib.soc_last_error_string().decode()
    assert not im["target"].any() and not ae.any()
    # unknown flag bits are refused as well
    fake = np.zeros(_abi.LIGHT_BOUNDS_DEVICE_BYTES, np.uint8)
    assert lib.soc_composition_bounded(C.byref(g), None, *args, fake.ctypes.data, 2, None, None) == -1
    assert lib.soc_renderer_set_light_bounds(None, None, 0) == -1
