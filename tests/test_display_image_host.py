"""CPU: bhray_diag_display_image, the display pass over a supplied image - what of it needs no device.  The symbol is a
verification entry point (include/bhray_diag.h only), every refusal is a code and comes before the device is touched, and a valid call on
a device the machine does not have is the library's no-device error.  The kernels' side is tests/test_gpu_display_image.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import bhusie_amd as B
from bhusie_amd import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NO_DEVICE = -1, -2
NAME = "bhray_diag_display_image"


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _call(img, w, h, dst, fxaa=None, mix=None, flags=0, stages=None, texels=0, device=0):
    return B.lib().bhray_diag_display_image(device, img.ctypes.data if img is not None else None, w, h, fxaa, mix, flags,
                                            dst.ctypes.data if dst is not None else None, stages.ctypes.data if stages is not None else None, texels)


def _scratch_texels(w, h):
    return sum(lw * lh for lw, lh in B.bloom_sizes(w, h)[:9]) + w * h


def test_the_symbol_is_declared_in_the_diagnostic_header_only_and_bound():
    product, diag = _header("bhray.h"), _header("bhray_diag.h")
    assert NAME not in product and "BHRAY_DIAG_DISPLAY_FXAA_ONLY" not in product
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, diag, flags=re.S)
    assert m and m.group(1).count(",") + 1 == 10 == len(layouts.DIAG_SYMBOLS[NAME][1])
    assert NAME not in layouts.SYMBOLS
    flag = re.search(r"#define\s+BHRAY_DIAG_DISPLAY_FXAA_ONLY\s+(\d+)u?\b", diag)
    assert flag and int(flag.group(1)) == layouts.DIAG_DISPLAY_FXAA_ONLY == 1
    assert hasattr(B.lib(), NAME)
    p = inspect.signature(B.display_image).parameters
    assert list(p) == ["sky16", "fxaa", "mix", "device", "fxaa_only", "stages"]
    assert [p[k].default for k in list(p)[1:]] == [None, None, 0, False, False]


def test_refusals_are_codes_and_come_before_the_device():
    img, dst = np.zeros((32, 32, 4), np.uint16), np.zeros((32, 32, 4), np.uint8)
    n = _scratch_texels(32, 32)
    assert n == 16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1 + 2 * 2 + 4 * 4 + 8 * 8 + 16 * 16 + 32 * 32
    stages = np.zeros((n + 1, 4), np.uint16)
    fx = lambda it: bytes(layouts.BhrayFxaaDetails(0.0156, 0.063, it, 0.75))    # noqa: E731
    refused = {
        "NULL image": dict(img=None, w=32, h=32, dst=dst),
        "NULL destination": dict(img=img, w=32, h=32, dst=None),
        "31 x 32": dict(img=img, w=31, h=32, dst=dst),
        "32 x 31": dict(img=img, w=32, h=31, dst=dst),
        "0 x 0": dict(img=img, w=0, h=0, dst=dst),
        "31 x 32, fxaa only": dict(img=img, w=31, h=32, dst=dst, flags=1),
        "32 x 31, fxaa only": dict(img=img, w=32, h=31, dst=dst, flags=1),
        "wider than any frame": dict(img=img, w=32768, h=32, dst=dst),
        "iterations above the bound": dict(img=img, w=32, h=32, dst=dst, fxaa=fx(layouts.FXAA_MAX_ITERATIONS + 1)),
        "iterations above the bound, fxaa only": dict(img=img, w=32, h=32, dst=dst, fxaa=fx(layouts.FXAA_MAX_ITERATIONS + 1), flags=1),
        "flag bit 1": dict(img=img, w=32, h=32, dst=dst, flags=2),
        "flag bit 31": dict(img=img, w=32, h=32, dst=dst, flags=0x80000001),
        "stage buffer one texel short": dict(img=img, w=32, h=32, dst=dst, stages=stages, texels=n - 1),
        "stage buffer one texel long": dict(img=img, w=32, h=32, dst=dst, stages=stages, texels=n + 1),
        "stage buffer of no texels": dict(img=img, w=32, h=32, dst=dst, stages=stages, texels=0),
        "stage buffer beside the flag": dict(img=img, w=32, h=32, dst=dst, stages=stages, texels=n, flags=1),
    }
    L = B.lib()
    for what, kw in refused.items():
        # a device index no machine has: a refusal that reached the device check would come back as BHRAY_E_NO_DEVICE
        assert _call(device=1 << 20, **kw) == E_INVALID, what
        assert L.bhray_last_error(None), what
    assert (dst == 0).all() and (stages == 0).all()


def test_a_valid_call_on_a_device_that_is_not_there_is_the_no_device_error():
    """On a machine without a GPU that is device 0; with GPUs, the first index past them (nothing is launched here either way)."""
    img, dst = np.zeros((32, 32, 4), np.uint16), np.full((32, 32, 4), 7, np.uint8)
    absent = B.lib().bhray_device_count()
    n = _scratch_texels(32, 32)
    for kw in (dict(), dict(flags=1), dict(stages=np.zeros((n, 4), np.uint16), texels=n), dict(fxaa=bytes(B.post_defaults()[0]), mix=bytes(B.post_defaults()[1]))):
        assert _call(img, 32, 32, dst, device=absent, **kw) == E_NO_DEVICE
    assert _call(img, 32, 32, dst, device=-1) == E_NO_DEVICE
    msg = B.lib().bhray_last_error(None)
    assert b"device" in msg
    try:
        B.display_image(img.view(np.float16), device=absent)
    except B.BhrayError as e:
        assert e.code == E_NO_DEVICE
    else:
        raise AssertionError("display_image returned an image without a device")
    assert (dst == 7).all()
