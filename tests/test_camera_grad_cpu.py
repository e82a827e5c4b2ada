"""CPU checks of the camera-gradient entry points (include/gsraster.h: gsr_preprocess_backward_cams): declared,
exported, bound, and every argument check answers before any device work."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gsr_preprocess_backward_cams_bytes", "gsr_preprocess_backward_cams")
EINVAL, ENOSPACE = -1, -2


def _lib():
    from diff_gaussian_rasterization import _lib

    return _lib


def test_symbols_are_declared_exported_and_bound():
    _l = _lib()
    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_l.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/gsraster.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _l.SIGNATURES
    assert len(_l.SIGNATURES["gsr_preprocess_backward_cams"][1]) == 23
    assert _l.lib.gsr_abi_version() == 15 == _l.ABI_VERSION  # two new symbols, no version bump (gsr_densify_* precedent)


def test_workspace_size_is_positive_and_monotone():
    lib = _lib().lib
    sizes = (0, 1, 255, 256, 257, 3001, 10**5, 10**6, 10**7, 2**31 - 1)
    for B in (1, 2, 3, 4, 8, 64):
        prev = 0
        for P in sizes:
            n = lib.gsr_preprocess_backward_cams_bytes(P, B)
            assert n > 0 and n % 8 == 0 and n >= prev, (P, B, n)
            prev = n
    for P in sizes:
        prev = 0
        for B in (1, 2, 3, 4, 8, 64):
            n = lib.gsr_preprocess_backward_cams_bytes(P, B)
            assert n >= prev, (P, B, n)
            prev = n


def _call(lib, P, B, deg=3, M=16, ws_bytes=None, null=(), W=64, H=48, gstride=0, rest_stride=45):
    """the entry point on HOST buffers: only argument checks may look at them"""
    n = max(P, 1) * max(B, 1)
    f = lambda k: (ctypes.c_float * k)()  # noqa: E731
    need = lib.gsr_preprocess_backward_cams_bytes(P, B)
    a = dict(means3D=f(3 * max(P, 1)), sh_dc=f(3), sh_rest=f(45), cams=f(40 * max(B, 1)),
             radii=(ctypes.c_int32 * n)(), cov3D=f(6), clamped=(ctypes.c_uint8 * (3 * n))(), g2=f(4), gco=f(4), grgb=f(4),
             ws=(ctypes.c_double * (need // 8 + 1))(), out=f(40 * max(B, 1)))
    p = {k: (None if k in null else ctypes.cast(v, ctypes.c_void_p)) for k, v in a.items()}
    return lib.gsr_preprocess_backward_cams(
        P, B, deg, M, p["means3D"], p["sh_dc"], 3, p["sh_rest"], rest_stride, p["cams"], W, H, p["radii"], p["cov3D"],
        p["clamped"], p["g2"], p["gco"], p["grgb"], gstride, p["ws"], need if ws_bytes is None else ws_bytes, p["out"],
        None)


def test_arguments_are_validated_before_any_device_work():
    lib = _lib().lib
    none = [None] * 23
    args = list(none)
    args[0:4] = [-1, 1, 3, 16]
    args[6], args[8], args[10], args[11], args[18], args[20] = 3, 45, 64, 48, 0, 0
    assert lib.gsr_preprocess_backward_cams(*args) == EINVAL  # negative size, all pointers NULL
    assert _call(lib, -1, 1) == EINVAL
    assert _call(lib, 10, 0) == EINVAL  # B < 1
    assert _call(lib, 10, -3) == EINVAL
    assert _call(lib, 10, 1, deg=4) == EINVAL
    assert _call(lib, 10, 1, deg=-1) == EINVAL
    assert _call(lib, 10, 1, deg=3, M=9) == EINVAL  # fewer coefficients than the degree reads
    assert _call(lib, 10, 1, W=0) == EINVAL
    assert _call(lib, 10, 1, rest_stride=0) == EINVAL  # a row of coefficients above DC holds 45 floats at degree 3
    assert _call(lib, 10, 1, deg=2, rest_stride=23) == EINVAL  # ... and 24 at degree 2
    assert _call(lib, 10, 1, deg=2, rest_stride=24, ws_bytes=0) == ENOSPACE
    assert _call(lib, 10, 1, gstride=5) == EINVAL  # a record row holds 9 floats
    for k in ("means3D", "sh_dc", "sh_rest", "cams", "radii", "cov3D", "clamped", "g2", "gco", "grgb", "ws", "out"):
        assert _call(lib, 10, 2, null=(k,)) == EINVAL, k
    need = lib.gsr_preprocess_backward_cams_bytes(3001, 3)
    assert _call(lib, 3001, 3, ws_bytes=need - 1) == ENOSPACE  # one byte short
    assert _call(lib, 3001, 3, ws_bytes=0) == ENOSPACE
    assert _call(lib, 10, 1, deg=0, M=1, null=("sh_rest",), ws_bytes=0) == ENOSPACE  # NULL rest is legal with M == 1
