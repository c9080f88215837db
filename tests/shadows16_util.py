"""Shared helpers of the tests of the 16-bit filterable shadow maps (test infrastructure): the fixture tests/golden/shadows16_golden.npz (written by
tests/golden/make_golden_shadows16.py from the reference's shader text), the host compilation of the product's header with the format as an argument
(tests/host_kernels/shadows16_host.cpp), and the bars both the CPU and the GPU tests hold the results to.

Bars.
  conversion  the stored outputs are CODES of the reference's strict build.  The result is widened and compared in util.assert_close's default measure plus one step
              of the format at the expected value (abs_slack; no outliers): a value that the fp32 arithmetic before the store leaves within the contract of the
              reference's can land on the other side of a rounding boundary of the 16-bit format, never further -- the same allowance the generator asserts between
              the reference's own two builds.
  look-up     the fixture's stored budget per case (0 = the project's contract, util.assert_close defaults, no outlier); the cascade index exact."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

import shadows_util as S
from util import assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
FMT_U16X2, FMT_F16X2, FMT_F16X4 = 512, 64, 8
FMT_OF_MODE = {S.MODE_VSM: FMT_U16X2, S.MODE_EVSM2: FMT_F16X2, S.MODE_EVSM4: FMT_F16X4}


@functools.lru_cache(maxsize=1)
def golden():
    g = dict(np.load(os.path.join(HERE, "golden", "shadows16_golden.npz")))
    g["map_depth"] = np.load(os.path.join(HERE, "golden", "shadows_golden.npz"))["map_depth"][:3]  # (the generator asserts that these are the slices it converted)
    g["map_evsm2"] = np.ascontiguousarray(g["map_evsm4"][..., :2])                                    # (... and that RG16_FLOAT is the first half of RGBA16_FLOAT)
    return g


def conv_cases():
    return [(i, str(n)) for i, n in enumerate(golden()["conv_names"])]


def look_cases():
    return [(i, str(n)) for i, n in enumerate(golden()["look_names"])]


def conv_inputs(g, i):
    """(attribs, mode, fmt, depth slices, expected codes, radii) of conversion case i"""
    q = f"v{i}_"
    want = g[q + "out"]
    n, h, w = want.shape[:3]
    return S.attribs_from_bytes(g[q + "attribs"]), int(g[q + "mode"]), int(g[q + "fmt"]), g[f"depth_{w}x{h}x{n}"], want, g[q + "radii"]


def lookup_inputs(g, i):
    """(camera floats, attribs, frame depth, the map's codes, fmt, mode, across, best) of look-up case i"""
    q = f"l{i}_"
    W, H = (int(v) for v in g[q + "frame_size"])
    mode, across, best = (int(v) for v in g[q + "params"])
    arr = {S.MODE_VSM: g["map_vsm"], S.MODE_EVSM2: g["map_evsm2"], S.MODE_EVSM4: g["map_evsm4"]}[mode]
    return g[f"camera_{W}x{H}"], S.attribs_from_bytes(g[q + "attribs"]), g[f"frame_{W}x{H}"], np.ascontiguousarray(arr), FMT_OF_MODE[mode], mode, across, best


def code_dtype(fmt):
    return np.uint16 if fmt == FMT_U16X2 else np.float16


def widen(codes, fmt):
    """float32 values of codes: code / 65535 correctly rounded, or the binary16 value"""
    codes = np.asarray(codes)
    if fmt == FMT_U16X2:
        return (codes.view(np.uint16).astype(np.float64) / 65535.0).astype(F)
    return codes.view(np.float16).astype(F)


def step_of(values, fmt):
    """One step of the format at each value: 1 / 65535, or the spacing of binary16 there"""
    if fmt == FMT_U16X2:
        return np.full(np.shape(values), 1.0 / 65535.0)
    return np.abs(np.spacing(np.asarray(values, np.float16))).astype(np.float64)


def check_codes(got_codes, want_codes, fmt, what):
    """The conversion bar (module docstring).  Prints the figures before it asserts."""
    got, want = widen(got_codes, fmt), widen(want_codes, fmt)
    differ = np.ascontiguousarray(got_codes).view(np.uint16) != np.ascontiguousarray(want_codes).view(np.uint16)
    steps = np.abs(got.astype(np.float64) - want) / step_of(want, fmt)
    print(f"{what}: {int(differ.sum())} of {differ.size} codes differ, by at most {float(steps.max()):.2f} steps of the format")
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert_close(got, want, abs_slack=step_of(want, fmt), what=what)


def check_light(got, want, tol, what):
    """The look-up bar: the stored budget (0 = the project's contract)"""
    print(f"{what}: max |diff| {np.abs(got - want).max():.3e}, pixels beyond 1e-3: {int((np.abs(got - want) > 1e-3).sum())} of {want.size}, stored budget {tol:g}")
    if tol > 0.0:
        assert np.abs(got.astype(np.float64) - want).max() <= tol, what
    else:
        assert_close(got, want, what=what)


def same_codes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint16), np.ascontiguousarray(b).view(np.uint16))


# ------------------------------------------------------------------------------------------------ the header on the host
@functools.lru_cache(maxsize=1)
def host_lib():
    """tests/host_kernels/shadows16_host.cpp as a shared object (None without hipcc)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(HERE, "host_kernels", "shadows16_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "shadows16_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n) for n in ("mifx_shadows.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"),
               "-I", os.path.join(ROOT, "include"), "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return ctypes.CDLL(out)


def host_convert(lib, depth, A, mode, fmt, tiled=False):
    """The two passes (or the fused kernel's tile stages) on the host; returns (status, codes or float32 values for fmt 0)"""
    n, h, w = depth.shape
    out = np.full((n, h, w, 4 if mode == S.MODE_EVSM4 else 2), 0x7BFF if fmt else -7.0, np.uint16 if fmt else F)
    rc = lib.mifx_host_shadow16_convert(S.fptr(np.ascontiguousarray(depth, F)), w, h, n, ctypes.byref(A), ctypes.c_uint32(mode), ctypes.c_uint32(fmt), out.ctypes.data_as(ctypes.c_void_p),
                                        int(tiled))
    return rc, (out.view(code_dtype(fmt)) if fmt else out)


def host_filter(lib, cam, A, frame, codes, fmt, mode, across, best):
    H, W = frame.shape
    light, casc = np.zeros((H, W), F), np.zeros((H, W, 2), F)
    cam_s = S.camera_struct(cam)
    codes = np.ascontiguousarray(codes)
    assert lib.mifx_host_shadow16_filter(S.fptr(np.ascontiguousarray(frame, F)), W, H, ctypes.byref(cam_s), ctypes.byref(A), ctypes.c_uint32(mode), across, best,
                                         codes.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(fmt), codes.shape[2], codes.shape[1], codes.shape[0], S.fptr(light), S.fptr(casc)) == 0
    return light, casc
