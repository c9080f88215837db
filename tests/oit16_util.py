"""Shared helpers of the tests of layered order-independent transparency in the native-storage build (test infrastructure): the cases of tests/oit_util.py with
the inputs an RGBA16_FLOAT plane can hold, the fixture tests/golden/oit16_golden.npz (written by tests/golden/make_golden_oit16.py from the reference's shader
text), and the emulated expectation -- the product's fp32 header on the host (tests/host_kernels/oit16_host.cpp) with the four targets rounded to binary16 where
the native-storage build stores them: after the attenuation and after every colour draw.

Bars (the same on the host and on the device): the K layer words and the tail's count exactly; the tail's transmittance by the project's contract
(util.assert_close at its defaults, no outlier); the four targets by the rule of h4_checks.assert_within_tol_after_the_store with the contract's allowance as the
tolerance before the store -- two values within it before the last store are at most that plus one binary16 spacing apart after it."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np

import oit_util as O
from util import ATOL, RTOL, assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
PLANES4 = ("base", "material", "radiance", "ibl")  # the slice planes that are 4-channel texels of the build; depth, alpha and the opaque depth stay fp32


def q16(a):
    """What a store to an RGBA16_FLOAT plane followed by a load does: round to nearest-even binary16, overflow -> infinity"""
    with np.errstate(over="ignore"):
        return np.asarray(a, F).astype(np.float16).astype(F)


def make_case16(c):
    """oit_util.make_case(c) with every 4-channel plane and the four targets rounded to binary16: what the native-storage build is given"""
    d = O.make_case(c)
    for k in PLANES4 + ("targets",):
        d[k] = q16(d[k])
    return d


@functools.lru_cache(maxsize=1)
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "oit16_golden.npz")))


def case_ids():
    return [(i, c["name"]) for i, c in enumerate(O.cases())]


@functools.lru_cache(maxsize=1)
def host_lib():
    """tests/host_kernels/oit16_host.cpp as a shared object (None without hipcc)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(HERE, "host_kernels", "oit16_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "oit16_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n) for n in ("mifx_oit.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"),
               "-I", os.path.join(ROOT, "include"), "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return ctypes.CDLL(out)


def emulate(lib, c, d):
    """(layers (H, W, K) uint32, tail (H, W, 2), targets (4, H, W, 4) binary16 values as float32) of the sequence on the host for the inputs `d` (make_case16), the
    targets rounded after the attenuation and after every colour draw"""
    w, h, k, n = c["w"], c["h"], c["k"], c["l"]
    cam = O.camera_struct(d["camera"])
    fp = lambda a: None if a is None else O.fptr(a)  # noqa: E731
    up = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))  # noqa: E731
    keep = {key: (np.ascontiguousarray(d[key], F) if d[key] is not None else None) for key in ("depth", "base", "material", "radiance", "ibl", "alpha", "opaque")}
    layers, tail = np.full((h, w, k), 0xDEADBEEF, np.uint32), np.full((h, w, 2), -7.0, F)
    assert lib.mifx_host_oit16_layers(k, w, h, n, fp(keep["depth"]), fp(keep["base"]), fp(keep["opaque"]), ctypes.byref(cam), up(layers), fp(tail)) == 0
    targets = np.ascontiguousarray(d["targets"], F).copy()
    assert lib.mifx_host_oit16_attenuate(k, w, h, ctypes.byref(cam), up(layers), fp(tail), fp(targets)) == 0
    targets = np.ascontiguousarray(q16(targets))
    for i in range(n):
        alpha = None if keep["alpha"] is None else np.ascontiguousarray(keep["alpha"][i])
        assert lib.mifx_host_oit16_blend(k, w, h, *[fp(np.ascontiguousarray(keep[key][i])) for key in ("depth", "base", "material", "radiance", "ibl")], fp(alpha), fp(keep["opaque"]),
                                         ctypes.byref(cam), up(layers), fp(tail), fp(targets)) == 0
        targets = np.ascontiguousarray(q16(targets))
    return layers, tail, targets


def check_against(got, want, what):
    """(layers, tail, targets) against (layers, tail, targets) at the module's bars.  `got` targets: the values of RGBA16_FLOAT planes, as float32."""
    from h4_checks import assert_within_tol_after_the_store

    (gl, gt, gg), (wl, wt, wg) = got, want
    wg = np.asarray(wg, F)
    print(f"{what}: {int((gl != wl).sum())} layer words differ, tail transmittance max |diff| {np.abs(gt[..., 1] - wt[..., 1]).max():.3e}, "
          f"targets max |diff| {np.abs(gg - wg).max():.3e}, {int((gg.astype(np.float16).view(np.uint16) != wg.astype(np.float16).view(np.uint16)).sum())} of {wg.size} codes differ")
    assert np.array_equal(gl, wl) and np.array_equal(gt[..., 0], wt[..., 0]), what
    assert_close(gt[..., 1], wt[..., 1], what=f"{what}: tail transmittance")
    tol = RTOL * np.maximum(np.abs(wg), ATOL / RTOL)  # the contract's allowance before the store
    assert_within_tol_after_the_store(gg, wg, tol, f"{what}: targets")
