"""The selection outline without a GPU: known answers of the float32 restatement (tests/selection_util.py) of the reference's jump flood and composite tail, and the
product's per-pixel bodies (diligentfx_amd/csrc/mifx_selection.h) compiled for the host against that restatement, bit for bit."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import selection_util as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def seeds_plane(w, h, points, depth=0.5, clear=1.0):
    sel = np.full((h, w), F(clear), F)
    for x, y in points:
        sel[y, x] = F(depth)
    return sel


def test_iteration_counts_follow_the_reference():
    # HnProcessSelectionTask.cpp:71: ceil(log2(max(d, 1))) + 1
    assert [S.iterations(d) for d in (0.0, 1.0, 2.0, 3.0, 4.0, 16.0, 100.0)] == [1, 1, 2, 3, 3, 5, 8]


def test_one_seed_is_found_within_chebyshev_seven_at_the_defaults():
    w = h = 48
    sx, sy = 20, 23
    out = S.jump_flood(seeds_plane(w, h, [(sx, sy)]), 1.0, 4.0)
    want = S.init(seeds_plane(w, h, [(sx, sy)]), 1.0)[sy, sx]
    yy, xx = np.mgrid[0:h, 0:w]
    near = np.maximum(abs(xx - sx), abs(yy - sy)) <= 7
    assert np.all(out[near] == want)
    assert np.all(out[~near] == 0)


def test_truncation_at_column_and_row_zero():
    # Pos - SampleRange = -0.5 truncates to 0: at range 2 the pixel in column 1 reads column 0 with its offset -1 tap, at range 1 column 0 reads itself
    w = h = 16
    p = S.init(seeds_plane(w, h, [(0, 8)]), 1.0)
    s = S.step(p, 2)
    assert s[8, 1, 1] > 0.25 and s[8, 1, 0] == p[8, 0, 0]  # (taps at columns -1 -> 0, 1, 3)
    assert s[8, 3, 1] == 0  # (taps at columns 1, 3, 5)
    s = S.step(S.init(seeds_plane(w, h, [(8, 0)]), 1.0), 2)
    assert s[1, 8, 1] > 0.25 and s[3, 8, 1] == 0
    # range 4: x + 0.5 - 4 = -0.5 at x = 3, so column 3 reads column 0 as well; column 2 (-1.5 -> -1) is outside
    s = S.step(S.init(seeds_plane(w, h, [(0, 8)]), 1.0), 4)
    assert s[8, 3, 1] > 0.25 and s[8, 2, 1] == 0


def test_ties_go_to_the_first_tap_in_the_shaders_order():
    w = h = 16  # (powers of two: the distances of the two candidates are exactly equal)
    p = S.init(seeds_plane(w, h, [(4, 5), (6, 5)]), 1.0)
    s = S.step(p, 1)
    assert s[5, 5, 0] == p[5, 4, 0]  # (-1, 0) comes before (+1, 0)
    p = S.init(seeds_plane(w, h, [(5, 4), (5, 6)]), 1.0)
    s = S.step(p, 1)
    assert s[5, 5, 1] == p[4, 5, 1]  # (0, -1) comes before (0, +1)
    p = S.init(seeds_plane(w, h, [(6, 6), (4, 4)]), 1.0)
    s = S.step(p, 1)
    assert s[5, 5, 0] == p[4, 4, 0] and s[5, 5, 1] == p[4, 4, 1]  # (-1, -1) is the first tap


def test_empty_selection_is_a_cleared_plane():
    sel = seeds_plane(20, 10, [(3, 3)])
    assert not S.jump_flood(sel, 1.0, 4.0, selection_id=0).any()
    assert not S.jump_flood(np.ones((10, 20), F), 1.0, 16.0).any()


def test_reversed_depth_clear_value_zero():
    pts = [(5, 7), (30, 2), (17, 19)]
    a = S.jump_flood(seeds_plane(40, 24, pts, depth=0.3, clear=0.0), 0.0, 8.0)
    b = S.jump_flood(seeds_plane(40, 24, pts, depth=0.3, clear=1.0), 1.0, 8.0)
    assert np.array_equal(a, b) and (a[..., 1] > 0.25).any()


def test_composite_tail_known_answers():
    w, h = 16, 8
    depth = np.full((h, w), F(0.5), F)
    sel = seeds_plane(w, h, [(4, 4)], depth=0.5)
    closest = S.jump_flood(sel, 1.0, 4.0)
    rgba = np.full((h, w, 4), F(0.25), F)
    rgba[..., 0] = 1.0
    rgba[..., 3] = 0.75
    out = S.composite_tail(rgba, depth, sel, closest, (0.0, 1.0, 0.0), (1.0, 0.0, 1.0), desaturation=1.0, outline_width=2.0)
    assert np.array_equal(out[4, 4], rgba[4, 4])  # selected: neither desaturated nor outlined
    lum = F(1.0) * F(0.2126) + F(0.25) * F(0.7152) + F(0.25) * F(0.0722)
    assert np.all(out[0, 12, :3] == lum) and out[0, 12, 3] == F(0.75)  # far away: fully desaturated
    # one pixel to the right: distance 1 of 2 -> half way to the visible outline colour
    assert np.allclose(out[4, 5, :3], np.array([lum, lum, lum]) * 0.5 + np.array([0.0, 1.0, 0.0]) * 0.5)
    occluded = seeds_plane(w, h, [(4, 4)], depth=0.7)  # (the selection depth differs from the scene's: occluded)
    out = S.composite_tail(rgba, depth, occluded, S.jump_flood(occluded, 1.0, 4.0), (0.0, 1.0, 0.0), (1.0, 0.0, 1.0), outline_width=2.0)
    assert np.allclose(out[4, 5, :3], rgba[4, 5, :3] * 0.5 + np.array([1.0, 0.0, 1.0]) * 0.5)
    assert np.array_equal(out[4, 4], rgba[4, 4])  # (selection depth != clear: no outline on the prim itself)


@pytest.fixture(scope="module")
def host_lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(HERE, "host_kernels", "selection_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "selection_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n) for n in ("mifx_selection.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"), "-I",
               os.path.join(ROOT, "include"), "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return ctypes.CDLL(out)


def fptr(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


@pytest.mark.parametrize("w,h,max_distance,clear", [(31, 17, 1.0, 1.0), (31, 17, 4.0, 1.0), (64, 40, 16.0, 1.0), (57, 45, 100.0, 0.0), (40, 33, 2.0, 1.0), (23, 61, 32.0, 0.0)])
def test_product_jump_flood_on_the_host_equals_the_restatement(host_lib, w, h, max_distance, clear):
    rng = np.random.default_rng(w * 1000 + h)
    depth = rng.uniform(0.1, 0.9, (h, w)).astype(F)
    sel = S.make_selection_depth(depth, rng, clear_depth=clear, seeds=4, max_radius=3)
    sel[0, rng.integers(0, w)] = depth[0, 0]  # (seeds on the first row / column: the truncation rule)
    sel[rng.integers(0, h), 0] = depth[0, 0]
    got = np.zeros((h, w, 2), F)
    host_lib.mifx_host_jump_flood(fptr(np.ascontiguousarray(sel)), fptr(got), w, h, ctypes.c_float(clear), ctypes.c_float(max_distance))
    want = S.jump_flood(sel, clear, max_distance)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).any(-1).sum())


@pytest.mark.parametrize("desat,clear", [(0.0, 1.0), (0.6, 1.0), (1.0, 0.0)])
def test_product_composite_tail_on_the_host_equals_the_restatement(host_lib, desat, clear):
    from diligentfx_amd import binding as B

    w, h = 48, 36
    rng = np.random.default_rng(7)
    depth = rng.uniform(0.1, 0.9, (h, w)).astype(F)
    depth[:5, :7] = clear  # (background)
    sel = S.make_selection_depth(depth, rng, clear_depth=clear, seeds=5, max_radius=4)
    closest = S.jump_flood(sel, clear, 4.0)
    rgba = rng.uniform(0.0, 3.0, (h, w, 4)).astype(F)
    a = B.SelectionAttribs.default(selection_id=3, clear_depth=clear)
    a.nonselection_desaturation, a.outline_width = desat, 3.0
    got = np.zeros_like(rgba)
    host_lib.mifx_host_selection_tail(fptr(rgba), fptr(depth), fptr(sel), fptr(closest), fptr(got), w, h, ctypes.byref(a))
    want = S.composite_tail(rgba, depth, sel, closest, list(a.outline_color)[:3], list(a.occluded_outline_color)[:3], desat, clear, 3.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).any(-1).sum())
    assert not np.array_equal(got, rgba)
