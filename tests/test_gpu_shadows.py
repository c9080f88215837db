"""Cascaded shadow maps on the GPU: the C ABI against the reference fixture (tests/golden/shadows_golden.npz), the fused conversion against the two-launch path, pitched and
offset planes, the Python mirror, and one larger comparison against the header compiled for the host.

Tolerances are the fixture's, which come from the reference alone (tests/golden/make_golden_shadows.py): its strict and contracted builds stay within 0.5e-3 of each other
on every stored case and no PCF pixel flips, so every case is held to the project's contract -- util.assert_close defaults, no outlier.  (A case whose budget were not zero
would get twice the reference's own difference, with a flipped PCF pixel capped at one comparison sample's weight: _check_light.)  The device's expf is not the host's libm,
so the EVSM moments and light amounts are compared in that measure, not bit for bit; the two conversion paths on the device are compared bit for bit."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

import shadows_util as S
import test_shadows_cpu as C
from util import assert_close, blue_noise_tables

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def host_lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return C.build_host_lib(hipcc)


@pytest.fixture(scope="module")
def ctx():
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    return api.PostFXContext(0, sobol, tile)


def _dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _pitched_array(n, h, w, ch, ctx):
    """(n, h, w[, ch]) float32 view with a row pitch of w + 5 texels, a slice pitch of h + 3 rows and an offset of 2 rows and 4 texels into a sentinel-filled block"""
    c = max(ch, 1)
    block = torch.full((n + 1, h + 3, w + 5, c), SENTINEL, dtype=torch.float32, device=ctx.device)
    view = block[:n, 2:2 + h, 4:4 + w, :]
    return (view if ch else view[..., 0]), block


def _untouched_outside(view_mask_block):
    block, n, h, w = view_mask_block
    m = torch.ones_like(block, dtype=torch.bool)
    m[:n, 2:2 + h, 4:4 + w, :] = False
    return bool(torch.all(block[m] == SENTINEL))


def _launches(ctx, name, fn):
    """How often the kernel-timing bracket `name` was passed while fn() ran (mifx_postfx_set_kernel_timing / _get_kernel_times)"""
    from diligentfx_amd import binding as B

    B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, name.encode(), 8))
    try:
        fn()
        times, n = (ctypes.c_float * 8)(), ctypes.c_uint32(0)
        B.check(ctx.lib.mifx_postfx_get_kernel_times(ctx.handle, times, 8, ctypes.byref(n)))
        return n.value
    finally:
        B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, None, 0))


def _convert(ctx, depth_t, A, mode, out_t):
    from diligentfx_amd import binding as B

    src, dst = B.shadow_map_array(depth_t), B.filterable_shadow_map(out_t)
    torch.cuda.synchronize()
    B.check(ctx.lib.mifx_shadow_convert_to_filterable(ctx.handle, ctypes.byref(src), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(dst)))
    torch.cuda.synchronize()
    return out_t


def _filter(ctx, frame_t, cam, A, mode, across, best, arr_t, light_t=None, casc_t=None):
    from diligentfx_amd import binding as B

    light_t = torch.empty_like(frame_t) if light_t is None else light_t
    casc_t = torch.empty(tuple(frame_t.shape) + (2,), dtype=torch.float32, device=frame_t.device) if casc_t is None else casc_t
    p = B.ShadowFilterParams(mode, across, best, 0)
    sm = B.shadow_map_array(arr_t) if mode == S.MODE_PCF else None
    fm = B.filterable_shadow_map(arr_t) if mode != S.MODE_PCF else None
    d, o, c = B.image(frame_t), B.image(light_t), B.image(casc_t)
    cam_s = S.camera_struct(cam)
    torch.cuda.synchronize()
    B.check(ctx.lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(cam_s), ctypes.byref(A), ctypes.byref(p), ctypes.byref(sm) if sm is not None else None,
                                               ctypes.byref(fm) if fm is not None else None, ctypes.byref(o), ctypes.byref(c)))
    torch.cuda.synchronize()
    return light_t, casc_t


def _check_light(got, want, g, i, what):
    """The fixture's budget for look-up case i (all zero today: the project's contract)"""
    tol, flip, cap = float(g[f"l{i}_tol"]), float(g[f"l{i}_flip_budget"]), float(g[f"l{i}_cap"])
    print(f"{what}: max |diff| {np.abs(got - want).max():.3e}, pixels beyond 1e-3: {int((np.abs(got - want) > 1e-3).sum())} of {want.size}")
    if tol > 0.0:
        assert np.abs(got.astype(np.float64) - want).max() <= tol, what
    else:
        assert_close(got, want, max_outlier_frac=flip, outlier_cap=cap if flip > 0.0 else None, what=what)


# ------------------------------------------------------------------------------------------------ conversion
@pytest.mark.parametrize("i,name", C.conv_cases())
def test_conversion_against_the_reference_fixture_fused_and_two_launch(mifx_lib, ctx, i, name):
    """Every conversion case through the C ABI on pitched, offset arrays: against the fixture in the contract's measure; the fused path equals the two-launch path bit for
    bit; nothing outside the target is written."""
    g = C.golden()
    q = f"v{i}_"
    A, mode, depth, want = S.attribs_from_bytes(g[q + "attribs"]), int(g[q + "mode"]), g[q + "depth"], g[q + "out"]
    n, h, w = depth.shape
    ch = want.shape[3]
    src, _ = _pitched_array(n, h, w, 0, ctx)
    src.copy_(_dev(depth, ctx))
    results = {}
    default = mifx_lib.mifx_shadow_set_conversion_fusion(1)
    try:
        for fused in (1, 0):
            mifx_lib.mifx_shadow_set_conversion_fusion(fused)
            out, block = _pitched_array(n, h, w, ch, ctx)
            # which kernels ran: the size-2 filter is the horizontal kernel alone; a range above 3 takes the two launches whatever the switch says
            fits = A.iFixedFilterSize != 2 and not bool((np.floor(g[q + "radii"] + F(0.5)) > 3).any())
            want_name = "shadow_convert_horz_kernel" if A.iFixedFilterSize == 2 else "shadow_convert_fused_kernel" if (fused and fits) else "shadow_convert_two_launch"
            counts = {k: _launches(ctx, k, lambda: _convert(ctx, src, A, mode, out)) for k in ("shadow_convert_horz_kernel", "shadow_convert_fused_kernel", "shadow_convert_two_launch")}
            assert counts == {k: int(k == want_name) for k in counts}, (name, fused, counts)
            assert _untouched_outside((block, n, h, w)), f"{name}: fused={fused} wrote outside the filterable array"
            results[fused] = out.contiguous().cpu().numpy()
    finally:
        mifx_lib.mifx_shadow_set_conversion_fusion(default)
    print(f"{name}: fused vs two-launch: {int((results[1].view(np.uint32) != results[0].view(np.uint32)).sum())} of {want.size} values differ in their bits")
    assert C.same_bits(results[1], results[0]), name
    assert_close(results[1], want, what=name)


def test_two_contexts_keep_their_own_intermediate_array(mifx_lib, ctx):
    """The two-launch conversion's intermediate array belongs to the context: two contexts converting different arrays in turn get what each gets alone, and a context
    that is closed takes its block with it."""
    from diligentfx_amd import api

    g = C.golden()
    other = api.PostFXContext(0, *blue_noise_tables())
    default = mifx_lib.mifx_shadow_set_conversion_fusion(0)
    try:
        names = [str(n) for n in g["conv_names"]]
        jobs = []
        for c, nm in ((ctx, "conv_260x70_m4_f7"), (other, "conv_50x38_m2_f5")):
            q = f"v{names.index(nm)}_"
            jobs.append((c, _dev(g[q + "depth"], ctx), S.attribs_from_bytes(g[q + "attribs"]), int(g[q + "mode"]), g[q + "out"]))
        for _ in range(2):
            for c, depth_t, A, mode, want in jobs:
                out = torch.empty(want.shape, dtype=torch.float32, device=ctx.device)
                assert_close(_convert(c, depth_t, A, mode, out).cpu().numpy(), want, what="two contexts")
    finally:
        mifx_lib.mifx_shadow_set_conversion_fusion(default)
        other.close()


def test_refusals_through_the_entries_with_a_context(mifx_lib, ctx):
    """A refusal of the entries themselves (real context, real planes: nothing is launched, the target keeps its sentinel)"""
    from diligentfx_amd import binding as B

    depth = torch.zeros((3, 8, 16), dtype=torch.float32, device=ctx.device)
    out = torch.full((3, 8, 16, 2), SENTINEL, dtype=torch.float32, device=ctx.device)
    src, dst = B.shadow_map_array(depth), B.filterable_shadow_map(out)
    for A, mode in ((S.make_attribs(3, 16, 8), 5), (S.make_attribs(2, 16, 8), 2), (S.make_attribs(3, 16, 8), 4), (S.make_attribs(3, 16, 8, iFixedFilterSize=0, fFilterWorldSize=1e6), 2)):
        assert ctx.lib.mifx_shadow_convert_to_filterable(ctx.handle, ctypes.byref(src), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(dst)) == -1
    frame = torch.full((4, 8), 0.5, dtype=torch.float32, device=ctx.device)
    light = torch.full((4, 8), SENTINEL, dtype=torch.float32, device=ctx.device)
    d, o, cam = B.image(frame), B.image(light), B.CameraAttribs()
    for A, mode in ((S.make_attribs(3, 16, 8, iFixedFilterSize=4), 1), (S.make_attribs(3, 16, 8), 0), (S.make_attribs(3, 32, 8), 1), (S.make_attribs(3, 16, 8), 2)):
        p = B.ShadowFilterParams(mode, 0, 0, 0)
        assert ctx.lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(cam), ctypes.byref(A), ctypes.byref(p), ctypes.byref(src), None, ctypes.byref(o), None) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL)) and bool(torch.all(light == SENTINEL))


# ------------------------------------------------------------------------------------------------ look-up
@pytest.mark.parametrize("i,name", C.look_cases())
def test_lookup_against_the_reference_fixture(mifx_lib, ctx, i, name):
    """Every look-up case through the C ABI, fed the fixture's own filterable arrays, on pitched and offset planes"""
    g = C.golden()
    cam, A, frame, arr, mode, across, best = C.lookup_inputs(g, i)
    H, W = frame.shape
    n, mh, mw = arr.shape[:3]
    arr_t, _ = _pitched_array(n, mh, mw, 0 if arr.ndim == 3 else arr.shape[3], ctx)
    arr_t.copy_(_dev(arr, ctx))
    frame_t, _ = _pitched_array(1, H, W, 0, ctx)
    frame_t[0].copy_(_dev(frame, ctx))
    light_t, lblock = _pitched_array(1, H, W, 0, ctx)
    casc_t, cblock = _pitched_array(1, H, W, 2, ctx)
    _filter(ctx, frame_t[0], cam, A, mode, across, best, arr_t, light_t[0], casc_t[0])
    assert _untouched_outside((lblock, 1, H, W)) and _untouched_outside((cblock, 1, H, W)), name
    light, casc = light_t[0].contiguous().cpu().numpy(), casc_t[0].contiguous().cpu().numpy()
    want_l, want_c = g[f"l{i}_light"], g[f"l{i}_cascade"]
    changed = casc[..., 0] != want_c[..., 0]
    print(f"{name}: cascade index changes {int(changed.sum())}")
    assert not changed.any(), name  # (the index is decided by comparisons of strict fp32 values that the device computes with the same operations)
    _check_light(light, want_l, g, i, name)
    assert_close(casc[..., 1], want_c[..., 1], what=name + " blend amount")


def test_convert_then_filter_end_to_end_through_the_python_mirror(mifx_lib, ctx):
    """ShadowMapManager of the Python mirror: convert the fixture's depth slices (3x3), filter with the result; against the fixture's EVSM4 look-up, whose filterable
    array is the reference's conversion of the same slices"""
    from diligentfx_amd import api
    from diligentfx_amd import binding as B

    g = C.golden()
    names = [str(n) for n in g["look_names"]]
    i = names.index("look_evsm4_n3_across_best")
    cam, A, frame, arr, mode, across, best = C.lookup_inputs(g, i)
    mgr = api.ShadowMapManager(ctx, B.SHADOW_MODE_EVSM4)
    fm = mgr.convert_to_filterable(_dev(g["map_depth"][:3], ctx), S.attribs_from_bytes(g["map_conv_attribs"]))
    torch.cuda.synchronize()
    assert tuple(fm.shape) == (3, 48, 64, 4)
    assert_close(fm.cpu().numpy(), g["map_evsm4"], what="python mirror: convert_to_filterable")
    light, casc = mgr.filter(ctx, _dev(frame, ctx), S.camera_struct(cam), A, filter_across_cascades=True, best_cascade_search=True, cascade_info=True)
    torch.cuda.synchronize()
    assert np.array_equal(casc.cpu().numpy()[..., 0], g[f"l{i}_cascade"][..., 0])
    _check_light(light.cpu().numpy(), g[f"l{i}_light"], g, i, "python mirror: convert, then filter")
    # PCF through the mirror, without the cascade plane
    j = names.index("look_pcf5_n5_across_best")
    cam, A, frame, arr, mode, across, best = C.lookup_inputs(g, j)
    light = api.ShadowMapManager(ctx).filter(ctx, _dev(frame, ctx), S.camera_struct(cam), A, shadow_map=_dev(arr, ctx), filter_across_cascades=True, best_cascade_search=True)
    torch.cuda.synchronize()
    _check_light(light.cpu().numpy(), g[f"l{j}_light"], g, j, "python mirror: PCF")
    assert api.ShadowMapManager(ctx).convert_to_filterable(_dev(arr, ctx), A) is None
    with pytest.raises(B.MifxError):
        mgr.convert_to_filterable(_dev(g["map_depth"][:2], ctx), S.attribs_from_bytes(g["map_conv_attribs"]))  # two slices, three cascades


# ------------------------------------------------------------------------------------------------ a larger comparison against the header compiled for the host
def test_larger_arrays_and_frame_against_the_host_header(mifx_lib, ctx, host_lib):
    """512 x 512 x 4 cascades and a 640 x 360 frame, device against the host compilation of the same header (not the fixture): conversions in the contract's measure and
    fused against two-launch bit for bit; look-ups held to the same budgets as the fixture's cases -- the contract for the filterable modes, no differing PCF pixel."""
    n, mw, mh, W, H = 4, 512, 512, 640, 360
    slices = S.shadow_slices(n, mw, mh, seed=1)
    cam = S.frame_camera(W, H)
    frame = S.frame_depth(cam, W, H)
    slices_t, frame_t = _dev(slices, ctx), _dev(frame, ctx)
    filterable = {}
    for mode, fs in ((S.MODE_VSM, 5), (S.MODE_EVSM4, 7)):
        A = S.make_attribs(n, mw, mh, iFixedFilterSize=fs)
        want = C.host_convert(host_lib, slices, A, mode)
        got = {}
        default = mifx_lib.mifx_shadow_set_conversion_fusion(1)
        try:
            for fused in (1, 0):
                mifx_lib.mifx_shadow_set_conversion_fusion(fused)
                out = torch.empty((n, mh, mw, want.shape[3]), dtype=torch.float32, device=ctx.device)
                got[fused] = _convert(ctx, slices_t, A, mode, out).cpu().numpy()
        finally:
            mifx_lib.mifx_shadow_set_conversion_fusion(default)
        assert C.same_bits(got[1], got[0]), mode
        worst, _ = assert_close(got[1], want, what=f"512x512x4 conversion, mode {mode}")
        print(f"conversion mode {mode} filter {fs}: device vs host max rel {worst:.3e}, bit-identical values {float((got[1].view(np.uint32) == want.view(np.uint32)).mean()):.4f}")
        filterable[mode] = want
    for mode, across, best, over in ((S.MODE_PCF, 1, 0, dict(iFixedFilterSize=7)), (S.MODE_PCF, 1, 1, dict(iFixedFilterSize=0, fFilterWorldSize=0.4)),
                                     (S.MODE_VSM, 0, 1, dict(fVSMLightBleedingReduction=0.2)), (S.MODE_EVSM4, 1, 0, dict())):
        A = S.make_attribs(n, mw, mh, **over)
        arr = slices if mode == S.MODE_PCF else filterable[mode]
        want_l, want_c = C.host_filter(host_lib, cam, A, frame, arr, mode, across, best)
        light, casc = _filter(ctx, frame_t, cam, A, mode, across, best, _dev(arr, ctx))
        light, casc = light.cpu().numpy(), casc.cpu().numpy()
        d = np.abs(light.astype(np.float64) - want_l)
        print(f"look-up mode {mode} across {across} best {best} {over}: differing share {float((d > 1e-3).mean()):.3e}, largest difference {d.max():.3e}, "
              f"index changes {int((casc[..., 0] != want_c[..., 0]).sum())}")
        assert np.array_equal(casc[..., 0], want_c[..., 0])
        assert_close(light, want_l, what=f"640x360 look-up, mode {mode}")
        assert_close(casc[..., 1], want_c[..., 1], what=f"640x360 blend amount, mode {mode}")
