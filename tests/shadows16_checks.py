"""The GPU checks of the 16-bit filterable shadow maps as functions of a context (test infrastructure): tests/test_gpu_shadows16.py runs them in the fp32 library,
tests/h4_checks_shadows_oit.py in the native-storage library, where the same kernels are compiled and the same fixture applies unchanged.  The bars are
shadows16_util's."""
import ctypes

import numpy as np
import torch

import shadows16_util as U
import shadows_util as S

F = np.float32
# the code every channel of a block holds before a launch, as int16: bits 0xFBFB = -65376.0 as binary16 (the EVSM moments lie in [-e^5.54, e^11.08]) and 0.984 as
# UNORM16 (the VSM moments of depths up to 0.95 stay below 0.95) -- no case's result
POISON = 0xFBFB - 0x10000
POISON_BITS = 0xFBFB


def torch_dtype(fmt):
    return torch.int16 if fmt == U.FMT_U16X2 else torch.float16


def dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def codes_to_torch(codes, fmt, ctx):
    """numpy codes (uint16 / float16) -> the tensor binding.filterable_shadow_map takes for the format (int16 holds the UNORM16 codes)"""
    c = np.ascontiguousarray(codes)
    return dev(c.view(np.int16) if fmt == U.FMT_U16X2 else c, ctx)


def codes_to_numpy(t, fmt):
    a = t.contiguous().cpu().numpy()
    return a.view(np.uint16) if fmt == U.FMT_U16X2 else a


def pitched_codes(n, h, w, ch, fmt, ctx):
    """(n, h, w, ch) view of the format's dtype with a row pitch of w + 5 texels, a slice pitch of h + 3 rows and an offset of 2 rows and 4 texels into a poisoned block"""
    block = torch.full((n + 1, h + 3, w + 5, ch), POISON, dtype=torch.int16, device=ctx.device)
    typed = block if fmt == U.FMT_U16X2 else block.view(torch.float16)
    return typed[:n, 2:2 + h, 4:4 + w, :], block


def untouched_outside(block, n, h, w):
    m = torch.ones_like(block, dtype=torch.bool)
    m[:n, 2:2 + h, 4:4 + w, :] = False
    return bool(torch.all(block[m] == POISON))


def pitched_f32(h, w, ch, ctx, sentinel=12345.0):
    block = torch.full((h + 3, w + 5, max(ch, 1)), sentinel, dtype=torch.float32, device=ctx.device)
    view = block[2:2 + h, 4:4 + w, :]
    return (view if ch else view[..., 0]), block


def launches(ctx, name, fn):
    from diligentfx_amd import binding as B

    B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, name.encode(), 8))
    try:
        fn()
        times, n = (ctypes.c_float * 8)(), ctypes.c_uint32(0)
        B.check(ctx.lib.mifx_postfx_get_kernel_times(ctx.handle, times, 8, ctypes.byref(n)))
        return n.value
    finally:
        B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, None, 0))


def convert(ctx, depth_t, A, mode, out_t):
    from diligentfx_amd import binding as B

    src, dst = B.shadow_map_array(depth_t), B.filterable_shadow_map(out_t)
    torch.cuda.synchronize()
    B.check(ctx.lib.mifx_shadow_convert_to_filterable(ctx.handle, ctypes.byref(src), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(dst)))
    torch.cuda.synchronize()
    return out_t


def filter_(ctx, frame_t, cam, A, mode, across, best, arr_t, light_t, casc_t):
    from diligentfx_amd import binding as B

    p = B.ShadowFilterParams(mode, across, best, 0)
    fm = B.filterable_shadow_map(arr_t)
    d, o, c = B.image(frame_t), B.image(light_t), B.image(casc_t)
    cam_s = S.camera_struct(cam)
    torch.cuda.synchronize()
    B.check(ctx.lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(cam_s), ctypes.byref(A), ctypes.byref(p), None, ctypes.byref(fm), ctypes.byref(o), ctypes.byref(c)))
    torch.cuda.synchronize()


def check_conversion_case(ctx, i, name):
    """One conversion case through the C ABI into a pitched, offset, poisoned array, with the fusion switch on and off: which kernels ran, nothing outside the target
    written, fused against two-launch bit for bit, the codes against the fixture"""
    g = U.golden()
    A, mode, fmt, depth, want, radii = U.conv_inputs(g, i)
    n, h, w, ch = want.shape
    src = dev(depth, ctx)
    results = {}
    default = ctx.lib.mifx_shadow_set_conversion_fusion(1)
    try:
        for fused in (1, 0):
            ctx.lib.mifx_shadow_set_conversion_fusion(fused)
            out, block = pitched_codes(n, h, w, ch, fmt, ctx)
            fits = A.iFixedFilterSize != 2 and not bool((np.floor(radii + F(0.5)) > 3).any())
            want_name = "shadow_convert_horz_kernel" if A.iFixedFilterSize == 2 else "shadow_convert_fused_kernel" if (fused and fits) else "shadow_convert_two_launch"
            counts = {k: launches(ctx, k, lambda: convert(ctx, src, A, mode, out)) for k in ("shadow_convert_horz_kernel", "shadow_convert_fused_kernel", "shadow_convert_two_launch")}
            assert counts == {k: int(k == want_name) for k in counts}, (name, fused, counts)
            assert untouched_outside(block, n, h, w), f"{name}: fused={fused} wrote outside the filterable array"
            results[fused] = codes_to_numpy(out, fmt)
            assert not (results[fused].view(np.uint16) == POISON_BITS).any(), f"{name}: fused={fused} left texels unwritten"
    finally:
        ctx.lib.mifx_shadow_set_conversion_fusion(default)
    print(f"{name}: fused vs two-launch: {int((results[1].view(np.uint16) != results[0].view(np.uint16)).sum())} of {want.size} codes differ")
    assert U.same_codes(results[1], results[0]), name
    U.check_codes(results[1], want, fmt, name)


def check_lookup_case(ctx, i, name):
    """One look-up case through the C ABI, fed the fixture's 16-bit map in a pitched array, into pitched light and cascade planes"""
    g = U.golden()
    cam, A, frame, codes, fmt, mode, across, best = U.lookup_inputs(g, i)
    H, W = frame.shape
    n, mh, mw, ch = codes.shape
    arr_t, _ = pitched_codes(n, mh, mw, ch, fmt, ctx)
    arr_t.copy_(codes_to_torch(codes, fmt, ctx))
    frame_t = dev(frame, ctx)
    light_t, lblock = pitched_f32(H, W, 0, ctx)
    casc_t, cblock = pitched_f32(H, W, 2, ctx)
    filter_(ctx, frame_t, cam, A, mode, across, best, arr_t, light_t, casc_t)
    for view, block in ((light_t, lblock), (casc_t, cblock)):
        m = torch.ones_like(block, dtype=torch.bool)
        m[2:2 + H, 4:4 + W, :] = False
        assert bool(torch.all(block[m] == 12345.0)), name
    light, casc = light_t.contiguous().cpu().numpy(), casc_t.contiguous().cpu().numpy()
    want_l, want_c = g[f"l{i}_light"], g[f"l{i}_cascade"]
    changed = casc[..., 0] != want_c[..., 0]
    print(f"{name}: cascade index changes {int(changed.sum())}")
    assert not changed.any(), name
    U.check_light(light, want_l, float(g[f"l{i}_tol"]), name)
    U.check_light(casc[..., 1], want_c[..., 1], 0.0, name + " blend amount")


def check_refusals_with_a_context(ctx):
    """The refusals of section A through the entries themselves (real context, real planes): nothing is launched, the target keeps its poison"""
    from diligentfx_amd import binding as B

    depth = torch.zeros((3, 8, 16), dtype=torch.float32, device=ctx.device)
    src = B.shadow_map_array(depth)
    A32, A16 = S.make_attribs(3, 16, 8), S.make_attribs(3, 16, 8, bIs32BitEVSM=0)
    outs = {"u2": torch.full((3, 8, 16, 2), POISON, dtype=torch.int16, device=ctx.device), "h2": torch.full((3, 8, 16, 2), POISON, dtype=torch.int16, device=ctx.device).view(torch.float16),
            "h4": torch.full((3, 8, 16, 4), POISON, dtype=torch.int16, device=ctx.device).view(torch.float16)}
    before = {k: v.clone() for k, v in outs.items()}
    conv = lambda A, mode, t: ctx.lib.mifx_shadow_convert_to_filterable(ctx.handle, ctypes.byref(src), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(B.filterable_shadow_map(t)))  # noqa: E731
    err = lambda: ctx.lib.mifx_last_error().decode()  # noqa: E731
    assert conv(A16, B.SHADOW_MODE_VSM, outs["h2"]) == -1 and "U16X2" in err()       # RG16_FLOAT is not VSM's 16-bit format
    assert conv(A16, B.SHADOW_MODE_EVSM2, outs["u2"]) == -1 and "F16X2" in err()     # ... nor RG16_UNORM EVSM2's
    assert conv(A16, B.SHADOW_MODE_EVSM4, outs["h2"]) == -1 and "F32X4" in err()
    assert conv(A16, B.SHADOW_MODE_VSM, outs["h4"]) == -1
    assert conv(A32, B.SHADOW_MODE_EVSM2, outs["h2"]) == -1 and "bIs32BitEVSM" in err()
    assert conv(A32, B.SHADOW_MODE_EVSM4, outs["h4"]) == -1 and "bIs32BitEVSM" in err()
    frame = torch.full((4, 8), 0.5, dtype=torch.float32, device=ctx.device)
    light = torch.full((4, 8), 12345.0, dtype=torch.float32, device=ctx.device)
    d, o, cam = B.image(frame), B.image(light), B.CameraAttribs()
    for A, mode, key in ((A32, B.SHADOW_MODE_EVSM4, "h4"), (A32, B.SHADOW_MODE_EVSM2, "h2"), (A16, B.SHADOW_MODE_VSM, "h2"), (A16, B.SHADOW_MODE_EVSM4, "h2")):
        p = B.ShadowFilterParams(mode, 0, 0, 0)
        fm = B.filterable_shadow_map(outs[key])
        assert ctx.lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(cam), ctypes.byref(A), ctypes.byref(p), None, ctypes.byref(fm), ctypes.byref(o), None) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k].view(torch.int16), before[k].view(torch.int16)) for k in outs) and bool(torch.all(light == 12345.0))


def check_python_mirror(ctx, host_lib, mode):
    """api.ShadowMapManager(is_32bit_filterable=False) end to end: convert the fixture's depth slices (3x3) into the mode's 16-bit format, then filter with the result.
    The converted map against the fixture's map at the conversion bar; the look-up of the device's OWN map against the host harness fed that same map's bits (not
    against the reference, whose map may differ in a code, which the look-up would amplify) at the project's contract, the cascade index exact."""
    from diligentfx_amd import api
    from diligentfx_amd import binding as B
    from util import assert_close

    g = U.golden()
    fmt = U.FMT_OF_MODE[mode]
    want_map = {S.MODE_VSM: g["map_vsm"], S.MODE_EVSM2: g["map_evsm2"], S.MODE_EVSM4: g["map_evsm4"]}[mode]
    mgr = api.ShadowMapManager(ctx, mode, is_32bit_filterable=False)
    Aconv = S.attribs_from_bytes(g["map_conv_attribs"])
    Aconv.bIs32BitEVSM = 1  # (the manager sets it, as ShadowMapManager.cpp:157 does)
    fm = mgr.convert_to_filterable(dev(g["map_depth"], ctx), Aconv)
    torch.cuda.synchronize()
    assert Aconv.bIs32BitEVSM == 0 and fm.dtype == torch_dtype(fmt) and tuple(fm.shape) == want_map.shape
    codes = codes_to_numpy(fm, fmt)
    U.check_codes(codes, want_map, fmt, f"python mirror: convert_to_filterable, mode {mode}")
    assert np.array_equal(api.ShadowMapManager.widen(fm).cpu().numpy(), U.widen(codes, fmt))
    i = [k for k, _ in U.look_cases() if int(g[f"l{k}_params"][0]) == mode and tuple(g[f"l{k}_frame_size"]) == (67, 45)][0]
    cam, A, frame, _, _, _, across, best = U.lookup_inputs(g, i)
    A.bIs32BitEVSM = 1
    light, casc = mgr.filter(ctx, dev(frame, ctx), S.camera_struct(cam), A, filter_across_cascades=bool(across), best_cascade_search=bool(best), cascade_info=True)
    torch.cuda.synchronize()
    assert A.bIs32BitEVSM == 0
    want_l, want_c = U.host_filter(host_lib, cam, A, frame, codes, fmt, mode, across, best)
    light, casc = light.cpu().numpy(), casc.cpu().numpy()
    print(f"python mirror, mode {mode}: look-up of the device's own map vs the host harness on the same bits: max |diff| {np.abs(light - want_l).max():.3e}")
    assert np.array_equal(casc[..., 0], want_c[..., 0])
    assert_close(light, want_l, what=f"python mirror: convert, then filter, mode {mode}")
    assert_close(casc[..., 1], want_c[..., 1], what=f"python mirror: blend amount, mode {mode}")


def check_python_mirror_keeps_the_callers_flag_for_fp32_maps(ctx):
    """api.ShadowMapManager with an fp32 filterable array and bIs32BitEVSM = 0 (the exponent clamp alone: the 32-bit fixture's conv_13x9_m4_f3_16bit_clamp): the
    flag stays as the caller gave it and the result is the clamped one, as before the 16-bit formats existed; the same array handed to a manager created for 16-bit
    maps is still described by its own dtype"""
    import test_shadows_cpu as C32
    from diligentfx_amd import api
    from diligentfx_amd import binding as B
    from util import assert_close

    g = C32.golden()
    i = [str(n) for n in g["conv_names"]].index("conv_13x9_m4_f3_16bit_clamp")
    q = f"v{i}_"
    for is32 in (True, False):
        A = S.attribs_from_bytes(g[q + "attribs"])
        assert A.bIs32BitEVSM == 0
        mgr = api.ShadowMapManager(ctx, B.SHADOW_MODE_EVSM4, is_32bit_filterable=is32)
        out = torch.empty(g[q + "out"].shape, dtype=torch.float32, device=ctx.device)
        fm = mgr.convert_to_filterable(dev(g[q + "depth"], ctx), A, out=out)
        torch.cuda.synchronize()
        assert A.bIs32BitEVSM == 0 and fm.dtype == torch.float32
        assert_close(fm.cpu().numpy(), g[q + "out"], what=f"python mirror: fp32 map, bIs32BitEVSM = 0, is_32bit_filterable={is32}")
        A1 = S.attribs_from_bytes(g[q + "attribs"])
        A1.bIs32BitEVSM = 1
        mgr.convert_to_filterable(dev(g[q + "depth"], ctx), A1, out=out)
        torch.cuda.synchronize()
        assert A1.bIs32BitEVSM == 1 and float(out.max()) > float(g[q + "out"].max()) * 10.0  # (unclamped exponents: e^80 against e^11)
