"""The 16-bit filterable shadow maps without a GPU: the accept / refuse table of the check entries in both libraries, and the product's per-texel bodies
(diligentfx_amd/csrc/mifx_shadows.h) compiled for the host with a 16-bit filterable array against the reference's outputs (tests/golden/shadows16_golden.npz).
The bars are shadows16_util's: conversion codes within one step of the format on top of the project's contract, no outliers; the fused kernel's tile stages equal the
two passes bit for bit; look-ups within the stored budgets, the cascade index exact."""
import ctypes
import os

import numpy as np
import pytest

import shadows16_util as U
import shadows_util as S

F = np.float32


@pytest.fixture(scope="module")
def host_lib():
    lib = U.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


@pytest.fixture(scope="module")
def h4_lib():
    from diligentfx_amd import binding as B
    from diligentfx_amd import build

    assert os.path.exists(build.OUT_H4), "libmifx_h4.so missing: python -m diligentfx_amd.build"
    lib = ctypes.CDLL(build.OUT_H4)
    lib.mifx_last_error.restype = ctypes.c_char_p
    lib.mifx_storage_mode.restype = ctypes.c_uint32
    assert lib.mifx_storage_mode() == 1
    assert B.FORMAT_U16X2 == 512
    return lib


# ------------------------------------------------------------------------------------------------ the C ABI
def _check_format_table(lib):
    """Section A's table through mifx_shadow_convert_check / mifx_shadow_map_filter_check: no context, no device"""
    from diligentfx_amd import binding as B

    err = lambda: lib.mifx_last_error().decode()  # noqa: E731
    sm = B.ShadowMapArray(0x1000, 16, 8, 3, 64, 512)
    d, o, cam = B.Image2D(0x1000, 8, 4, 32, B.FORMAT_F32), B.Image2D(0x2000, 8, 4, 32, B.FORMAT_F32), B.CameraAttribs()
    A32, A16 = S.make_attribs(3, 16, 8), S.make_attribs(3, 16, 8, bIs32BitEVSM=0)
    texel = {B.FORMAT_F32X2: 8, B.FORMAT_F32X4: 16, B.FORMAT_U16X2: 4, B.FORMAT_F16X2: 4, B.FORMAT_F16X4: 8, B.FORMAT_F32: 4, B.FORMAT_F16: 2, B.FORMAT_U16: 2, B.FORMAT_U8: 1,
             B.FORMAT_R11G11B10: 4}

    def fm(fmt, pitch=None, slice_pitch=None, data=0x1000):
        p = 16 * texel[fmt] if pitch is None else pitch
        return B.FilterableShadowMap(data, 16, 8, 3, fmt, p, p * 8 if slice_pitch is None else slice_pitch)

    def conv(A, mode, m):
        return lib.mifx_shadow_convert_check(ctypes.byref(sm), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(m))

    def filt(A, mode, m):
        p = B.ShadowFilterParams(mode, 0, 0, 0)
        return lib.mifx_shadow_map_filter_check(ctypes.byref(d), ctypes.byref(cam), ctypes.byref(A), ctypes.byref(p), None, ctypes.byref(m), ctypes.byref(o), None)

    accepted = {B.SHADOW_MODE_VSM: (B.FORMAT_F32X2, B.FORMAT_U16X2), B.SHADOW_MODE_EVSM2: (B.FORMAT_F32X2, B.FORMAT_F16X2), B.SHADOW_MODE_EVSM4: (B.FORMAT_F32X4, B.FORMAT_F16X4)}
    for mode, formats in accepted.items():
        for fmt in texel:
            for entry in (conv, filt):
                rc = entry(A16, mode, fm(fmt))
                assert rc == (0 if fmt in formats else -1), (entry.__name__, mode, fmt, err())
    # the message of a wrong format still names the mode's fp32 format
    assert conv(A32, B.SHADOW_MODE_EVSM4, fm(B.FORMAT_F32X2)) == -1 and "F32X4" in err() and "F16X4" in err()
    assert conv(A32, B.SHADOW_MODE_VSM, fm(B.FORMAT_F32X4)) == -1 and "F32X2" in err() and "U16X2" in err()
    # a 16-bit EVSM format with bIs32BitEVSM != 0: exp(40 d) is not a binary16 value
    for entry in (conv, filt):
        assert entry(A32, B.SHADOW_MODE_EVSM2, fm(B.FORMAT_F16X2)) == -1 and "bIs32BitEVSM" in err()
        assert entry(A32, B.SHADOW_MODE_EVSM4, fm(B.FORMAT_F16X4)) == -1 and "bIs32BitEVSM" in err()
        assert entry(A32, B.SHADOW_MODE_VSM, fm(B.FORMAT_U16X2)) == 0, err()             # VSM has no exponent: the flag does not matter
        assert entry(A16, B.SHADOW_MODE_EVSM4, fm(B.FORMAT_F32X4)) == 0, err()           # bIs32BitEVSM == 0 with an fp32 format stays accepted
        assert entry(A16, B.SHADOW_MODE_EVSM2, fm(B.FORMAT_F32X2)) == 0, err()
    # data and both pitches are multiples of the texel size: 4 bytes (U16X2, F16X2), 8 bytes (F16X4)
    for mode, fmt, t in ((B.SHADOW_MODE_VSM, B.FORMAT_U16X2, 4), (B.SHADOW_MODE_EVSM2, B.FORMAT_F16X2, 4), (B.SHADOW_MODE_EVSM4, B.FORMAT_F16X4, 8)):
        assert conv(A16, mode, fm(fmt, pitch=16 * t + t)) == 0, err()                      # padded by one texel
        assert conv(A16, mode, fm(fmt, pitch=16 * t - t)) == -1 and "pitch" in err()       # narrower than the row
        assert conv(A16, mode, fm(fmt, pitch=16 * t + t // 2)) == -1 and "pitch" in err()
        assert conv(A16, mode, fm(fmt, slice_pitch=16 * t * 8 + t // 2)) == -1 and "slice pitch" in err()
        assert conv(A16, mode, fm(fmt, slice_pitch=16 * t * 8 - t)) == -1 and "slice pitch" in err()
        assert conv(A16, mode, fm(fmt, data=0x1000 + t // 2)) == -1 and "alignment" in err()
        assert conv(A16, mode, fm(fmt, data=0x1000 + t)) == 0, err()


def test_format_table_of_the_check_entries(mifx_lib):
    _check_format_table(mifx_lib)


def test_format_table_of_the_check_entries_in_the_native_storage_library(h4_lib):
    _check_format_table(h4_lib)


def test_oit_frame_check_follows_the_build(mifx_lib, h4_lib):
    """mifx_oit_frame_check: the 4-channel planes are F32X4 in the fp32 library and F16X4 in the native-storage one; depth, colour alpha and the opaque depth are
    F32 in both"""
    from diligentfx_amd import binding as B

    def run(lib, fmt4, texel4, alpha_fmt=B.FORMAT_F32):
        cam = B.CameraAttribs()
        img = lambda fmt, t: B.Image2D(0x1000, 8, 4, 8 * t, fmt)  # noqa: E731
        planes = [img(B.FORMAT_F32, 4)] + [img(fmt4, texel4) for _ in range(4)] + [img(alpha_fmt, 4 if alpha_fmt == B.FORMAT_F32 else 2)]
        sl = (B.OITSlice * 1)(B.OITSlice(*[ctypes.pointer(p) for p in planes]))
        tg = [img(fmt4, texel4) for _ in range(4)]
        targets = B.OITTargets(*[ctypes.pointer(t) for t in tg])
        od = img(B.FORMAT_F32, 4)
        return lib.mifx_oit_frame_check(ctypes.c_uint32(8), ctypes.c_uint32(4), sl, ctypes.c_uint32(1), ctypes.byref(od), ctypes.byref(cam), ctypes.byref(targets))

    assert run(mifx_lib, B.FORMAT_F32X4, 16) == 0, mifx_lib.mifx_last_error()
    assert run(mifx_lib, B.FORMAT_F16X4, 8) == -1
    assert run(h4_lib, B.FORMAT_F16X4, 8) == 0, h4_lib.mifx_last_error()
    assert run(h4_lib, B.FORMAT_F32X4, 16) == -1 and b"F16X4" in h4_lib.mifx_last_error()
    assert run(h4_lib, B.FORMAT_F16X4, 8, alpha_fmt=B.FORMAT_F16) == -1  # colour alpha stays F32
    assert h4_lib.mifx_oit_create_check(ctypes.c_uint32(8), ctypes.c_uint32(4), ctypes.c_uint32(4)) == 0


# ------------------------------------------------------------------------------------------------ the converters on the host
def test_host_converters_are_the_render_target_conversions(host_lib):
    """shadow_quantize on the host: binary16 is numpy's round-to-nearest-even (ties, subnormals, overflow to infinity), UNORM16 is NaN -> 0, clamp, x 65535, + 0.5,
    truncate, read back as code / 65535 correctly rounded"""
    rng = np.random.default_rng(3)
    v = np.concatenate([np.linspace(-70000, 70000, 4001), 2.0 ** np.arange(-30, 17), (1.0 + 2.0 ** -11) * 2.0 ** np.arange(-26, 16), (1.0 + 3 * 2.0 ** -11) * 2.0 ** np.arange(-26, 16),
                        rng.standard_normal(4000) * 1e-5, rng.uniform(-0.1, 1.1, 4000), np.arange(65536) / 65535.0, (np.arange(65535) + 0.5) / 65535.0,
                        [65519.99, 65520.0, 0.0, -0.0, np.inf, -np.inf, np.nan]]).astype(F)
    out = np.zeros_like(v)
    for fmt in (U.FMT_F16X2, U.FMT_F16X4):
        host_lib.mifx_host_shadow16_quantize(S.fptr(v), v.size, ctypes.c_uint32(fmt), S.fptr(out))
        with np.errstate(over="ignore"):
            want = v.astype(np.float16).astype(F)
        assert np.array_equal(out, want, equal_nan=True)
    host_lib.mifx_host_shadow16_quantize(S.fptr(v), v.size, ctypes.c_uint32(U.FMT_U16X2), S.fptr(out))
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(v), F(0), np.clip(v, F(0), F(1)))
        code = np.floor((c * F(65535.0)).astype(F) + F(0.5)).astype(np.float64)
    assert np.array_equal(out, (code / 65535.0).astype(F))
    host_lib.mifx_host_shadow16_quantize(S.fptr(v), v.size, ctypes.c_uint32(0), S.fptr(out))
    assert np.array_equal(out.view(np.uint32), v.view(np.uint32))  # fp32: the identity


# ------------------------------------------------------------------------------------------------ the header on the host against the reference
@pytest.mark.parametrize("i,name", U.conv_cases())
def test_conversion_on_the_host_against_the_reference_codes(host_lib, i, name):
    g = U.golden()
    A, mode, fmt, depth, want, radii = U.conv_inputs(g, i)
    rc, got = U.host_convert(host_lib, depth, A, mode, fmt)
    assert rc == 0
    U.check_codes(got, want, fmt, name)


@pytest.mark.parametrize("i,name", U.conv_cases())
def test_fused_tile_stages_on_the_host_equal_the_two_passes_bit_for_bit(host_lib, i, name):
    """The fused kernel's three stages with stage B's results rounded to the format's values (LDS stays fp32) against the two passes through a 16-bit intermediate"""
    g = U.golden()
    A, mode, fmt, depth, want, radii = U.conv_inputs(g, i)
    rc2, two = U.host_convert(host_lib, depth, A, mode, fmt)
    rc, tiled = U.host_convert(host_lib, depth, A, mode, fmt, tiled=True)
    takes_two_launches = A.iFixedFilterSize == 2 or bool((np.floor(radii + F(0.5)) > 3).any())
    assert rc2 == 0 and rc == (-2 if takes_two_launches else 0), name
    if rc == 0:
        print(f"{name}: {int((tiled.view(np.uint16) != two.view(np.uint16)).sum())} of {two.size} codes differ between the tile stages and the two passes")
        assert U.same_codes(tiled, two), name


def test_the_intermediate_rounding_is_visible(host_lib):
    """The cases would not notice a fused path that skipped the rounding of stage B unless that rounding changed some output code: the two-pass result through an
    fp32 intermediate, rounded at the end only, differs from the fixture's in some code of every blurred format"""
    g = U.golden()
    names = [str(n) for n in g["conv_names"]]
    for nm in ("conv16_260x70_m2_f3", "conv16_260x70_m3_f3", "conv16_260x70_m4_f3"):
        A, mode, fmt, depth, want, radii = U.conv_inputs(g, names.index(nm))
        rc, wide = U.host_convert(host_lib, depth, A, mode, 0)
        assert rc == 0
        if fmt == U.FMT_U16X2:
            late = np.floor((np.clip(wide, 0, 1) * F(65535.0)).astype(F) + F(0.5)).astype(np.uint16)
        else:
            late = wide.astype(np.float16)
        assert not U.same_codes(late, want), nm


@pytest.mark.parametrize("i,name", U.look_cases())
def test_lookup_on_the_host_from_the_16bit_maps(host_lib, i, name):
    g = U.golden()
    cam, A, frame, codes, fmt, mode, across, best = U.lookup_inputs(g, i)
    light, casc = U.host_filter(host_lib, cam, A, frame, codes, fmt, mode, across, best)
    want_l, want_c = g[f"l{i}_light"], g[f"l{i}_cascade"]
    assert np.array_equal(casc[..., 0], want_c[..., 0]), name
    U.check_light(light, want_l, float(g[f"l{i}_tol"]), name)
    U.check_light(casc[..., 1], want_c[..., 1], 0.0, name + " blend amount")


def test_fixture_covers_the_formats_and_paths():
    g = U.golden()
    seen = set()
    for i, name in U.conv_cases():
        A, mode, fmt, depth, want, radii = U.conv_inputs(g, i)
        assert fmt == U.FMT_OF_MODE[mode] and A.bIs32BitEVSM == 0 and want.dtype == U.code_dtype(fmt)
        path = "horz" if A.iFixedFilterSize == 2 else "two" if (np.floor(radii + F(0.5)) > 3).any() else "fused"
        seen.add((fmt, path, want.shape[:3]))
        assert float(g[f"v{i}_strict_vs_contracted_steps"]) <= 1.0
    for fmt in U.FMT_OF_MODE.values():
        assert {(p, s) for f, p, s in seen if f == fmt} == {("horz", (1, 9, 13)), ("fused", (1, 9, 13)), ("fused", (3, 38, 50)), ("two", (3, 38, 50)), ("fused", (2, 70, 260))}
    sizes = {tuple(int(v) for v in g[f"l{i}_frame_size"]) for i, _ in U.look_cases()}
    assert sizes == {(67, 45), (2, 2), (1, 1)} and {int(g[f"l{i}_params"][0]) for i, _ in U.look_cases()} == {2, 3, 4}
    # the EVSM moments use the binary16 range that the clamped exponents leave (5.54: e^11.08 < 65504), the UNORM ones the whole of [0, 1]
    assert 1000.0 < float(U.widen(g["map_evsm4"], U.FMT_F16X4).max()) < 65504.0 and np.isfinite(U.widen(g["map_evsm4"], U.FMT_F16X4)).all()
    assert g["map_vsm"].dtype == np.uint16 and g["map_vsm"].max() > 40000


def test_python_mirror_formats():
    """api.ShadowMapManager(is_32bit_filterable=False): the dtypes, bIs32BitEVSM set to 0 for a 16-bit array (ShadowMapManager.cpp:157) and left as the caller gave it
    for an fp32 one -- also by the dtype of an array handed over explicitly, whatever the manager's own flag says -- and widen()"""
    import torch

    from diligentfx_amd import api
    from diligentfx_amd import binding as B

    for mode, dt in ((B.SHADOW_MODE_VSM, torch.int16), (B.SHADOW_MODE_EVSM2, torch.float16), (B.SHADOW_MODE_EVSM4, torch.float16)):
        m16, m32 = api.ShadowMapManager(None, mode, is_32bit_filterable=False), api.ShadowMapManager(None, mode)
        assert m16.filterable_dtype() == dt and m32.filterable_dtype() == torch.float32
        ch = 4 if mode == B.SHADOW_MODE_EVSM4 else 2
        wide, narrow = torch.zeros((1, 2, 2, ch), dtype=torch.float32), torch.zeros((1, 2, 2, ch), dtype=dt)
        for given in (0, 1):  # an fp32 array: the caller's flag stays (0 with an fp32 map is the exponent clamp alone, accepted by the library)
            for mgr in (m16, m32):
                A = B.ShadowMapAttribs.default()
                A.bIs32BitEVSM = given
                assert mgr.set_format_attribs(A, wide).bIs32BitEVSM == given
            A = B.ShadowMapAttribs.default()
            A.bIs32BitEVSM = given
            assert m32.set_format_attribs(A).bIs32BitEVSM == given
            for mgr, arr in ((m16, None), (m16, narrow), (m32, narrow)):  # a 16-bit array: 0
                A = B.ShadowMapAttribs.default()
                A.bIs32BitEVSM = given
                assert mgr.set_format_attribs(A, arr).bIs32BitEVSM == 0
    A = B.ShadowMapAttribs.default()
    assert api.ShadowMapManager(None, B.SHADOW_MODE_PCF, is_32bit_filterable=False).set_format_attribs(A).bIs32BitEVSM == 1  # PCF has no filterable map: untouched
    codes = np.array([0, 1, 32767, 32768, 65535], np.uint16)
    w = api.ShadowMapManager.widen(torch.from_numpy(codes.view(np.int16).copy()))
    assert w.dtype == torch.float32 and np.array_equal(w.numpy(), U.widen(codes, U.FMT_U16X2))
    h = np.array([0.5, -2.25, 65504.0, 6e-8], np.float16)
    assert np.array_equal(api.ShadowMapManager.widen(torch.from_numpy(h)).numpy(), h.astype(F))
    t16 = torch.zeros((3, 8, 16, 2), dtype=torch.int16)
    d = B.filterable_shadow_map(t16)
    assert (d.format, d.pitch_bytes, d.slice_pitch_bytes) == (B.FORMAT_U16X2, 64, 512)
    d = B.filterable_shadow_map(torch.zeros((3, 8, 16, 4), dtype=torch.float16))
    assert (d.format, d.pitch_bytes, d.slice_pitch_bytes) == (B.FORMAT_F16X4, 128, 1024)
    d = B.filterable_shadow_map(torch.zeros((3, 8, 16, 2), dtype=torch.float32))
    assert (d.format, d.pitch_bytes, d.slice_pitch_bytes) == (B.FORMAT_F32X2, 128, 1024)
