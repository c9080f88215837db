"""Cascaded shadow maps without a GPU: the product's per-texel bodies (diligentfx_amd/csrc/mifx_shadows.h) compiled for the host against the reference's outputs
(tests/golden/shadows_golden.npz, written by tests/golden/make_golden_shadows.py from the reference's shader text), and the C ABI of the feature.

Criterion: the header compiled for the host reproduces every stored array of the reference's strict build BIT FOR BIT -- the moment arrays of every conversion case, the
light amount, the cascade index and the blend amount of every look-up case.  (Both are the same fp32 operations in the same order and, on the host, the same libm expf;
no case had to be excepted.)"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import shadows_util as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32


def golden():
    return np.load(os.path.join(HERE, "golden", "shadows_golden.npz"))


def conv_cases():
    return [(i, str(n)) for i, n in enumerate(golden()["conv_names"])]


def look_cases():
    return [(i, str(n)) for i, n in enumerate(golden()["look_names"])]


def lookup_inputs(g, i):
    """(camera floats, attribs struct, frame depth, the array the mode reads, mode, across, best) of look-up case i"""
    q = f"l{i}_"
    W, H = (int(v) for v in g[q + "frame_size"])
    mode, across, best = (int(v) for v in g[q + "params"])
    A = S.attribs_from_bytes(g[q + "attribs"])
    n = A.iNumCascades
    arr = {S.MODE_PCF: g["map_depth"][:n], S.MODE_VSM: g["map_vsm"], S.MODE_EVSM2: g["map_evsm4"][..., :2], S.MODE_EVSM4: g["map_evsm4"]}[mode]
    return g[f"camera_{W}x{H}"], A, g[f"frame_{W}x{H}"], np.ascontiguousarray(arr), mode, across, best


@pytest.fixture(scope="module")
def host_lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return build_host_lib(hipcc)


def build_host_lib(hipcc):
    from test_grid_cpu import has_openmp

    src = os.path.join(HERE, "host_kernels", "shadows_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "shadows_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n) for n in ("mifx_shadows.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"),
               "-I", os.path.join(ROOT, "include"), "-o", out, src]
        if not has_openmp(hipcc):  # (a toolchain without the OpenMP runtime: the loops then run on one thread)
            cmd.remove("-fopenmp")
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return ctypes.CDLL(out)


def host_convert(lib, depth, A, mode):
    n, h, w = depth.shape
    out = np.zeros((n, h, w, 4 if mode == S.MODE_EVSM4 else 2), F)
    assert lib.mifx_host_shadow_convert(S.fptr(np.ascontiguousarray(depth)), w, h, n, ctypes.byref(A), ctypes.c_uint32(mode), S.fptr(out)) == 0
    return out


def host_filter(lib, cam, A, frame, arr, mode, across, best):
    H, W = frame.shape
    light, casc = np.zeros((H, W), F), np.zeros((H, W, 2), F)
    cam_s = S.camera_struct(cam)
    assert lib.mifx_host_shadow_filter(S.fptr(np.ascontiguousarray(frame)), W, H, ctypes.byref(cam_s), ctypes.byref(A), ctypes.c_uint32(mode), across, best, S.fptr(arr), arr.shape[2],
                                       arr.shape[1], arr.shape[0], S.fptr(light), S.fptr(casc)) == 0
    return light, casc


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the product's header on the host against the reference
@pytest.mark.parametrize("i,name", conv_cases())
def test_conversion_on_the_host_reproduces_the_reference_bit_for_bit(host_lib, i, name):
    g = golden()
    q = f"v{i}_"
    A = S.attribs_from_bytes(g[q + "attribs"])
    got = host_convert(host_lib, g[q + "depth"], A, int(g[q + "mode"]))
    want = g[q + "out"]
    print(f"{name}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} values differ in their bits; max |diff| {np.abs(got - want).max():.3e}")
    assert np.isfinite(got).all() and same_bits(got, want)


@pytest.mark.parametrize("i,name", conv_cases())
def test_fused_tile_stages_on_the_host_equal_the_two_passes_bit_for_bit(host_lib, i, name):
    """shadow_convert_fused_kernel's three stages (the same functions, walked serially, the staging arrays poisoned beforehand) against the reference's two draws"""
    g = golden()
    q = f"v{i}_"
    A, mode, depth, want = S.attribs_from_bytes(g[q + "attribs"]), int(g[q + "mode"]), np.ascontiguousarray(g[q + "depth"]), g[q + "out"]
    n, h, w = depth.shape
    out = np.full(want.shape, -7.0, F)
    rc = host_lib.mifx_host_shadow_convert_tiled(S.fptr(depth), w, h, n, ctypes.byref(A), ctypes.c_uint32(mode), S.fptr(out))
    takes_two_launches = A.iFixedFilterSize == 2 or bool((np.floor(g[q + "radii"] + F(0.5)) > 3).any())
    assert rc == (-2 if takes_two_launches else 0), name
    if rc == 0:
        assert same_bits(out, want), name


def test_conversion_radii_are_the_hosts():
    """The radii the fixture's generator handed to the reference's shaders are what ConvertToFilterable computes from the attribs (ShadowMapManager.cpp:545-579): the
    cases cover range 0 with a fractional radius, unequal axes and a range beyond the fused kernel's tile."""
    g = golden()
    names = [str(n) for n in g["conv_names"]]
    r = g[f"v{names.index('conv_50x38_m3_world')}_radii"]
    assert np.allclose(r, [[2.6, 0.3], [1.2, 1.7], [3.4, 0.0]], atol=1e-6) and not np.array_equal(r[:, 0], r[:, 1])
    assert np.floor(r[0, 1] + F(0.5)) == 0 and r[0, 1] > 0
    big = g[f"v{names.index('conv_50x38_m2_world_large')}_radii"]
    assert np.floor(big + F(0.5)).max() > 3
    # the 16-bit flag and the exponents above the clamp change the result (GetEVSMExponents: 5.54 / 42)
    base, half, above = (g[f"v{names.index(n)}_out"] for n in ("conv_13x9_m4_f5", "conv_13x9_m4_f3_16bit_clamp", "conv_13x9_m4_f5_above_clamp"))
    assert half.max() < np.exp(2 * 5.54) * 1.01 and above.max() > base.max() and above.max() <= np.exp(2 * 42.0) * 1.01


@pytest.mark.parametrize("i,name", look_cases())
def test_lookup_on_the_host_reproduces_the_reference_bit_for_bit(host_lib, i, name):
    g = golden()
    cam, A, frame, arr, mode, across, best = lookup_inputs(g, i)
    light, casc = host_filter(host_lib, cam, A, frame, arr, mode, across, best)
    want_l, want_c = g[f"l{i}_light"], g[f"l{i}_cascade"]
    print(f"{name}: light amount max |diff| {np.abs(light - want_l).max():.3e}, index changes {int((casc[..., 0] != want_c[..., 0]).sum())}")
    assert same_bits(light, want_l) and same_bits(casc, want_c)


def test_fixture_covers_what_the_lookup_can_do():
    g = golden()
    names = [str(n) for n in g["look_names"]]
    seen_modes, seen_sizes, seen_counts, seen_switches = set(), set(), set(), set()
    for i, name in enumerate(names):
        A = S.attribs_from_bytes(g[f"l{i}_attribs"])
        mode, across, best = (int(v) for v in g[f"l{i}_params"])
        seen_modes.add(mode), seen_counts.add(A.iNumCascades), seen_switches.add((across, best))
        if mode == S.MODE_PCF:
            seen_sizes.add(max(A.iFixedFilterSize, 0))
        W, H = (int(v) for v in g[f"l{i}_frame_size"])
        if (W, H) == (67, 45):
            idx, light = g[f"l{i}_cascade"][..., 0], g[f"l{i}_light"]
            frame, cam = g["frame_67x45"], g["camera_67x45"]
            assert (frame == cam[11]).any() and np.all(light[frame == cam[11]] == 1) and np.all(idx[frame == cam[11]] == A.iNumCascades)  # background pixels
            assert A.iNumCascades == 8 or ((idx == A.iNumCascades) & (frame != cam[11])).any()                                       # beyond the last cascade (eight reach the far plane)
            assert set(range(min(A.iNumCascades, 4))) <= set(int(v) for v in idx.reshape(-1))                                         # points in the near cascades
            assert (light < 0.5).any() and (light > 0.95).any() and ((light > 0.2) & (light < 0.8)).any()  # shadowed, lit and penumbra pixels
            if across:
                b = g[f"l{i}_cascade"][..., 1]
                assert ((b > 0) & (b < 1)).any()                                                                                      # points in the transition regions
    assert seen_modes == {1, 2, 3, 4} and seen_sizes == {0, 2, 3, 5, 7} and seen_counts == {1, 3, 5, 8} and seen_switches == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # best-cascade search: some pixel lies outside the margin of the cascade its camera z selects, and takes the next one
    i0, i1 = names.index("look_evsm4_n3_lbr"), names.index("look_evsm4_n3_across_best")
    assert (g[f"l{i1}_cascade"][..., 0] != g[f"l{i0}_cascade"][..., 0]).any()
    # the small receiver-plane bias clamp acts
    assert not np.array_equal(g[f"l{names.index('look_pcf3_n3')}_light"], g[f"l{names.index('look_pcf3_n3_bias_clamp')}_light"])
    for i in range(len(names)):
        assert float(g[f"l{i}_tol"]) == 0.0 and float(g[f"l{i}_flip_budget"]) == 0.0  # every case is held to the project's contract (see the generator)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_struct_layout_and_defaults(mifx_lib):
    from diligentfx_amd import binding as B

    assert ctypes.sizeof(B.ShadowMapAttribs) == 1200 == mifx_lib.mifx_sizeof(b"shadow_map_attribs")
    assert ctypes.sizeof(B.CascadeAttribs) == 64 == mifx_lib.mifx_sizeof(b"cascade_attribs")
    assert B.MAX_CASCADES == 8 and (B.SHADOW_MODE_PCF, B.SHADOW_MODE_VSM, B.SHADOW_MODE_EVSM2, B.SHADOW_MODE_EVSM4) == (1, 2, 3, 4)
    off = {n: getattr(B.ShadowMapAttribs, n).offset for n, _ in B.ShadowMapAttribs._fields_}
    assert (off["mWorldToLightView"], off["Cascades"], off["mWorldToShadowMapUVDepth"], off["fCascadeCamSpaceZEnd"], off["f4ShadowMapDim"], off["iNumCascades"],
            off["fReceiverPlaneDepthBiasClamp"], off["fVSMBias"], off["bIs32BitEVSM"], off["fDummy"]) == (0, 64, 576, 1088, 1120, 1136, 1152, 1168, 1184, 1196)
    a = B.ShadowMapAttribs()
    ctypes.memset(ctypes.byref(a), 0xFF, 1200)
    assert mifx_lib.mifx_shadow_map_default_attribs(ctypes.byref(a)) == 0
    assert bytes(a) == bytes(B.ShadowMapAttribs.default())
    # BasicStructures.fxh:47-65
    assert (a.iNumCascades, a.fNumCascades, a.bVisualizeCascades, a.bVisualizeShadowing) == (0, 0.0, 0, 0)
    assert (a.fReceiverPlaneDepthBiasClamp, a.fFixedDepthBias, a.fCascadeTransitionRegion, a.iMaxAnisotropy) == (10.0, float(F(1e-5)), float(F(0.1)), 4)
    assert (a.fVSMBias, a.fVSMLightBleedingReduction, a.fEVSMPositiveExponent, a.fEVSMNegativeExponent) == (float(F(1e-4)), 0.0, 40.0, 5.0)
    assert (a.bIs32BitEVSM, a.iFixedFilterSize, a.fFilterWorldSize) == (1, 3, 0.0)
    assert mifx_lib.mifx_shadow_map_default_attribs(None) == -1


def test_refusals(mifx_lib):
    """Every refusal through the check entries, which run the argument checks of the two entries and nothing else (no context, no device): a refusal that regressed is a
    failed assertion here.  The entries themselves refuse a null context first."""
    from diligentfx_amd import binding as B

    A = S.make_attribs(3, 16, 8)
    sm = B.ShadowMapArray(0x1000, 16, 8, 3, 64, 512)
    fm2 = B.FilterableShadowMap(0x1000, 16, 8, 3, B.FORMAT_F32X2, 128, 1024)
    fm4 = B.FilterableShadowMap(0x1000, 16, 8, 3, B.FORMAT_F32X4, 256, 2048)
    conv = lambda sm_, A_, mode, fm_: mifx_lib.mifx_shadow_convert_check(ctypes.byref(sm_), ctypes.byref(A_), ctypes.c_uint32(mode), ctypes.byref(fm_))  # noqa: E731
    err = lambda: mifx_lib.mifx_last_error().decode()  # noqa: E731
    for mode, fm in ((B.SHADOW_MODE_VSM, fm2), (B.SHADOW_MODE_EVSM2, fm2), (B.SHADOW_MODE_EVSM4, fm4)):
        assert conv(sm, A, mode, fm) == 0, err()                                      # what is asked for is accepted
    assert conv(sm, A, 1, fm2) == -1 and "mode" in err()
    assert conv(sm, A, 5, fm2) == -1 and "mode" in err()
    assert conv(sm, A, B.SHADOW_MODE_EVSM4, fm2) == -1 and "F32X4" in err()          # wrong format for the mode
    assert conv(sm, A, B.SHADOW_MODE_VSM, fm4) == -1 and "F32X2" in err()
    assert conv(B.ShadowMapArray(0x1000, 16, 8, 2, 64, 512), A, B.SHADOW_MODE_VSM, fm2) == -1 and "cascades" in err()  # slice count != iNumCascades
    assert conv(sm, A, B.SHADOW_MODE_VSM, B.FilterableShadowMap(0x1000, 16, 9, 3, B.FORMAT_F32X2, 128, 2048)) == -1  # another size
    assert conv(sm, A, B.SHADOW_MODE_VSM, B.FilterableShadowMap(0x1000, 16, 8, 3, B.FORMAT_F32X2, 120, 1024)) == -1 and "pitch" in err()
    assert conv(sm, A, B.SHADOW_MODE_VSM, B.FilterableShadowMap(0x1000, 16, 8, 3, B.FORMAT_F32X2, 128, 1000)) == -1 and "slice pitch" in err()
    assert conv(B.ShadowMapArray(0x1000, 16, 8, 3, 0x80000000, 0x80000000 * 8), A, B.SHADOW_MODE_VSM, fm2) == -1 and "pitch" in err()  # a pitch beyond 2^31 - 1
    A9 = S.make_attribs(9, 16, 8)
    assert conv(B.ShadowMapArray(0x1000, 16, 8, 9, 64, 512), A9, B.SHADOW_MODE_VSM, B.FilterableShadowMap(0x1000, 16, 8, 9, B.FORMAT_F32X2, 128, 1024)) == -1 and "iNumCascades" in err()
    assert mifx_lib.mifx_shadow_convert_check(None, ctypes.byref(A), 2, ctypes.byref(fm2)) == -1
    # every finite radius is taken, also one wider than the slice (here about 48 texels on a 16 x 8 slice) ...
    assert conv(sm, S.make_attribs(3, 16, 8, iFixedFilterSize=0, fFilterWorldSize=100.0), B.SHADOW_MODE_VSM, fm2) == 0, err()
    # ... up to MIFX_SHADOW_MAX_FILTER_RADIUS: a radius is a loop count on the device
    assert conv(sm, S.make_attribs(3, 16, 8, iFixedFilterSize=0, fFilterWorldSize=float("inf")), B.SHADOW_MODE_VSM, fm2) == -1 and "radii" in err()
    assert conv(sm, S.make_attribs(3, 16, 8, iFixedFilterSize=0, fFilterWorldSize=1e6), B.SHADOW_MODE_VSM, fm2) == -1 and "radii" in err()
    # the entry itself: a null context is refused before anything else is looked at
    assert mifx_lib.mifx_shadow_convert_to_filterable(None, ctypes.byref(sm), ctypes.byref(A), 2, ctypes.byref(fm2)) == -1 and "context" in err()

    cam = B.CameraAttribs()
    d = B.Image2D(0x1000, 8, 4, 32, B.FORMAT_F32)
    o = B.Image2D(0x2000, 8, 4, 32, B.FORMAT_F32)

    def filt(A_, mode, sm_=sm, fm_=None, out=o, casc=None, across=0, best=0):
        p = B.ShadowFilterParams(mode, across, best, 0)
        return mifx_lib.mifx_shadow_map_filter_check(ctypes.byref(d), ctypes.byref(cam), ctypes.byref(A_), ctypes.byref(p), ctypes.byref(sm_) if sm_ is not None else None,
                                                     ctypes.byref(fm_) if fm_ is not None else None, ctypes.byref(out), ctypes.byref(casc) if casc is not None else None)

    for fs in (2, 3, 5, 7, 0, -1):
        assert filt(S.make_attribs(3, 16, 8, iFixedFilterSize=fs, fFilterWorldSize=0.5), B.SHADOW_MODE_PCF, casc=B.Image2D(0x3000, 8, 4, 64, B.FORMAT_F32X2)) == 0, err()
    assert filt(A, B.SHADOW_MODE_VSM, sm_=None, fm_=fm2) == 0 and filt(A, B.SHADOW_MODE_EVSM2, sm_=None, fm_=fm2) == 0 and filt(A, B.SHADOW_MODE_EVSM4, sm_=None, fm_=fm4) == 0, err()
    assert filt(A, 0) == -1 and filt(A, 5) == -1
    assert filt(A, 1, across=2) == -1
    for bad in (1, 4, 6, 9):
        assert filt(S.make_attribs(3, 16, 8, iFixedFilterSize=bad), B.SHADOW_MODE_PCF) == -1 and "PCF_FILTER_SIZE" in err()
    assert filt(A, B.SHADOW_MODE_PCF, sm_=None) == -1 and filt(A, B.SHADOW_MODE_VSM, fm_=None) == -1       # the map the mode reads is missing
    assert filt(A, B.SHADOW_MODE_EVSM4, fm_=fm2) == -1 and filt(A, B.SHADOW_MODE_EVSM2, fm_=fm4) == -1     # wrong format
    assert filt(A9, B.SHADOW_MODE_PCF) == -1                                                               # more than 8 cascades
    assert filt(S.make_attribs(5, 16, 8), B.SHADOW_MODE_PCF) == -1                                         # fewer slices than cascades
    assert filt(A, B.SHADOW_MODE_PCF, out=B.Image2D(0x2000, 8, 5, 32, B.FORMAT_F32)) == -1                 # light amount of another size
    assert filt(S.make_attribs(3, 32, 8), B.SHADOW_MODE_PCF) == -1 and "f4ShadowMapDim" in err()           # the attribs describe another map size
    assert filt(A, B.SHADOW_MODE_PCF, casc=B.Image2D(0x3000, 8, 4, 64, B.FORMAT_F32)) == -1                # the cascade plane is F32X2
    # the varying filter's footprint is a loop count per pixel: beyond MIFX_SHADOW_MAX_VARYING_PCF_TEXELS (128) it is refused
    big = B.ShadowMapArray(0x1000, 4096, 4096, 3, 16384, 16384 * 4096)
    assert filt(S.make_attribs(3, 4096, 4096, iFixedFilterSize=0, fFilterWorldSize=0.4), B.SHADOW_MODE_PCF, sm_=big) == 0, err()     # about 99 texels in cascade 0
    assert filt(S.make_attribs(3, 4096, 4096, iFixedFilterSize=0, fFilterWorldSize=0.6), B.SHADOW_MODE_PCF, sm_=big) == -1 and "varying" in err()
    assert filt(S.make_attribs(3, 4096, 4096, iFixedFilterSize=0, fFilterWorldSize=float("nan")), B.SHADOW_MODE_PCF, sm_=big) == -1 and "varying" in err()
    p = B.ShadowFilterParams(1, 0, 0, 0)
    assert mifx_lib.mifx_shadow_map_filter(None, ctypes.byref(d), ctypes.byref(cam), ctypes.byref(A), ctypes.byref(p), ctypes.byref(sm), None, ctypes.byref(o), None) == -1 and "context" in err()
    default = mifx_lib.mifx_shadow_set_conversion_fusion(0)  # the internal A/B switch returns the previous value
    assert default in (0, 1) and mifx_lib.mifx_shadow_set_conversion_fusion(1) == 0 and mifx_lib.mifx_shadow_set_conversion_fusion(default) == 1
