"""The composite's fused instance (mifx_composite.h, FUSE_R7) does not enter its reflection block where the reflection mask is 0: compiled for the HOST (the build of
tests/test_host_kernel_chain.py) and held to the unfused body fed with the plane of the stand-alone R7 on frames whose mask changes from pixel to pixel, and to
colour x AO factor where the planes the block would have read hold a sentinel.  Test infrastructure: the product never builds, loads or calls this."""
import ctypes

import numpy as np
import pytest

from test_host_kernel_chain import fptr, host_lib  # noqa: F401 -- (the fixture that builds tests/host_kernels/chain_host.cpp)

F = np.float32


def _frame(w, h, seed):
    """Finite random planes.  Mask: a per-pixel coin, so that neighbouring pixels (the lanes of one wave) differ.  A fifth of the frame is background (opacity 0).  Half of
    the pixels have no variance (R7 passes their accumulated radiance through, no taps) and 40 % an accumulated radiance of exactly 0 (every ray of the history missed), so
    that inside the mask both `refl.w == 0` and `refl.w != 0` occur; the other half runs R7's tap loop over neighbours of both kinds."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.random(s, dtype=F)  # noqa: E731
    p = {}
    p["color"] = np.concatenate([u(h, w, 3) * F(4.0) + F(0.01), (u(h, w, 1) > 0.2).astype(F)], -1)
    p["specular_ibl"] = u(h, w, 4) * F(2.0)
    n = rng.standard_normal((h, w, 3)).astype(F)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True).astype(F)
    p["normal"] = np.ascontiguousarray(np.concatenate([n, np.zeros((h, w, 1), F)], -1).astype(F))
    p["base_color"] = u(h, w, 4)
    p["material"] = u(h, w, 4)
    p["ssao"] = u(h, w)
    p["depth"] = F(0.2) + F(0.7) * u(h, w)
    p["roughness"] = u(h, w) * F(0.3)
    p["variance"] = np.where(u(h, w) < 0.5, F(0.0), u(h, w) * F(0.01)).astype(F)
    p["radiance"] = (u(h, w, 4) * (u(h, w, 1) > 0.4)).astype(F)
    p["mask"] = (u(h, w) < 0.5).astype(F)
    p["lut"] = u(32, 32, 2)
    return {k: np.ascontiguousarray(v) for k, v in p.items()}


def _run(host_lib, p, w, h, cam, a, fused, ssr=None):
    null = ctypes.POINTER(ctypes.c_float)()
    out = np.zeros((h, w, 4), F)
    lut = p["lut"]
    rc = host_lib.mifx_host_composite(fptr(p["color"]), fptr(p["specular_ibl"]), null if fused else fptr(ssr), fptr(p["ssao"]), fptr(p["normal"]), fptr(p["base_color"]),
                                      fptr(p["material"]), fptr(lut), lut.shape[1], lut.shape[0], lut.shape[2], fptr(out), w, h, ctypes.byref(cam), ctypes.c_float(1.0),
                                      ctypes.c_float(1.0), fptr(p["depth"]), fptr(p["roughness"]), fptr(p["radiance"]), fptr(p["variance"]), fptr(p["mask"]),
                                      ctypes.c_float(a.RoughnessThreshold), ctypes.c_float(a.BilateralCleanupSpatialSigmaFactor), ctypes.c_float(a.AlphaInterpolation))
    assert rc == 0
    return out


def _r7_plane(host_lib, p, w, h, cam, a):
    proj = np.array(list(cam.mProj), F)
    out = np.zeros((h, w, 4), F)
    rc = host_lib.mifx_host_ssr_bilateral_cleanup(fptr(p["depth"]), fptr(p["normal"]), fptr(p["roughness"]), fptr(p["radiance"]), fptr(p["variance"]), fptr(p["mask"]), fptr(out), w, h,
                                                  fptr(proj), ctypes.c_float(a.RoughnessThreshold), ctypes.c_float(a.BilateralCleanupSpatialSigmaFactor),
                                                  ctypes.c_float(a.AlphaInterpolation), 0)
    assert rc == 0
    return out


def _classes(p, ssr):
    """The three classes of a geometry pixel, as shares of the frame (read from the mask and the plane of the stand-alone R7): each must hold at least 5 %."""
    geom, mask = p["color"][..., 3] > 0, p["mask"] != 0
    shares = {"outside the mask": (geom & ~mask).mean(), "inside, refl.w == 0": (geom & mask & (ssr[..., 3] == 0)).mean(), "inside, refl.w != 0": (geom & mask & (ssr[..., 3] != 0)).mean()}
    assert all(s >= 0.05 for s in shares.values()), shares
    return geom, mask


def test_fused_composite_equals_the_unfused_one_on_a_per_pixel_mask(host_lib):
    from diligentfx_amd import binding as B, synth

    a = B.SSRAttribs.default()
    for seed, (w, h) in enumerate(((96, 64), (67, 37))):
        cam = synth.make_camera(3 + seed, w, h)
        p = _frame(w, h, 700 + seed)
        ssr = _r7_plane(host_lib, p, w, h, cam, a)
        geom, mask = _classes(p, ssr)
        assert not ssr[~mask].any()  # (the stand-alone R7 writes 0 outside the mask: what the fused body must behave like without evaluating anything)
        want = _run(host_lib, p, w, h, cam, a, fused=False, ssr=ssr)
        got = _run(host_lib, p, w, h, cam, a, fused=True)
        assert np.isfinite(want).all()
        assert np.array_equal(got, want), f"{w}x{h}: {(got != want).mean():.2e} of the values differ, max {np.abs(got - want).max():.3e}"
        # and the reflection is in the picture where it should be: a pixel with a reflection differs from colour x AO, a pixel outside the mask does not
        flat = p["color"][..., :3] * (F(1.0) + p["color"][..., 3:] * (p["ssao"][..., None] - F(1.0)))
        assert (got[..., :3] != flat)[geom & mask & (ssr[..., 3] != 0)].any(-1).mean() > 0.5  # (most: a weak reflection can vanish in the rounding of the sum)


@pytest.mark.parametrize("sentinel", [1e30, float("inf"), float("nan")], ids=["1e30", "inf", "nan"])
def test_masked_out_pixels_do_not_consult_the_reflection_inputs(host_lib, sentinel):
    """A sentinel in specular IBL / normal / base colour / material at every pixel outside the mask: the output there is colour x lerp(1, ao, ssaoScale), and every other
    pixel is what it was without the sentinel.  1e30: a finite value that would have to show in a result that used it.  inf / nan: values that an added `x * 0` turns
    into NaN -- a body that evaluated the block and multiplied by the zero reflection fails these two.  (R7's taps read the normal of neighbours inside the mask only -- is_reflection_sample -- so the sentinel normal of a
    masked-out neighbour is not one of them: roughness above the threshold there, as SSR's mask pass would have it.)"""
    from diligentfx_amd import binding as B, synth

    a = B.SSRAttribs.default()
    w, h = 96, 64
    cam = synth.make_camera(5, w, h)
    p = _frame(w, h, 811)
    out_of_mask = p["mask"] == 0
    p["roughness"][out_of_mask] = F(a.RoughnessThreshold) + F(0.1) + p["roughness"][out_of_mask]  # (consistent with the mask: no tap of R7 lands on such a pixel)
    ssr = _r7_plane(host_lib, p, w, h, cam, a)
    geom, mask = _classes(p, ssr)
    clean = _run(host_lib, p, w, h, cam, a, fused=True)
    q = dict(p)
    for name in ("specular_ibl", "normal", "base_color", "material"):
        q[name] = p[name].copy()
        q[name][out_of_mask] = F(sentinel)
    got = _run(host_lib, q, w, h, cam, a, fused=True)
    opacity, ao = p["color"][..., 3], p["ssao"]
    factor = np.where(opacity > 0, F(1.0) + (F(1.0) * opacity) * (ao - F(1.0)), F(1.0)).astype(F)  # lerpf(1, ao, ssaoScale) = 1 + ssaoScale * (ao - 1); ssaoScale = 1 x opacity
    want = (p["color"][..., :3] * factor[..., None]).astype(F)
    assert np.array_equal(got[out_of_mask][:, :3], want[out_of_mask])
    assert np.array_equal(got[..., 3], opacity)
    assert np.array_equal(got[mask], clean[mask]) and np.array_equal(got, clean)
    assert (clean[..., :3] != want)[geom & mask & (ssr[..., 3] != 0)].any(-1).mean() > 0.5  # (not a frame on which the block does nothing anywhere)
