"""GPU parity of Bloom (B1-B3) and TemporalAntiAliasing (T1), per pass and end to end, plus the host-side jitter helpers."""
import numpy as np
import pytest
import torch

import cpu_chain
from util import assert_close, blue_noise_tables, centre_tap_slack, to_np

pytestmark = pytest.mark.gpu


def checker(symbol):
    import pyref

    r = pyref.ref_lib()
    if r is not None:
        return r, "ref_"
    o = pyref.oracle_lib()
    if not o.has("oracle_" + symbol):
        pytest.skip("no checker available for " + symbol)
    return o, "oracle_"


def hdr_scene(w, h, device, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = torch.rand(h, w, 4, generator=g) * 0.8
    img[..., :3] *= torch.exp2(torch.rand(h, w, 1, generator=g) * 6 - 3)  # some pixels above the bloom threshold
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    img[..., :3] += 40.0 * torch.exp(-((xx - w * 0.3) ** 2 + (yy - h * 0.6) ** 2) / 18.0)[..., None]  # a hot spot
    return img.contiguous().to(device)


@pytest.mark.parametrize("size,radius", [((256, 144), 0.75), ((202, 118), 0.75), ((64, 40), 0.75), ((176, 104), 1.0), ((70, 36), 1.0), ((256, 144), 1.0)])
def test_bloom_per_pass_and_output(mifx_lib, size, radius):
    """Radius 1.0 runs the whole pyramid: 176x104 ends in 5x3 / 2x1 / 1x1, 70x36 in 4x2 / 2x1 / 1x1 after odd levels (35x18, 17x9, 8x4), 256x144 in 2x1 / 1x1."""
    from diligentfx_amd import api, binding as B

    lib, pfx = checker("bloom_prefilter")
    w, h = size
    ctx = api.PostFXContext(0)
    ctx.prepare_resources(0, w, h)
    bloom = api.Bloom(ctx)
    bloom.prepare_resources()
    color = hdr_scene(w, h, ctx.device)
    attribs = B.BloomAttribs.default()
    attribs.AlphaInterpolation = 0.85
    attribs.Radius = radius
    bloom.execute(color, attribs)
    got = to_np(bloom.get_bloom_texture())
    keep = {}
    want = cpu_chain.CpuChain(lib, pfx).bloom(to_np(color), attribs, keep)
    # the test image has an 80:1 hot spot; bilinear taps that fall exactly on texel centres / midpoints have fp32 weight errors of ~1e-5,
    # which that contrast amplifies to ~1e-3 on a few texels next to the spot: bounded by the derived centre-tap allowance where the pass has
    # one, by a small outlier budget with a cap on the outlier size elsewhere
    assert len(keep["bloom_down"]) == int(np.float32(radius) * np.float32(cpu_chain.compute_mip_levels_count(w // 2, h // 2)))
    for i, d in enumerate(keep["bloom_down"]):
        assert_close(to_np(bloom.get_intermediate(f"down{i}")), d, max_outlier_frac=0.0, what=f"down{i}")
    for i, u in enumerate(keep["bloom_up"]):
        assert_close(to_np(bloom.get_intermediate(f"up{i}")), u, max_outlier_frac=0.0, what=f"up{i}", abs_slack=centre_tap_slack(keep["bloom_down"][i]))
    assert_close(got, want, max_outlier_frac=0.0, what="bloom output", abs_slack=centre_tap_slack(to_np(color)))
    assert np.array_equal(got[..., 3], to_np(color)[..., 3])
    assert (got[..., :3] >= to_np(color)[..., :3] - 1e-4).all()  # bloom only adds light
    # the small levels are taken down and up again by one workgroup (launch_bloom_tail): bit-identical to one dispatch per level
    levels = {f"down{i}": to_np(bloom.get_intermediate(f"down{i}")).copy() for i in range(len(keep["bloom_down"]))}
    levels.update({f"up{i}": to_np(bloom.get_intermediate(f"up{i}")).copy() for i in range(len(keep["bloom_up"]))})
    B.check(mifx_lib.mifx_debug_bloom_set_tail(bloom.handle, 0))
    bloom.execute(color, attribs)
    assert np.array_equal(to_np(bloom.get_bloom_texture()), got)
    for name, plane in levels.items():
        assert np.array_equal(to_np(bloom.get_intermediate(name)), plane), name
    B.check(mifx_lib.mifx_debug_bloom_set_tail(bloom.handle, 1))
    # property at an arbitrary size: AlphaInterpolation = 0 returns the input colour
    attribs.AlphaInterpolation = 0.0
    bloom.execute(color, attribs)
    # (the source is fetched through the bilinear sampler at the texel centre, whose fp32 weights are 1 - O(1e-5), not exactly 1)
    assert_close(to_np(bloom.get_bloom_texture())[..., :3], to_np(color)[..., :3], rtol=1e-2, what="alpha 0")
    attribs.Radius = 0.1 if radius < 1.0 else 0.05
    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        bloom.execute(color, attribs)
    bloom.close()
    ctx.close()


def test_bloom_temporal_upscaling_output_size(mifx_lib):
    """PostFXContext::FEATURE_FLAG_TEMPORAL_UPSCALING (PostFXContext.hpp:56): Bloom sizes its pyramid and output from FrameDesc.OutputWidth x OutputHeight
    (Bloom.cpp:84-85) -- the render size stays with the passes in front of the up-scaler.  Against the checker run at the output size."""
    from diligentfx_amd import api, binding as B

    lib, pfx = checker("bloom_prefilter")
    w, h, ow, oh = 128, 72, 256, 144
    ctx = api.PostFXContext(0)
    ctx.prepare_resources(0, w, h, api.PostFXContext.FEATURE_FLAG_TEMPORAL_UPSCALING, ow, oh)
    bloom = api.Bloom(ctx)
    bloom.prepare_resources()
    color = hdr_scene(ow, oh, ctx.device)
    attribs = B.BloomAttribs.default()
    bloom.execute(color, attribs)
    got = to_np(bloom.get_bloom_texture())
    assert got.shape == (oh, ow, 4) and to_np(bloom.get_intermediate("down0")).shape == (oh // 2, ow // 2, 4)
    want = cpu_chain.CpuChain(lib, pfx).bloom(to_np(color), attribs)
    assert_close(got, want, max_outlier_frac=0.0, what="bloom at the output size", abs_slack=centre_tap_slack(to_np(color)))
    with pytest.raises(B.MifxError, match="INVALID_ARG"):  # the input has to be at the output size
        bloom.execute(hdr_scene(w, h, ctx.device), attribs)
    # without the flag the same context sizes the effect from Width x Height; with the flag but no output size the context refuses
    ctx.prepare_resources(1, w, h)
    bloom.prepare_resources()
    bloom.execute(hdr_scene(w, h, ctx.device), attribs)
    assert to_np(bloom.get_bloom_texture()).shape == (h, w, 4)
    frame = B.FrameDesc(2, w, h, 0, 0)
    import ctypes

    assert mifx_lib.mifx_postfx_prepare(ctx.handle, ctypes.byref(frame), 4) == -1
    bloom.close()
    ctx.close()


@pytest.mark.parametrize("flags", list(range(8)))
def test_taa_multi_frame(mifx_lib, flags):
    taa_multi_frame(flags)


def taa_multi_frame(flags, size=(176, 100), attribs=None):
    """Five frames; each frame's HIP output is compared with the checker fed with the HIP history (per-pass isolation),
    and the checker's independent history is compared end to end.  attribs: a TAAAttribs block other than the default (tests/test_gpu_attribute_sweeps.py).
    Returns the worst relative error of the isolated and of the end-to-end comparison."""
    from diligentfx_amd import api, binding as B, synth

    lib, pfx = checker(f"taa_flags{flags}")
    w, h = size
    sobol, tile = blue_noise_tables()
    ctx = api.PostFXContext(0, sobol, tile)
    taa = api.TemporalAntiAliasing(ctx)
    chain = cpu_chain.CpuChain(lib, pfx, taa_flags=flags)
    scene = synth.Scene()
    attribs = attribs if attribs is not None else B.TAAAttribs.default()
    prev_hist = np.zeros((h, w, 4), np.float32)
    worst = [0.0, 0.0]
    for frame in range(5):
        f = synth.make_frame(scene, frame, w, h, ctx.device)
        color = torch.cat([f["base_color"][..., :3] * 2.0 + 0.05 * f["normal"][..., :3].abs(), f["base_color"][..., 3:4]], -1).contiguous()
        ctx.prepare_resources(frame, w, h)
        taa.prepare_resources(flags)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        st = taa.execute(color, attribs)
        assert st == (1 if frame == 0 else 0)
        got = to_np(taa.get_accumulated_frame())
        a = B.TAAAttribs.from_buffer_copy(bytes(attribs))
        a.ResetAccumulation = 0
        want = np.zeros((h, w, 4), np.float32)
        if frame == 0:
            # the first frame of a flag set is the reference's placeholder: the colour copied into the accumulation buffer, alpha included
            # (TemporalAntiAliasing.cpp:161-171, 191-198, 302-311; tests/test_host_sequence_vs_ref.py::test_taa_first_frame_of_a_flag_set_is_a_copy)
            want = to_np(color).copy()
            assert np.array_equal(got, want)
        else:
            lib.call(pfx + f"taa_flags{flags}", [to_np(color), prev_hist, to_np(ctx.get_closest_motion_vectors()), to_np(ctx.get_reprojected_depth()), to_np(f["prev_depth"])],
                     [want], cam0=bytes(f["camera"]), cam1=bytes(f["prev_camera"]), attribs=bytes(a))
        # disocclusion / inside-screen tests are thresholds on computed values => a few pixels may flip
        worst[0] = max(worst[0], assert_close(got, want, max_outlier_frac=0.0, what=f"TAA flags {flags} frame {frame} (isolated)")[0])
        pf = chain.postfx(frame, to_np(f["depth"]), to_np(f["prev_depth"]), to_np(f["motion"]), bytes(f["camera"]), bytes(f["prev_camera"]), (sobol, tile))
        e2e = chain.taa(pf, to_np(color), attribs)
        worst[1] = max(worst[1], assert_close(got, e2e, max_outlier_frac=0.0, what=f"TAA flags {flags} frame {frame} (end to end)")[0])
        if frame > 0:
            assert torch.equal(taa.get_accumulated_frame(is_prev_frame=True), torch.from_numpy(prev_hist).to(ctx.device))
        prev_hist = got.copy()
        assert np.isfinite(got).all()
    taa.close()
    ctx.close()
    return tuple(worst)


def test_taa_history_imported_into_a_fresh_object(mifx_lib):
    """mifx_taa_import_history into an object that has never executed a frame: the next execute continues the accumulation as if the object had run the imported frame
    (include/mifx.h) -- it must not take the placeholder copy a flag set's first frame takes, which would overwrite the import (round 4 did).  create, prepare, import,
    prepare, execute equals the object that ran all frames, bit for bit."""
    from diligentfx_amd import api, binding as B, synth

    flags, w, h = 2, 176, 100
    sobol, tile = blue_noise_tables()
    scene = synth.Scene()
    attribs = B.TAAAttribs.default()

    def colour(f):
        return torch.cat([f["base_color"][..., :3] * 2.0 + 0.05 * f["normal"][..., :3].abs(), f["base_color"][..., 3:4]], -1).contiguous()

    def step(ctx, taa, frame):
        f = synth.make_frame(scene, frame, w, h, ctx.device)
        ctx.prepare_resources(frame, w, h)
        taa.prepare_resources(flags)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        return taa.execute(colour(f), attribs)

    ctx_a = api.PostFXContext(0, sobol, tile)
    a = api.TemporalAntiAliasing(ctx_a)
    for frame in range(4):
        step(ctx_a, a, frame)
    hist, idx = a.export_history()
    assert idx == 3
    assert step(ctx_a, a, 4) == 0
    want = a.get_accumulated_frame().clone()

    ctx_b = api.PostFXContext(0, sobol, tile)
    b = api.TemporalAntiAliasing(ctx_b)
    ctx_b.prepare_resources(4, w, h)
    b.prepare_resources(flags)  # (the planes take the prepared size)
    b.import_history(hist, idx)
    assert step(ctx_b, b, 4) == 0, "the frame after an import has its history"
    assert torch.equal(b.get_accumulated_frame(), want)
    for o in (a, b, ctx_a, ctx_b):
        o.close()


def test_taa_jitter_helpers(mifx_lib):
    import ctypes

    from diligentfx_amd import api, synth

    for frame in (0, 1, 7, 15, 16, 33):
        jx, jy = api.TemporalAntiAliasing.get_jitter_offset(frame, 1920, 1080)
        ex, ey = synth.taa_jitter(frame, 1920, 1080)
        assert abs(jx - ex) < 1e-9 and abs(jy - ey) < 1e-9
        assert abs(jx) <= 1.0 / 1920 + 1e-9 and abs(jy) <= 1.0 / 1080 + 1e-9  # +-0.5 px in NDC units
    assert api.TemporalAntiAliasing.get_jitter_offset(5, 0, 0) == (0.0, 0.0)
    proj = (ctypes.c_float * 16)(*[1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1.001, 1, 0, 0, -0.1, 0])
    out = (ctypes.c_float * 16)()
    mifx_lib.mifx_taa_get_jittered_proj_matrix(proj, (ctypes.c_float * 2)(0.25, -0.5), out)
    assert out[8] == 0.25 and out[9] == -0.5 and out[12] == 0.0
    ortho = (ctypes.c_float * 16)(*[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    mifx_lib.mifx_taa_get_jittered_proj_matrix(ortho, (ctypes.c_float * 2)(0.25, -0.5), out)
    assert out[12] == 0.25 and out[13] == -0.5 and out[8] == 0.0
