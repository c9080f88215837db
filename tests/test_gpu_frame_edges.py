"""Every pass at the boundary frame sizes, against the same checker and at the same tolerance as its own test: the smallest frame the library accepts, thin
frames (1xN, Nx1, 2xN, 3x97, 97x3), sizes whose pyramid levels are all odd (2^k + 1), and sizes where one pyramid dimension reaches 1 long before the other.
These are where the tiled paths of the kernels (8x8 wave tiles, LDS halo tiles, the fused pyramid levels, the single-workgroup tails, the work-list resolve,
the one-launch jump flood) meet partial tiles and 1-texel levels.  Each comparison reads back the intermediate levels its own test reads, at their collapsed sizes.

Non-finite values: util.assert_close counts a texel whose NaN-ness differs from the checker's, or an infinity where the checker has a finite value, as a mismatch,
so wherever the checker produces a non-finite value the product must produce one at the same texel.

One size just below each pass' minimum must be refused with INVALID_ARG before anything is launched (size checks: mifx_core.cpp to_img, mifx_postfx_prepare,
api_ssao.cpp / api_ssr.cpp half resolution, api_bloom_taa.cpp Bloom, api_dof.cpp)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_pbr import ibl_np  # noqa: F401 -- (the module-scoped fixture of the shade's own test)
from util import assert_close, blue_noise_tables, to_np

pytestmark = pytest.mark.gpu

THIN = [(1, 1), (1, 9), (9, 1), (2, 7), (7, 2), (3, 97), (97, 3)]
ODD = [(33, 17), (65, 9), (129, 65)]  # 2^k + 1: every level of the pyramids has an odd size
COLLAPSE = [(300, 12)]  # the height reaches one texel four levels before the width

# (entry point of include/mifx.h, what runs it here): the coverage guard tests/test_frame_edges_coverage.py reads this table
SIZE_MATRIX = {
    "mifx_postfx_execute": "test_prep_edges",
    "mifx_ssao_execute": "test_ssao_edges, test_ssao_half_resolution_edges",
    "mifx_ssr_execute": "test_ssr_edges, test_ssr_half_resolution_edges",
    "mifx_taa_execute": "test_taa_edges",
    "mifx_bloom_execute": "test_bloom_edges",
    "mifx_dof_execute": "test_dof_edges",
    "mifx_pbr_shade_execute": "test_pbr_shade_edges",
    "mifx_composite_execute": "test_composite_edges",
    "mifx_composite_execute_selection": "test_selection_composite_edges",
    "mifx_selection_execute": "test_jump_flood_edges",
    "mifx_autoexposure_execute": "test_autoexposure_edges",
    "mifx_tonemap_execute": "test_tonemap_edges",
    "mifx_tonemap_execute_auto": "test_tonemap_edges",
    "mifx_chain_execute": "test_chain_edges",
}


def _ssao():
    import test_gpu_ssao

    return test_gpu_ssao


def _ssr():
    import test_gpu_ssr

    return test_gpu_ssr


@pytest.mark.parametrize("size", THIN + ODD + COLLAPSE)
def test_ssao_edges(mifx_lib, size):
    """GTAO at full resolution (smallest frame 1x1), the fused resolve; A2 / A6 levels compared at their collapsed sizes."""
    _ssao().ssao_per_pass(size, "gtao", False, False, True, frames=2, edge=True)


@pytest.mark.parametrize("size,algo,rev,fused", [((1, 1), "hbao", False, True), ((33, 17), "hbao", False, True), ((1, 1), "vbao", False, True),
                                                 ((65, 9), "vbao", False, True), ((3, 97), "gtao", True, True), ((97, 3), "gtao", False, False)])
def test_ssao_variants_edges(mifx_lib, size, algo, rev, fused):
    _ssao().ssao_per_pass(size, algo, rev, False, fused, frames=2, edge=True)


@pytest.mark.parametrize("size", [(32, 32), (33, 65), (65, 33), (300, 32)])
def test_ssao_half_resolution_edges(mifx_lib, size):
    """FEATURE_FLAG_HALF_RESOLUTION from its smallest frame (32x32: a 16x16 pyramid base) on."""
    _ssao().ssao_half_resolution(size, "gtao", 0, frames=2, edge=True)


@pytest.mark.parametrize("size", THIN + ODD + COLLAPSE)
def test_ssr_edges(mifx_lib, size):
    """Hi-Z levels 1 .. 6 (bit-exact) and R2 .. R7 at full resolution, smallest frame 1x1."""
    _ssr().ssr_per_pass(size, 0, 0, False, frames=2, edge=True)


@pytest.mark.parametrize("size,mdm,flags,rev", [((1, 9), 1, 0, False), ((33, 17), 0, 1, False), ((97, 3), 0, 0, True)])
def test_ssr_variants_edges(mifx_lib, size, mdm, flags, rev):
    _ssr().ssr_per_pass(size, mdm, flags, rev, frames=2, edge=True)


@pytest.mark.parametrize("size", [(4, 4), (5, 97), (33, 17), (300, 12)])
def test_ssr_half_resolution_edges(mifx_lib, size):
    """FEATURE_FLAG_HALF_RESOLUTION from its smallest frame (4x4: a 2x2 ray pass) on."""
    _ssr().ssr_half_resolution(size, frames=2, edge=True)


@pytest.mark.parametrize("size,flags", [((1, 1), 0), ((1, 9), 7), ((9, 1), 2), ((3, 97), 5), ((97, 3), 0), ((33, 17), 7), ((8, 8), 3)])
def test_taa_edges(mifx_lib, size, flags):
    import test_gpu_bloom_taa

    test_gpu_bloom_taa.taa_multi_frame(flags, size)


@pytest.mark.parametrize("size,radius", [((8, 8), 1.0), ((8, 8), 0.75), ((8, 97), 1.0), ((97, 8), 1.0), ((33, 17), 1.0), ((65, 9), 1.0), ((129, 65), 1.0),
                                         ((520, 9), 1.0), ((9, 520), 0.75)])
def test_bloom_edges(mifx_lib, size, radius):
    """Bloom from its smallest frame (8x8: a 4x4 first level) on; every level down and up compared, the tail kernel against one launch per level (bit for bit)."""
    import test_gpu_bloom_taa

    test_gpu_bloom_taa.test_bloom_per_pass_and_output(mifx_lib, size, radius)


@pytest.mark.parametrize("size,flags", [((16, 16), 3), ((16, 16), 0), ((17, 33), 1), ((33, 17), 2), ((97, 16), 3)])
def test_dof_edges(mifx_lib, size, flags):
    """Depth of field from its smallest frame (16x16: three dilation levels of 8x8, 4x4, 2x2) on; every pass compared."""
    import test_gpu_dof

    test_gpu_dof.dof_per_pass_and_output(size, flags, (2, 2), frames=(7, 8), edge=True)


@pytest.mark.parametrize("size", THIN + [(33, 17)])
def test_pbr_shade_edges(mifx_lib, ibl_np, size):  # noqa: F811
    import test_gpu_pbr

    test_gpu_pbr.pbr_shade(ibl_np, size, True, edge=True)


@pytest.mark.parametrize("size", THIN + [(33, 17)])
def test_composite_edges(mifx_lib, ibl_np, size):  # noqa: F811
    import test_gpu_pbr

    test_gpu_pbr.composite(ibl_np, 4, size)


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (3, 97), (97, 3), (33, 17)])
def test_selection_composite_edges(mifx_lib, size):
    import test_gpu_selection

    test_gpu_selection.selection_composite(4, size, edge=True)


@pytest.mark.parametrize("size", THIN + ODD + [(300, 12)])
@pytest.mark.parametrize("max_distance", [4.0, 16.0])
def test_jump_flood_edges(mifx_lib, size, max_distance):
    """The one-launch jump flood (7-texel LDS halo) on frames smaller than its halo and its 32x16 tile: bit-exact against the restatement."""
    import selection_util as S
    import test_gpu_selection

    w, h = size
    got, sel = test_gpu_selection._jump_flood_plane(w, h, max_distance, w + h)
    want = S.jump_flood(sel, 1.0, max_distance)
    assert got.shape == want.shape == (h, w, 2)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())
    assert bad == 0, f"{bad} texels differ"


@pytest.mark.parametrize("size", THIN + ODD + COLLAPSE)
def test_autoexposure_edges(mifx_lib, size):
    import test_gpu_autoexposure

    test_gpu_autoexposure.test_autoexposure_parity(mifx_lib, size)


@pytest.mark.parametrize("size", THIN + [(33, 17), (65, 9)])
def test_prep_edges(mifx_lib, oracle, size):
    """Reprojected depth and closest motion (3x3 neighbourhood, clamped at the frame's edges) on frames down to 1x1."""
    import test_gpu_tonemap_prep
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    ctx = api.PostFXContext(0, sobol, tile)
    test_gpu_tonemap_prep.test_prep_passes(ctx, oracle, size)
    ctx.close()


@pytest.mark.parametrize("size", THIN + [(33, 17)])
def test_tonemap_edges(mifx_lib, oracle, size):
    """ToneMap() on frames down to 1x1 (its 64x4 block), with the host average and with the auto-exposure plane's."""
    import test_gpu_tonemap_prep
    from diligentfx_amd import api, binding as B, synth

    w, h = size
    ctx = api.PostFXContext(0)
    hdr = synth.make_hdr_buffer(w, h, ctx.device)
    for mode in (4, 8):
        attr = B.ToneMappingAttribs.default(mode)
        got = to_np(ctx.tone_map(hdr, attr, 0.3, flags=1))
        for prefix, lib in test_gpu_tonemap_prep.checkers(oracle):
            want = np.zeros_like(got)
            lib.call(prefix + "tonemap", [to_np(hdr)], [want], attribs=bytes(attr), fval=[0.3], ival=[1])
            assert_close(got, want, what=f"tonemap {size} mode {mode} vs {prefix}")
    ae = api.AutoExposure(ctx)
    ae.execute(hdr, 0.0, False)
    tm = B.ToneMappingAttribs.default(4)
    assert torch.equal(ae.tone_map(hdr, tm, flags=1), ctx.tone_map(hdr, tm, ae.average(), flags=1))
    ae.close()
    ctx.close()


@pytest.mark.parametrize("size", [(8, 8), (33, 17)])
def test_chain_edges(mifx_lib, size):
    """The chain with its default effects at the smallest frame it accepts (Bloom's 8x8) and at 33x17: four frames against the CPU chain at the budgets of
    tests/test_gpu_chain.py::test_chain_vs_cpu_chain."""
    import test_gpu_chain

    test_gpu_chain.chain_vs_cpu_chain(size, frames=4)


# ---- one size below the minimum: INVALID_ARG, nothing launched


def _narrow(t):
    """A descriptor of `t` with no columns (a valid pointer and pitch): one below every 1x1 minimum."""
    from diligentfx_amd import binding as B

    d = B.image(t)
    d.width = 0
    return d


def _invalid_arg(status):
    from diligentfx_amd import binding as B

    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        B.check(status)


def test_sizes_below_the_minimum_are_refused(mifx_lib):
    from diligentfx_amd import api, binding as B, synth

    sobol, tile = blue_noise_tables()
    ctx = api.PostFXContext(0, sobol, tile)
    dev = ctx.device
    # a frame without columns or rows: prep, SSAO, SSR, TAA (all prepared through the context)
    for w, h in ((0, 8), (8, 0)):
        with pytest.raises(B.MifxError, match="INVALID_ARG"):
            ctx.prepare_resources(0, w, h)
    # the effects with their own minimum
    for fx_cls, flags, sizes in ((api.Bloom, 0, ((7, 8), (8, 7))), (api.DepthOfField, 0, ((15, 16), (16, 15))),
                                 (api.ScreenSpaceAmbientOcclusion, 2, ((31, 32), (32, 31))), (api.ScreenSpaceReflection, 2, ((3, 4), (4, 3)))):
        for w, h in sizes:
            ctx.prepare_resources(0, w, h)
            fx = fx_cls(ctx)
            with pytest.raises(B.MifxError, match="INVALID_ARG"):
                fx.prepare_resources(flags)
            fx.close()
    # the stand-alone passes take an image with no columns as INVALID_ARG (mifx_core.cpp to_img)
    hdr = synth.make_hdr_buffer(8, 8, dev)
    attr = B.ToneMappingAttribs.default(4)
    i, o = _narrow(hdr), _narrow(torch.zeros_like(hdr))
    _invalid_arg(mifx_lib.mifx_tonemap_execute(ctx.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(attr), ctypes.c_float(0.3), ctypes.c_uint32(0)))
    ae = api.AutoExposure(ctx)
    _invalid_arg(mifx_lib.mifx_autoexposure_execute(ae.handle, ctypes.byref(i), ctypes.c_float(0.0), ctypes.c_int32(0)))
    ae.close()
    sel = api.ProcessSelection(ctx)
    d = _narrow(torch.ones(8, 8, device=dev))
    _invalid_arg(mifx_lib.mifx_selection_execute(sel.handle, ctypes.byref(d), ctypes.byref(B.SelectionAttribs.default(selection_id=1))))
    sel.close()
    f = synth.make_frame(synth.Scene(), 0, 8, 8, dev)
    lut = torch.zeros(8, 8, 2, device=dev)
    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        api.composite(ctx, hdr, hdr, hdr, torch.ones(8, 8, device=dev), f["normal"], f["base_color"], f["material"], lut, f["camera"], out=torch.zeros(8, 8, 4, device=dev)[:, :0])
    # the chain: below Bloom's 8x8
    import chain_util

    chain = api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(chain.postfx, synth.make_sky_cube(16, dev), lut_size=16, irradiance_size=4, prefiltered_size=8, lut_samples=16, diffuse_samples=16,
                             specular_samples=8)
    sa = chain_util.shade_attribs(len(ibl.pre) - 1)
    g = synth.make_frame(synth.Scene(), 0, 7, 8, dev)
    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        chain.execute(chain.bind_frame(0, g, ibl, sa, torch.zeros(8, 7, 4, device=dev)))
    torch.cuda.synchronize()
    chain.close()
    ctx.close()
