"""GPU parity of the material fetch (mifx_pbr_material_fetch) against tests/golden/material_fetch_golden.npz: the head of the reference's pixel shader, compiled per permutation
from the reference's text with the sampler and the quad derivatives of include/mifx.h around it (tests/golden/make_golden_material_fetch.py).  The generator asserts that the
reference's own strict and contracted builds agree within 0.5e-3 on every stored value, so util.assert_close at its defaults with no outlier is the bar here."""
import numpy as np
import pytest
import torch

import material_fetch_util as M
from util import assert_close, to_np

pytestmark = pytest.mark.gpu
CASES = M.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def golden():
    return M.load_golden()[0]


def device_inputs(c, device):
    from diligentfx_amd import api, binding as B

    textures = [api.TextureArray(t, device) for t in c["textures"]]
    materials = [B.PBRMaterial.from_buffer_copy(M.material_words(m).tobytes()) for m in c["materials"]]
    interp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in c["interp"].items()}
    return interp, materials, textures


def caller_planes(c, device, fill=None):
    """Every output plane of the case's call holding `fill` (default: the sentinel), split into the G-buffer's and the layers'"""
    blank = M.blank_outputs(c)
    if fill is not None:
        for n, p in blank.items():
            p[...] = np.asarray(fill[n], np.float32)
    t = {n: torch.from_numpy(p).to(device) for n, p in blank.items()}
    g = {n: t[n] for n, _ in M.GBUFFER_OUT}
    return g, {n: v for n, v in t.items() if n not in g}


def fetch(ctx, c, place=lambda t, output=False: t, fill=None):
    """The case through api.pbr_material_fetch into caller planes that hold the sentinel (or `fill`); place: how a plane is laid out (tests/test_gpu_plane_layouts.py)"""
    from diligentfx_amd import api, binding as B

    interp, mats, textures = device_inputs(c, ctx.device)
    g, ly = caller_planes(c, ctx.device, fill)
    interp = {k: place(v) for k, v in interp.items()}
    g, ly = ({k: place(v, output=fill is None) for k, v in d.items()} for d in (g, ly))
    out_g, out_l = api.pbr_material_fetch(ctx, interp, mats, textures, B.camera_from_bytes(c["camera"].tobytes()), layer_flags=c["layers"], flags=c["flags"], mip_bias=c["mip_bias"],
                                          gbuffer=g, layers=ly)
    torch.cuda.synchronize()
    return out_g, out_l


def make_ctx(c):
    from diligentfx_amd import api
    from util import blue_noise_tables

    ctx = api.PostFXContext(0, *blue_noise_tables())
    if c["reversed"]:  # (the far plane is depth 0: the context's convention, as for the shade)
        h, w = c["interp"]["depth"].shape
        ctx.prepare_resources(0, w, h, feature_flags=ctx.FEATURE_FLAG_REVERSED_DEPTH)
    return ctx


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_material_fetch_against_the_fixture(mifx_lib, golden, c):
    """Every fixture case through api.pbr_material_fetch; a pixel without a fragment keeps the sentinel in every output plane, bit for bit"""
    ctx = make_ctx(c)
    g, ly = fetch(ctx, c)
    frag = M.has_fragment(c)
    got = {**{k: v for k, v in g.items() if k != "depth"}, **ly}
    assert set(got) == set(M.output_names(c))
    for name, t in got.items():
        a = to_np(t)
        want = M.expected_plane(golden[c["name"]], name, M.channels_of(name))
        assert np.array_equal(a[~frag].view(np.uint32), np.full_like(a[~frag], M.SENTINEL).view(np.uint32)), f"{c['name']}, {name}: a pixel without a fragment was stored"
        assert np.isfinite(a).all()
        assert_close(a[frag], want[frag], max_outlier_frac=0.0, what=f"{c['name']}, {name}")
    ctx.close()


def test_pitched_and_offset_planes_equal_the_packed_run(mifx_lib):
    """Case (l) with every plane pitched and offset (the layouts of tests/test_gpu_plane_layouts.py): equal to the packed run bit for bit, nothing outside a view written"""
    from test_gpu_plane_layouts import Layout, _bits

    c = BY_NAME["l_every_layer"]
    ctx = make_ctx(c)
    results = {}
    for kind in ("a", "b", "c"):
        lay = Layout(kind)
        g, ly = fetch(ctx, c, place=lay)
        results[kind] = {k: _bits(v) for k, v in {**g, **ly}.items() if k != "depth"}
        lay.check()
    assert set(results["a"]) == set(M.ALL_OUTPUTS)
    for kind in ("b", "c"):
        for name, want in results["a"].items():
            assert np.array_equal(results[kind][name], want), f"layout {kind}: {name} differs from the contiguous run"
    ctx.close()


@pytest.mark.parametrize("name", sorted(M.SHADED))
def test_fetch_then_shade_against_the_reference_radiance(mifx_lib, golden, name):
    """Cases (v): the fetch, then mifx_pbr_shade_execute_layers on the device, against what the reference's shade makes of the reference-fetched planes (two lights, the IBL of
    the layers fixture), at the tolerance tests/test_gpu_pbr_layers.py uses for that shade"""
    from diligentfx_amd import api, binding as B
    from layers_util import BACKGROUND
    from test_gpu_pbr_layers import ibl_to_device

    c = BY_NAME[name]
    ctx = make_ctx(c)
    ibl_np, albedo, charlie, sa = M.shade_setup()
    g, ly = fetch(ctx, c, fill=M.CALLER)
    if c["layers"] & B.PBR_LAYER_SHEEN:
        ly["sheen_albedo_scaling_lut"] = torch.from_numpy(albedo).to(ctx.device)
        ly["preintegrated_charlie"] = torch.from_numpy(np.repeat(charlie[..., None], 4, -1).copy()).to(ctx.device)
    rad, spec = api.pbr_shade_layers(ctx, g, ly, c["layers"], B.camera_from_bytes(c["camera"].tobytes()), sa, ibl_to_device(ibl_np, ctx.device), background=BACKGROUND,
                                     iridescence_ior=M.IOR, anisotropy_rotation=M.ROTATION)
    want, want_spec = (np.moveaxis(golden[name][k], 0, -1) for k in ("shaded_radiance", "shaded_specular_ibl"))
    assert np.isfinite(to_np(rad)).all()
    assert_close(to_np(rad), want, max_outlier_frac=0.0, what=f"{name}: radiance of the fetched planes")
    assert_close(to_np(spec), want_spec, max_outlier_frac=0.0, what=f"{name}: specular IBL of the fetched planes")
    ctx.close()


def test_a_layer_that_is_off_leaves_its_plane_untouched(mifx_lib):
    """Case (l) with only clear coat and transmission on: the other layers' planes are not even bound, and bound but off they keep the sentinel"""
    from diligentfx_amd import api, binding as B

    c = BY_NAME["l_every_layer"]
    ctx = make_ctx(c)
    full_g, full_l = fetch(ctx, c)
    on = B.PBR_LAYER_CLEAR_COAT | B.PBR_LAYER_TRANSMISSION
    interp, mats, textures = device_inputs(c, ctx.device)
    g, ly = caller_planes(c, ctx.device)
    cam = B.camera_from_bytes(c["camera"].tobytes())
    api.pbr_material_fetch(ctx, interp, mats, textures, cam, layer_flags=on, flags=c["flags"], mip_bias=c["mip_bias"], gbuffer=g, layers=ly)
    torch.cuda.synchronize()
    for name in ("sheen", "anisotropy", "iridescence"):
        assert bool((ly[name] == float(M.SENTINEL)).all()), name
    for name in ("clearcoat", "clearcoat_normal", "transmission"):
        assert torch.equal(ly[name], full_l[name]), name
    for name in ("base_color", "normal", "material", "emissive", "occlusion"):
        assert torch.equal(g[name], full_g[name]), name
    ctx.close()


def test_texture_index_minus_one_equals_the_run_without_the_map(mifx_lib):
    """texture[slot] = -1 is the permutation without that USE_*_MAP: bit for bit the run of a material that never had the map (whatever the slot's attribs hold)"""
    import copy

    c = BY_NAME["d_two_uv_sets"]
    ctx = make_ctx(c)
    without = copy.deepcopy(c)
    for slot in ("OCCLUSION", "PHYS_DESC"):
        del without["materials"][0]["maps"][slot]
    minus_one = copy.deepcopy(c)
    for slot in ("OCCLUSION", "PHYS_DESC"):
        t, a = minus_one["materials"][0]["maps"][slot]
        minus_one["materials"][0]["maps"][slot] = (-1, a)  # the attribs stay, the binding goes
    (ga, _), (gb, _), (gc, _) = fetch(ctx, without), fetch(ctx, minus_one), fetch(ctx, c)
    for name in ("base_color", "normal", "material", "emissive", "occlusion"):
        assert torch.equal(ga[name].view(torch.int32), gb[name].view(torch.int32)), name
    assert not torch.equal(gc["occlusion"], ga["occlusion"]) and not torch.equal(gc["material"], ga["material"])  # (the maps were in the picture)
    ctx.close()


def test_refusals_reach_python_with_a_message(mifx_lib):
    from diligentfx_amd import api, binding as B

    c = BY_NAME["a_minified"]
    ctx = make_ctx(c)
    interp, mats, textures = device_inputs(c, ctx.device)
    cam = B.camera_from_bytes(c["camera"].tobytes())
    mats[0].texture[B.PBR_TEXTURE_BASE_COLOR] = len(textures)
    with pytest.raises(B.MifxError, match="outside the texture table"):
        api.pbr_material_fetch(ctx, interp, mats, textures, cam)
    ctx.close()


# the same tables twice, other and larger tables, the first again, a 1x1 frame (tests/cpu_product/run.py material_fetch runs the same sequence on the host code alone)
SEQUENCE = ("a_minified", "a_minified", "o_three_materials", "m_every_layer_rgba8", "a_minified", "p_frame_1x1")


def test_one_context_serves_calls_with_different_tables(mifx_lib):
    """SEQUENCE on one context, every call into output planes of its own, queued without a host synchronisation in between (the entry itself waits for the stream before it
    overwrites the tables a call queued earlier may still read) and one at the end: each call's planes equal the same case on a fresh context bit for bit -- the same kernel
    on the same inputs, so the tables the context holds are all that could differ"""
    from diligentfx_amd import api, binding as B

    ctx = make_ctx(BY_NAME[SEQUENCE[0]])
    inputs = {n: device_inputs(BY_NAME[n], ctx.device) for n in set(SEQUENCE)}  # (made once a case: a repeated case hands the entry the very same tables)
    planes = [caller_planes(BY_NAME[n], ctx.device) for n in SEQUENCE]
    got = []
    for n, (g, ly) in zip(SEQUENCE, planes):
        c = BY_NAME[n]
        interp, mats, textures = inputs[n]
        got.append(api.pbr_material_fetch(ctx, interp, mats, textures, B.camera_from_bytes(c["camera"].tobytes()), layer_flags=c["layers"], flags=c["flags"], mip_bias=c["mip_bias"],
                                          gbuffer=g, layers=ly))
    torch.cuda.synchronize()
    want = {}
    for n in set(SEQUENCE):
        fresh = make_ctx(BY_NAME[n])
        want[n] = fetch(fresh, BY_NAME[n])
        fresh.close()
    for step, (n, (g, ly)) in enumerate(zip(SEQUENCE, got)):
        wg, wl = want[n]
        assert set(g) == set(wg) and set(ly) == set(wl) and set(g) | set(ly) == set(M.output_names(BY_NAME[n])) | {"depth"}
        for name, t in {**g, **ly}.items():
            if name != "depth":
                assert torch.equal(t.view(torch.int32), {**wg, **wl}[name].view(torch.int32)), f"call {step} ({n}): {name} differs from the run on a fresh context"
    ctx.close()
