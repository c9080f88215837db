"""GPU tests of the shade's output stage (mifx_pbr_shade_output): the debug views, in-shader tone mapping, alpha modes, unlit, highlight, loading animation and sRGB output of
RenderPBR.psh `main` behind the layered shade.  At 56 x 36 against tests/golden/shade_output_golden.npz (the reference's shader text compiled per permutation); at 131 x 67
(several blocks both ways, no dimension a multiple of 64, 32, 16 or 4) against the layered shade itself, the numpy restatement that test_shade_output_cpu.py pins to the
fixture, and itself on pitched, offset planes.  Needs neither the reference tree nor oracle/_ref."""
import types

import numpy as np
import pytest
import torch

import shade_output_util as S
from util import assert_close, to_np

pytestmark = pytest.mark.gpu
CASES = S.cases()
BIG = (131, 67)
POISON = -7.7e30


def _env(ctx, G, gn, planes, albedo, charlie, camera, sa, motion, mesh_normal):
    from diligentfx_amd import api

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)  # noqa: E731
    layers = {k: t(v) for k, v in planes.items()}
    layers["transmission"] = layers["transmission"][..., 0].contiguous()
    layers["sheen_albedo_scaling_lut"], layers["preintegrated_charlie"] = t(albedo), t(charlie)
    ibl = api.IBLResources(t(G["ibl"]["lut"]), [t(m) for m in G["ibl"]["irradiance"]], [t(m) for m in G["ibl"]["prefiltered"]])
    return types.SimpleNamespace(g={k: t(v) for k, v in gn.items()}, gn=gn, planes=planes, layers=layers, ibl=ibl, camera=camera, sa=sa,
                                 shadows=(t(np.stack(G["shadows"][0])), G["shadows"][1], S.PCF), motion=t(motion), mesh_normal=t(mesh_normal))


@pytest.fixture(scope="module")
def world(mifx_lib):
    """One context, the fixture's frame and one frame of 131 x 67 (the fixture's IBL and shadow maps), shared by every test of the module and left unchanged"""
    from diligentfx_amd import api, binding as B
    from layers_util import make_case

    ctx = api.PostFXContext(0)
    G = S.load_golden()
    small = _env(ctx, G, G["gn"], G["planes"], G["albedo"], G["charlie"], B.camera_from_bytes(G["camera"]), G["attribs"], G["motion"], G["mesh_normal"])
    f, gn, sa, planes, albedo, charlie = make_case("shade_output", BIG, G["ibl"], ctx.device, shadowed=True)
    gn["base_color"], motion, mesh = S.make_extra_inputs(gn, seed=23)
    cam = B.camera_from_bytes(bytes(f["camera"]))
    cam.fSceneNearZ, cam.fSceneFarZ = 4.0, 9.0
    big = _env(ctx, G, gn, planes, albedo, charlie, cam, sa, motion, mesh)
    yield types.SimpleNamespace(ctx=ctx, G=G, small=small, big=big)
    ctx.close()


def run(ctx, e, c, g=None, layers=None, motion=None, mesh_normal=None, **kw):
    from diligentfx_amd import api

    return api.pbr_shade_output(ctx, g or e.g, (layers or e.layers) if c["flags"] else None, c["flags"], e.camera, e.sa, e.ibl, output=S.output_desc_fields(c), shadows=e.shadows,
                                motion=(motion if motion is not None else e.motion) if c["motion"] else None,
                                mesh_normal=(mesh_normal if mesh_normal is not None else e.mesh_normal) if c["mesh_normal"] else None, background=S.BACKGROUND,
                                iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION, **kw)


def layered(ctx, e, flags=S.ALL_LAYERS):
    from diligentfx_amd import api

    return api.pbr_shade_layers(ctx, e.g, e.layers if flags else {}, flags, e.camera, e.sa, e.ibl, background=S.BACKGROUND, iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION,
                                shadows=e.shadows)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_fixture_case_through_the_c_abi(world, c):
    color, spec = run(world.ctx, world.small, c)
    want, want_spec = world.G["out"][c["name"]]
    got = to_np(color)
    assert np.isfinite(got).all()
    assert_close(got, want, max_outlier_frac=0.0, what=f"shade output, {c['name']}")
    assert_close(to_np(spec), want_spec, max_outlier_frac=0.0, what=f"specular IBL, {c['name']}")


def test_identity_case_is_the_layered_shade_bit_for_bit(world):
    """View NONE, no tone map, HighlightColor.a = 0, no animation, OPAQUE, no sRGB: the rgb of the layered shade (all layers, shadows) and of the default shade (no layers),
    alpha 1 on geometry; the specular IBL target is theirs"""
    from diligentfx_amd import api

    ctx, e = world.ctx, world.big
    none = CASES[0]
    assert none["name"] == "none"
    geom = torch.from_numpy(e.gn["depth"] < 1.0 - 1e-6).to(ctx.device)
    color, spec = run(ctx, e, none)
    want, want_spec = layered(ctx, e)
    assert torch.equal(color[..., :3], want[..., :3]) and torch.equal(spec, want_spec)
    assert bool((color[..., 3][geom] == 1.0).all()) and torch.equal(color[~geom], want[~geom])
    plain = dict(none, flags=0)
    color0, spec0 = run(ctx, e, plain)
    want0, want_spec0 = api.pbr_shade(ctx, e.g, e.camera, e.sa, e.ibl, background=S.BACKGROUND, shadows=e.shadows)
    assert torch.equal(color0[..., :3], want0[..., :3]) and torch.equal(spec0, want_spec0) and bool((color0[..., 3][geom] == 1.0).all())
    assert not torch.equal(color0, color)


TAIL_CASES = [c for c in CASES if S.is_tail_case(c)]


@pytest.mark.parametrize("c", TAIL_CASES, ids=[c["name"] for c in TAIL_CASES])
def test_tail_cases_at_the_second_size_against_the_numpy_restatement(world, c):
    """The tail cases at 131 x 67: shade_output_util.tail_np (pinned to the fixture by test_shade_output_cpu.py) applied to the device's own layered shade; the tone-map cases
    go through the library's tone-mapping entry first"""
    from diligentfx_amd import binding as B

    ctx, e = world.ctx, world.big
    lit, _ = layered(ctx, e)
    tone_mapped = None
    if c["tm"]:
        R = S.RENDERER
        src = lit
        if c["unlit"]:
            src = e.g["base_color"]
        tm = B.ToneMappingAttribs(c["tm"], 0, R["MiddleGray"], 0, R["WhitePoint"], 1.0, 0, 0, 1.0, 1.0, 1.0, 0.0)
        tone_mapped = to_np(ctx.tone_map(src.contiguous(), tm, R["AverageLogLum"]))
    want = S.tail_np(c, to_np(lit), e.gn["base_color"], e.gn["depth"], bytes(e.camera), transmission=e.planes["transmission"][..., 0], tone_mapped=tone_mapped)
    color, _ = run(ctx, e, c)
    assert_close(to_np(color), want, max_outlier_frac=0.0, what=f"shade output at 131 x 67, {c['name']}")


def _in_poison(t, oy=3, ox=5, py=4, px=6):
    """`t` as a view into a larger poison-filled tensor: row pitch greater than the width, a non-zero origin"""
    h, w = t.shape[:2]
    big = torch.full((h + oy + py, w + ox + px) + tuple(t.shape[2:]), POISON, device=t.device, dtype=t.dtype)
    view = big[oy:oy + h, ox:ox + w]
    view.copy_(t)
    return big, view


def test_pitched_and_offset_planes(world):
    ctx, e = world.ctx, world.big
    w, h = BIG
    everything = dict(next(c for c in CASES if c["name"] == "everything"))
    for c in (everything, next(c for c in CASES if c["name"] == "view_motion_vectors_plane"), next(c for c in CASES if c["name"] == "view_mesh_normal_plane")):
        want, want_spec = run(ctx, e, c)
        g = {k: _in_poison(v)[1] for k, v in e.g.items()}
        layers = {k: (_in_poison(v)[1] if v.shape[:2] == (h, w) else v) for k, v in e.layers.items()}
        (big_c, out_c), (big_s, out_s) = _in_poison(torch.zeros(h, w, 4, device=ctx.device)), _in_poison(torch.zeros(h, w, 4, device=ctx.device))
        before_c, before_s = big_c.clone(), big_s.clone()
        got, got_spec = run(ctx, e, c, g=g, layers=layers, motion=_in_poison(e.motion)[1], mesh_normal=_in_poison(e.mesh_normal)[1], out_color=out_c, out_specular_ibl=out_s)
        assert got.data_ptr() == out_c.data_ptr() and not got.is_contiguous()
        assert torch.equal(got, want) and torch.equal(got_spec, want_spec), c["name"]
        for big, before in ((big_c, before_c), (big_s, before_s)):  # the poison around both outputs is untouched
            big[3:3 + h, 5:5 + w] = 0
            before[3:3 + h, 5:5 + w] = 0
            assert torch.equal(big, before), c["name"]


@pytest.mark.parametrize("view", ["ROUGHNESS", "SHADING_NORMAL", "DIFFUSE_IBL", "CLEAR_COAT_FACTOR", "SCENE_DEPTH"])
def test_a_view_changes_the_picture(world, view):
    ctx, e = world.ctx, world.big
    none, _ = run(ctx, e, CASES[0])
    got, _ = run(ctx, e, dict(CASES[0], view=S.V[view]))
    geom = e.gn["depth"] < 1.0 - 1e-6
    differ = (np.abs(to_np(got) - to_np(none))[..., :3] > 1e-3).any(-1)
    assert differ[geom].mean() > 0.2, view


def test_refusals_on_the_device(world):
    """(the argument checks precede any device call: test_shade_output_abi.py runs them without a device; here with a live context)"""
    from diligentfx_amd import binding as B

    ctx, e = world.ctx, world.big
    for bad in (dict(CASES[0], view=35), dict(CASES[0], unlit=1, view=S.V["ROUGHNESS"]), dict(CASES[0], tm=9)):
        with pytest.raises(B.MifxError, match="INVALID_ARG"):
            run(ctx, e, bad)
