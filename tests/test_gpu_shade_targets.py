"""GPU tests of the shade's G-buffer targets (mifx_pbr_shade_targets) and of the chain that reads them (mifx_chain_set_shade_output): the footer of Hydrogent's pixel shader
(USD_Renderer.cpp:85-168) behind the shade's output stage.  The entry at 56 x 36 against tests/golden/shade_targets_golden.npz (the reference's shader text, footer included,
compiled per permutation) and at 131 x 67 against the entries it stands on; the chain at 224 x 128 against the reference's passes fed with the entry's planes -- the two-step
argument: the entry against the reference's text, then the chain against the reference's passes on the entry's planes."""
import types

import numpy as np
import pytest
import torch

import shade_output_util as S
import shade_targets_util as T
from test_gpu_shade_output import BIG, _env, _in_poison
from util import assert_close, to_np

pytestmark = pytest.mark.gpu
CASES = T.cases()
PLANES = ("normal", "base_color", "material", "ibl")
CHAIN_SIZE = (224, 128)


@pytest.fixture(scope="module")
def world(mifx_lib):
    """One context, the fixture's frame and one frame of 131 x 67 with an opaque band and exact clear-coat factors, shared by the tests of the entry and left unchanged"""
    from diligentfx_amd import api, binding as B
    from layers_util import make_case

    ctx = api.PostFXContext(0)
    G = T.load_golden()
    small = _env(ctx, G, G["gn"], G["planes"], G["albedo"], G["charlie"], B.camera_from_bytes(G["camera"]), G["attribs"], G["motion"], G["mesh_normal"])
    f, gn, sa, planes, albedo, charlie = make_case("shade_targets", BIG, G["ibl"], ctx.device, shadowed=True)
    gn["base_color"], motion, mesh = S.make_extra_inputs(gn, seed=29)
    gn["base_color"][:, 20:70, 3] = 1.0
    planes["clearcoat"][:, 40:90, 0] = 0.0
    planes["clearcoat"][:, 90:100, 0] = 1.0
    big = _env(ctx, G, gn, planes, albedo, charlie, B.camera_from_bytes(bytes(f["camera"])), sa, motion, mesh)
    yield types.SimpleNamespace(ctx=ctx, G=G, small=small, big=big)
    ctx.close()


def run(ctx, e, c, g=None, layers=None, output=True, **kw):
    """mifx_pbr_shade_targets of a case: (color, normal, base_color, material, ibl)"""
    from diligentfx_amd import api

    ly = None
    if c["flags"]:
        ly = dict(layers or e.layers)
        if not c.get("cc_normal", 1):
            ly.pop("clearcoat_normal")
    return api.pbr_shade_targets(ctx, g or e.g, ly, c["flags"], e.camera, e.sa, e.ibl, output=S.output_desc_fields(c) if output else None, shadows=e.shadows,
                                 motion=e.motion if c["motion"] else None, mesh_normal=e.mesh_normal if c["mesh_normal"] else None, background=S.BACKGROUND,
                                 iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION, **kw)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_every_fixture_case_through_the_c_abi(world, c):
    """The bar: util.assert_close at its defaults with no outliers -- the reference's own strict and contracted builds differ by 2.6e-4 in that measure, below them"""
    got = run(world.ctx, world.small, c)
    want = world.G["out"][c["name"]]
    for o, t in zip(T.OUTPUTS, got):
        assert np.isfinite(to_np(t)).all()
        assert_close(to_np(t), want[o], max_outlier_frac=0.0, what=f"shade targets, {c['name']}, {o}")


def test_entry_equivalence(world):
    """131 x 67, all layers, shadows.  out_color is mifx_pbr_shade_output's bit for bit; with output = NULL the rgb is mifx_pbr_shade_execute_layers's, and where the clear-coat
    factor is exactly 0 and alpha exactly 1 the IBL target is its out_specular_ibl and base_color / material.xy are the inputs"""
    from diligentfx_amd import api

    ctx, e = world.ctx, world.big
    everything = next(c for c in CASES if c["name"] == "everything")
    for c in (everything, CASES[1], next(c for c in CASES if c["name"] == "mask")):
        want, _ = api.pbr_shade_output(ctx, e.g, e.layers, c["flags"], e.camera, e.sa, e.ibl, output=S.output_desc_fields(c), shadows=e.shadows, background=S.BACKGROUND,
                                       iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION)
        assert torch.equal(run(ctx, e, c)[0], want), c["name"]
    color, normal, base, material, ibl = run(ctx, e, CASES[1], output=False)
    lit, spec = api.pbr_shade_layers(ctx, e.g, e.layers, S.ALL_LAYERS, e.camera, e.sa, e.ibl, background=S.BACKGROUND, iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION,
                                     shadows=e.shadows)
    assert torch.equal(color[..., :3], lit[..., :3])
    geom = e.gn["depth"] < 1.0 - 1e-6
    sel = geom & (e.planes["clearcoat"][..., 0] == 0.0) & (e.gn["base_color"][..., 3] == 1.0)
    assert sel.sum() > 500
    m = torch.from_numpy(sel).to(ctx.device)
    assert torch.equal(ibl[m], spec[m]) and torch.equal(base[m], e.g["base_color"][m]) and torch.equal(material[m][:, :2], e.g["material"][m][:, :2])
    assert torch.equal(normal[m][:, :3], e.g["normal"][m][:, :3]) or float((normal[m][:, :3] - e.g["normal"][m][:, :3]).abs().max()) < 1e-6  # normalize(lerp(N, ccN, 0))
    bg = torch.from_numpy(~geom).to(ctx.device)  # no fragment: the caller's texels, a zero IBL
    assert torch.equal(normal[bg], e.g["normal"][bg]) and torch.equal(base[bg], e.g["base_color"][bg]) and torch.equal(material[bg], e.g["material"][bg]) and bool((ibl[bg] == 0).all())
    one = torch.from_numpy(geom & (e.planes["clearcoat"][..., 0] == 1.0)).to(ctx.device)  # the clear coat is in the planes
    assert float((material[one][:, 1]).abs().max()) == 0.0 and not torch.equal(ibl[one], spec[one])


def test_pitched_and_offset_planes(world):
    """All five outputs (and every input) as views into larger poison-filled tensors: the contiguous result bit for bit, the poison around each output untouched"""
    ctx, e = world.ctx, world.big
    w, h = BIG
    c = next(c for c in CASES if c["name"] == "everything")
    want = run(ctx, e, c)
    g = {k: _in_poison(v)[1] for k, v in e.g.items()}
    layers = {k: (_in_poison(v)[1] if v.shape[:2] == (h, w) else v) for k, v in e.layers.items()}
    outs = [_in_poison(torch.zeros(h, w, 4, device=ctx.device)) for _ in range(5)]
    before = [big.clone() for big, _ in outs]
    got = run(ctx, e, c, g=g, layers=layers, out_color=outs[0][1], out_targets={k: outs[i + 1][1] for i, k in enumerate(PLANES)})
    assert got[0].data_ptr() == outs[0][1].data_ptr() and not got[0].is_contiguous()
    for i, o in enumerate(T.OUTPUTS):
        assert torch.equal(got[i], want[i]), o
        big, b = outs[i][0], before[i]
        big[3:3 + h, 5:5 + w] = 0
        b[3:3 + h, 5:5 + w] = 0
        assert torch.equal(big, b), o


def test_refusals_on_the_device(world):
    """(the argument checks precede any device call: test_shade_targets_abi.py runs them without a device; here with a live context)"""
    from diligentfx_amd import binding as B

    ctx, e = world.ctx, world.big
    for bad in (dict(CASES[1], view=35), dict(CASES[1], tm=9)):
        with pytest.raises(B.MifxError, match="INVALID_ARG"):
            run(ctx, e, bad)
    h, w = e.gn["depth"].shape
    with pytest.raises(B.MifxError, match="targets->material"):
        run(ctx, e, CASES[1], out_targets={k: torch.zeros(h + (k == "material"), w, 4, device=ctx.device) for k in PLANES})
    with pytest.raises(B.MifxError, match="aliases a G-buffer plane"):
        run(ctx, e, CASES[1], out_targets={k: (e.g["normal"] if k == "normal" else torch.zeros(h, w, 4, device=ctx.device)) for k in PLANES})


# ------------------------------------------------------------------------------------------------ the chain
DESC_CASE = dict(S._case("chain"), highlight=0.35, anim=S.ANIM_TRANSITIONING, factor=0.4)


class Frames:
    """Four frames of 224 x 128 with all five layers and two shadow-mapped lights, made once and left unchanged"""

    def __init__(self, device, ibl_np):
        import chain_util
        from diligentfx_amd import api, synth
        from layers_util import make_layers

        w, h = CHAIN_SIZE
        self.ibl_np = ibl_np
        self.ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]).to(device), [torch.from_numpy(m).to(device) for m in ibl_np["irradiance"]],
                                    [torch.from_numpy(m).to(device) for m in ibl_np["prefiltered"]])
        self.sa = chain_util.shadowed_shade_attribs(len(ibl_np["prefiltered"]) - 1)
        self.slices, self.infos = chain_util.make_shadow_inputs()
        self.sm = torch.from_numpy(np.stack(self.slices)).to(device)
        self.f, self.layers, self.planes = [], [], []
        scene = synth.Scene()
        for i in range(4):
            f = synth.make_frame(scene, i, w, h, device)
            planes, albedo, charlie = make_layers(to_np(f["normal"]), seed=i + 5)
            dev = {k: torch.from_numpy(v).to(device) for k, v in planes.items()}
            dev["transmission"] = dev["transmission"][..., 0].contiguous()
            dev["sheen_albedo_scaling_lut"], dev["preintegrated_charlie"] = torch.from_numpy(albedo).to(device), torch.from_numpy(charlie).to(device)
            self.f.append(f)
            self.layers.append(dev)
            self.planes.append(planes)

    def run(self, chain, i, out, desc=True, targets=True, layers=True):
        """Frame i through `chain` with the layers, the desc and the targets switched as asked"""
        from layers_util import IOR, ROTATION

        chain.set_material_layers(self.layers[i] if layers else None, 31 if layers else 0, IOR, ROTATION, shadows=(self.sm, self.infos, 3))
        if (desc or targets) and getattr(chain, "_shade_output_set", None) != (desc, targets):  # (once per chain: the call makes the next frame fork its lanes anew)
            chain.set_shade_output(S.output_desc_fields(DESC_CASE) if desc else None, targets)
            chain._shade_output_set = (desc, targets)
        chain.execute(chain.bind_frame(i, self.f[i], self.ibl, self.sa, out))
        return out


@pytest.fixture(scope="module")
def frames(mifx_lib):
    import chain_util
    from layers_util import ref_checker

    return Frames(torch.device("cuda", 0), chain_util.make_ibl(ref_checker(), "ref_"))


def new_chain():
    from diligentfx_amd import api
    from util import blue_noise_tables

    return api.Chain(0, *blue_noise_tables())


@pytest.fixture(scope="module")
def on_and_off(frames):
    """The four frames through a chain with targets on and through one with targets off (same layers, same desc): final images, and SSR's output of the last frame"""
    w, h = CHAIN_SIZE
    on, off = new_chain(), new_chain()
    outs_on, outs_off = [], []
    for i in range(4):
        outs_on.append(frames.run(on, i, torch.zeros(h, w, 4, device=on.device)).clone())
        outs_off.append(frames.run(off, i, torch.zeros(h, w, 4, device=off.device), targets=False).clone())
    ssr_on, ssr_off = on.effect_output("ssr").clone(), off.effect_output("ssr").clone()
    on.close()
    off.close()
    return types.SimpleNamespace(on=outs_on, off=outs_off, ssr_on=ssr_on, ssr_off=ssr_off)


def test_chain_against_the_reference_passes_on_the_entrys_planes(frames, on_and_off):
    """Four frames, all five layers, two shadow-mapped lights, highlight and TRANSITIONING at 0.4, targets on, against the CPU chain: its passes read the planes the stand-alone
    entry wrote for the frame, its shade is that entry's colour and IBL target.  The budget of test_chain_with_material_layers."""
    import chain_util
    import cpu_chain
    from diligentfx_amd import api
    from layers_util import IOR, ROTATION, ref_checker

    cpu = cpu_chain.CpuChain(ref_checker(), "ref_")
    ctx = api.PostFXContext(0)
    fracs = []
    for i in range(4):
        f = frames.f[i]
        gdev = {k: f[k] for k in ("base_color", "normal", "material", "depth")}
        color, normal, base, material, ibl = api.pbr_shade_targets(ctx, gdev, frames.layers[i], 31, f["camera"], frames.sa, frames.ibl, output=S.output_desc_fields(DESC_CASE),
                                                                   shadows=(frames.sm, frames.infos, 3), background=(0.02, 0.03, 0.05, 0.0), iridescence_ior=IOR,
                                                                   anisotropy_rotation=ROTATION)
        g = {k: to_np(v) for k, v in f.items() if isinstance(v, torch.Tensor)}
        g["emissive"] = g["occlusion"] = None
        g["normal"], g["base_color"], g["material"] = to_np(normal), to_np(base), to_np(material)
        shade = lambda gg, cam, a, c=color, s=ibl: (to_np(c), to_np(s))  # noqa: E731
        want = chain_util.run_frame_inputs(cpu, g, bytes(f["camera"]), bytes(f["prev_camera"]), i, frames.ibl_np, frames.sa, shade=shade)
        got = to_np(on_and_off.on[i])
        assert np.isfinite(got).all()
        _, frac = assert_close(got, want, max_outlier_frac=5e-3, outlier_cap=(5e-2, 2e-4), what=f"chain with shade targets, final image frame {i}")
        fracs.append(frac)
        assert np.abs(got[..., :3] - want[..., :3]).mean() < 1e-3
    print("chain with shade targets, outlier fractions per frame:", [round(x, 5) for x in fracs])
    ctx.close()


def test_the_planes_are_in_the_picture(frames, on_and_off):
    """Targets off, same layers and desc: the final image differs inside the clear-coat region, and so does SSR's output"""
    i = 3
    geom = to_np(frames.f[i]["depth"]) < 1.0 - 1e-6
    region = geom & (frames.planes[i]["clearcoat"][..., 0] > 0.5)
    d = np.abs(to_np(on_and_off.on[i]) - to_np(on_and_off.off[i]))[..., :3].max(-1)
    assert region.any() and d[region].max() > 1e-3, d[region].max()
    assert not torch.equal(on_and_off.ssr_on, on_and_off.ssr_off)
    assert float((on_and_off.ssr_on - on_and_off.ssr_off).abs().max()) > 1e-3


def _three_frames(frames, configure):
    w, h = CHAIN_SIZE
    chain = new_chain()
    configure(chain)
    outs = [frames.run(chain, i, torch.zeros(h, w, 4, device=chain.device)) for i in range(3)]
    torch.cuda.synchronize()
    chain.close()
    return outs


def test_overlap_modes_equal_one_stream(frames, on_and_off):
    for mode in range(1, 6):
        outs = _three_frames(frames, lambda c: c.set_overlap(mode))
        for i in range(3):
            assert torch.equal(outs[i], on_and_off.on[i]), (mode, i)


def test_fusion_equals_fusion_off(frames, on_and_off):
    """(on_and_off ran with the default fusion set)"""
    from diligentfx_amd import api

    for mask in (0, api.Chain.FUSE_EVERY_SWITCH):
        outs = _three_frames(frames, lambda c: c.set_fusion_mask(mask))
        for i in range(3):
            assert torch.equal(outs[i], on_and_off.on[i]), (mask, i)


def test_turning_it_off(frames):
    """set_shade_output(None, False), then a history reset on both: the frame of a chain that never had the call, bit for bit"""
    w, h = CHAIN_SIZE
    chain, plain = new_chain(), new_chain()
    out = torch.zeros(h, w, 4, device=chain.device)
    for i in range(2):
        frames.run(chain, i, out)
        frames.run(plain, i, torch.zeros_like(out), desc=False, targets=False)
    chain.set_shade_output(None, False)
    chain.reset_history()
    plain.reset_history()
    a = frames.run(chain, 2, torch.zeros_like(out), desc=False, targets=False)
    b = frames.run(plain, 2, torch.zeros_like(out), desc=False, targets=False)
    assert torch.equal(a, b)
    chain.close()
    plain.close()


def test_chain_refusals(frames):
    from diligentfx_amd import binding as B

    chain = new_chain()
    desc = S.output_desc_fields(DESC_CASE)
    with pytest.raises(B.MifxError, match="tone_mapping_mode 4"):
        chain.set_shade_output(dict(desc, tone_mapping_mode=4), True)
    with pytest.raises(B.MifxError, match="CONVERT_OUTPUT_TO_SRGB"):
        chain.set_shade_output(dict(desc, flags=1), True)
    chain.set_shade_output(desc, True)
    with pytest.raises(B.MifxError, match="mifx_chain_set_shade_output"):
        chain.set_row_band(16, 48, 4)
    chain.set_shade_output(None, False)
    chain.set_row_band(16, 48, 4)
    with pytest.raises(B.MifxError, match="row band or sharding"):
        chain.set_shade_output(desc, True)
    chain.close()
