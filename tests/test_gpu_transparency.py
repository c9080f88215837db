"""Transparent draws on the GPU: mifx_oit_shade_blend (one launch: the layered shade's body and the OIT colour pass behind it) against the two-step sequence it replaces
-- mifx_pbr_shade_execute_layers into two planes, then mifx_oit_blend -- bit for bit on all four targets, at the fixture's boundary frame sizes, every plane pitched and
offset inside a sentinel block; the 24x16 end-to-end case against the reference's targets (tests/golden/oit_golden.npz) by the project's contract, util.assert_close at
its defaults with no outlier; and mifx_chain_set_transparency: fused against unfused, the overlap modes against one stream, the chain against the public entries run
outside it -- all bit for bit --, the chain with transparency off, and its refusals; then the chain's picture against the CPU chain fed the entries' planes, layers / shadow maps / color_alpha passed
through the chain, the boundary frame sizes, and a fixed sequence of switches in the middle of a run.  Inputs: tests/transparency_util.py."""
import numpy as np
import pytest
import torch

import oit_util as O
import test_gpu_oit as G
import test_oit_cpu as C
import transparency_util as T
from util import assert_close, blue_noise_tables

pytestmark = pytest.mark.gpu
F = np.float32
ODD = np.array([0x7FC12345, 0x00000001, 0x80000000, 0xFF800000], np.uint32).view(F)  # a NaN payload, a denormal, -0, -inf


@pytest.fixture(scope="module")
def world(mifx_lib):
    import chain_util
    from diligentfx_amd import api
    from test_gpu_pbr import checker, ibl_to_device

    lib, pfx = checker("ibl_brdf_lut")
    ibl_np = chain_util.make_ibl(lib, pfx)
    ctx = api.PostFXContext(0, *blue_noise_tables())
    slices, infos = chain_util.make_shadow_inputs()
    last = len(ibl_np["prefiltered"]) - 1
    return dict(ctx=ctx, ibl=ibl_to_device(ibl_np, ctx.device), ibl_np=ibl_np, sa=chain_util.shade_attribs(last), sa_shadowed=chain_util.shadowed_shade_attribs(last),
                shadows=(torch.from_numpy(np.stack(slices)).to(ctx.device), infos, 3))


def _layers(world, s, seed):
    """All five layers for the slices' frame size (layers_util.make_layers), on the device"""
    from layers_util import make_layers

    planes, albedo, charlie = make_layers(s["gbuffers"][0]["normal"], seed=seed)
    dev = {k: torch.from_numpy(v).to(world["ctx"].device) for k, v in planes.items()}
    dev["transmission"] = dev["transmission"][..., 0].contiguous()
    dev["sheen_albedo_scaling_lut"], dev["preintegrated_charlie"] = torch.from_numpy(albedo).to(world["ctx"].device), torch.from_numpy(charlie).to(world["ctx"].device)
    return dev


def _both_ways(world, s, k, all_layers=False, reversed_=False, plant_odd=None):
    """The slices of `s` blended into two copies of the targets -- by the two-step sequence and by mifx_oit_shade_blend -- behind the same build_layers and
    apply_attenuation; every plane pitched and offset.  Returns (two-step targets, fused targets, blocks, the targets' start values); targets as (4, H, W, 4)
    arrays, blocks = (block, h, w) of every plane, to check the sentinels."""
    ctx = world["ctx"]
    h, w = s["targets"].shape[1:3]
    if reversed_:
        ctx.prepare_resources(0, w, h, feature_flags=1)  # (the shade reads reversed depth from the context)
    try:
        return _both_ways_on(world, s, k, all_layers, plant_odd)
    finally:
        if reversed_:
            ctx.prepare_resources(0, w, h, feature_flags=0)


def _both_ways_on(world, s, k, all_layers, plant_odd):
    from diligentfx_amd import api
    from layers_util import IOR, ROTATION

    ctx = world["ctx"]
    h, w = s["targets"].shape[1:3]
    blocks = []

    def up(a):
        v, b = G._pitched(a, ctx)
        blocks.append((b, a.shape[0], a.shape[1]))
        return v

    gbs = [{n: up(v) for n, v in gb.items()} for gb in s["gbuffers"]]
    alphas = [up(a) for a in s["alpha"]] if s["alpha"] is not None else [None] * len(gbs)
    opaque = up(s["opaque"]) if s["opaque"] is not None else None
    start = s["targets"].copy()
    if plant_odd is not None:
        start[:, plant_odd[1], plant_odd[0]] = ODD
    sets = [{name: up(start[j]) for j, name in enumerate(api.OIT_TARGETS)} for _ in range(2)]
    layers, flags, sa, shadows = ({}, 0, world["sa"], None)
    if all_layers:
        layers, flags, sa, shadows = _layers(world, s, 11), 31, world["sa_shadowed"], world["shadows"]
    oit = api.OITResources(ctx, w, h, k)
    G._poison(oit)
    cam = s["camera"]
    oit.build_layers([dict(depth=g["depth"], base_color=g["base_color"]) for g in gbs], cam, opaque)
    for t in sets:
        oit.apply_attenuation(t)
    for g, a in zip(gbs, alphas):
        rad, spec = api.pbr_shade_layers(ctx, g, layers, flags, cam, sa, world["ibl"], background=(0.0, 0.0, 0.0, 0.0), iridescence_ior=IOR, anisotropy_rotation=ROTATION,
                                         shadows=shadows)
        two = dict(depth=g["depth"], base_color=g["base_color"], material=g["material"], radiance=rad, specular_ibl=spec)
        if a is not None:
            two["color_alpha"] = a
        oit.blend(two, cam, sets[0], opaque)
        oit.shade_blend(dict(gbuffer=g, layers=layers, flags=flags, iridescence_ior=IOR, anisotropy_rotation=ROTATION, color_alpha=a), cam, sa, world["ibl"], sets[1], opaque,
                        shadows=shadows)
    torch.cuda.synchronize()
    out = [np.stack([t[name].contiguous().cpu().numpy() for name in api.OIT_TARGETS]) for t in sets]
    oit.close()
    return out[0], out[1], blocks, start


ENTRY_CASES = [
    ("oit_1x1_k4_l4", {}), ("oit_2x2_k4_l7", {}), ("oit_5x3_k4_l7", dict(plant_odd=(0, 0))), ("oit_5x3_k4_l7", dict(all_layers=True)),
    ("oit_5x3_k3_l6_reversed", dict(reversed_=True)), ("oit_5x3_k4_l7_color_alpha", {}), ("oit_5x3_k4_l7_no_opaque", {}),
    ("oit_67x35_k4_l7", dict(all_layers=True, plant_odd="uncovered")), ("oit_67x35_k8_l2_reversed", dict(reversed_=True)), ("e2e", {}),
]


@pytest.mark.parametrize("name,kw", ENTRY_CASES, ids=[n + ("_" + "_".join(sorted(k)) if k else "") for n, k in ENTRY_CASES])
def test_entry_equals_shade_then_blend_bit_for_bit(world, name, kw):
    """No layers and all five layers with two shadow-mapped lights, reversed depth, color_alpha, no opaque depth; 67x35 spans more than one workgroup both ways.  A pixel
    without a fragment keeps its bits, NaN payloads included; nothing is written outside any plane."""
    kw = dict(kw)
    if name == "e2e":
        s, k = T.e2e_slices(), O.E2E["k"]
    else:
        c = T.case(name)
        s, k = T.make_slices(c), c["k"]
    if kw.get("plant_odd") == "uncovered":
        y, x = np.argwhere(~s["fragments"].any(0))[0]
        kw["plant_odd"] = (int(x), int(y))
    two, fused, blocks, start = _both_ways(world, s, k, **kw)
    for b, h, w in blocks:
        assert G._untouched_outside(b, h, w), f"{name}: something was written outside a plane"
    differ = int((two.view(np.uint32) != fused.view(np.uint32)).sum())
    print(f"{name}: {differ} of {two.size} target values differ in their bits; {int((fused.view(np.uint32) != start.view(np.uint32)).any(-1).sum())} texels changed")
    assert C.same_bits(two, fused), name
    assert s["fragments"].any() and not C.same_bits(fused, start)  # something was blended
    if kw.get("plant_odd") is not None:
        x, y = kw["plant_odd"]
        assert not s["fragments"][:, y, x].any()
        assert np.array_equal(fused[:, y, x].view(np.uint32), np.tile(ODD.view(np.uint32), (4, 1)))


def test_end_to_end_case_meets_the_references_targets(world):
    """24x16, two slices, K = 4, through OITResources.shade_blend against the fixture's targets, which the generator shaded and blended with the reference's own shaders:
    util.assert_close at its defaults, no outlier (the rule of test_gpu_oit.py::test_end_to_end_shade_two_slices_then_render for this fixture)"""
    from diligentfx_amd import api

    g = C.golden()
    ctx = world["ctx"]
    e = O.e2e_inputs()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)  # noqa: E731
    gbs = [{k: dev(v) for k, v in gb.items()} for gb in e["gbuffers"]]
    t = {k: dev(e["targets"][j]) for j, k in enumerate(api.OIT_TARGETS)}
    oit = api.OITResources(ctx, O.E2E["w"], O.E2E["h"], O.E2E["k"])
    oit.build_layers([dict(depth=gd["depth"], base_color=gd["base_color"]) for gd in gbs], e["camera"])
    oit.apply_attenuation(t)
    for gd in gbs:
        oit.shade_blend(dict(gbuffer=gd), e["camera"], world["sa"], world["ibl"], t)
    layers, tail, targets = G._read(oit, t)
    assert np.array_equal(layers, g["e2e_layers"]) and np.array_equal(tail[..., 0], g["e2e_tail"][..., 0])
    assert (targets != e["targets"]).any(-1).mean() > 0.5  # most texels are covered by a slice
    for j, k in enumerate(api.OIT_TARGETS):
        print(f"target {k}: max |diff| {np.abs(targets[j] - g['e2e_targets'][j]).max():.3e}")
        assert_close(targets[j], g["e2e_targets"][j], what=f"shade-and-blend, end to end: target {k}")
    oit.close()


# ------------------------------------------------------------------------------------------------ the chain
PLANES = ("normal", "base_color", "material", "ibl")
CHAIN_SIZES = [(67, 35), (24, 16)]


class ChainCase:
    """Three consecutive frames of one history at w x h and two transparent slices (K = 4), on the device, made once and left unchanged"""

    def __init__(self, world, w, h):
        from diligentfx_amd import synth

        dev = world["ctx"].device
        self.w, self.h, self.world = w, h, world
        scene = synth.Scene()
        self.f = [synth.make_frame(scene, i, w, h, dev) for i in range(3)]
        s = T.e2e_slices() if (w, h) == (24, 16) else T.make_slices(T.case("oit_67x35_k4_l7"))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.slices = [dict(gbuffer={k: up(v) for k, v in gb.items()}) for gb in s["gbuffers"][:2]]
        assert len(self.slices) == 2

    def run(self, configure=None, transparency=True):
        """(out_ldr, {plane: tensor}) per frame"""
        from diligentfx_amd import api

        chain = api.Chain(0, *blue_noise_tables())
        chain.set_shade_output(None, True)
        if transparency:
            chain.set_transparency(self.slices, 4)
        if configure:
            configure(chain)
        outs = []
        for i in range(3):
            out = torch.zeros(self.h, self.w, 4, device=chain.device)
            chain.execute(chain.bind_frame(i, self.f[i], self.world["ibl"], self.world["sa"], out))
            torch.cuda.synchronize()
            outs.append((out, {p: chain.shade_target(p).clone() for p in PLANES}))
        chain.close()
        return outs


@pytest.fixture(scope="module", params=CHAIN_SIZES, ids=[f"{w}x{h}" for w, h in CHAIN_SIZES])
def chain_case(world, request):
    cc = ChainCase(world, *request.param)
    cc.reference = cc.run()  # one stream, the default fusion set, the fused launch
    return cc


def _same(a, b, what):
    for i in range(3):
        assert torch.equal(a[i][0].view(torch.int32), b[i][0].view(torch.int32)), (what, i, "out_ldr")
        for p in PLANES:
            assert torch.equal(a[i][1][p].view(torch.int32), b[i][1][p].view(torch.int32)), (what, i, p)


def test_chain_fused_equals_unfused(mifx_lib, chain_case):
    default = mifx_lib.mifx_chain_set_transparency_fusion(0)
    try:
        unfused = chain_case.run()
        mifx_lib.mifx_chain_set_transparency_fusion(1)
        fused = chain_case.run()
    finally:
        mifx_lib.mifx_chain_set_transparency_fusion(default)
    _same(fused, unfused, "fused against unfused")
    _same(fused, chain_case.reference, "fused against the default")


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
def test_chain_overlap_modes_equal_one_stream(chain_case, mode):
    _same(chain_case.run(lambda c: c.set_overlap(mode)), chain_case.reference, f"overlap {mode}")


def test_chain_fusion_masks_equal_the_default(chain_case):
    """Every fusion switch of the chain off, and every switch on (the reference ran with the default set): the same bits"""
    from diligentfx_amd import api

    for mask in (0, api.Chain.FUSE_EVERY_SWITCH):
        _same(chain_case.run(lambda c: c.set_fusion_mask(mask)), chain_case.reference, f"fusion mask {mask}")


def test_chain_equals_the_public_entries_outside_it(chain_case):
    """mifx_pbr_shade_targets, then build_layers, apply_attenuation and one shade_blend per slice with the frame's depth as the opaque depth: the chain's target planes
    bit for bit (the Normal target is not blended)"""
    from diligentfx_amd import api

    world, ctx = chain_case.world, chain_case.world["ctx"]
    oit = api.OITResources(ctx, chain_case.w, chain_case.h, 4)
    for i in range(3):
        f = chain_case.f[i]
        gdev = {k: f[k] for k in ("base_color", "normal", "material", "depth")}
        color, normal, base, material, ibl = api.pbr_shade_targets(ctx, gdev, None, 0, f["camera"], world["sa"], world["ibl"], background=(0.02, 0.03, 0.05, 0.0))
        untouched = base.clone()
        t = dict(color=color, base_color=base, material=material, ibl=ibl)
        oit.build_layers([dict(depth=s["gbuffer"]["depth"], base_color=s["gbuffer"]["base_color"]) for s in chain_case.slices], f["camera"], f["depth"])
        oit.apply_attenuation(t)
        for s in chain_case.slices:
            oit.shade_blend(s, f["camera"], world["sa"], world["ibl"], t, f["depth"])
        torch.cuda.synchronize()
        assert not torch.equal(untouched, base)
        got = chain_case.reference[i][1]
        for p, want in (("normal", normal), ("base_color", base), ("material", material), ("ibl", ibl)):
            assert torch.equal(got[p].view(torch.int32), want.view(torch.int32)), (i, p)
    oit.close()


def test_chain_transparency_is_in_the_picture_and_off_is_off(mifx_lib, chain_case):
    """The image differs from the chain without slices; a chain whose transparency was turned off again (count == 0) launches no OIT kernel and gives the image of a chain
    that never had the call, bit for bit"""
    from diligentfx_amd import api

    never = chain_case.run(transparency=False)
    assert not torch.equal(never[2][0], chain_case.reference[2][0])
    assert float((never[2][0] - chain_case.reference[2][0]).abs().max()) > 1e-3
    _same(chain_case.run(lambda c: c.set_transparency([], 4)), never, "count == 0")
    _same(chain_case.run(lambda c: c.set_transparency(None)), never, "slices == NULL")
    chain = api.Chain(0, *blue_noise_tables())
    chain.set_shade_output(None, True)
    chain.set_transparency(chain_case.slices, 4)
    chain.set_transparency([], 4)
    out = torch.zeros(chain_case.h, chain_case.w, 4, device=chain.device)
    names = ("oit_shade_blend_kernel",) + G.FUSED_KERNELS + G.SEQUENCE_KERNELS
    frame = lambda i: chain.execute(chain.bind_frame(i, chain_case.f[i], chain_case.world["ibl"], chain_case.world["sa"], out))  # noqa: E731
    counts = {k: G._launches(chain.postfx, k, lambda: frame(0)) for k in names}
    assert counts == {k: 0 for k in names}, counts
    chain.set_transparency(chain_case.slices, 4)  # ... and on: one launch per slice behind one build and one attenuation
    counts = {k: G._launches(chain.postfx, k, lambda: frame(0)) for k in names}
    assert counts["oit_shade_blend_kernel"] == 2 and counts["oit_build_kernel"] == 1 and counts["oit_attenuate_kernel"] == 1 and counts["oit_blend_kernel"] == 0, counts
    assert chain.oit() is not None and chain.oit().get_layers().shape == (chain_case.h, chain_case.w, 4)
    chain.close()


def test_chain_refusals(world):
    from diligentfx_amd import api
    from diligentfx_amd import binding as B

    cc = ChainCase(world, 24, 16)
    chain = api.Chain(0, *blue_noise_tables())
    with pytest.raises(B.MifxError, match="write_targets"):  # the precondition, in this order ...
        chain.set_transparency(cc.slices, 4)
    chain.set_shade_output(None, True)
    chain.set_transparency(cc.slices, 4)
    with pytest.raises(B.MifxError, match="mifx_chain_set_transparency"):  # ... and in the other
        chain.set_shade_output({"renderer": B.PBRRendererShaderParameters()}, False)
    with pytest.raises(B.MifxError, match="MIFX_OIT_MAX_SLICES"):
        chain.set_transparency(cc.slices * 17, 4)
    for k in (0, 17):
        with pytest.raises(B.MifxError, match="layer_count"):
            chain.set_transparency(cc.slices, k)
    with pytest.raises(B.MifxError, match="mifx_chain_set_shade_output"):  # a row band behind transparency: refused because of the shade output transparency needs
        chain.set_row_band(4, 12, 2)
    out = torch.zeros(cc.h, cc.w, 4, device=chain.device)
    chain.execute(chain.bind_frame(0, cc.f[0], world["ibl"], world["sa"], out))  # (the last accepted call still stands)
    # a slice whose planes are not the frame's size, at execute time: nothing of the frame is launched
    big = ChainCase(world, 67, 35)
    chain.set_transparency(big.slices, 4)
    before = out.clone()
    with pytest.raises(B.MifxError, match="size"):
        chain.execute(chain.bind_frame(1, cc.f[1], world["ibl"], world["sa"], out))
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    chain.close()
    # a row band first: transparency cannot be reached, because the shade output it needs is refused
    chain = api.Chain(0, *blue_noise_tables())
    chain.set_row_band(4, 12, 2)
    with pytest.raises(B.MifxError, match="row band or sharding"):
        chain.set_shade_output(None, True)
    with pytest.raises(B.MifxError, match="write_targets"):
        chain.set_transparency(cc.slices, 4)
    chain.close()


# ------------------------------------------------------------------------------------------------ the chain: the picture, what it passes through, boundary sizes, switches
class FeatureCase:
    """Consecutive frames of one history at w x h with two hash-made transparent slices (T.chain_slices: its coverage conditions are asserted there on the CPU and here
    against the device's own frame depth), made once and left unchanged.  rich: both slices carry all five material layers (layers_util.make_layers), the second a
    color_alpha plane, and the chain shades with all five layers and two shadow-mapped lights (set_material_layers(..., shadows=...))."""

    def __init__(self, world, w, h, frames=3, rich=True, first=0):
        from diligentfx_amd import synth
        from layers_util import IOR, ROTATION

        dev = world["ctx"].device
        self.w, self.h, self.world, self.rich = w, h, world, rich
        scene = synth.Scene()
        self.f = [synth.make_frame(scene, first + i, w, h, dev) for i in range(frames)]
        self.index = [first + i for i in range(frames)]
        s = T.chain_slices(w, h)
        depth = np.stack([g["depth"] for g in s["gbuffers"]])
        for f in self.f:
            T.check_coverage(T.fragment_mask(depth, f["depth"].cpu().numpy(), False), f"{w}x{h}")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.slices = [dict(gbuffer={k: up(v) for k, v in gb.items()}) for gb in s["gbuffers"]]
        self.sa, self.shadows, self.layers = world["sa"], None, None
        if rich:
            for j, sl in enumerate(self.slices):
                sl.update(layers=_layers(world, s, 11 + j), flags=31, iridescence_ior=IOR, anisotropy_rotation=ROTATION)
            self.sa, self.shadows = world["sa_shadowed"], world["shadows"]
            self.layers = _layers(world, dict(gbuffers=[dict(normal=self.f[0]["normal"].cpu().numpy())]), 5)
        self.slices[1]["color_alpha"] = up(s["alpha"][1])

    def set_layers(self, chain):
        from layers_util import IOR, ROTATION

        if self.rich:
            chain.set_material_layers(self.layers, 31, IOR, ROTATION, shadows=self.shadows)

    def entries(self, i, oit, count=2):
        """The public entries outside the chain for frame i: mifx_pbr_shade_targets, then -- `count` slices -- build_layers, apply_attenuation and one shade_blend per slice
        with the frame's depth.  Returns (colour, {plane: tensor})"""
        from diligentfx_amd import api
        from layers_util import IOR, ROTATION

        world, f = self.world, self.f[i]
        gdev = {k: f[k] for k in ("base_color", "normal", "material", "depth")}
        color, normal, base, material, ibl = api.pbr_shade_targets(world["ctx"], gdev, self.layers, 31 if self.rich else 0, f["camera"], self.sa, world["ibl"], shadows=self.shadows,
                                                                   background=(0.02, 0.03, 0.05, 0.0), iridescence_ior=IOR, anisotropy_rotation=ROTATION)
        if count:
            t = dict(color=color, base_color=base, material=material, ibl=ibl)
            sl = self.slices[:count]
            oit.build_layers([dict(depth=x["gbuffer"]["depth"], base_color=x["gbuffer"]["base_color"]) for x in sl], f["camera"], f["depth"])
            oit.apply_attenuation(t)
            for x in sl:
                oit.shade_blend(x, f["camera"], self.sa, world["ibl"], t, f["depth"], shadows=self.shadows)
        torch.cuda.synchronize()
        return color, dict(normal=normal, base_color=base, material=material, ibl=ibl)

    def run(self, configure=None):
        """(out_ldr, {plane: tensor}) per frame of a chain with the shade's targets and the case's slices"""
        from diligentfx_amd import api

        chain = api.Chain(0, *blue_noise_tables())
        chain.set_shade_output(None, True)
        self.set_layers(chain)
        chain.set_transparency(self.slices, 4)
        if configure:
            configure(chain)
        outs = []
        for i, f in enumerate(self.f):
            out = torch.zeros(self.h, self.w, 4, device=chain.device)
            chain.execute(chain.bind_frame(self.index[i], f, self.world["ibl"], self.sa, out))
            torch.cuda.synchronize()
            outs.append((out, {p: chain.shade_target(p).clone() for p in PLANES}))
        chain.close()
        return outs


def _equal_to_the_entries(mifx_lib, case, what):
    """The chain of `case`, fused and unfused, against the public entries outside it: all four targets of every frame, bit for bit"""
    from diligentfx_amd import api

    default = mifx_lib.mifx_chain_set_transparency_fusion(0)
    try:
        unfused = case.run()
        mifx_lib.mifx_chain_set_transparency_fusion(1)
        fused = case.run()
    finally:
        mifx_lib.mifx_chain_set_transparency_fusion(default)
    oit = api.OITResources(case.world["ctx"], case.w, case.h, 4)
    for i in range(len(case.f)):
        _, opaque = case.entries(i, oit, count=0)
        _, want = case.entries(i, oit)
        assert not torch.equal(opaque["base_color"], want["base_color"])  # (something was blended)
        for p in PLANES:
            assert torch.equal(fused[i][1][p].view(torch.int32), want[p].view(torch.int32)), (what, "fused", i, p)
            assert torch.equal(unfused[i][1][p].view(torch.int32), want[p].view(torch.int32)), (what, "unfused", i, p)
        assert torch.equal(fused[i][0].view(torch.int32), unfused[i][0].view(torch.int32)), (what, i, "out_ldr, fused against unfused")
    oit.close()


@pytest.mark.parametrize("size", CHAIN_SIZES, ids=[f"{w}x{h}" for w, h in CHAIN_SIZES])
def test_chain_passes_layers_shadow_maps_and_color_alpha_through(mifx_lib, world, size):
    """test_chain_equals_the_public_entries_outside_it with what chain_transparency passes through and the other chain tests leave out: both slices carry all five material
    layers, the second a color_alpha plane, and the chain itself shades with all five layers and two shadow-mapped lights, which the transparent draws share.  All four
    targets bit for bit, the fused launch and the unfused sequence."""
    _equal_to_the_entries(mifx_lib, FeatureCase(world, *size), f"layers, shadow maps, color_alpha at {size}")


@pytest.mark.parametrize("size", [(8, 8), (33, 17)], ids=["8x8", "33x17"])
def test_chain_equals_the_public_entries_at_boundary_sizes(mifx_lib, world, size):
    """The same equality at the frame sizes of test_chain_edges -- 8x8: one partial workgroup; 33x17: one texel beyond a tile in x, one row beyond in y -- with slices made
    for those sizes (transparency_util.CHAIN_SEEDS: every slice covers 5 % of the texels, one texel is covered by none)"""
    _equal_to_the_entries(mifx_lib, FeatureCase(world, *size), f"boundary size {size}")


def test_chain_picture_against_the_cpu_chain_on_the_entries_planes(world):
    """The chain blends the transparent colour into its own radiance plane, which no entry reads back: held here through the picture made from it.  Three frames at 224x128,
    two hash-made slices, the final image against the CPU chain whose shade is the colour and the IBL target the stand-alone entries produced for the frame (shade targets,
    build_layers, apply_attenuation, one shade_blend per slice) and whose passes read those entries' normal / base colour / material.  The budget of
    tests/test_gpu_shade_targets.py::test_chain_against_the_reference_passes_on_the_entrys_planes, whose later passes are the same."""
    import chain_util
    import cpu_chain
    from diligentfx_amd import api
    from layers_util import ref_checker

    case = FeatureCase(world, 224, 128, rich=False)
    got = case.run()
    cpu = cpu_chain.CpuChain(ref_checker(), "ref_")
    oit = api.OITResources(world["ctx"], case.w, case.h, 4)
    to_np = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())  # noqa: E731
    fracs = []
    for i, f in enumerate(case.f):
        opaque_color, _ = case.entries(i, oit, count=0)
        color, planes = case.entries(i, oit)
        assert float((color - opaque_color).abs().max()) > 1e-2  # (the transparent colour is in the radiance the passes are fed)
        g = {k: to_np(v) for k, v in f.items() if isinstance(v, torch.Tensor)}
        g["emissive"] = g["occlusion"] = None
        g["normal"], g["base_color"], g["material"] = to_np(planes["normal"]), to_np(planes["base_color"]), to_np(planes["material"])
        shade = lambda gg, cam, a, c=color, s=planes["ibl"]: (to_np(c), to_np(s))  # noqa: E731
        want = chain_util.run_frame_inputs(cpu, g, bytes(f["camera"]), bytes(f["prev_camera"]), i, world["ibl_np"], case.sa, shade=shade)
        out = to_np(got[i][0])
        assert np.isfinite(out).all()
        _, frac = assert_close(out, want, max_outlier_frac=5e-3, outlier_cap=(5e-2, 2e-4), what=f"chain with transparency, final image frame {i}")
        fracs.append(frac)
        mean = float(np.abs(out[..., :3] - want[..., :3]).mean())
        print(f"chain with transparency at 224x128, frame {i}: outlier fraction {frac:.5f}, mean |RGB difference| {mean:.3e}")
        assert mean < 1e-3
    print("chain with transparency, outlier fractions per frame:", [round(x, 5) for x in fracs])
    oit.close()


def _mid_run(world, cases, mode, read_planes):
    """The sequence of T.mid_run_state through one chain object in overlap `mode`.  read_planes: the four target planes of every frame where the shade writes them (a host
    synchronisation per frame, to read them); otherwise every frame's out_ldr, the frames queued without a host synchronisation, as an application queues them."""
    from diligentfx_amd import api

    chain = api.Chain(0, *blue_noise_tables())
    chain.set_overlap(mode)
    outs, before = [], None
    for i in range(T.MID_RUN_FRAMES):
        targets, count, k, second = state = T.mid_run_state(i)
        case = cases[1 if second else 0]
        if before is None or state[:3] != before[:3]:
            if not targets:
                chain.set_transparency(None)
                chain.set_shade_output(None, False)
            else:
                chain.set_shade_output(None, True)
                chain.set_transparency(case.slices[:count], k)
        before = state
        out = torch.zeros(case.h, case.w, 4, device=chain.device)
        chain.execute(chain.bind_frame(i, case.f[i], world["ibl"], case.sa, out))
        if read_planes:
            torch.cuda.synchronize()
            outs.append({p: chain.shade_target(p).clone() for p in PLANES} if targets else None)
        else:
            outs.append(out)
    torch.cuda.synchronize()
    chain.close()
    return outs


def test_chain_switches_in_the_middle_of_a_run(world):
    """One chain object through transparency on (frame 2), one slice instead of two (3), another layer_count (4: the OIT object is destroyed and re-created), transparency
    off (5), the shade output off (6), a resize from 24x16 to 33x17 (7) and everything back on (8), in overlap modes 0, 3, 4 and 5.  Wherever the shade writes its targets
    they equal the public entries run outside the chain for that frame's state -- those do not depend on history -- and, the ten frames queued without a host
    synchronisation, the final images of modes 3, 4 and 5 equal one stream's, bit for bit."""
    from diligentfx_amd import api

    cases = [FeatureCase(world, 24, 16, frames=T.MID_RUN_FRAMES, rich=False), FeatureCase(world, 33, 17, frames=T.MID_RUN_FRAMES, rich=False)]
    planes = {mode: _mid_run(world, cases, mode, True) for mode in (0, 3, 4, 5)}
    images = {mode: _mid_run(world, cases, mode, False) for mode in (0, 3, 4, 5)}
    oits = {}
    for i in range(T.MID_RUN_FRAMES):
        targets, count, k, second = T.mid_run_state(i)
        case = cases[1 if second else 0]
        if targets:
            oit = oits.setdefault((case.w, k), api.OITResources(world["ctx"], case.w, case.h, k))
            _, want = case.entries(i, oit, count=count)
        for mode in (0, 3, 4, 5):
            if targets:
                for p in PLANES:
                    assert torch.equal(planes[mode][i][p].view(torch.int32), want[p].view(torch.int32)), (mode, i, p)
            assert torch.equal(images[mode][i].view(torch.int32), images[0][i].view(torch.int32)), (mode, i, "out_ldr against one stream")
    assert not torch.equal(images[0][4], images[0][5]) and float((images[0][4] - images[0][5]).abs().max()) > 1e-3  # (the switches are in the picture)
    for oit in oits.values():
        oit.close()
