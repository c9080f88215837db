"""Transparent draws on the GPU: mifx_oit_shade_blend (one launch: the layered shade's body and the OIT colour pass behind it) against the two-step sequence it replaces
-- mifx_pbr_shade_execute_layers into two planes, then mifx_oit_blend -- bit for bit on all four targets, at the fixture's boundary frame sizes, every plane pitched and
offset inside a sentinel block; the 24x16 end-to-end case against the reference's targets (tests/golden/oit_golden.npz) by the project's contract, util.assert_close at
its defaults with no outlier; and mifx_chain_set_transparency: fused against unfused, the overlap modes against one stream, the chain against the public entries run
outside it -- all bit for bit --, the chain with transparency off, and its refusals.  Inputs: tests/transparency_util.py."""
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
    return dict(ctx=ctx, ibl=ibl_to_device(ibl_np, ctx.device), sa=chain_util.shade_attribs(last), sa_shadowed=chain_util.shadowed_shade_attribs(last),
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
