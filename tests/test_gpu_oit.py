"""Layered order-independent transparency on the GPU: the C ABI against the reference fixture (tests/golden/oit_golden.npz; inputs from tests/oit_util.py) by the
reference's sequence of launches and by the fused kernels, the two against each other, every plane pitched and offset inside a sentinel block (the boundary frame sizes
1x1, 2x2, 5x3 and 67x35 are the fixture's own), the layers' persistence across calls, and one end-to-end case through the Python mirror.

Tolerances: the layers and the tail's count are integers of strict fp32 comparisons and one product (==); the tail's transmittance and the four targets are held to the
project's contract, util.assert_close at its defaults with no outlier -- the fixture stores the difference between the reference's own strict and contracted builds for
every case (at most 2.5e-7, far inside 0.5e-3: tests/golden/make_golden_oit.py asserts it).  The fused kernels and the sequence are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import oit_util as O
import test_oit_cpu as C
from util import assert_close, blue_noise_tables

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 12345.0
SEQUENCE_KERNELS = ("oit_clear_kernel", "oit_update_kernel", "oit_attenuate_kernel", "oit_blend_kernel")
FUSED_KERNELS = ("oit_build_kernel", "oit_resolve_kernel")


@pytest.fixture(scope="module")
def ctx():
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    return api.PostFXContext(0, sobol, tile)


def _pitched(a, ctx):
    """`a` (H, W) or (H, W, 4) on the device as a view with a row pitch of W + 5 texels and an offset of 2 rows and 4 texels into a sentinel-filled block"""
    h, w = a.shape[:2]
    block = torch.full((h + 3, w + 5) + tuple(a.shape[2:]), SENTINEL, dtype=torch.float32, device=ctx.device)
    view = block[2:2 + h, 4:4 + w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device))
    return view, block


def _untouched_outside(block, h, w):
    m = torch.ones_like(block, dtype=torch.bool)
    m[2:2 + h, 4:4 + w] = False
    return bool(torch.all(block[m] == SENTINEL))


def _device_case(d, ctx):
    """(slices, opaque depth, targets, blocks): every plane of case `d` pitched and offset; blocks = (block, h, w) of every plane, to check the sentinels afterwards"""
    blocks = []

    def up(a):
        v, b = _pitched(a, ctx)
        blocks.append((b, a.shape[0], a.shape[1]))
        return v

    slices = []
    for i in range(d["depth"].shape[0]):
        s = dict(depth=up(d["depth"][i]), base_color=up(d["base"][i]), material=up(d["material"][i]), radiance=up(d["radiance"][i]), specular_ibl=up(d["ibl"][i]))
        if d["alpha"] is not None:
            s["color_alpha"] = up(d["alpha"][i])
        slices.append(s)
    opaque = up(d["opaque"]) if d["opaque"] is not None else None
    return slices, opaque, blocks


def _targets(d, ctx, blocks):
    from diligentfx_amd import api

    t = {}
    for j, k in enumerate(api.OIT_TARGETS):
        t[k], b = _pitched(d["targets"][j], ctx)
        blocks.append((b, d["targets"].shape[1], d["targets"].shape[2]))
    return t


def _read(oit, t):
    from diligentfx_amd import api

    torch.cuda.synchronize()
    layers = oit.get_layers().cpu().numpy().view(np.uint32)
    tail = oit.get_tail().contiguous().cpu().numpy()
    return layers, tail, (np.stack([t[k].contiguous().cpu().numpy() for k in api.OIT_TARGETS]) if t is not None else None)


def _poison(oit):
    oit.get_layers().fill_(0x5EADBEEF)
    oit.get_tail().fill_(-7.0)


def _launches(ctx, name, fn):
    """How often the kernel-timing bracket `name` was passed while fn() ran (mifx_postfx_set_kernel_timing / _get_kernel_times); at most 8 are counted"""
    from diligentfx_amd import binding as B

    B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, name.encode(), 8))
    try:
        fn()
        times, n = (ctypes.c_float * 8)(), ctypes.c_uint32(0)
        B.check(ctx.lib.mifx_postfx_get_kernel_times(ctx.handle, times, 8, ctypes.byref(n)))
        return n.value
    finally:
        B.check(ctx.lib.mifx_postfx_set_kernel_timing(ctx.handle, None, 0))


def _sequence(oit, slices, opaque, cam, t):
    """The reference's sequence through the per-launch entries"""
    oit.clear_layers()
    for s in slices:
        oit.update_layers(s, cam, opaque)
    oit.apply_attenuation(t)
    for s in slices:
        oit.blend(s, cam, t, opaque)


@pytest.mark.parametrize("i,name", C.case_ids())
def test_every_fixture_case_by_the_sequence_and_by_the_fused_entries(mifx_lib, ctx, i, name):
    """Every case through the C ABI on pitched, offset planes: the per-launch entries and the fused entries against the fixture, fused against sequence bit for bit,
    the kernel-timing names saying which kernels ran, nothing written outside any plane."""
    from diligentfx_amd import api

    g = C.golden()
    c = O.cases()[i]
    d = O.make_case(c)
    cam = O.camera_struct(d["camera"])
    want_l, want_t, want_g = g[f"c{i}_layers"], g[f"c{i}_tail"], g[f"c{i}_targets"]
    slices, opaque, blocks = _device_case(d, ctx)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    default = mifx_lib.mifx_oit_set_fusion(1)
    try:
        _poison(oit)
        t = _targets(d, ctx, blocks)
        _sequence(oit, slices, opaque, cam, t)
        seq = _read(oit, t)
        results = {}
        for fused in (1, 0):
            mifx_lib.mifx_oit_set_fusion(fused)
            _poison(oit)
            t = _targets(d, ctx, blocks)
            oit.render(slices, t, cam, opaque)
            results[fused] = _read(oit, t)
        # which kernels run: the fused pair where a fused kernel exists for the layer count and the switch is on, otherwise the sequence's launches
        for fused in (1, 0):
            mifx_lib.mifx_oit_set_fusion(fused)
            takes_fused = bool(fused) and c["k"] in C.FUSED_K
            counts = {k: _launches(ctx, k, lambda: oit.render(slices, _targets(d, ctx, []), cam, opaque)) for k in FUSED_KERNELS + SEQUENCE_KERNELS}
            want = {k: int(takes_fused) for k in FUSED_KERNELS}
            want.update({"oit_clear_kernel": int(not takes_fused), "oit_attenuate_kernel": int(not takes_fused),
                         "oit_update_kernel": 0 if takes_fused else min(c["l"], 8), "oit_blend_kernel": 0 if takes_fused else min(c["l"], 8)})
            assert counts == want, (name, fused, counts)
    finally:
        mifx_lib.mifx_oit_set_fusion(default)
    torch.cuda.synchronize()
    for b, h, w in blocks:
        assert _untouched_outside(b, h, w), f"{name}: something was written outside a plane"
    for what, (layers, tail, targets) in (("sequence entries", seq), ("fused entries", results[1]), ("fused entries, fusion off", results[0])):
        print(f"{name}: {what}: {int((layers != want_l).sum())} layer words differ, tail transmittance max |diff| {np.abs(tail[..., 1] - want_t[..., 1]).max():.3e}, "
              f"targets max |diff| {np.abs(targets - want_g).max():.3e}")
        assert np.array_equal(layers, want_l) and np.array_equal(tail[..., 0], want_t[..., 0]), (name, what)
        assert_close(tail[..., 1], want_t[..., 1], what=f"{name}: {what}: tail transmittance")
        for j, k in enumerate(api.OIT_TARGETS):
            assert_close(targets[j], want_g[j], what=f"{name}: {what}: target {k}")
    for other in (results[1], results[0]):
        assert np.array_equal(other[0], seq[0]) and C.same_bits(other[1], seq[1]) and C.same_bits(other[2], seq[2]), name
    oit.close()


def test_a_pixel_no_slice_covers_keeps_its_bits(mifx_lib, ctx):
    """The attenuation discards where the transmittance is 1 and the fused resolve does not store an untouched pixel: texels holding NaN payloads and denormals survive"""
    from diligentfx_amd import api

    c = next(c for c in O.cases() if c["name"] == "oit_5x3_k4_l7")
    d = O.make_case(c)
    odd = np.array([0x7FC12345, 0x00000001, 0x80000000, 0xFF800000], np.uint32).view(F)
    for j in range(4):
        d["targets"][j, 0, 0] = odd  # pixel 0: no slice covers it
    cam = O.camera_struct(d["camera"])
    slices, opaque, blocks = _device_case(d, ctx)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    default = mifx_lib.mifx_oit_set_fusion(1)
    try:
        for fused in (1, 0):
            mifx_lib.mifx_oit_set_fusion(fused)
            t = _targets(d, ctx, blocks)
            oit.render(slices, t, cam, opaque)
            got = _read(oit, t)[2]
            assert np.array_equal(got[:, 0, 0].view(np.uint32), np.tile(odd.view(np.uint32), (4, 1))), fused
    finally:
        mifx_lib.mifx_oit_set_fusion(default)
    oit.close()


def test_the_layers_persist_across_calls(mifx_lib, ctx):
    """update_layers of slices 0 .. 1, then of 2 .. 4, on the cleared object equals build_layers of 0 .. 4 (fused and not): layers and tail bit for bit"""
    from diligentfx_amd import api

    c = next(c for c in O.cases() if c["name"] == "oit_5x3_k3_l6")
    d = O.make_case(c)
    cam = O.camera_struct(d["camera"])
    slices, opaque, _ = _device_case(d, ctx)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    _poison(oit)
    oit.clear_layers()
    for s in slices[0:2]:
        oit.update_layers(s, cam, opaque)
    torch.cuda.synchronize()
    first = _read(oit, None)
    for s in slices[2:5]:
        oit.update_layers(s, cam, opaque)
    step = _read(oit, None)
    assert not np.array_equal(first[0], step[0])
    default = mifx_lib.mifx_oit_set_fusion(1)
    try:
        for fused in (1, 0):
            mifx_lib.mifx_oit_set_fusion(fused)
            _poison(oit)
            oit.build_layers(slices[0:5], cam, opaque)
            built = _read(oit, None)
            assert np.array_equal(built[0], step[0]) and C.same_bits(built[1], step[1]), fused
    finally:
        mifx_lib.mifx_oit_set_fusion(default)
    oit.close()


def test_refusals_through_the_entries_with_an_object(mifx_lib, ctx):
    """A refusal of the entries themselves (real object, real planes: nothing is launched, the targets keep their values)"""
    from diligentfx_amd import api
    from diligentfx_amd import binding as B

    c = next(c for c in O.cases() if c["name"] == "oit_5x3_k4_l4")
    d = O.make_case(c)
    cam = O.camera_struct(d["camera"])
    slices, opaque, blocks = _device_case(d, ctx)
    t = _targets(d, ctx, blocks)
    with pytest.raises(B.MifxError):
        api.OITResources(ctx, 5, 3, 17)
    oit = api.OITResources(ctx, 6, 3, 4)  # another size than the planes
    with pytest.raises(B.MifxError):
        oit.render(slices, t, cam, opaque)
    oit.close()
    oit = api.OITResources(ctx, 5, 3, 4)
    with pytest.raises(B.MifxError):
        oit.build_layers(slices * 9, cam, opaque)  # 36 slices
    with pytest.raises(B.MifxError):
        oit.blend(dict(depth=slices[0]["depth"], base_color=slices[0]["base_color"]), cam, t, opaque)  # a colour entry without the colour planes
    torch.cuda.synchronize()
    assert np.array_equal(_read(oit, t)[2], d["targets"])
    oit.close()


def test_end_to_end_shade_two_slices_then_render(mifx_lib, ctx):
    """Through the Python mirror: two transparent slices shaded with mifx_pbr_shade_execute, then OITResources.render; against the fixture's targets for the same
    G-buffers, which the generator shaded with the reference's own shade.  (The shade is held to its checker with no outlier by tests/test_gpu_pbr.py; the blend adds
    products of its values, so the contract's measure carries over.)"""
    import chain_util
    from diligentfx_amd import api
    from test_gpu_pbr import checker, ibl_to_device

    g = C.golden()
    lib, pfx = checker("ibl_brdf_lut")
    ibl_np = chain_util.make_ibl(lib, pfx)
    ibl = ibl_to_device(ibl_np, ctx.device)
    sa = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    e = O.e2e_inputs()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)  # noqa: E731
    slices = []
    for gb in e["gbuffers"]:
        gd = {k: dev(v) for k, v in gb.items()}
        rad, spec = api.pbr_shade(ctx, gd, e["camera"], sa, ibl, background=(0.0, 0.0, 0.0, 0.0))
        slices.append(dict(depth=gd["depth"], base_color=gd["base_color"], material=gd["material"], radiance=rad, specular_ibl=spec))
    t = {k: dev(e["targets"][j]) for j, k in enumerate(api.OIT_TARGETS)}
    oit = api.OITResources(ctx, O.E2E["w"], O.E2E["h"], O.E2E["k"])
    oit.render(slices, t, e["camera"])
    layers, tail, targets = _read(oit, t)
    assert np.array_equal(layers, g["e2e_layers"]) and np.array_equal(tail[..., 0], g["e2e_tail"][..., 0])
    assert (targets != e["targets"]).any(-1).mean() > 0.5  # most texels are covered by a slice
    for j, k in enumerate(api.OIT_TARGETS):
        assert_close(targets[j], g["e2e_targets"][j], what=f"end to end: target {k}")
    oit.close()
