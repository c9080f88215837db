"""Run in its own process with MIFX_STORAGE=h4 (tests/test_gpu_storage_h4_shadows_oit.py does): the cascaded shadow maps and the layered order-independent
transparency in the native-storage build of the library (libmifx_h4.so).

shadows  Depth, light amount and the cascade plane are F32 / F32X2 in both builds and the filterable array names its own format, so the same kernels compile and
         the same fixtures apply unchanged: three conversion cases and four look-up cases of the 32-bit fixture through the checks of tests/test_gpu_shadows.py,
         and every check of the 16-bit formats (tests/shadows16_checks.py), at their own bars.
oit      Every case of oit_util.cases() on pitched, offset planes -- the 4-channel planes RGBA16_FLOAT, depth / colour alpha / opaque depth F32 -- by the sequence
         entries, the fused entries and the fused entries with the fusion off: the three bit for bit the same, against the emulated expectation (the fp32 header on
         the host, the targets rounded where the build stores them: tests/oit16_util.py) and against the reference fixture under the same rounding
         (tests/golden/oit16_golden.npz) at oit16_util's bars; nothing written outside a plane; a pixel that nothing touches keeps its bits.

Prints what it measured; exits non-zero on the first violated bound."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oit16_util as U  # noqa: E402
import oit_util as O  # noqa: E402
from diligentfx_amd import api, binding as B  # noqa: E402
from h4_checks import same_bits  # noqa: E402
from util import blue_noise_tables  # noqa: E402

F = np.float32
SENTINEL = 12344.0  # (a binary16 value)
FUSED_K = (1, 2, 3, 4, 8)


def make_ctx():
    lib = B.load()
    assert lib.mifx_storage_mode() == 1 and B.storage_dtype() == torch.float16, "not the RGBA16_FLOAT storage build"
    sobol, tile = blue_noise_tables()
    return lib, api.PostFXContext(0, sobol, tile)


# ------------------------------------------------------------------------------------------------ shadows
CONV32 = ("conv_13x9_m4_f3_16bit_clamp", "conv_50x38_m3_world", "conv_260x70_m4_f7")
LOOK32 = ("look_pcf3_n3", "look_vsm_n3_across_best_lbr", "look_evsm2_n3_across", "look_evsm4_n3_2x2")


def section_shadows(lib, ctx):
    import shadows16_checks as K
    import shadows16_util as U16
    import test_gpu_shadows as T32
    import test_shadows_cpu as C32

    conv, look = dict((n, i) for i, n in C32.conv_cases()), dict((n, i) for i, n in C32.look_cases())
    for name in CONV32:
        T32.test_conversion_against_the_reference_fixture_fused_and_two_launch(lib, ctx, conv[name], name)
    for name in LOOK32:
        T32.test_lookup_against_the_reference_fixture(lib, ctx, look[name], name)
    for i, name in U16.conv_cases():
        K.check_conversion_case(ctx, i, name)
    for i, name in U16.look_cases():
        K.check_lookup_case(ctx, i, name)
    K.check_refusals_with_a_context(ctx)
    K.check_python_mirror_keeps_the_callers_flag_for_fp32_maps(ctx)
    host = U16.host_lib()
    assert host is not None, "hipcc not available: the host harness cannot be built"
    for mode in (2, 3, 4):
        K.check_python_mirror(ctx, host, mode)


# ------------------------------------------------------------------------------------------------ oit
def _pitched(a, ctx, dtype):
    """`a` (H, W) or (H, W, 4) on the device as a view of `dtype` with a row pitch of W + 5 texels and an offset of 2 rows and 4 texels into a sentinel-filled block"""
    h, w = a.shape[:2]
    block = torch.full((h + 3, w + 5) + tuple(a.shape[2:]), SENTINEL, dtype=dtype, device=ctx.device)
    view = block[2:2 + h, 4:4 + w]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device).to(dtype))
    return view, block


def _untouched_outside(block, h, w):
    m = torch.ones_like(block, dtype=torch.bool)
    m[2:2 + h, 4:4 + w] = False
    return bool(torch.all(block[m] == SENTINEL))


def _device_case(d, ctx, blocks):
    def up(a, dtype):
        v, b = _pitched(a, ctx, dtype)
        blocks.append((b, a.shape[0], a.shape[1]))
        return v

    slices = []
    for i in range(d["depth"].shape[0]):
        s = dict(depth=up(d["depth"][i], torch.float32), base_color=up(d["base"][i], torch.float16), material=up(d["material"][i], torch.float16),
                 radiance=up(d["radiance"][i], torch.float16), specular_ibl=up(d["ibl"][i], torch.float16))
        if d["alpha"] is not None:
            s["color_alpha"] = up(d["alpha"][i], torch.float32)
        slices.append(s)
    opaque = up(d["opaque"], torch.float32) if d["opaque"] is not None else None
    return slices, opaque


def _targets(d, ctx, blocks):
    t = {}
    for j, k in enumerate(api.OIT_TARGETS):
        t[k], b = _pitched(d["targets"][j], ctx, torch.float16)
        blocks.append((b, d["targets"].shape[1], d["targets"].shape[2]))
    return t


def _read(oit, t):
    torch.cuda.synchronize()
    layers = oit.get_layers().cpu().numpy().view(np.uint32)
    tail = oit.get_tail().contiguous().cpu().numpy()
    assert tail.dtype == np.float32 and layers.dtype == np.uint32
    return layers, tail, torch.stack([t[k].contiguous() for k in api.OIT_TARGETS])


def _poison(oit):
    oit.get_layers().fill_(0x5EADBEEF)
    oit.get_tail().fill_(-7.0)


def _oit_case(lib, ctx, host, i, c):
    g = U.golden()
    name = c["name"]
    d = U.make_case16(c)
    cam = O.camera_struct(d["camera"])
    blocks = []
    slices, opaque = _device_case(d, ctx, blocks)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    assert oit.plane_dtype == torch.float16
    runs = {}
    default = lib.mifx_oit_set_fusion(1)
    try:
        _poison(oit)
        t = _targets(d, ctx, blocks)
        oit.clear_layers()
        for s in slices:
            oit.update_layers(s, cam, opaque)
        oit.apply_attenuation(t)
        for s in slices:
            oit.blend(s, cam, t, opaque)
        runs["sequence entries"] = _read(oit, t)
        for fused, what in ((1, "fused entries"), (0, "fused entries, fusion off")):
            lib.mifx_oit_set_fusion(fused)
            _poison(oit)
            t = _targets(d, ctx, blocks)
            oit.render(slices, t, cam, opaque)
            runs[what] = _read(oit, t)
    finally:
        lib.mifx_oit_set_fusion(default)
    for b, h, w in blocks:
        assert _untouched_outside(b, h, w), f"{name}: something was written outside a plane"
    seq = runs["sequence entries"]
    for what in ("fused entries", "fused entries, fusion off"):
        other = runs[what]
        assert np.array_equal(other[0], seq[0]) and np.array_equal(other[1].view(np.uint32), seq[1].view(np.uint32)) and same_bits(other[2], seq[2]), f"{name}: {what} differ from the sequence"
    emulated = U.emulate(host, c, d)
    fixture = (g[f"c{i}_layers"], g[f"c{i}_tail"], g[f"c{i}_targets"].astype(F))
    for what, (layers, tail, targets) in runs.items():
        got = (layers, tail, targets.float().cpu().numpy())
        U.check_against(got, emulated, f"{name}: {what} vs the emulated sequence")
        U.check_against(got, fixture, f"{name}: {what} vs the reference fixture")
    oit.close()


def _untouched_pixel_keeps_its_bits(lib, ctx):
    """The attenuation discards where the transmittance is 1 and the fused resolve does not store an untouched pixel: binary16 texels holding a NaN payload, a
    denormal, -0 and -infinity survive (a load and a store of them would quieten or keep them, a rounding in registers must not be stored)"""
    c = next(c for c in O.cases() if c["name"] == "oit_5x3_k4_l7")
    d = U.make_case16(c)
    cam = O.camera_struct(d["camera"])
    odd = torch.tensor([0x7D23, 0x0001, 0x8000 - 0x10000, 0xFC00 - 0x10000], dtype=torch.int16, device=ctx.device)  # signalling NaN payload, smallest denormal, -0, -inf
    blocks = []
    slices, opaque = _device_case(d, ctx, blocks)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    default = lib.mifx_oit_set_fusion(1)
    try:
        for fused in (1, 0):
            lib.mifx_oit_set_fusion(fused)
            t = _targets(d, ctx, blocks)
            for k in api.OIT_TARGETS:
                t[k].view(torch.int16)[0, 0] = odd  # pixel 0: no slice covers it
            oit.render(slices, t, cam, opaque)
            torch.cuda.synchronize()
            for k in api.OIT_TARGETS:
                assert torch.equal(t[k].view(torch.int16)[0, 0], odd), (fused, k)
                assert not torch.equal(t[k].view(torch.int16)[1, 3], _targets(d, ctx, [])[k].view(torch.int16)[1, 3])  # (pixel 8, seven fragments front to back, did change)
    finally:
        lib.mifx_oit_set_fusion(default)
    oit.close()


def section_oit(lib, ctx):
    host = U.host_lib()
    assert host is not None, "hipcc not available: the host harness cannot be built"
    cs = O.cases()
    for i, c in enumerate(cs):
        _oit_case(lib, ctx, host, i, c)
    # a layer count without a fused kernel: the fused entries take the sequence's launches
    c = dict(next(c for c in cs if c["name"] == "oit_5x3_k4_l7"), k=5, name="oit_5x3_k5_l7_no_fused_kernel")
    assert c["k"] not in FUSED_K
    d = U.make_case16(c)
    cam = O.camera_struct(d["camera"])
    blocks = []
    slices, opaque = _device_case(d, ctx, blocks)
    oit = api.OITResources(ctx, c["w"], c["h"], c["k"])
    _poison(oit)
    t = _targets(d, ctx, blocks)
    oit.render(slices, t, cam, opaque)
    layers, tail, targets = _read(oit, t)
    U.check_against((layers, tail, targets.float().cpu().numpy()), U.emulate(host, c, d), f"{c['name']}: fused entries vs the emulated sequence")
    oit.close()
    _untouched_pixel_keeps_its_bits(lib, ctx)


SECTIONS = {"shadows": section_shadows, "oit": section_oit}


def main():
    names = sys.argv[1:] or list(SECTIONS)
    lib, ctx = make_ctx()
    for n in names:
        SECTIONS[n](lib, ctx)
        print(f"h4 section {n} OK", flush=True)
    print("h4 checks OK")


if __name__ == "__main__":
    main()
