"""Caller planes in every layout include/mifx.h allows: pitched, borrowed planes.  Each image a pass takes from the caller, inputs and caller-owned outputs alike,
is given (a) contiguous, (b) row-padded -- a view [:, :W] of a wider parent whose rows are an odd number of texels, so that a float plane's pitch is a multiple of
neither 8 nor 256 bytes -- and (c) column-offset -- a view [:, 1:W + 1], whose base is one texel off the parent's alignment (4 bytes off 8 for a float plane,
16 off 256 for a float4 plane).  Only the addressing differs, so (b) and (c) must give (a)'s values bit for bit; (a) is held to the checker by each pass' own test.
Every parent is filled with a NaN sentinel first: no byte outside a view may change, and no input may change at all."""
import numpy as np
import pytest
import torch

from util import blue_noise_tables

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a quiet NaN with a payload
SIZES = [(64, 36), (67, 37)]  # an even and an odd width

# (entry point of include/mifx.h, what runs it here): the coverage guard tests/test_frame_edges_coverage.py reads this table
LAYOUT_MATRIX = {
    "mifx_postfx_execute": "test_prep_layouts",
    "mifx_ssao_execute": "test_ssao_layouts",
    "mifx_ssr_execute": "test_ssr_layouts, test_ssr_direct_level0",
    "mifx_taa_execute": "test_taa_layouts",
    "mifx_bloom_execute": "test_bloom_layouts",
    "mifx_dof_execute": "test_dof_layouts",
    "mifx_pbr_shade_execute": "test_pbr_shade_layouts",
    "mifx_composite_execute": "test_composite_layouts",
    "mifx_composite_execute_selection": "test_composite_layouts",
    "mifx_selection_execute": "test_selection_layouts",
    "mifx_autoexposure_execute": "test_autoexposure_layouts",
    "mifx_tonemap_execute": "test_tonemap_layouts",
    "mifx_tonemap_execute_auto": "test_tonemap_layouts",
    "mifx_chain_execute": "test_chain_layouts",
}


class Layout:
    """Places caller planes in one layout and checks afterwards that nothing outside them (nothing at all, for inputs) was written."""

    def __init__(self, kind):
        self.kind, self.planes = kind, []

    def __call__(self, t, output=False):
        t = t.contiguous()
        h, w = t.shape[:2]
        if self.kind == "a":
            parent, cols = torch.empty_like(t), slice(0, w)
        elif self.kind == "b":
            pad = 3 if w % 2 == 0 else 2  # parent rows of an odd number of texels
            parent, cols = torch.empty((h, w + pad, *t.shape[2:]), dtype=t.dtype, device=t.device), slice(0, w)
        else:
            parent, cols = torch.empty((h, w + 2, *t.shape[2:]), dtype=t.dtype, device=t.device), slice(1, w + 1)
        parent.view(torch.int32).fill_(SENTINEL)
        view = parent[:, cols]
        if not output:
            view.copy_(t)
        assert view.data_ptr() != t.data_ptr() and (self.kind == "a") == view.is_contiguous()
        self.planes.append((parent, cols, None if output else t.clone()))
        return view

    def check(self):
        torch.cuda.synchronize()
        for parent, cols, original in self.planes:
            bits = parent.view(torch.int32)
            outside = torch.ones(bits.shape[:2], dtype=torch.bool, device=bits.device)
            outside[:, cols] = False
            assert bool((bits[outside] == SENTINEL).all()), f"layout {self.kind}: bytes outside a {tuple(parent.shape)} caller plane's view were written"
            if original is not None:
                assert torch.equal(parent[:, cols].view(torch.int32), original.view(torch.int32)), f"layout {self.kind}: an input plane was written"


def _bits(x):
    return x.contiguous().view(torch.int32).cpu().numpy().copy() if isinstance(x, torch.Tensor) else x


def _same_in_every_layout(run, w, h):
    """run(lay, w, h) -> dict of result planes (torch tensors, read before the next run); (b) and (c) against (a), bit for bit."""
    results = {}
    for kind in ("a", "b", "c"):
        lay = Layout(kind)
        results[kind] = {k: _bits(v) for k, v in run(lay, w, h).items()}
        lay.check()
    for kind in ("b", "c"):
        for name, want in results["a"].items():
            got = results[kind][name]
            assert np.array_equal(got, want), f"layout {kind} {w}x{h}: {name} differs from the contiguous run in {int((got != want).sum())} values"


def _frame(frame, w, h, dev, **kw):
    from diligentfx_amd import synth

    return synth.make_frame(synth.Scene(), frame, w, h, dev, **kw)


def _colour(f):
    return torch.cat([f["base_color"][..., :3] * 2.0 + 0.05 * f["normal"][..., :3].abs(), f["base_color"][..., 3:4]], -1).contiguous()


def _ctx():
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    return api.PostFXContext(0, sobol, tile)


@pytest.mark.parametrize("size", SIZES)
def test_prep_layouts(mifx_lib, size):
    def run(lay, w, h):
        ctx = _ctx()
        out = {}
        for fi in range(2):
            f = _frame(fi, w, h, ctx.device)
            ctx.prepare_resources(fi, w, h)
            ctx.execute(lay(f["depth"]), lay(f["prev_depth"]), lay(f["motion"]), f["camera"], f["prev_camera"])
            out[f"reprojected_depth{fi}"] = ctx.get_reprojected_depth()
            out[f"closest_motion{fi}"] = ctx.get_closest_motion_vectors()
            out = {k: _bits(v) for k, v in out.items()}
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("half", [0, 2])
def test_ssao_layouts(mifx_lib, size, half):
    from diligentfx_amd import api, binding as B

    def run(lay, w, h):
        ctx = _ctx()
        fx = api.ScreenSpaceAmbientOcclusion(ctx)
        attribs = B.SSAOAttribs.default()
        out = {}
        for fi in range(2):
            f = _frame(fi, w, h, ctx.device)
            ctx.prepare_resources(fi, w, h)
            fx.prepare_resources(feature_flags=half)
            ctx.execute(lay(f["depth"]), lay(f["prev_depth"]), lay(f["motion"]), f["camera"], f["prev_camera"])
            fx.execute(lay(f["depth"]), lay(f["normal"]), attribs)
            out[f"ao{fi}"] = _bits(fx.get_ambient_occlusion())
            for k in range(1, 5):
                out[f"prefiltered_depth{k} {fi}"] = _bits(fx.get_intermediate(f"prefiltered_depth{k}"))
                out[f"conv_depth{k} {fi}"] = _bits(fx.get_intermediate(f"conv_depth{k}"))
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


def _ssr_run(direct0=None, half=0, frames=2):
    import os

    from diligentfx_amd import api, binding as B

    def run(lay, w, h):
        ctx = _ctx()
        old = os.environ.get("MIFX_SSR_DIRECT_LEVEL0")
        if direct0 is not None:
            os.environ["MIFX_SSR_DIRECT_LEVEL0"] = str(direct0)  # (read by mifx_ssr_create)
        try:
            fx = api.ScreenSpaceReflection(ctx)
        finally:
            if old is None:
                os.environ.pop("MIFX_SSR_DIRECT_LEVEL0", None)
            else:
                os.environ["MIFX_SSR_DIRECT_LEVEL0"] = old
        attribs = B.SSRAttribs.default()
        out = {}
        for fi in range(frames):
            f = _frame(fi, w, h, ctx.device)
            ctx.prepare_resources(fi, w, h)
            fx.prepare_resources(feature_flags=half)
            ctx.execute(lay(f["depth"]), lay(f["prev_depth"]), lay(f["motion"]), f["camera"], f["prev_camera"])
            import test_gpu_ssr

            fx.execute(lay(test_gpu_ssr.scene_color(f)), lay(f["depth"]), lay(f["normal"]), lay(f["material"]), lay(f["motion"]), attribs)
            out[f"ssr{fi}"] = _bits(fx.get_ssr_radiance())
            for k in range(1, 7):
                out[f"hiz{k} {fi}"] = _bits(fx.get_intermediate(f"hiz{k}"))
            for n in ("ray_radiance", "ray_dir_pdf"):
                out[f"{n} {fi}"] = _bits(fx.get_intermediate(n))
        fx.close()
        ctx.close()
        return out

    return run


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("half", [0, 2])
def test_ssr_layouts(mifx_lib, size, half):
    _same_in_every_layout(_ssr_run(direct0=0, half=half), *size)


@pytest.mark.parametrize("size", SIZES)
def test_ssr_direct_level0(mifx_lib, size):
    """MIFX_SSR_DIRECT_LEVEL0=1: the ray march reads Hi-Z level 0 from the caller's depth plane itself (its pitch, its base) instead of the library's copy.
    In all three layouts the output and every level equal the copy path's, bit for bit."""
    w, h = size
    copy = {k: _bits(v) for k, v in _ssr_run(direct0=0)(Layout("a"), w, h).items()}
    for kind in ("a", "b", "c"):
        lay = Layout(kind)
        got = {k: _bits(v) for k, v in _ssr_run(direct0=1)(lay, w, h).items()}
        lay.check()
        for name, want in copy.items():
            assert np.array_equal(got[name], want), f"DIRECT0 layout {kind} {w}x{h}: {name} differs from the copy path in {int((got[name] != want).sum())} values"


@pytest.mark.parametrize("size", SIZES)
def test_taa_layouts(mifx_lib, size):
    from diligentfx_amd import api, binding as B

    def run(lay, w, h):
        ctx = _ctx()
        fx = api.TemporalAntiAliasing(ctx)
        out = {}
        for fi in range(3):
            f = _frame(fi, w, h, ctx.device)
            ctx.prepare_resources(fi, w, h)
            fx.prepare_resources(7)
            ctx.execute(lay(f["depth"]), lay(f["prev_depth"]), lay(f["motion"]), f["camera"], f["prev_camera"])
            fx.execute(lay(_colour(f)), B.TAAAttribs.default())
            out[f"taa{fi}"] = _bits(fx.get_accumulated_frame())
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_bloom_layouts(mifx_lib, size):
    from diligentfx_amd import api, binding as B
    import test_gpu_bloom_taa

    def run(lay, w, h):
        ctx = _ctx()
        ctx.prepare_resources(0, w, h)
        fx = api.Bloom(ctx)
        fx.prepare_resources()
        attribs = B.BloomAttribs.default()
        attribs.Radius = 1.0
        fx.execute(lay(test_gpu_bloom_taa.hdr_scene(w, h, ctx.device)), attribs)
        out = {"bloom": _bits(fx.get_bloom_texture()), "down0": _bits(fx.get_intermediate("down0")), "up0": _bits(fx.get_intermediate("up0"))}
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_dof_layouts(mifx_lib, size):
    from diligentfx_amd import api, binding as B
    import test_gpu_dof

    def run(lay, w, h):
        ctx = _ctx()
        fx = api.DepthOfField(ctx)
        attribs = B.DOFAttribs.default()
        attribs.MaxCircleOfConfusion = 0.02
        out = {}
        for fi in range(7, 9):
            f = _frame(fi, w, h, ctx.device)
            ctx.prepare_resources(fi, w, h)
            fx.prepare_resources(3)
            ctx.execute(lay(f["depth"]), lay(f["prev_depth"]), lay(f["motion"]), test_gpu_dof.lens_camera(f["camera"]), f["prev_camera"])
            fx.execute(lay(test_gpu_dof.hdr_colour(f, ctx.device)), lay(f["depth"]), attribs)
            out[f"dof{fi}"] = _bits(fx.get_depth_of_field_texture())
            out[f"coc{fi}"] = _bits(fx.get_intermediate("coc"))
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


def _ibl(ctx):
    from diligentfx_amd import api, synth

    return api.precompute_ibl(ctx, synth.make_sky_cube(16, ctx.device), lut_size=16, irradiance_size=4, prefiltered_size=8, lut_samples=16, diffuse_samples=16,
                              specular_samples=8)


@pytest.mark.parametrize("size", SIZES)
def test_pbr_shade_layouts(mifx_lib, size):
    import chain_util
    from diligentfx_amd import api

    def run(lay, w, h):
        ctx = _ctx()
        ibl = _ibl(ctx)
        f = _frame(4, w, h, ctx.device)
        gen = torch.Generator(device="cpu").manual_seed(3)
        g = {k: lay(f[k]) for k in ("base_color", "normal", "material", "depth")}
        g["emissive"] = lay((torch.rand(h, w, 4, generator=gen) * 0.3).to(ctx.device))
        g["occlusion"] = lay((0.3 + 0.7 * torch.rand(h, w, generator=gen)).to(ctx.device))
        rad, spec = lay(torch.empty(h, w, 4, device=ctx.device), output=True), lay(torch.empty(h, w, 4, device=ctx.device), output=True)
        api.pbr_shade(ctx, g, f["camera"], chain_util.shade_attribs(len(ibl.pre) - 1), ibl, background=(0.02, 0.03, 0.05, 0.0), out_radiance=rad, out_specular_ibl=spec)
        out = {"radiance": _bits(rad), "specular_ibl": _bits(spec)}
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_composite_layouts(mifx_lib, size):
    """mifx_composite_execute and mifx_composite_execute_selection: eight (eleven) caller inputs and the caller's output."""
    import selection_util as S
    from diligentfx_amd import api, binding as B

    def run(lay, w, h):
        ctx = _ctx()
        ibl = _ibl(ctx)
        f = _frame(2, w, h, ctx.device)
        gen = torch.Generator(device="cpu").manual_seed(11)
        rnd = lambda *s: torch.rand(*s, generator=gen).to(ctx.device)  # noqa: E731
        color = torch.cat([rnd(h, w, 3) * 3.0, f["base_color"][..., 3:4]], -1)
        ins = [lay(t) for t in (color, rnd(h, w, 4), rnd(h, w, 4), rnd(h, w), f["normal"], f["base_color"], f["material"], ibl.lut)]
        tm = B.ToneMappingAttribs.default(4)
        out0 = lay(torch.empty(h, w, 4, device=ctx.device), output=True)
        api.composite(ctx, *ins, f["camera"], 0.9, 0.8, tone_mapping=tm, ave_log_lum=0.3, out=out0)
        sel = S.make_selection_depth(f["depth"].cpu().numpy(), np.random.default_rng(4), seeds=5, max_radius=10)
        fx = api.ProcessSelection(ctx)
        a = B.SelectionAttribs.default(selection_id=2)
        a.nonselection_desaturation, a.outline_width = 0.4, 5.0
        sd = lay(torch.from_numpy(sel).to(ctx.device))
        fx.execute(sd, a)
        closest = lay(fx.get_output())
        out1 = lay(torch.empty(h, w, 4, device=ctx.device), output=True)
        api.composite_selection(ctx, *ins, f["camera"], lay(f["depth"]), sd, closest, a, 0.9, 0.8, tone_mapping=tm, ave_log_lum=0.3, out=out1)
        out = {"composite": _bits(out0), "composite_selection": _bits(out1)}
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_selection_layouts(mifx_lib, size):
    import test_gpu_selection
    from diligentfx_amd import api, binding as B

    def run(lay, w, h):
        ctx = _ctx()
        _, sel = test_gpu_selection._selection_inputs(w, h, 5)
        fx = api.ProcessSelection(ctx)
        a = B.SelectionAttribs.default(selection_id=7)
        a.max_distance = 16.0
        fx.execute(lay(torch.from_numpy(sel).to(ctx.device)), a)
        out = {"closest": _bits(fx.get_output())}
        fx.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_autoexposure_layouts(mifx_lib, size):
    from diligentfx_amd import api, synth

    def run(lay, w, h):
        ctx = _ctx()
        ae = api.AutoExposure(ctx)
        ae.execute(lay(synth.make_hdr_buffer(w, h, ctx.device)), 0.4, True)
        out = {"low_res_luminance": _bits(ae.plane("low_res_luminance")), "average_luminance": _bits(ae.plane("average_luminance"))}
        ae.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


@pytest.mark.parametrize("size", SIZES)
def test_tonemap_layouts(mifx_lib, size):
    from diligentfx_amd import api, binding as B, synth

    def run(lay, w, h):
        ctx = _ctx()
        hdr = lay(synth.make_hdr_buffer(w, h, ctx.device))
        tm = B.ToneMappingAttribs.default(4)
        o0, o1 = lay(torch.empty(h, w, 4, device=ctx.device), output=True), lay(torch.empty(h, w, 4, device=ctx.device), output=True)
        ctx.tone_map(hdr, tm, 0.3, flags=1, out=o0)
        ae = api.AutoExposure(ctx)
        ae.execute(hdr, 0.0, False)
        ae.tone_map(hdr, tm, flags=1, out=o1)
        out = {"tonemap": _bits(o0), "tonemap_auto": _bits(o1)}
        ae.close()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)


def _chain_run(frames=4):
    import chain_util
    from diligentfx_amd import api, binding as B, synth

    def run(lay, w, h):
        sobol, tile = blue_noise_tables()
        chain = api.Chain(0, sobol, tile)
        ibl = _ibl(chain.postfx)
        sa = chain_util.shade_attribs(len(ibl.pre) - 1)
        scene = synth.Scene()
        out = {}
        for fi in range(frames):
            f = synth.make_frame(scene, fi, w, h, chain.device)
            g = dict(f)
            for k in ("base_color", "normal", "material", "depth", "motion", "prev_depth"):
                g[k] = lay(B.to_storage(f[k]))  # (4-channel planes in this build's storage: float16 in the native-storage build)
            ldr = lay(torch.empty(h, w, 4, device=chain.device, dtype=B.storage_dtype()), output=True)
            chain.execute(chain.bind_frame(fi, g, ibl, sa, ldr))
            out[f"ldr{fi}"] = _bits(ldr)
            out[f"taa{fi}"] = _bits(chain.effect_output("taa"))
        chain.close()
        return out

    return run


@pytest.mark.parametrize("size", SIZES)
def test_chain_layouts(mifx_lib, size):
    """Every caller plane of the chain's frames row-padded, 4 frames: the same images (and the same TAA history) as with contiguous planes."""
    w, h = size
    want = {}
    for kind in ("a", "b"):
        lay = Layout(kind)
        got = _chain_run()(lay, w, h)
        lay.check()
        if kind == "a":
            want = got
        else:
            for name in want:
                assert np.array_equal(got[name], want[name]), f"chain, row-padded planes {w}x{h}: {name} differs in {int((got[name] != want[name]).sum())} values"


CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {tests!r}]
import numpy as np, test_gpu_plane_layouts as T
res = {{}}
for kind in ("a", "b", "c"):
    lay = T.Layout(kind)
    res[kind] = T._chain_run()(lay, {w}, {h})
    lay.check()
for kind in ("b", "c"):
    for name, want in res["a"].items():
        assert np.array_equal(res[kind][name], want), (kind, name)
print("layouts OK")
"""


def test_chain_layouts_native_storage_build(mifx_lib):
    """The chain once more in the RGBA16_FLOAT storage build (libmifx_h4.so, in a child process): its 2-byte channels give other pitches and alignments."""
    import os
    import subprocess
    import sys

    from diligentfx_amd import binding as B

    if not os.path.exists(os.path.join(os.path.dirname(B.LIB_PATH), "libmifx_h4.so")):
        pytest.fail("libmifx_h4.so was not built")
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MIFX_STORAGE="h4")
    env.pop("MIFX_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=os.path.dirname(here), tests=here, w=67, h=37)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "layouts OK" in r.stdout, r.stderr[-3000:]
