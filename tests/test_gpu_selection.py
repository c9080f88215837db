"""The selection outline on the GPU (selection.hip, composite.hip's selection instance, mifx_chain_set_selection) against the float32 restatement of the reference
(tests/selection_util.py): the jump-flood plane bit for bit, the selection composite on the GPU's own composite, and the chain's frames."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import selection_util as S
from util import assert_close, blue_noise_tables

pytestmark = pytest.mark.gpu
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _selection_inputs(w, h, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.1, 0.9, (h, w)).astype(F)
    sel = S.make_selection_depth(depth, rng, seeds=8, max_radius=max(2, min(w, h) // 20))
    sel[0, rng.integers(0, w)] = depth[0, 0]  # (seeds on the frame's first row and column: the truncation rule of the taps)
    sel[rng.integers(0, h), 0] = depth[0, 0]
    sel[h - 1, w - 1] = depth[h - 1, w - 1]
    return depth, sel


def _jump_flood_plane(w, h, max_distance, seed):
    """This process' library: the plane of mifx_selection_execute (numpy), and the inputs."""
    import torch

    from diligentfx_amd import api, binding as B

    depth, sel = _selection_inputs(w, h, seed)
    ctx = api.PostFXContext(0)
    fx = api.ProcessSelection(ctx)
    a = B.SelectionAttribs.default(selection_id=7)
    a.max_distance = max_distance
    sd = torch.from_numpy(sel).to(ctx.device)
    fx.execute(sd, a)
    torch.cuda.synchronize()
    got = fx.get_output().cpu().numpy().copy()
    fx.close()
    ctx.close()
    return got, sel


@pytest.mark.parametrize("w,h", [(31, 17), (230, 150), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("max_distance", [1.0, 4.0, 16.0, 100.0])
def test_jump_flood_plane_equals_the_restatement(mifx_lib, w, h, max_distance):
    got, sel = _jump_flood_plane(w, h, max_distance, w + h)
    want = S.jump_flood(sel, 1.0, max_distance)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())
    assert bad == 0, f"{bad} texels differ"
    assert (want[..., 1] > 0.25).any()


def test_empty_selection_and_reversed_depth(mifx_lib):
    import torch

    from diligentfx_amd import api, binding as B

    w, h = 96, 64
    depth, sel = _selection_inputs(w, h, 3)
    ctx = api.PostFXContext(0)
    fx = api.ProcessSelection(ctx)
    a = B.SelectionAttribs.default(selection_id=1)
    fx.execute(torch.from_numpy(sel).to(ctx.device), a)
    assert fx.get_output().abs().sum() > 0
    a.selection_id = 0  # nothing selected: the plane is cleared
    fx.execute(torch.from_numpy(sel).to(ctx.device), a)
    assert not fx.get_output().any()
    rev = np.where(sel == F(1.0), F(0.0), sel).astype(F)  # (reversed depth: the clear value is 0)
    a = B.SelectionAttribs.default(selection_id=1, clear_depth=0.0)
    fx.execute(torch.from_numpy(rev).to(ctx.device), a)
    got = fx.get_output().cpu().numpy()
    assert np.array_equal(got, S.jump_flood(rev, 0.0, 4.0)) and np.array_equal(got, S.jump_flood(sel, 1.0, 4.0))
    fx.close()
    ctx.close()


H4_SCRIPT = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
from test_gpu_selection import _jump_flood_plane
got, _ = _jump_flood_plane(230, 150, 16.0, 5)
np.save({out!r}, got)
"""


def test_native_storage_build_gives_the_same_plane(mifx_lib, tmp_path):
    from diligentfx_amd import binding as B

    if not os.path.exists(os.path.join(os.path.dirname(B.LIB_PATH), "libmifx_h4.so")):
        pytest.fail("libmifx_h4.so was not built")
    got, _ = _jump_flood_plane(230, 150, 16.0, 5)
    out = str(tmp_path / "h4.npy")
    env = dict(os.environ, MIFX_STORAGE="h4")
    env.pop("MIFX_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", H4_SCRIPT.format(root=ROOT, tests=HERE, out=out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.array_equal(np.load(out).view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("tm_mode", [0, 4])
def test_selection_composite_equals_the_restatement_on_the_composite(mifx_lib, tm_mode):
    selection_composite(tm_mode)


def selection_composite(tm_mode, size=(150, 90), edge=False):
    """The composite with the selection tail against the restatement at any frame size (edge: the frame may be too small for the tail to change a texel)."""
    import torch

    from diligentfx_amd import api, binding as B, synth

    w, h = size
    ctx = api.PostFXContext(0)
    f = synth.make_frame(synth.Scene(), 2, w, h, ctx.device)
    ibl = api.precompute_ibl(ctx, synth.make_sky_cube(16, ctx.device), lut_size=32, irradiance_size=8, prefiltered_size=16, lut_samples=32, diffuse_samples=64,
                             specular_samples=16)
    gen = torch.Generator(device="cpu").manual_seed(11)
    rnd = lambda *s: torch.rand(*s, generator=gen).to(ctx.device)  # noqa: E731
    color = torch.cat([rnd(h, w, 3) * 3.0, f["base_color"][..., 3:4]], -1).contiguous()
    spec, ssr, ssao = rnd(h, w, 4), rnd(h, w, 4), rnd(h, w)
    tm = B.ToneMappingAttribs.default(tm_mode) if tm_mode else None
    args = (ctx, color, spec, ssr, ssao, f["normal"], f["base_color"], f["material"], ibl.lut, f["camera"])
    plain = api.composite(*args, 0.9, 0.8, tone_mapping=tm, ave_log_lum=0.3).cpu().numpy()
    depth = f["depth"].cpu().numpy()
    sel = S.make_selection_depth(depth, np.random.default_rng(4), seeds=5, max_radius=10)
    fx = api.ProcessSelection(ctx)
    a = B.SelectionAttribs.default(selection_id=2)
    a.nonselection_desaturation, a.outline_width = 0.4, 5.0
    sd = torch.from_numpy(sel).to(ctx.device)
    fx.execute(sd, a)
    closest = fx.get_output()
    got = api.composite_selection(*args, f["depth"], sd, closest, a, 0.9, 0.8, tone_mapping=tm, ave_log_lum=0.3).cpu().numpy()
    cl = closest.cpu().numpy()
    want = S.composite_tail(plain, depth, sel, cl, list(a.outline_color)[:3], list(a.occluded_outline_color)[:3], 0.4, 1.0, 5.0)
    assert_close(got, want, what=f"selection composite tm={tm_mode}")
    assert edge or not np.array_equal(got, plain)
    fx.close()
    ctx.close()


def _chain_setup(w, h):
    import torch

    from diligentfx_amd import api, synth

    sobol, tile = blue_noise_tables()
    env_chain = api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(env_chain.postfx, synth.make_sky_cube(32, env_chain.device), lut_size=64, irradiance_size=8, prefiltered_size=32, lut_samples=64,
                             diffuse_samples=128, specular_samples=32)
    sa = synth.make_lights()
    sa.PrefilteredCubeLastMip = float(len(ibl.pre) - 1)
    scene = synth.Scene()
    frames = [synth.make_frame(scene, i, w, h, env_chain.device) for i in range(4)]
    env_chain.close()
    return (sobol, tile), ibl, sa, frames, torch


def _chain_selection(frames, clear_everywhere=False):
    import torch

    from diligentfx_amd import binding as B

    depth = frames[0]["depth"].cpu().numpy()
    sel = np.ones_like(depth) if clear_everywhere else S.make_selection_depth(depth, np.random.default_rng(9), seeds=6, max_radius=12)
    a = B.SelectionAttribs.default(selection_id=11)
    a.nonselection_desaturation = 0.0 if clear_everywhere else 0.5
    return a, torch.from_numpy(sel.astype(F)).to(frames[0]["depth"].device), sel


def test_chain_with_a_clear_selection_and_no_desaturation_is_bit_identical(mifx_lib):
    from diligentfx_amd import api

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames, torch = _chain_setup(w, h)
    on, off = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    a, sd, _ = _chain_selection(frames, clear_everywhere=True)
    on.set_selection(a, sd)
    x, y = torch.zeros(h, w, 4, device=on.device), torch.zeros(h, w, 4, device=on.device)
    for i, f in enumerate(frames):
        on.execute(on.bind_frame(i, f, ibl, sa, x))
        off.execute(off.bind_frame(i, f, ibl, sa, y))
        assert torch.equal(x, y), i
        assert torch.equal(on.effect_output("taa"), off.effect_output("taa")), i
    assert not on.effect_output("selection").any()
    on.close()
    off.close()


@pytest.mark.parametrize("tm_mode", [4, 0])
def test_chain_frame_one_equals_the_restatement_on_the_selection_off_taa_output(mifx_lib, tm_mode):
    """TAA's first frame is a copy of the composite (the placeholder frame, include/mifx.h), so the selection-on TAA output of frame 1 is the restatement's tail on the
    selection-off one, with the outline colours converted by ReverseExpToneMap when the frame is tone-mapped (HnPostProcessTask.cpp:843-850)."""
    from diligentfx_amd import api, binding as B

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames, torch = _chain_setup(w, h)
    on, off = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    for c in (on, off):
        c.tone_mapping = B.ToneMappingAttribs.default(tm_mode)
    a, sd, sel = _chain_selection(frames)
    on.set_selection(a, sd)
    x, y = torch.zeros(h, w, 4, device=on.device), torch.zeros(h, w, 4, device=on.device)
    on.execute(on.bind_frame(0, frames[0], ibl, sa, x))
    off.execute(off.bind_frame(0, frames[0], ibl, sa, y))
    got, base = on.effect_output("taa").cpu().numpy(), off.effect_output("taa").cpu().numpy()
    closest = on.effect_output("selection").cpu().numpy()
    assert np.array_equal(closest, S.jump_flood(sel, 1.0, 4.0))
    hdr = api.ProcessSelection.hdr_colors(a, on.tone_mapping if tm_mode else None, on.ave_log_lum)
    if tm_mode:
        assert list(hdr.outline_color)[:3] != list(a.outline_color)[:3]
    want = S.composite_tail(base, frames[0]["depth"].cpu().numpy(), sel, closest, list(hdr.outline_color)[:3], list(hdr.occluded_outline_color)[:3],
                            a.nonselection_desaturation, 1.0, a.outline_width)
    assert_close(got, want, what=f"chain frame 1 tm={tm_mode}")
    assert not np.array_equal(got, base)
    on.close()
    off.close()


def test_chain_overlap_modes_agree_with_selection_on(mifx_lib):
    from diligentfx_amd import api

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames, torch = _chain_setup(w, h)
    m0, m5 = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    m5.set_overlap(5)
    a, sd, _ = _chain_selection(frames)
    for c in (m0, m5):
        c.set_selection(a, sd)
    x, y = torch.zeros(h, w, 4, device=m0.device), torch.zeros(h, w, 4, device=m0.device)
    for i, f in enumerate(frames):
        m0.execute(m0.bind_frame(i, f, ibl, sa, x))
        m5.execute(m5.bind_frame(i, f, ibl, sa, y))
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    assert torch.equal(m0.effect_output("taa"), m5.effect_output("taa"))
    m0.close()
    m5.close()


def test_changing_the_selected_prim_resets_taa(mifx_lib):
    from diligentfx_amd import api

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames, torch = _chain_setup(w, h)
    changed, reset, kept = (api.Chain(0, sobol, tile) for _ in range(3))
    a, sd, _ = _chain_selection(frames)
    for c in (changed, reset, kept):
        c.set_selection(a, sd)
    outs = {}
    for i, f in enumerate(frames):
        for name, c in (("changed", changed), ("reset", reset), ("kept", kept)):
            if i == len(frames) - 1:
                if name == "changed":
                    b = type(a).from_buffer_copy(bytes(a))
                    b.selection_id = a.selection_id + 1
                    c.set_selection(b, sd)
                c.taa_attribs.ResetAccumulation = 1 if name == "reset" else 0
            o = torch.zeros(h, w, 4, device=c.device)
            c.execute(c.bind_frame(i, f, ibl, sa, o))
            outs[name] = c.effect_output("taa").clone()
    assert torch.equal(outs["changed"], outs["reset"])
    assert not torch.equal(outs["changed"], outs["kept"])
    for c in (changed, reset, kept):
        c.close()


def test_three_in_library_ranks_equal_the_unsharded_chain(mifx_lib):
    from diligentfx_amd import api

    w, h, world = 320, 192, 3
    cuts = [0, 70, 131, h]
    (sobol, tile), ibl, sa, frames, torch = _chain_setup(w, h)
    a, sd, _ = _chain_selection(frames)
    ref = api.Chain(0, sobol, tile)
    ref.set_selection(a, sd)
    max_motion = int(max(float(f["motion"][..., 1].abs().max()) for f in frames) * 0.5 * h) + 2
    chains = [api.Chain(0, sobol, tile) for _ in range(world)]
    comms = api.Comm.local_group(chains[0].postfx, world)
    for r in range(world):
        chains[r].set_selection(a, sd)
        chains[r].set_sharding(comms[r], cuts, max_motion)
    outs = [torch.zeros(h, w, 4, device=ref.device) for _ in range(world)]
    streams = [torch.cuda.Stream(device=ref.device) for _ in range(world)]
    want = torch.zeros(h, w, 4, device=ref.device)
    errors = []
    for i, f in enumerate(frames):
        ref.execute(ref.bind_frame(i, f, ibl, sa, want))
        torch.cuda.synchronize()

        def run(r):
            try:
                with torch.cuda.stream(streams[r]):
                    chains[r].execute_sharded(chains[r].bind_frame(i, f, ibl, sa, outs[r]))
                streams[r].synchronize()
            except Exception as e:  # noqa: BLE001
                errors.append((r, repr(e)))

        threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not errors, errors
        for r in range(world):
            b, e = cuts[r], cuts[r + 1]
            assert torch.equal(outs[r][b:e], want[b:e]), (i, r)
    for r in range(world):
        chains[r].set_sharding(None)
    for c in comms:
        c.close()
    for c in chains + [ref]:
        c.close()
