"""The coordinate grid and axes on the GPU (grid.hip through the C ABI: mifx_coordinate_grid_render, mifx_copy_frame_render, mifx_chain_set_coordinate_grid).

Criteria (see tests/test_grid_cpu.py for where the numbers come from).  Against the reference fixture (tests/golden/grid_golden.npz): small cases within 1e-3, no value
left out; the window of a 3840x2160 frame within the fixture's `window_tolerance` T.  Device against the product's header compiled for the host on whole 3840x2160 and
7680x4320 frames: Coord and fwidth(Coord) bit for bit, the final RGBA within T -- the count of differing values and the largest difference are printed.  Chain: a frame
with the grid equals the chain's own Bloom output pushed through mifx_copy_frame_render bit for bit; overlap modes 0 and 5 agree; with selection + depth of field + auto
exposure; three in-library ranks equal the unsharded frame bit for bit; grid off equals the plain chain bit for bit; mifx_chain_execute_native with a grid is refused.
The frame-edge coverage guard only sees *_execute* entries, so the boundary sizes and the three plane layouts of the two new image-taking entries are covered here, with
the size lists and the layout harness of tests/test_gpu_frame_edges.py and tests/test_gpu_plane_layouts.py."""
import ctypes
import shutil
import threading

import numpy as np
import pytest
import torch

import grid_util as G
import test_grid_cpu as C
from test_gpu_frame_edges import COLLAPSE, ODD, THIN
from test_gpu_plane_layouts import SIZES, _same_in_every_layout
from util import blue_noise_tables

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 1e-3


@pytest.fixture(scope="module")
def host_lib():
    import os

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return C.build_host_lib(hipcc)


def _ctx():
    from diligentfx_amd import api

    sobol, tile = blue_noise_tables()
    return api.PostFXContext(0, sobol, tile)


def _cam(cam):
    from diligentfx_amd import binding as B

    return B.camera_from_bytes(cam.tobytes())


def _attribs(a):
    from diligentfx_amd import binding as B

    return B.CoordinateGridAttribs.from_buffer_copy(a.tobytes())


def _tm(words):
    from diligentfx_amd import binding as B

    return B.ToneMappingAttribs.from_buffer_copy(np.ascontiguousarray(words).tobytes())


def _dev(a, ctx):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _same(a, b):
    """Bit for bit.  (Where two axes cross their alphas add up beyond 1, lerp leaves a negative colour and LinearToSRGB of it is NaN -- in the reference as here; a NaN
    equals itself only bit-wise.)"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _render(ctx, depth, cam, attribs, flags, target=None, raw=True):
    from diligentfx_amd import api

    return api.CoordinateGridRenderer(ctx).render(depth, _cam(cam), _attribs(attribs) if attribs is not None else None, flags, color_target=target, raw=raw)


# ------------------------------------------------------------------------------------------------ 4. against the reference fixture
@pytest.mark.parametrize("i,name", C.golden_cases(("render",)))
def test_render_raw_and_blended_against_the_reference_fixture(mifx_lib, i, name):
    c = C.case(C.golden(), i)
    ctx = _ctx()
    depth = _dev(c["depth"], ctx)
    got = _render(ctx, depth, c["camera"], c["attribs"], c["flags"]).cpu().numpy()
    diff = np.abs(got - c["out"])
    print(f"{name}: device vs reference (raw): max {diff.max():.3e}, differing values {int((got != c['out']).sum())} of {got.size}")
    assert np.isfinite(got).all() and diff.max() <= TOL
    # blended into a colour target as BS_AlphaBlend does on rgb; the target's alpha stays
    rng = np.random.default_rng(i)
    dst = rng.uniform(0.0, 2.0, c["out"].shape).astype(F)
    target = _dev(dst, ctx)
    _render(ctx, depth, c["camera"], c["attribs"], c["flags"], target=target, raw=False)
    blended = target.cpu().numpy()
    want = G.blend(dst, c["out"])
    assert np.abs(blended - want).max() <= TOL and np.array_equal(blended[..., 3], dst[..., 3])
    assert not np.array_equal(blended, dst)
    ctx.close()


@pytest.mark.parametrize("i,name", C.golden_cases(("copy",)))
def test_copy_frame_against_the_reference_fixture(mifx_lib, i, name):
    c = C.case(C.golden(), i)
    ctx = _ctx()
    got = ctx.copy_frame(_dev(c["color"], ctx), _dev(c["depth"], ctx), _cam(c["camera"]), _tm(c["tone_mapping"]), float(c["ave_log_lum"]), int(c["tonemap_flags"]),
                         _attribs(c["attribs"]), c["flags"]).cpu().numpy()
    diff = np.abs(got - c["out"])
    print(f"{name}: device vs reference: max {diff.max():.3e}")
    assert np.isfinite(got).all() and diff.max() <= TOL
    ctx.close()


def test_window_of_a_4k_frame_against_the_reference_fixture(mifx_lib):
    g = C.golden()
    (i, _), = C.golden_cases(("window",))
    c = C.case(g, i)
    T = float(g["window_tolerance"])
    ctx = _ctx()
    h, w = c["depth"].shape
    depth = torch.full((c["H"], c["W"]), float(c["camera"][G.CAM_FAR_DEPTH]), device=ctx.device)  # (the fixture's window lies on the far plane, like the rest of the frame)
    depth[c["y0"]:c["y0"] + h, c["x0"]:c["x0"] + w] = _dev(c["depth"], ctx)
    got = _render(ctx, depth, c["camera"], c["attribs"], c["flags"])[c["y0"]:c["y0"] + h, c["x0"]:c["x0"] + w].cpu().numpy()
    diff = np.abs(got - c["out"])
    print(f"4K window: device vs reference: max {diff.max():.3e}, differing values {int((got != c['out']).sum())} of {got.size}; T = {T:.3e}")
    assert diff.max() <= T
    ctx.close()


def test_no_plane_or_axis_flag(mifx_lib):
    ctx = _ctx()
    cam = G.make_camera(64, 36, eye=(3.0, 2.5, -6.0), at=(0.0, 0.5, 0.0))
    depth = torch.ones(36, 64, device=ctx.device)
    a = G.default_attribs()
    for attribs, flags in ((a, 0), (a, G.FLAG_SRGB), (None, G.ALL)):
        target = torch.full((36, 64, 4), 0.25, device=ctx.device)
        raw = _render(ctx, depth, cam, attribs, flags, target=target, raw=True)
        assert not raw.any() and bool((target == 0.25).all())
    color = torch.rand(36, 64, 4, device=ctx.device) * 3.0
    from diligentfx_amd import binding as B

    tm = B.ToneMappingAttribs.default(4)
    want = ctx.tone_map(color, tm, 0.3, 1)
    for attribs, flags in ((_attribs(a), 0), (None, G.ALL)):
        assert torch.equal(ctx.copy_frame(color, None, None, tm, 0.3, 1, attribs, flags), want)  # the plain tone map, bit for bit; depth and camera are not read
    with pytest.raises(B.MifxError):
        ctx.copy_frame(color, depth, _cam(cam), tm, 0.3, 1, _attribs(a), 512)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. device against the host-compiled header on whole large frames
@pytest.mark.parametrize("W,H", [(3840, 2160), (7680, 4320)])
def test_device_against_the_host_header_on_whole_frames(mifx_lib, host_lib, W, H):
    T = float(C.golden()["window_tolerance"])
    ctx = _ctx()
    cam = G.make_camera(W, H, eye=(3.0, 2.5, -6.0), at=(0.0, 0.5, 0.0), jitter=(0.37 / W, -0.21 / H))
    a = G.default_attribs()
    rng = np.random.default_rng(W)
    depth_np = G.camera_z_to_depth(rng.uniform(0.5, 80.0, (H // 8, W // 8)), cam).repeat(8, 0).repeat(8, 1)  # 8x8 blocks of geometry at random distances
    depth = _dev(depth_np, ctx)
    n = 200_000
    xs = np.concatenate([rng.integers(0, W, n), np.arange(W), np.arange(W), np.zeros(H, np.int64), np.full(H, W - 1)]).astype(np.int32)
    ys = np.concatenate([rng.integers(0, H, n), np.zeros(W, np.int64), np.full(W, H - 1), np.arange(H), np.arange(H)]).astype(np.int32)
    d = np.ascontiguousarray(depth_np[ys, xs])
    ix, iy = torch.from_numpy(xs.astype(np.int64)).to(ctx.device), torch.from_numpy(ys.astype(np.int64)).to(ctx.device)
    for flag in (G.FLAG_YZ, G.FLAG_XZ, G.FLAG_XY):  # Coord and fwidth(Coord): no transcendental, every bit
        got = _render(ctx, depth, cam, a, flag | G.FLAG_DEBUG_COORD)[iy, ix].cpu().numpy()
        want = C.host_pixels(host_lib, W, H, xs, ys, d, d, cam, a, flag | G.FLAG_DEBUG_COORD)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{W}x{H} plane flag {flag}: Coord / fwidth values that differ from the host header: {bad} of {got.size}")
        assert bad == 0
    for flags in (G.FLAG_XZ | G.AXES, G.ALL):
        got = _render(ctx, depth, cam, a, flags)[iy, ix].cpu().numpy()
        want = C.host_pixels(host_lib, W, H, xs, ys, d, d, cam, a, flags)
        diff = np.abs(got - want)
        print(f"{W}x{H} flags {flags}: RGBA values that differ from the host header: {int((got != want).sum())} of {got.size}, largest difference {diff.max():.3e} (T = {T:.3e})")
        assert diff.max() <= T
    if W == 3840:  # the copy-frame kernel on the same frame: a black colour and no tone mapping leave grid.rgb * grid.a, with the depth range of the 3x3 neighbourhood
        from diligentfx_amd import binding as B

        lo, hi = (torch.nn.functional.max_pool2d(s * torch.nn.functional.pad(depth, (1, 1, 1, 1))[None, None], 3, 1)[0, 0] * s for s in (-1.0, 1.0))
        lo, hi = torch.minimum(lo, torch.ones_like(lo)), torch.maximum(hi, torch.zeros_like(hi))
        color = torch.zeros(H, W, 4, device=ctx.device)
        got = ctx.copy_frame(color, depth, _cam(cam), B.ToneMappingAttribs.default(0), 0.3, 0, _attribs(a), G.FLAG_XZ | G.AXES)[iy, ix].cpu().numpy()
        g = C.host_pixels(host_lib, W, H, xs, ys, np.ascontiguousarray(lo[iy, ix].cpu().numpy()), np.ascontiguousarray(hi[iy, ix].cpu().numpy()), cam, a, G.FLAG_XZ | G.AXES)
        want = (F(0) + g[:, 3:4] * (g[:, :3] - F(0))).astype(F)
        diff = np.abs(got[:, :3] - want)
        print(f"{W}x{H} copy frame: largest difference from the host header {diff.max():.3e}")
        assert diff.max() <= T and not got[:, 3].any()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the chain
def _chain_setup(w, h, n=4):
    from diligentfx_amd import api, synth

    sobol, tile = blue_noise_tables()
    env_chain = api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(env_chain.postfx, synth.make_sky_cube(32, env_chain.device), lut_size=64, irradiance_size=8, prefiltered_size=32, lut_samples=64,
                             diffuse_samples=128, specular_samples=32)
    sa = synth.make_lights()
    sa.PrefilteredCubeLastMip = float(len(ibl.pre) - 1)
    scene = synth.Scene()
    frames = [synth.make_frame(scene, i, w, h, env_chain.device) for i in range(n)]
    env_chain.close()
    return (sobol, tile), ibl, sa, frames


GRID_FLAGS = G.FLAG_XZ | G.AXES


def _grid():
    from diligentfx_amd import binding as B

    return B.CoordinateGridAttribs.default()


@pytest.mark.parametrize("variant", ["plain", "selection_dof_auto_exposure"])
def test_chain_frame_equals_copy_frame_on_its_own_bloom_output(mifx_lib, variant):
    from diligentfx_amd import api, binding as B

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames = _chain_setup(w, h)
    on, off = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    grid = _grid()
    on.set_coordinate_grid(grid, GRID_FLAGS)
    if variant != "plain":
        sel = torch.ones(h, w, device=on.device)
        sel[30:60, 50:90] = frames[0]["depth"][30:60, 50:90]
        s = B.SelectionAttribs.default(selection_id=5)
        s.nonselection_desaturation = 0.5
        for c in (on, off):
            c.set_selection(s, sel)
            c.set_depth_of_field(B.DOFAttribs.default(), 0)
            c.set_auto_exposure(True, 1.0 / 60.0, True)
    x, y = torch.zeros(h, w, 4, device=on.device), torch.zeros(h, w, 4, device=on.device)
    changed = False
    for i, f in enumerate(frames):
        on.execute(on.bind_frame(i, f, ibl, sa, x))
        off.execute(off.bind_frame(i, f, ibl, sa, y))
        torch.cuda.synchronize()
        bloom = on.effect_output("bloom")
        assert torch.equal(bloom, off.effect_output("bloom")), i  # (everything in front of the last pass is what the chain computes without the grid)
        ave = on.auto_exposure_average() if variant != "plain" else on.ave_log_lum
        want = on.postfx.copy_frame(bloom, f["depth"], f["camera"], on.tone_mapping, ave, on.tonemap_flags, grid, GRID_FLAGS)
        torch.cuda.synchronize()
        assert _same(x, want), (i, int((x.view(torch.int32) != want.view(torch.int32)).sum()))
        changed |= not _same(x, y)
    assert changed
    with pytest.raises(B.MifxError):
        on.execute_native(on.bind_frame(0, frames[0], ibl, sa, x), "RGBA8_UNORM_SRGB")
    # grid off again: the plain chain's output, bit for bit (the history is the plain chain's: the grid touches the last pass only)
    for k, (attribs, flags) in enumerate(((None, 0), (grid, GRID_FLAGS), (grid, G.FLAG_SRGB))):
        on.set_coordinate_grid(attribs, flags)
        f = frames[-1]
        on.execute(on.bind_frame(len(frames) + k, f, ibl, sa, x))
        off.execute(off.bind_frame(len(frames) + k, f, ibl, sa, y))
        torch.cuda.synchronize()
        assert _same(x, y) == (flags != GRID_FLAGS), k
    on.close()
    off.close()


def test_chain_overlap_modes_agree_with_the_grid_on(mifx_lib):
    from diligentfx_amd import api

    w, h = 208, 120
    (sobol, tile), ibl, sa, frames = _chain_setup(w, h)
    m0, m5 = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    m5.set_overlap(5)
    for c in (m0, m5):
        c.set_coordinate_grid(_grid(), GRID_FLAGS)
    x, y = torch.zeros(h, w, 4, device=m0.device), torch.zeros(h, w, 4, device=m0.device)
    for i, f in enumerate(frames):
        m0.execute(m0.bind_frame(i, f, ibl, sa, x))
        m5.execute(m5.bind_frame(i, f, ibl, sa, y))
        torch.cuda.synchronize()
        assert _same(x, y), i
    m0.close()
    m5.close()


@pytest.mark.parametrize("auto_exposure", [False, True])
def test_three_in_library_ranks_equal_the_unsharded_chain(mifx_lib, auto_exposure):
    from diligentfx_amd import api

    w, h, world = 320, 192, 3
    cuts = [0, 70, 131, h]
    (sobol, tile), ibl, sa, frames = _chain_setup(w, h)
    ref = api.Chain(0, sobol, tile)
    max_motion = int(max(float(f["motion"][..., 1].abs().max()) for f in frames) * 0.5 * h) + 2
    chains = [api.Chain(0, sobol, tile) for _ in range(world)]
    comms = api.Comm.local_group(chains[0].postfx, world)
    for c in chains + [ref]:
        c.set_coordinate_grid(_grid(), GRID_FLAGS)
        if auto_exposure:
            c.set_auto_exposure(True, 1.0 / 60.0, True)
    for r in range(world):
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
            assert _same(outs[r][b:e], want[b:e]), (i, r)
    for r in range(world):
        chains[r].set_sharding(None)
    for c in comms:
        c.close()
    for c in chains + [ref]:
        c.close()


# ------------------------------------------------------------------------------------------------ 7. boundary sizes and plane layouts (what the coverage guard cannot see)
def _edge_inputs(w, h, seed):
    cam = G.make_camera(w, h, eye=(3.0, 2.5, -6.0), at=(0.0, 0.5, 0.0), jitter=(0.2 / w, -0.3 / h))
    rng = np.random.default_rng(seed)
    depth = G.camera_z_to_depth(rng.uniform(1.0, 60.0, (h, w)), cam)
    depth[rng.random((h, w)) < 0.4] = 1.0
    color = rng.uniform(0.0, 3.0, (h, w, 4)).astype(F)
    return cam, depth, color


@pytest.mark.parametrize("size", THIN + ODD + COLLAPSE)
def test_render_and_copy_frame_edges(mifx_lib, host_lib, size):
    """Both entries at the boundary frame sizes against the product's header compiled for the host (held to the reference by tests/test_grid_cpu.py), 1e-3, none left out."""
    from diligentfx_amd import binding as B

    w, h = size
    cam, depth, color = _edge_inputs(w, h, w * 131 + h)
    a = G.default_attribs()
    ctx = _ctx()
    got = _render(ctx, _dev(depth, ctx), cam, a, G.ALL).cpu().numpy()
    assert np.abs(got - C.host_render(host_lib, depth, cam, a, G.ALL)).max() <= TOL
    dst = _dev(color, ctx)
    _render(ctx, _dev(depth, ctx), cam, a, G.ALL, target=dst, raw=False)
    assert np.abs(dst.cpu().numpy() - G.blend(color, got)).max() <= TOL
    words = np.frombuffer(bytes(B.ToneMappingAttribs.default(4)), np.uint32)
    c = dict(color=color, depth=depth, camera=cam, tone_mapping=words, ave_log_lum=0.3, tonemap_flags=1, attribs=a, flags=G.FLAG_XZ | G.FLAG_AXIS_X)
    got = ctx.copy_frame(_dev(color, ctx), _dev(depth, ctx), _cam(cam), _tm(words), 0.3, 1, _attribs(a), c["flags"]).cpu().numpy()
    assert np.abs(got - C.host_copy_frame(host_lib, c)).max() <= TOL
    ctx.close()


@pytest.mark.parametrize("size", SIZES)
def test_render_and_copy_frame_layouts(mifx_lib, size):
    from diligentfx_amd import binding as B

    def run(lay, w, h):
        cam, depth, color = _edge_inputs(w, h, 7)
        a = G.default_attribs()
        ctx = _ctx()
        out = {}
        raw = lay(torch.zeros(h, w, 4, device=ctx.device), output=True)
        target = lay(torch.zeros(h, w, 4, device=ctx.device), output=True)
        target.copy_(_dev(color, ctx))
        d, t, o = B.image(lay(_dev(depth, ctx))), B.image(target), B.image(raw)
        B.check(ctx.lib.mifx_coordinate_grid_render(ctx.handle, ctypes.byref(d), ctypes.byref(_cam(cam)), ctypes.byref(_attribs(a)), ctypes.c_uint32(G.ALL), ctypes.byref(t),
                                                    ctypes.byref(o)))
        out["raw"], out["blended"] = raw.clone(), target.clone()
        ldr = lay(torch.zeros(h, w, 4, device=ctx.device), output=True)
        ctx.copy_frame(lay(_dev(color, ctx)), lay(_dev(depth, ctx)), _cam(cam), B.ToneMappingAttribs.default(4), 0.3, 1, _attribs(a), G.ALL, out=ldr)
        out["copy_frame"] = ldr.clone()
        assert bool(out["raw"][..., 3].any())
        torch.cuda.synchronize()
        ctx.close()
        return out

    _same_in_every_layout(run, *size)
