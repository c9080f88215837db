"""TAA's history skip (csrc/taa.hip "History skip"): a pixel whose motion factor is exactly 0 stores its current colour without fetching the history or
the previous depth.  Bit identity with the kernel that runs its whole body for every pixel.

Two TemporalAntiAliasing objects on one PostFXContext get the same inputs frame by frame: `ref` with the switch off (mifx_debug_taa_set_history_skip 0) and `dut` as
created.  The accumulated frame is compared as integers after every frame (no tolerance, NaN-safe); each object accumulates onto its own history, so an error compounds.
The motion is written straight into the closest-motion plane the kernel reads, and every case checks on the host, with the kernel's own expression in float32, that the
pattern makes the share of skipped pixels it is meant to make."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import ROOT, blue_noise_tables

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 8), (33, 17), (67, 37), (129, 65), (131, 77), (300, 12)]  # partial 32x8 blocks, one-row tails, a frame thinner than a block
PATTERNS = ("zero", "fast", "checker", "blocks", "blocks_off1", "threshold", "below_threshold", "leaves", "synth")
FRAMES = 7  # frame 0 is the placeholder copy of a new object (no kernel); frames 1 - 6 run the kernel
RESET_FRAME = 3
f32 = np.float32


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def motion_factor(m, cam):
    """taa.hip motion_factor(), operation by operation in float32 (the library is built without contraction, with correctly rounded sqrt).  m: (h, w, 2) float32."""
    vw, vh, ivw, ivh = (f32(v) for v in cam.f4ViewportSize)
    mx, my = m[..., 0] * f32(0.5), m[..., 1] * f32(-0.5)
    ax = mx * (vw * ivh)
    return np.clip(f32(1.0) - np.sqrt(ax * ax + my * my) * f32(256.0), f32(0.0), f32(1.0))


def prev_position(m, cam):
    vw, vh = f32(cam.f4ViewportSize[0]), f32(cam.f4ViewportSize[1])
    h, w = m.shape[:2]
    x, y = np.arange(w, dtype=f32)[None, :] + f32(0.5), np.arange(h, dtype=f32)[:, None] + f32(0.5)
    return x - (m[..., 0] * f32(0.5)) * vw, y - (m[..., 1] * f32(-0.5)) * vh


def inside(m, cam):
    px, py = prev_position(m, cam)
    return (px >= 0) & (py >= 0) & (px < f32(cam.f4ViewportSize[0])) & (py < f32(cam.f4ViewportSize[1]))


def pattern(kind, w, h, half=False):
    """(motion plane (h, w, 2) or None for the frame's own, what the share of pixels with motionFactor == 0 must be as (lo, hi), the same for `inside`).
    half: the plane stores binary16 (the native-storage build): \"one ulp below\" is then one binary16 ulp."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    # 1.5 px to the left / up per frame: the motion factor is 0 from h / 256 px on, at most 0.31 px at these sizes; the previous position stays inside except at the border
    fast = np.stack([np.full((h, w), 3.0 / w, f32), np.full((h, w), -3.0 / h, f32)], -1)
    zero = np.zeros((h, w, 2), f32)
    line = max(w, h) / (w * h)  # one row or one column of the frame
    if kind == "zero":
        return zero, (0.0, 0.0), (1.0, 1.0)
    if kind == "fast":
        return fast, (1.0, 1.0), (0.5, 1.0)
    if kind == "checker":  # every wave diverges
        return np.where(((xx + yy) % 2 == 0)[..., None], fast, zero), (0.5 - line, 0.5 + line), (0.5, 1.0)
    if kind in ("blocks", "blocks_off1"):  # the 32x2 footprint of a wave, and the same one pixel off in both directions
        o = 1 if kind == "blocks_off1" else 0
        sel = (((xx + o) // 32 + (yy + o) // 2) % 2 == 0)[..., None]
        # (0.5 exactly at 8x8, 9x8 and 300x12, 0.526 - 0.528 at 33x17, 0.5001 - 0.5006 at the other sizes: inside one row or column everywhere)
        return np.where(sel, fast, zero), (0.5 - line, 0.5 + line), (0.5, 1.0)
    if kind == "threshold":  # 1 - (0.5 / 128) * 256 = 0 exactly
        m = zero.copy()
        m[..., 1] = 1.0 / 128.0
        return m, (1.0, 1.0), (0.5, 1.0)
    if kind == "below_threshold":  # one ulp below: sqrt((2^-8 (1 - 2^-24))^2) = 2^-8 (1 - 2^-24), the factor is 2^-24 (2^-11 for a binary16 ulp): the whole body
        m = zero.copy()
        m[..., 1] = f32(np.nextafter(np.float16(1.0 / 128.0), np.float16(0.0))) if half else np.nextafter(f32(1.0 / 128.0), f32(0.0))
        return m, (0.0, 0.0), (0.5, 1.0)
    if kind == "leaves":  # two frame widths per frame: the `!inside` exit wins everywhere
        m = zero.copy()
        m[..., 0] = 4.0
        return m, (1.0, 1.0), (0.0, 0.0)
    assert kind == "synth"
    # The orbit's own motion: 0.35 - 0.43 of the closest-motion plane's pixels from 33x17 up (counted with the CPU checker's plane for frames 1 - 6 of every size
    # here), held to 0.3 - 0.6.  The scene itself, not the kernel, gives 0.27 - 0.35 at 8x8 / 9x8 (17 - 25 pixels) and 0.64 in the 12-row strip, which sees the
    # fast-moving ground only: those three frames are held to 0.2 - 0.7 -- both paths run in every frame either way.
    return None, ((0.3, 0.6) if w * h >= 33 * 17 and h >= 17 else (0.2, 0.7)), (0.5, 1.0)


def colour_of(f):
    return torch.cat([f["base_color"][..., :3] * 2.0 + 0.05 * f["normal"][..., :3].abs(), f["base_color"][..., 3:4]], -1).contiguous()


def pitched(t):
    """`t` as a view two rows and one column inside a wider, taller parent filled with NaN."""
    h, w = t.shape[:2]
    parent = torch.full((h + 3, w + 5, *t.shape[2:]), float("nan"), dtype=t.dtype, device=t.device)
    view = parent[2:2 + h, 1:1 + w]
    view.copy_(t)
    assert not view.is_contiguous()
    return view


class Pair:
    def __init__(self, api, ctx, flags, skip_rejection):
        self.ref, self.dut = api.TemporalAntiAliasing(ctx), api.TemporalAntiAliasing(ctx)
        self.ref.set_history_skip(False)
        self.flags, self.skip_rejection = flags, skip_rejection

    def close(self):
        self.ref.close()
        self.dut.close()


def run_patterns(w, h, patterns, flag_sets, skip_rejections=(0, 1), layout=None):
    """Every (pattern, flag set, SkipRejection) as a pair of objects of its own, all on one context: per frame the context runs once, each pattern is written into the
    closest-motion plane in turn and its pairs execute and are compared."""
    from diligentfx_amd import api, binding as B, synth

    sobol, tile = blue_noise_tables()
    ctx = api.PostFXContext(0, sobol, tile)
    scene = synth.Scene()
    pairs = {(p, fl, sr): Pair(api, ctx, fl, sr) for p in patterns for fl in flag_sets for sr in skip_rejections}
    half = ctx.lib.mifx_storage_mode() == 1
    differed = 0
    for frame in range(FRAMES):
        f = synth.make_frame(scene, frame, w, h, ctx.device)
        color = B.to_storage(colour_of(f))
        if layout is not None:
            color = layout(color)
        ctx.prepare_resources(frame, w, h)
        for p in pairs.values():
            p.ref.prepare_resources(p.flags)
            p.dut.prepare_resources(p.flags)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        plane = ctx.get_closest_motion_vectors()
        own = plane.clone()
        for kind in patterns:
            m, dead_share, inside_share = pattern(kind, w, h, half)
            plane.copy_(own if m is None else torch.from_numpy(m).to(ctx.device))
            if frame > 0:
                host = api.widen(plane).float().cpu().numpy()
                dead, ins = (motion_factor(host, f["camera"]) == 0).mean(), inside(host, f["camera"]).mean()
                assert dead_share[0] <= dead <= dead_share[1], f"{kind} {w}x{h} frame {frame}: {dead:.3f} of the pixels have a zero motion factor, meant {dead_share}"
                assert inside_share[0] <= ins <= inside_share[1], f"{kind} {w}x{h} frame {frame}: {ins:.3f} of the previous positions are inside, meant {inside_share}"
            for (pk, flags, sr), p in pairs.items():
                if pk != kind:
                    continue
                a = B.TAAAttribs.default()
                a.SkipRejection, a.ResetAccumulation = sr, 1 if frame == RESET_FRAME else 0
                sa, sb = p.ref.execute(color, a), p.dut.execute(color, a)
                ra, rb = bits(p.ref.get_accumulated_frame()), bits(p.dut.get_accumulated_frame())
                assert sa == sb and torch.equal(ra, rb), f"{kind} {w}x{h} flags {flags} SkipRejection {sr} frame {frame}: {int((ra != rb).sum())} values differ"
                differed += int(not torch.equal(ra, bits(color)))
    assert differed > 0, "the accumulated frame never differed from the colour: no history was blended"
    for p in pairs.values():
        p.close()
    ctx.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_history_skip_bit_identical(mifx_lib, size):
    """Every motion pattern, TAA flag set 0 - 7, SkipRejection 0 and 1 (nothing is skipped there: equal trivially, and it must stay so), ResetAccumulation on frame 3."""
    run_patterns(*size, PATTERNS, range(8))


def test_history_skip_on_a_pitched_row_offset_colour_plane(mifx_lib):
    run_patterns(67, 37, ("checker", "blocks_off1", "synth"), (2, 7), (0,), layout=pitched)


# ------------------------------------------------------------------------------------------------ the skipped taps are really not read
def _independence_run(switch_on, poison, flags):
    """Frames 0 - 2 build a history; frame 3 has a still left part and a right part that moves 12.25 px to the right per frame.  Before frame 3 executes, every history and
    previous-depth texel that only skipped pixels can reach is overwritten with `poison`: the complement of the 7x7 neighbourhoods (the bicubic taps lie within 3 texels
    of int(PrevPosition), the depth taps within 1) of the previous positions of the pixels that take the whole body.  Returns the bits of frame 3."""
    from diligentfx_amd import api, binding as B, synth

    w, h = 67, 37
    sobol, tile = blue_noise_tables()
    ctx = api.PostFXContext(0, sobol, tile)
    taa = api.TemporalAntiAliasing(ctx)
    taa.set_history_skip(switch_on)
    scene = synth.Scene()
    out = None
    for frame in range(4):
        f = synth.make_frame(scene, frame, w, h, ctx.device)
        ctx.prepare_resources(frame, w, h)
        taa.prepare_resources(flags)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        if frame == 3:
            m = np.zeros((h, w, 2), f32)
            m[:, 34:, 0] = -24.5 / w
            plane = ctx.get_closest_motion_vectors()
            plane.copy_(torch.from_numpy(m).to(ctx.device))
            host = plane.float().cpu().numpy()
            dead = (motion_factor(host, f["camera"]) == 0) & inside(host, f["camera"])
            alive = ~(motion_factor(host, f["camera"]) == 0) & inside(host, f["camera"])
            px, py = prev_position(host, f["camera"])
            reach = np.zeros((h, w), bool)
            reach[py[alive].astype(np.int32), px[alive].astype(np.int32)] = True
            reach = torch.nn.functional.max_pool2d(torch.from_numpy(reach)[None, None].float(), 7, 1, 3)[0, 0] > 0
            only_dead = (~reach).to(ctx.device)
            # the test sees something: skipped pixels exist whose taps all lie in the overwritten set, and the set leaves the other pixels' taps alone
            dx, dy = px[dead].astype(np.int32), py[dead].astype(np.int32)
            assert dead.sum() >= 0.25 * w * h and alive.sum() >= 0.25 * w * h and bool(only_dead.cpu().numpy()[dy, dx].any())
            if poison is not None:
                taa.get_accumulated_frame(is_prev_frame=True)[only_dead] = poison
                ctx.get_previous_depth()[only_dead] = poison
        taa.execute(colour_of(f), B.TAAAttribs.default())
        out = bits(taa.get_accumulated_frame()).clone()
    taa.close()
    ctx.close()
    return out


@pytest.mark.parametrize("flags", [0, 2])
def test_history_skip_does_not_read_what_only_skipped_pixels_reach(mifx_lib, flags):
    """NaN, a large finite value and +inf behind the skipped pixels leave every bit of the frame alone.  That the overwritten texels are the ones those pixels tap shows
    with the whole body everywhere and +inf under the bilinear filter (flags 0: positive weights, inf stays inf, and 0 * inf is NaN).  A NaN cannot show it: the
    kernel's max(history, 0) returns 0 for a NaN, as fmaxf does, and so does the sum of infinities under the bicubic filter's weights of both signs -- a finite history
    at zero weight then changes nothing, which is the premise."""
    clean = _independence_run(True, None, flags)
    assert torch.equal(clean, _independence_run(False, None, flags))
    for poison in (float("nan"), 3.0e38, float("inf")):
        assert torch.equal(clean, _independence_run(True, poison, flags)), f"{poison} behind skipped pixels only changed the frame"
    if flags == 0:
        assert not torch.equal(clean, _independence_run(False, float("inf"), flags)), "with the whole body everywhere the +inf must show: the overwritten texels are not the ones those pixels tap"


# ------------------------------------------------------------------------------------------------ the chain
def _chain_case(w, h, mask):
    import chain_util
    from diligentfx_amd import api, binding as B, synth

    dev = torch.device("cuda", 0)
    sobol, tile = blue_noise_tables()
    scene = synth.Scene()
    chains = [api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)]
    chains[0].effect("taa").set_history_skip(False)
    for c in chains:
        c.set_fusion_mask(mask)
    ibls = [api.precompute_ibl(c.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32, lut_samples=32, diffuse_samples=32,
                               specular_samples=16) for c in chains]
    shade = chain_util.shade_attribs(len(ibls[0].pre) - 1)
    outs = [torch.zeros(h, w, 4, device=dev, dtype=B.storage_dtype()) for _ in chains]
    shares = []
    for fi in range(6):
        g = synth.make_frame(scene, fi, w, h, dev)
        for c, ibl, o in zip(chains, ibls, outs):
            c.execute(c.bind_frame(fi, g, ibl, shade, o))
        torch.cuda.synchronize()
        if fi > 0:
            shares.append(float((motion_factor(api.widen(chains[1].postfx.get_closest_motion_vectors()).float().cpu().numpy(), g["camera"]) == 0).mean()))
    assert all(0.3 <= s <= 0.6 for s in shares), f"share of pixels with a zero motion factor per frame: {shares}"
    assert torch.equal(bits(outs[0]), bits(outs[1])), f"{w}x{h} fusion mask {mask:#x}: the final frames differ"
    a, b = (bits(c.effect("taa").get_accumulated_frame()) for c in chains)
    assert torch.equal(a, b), f"{w}x{h} fusion mask {mask:#x}: the TAA histories differ in {int((a != b).sum())} values"
    for c in chains:
        c.close()


@pytest.mark.parametrize("mask", [0x1F, 0x3F], ids=hex)
@pytest.mark.parametrize("size", [(67, 37), (176, 100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_history_skip_through_the_chain(mifx_lib, size, mask):
    """The chain's TAA follows its effect object's switch: six frames, on against off, the final frame and the TAA history bit for bit; with fusion bit 5 the
    COMPOSITE = true instance of the kernel runs."""
    _chain_case(*size, mask)


# ------------------------------------------------------------------------------------------------ the native-storage build (the same source under MIFX_STORAGE_H4)
H4_PARTS = {"patterns_small": SIZES[:4], "patterns_large": SIZES[4:], "chain": None}


@pytest.mark.parametrize("part", list(H4_PARTS))
def test_history_skip_native_storage_build(mifx_lib, part):
    """The storage mode is a property of the loaded library: the two-object comparison (every size, pattern, flag set and SkipRejection, as above) and the chain
    comparison (both sizes, fusion masks 0x1F and 0x3F: the COMPOSITE = true instance fills its tile through the RGBA16_FLOAT rounding) run in processes of their own
    with MIFX_STORAGE=h4."""
    from diligentfx_amd import build

    if not os.path.exists(build.OUT_H4):
        pytest.skip("libmifx_h4.so is not built")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), part], cwd=ROOT, env=dict(os.environ, MIFX_STORAGE="h4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"history skip h4 {part} OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from diligentfx_amd import binding

    assert binding.load().mifx_storage_mode() == 1, "run with MIFX_STORAGE=h4"
    part = sys.argv[1]
    if part == "chain":
        for size in ((67, 37), (176, 100)):
            for mask in (0x1F, 0x3F):
                _chain_case(*size, mask)
    else:
        for size in H4_PARTS[part]:
            run_patterns(*size, PATTERNS, range(8))
    print(f"history skip h4 {part} OK")
