"""GPU: the chain's composite with SSR's cleanup inside (composite_kernel<0, true>, and the same pixel body inside the TAA kernel) skips its reflection block where the
reflection mask is 0.  The chain with the default fusion mask, and with every switch, against the chain of separate passes (mask 0, whose stand-alone composite reads
R7's plane and has no such test): the frame and the TAA output, bit for bit -- on the synthetic orbit, whose mask follows the objects, and on frames whose roughness is
per-pixel noise on both sides of SSR's threshold, so that the lanes of one wave fall into different classes.  Every comparison first shows that the three classes of a
geometry pixel are in the picture: outside the mask, inside with a reflection of exactly zero weight, inside with a reflection."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import blue_noise_tables

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# 31x17: smaller than one 64 x 4 block; 200x111: neither side a multiple of the block; 208x120: the size of test_chain_fusion_is_bit_identical
SIZES = [(31, 17), (200, 111), (208, 120)]
MIN_SHARE = 0.05


def frames_for(size):
    """Frames per comparison, from a fresh history, every one compared.  Reflections with a weight build up with SSR's history; counted with the CPU checker on these
    very frames (oracle/cpu_chain.py), the class `inside the mask, refl.w != 0` holds: at 200x111 / 208x120, 11 % of the pixels of the first 6 frames and 16 % of 16 on
    the orbit; with noisy roughness 4.4 - 4.8 % of 6 frames, 7.0 - 7.5 % of 12, 8.2 - 8.5 % of 16.  At 31x17 hardly a ray finds anything in the first dozen frames
    (0.2 - 3 % of the pixels per frame), 20 - 30 % / 10 - 12 % per frame from frame 24 on: 18.5 % / 8.0 % of the pixels of 48 frames.  The other two classes hold
    15 - 25 % and 32 - 38 % throughout."""
    return 48 if size[0] * size[1] < 64 * 64 else 16


def noisy_roughness(f, w, h, threshold):
    """The frame with the roughness of every fourth geometry pixel, chosen by per-pixel noise, moved to the other side of SSR's threshold (a reflecting pixel becomes
    rough: 0.5; a rough one becomes a reflector: a quarter of the threshold), so that the lanes of one wave fall into different classes while most of the scene's
    reflectors still see what they reflect.  The same pattern in every frame of a size (screen-space noise: the histories still accumulate)."""
    g = torch.Generator(device="cpu").manual_seed(9000 + 131 * w + h)
    flip = (torch.rand(h, w, generator=g) < 0.25).to(f["material"].device)
    rough = f["material"][..., 0]
    flipped = torch.where(rough <= threshold, torch.full_like(rough, 0.5), torch.full_like(rough, 0.25 * threshold))
    out = dict(f)
    mat = f["material"].clone()
    mat[..., 0] = torch.where(flip & (f["base_color"][..., 3] > 0), flipped, rough)
    out["material"] = mat
    return out


def class_shares(f, mask, ssr):
    """(outside the mask, inside with refl.w == 0, inside with refl.w != 0) as pixel counts, from the unfused chain's mask and SSR output."""
    geom = f["base_color"][..., 3] > 0
    inside = geom & (mask != 0)
    w0 = ssr[..., 3].float() == 0
    return np.array([int((geom & (mask == 0)).sum()), int((inside & w0).sum()), int((inside & ~w0).sum())], np.int64)


def fused_chain_equals_separate_passes(size, noisy, fusion_mask=None):
    """Returns the class shares over the compared frames (asserted >= MIN_SHARE each).  fusion_mask None: what a new chain has."""
    import chain_util
    from diligentfx_amd import api, binding as B, synth

    w, h = size
    frames = frames_for(size)
    sobol, tile = blue_noise_tables()
    fused, plain = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    plain.set_fusion_mask(0)
    if fusion_mask is not None:
        fused.set_fusion_mask(fusion_mask)
    env = synth.make_sky_cube(32, fused.device).clamp(max=200.0)
    ibl = api.precompute_ibl(fused.postfx, env, lut_size=32, irradiance_size=8, prefiltered_size=16, lut_samples=64, diffuse_samples=128, specular_samples=32)
    sa = chain_util.shade_attribs(len(ibl.pre) - 1)
    scene = synth.Scene()
    threshold = float(fused.ssr_attribs.RoughnessThreshold)
    a = torch.zeros(h, w, 4, device=fused.device, dtype=B.storage_dtype())
    b = torch.zeros_like(a)
    counts = np.zeros(3, np.int64)
    for frame in range(frames):
        f = synth.make_frame(scene, frame, w, h, fused.device)
        if noisy:
            f = noisy_roughness(f, w, h, threshold)
        fused.execute(fused.bind_frame(frame, f, ibl, sa, a))
        plain.execute(plain.bind_frame(frame, f, ibl, sa, b))
        c = class_shares(f, plain.effect("ssr").get_intermediate("mask"), plain.effect_output("ssr"))
        print(f"{w}x{h} noisy {noisy} mask {fusion_mask} frame {frame}: outside the mask {c[0] / (w * h):.3f}, inside refl.w == 0 {c[1] / (w * h):.3f}, inside refl.w != 0 {c[2] / (w * h):.3f}")
        counts += c
        assert torch.equal(a, b), (size, noisy, frame, int((a != b).sum()))
        assert torch.equal(fused.effect_output("taa"), plain.effect_output("taa")), (size, noisy, frame)
        assert bool(torch.isfinite(a.float()).all())
    fused.close()
    plain.close()
    shares = counts / float(frames * w * h)
    assert (shares >= MIN_SHARE).all(), f"{w}x{h} noisy {noisy}: a class of pixels is missing from the frames compared: outside / inside w == 0 / inside w != 0 = {shares}"
    return shares


@pytest.mark.parametrize("noisy", [False, True], ids=["orbit", "noisy_roughness"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_fusion_equals_separate_passes(mifx_lib, size, noisy):
    fused_chain_equals_separate_passes(size, noisy)


@pytest.mark.parametrize("noisy", [False, True], ids=["orbit", "noisy_roughness"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_switch_equals_separate_passes(mifx_lib, size, noisy):
    """FUSE_EVERY_SWITCH: the composite inside the TAA kernel -- the other instance of the pixel body."""
    from diligentfx_amd import api

    fused_chain_equals_separate_passes(size, noisy, api.Chain.FUSE_EVERY_SWITCH)


CHILD = """
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {tests!r}]
import test_gpu_composite_skip as T
from diligentfx_amd import api, binding as B
assert B.load().mifx_storage_mode() == 1
for size in T.SIZES:
    for noisy in (False, True):
        for mask in (None, api.Chain.FUSE_EVERY_SWITCH):
            T.fused_chain_equals_separate_passes(size, noisy, mask)
print("composite skip h4 OK")
"""


def test_native_storage_build(mifx_lib):
    """The same comparisons in the RGBA16_FLOAT storage build (libmifx_h4.so, a process of its own): the fused body rounds R7's value as the plane would have."""
    from diligentfx_amd import binding as B

    if not os.path.exists(os.path.join(os.path.dirname(B.LIB_PATH), "libmifx_h4.so")):
        pytest.fail("libmifx_h4.so was not built")
    env = dict(os.environ, MIFX_STORAGE="h4")
    env.pop("MIFX_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "composite skip h4 OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
