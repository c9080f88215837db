"""Inputs of the transparency tests (test infrastructure): the transparent draws of a case as G-buffers.  Depth and opacity are those of oit_util.make_case -- its
planted SITUATIONS on the small frames, sparse random coverage at 67x35 --, normals and materials are hash-made as oit_util.e2e_inputs makes them, the camera is the
synthetic scene's (diligentfx_amd.synth.make_frame), reversed where the case is.  The conditions the tests rely on are asserted here, on the CPU."""
import numpy as np

import oit_util as O

F = np.float32


def fragment_mask(depth, opaque, reversed_):
    """(L, H, W) bool: the coverage test and the depth test of mifx_oit.h (oit_has_fragment)"""
    background = (depth < F(1e-6)) if reversed_ else (depth >= F(1.0) - F(1e-6))
    frag = ~background
    if opaque is not None:
        s = F(-1.0) if reversed_ else F(1.0)
        frag &= ~(depth * s >= opaque[None] * s)
    return frag


def case(name):
    return next(c for c in O.cases() if c["name"] == name)


def make_slices(c):
    """dict: gbuffers (L dicts of base_color / normal / material / depth), alpha (L planes or None), opaque (H, W) or None, targets (4, H, W, 4), camera (the
    CameraAttribs struct), fragments (L, H, W) bool"""
    import torch

    from diligentfx_amd import synth

    w, h, n, seed = c["w"], c["h"], c["l"], c["seed"]
    d = O.make_case(c)
    camera = synth.make_frame(synth.Scene(), 4, w, h, torch.device("cpu"), reversed_depth=c["reversed"])["camera"]
    assert (camera.fNearPlaneDepth > camera.fFarPlaneDepth) == c["reversed"]
    gbuffers = []
    for i in range(n):
        s = seed + 1000 + 20 * i
        nrm = O.field(s + 3, h, w, 4) * F(2.0) - F(1.0)
        nrm[..., 1] = np.abs(nrm[..., 1]) + F(0.2)
        nrm[..., 3] = 0
        nrm /= np.sqrt((nrm[..., :3] ** 2).sum(-1, keepdims=True)).astype(F)
        material = O.field(s + 6, h, w, 4)
        material[..., 0] = F(0.1) + F(0.8) * material[..., 0]
        material[..., 2:] = 0
        gbuffers.append(dict(base_color=np.ascontiguousarray(d["base"][i]), normal=nrm.astype(F), material=material, depth=np.ascontiguousarray(d["depth"][i])))
    frag = fragment_mask(d["depth"], d["opaque"], c["reversed"])
    if (w, h) == (5, 3):
        assert set(O.PIXEL_SITUATIONS[(5, 3)]) == set(O.SITUATIONS)  # every situation occurs
        assert not frag[:, 0, 0].any()                               # situation 0: no slice covers pixel 0
    if (w, h) == (67, 35):
        assert n > 0 and frag.mean(axis=(1, 2)).min() >= 0.05, frag.mean(axis=(1, 2))  # every slice has a fragment on at least 5 % of the pixels
        assert (~frag.any(0)).any()                                                     # at least one pixel has no fragment in any slice
    return dict(gbuffers=gbuffers, alpha=d["alpha"], opaque=d["opaque"], targets=d["targets"], camera=camera, fragments=frag)


def e2e_slices():
    """The end-to-end case of oit_util (24x16, two slices, K = 4) in the same shape"""
    e = O.e2e_inputs()
    depth = np.stack([g["depth"] for g in e["gbuffers"]])
    return dict(gbuffers=e["gbuffers"], alpha=None, opaque=None, targets=e["targets"], camera=e["camera"], fragments=fragment_mask(depth, None, False))


# ---- the chain's tests beyond the two fixture sizes: slices made for a frame size, and the fixed sequence of switches
# hash seeds per frame size, chosen so that the conditions chain_slices asserts hold against the synthetic scene's depth of frames 0 - 2 (at 8x8 a slice covers 6 texels)
CHAIN_SEEDS = {(8, 8): 7013, (33, 17): 7002, (224, 128): 7003}


def chain_slices(w, h, frames=3):
    """Two hash-made slices (K = 4) for a w x h chain frame, made as make_slices makes the 67x35 ones, with a color_alpha plane.  Asserted here, on the CPU, against the
    opaque depth the chain uses -- the synthetic scene's depth of each of the first `frames` frames: every slice has a fragment on at least 5 % of the pixels, at least one
    pixel is covered by no slice, and at least one by both."""
    import torch

    from diligentfx_amd import synth

    s = make_slices(dict(name=f"chain_{w}x{h}", w=w, h=h, k=4, l=2, reversed=False, opaque=True, alpha=True, seed=CHAIN_SEEDS.get((w, h), 7000 + w + h)))
    depth = np.stack([g["depth"] for g in s["gbuffers"]])
    scene = synth.Scene()
    for i in range(frames):
        opaque = synth.make_frame(scene, i, w, h, torch.device("cpu"))["depth"].numpy()
        check_coverage(fragment_mask(depth, opaque, False), f"{w}x{h}, frame {i}")
    return s


def check_coverage(frag, what=""):
    """The conditions of the chain's transparency tests on (L, H, W) fragment masks: every slice covers 5 % of the texels, one texel is covered by none, one by both"""
    assert frag.mean(axis=(1, 2)).min() >= 0.05, (what, frag.mean(axis=(1, 2)))
    assert (~frag.any(0)).any(), what
    assert frag.shape[0] < 2 or frag[:2].all(0).any(), what  # (a texel both slices cover: there the second blend reads what the first wrote)


def mid_run_state(i):
    """The fixed sequence of switches of a chain run (tests/cpu_product/run.py order_features, tests/test_gpu_transparency.py), as the state in force for frame i:
    (shade output and targets on, number of transparent slices, layer_count, at the second frame size).  Frames 0 - 1: the shade's targets alone; transparency on at 2;
    one slice instead of two at 3; another layer_count at 4 (the OIT object is destroyed and re-created); transparency off at 5; the shade output off at 6; a resize at 7;
    everything back on at 8."""
    if i < 2:
        return True, 0, 4, False
    if i < 5:
        return True, (2, 1, 1)[i - 2], (4, 4, 2)[i - 2], False
    if i == 5:
        return True, 0, 2, False
    if i < 8:
        return False, 0, 2, i == 7
    return True, 2, 4, True


MID_RUN_FRAMES = 10

