"""Inputs of the order-independent-transparency tests (test infrastructure): the cases of tests/golden/oit_golden.npz and the slices, opaque depth, targets and camera of
each, generated from the case alone -- an integer hash, no library's random stream -- so that the fixture stores only what the reference made of them.

Small frames (1x1, 2x2, 5x3) hold one planted situation per pixel (SITUATIONS); the 67x35 frame is sparse random coverage over more than one workgroup in both directions."""
import ctypes

import numpy as np

F = np.float32
M32 = np.uint64(0xFFFFFFFF)
BELOW_BACKGROUND = np.nextafter(F(1.0) - F(1e-6), F(0.0))  # the largest depth that fails the shade's background test (depth >= 1 - 1e-6)

# what a pixel of a small frame holds, by index (planted()):
SITUATIONS = {
    0: "no slice covers the pixel", 1: "every fragment has the same packed word", 2: "opacity at and below 1/255", 3: "opacity 1: the transmittance packs to 0",
    4: "depth 0", 5: "the largest depth that is a fragment, and 0", 6: "24-bit depths one apart", 7: "24-bit depths two apart", 8: "front to back", 9: "back to front",
    10: "shuffled order", 11: "fragments in front of and behind the opaque depth", 12: "a fragment at the opaque depth", 13: "random", 14: "random",
}
PIXEL_SITUATIONS = {(1, 1): [10], (2, 2): [8, 9, 10, 11], (5, 3): list(range(15))}


def _mix(x):
    x = x & M32
    x = ((x ^ (x >> np.uint64(16))) * np.uint64(0x7FEB352D)) & M32
    x = ((x ^ (x >> np.uint64(15))) * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def field(seed, *shape):
    """float32 array of `shape`, 24-bit values in [0, 1), a function of (seed, index) alone"""
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    h = _mix(idx + _mix(np.uint64(seed) * np.uint64(0x9E3779B1)))
    return (h >> np.uint64(8)).astype(F) / F(16777216.0)


def cases():
    cs = []
    for (w, h) in ((1, 1), (2, 2), (5, 3)):
        for k in (1, 3, 4, 8):
            for n in sorted({0, 1, k, k + 3}):
                cs.append(dict(name=f"oit_{w}x{h}_k{k}_l{n}", w=w, h=h, k=k, l=n, reversed=False, opaque=(w, h) != (1, 1), alpha=False))
    cs.append(dict(name="oit_5x3_k3_l6_reversed", w=5, h=3, k=3, l=6, reversed=True, opaque=True, alpha=False))
    cs.append(dict(name="oit_5x3_k4_l7_color_alpha", w=5, h=3, k=4, l=7, reversed=False, opaque=True, alpha=True))
    cs.append(dict(name="oit_5x3_k4_l7_no_opaque", w=5, h=3, k=4, l=7, reversed=False, opaque=False, alpha=False))
    cs.append(dict(name="oit_67x35_k4_l7", w=67, h=35, k=4, l=7, reversed=False, opaque=True, alpha=True))
    cs.append(dict(name="oit_67x35_k8_l2_reversed", w=67, h=35, k=8, l=2, reversed=True, opaque=False, alpha=False))
    for i, c in enumerate(cs):
        c["seed"] = 100 + i
    return cs


def case_names():
    return [c["name"] for c in cases()]


def planted(sit, i, r):
    """(covered, depth, opacity, opaque depth or None) of slice i at a pixel holding situation `sit`; r = the pixel's random number for this slice"""
    a = F(0.15) + F(0.7) * r
    if sit == 0:
        return False, F(1.0), a, None
    if sit == 1:
        return True, F(0.4), F(0.5), None
    if sit == 2:
        return True, F(0.2) + F(0.05) * F(i), (F(1.0) / F(255.0)) if i % 2 == 0 else F(0.003), None
    if sit == 3:
        return True, F(0.3) + F(0.04) * F(i), F(1.0), None
    if sit == 4:
        return True, F(0.0), a, None
    if sit == 5:
        return True, BELOW_BACKGROUND if i % 2 == 0 else F(0.0), a, None
    if sit == 6:
        return True, F((1000 + i + 0.5) / 16777215.0), a, None
    if sit == 7:
        return True, F((5000 + 2 * i + 0.5) / 16777215.0), a, None
    if sit == 8:
        return True, F(0.1) + F(0.07) * F(i), a, None
    if sit == 9:
        return True, F(0.85) - F(0.07) * F(i), a, None
    if sit == 10:
        return True, F(0.1) + F(0.07) * F((i * 7 + 3) % 11), a, None
    if sit == 11:
        return True, F(0.3) if i % 2 == 0 else F(0.7), a, F(0.5)
    if sit == 12:
        return True, F(0.45) if i % 2 == 0 else F(0.2), a, F(0.45)
    return None


def make_case(c):
    """dict: depth (L, H, W), base / material / radiance / ibl (L, H, W, 4), alpha (L, H, W) or None, opaque (H, W) or None, targets (4, H, W, 4) in the order colour,
    base colour, material, IBL, camera (144 floats)"""
    w, h, n, seed = c["w"], c["h"], c["l"], c["seed"]
    cover, dep, opa = field(seed + 1, n, h, w), field(seed + 2, n, h, w), field(seed + 3, n, h, w)
    kind = field(seed + 4, n, h, w)
    # (a tenth of the large frames per slice: what a slice touches does not compress, and the fixture is committed)
    depth = np.where(cover < F(0.4 if w * h <= 15 else 0.1), F(0.05) + F(0.9) * dep, F(1.0)).astype(F)
    a = np.where(kind < F(0.1), F(1.0), np.where(kind < F(0.2), opa * (F(1.0) / F(255.0)), F(0.02) + F(0.96) * opa)).astype(F)
    opaque = (F(0.35) + F(0.6) * field(seed + 5, h, w)).astype(F)
    for p, sit in enumerate(PIXEL_SITUATIONS.get((w, h), [])):
        y, x = divmod(p, w)
        for i in range(n):
            got = planted(sit, i, opa[i, y, x])
            if got is None:
                continue
            covered, d, al, od = got
            depth[i, y, x], a[i, y, x] = (d if covered else F(1.0)), al
            opaque[y, x] = od if od is not None else F(1.0)  # (the opaque surface of the other planted pixels is at the far plane: every fragment passes)
    out = {}
    base = field(seed + 6, n, h, w, 4)
    base[..., 3] = a
    material = field(seed + 7, n, h, w, 4)
    material[..., 2:] = 0
    radiance = field(seed + 8, n, h, w, 4) * F(3.0)
    radiance[..., 3] = 1
    ibl = field(seed + 9, n, h, w, 4) * F(0.5)
    ibl[..., 3] = 0
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    q = lambda s, scale: (((xx * 3 + yy * 5 + cc * 7 + s) % 17).astype(F) / F(16.0) * F(scale)).astype(F)  # noqa: E731  (a periodic background: the untouched texels of the large frames compress)
    targets = np.stack([q(seed + 10, 2.0), q(seed + 11, 1.0), q(seed + 12, 1.0), q(seed + 13, 0.5)])
    targets[0, ..., 3] = 1
    cam = np.zeros(144, F)
    cam[4:8] = [w, h, 1.0 / w, 1.0 / h]
    cam[8:12] = [0.1, 100.0, 0.0, 1.0]
    if c["reversed"]:
        depth, opaque = (F(1.0) - depth).astype(F), (F(1.0) - opaque).astype(F)
        cam[10:12] = [1.0, 0.0]
    out.update(depth=depth, base=base, material=material, radiance=radiance, ibl=ibl, alpha=field(seed + 14, n, h, w) if c["alpha"] else None,
               opaque=opaque if c["opaque"] else None, targets=targets, camera=cam)
    return out


E2E = dict(name="oit_e2e_24x16_k4_l2", w=24, h=16, k=4, l=2, seed=900)


def e2e_inputs():
    """The end-to-end case: the G-buffers of two transparent slices (hash-made surfaces in front of the synthetic scene's camera), to be shaded with mifx_pbr_shade_execute
    (the fixture: with the reference's shade) and blended over a periodic background.  dict: gbuffers (two dicts of base_color / normal / material / depth), camera
    (the CameraAttribs struct), targets (4, H, W, 4)."""
    import torch

    from diligentfx_amd import synth

    w, h, seed = E2E["w"], E2E["h"], E2E["seed"]
    camera = synth.make_frame(synth.Scene(), 4, w, h, torch.device("cpu"))["camera"]
    gbuffers = []
    for i, (cover, opacity) in enumerate(((0.7, 0.6), (0.5, 0.35))):
        s = seed + 20 * i
        depth = np.where(field(s + 1, h, w) < F(cover), F(0.90) + F(0.08) * field(s + 2, h, w) - F(0.02) * F(i), F(1.0)).astype(F)
        n = field(s + 3, h, w, 4) * F(2.0) - F(1.0)
        n[..., 1] = np.abs(n[..., 1]) + F(0.2)
        n[..., 3] = 0
        n /= np.sqrt((n[..., :3] ** 2).sum(-1, keepdims=True)).astype(F)
        base = field(s + 4, h, w, 4)
        base[..., 3] = F(opacity) + F(0.3) * field(s + 5, h, w)
        material = field(s + 6, h, w, 4)
        material[..., 0] = F(0.1) + F(0.8) * material[..., 0]
        material[..., 2:] = 0
        gbuffers.append(dict(base_color=base, normal=n.astype(F), material=material, depth=depth))
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    targets = np.stack([(((xx * 3 + yy * 5 + cc * 7 + j) % 17).astype(F) / F(16.0) * F(sc)).astype(F) for j, sc in enumerate((2.0, 1.0, 1.0, 0.5))])
    targets[0, ..., 3] = 1
    return dict(gbuffers=gbuffers, camera=camera, targets=targets)


def fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def camera_struct(cam):
    from diligentfx_amd import binding as B

    return B.CameraAttribs.from_buffer_copy(np.ascontiguousarray(cam, F).tobytes())
