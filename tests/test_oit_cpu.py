"""Layered order-independent transparency without a GPU: the product's per-pixel bodies (diligentfx_amd/csrc/mifx_oit.h) compiled for the host against the reference's
outputs (tests/golden/oit_golden.npz, written by tests/golden/make_golden_oit.py from the reference's shader text; inputs from tests/oit_util.py), and the argument
checks of the C ABI.

Criterion: the header compiled for the host reproduces every stored array of the reference's strict build BIT FOR BIT -- the K layer words, the tail's count and
transmittance, and the four targets -- by the reference's sequence and by the fused kernels' order of operations."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import oit_util as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
FUSED_K = (1, 2, 3, 4, 8)  # the layer counts with a fused kernel (diligentfx_amd/csrc/oit.hip)


def golden():
    return np.load(os.path.join(HERE, "golden", "oit_golden.npz"))


def case_ids():
    return [(i, str(n)) for i, n in enumerate(golden()["names"])]


@pytest.fixture(scope="module")
def host_lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return build_host_lib(hipcc)


def build_host_lib(hipcc):
    src = os.path.join(HERE, "host_kernels", "oit_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "oit_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n) for n in ("mifx_oit.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"),
               "-I", os.path.join(ROOT, "include"), "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    lib = ctypes.CDLL(out)
    lib.mifx_host_oit_pack.restype = ctypes.c_uint32
    lib.mifx_host_oit_layer_transmittance.restype = ctypes.c_float
    return lib


def host_run(lib, c, d, fused):
    """(status, layers (H, W, K), tail (H, W, 2), targets (4, H, W, 4)) of the header on the host; the outputs are poisoned beforehand"""
    w, h, k, n = c["w"], c["h"], c["k"], c["l"]
    layers, tail = np.full((h, w, k), 0xDEADBEEF, np.uint32), np.full((h, w, 2), -7.0, F)
    targets = np.ascontiguousarray(d["targets"]).copy()
    keep = [np.ascontiguousarray(d[key]) if d[key] is not None else None for key in ("depth", "base", "material", "radiance", "ibl", "alpha", "opaque")]
    cam = np.ascontiguousarray(d["camera"], F)
    fn = lib.mifx_host_oit_fused if fused else lib.mifx_host_oit_sequence
    rc = fn(k, w, h, n, *[None if a is None else O.fptr(a) for a in keep], O.fptr(cam), layers.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), O.fptr(tail), O.fptr(targets))
    return rc, layers, tail, targets


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ the product's header on the host against the reference
@pytest.mark.parametrize("i,name", case_ids())
def test_the_sequence_and_the_fused_order_on_the_host_reproduce_the_reference_bit_for_bit(host_lib, i, name):
    g = golden()
    c = O.cases()[i]
    assert c["name"] == name
    d = O.make_case(c)
    want_l, want_t, want_g = g[f"c{i}_layers"], g[f"c{i}_tail"], g[f"c{i}_targets"]
    rc, layers, tail, targets = host_run(host_lib, c, d, fused=False)
    assert rc == 0
    print(f"{name}: sequence: {int((layers != want_l).sum())} layer words, {int((tail.view(np.uint32) != want_t.view(np.uint32)).sum())} tail values, "
          f"{int((targets.view(np.uint32) != want_g.view(np.uint32)).sum())} of {want_g.size} target values differ in their bits")
    assert np.array_equal(layers, want_l) and np.array_equal(tail[..., 0], want_t[..., 0]), name  # layers and the tail's count exactly
    assert same_bits(tail, want_t) and same_bits(targets, want_g), name
    rc, fl, ft, fg = host_run(host_lib, c, d, fused=True)
    assert rc == (0 if c["k"] in FUSED_K else -2), name
    if rc == 0:
        assert np.array_equal(fl, layers) and same_bits(ft, tail) and same_bits(fg, targets), name


def test_fixture_covers_what_the_issue_plants():
    g = golden()
    cs = O.cases()
    assert [c["name"] for c in cs] == [str(n) for n in g["names"]] and len(set(c["name"] for c in cs)) == len(cs)
    assert {(c["w"], c["h"]) for c in cs} == {(1, 1), (2, 2), (5, 3), (67, 35)} and {c["k"] for c in cs} == {1, 3, 4, 8}
    for k in (1, 3, 4, 8):
        assert {0, 1, k, k + 3} <= {c["l"] for c in cs if c["k"] == k}
    assert any(c["reversed"] for c in cs) and any(c["alpha"] for c in cs) and any(not c["opaque"] and c["l"] for c in cs)
    for i in range(len(cs)):
        assert float(g[f"c{i}_strict_vs_contracted"]) <= 0.5e-3  # the project's contract is the right bar for every case (see the generator)
    # the planted pixels of a 5x3 frame with more fragments than layers: K = 4, L = 7, opaque depth
    i = [c["name"] for c in cs].index("oit_5x3_k4_l7")
    d = O.make_case(cs[i])
    layers, tail, targets = g[f"c{i}_layers"].reshape(15, 4), g[f"c{i}_tail"].reshape(15, 2), g[f"c{i}_targets"].reshape(4, 15, 4)
    before = d["targets"].reshape(4, 15, 4)
    EMPTY = 0xFFFFFFFF
    assert np.all(layers[0] == EMPTY) and same_bits(targets[:, 0], before[:, 0])                     # no slice covers the pixel: its texels keep their bits
    assert layers[1, 0] != EMPTY and np.all(layers[1, 1:] == EMPTY) and tail[1, 0] == 0               # identical packed words: one layer, nothing in the tail
    assert np.all(layers[2] == EMPTY) and tail[2, 0] == 0 and tail[2, 1] == 1                        # opacity 1 / 255 and 0.003: no fragment inserts anything ...
    assert not same_bits(targets[:, 2], before[:, 2])                                                 # ... and still blends
    assert np.all(layers[3] & 0xFF == 0)                                                              # opacity 1: the transmittance packs to 0
    assert np.all(layers[4] >> 8 == 0)                                                                # depth 0
    assert layers[5, 0] >> 8 == 0 and (layers[5] >> 8).max() == int(float(O.BELOW_BACKGROUND) * 16777215.0)
    assert list(layers[6] >> 8) == [1000, 1001, 1002, 1003] and list(layers[7] >> 8) == [5000, 5002, 5004, 5006]
    three = F(0.0)
    for _ in range(3):
        three = F(three + F(1.0) / F(255.0))
    for p in (8, 9, 10):                                                                              # seven fragments, four layers: three in the tail, the layers sorted
        assert tail[p, 0] == three and 0 < tail[p, 1] < 1 and np.all(np.diff(layers[p].astype(np.int64)) > 0)
    want = sorted(int(F(F(0.1) + F(0.07) * F((n * 7 + 3) % 11)) * F(16777215.0)) for n in range(7))[:4]
    assert list(layers[10] >> 8) == want                                                              # shuffled submission order: the four closest, sorted


def test_identical_words_and_the_fragment_behind_the_opaque_depth():
    """oit_5x3_k4_l7 pixel 11: slices 0, 2, 4, 6 lie at depth 0.3 in front of the opaque 0.5, slices 1, 3, 5 at 0.7 behind it: only the former reach the layers, each with its
    own opacity; pixel 12: the fragments AT the opaque depth (D * S >= opaque * S) are dropped, those in front are kept."""
    g, cs = golden(), O.cases()
    i = [c["name"] for c in cs].index("oit_5x3_k4_l7")
    layers = g[f"c{i}_layers"].reshape(15, 4)
    assert set(int(v) for v in layers[11] >> 8) == {int(F(0.3) * F(16777215.0))}
    assert set(int(v) for v in layers[12][layers[12] != 0xFFFFFFFF] >> 8) == {int(F(0.2) * F(16777215.0))} and int((layers[12] != 0xFFFFFFFF).sum()) == 3


def test_packing(host_lib):
    """PackOITLayer (OIT.fxh:1-8): 24 bits of depth over 8 bits of transmittance, both clamped and truncated"""
    pack = lambda d, t: host_lib.mifx_host_oit_pack(ctypes.c_float(d), ctypes.c_float(t))  # noqa: E731
    assert pack(0.0, 0.0) == 0 and pack(1.0, 1.0) == 0xFFFFFFFF and pack(2.0, -1.0) == 0xFFFFFF00 and pack(-1.0, 2.0) == 0xFF
    assert pack(0.5, 0.5) == (int(F(0.5) * F(16777215.0)) << 8) | 127
    assert host_lib.mifx_host_oit_layer_transmittance(0x12345680) == float(F(128.0) / F(255.0))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_struct_layout(mifx_lib):
    from diligentfx_amd import binding as B

    assert ctypes.sizeof(B.OITSlice) == 48 == mifx_lib.mifx_sizeof(b"oit_slice") and ctypes.sizeof(B.OITTargets) == 32 == mifx_lib.mifx_sizeof(b"oit_targets")
    assert B.OIT_MAX_SLICES == 32 and B.OIT_MAX_LAYERS == 16


def test_refusals(mifx_lib):
    """Every refusal through the check entries, which run the argument checks of the entries and nothing else (no context, no device)."""
    from diligentfx_amd import binding as B

    err = lambda: mifx_lib.mifx_last_error().decode()  # noqa: E731
    create = lambda w, h, k: mifx_lib.mifx_oit_create_check(ctypes.c_uint32(w), ctypes.c_uint32(h), ctypes.c_uint32(k))  # noqa: E731
    for k in (1, 3, 16):
        assert create(8, 4, k) == 0, err()
    assert create(8, 4, 0) == -1 and "layer_count" in err()
    assert create(8, 4, 17) == -1 and "layer_count" in err()
    assert create(0, 4, 4) == -1 and create(8, 0, 4) == -1 and create(16385, 4, 4) == -1
    assert mifx_lib.mifx_oit_create(None, 8, 4, 4, None) == -1

    W, H = 8, 4
    f1 = lambda w=W, h=H, fmt=B.FORMAT_F32, pitch=None: B.Image2D(0x1000, w, h, pitch or w * 4, fmt)  # noqa: E731
    f4 = lambda w=W, h=H, fmt=B.FORMAT_F32X4, pitch=None: B.Image2D(0x2000, w, h, pitch or w * 16, fmt)  # noqa: E731
    cam = B.CameraAttribs()
    keep = []

    def ptr(im):
        if im is None:
            return None
        keep.append(im)
        return ctypes.pointer(im)

    def slice_(depth=f1(), base=f4(), material=f4(), radiance=f4(), ibl=f4(), alpha=None):
        return B.OITSlice(ptr(depth), ptr(base), ptr(material), ptr(radiance), ptr(ibl), ptr(alpha))

    def targets(color=f4(), base=f4(), material=f4(), ibl=f4()):
        return B.OITTargets(ptr(color), ptr(base), ptr(material), ptr(ibl))

    def check(slices, opaque=None, t=None, camera=cam, count=None, w=W, h=H):
        arr = (B.OITSlice * max(len(slices), 1))(*slices)
        return mifx_lib.mifx_oit_frame_check(ctypes.c_uint32(w), ctypes.c_uint32(h), arr if slices else None, ctypes.c_uint32(len(slices) if count is None else count),
                                             ctypes.byref(opaque) if opaque is not None else None, ctypes.byref(camera) if camera is not None else None,
                                             ctypes.byref(t) if t is not None else None)

    # what is asked for is accepted: the layer entries (depth and base colour only), the colour entries, no slice at all, 32 slices
    assert check([slice_(material=None, radiance=None, ibl=None)], opaque=f1()) == 0, err()
    assert check([slice_(alpha=f1())], opaque=f1(), t=targets()) == 0, err()
    assert check([], t=targets(), camera=None) == 0 and check([]) == 0, err()
    assert check([slice_()] * 32, t=targets()) == 0, err()
    # count > MIFX_OIT_MAX_SLICES
    assert check([slice_()] * 33, t=targets()) == -1 and "MIFX_OIT_MAX_SLICES" in err()
    # a NULL required plane
    assert check([slice_(depth=None)]) == -1 and "null" in err()
    assert check([slice_(base=None)]) == -1
    for missing in ("material", "radiance", "ibl"):
        assert check([slice_(**{missing: None})], t=targets()) == -1 and "null" in err(), missing
    assert check([slice_()], t=targets(material=None)) == -1 and "null" in err()
    assert check([slice_()], camera=None) == -1 and check(None or [slice_()], count=1, camera=None) == -1
    assert mifx_lib.mifx_oit_frame_check(W, H, None, 1, None, ctypes.byref(cam), None) == -1
    # mismatched sizes
    assert check([slice_(depth=f1(w=9))]) == -1 and check([slice_(base=f4(h=5))]) == -1
    assert check([slice_()], opaque=f1(h=3)) == -1
    assert check([slice_(radiance=f4(w=7))], t=targets()) == -1 and check([slice_()], t=targets(ibl=f4(w=16))) == -1
    assert check([slice_(alpha=f1(w=4))], t=targets()) == -1
    assert check([slice_()], w=0) == -1
    # wrong formats
    assert check([slice_(depth=f4())]) == -1 and "format" in err()
    assert check([slice_(base=f1())]) == -1 and "format" in err()
    assert check([slice_(material=B.Image2D(0x2000, W, H, W * 8, B.FORMAT_F32X2))], t=targets()) == -1 and "format" in err()
    assert check([slice_()], opaque=f4()) == -1 and "format" in err()
    assert check([slice_()], t=targets(color=B.Image2D(0x2000, W, H, W * 8, B.FORMAT_F16X4))) == -1 and "format" in err()
    assert check([slice_(alpha=f4())], t=targets()) == -1 and "format" in err()
    # a bad pitch
    assert check([slice_(base=f4(pitch=W * 16 - 4))]) == -1 and "pitch" in err()
    # the entries themselves: a null object is refused before anything else is looked at
    s = slice_()
    t = targets()
    assert mifx_lib.mifx_oit_clear_layers(None) == -1 and mifx_lib.mifx_oit_update_layers(None, ctypes.byref(s), None, ctypes.byref(cam)) == -1
    assert mifx_lib.mifx_oit_apply_attenuation(None, ctypes.byref(t)) == -1 and mifx_lib.mifx_oit_blend(None, ctypes.byref(s), None, ctypes.byref(cam), ctypes.byref(t)) == -1
    assert mifx_lib.mifx_oit_build_layers(None, ctypes.byref(s), 1, None, ctypes.byref(cam)) == -1
    assert mifx_lib.mifx_oit_resolve(None, ctypes.byref(s), 1, None, ctypes.byref(cam), ctypes.byref(t)) == -1
    default = mifx_lib.mifx_oit_set_fusion(0)  # the internal A/B switch returns the previous value
    assert default in (0, 1) and mifx_lib.mifx_oit_set_fusion(1) == 0 and mifx_lib.mifx_oit_set_fusion(default) == 1
