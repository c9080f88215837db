"""The shade's output stage (mifx_pbr_shade_output) where there is no GPU: the kernel's per-pixel source compiled for the HOST (tests/host_kernels/shade_output_host.cpp
includes diligentfx_amd/csrc/mifx_pbr_output.h as layers_host.cpp includes the layered body) against tests/golden/shade_output_golden.npz -- the reference's own shader text
compiled per permutation (tests/golden/make_golden_shade_output.py) -- and the numpy restatement of the tail that the GPU test uses at its second frame size, pinned to the
same fixture.  Test infrastructure: the product never builds, loads or calls the host library."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import shade_output_util as S
from layers_util import LAYER_ORDER
from util import assert_close

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = S.cases()


class HostPlane(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int), ("c", ctypes.c_int)]


def plane(a):
    if a is None:
        return HostPlane(None, 0, 0, 0)
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return HostPlane(a.ctypes.data, a.shape[1], a.shape[0], a.shape[2] if a.ndim == 3 else 1)


@pytest.fixture(scope="module")
def host_lib():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(HERE, "host_kernels", "shade_output_host.cpp")
    out_dir = os.path.join(HERE, "host_kernels", "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "shade_output_host.so")
    deps = [src, os.path.join(ROOT, "include", "mifx.h")] + [os.path.join(ROOT, "diligentfx_amd", "csrc", n)
                                                             for n in ("mifx_pbr_output.h", "mifx_pbr_layers.h", "mifx_pbr.h", "mifx_tonemap.h", "mifx_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fopenmp", "-I", os.path.join(ROOT, "diligentfx_amd", "csrc"), "-I",
               os.path.join(ROOT, "include"), "-o", out, src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def run_on_host(host_lib, G, c):
    from diligentfx_amd import binding as B

    gn = G["gn"]
    h, w = gn["depth"].shape
    got, got_spec = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    P = (HostPlane * 10)(plane(gn["base_color"]), plane(gn["normal"]), plane(gn["material"]), plane(gn["depth"]), plane(gn["emissive"]), plane(gn["occlusion"]), plane(got),
                         plane(got_spec), plane(G["motion"] if c["motion"] else None), plane(G["mesh_normal"] if c["mesh_normal"] else None))
    layer_planes = {**G["planes"], "transmission": np.ascontiguousarray(G["planes"]["transmission"][..., 0])}
    L = (HostPlane * 7)(*[plane(layer_planes[k]) for k in LAYER_ORDER])
    charlie4 = np.repeat(G["charlie"][..., None], 4, -1).copy()
    U = (HostPlane * 3)(plane(G["ibl"]["lut"]), plane(G["albedo"]), plane(charlie4))
    irradiance = plane(G["ibl"]["irradiance"][0])
    prefiltered = (HostPlane * len(G["ibl"]["prefiltered"]))(*[plane(m) for m in G["ibl"]["prefiltered"]])
    stack = np.ascontiguousarray(np.stack(G["shadows"][0]))
    sm = (HostPlane * 1)(HostPlane(stack.ctypes.data, stack.shape[2], stack.shape[1], 1))
    infos = np.ascontiguousarray(G["shadows"][1], np.float32)
    f = S.output_desc_fields(c)
    renderer = f["renderer"]
    desc = B.PBRShadeOutputDesc(ctypes.pointer(renderer), f["debug_view"], f["tone_mapping_mode"], f["loading_animation"], f["alpha_mode"], f["alpha_mask_cutoff"], f["unlit"],
                                f["flags"], 0, None, None)
    rc = host_lib.mifx_host_pbr_shade_output(P, L, U, ctypes.byref(irradiance), prefiltered, len(G["ibl"]["prefiltered"]), G["camera"], bytes(G["attribs"]),
                                             (ctypes.c_float * 4)(*S.BACKGROUND), c["flags"], ctypes.c_float(S.IOR), ctypes.c_float(S.ROTATION), 0, sm, stack.shape[0],
                                             infos.ctypes.data_as(ctypes.c_void_p), infos.shape[0], S.PCF, ctypes.byref(desc))
    assert rc == 0
    return got, got_spec


def geometry(G, c):
    geom = G["gn"]["depth"] < 1.0 - 1e-6
    if c["alpha_mode"] == S.MASK:
        geom = geom & ~(G["gn"]["base_color"][..., 3] < S.CUTOFF)
    return geom


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_output_stage_source_on_the_host_against_the_fixture(host_lib, golden, c):
    """Every case against the reference, BIT FOR BIT like the layers harness: on the host the kernel's division and square root are the IEEE operations and its sin / pow /
    exp are glibc's -- the checker's own -- and every operation of the stage is written in the shader's order.  No case needed a looser bar: the tone-map curves, the sRGB
    pow and the animation's sin reproduce between the two compilations."""
    got, got_spec = run_on_host(host_lib, golden, c)
    want, want_spec = golden["out"][c["name"]]
    assert np.isfinite(got).all()
    assert np.array_equal(got_spec, want_spec), f"{c['name']}: {(got_spec != want_spec).mean():.2e} of the specular IBL values differ"
    geom = geometry(golden, c)
    assert np.array_equal(got[~geom], np.broadcast_to(np.array(S.BACKGROUND, np.float32), got[~geom].shape))
    assert np.array_equal(got, want), f"{c['name']}: {(got != want).mean():.2e} of the values differ, max {np.abs(got - want).max():.3e}"


def test_identity_case_is_the_layered_shade(golden):
    """The fixture's identity case holds the lit colour of the layered shade (alpha forced to 1), and `highlight_0` / `anim_transitioning_f00` are that picture again"""
    none = golden["out"]["none"][0]
    assert np.array_equal(none, golden["out"]["highlight_0"][0]) and np.array_equal(none, golden["out"]["anim_transitioning_f00"][0])
    geom = golden["gn"]["depth"] < 1.0 - 1e-6
    assert (none[geom][:, 3] == 1.0).all() and float(none[geom][:, :3].max()) > 1.0


TAIL_CASES = [c for c in CASES if S.is_tail_case(c) and not c["tm"]]


@pytest.mark.parametrize("c", TAIL_CASES, ids=[c["name"] for c in TAIL_CASES])
def test_numpy_restatement_of_the_tail_reproduces_the_fixture(golden, c):
    """shade_output_util.tail_np on the fixture's lit colour (view NONE) gives the fixture's tail cases: what the GPU test applies to the device's own layered shade"""
    lit = golden["out"]["none"][0]
    tr = golden["planes"]["transmission"][..., 0] if c["flags"] & 16 else None
    got = S.tail_np(c, lit, golden["gn"]["base_color"], golden["gn"]["depth"], golden["camera"], transmission=tr)
    assert_close(got, golden["out"][c["name"]][0], max_outlier_frac=0.0, what=c["name"])


def test_fixture_covers_what_the_issue_asks(golden):
    names = set(golden["out"])
    assert {"view_" + v.lower() for v in S.VIEWS[1:]} <= names and len(names) == len(CASES) == 60
    depth, a = golden["gn"]["depth"], golden["gn"]["base_color"][..., 3]
    geom = depth < 1.0 - 1e-6
    assert depth.shape == (36, 56) and (~geom).any() and (a[geom] < S.CUTOFF).any() and (a[geom] > S.CUTOFF).any() and (np.abs(a[geom] - S.CUTOFF) > 1e-3).all()
    assert max(golden["strict_vs_contracted"].values()) <= 0.5e-3
    for n in ("view_texcoord0", "view_texcoord1", "view_thickness", "view_clear_coat_layers_off", "view_sheen_color_layers_off", "view_iridescence_layers_off",
              "view_transmission_layers_off"):
        assert (golden["out"][n][0][geom][:, :3] == 0.0).all(), n
    assert (golden["out"]["view_mesh_normal"][0][geom][:, :3] == 0.5).all() and (golden["out"]["view_motion_vectors"][0][geom][:, :3] == 0.0).all()
