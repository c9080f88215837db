"""CPU-side checks of the boundary of the shade's output stage: mifx_pbr_shade_output is exported, mifx_pbr_shade_output_desc has one layout in the header (C), the library
and the ctypes mirror, the enum constants are the reference's, and the entry's argument checks -- all of which precede its first device call -- refuse what the header says
they refuse, with a message."""
import ctypes
import os
import re

import pytest

from util import ROOT


def test_symbol_is_exported_and_named_outside_the_frame_edge_matrices(mifx_lib):
    assert hasattr(mifx_lib, "mifx_pbr_shade_output")
    assert not re.fullmatch(r"mifx_\w*_execute\w*", "mifx_pbr_shade_output")  # (tests/test_frame_edges_coverage.py demands a row for every such name)
    header = open(os.path.join(ROOT, "include", "mifx.h")).read()
    assert re.search(r"MIFX_API\s+mifx_status\s+mifx_pbr_shade_output\s*\(", header)


def test_desc_layout_and_constants(mifx_lib):
    from diligentfx_amd import binding as B

    n = mifx_lib.mifx_sizeof(b"pbr_shade_output_desc")
    assert n == ctypes.sizeof(B.PBRShadeOutputDesc) == 56 and B.SIZEOF_NAMES["pbr_shade_output_desc"] is B.PBRShadeOutputDesc
    D = B.PBRShadeOutputDesc
    assert [getattr(D, f).offset for f in ("renderer", "debug_view", "tone_mapping_mode", "loading_animation", "alpha_mode", "alpha_mask_cutoff", "unlit", "flags", "motion",
                                           "mesh_normal")] == [0, 8, 12, 16, 20, 24, 28, 32, 40, 48]
    header = open(os.path.join(ROOT, "include", "mifx.h")).read()
    body = re.search(r"enum /\* PBR_Renderer::DebugViewType.*?\{(.*?)\};", header, re.S).group(1)
    names = re.findall(r"MIFX_PBR_DEBUG_VIEW_(\w+)", body)
    assert names[:-1] == list(B.PBR_DEBUG_VIEWS) and names[-1] == "COUNT" and B.PBR_DEBUG_VIEW_COUNT == 35  # PBR_Renderer.hpp:401-439, NumDebugViews
    assert (B.PBR_DEBUG_VIEW_NONE, B.PBR_DEBUG_VIEW_WHITE_BASE_COLOR, B.PBR_DEBUG_VIEW_SCENE_DEPTH) == (0, 19, 34)
    assert (B.PBR_LOADING_ANIMATION_NONE, B.PBR_LOADING_ANIMATION_ALWAYS, B.PBR_LOADING_ANIMATION_TRANSITIONING) == (0, 1, 2)
    assert (B.PBR_ALPHA_MODE_OPAQUE, B.PBR_ALPHA_MODE_MASK, B.PBR_ALPHA_MODE_BLEND) == (0, 1, 2)


def _call(lib, desc):
    """The entry with every pointer non-null and nothing behind them but zeros: a call that passes the argument checks would go on to the device, so only refusals are made"""
    from diligentfx_amd import binding as B

    ctx = ctypes.create_string_buffer(1 << 16)
    g, cam, sa, ibl, img = B.GBuffer(), B.CameraAttribs(), B.PBRShadeAttribs(), B.IBL(), B.Image2D()
    bg = (ctypes.c_float * 4)()
    rc = lib.mifx_pbr_shade_output(ctx, ctypes.byref(g), None, ctypes.byref(cam), ctypes.byref(sa), ctypes.byref(ibl), None, ctypes.byref(desc) if desc is not None else None, bg,
                                   ctypes.byref(img), None)
    return rc, lib.mifx_last_error().decode()


@pytest.mark.parametrize("what,fields,message", [
    ("view below the range", dict(debug_view=-1), "debug view -1"),
    ("view above the range", dict(debug_view=35), "debug view 35"),
    ("unknown flag", dict(flags=2), "unknown flag bits 0x2"),
    ("unlit with a lighting view", dict(unlit=1, debug_view=8), "unlit"),
    ("null renderer", dict(renderer=None), "renderer"),
    ("unknown tone mapping mode", dict(tone_mapping_mode=12), "tone mapping mode 12"),
    ("AgX custom", dict(tone_mapping_mode=9), "AGX_CUSTOM"),
    ("unknown animation mode", dict(loading_animation=3), "loading animation mode 3"),
    ("unknown alpha mode", dict(alpha_mode=3), "alpha mode 3"),
])
def test_refusals_precede_any_device_call(mifx_lib, what, fields, message):
    from diligentfx_amd import binding as B

    r = B.PBRRendererShaderParameters()
    desc = B.PBRShadeOutputDesc(ctypes.pointer(r), 0, 0, 0, 0, 0.5, 0, 0, 0, None, None)
    for k, v in fields.items():
        if k == "renderer":
            desc.renderer = ctypes.POINTER(B.PBRRendererShaderParameters)()
        else:
            setattr(desc, k, v)
    rc, err = _call(mifx_lib, desc)
    assert rc == -1 and message in err, (what, rc, err)  # MIFX_ERR_INVALID_ARG


def test_null_desc_is_refused(mifx_lib):
    rc, err = _call(mifx_lib, None)
    assert rc == -1 and "null argument" in err


def test_native_storage_build_says_not_implemented(mifx_lib):
    """libmifx_h4.so exports the entry, checks its arguments the same way, and answers a valid call with MIFX_ERR_NOT_IMPLEMENTED and a message before any device call"""
    from diligentfx_amd import binding as B

    path = os.path.join(os.path.dirname(B.__file__), "libmifx_h4.so")
    assert os.path.exists(path), "build() makes both libraries"
    h4 = ctypes.CDLL(path)
    h4.mifx_last_error.restype = ctypes.c_char_p
    r = B.PBRRendererShaderParameters()
    desc = B.PBRShadeOutputDesc(ctypes.pointer(r), B.PBR_DEBUG_VIEW_ROUGHNESS, 0, 0, 0, 0.5, 0, 0, 0, None, None)
    rc, err = _call(h4, desc)
    assert rc == -5 and "native-storage build" in err, (rc, err)
    desc.debug_view = 35
    rc, err = _call(h4, desc)
    assert rc == -1 and "debug view 35" in err
