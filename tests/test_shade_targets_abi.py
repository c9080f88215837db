"""CPU-side checks of the boundary of the shade's G-buffer targets: mifx_pbr_shade_targets and mifx_chain_set_shade_output are exported by both libraries, mifx_pbr_targets has
one layout in the header (C), the library and the ctypes mirror, and every refusal arrives with its message before any device call."""
import ctypes
import os
import re

import pytest

from util import ROOT

ENTRIES = ("mifx_pbr_shade_targets", "mifx_chain_set_shade_output", "mifx_chain_get_shade_target")


def _h4():
    from diligentfx_amd import binding as B

    path = os.path.join(os.path.dirname(B.__file__), "libmifx_h4.so")
    assert os.path.exists(path), "build() makes both libraries"
    h4 = ctypes.CDLL(path)
    h4.mifx_last_error.restype = ctypes.c_char_p
    return h4


def test_symbols_are_exported_by_both_libraries_and_named_outside_the_frame_edge_matrices(mifx_lib):
    header = open(os.path.join(ROOT, "include", "mifx.h")).read()
    h4 = _h4()
    for name in ENTRIES:
        assert hasattr(mifx_lib, name) and hasattr(h4, name), name
        assert not re.fullmatch(r"mifx_\w*_execute\w*", name)  # (tests/test_frame_edges_coverage.py demands a row for every such name)
        assert re.search(r"MIFX_API\s+mifx_status\s+" + name + r"\s*\(", header), name


def test_targets_layout(mifx_lib):
    from diligentfx_amd import binding as B

    n = mifx_lib.mifx_sizeof(b"pbr_targets")
    assert n == ctypes.sizeof(B.PBRTargets) == 32 and B.SIZEOF_NAMES["pbr_targets"] is B.PBRTargets
    assert [getattr(B.PBRTargets, f).offset for f in ("normal", "base_color", "material", "ibl")] == [0, 8, 16, 24]
    assert _h4().mifx_sizeof(b"pbr_targets") == 32


def _plane(w=8, h=4, data=0x1000, fmt=None, pitch=None):
    """A descriptor whose checks pass; nothing behind `data` -- only refusals (and the h4 answer) are made with it"""
    from diligentfx_amd import binding as B

    im = B.Image2D()
    im.data, im.width, im.height = data, w, h
    im.pitch_bytes = w * 16 if pitch is None else pitch
    im.format = B.FORMAT_F32X4 if fmt is None else fmt
    return im


def _call(lib, desc, planes, out=None, gbuffer=None):
    from diligentfx_amd import binding as B

    ctx = ctypes.create_string_buffer(1 << 16)
    g, cam, sa, ibl = gbuffer or B.GBuffer(), B.CameraAttribs(), B.PBRShadeAttribs(), B.IBL()
    out = out or _plane(data=0x9000)
    bg = (ctypes.c_float * 4)()
    tg = B.PBRTargets(*[ctypes.pointer(p) if p is not None else None for p in planes]) if planes is not None else None
    rc = lib.mifx_pbr_shade_targets(ctx, ctypes.byref(g), None, ctypes.byref(cam), ctypes.byref(sa), ctypes.byref(ibl), None, ctypes.byref(desc) if desc is not None else None, bg,
                                    ctypes.byref(out), ctypes.byref(tg) if tg is not None else None)
    return rc, lib.mifx_last_error().decode()


def _desc(**fields):
    from diligentfx_amd import binding as B

    r = B.PBRRendererShaderParameters()
    desc = B.PBRShadeOutputDesc(ctypes.pointer(r), 0, 0, 0, 0, 0.5, 0, 0, 0, None, None)
    desc._keep = r
    for k, v in fields.items():
        if k == "renderer":
            desc.renderer = ctypes.POINTER(B.PBRRendererShaderParameters)()
        else:
            setattr(desc, k, v)
    return desc


def _four():
    return [_plane(data=0x1000 * (i + 1)) for i in range(4)]


DESC_REFUSALS = [
    ("view below the range", dict(debug_view=-1), "debug view -1"),
    ("view above the range", dict(debug_view=35), "debug view 35"),
    ("unknown flag", dict(flags=2), "unknown flag bits 0x2"),
    ("unlit with a lighting view", dict(unlit=1, debug_view=8), "unlit"),
    ("null renderer", dict(renderer=None), "renderer"),
    ("unknown tone mapping mode", dict(tone_mapping_mode=12), "tone mapping mode 12"),
    ("AgX custom", dict(tone_mapping_mode=9), "AGX_CUSTOM"),
    ("unknown animation mode", dict(loading_animation=3), "loading animation mode 3"),
    ("unknown alpha mode", dict(alpha_mode=3), "alpha mode 3"),
]


@pytest.mark.parametrize("what,fields,message", DESC_REFUSALS)
def test_entry_refuses_what_the_output_entry_refuses(mifx_lib, what, fields, message):
    rc, err = _call(mifx_lib, _desc(**fields), _four())
    assert rc == -1 and message in err and err.startswith("mifx_pbr_shade_targets"), (what, rc, err)  # MIFX_ERR_INVALID_ARG


def test_entry_refuses_bad_target_planes(mifx_lib):
    from diligentfx_amd import binding as B

    rc, err = _call(mifx_lib, _desc(), None)
    assert rc == -1 and "null argument" in err
    for i, name in enumerate(("normal", "base_color", "material", "ibl")):
        planes = _four()
        planes[i] = None
        rc, err = _call(mifx_lib, _desc(), planes)
        assert rc == -1 and f"targets->{name} is null" in err, (name, err)
        for bad in (_plane(w=9), _plane(h=5), _plane(fmt=B.FORMAT_F32), _plane(pitch=8 * 16 - 4), _plane(data=0)):
            planes = _four()
            bad.data = bad.data and 0x1000 * (i + 1)
            planes[i] = bad
            rc, err = _call(mifx_lib, None, planes)  # (also with the NULL desc)
            assert rc == -1 and f"targets->{name}" in err, (name, err)
    # a target may not alias a G-buffer plane it is computed from, the colour or another target
    planes = _four()
    g = B.GBuffer()
    src = _plane(data=planes[2].data)
    g.normal = ctypes.pointer(src)
    rc, err = _call(mifx_lib, _desc(), planes, gbuffer=g)
    assert rc == -1 and "targets->material aliases a G-buffer plane" in err, err
    rc, err = _call(mifx_lib, _desc(), planes, out=_plane(data=planes[3].data))
    assert rc == -1 and "targets->ibl aliases out_color" in err, err
    planes[1].data = planes[0].data
    rc, err = _call(mifx_lib, _desc(), planes)
    assert rc == -1 and "targets->base_color aliases targets->normal" in err, err


def test_native_storage_build_says_not_implemented():
    """libmifx_h4.so checks the arguments the same way and answers a valid call with MIFX_ERR_NOT_IMPLEMENTED before any device call"""
    h4 = _h4()
    for desc in (_desc(debug_view=8), None):
        rc, err = _call(h4, desc, _four())
        assert rc == -5 and "native-storage build" in err, (rc, err)
    rc, err = _call(h4, _desc(debug_view=35), _four())
    assert rc == -1 and "debug view 35" in err
    planes = _four()
    planes[0] = None
    rc, err = _call(h4, _desc(), planes)
    assert rc == -1 and "targets->normal is null" in err


# ---- the chain's setter: no device call, so a chain object of zeros serves (the setter reads and writes its own fields only)
def _chain_set(lib, chain, desc, targets):
    rc = lib.mifx_chain_set_shade_output(chain, ctypes.byref(desc) if desc is not None else None, ctypes.c_int32(targets))
    return rc, lib.mifx_last_error().decode()


@pytest.fixture()
def blank_chain(mifx_lib):
    """sizeof(mifx_chain) is a few kilobytes; the setters touched here neither construct nor destroy anything in it"""
    chain = ctypes.create_string_buffer(1 << 16)
    post = ctypes.create_string_buffer(1 << 16)
    ctypes.cast(chain, ctypes.POINTER(ctypes.c_void_p))[0] = ctypes.addressof(post)  # mifx_chain::ctx, its first member (mifx_chain_set_row_band writes the band into it)
    chain._keep = post
    return chain


@pytest.mark.parametrize("what,fields,message", DESC_REFUSALS + [
    ("a tone mapping mode", dict(tone_mapping_mode=4), "tone_mapping_mode 4: the chain tone-maps at its own end"),
    ("the sRGB flag", dict(flags=1), "CONVERT_OUTPUT_TO_SRGB: the chain converts at its own end"),
])
def test_chain_setter_refusals(mifx_lib, blank_chain, what, fields, message):
    for targets in (0, 1):
        rc, err = _chain_set(mifx_lib, blank_chain, _desc(**fields), targets)
        assert rc == -1 and message in err and err.startswith("mifx_chain_set_shade_output"), (what, rc, err)
    rc, err = _chain_set(mifx_lib, None, _desc(), 1)
    assert rc == -1 and "null chain" in err


def test_chain_setter_and_row_band_refuse_each_other_in_both_orders(mifx_lib, blank_chain):
    assert _chain_set(mifx_lib, blank_chain, _desc(), 1)[0] == 0
    rc = mifx_lib.mifx_chain_set_row_band(blank_chain, 16, 48, 4)
    assert rc == -1 and "mifx_chain_set_shade_output" in mifx_lib.mifx_last_error().decode()
    assert mifx_lib.mifx_chain_set_row_band(blank_chain, 0, 0, 0) == 0  # (no band: not a refusal)
    assert _chain_set(mifx_lib, blank_chain, None, 0)[0] == 0           # off
    assert mifx_lib.mifx_chain_set_row_band(blank_chain, 16, 48, 4) == 0
    for desc, targets in ((_desc(), 0), (None, 1), (_desc(), 1)):
        rc, err = _chain_set(mifx_lib, blank_chain, desc, targets)
        assert rc == -1 and "row band or sharding" in err, err
    assert _chain_set(mifx_lib, blank_chain, None, 0)[0] == 0           # (turning it off is never refused)


def test_native_storage_chain_setter(blank_chain):
    h4 = _h4()
    rc, err = _chain_set(h4, blank_chain, _desc(), 1)
    assert rc == -5 and "native-storage build" in err
    rc, err = _chain_set(h4, blank_chain, _desc(tone_mapping_mode=4), 1)
    assert rc == -1 and "tone_mapping_mode 4" in err
    assert _chain_set(h4, blank_chain, None, 0)[0] == 0
