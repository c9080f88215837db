"""CPU-side: the refusals of the chain's shade-stage setters that no other test without a GPU reaches -- mifx_chain_set_material_layers, _set_shade_output, _set_transparency,
_get_shade_target and _set_row_band, in the order an entry checks its arguments.  Statuses and messages are what the library answered before the stage's state became one record
(mifx_objects.h mifx_chain::ShadeStage): a refactor of that record keeps them.  None of these calls reaches the device, so a chain object of zeros serves, as in
tests/test_shade_targets_abi.py (which holds the desc refusals and both orders of row band against shade output)."""
import ctypes

import pytest

from test_shade_targets_abi import _h4, _plane, blank_chain  # noqa: F401  (the fixture)

INVALID_ARG, NOT_IMPLEMENTED = -1, -5
NEEDS_TARGETS = ("mifx_chain_set_transparency: needs mifx_chain_set_shade_output with write_targets: the transparent draws blend into the chain's own BaseColor / Material / IBL "
                 "planes (without them base colour and material are the caller's const planes)")
TARGETS_GO_OFF = ("mifx_chain_set_shade_output: write_targets goes off while mifx_chain_set_transparency is on: the transparent draws blend into the chain's own target planes "
                  "(turn transparency off first)")
BAND_WITH_OUTPUT = "mifx_chain_set_row_band: a row band (or sharding) is not combined with mifx_chain_set_shade_output: the sharded hit fetch has no output stage or footer"
u = ctypes.c_uint32


def _slices(n, missing=None):
    """n transparent draws whose four required planes are descriptors with nothing behind them; missing = (slice, plane) left null"""
    from diligentfx_amd import binding as B

    arr, keep = (B.TransparentSlice * n)(), []
    for i in range(n):
        for k in ("base_color", "normal", "material", "depth"):
            if missing != (i, k):
                keep.append(_plane())
                setattr(arr[i].gbuffer, k, ctypes.pointer(keep[-1]))
    arr._keep = keep
    return arr


def _desc():
    from diligentfx_amd import binding as B

    d, r = B.PBRShadeOutputDesc(), B.PBRRendererShaderParameters()
    d.renderer = ctypes.pointer(r)
    d._keep = r
    return d


def _said(lib, rc, status, message):
    err = lib.mifx_last_error().decode()
    assert rc == status and err == message, (rc, err)


def _ok(rc):
    assert rc == 0, rc


def test_material_layers_refusals(mifx_lib, blank_chain):
    from diligentfx_amd import binding as B

    lib, sm, infos = mifx_lib, B.ShadowMapArray(), (B.PBRShadowMapInfo * 9)()
    _said(lib, lib.mifx_chain_set_material_layers(None, None, None), INVALID_ARG, "mifx_chain_set_material_layers: null chain")
    for block in (B.PBRShadows(None, infos, 1, 3), B.PBRShadows(ctypes.pointer(sm), infos, 9, 3), B.PBRShadows(ctypes.pointer(sm), None, 1, 3)):
        _said(lib, lib.mifx_chain_set_material_layers(blank_chain, None, ctypes.byref(block)), INVALID_ARG, "mifx_chain_set_material_layers: bad shadows block")
    _ok(lib.mifx_chain_set_material_layers(blank_chain, None, ctypes.byref(B.PBRShadows(ctypes.pointer(sm), None, 0, 3))))  # (no map info is needed for no map)
    _ok(lib.mifx_chain_set_material_layers(blank_chain, None, None))


def test_transparency_refusals_in_the_order_of_the_checks(mifx_lib, blank_chain):
    lib, c = mifx_lib, blank_chain
    _said(lib, lib.mifx_chain_set_transparency(None, u(4), _slices(1), u(1)), INVALID_ARG, "mifx_chain_set_transparency: null chain")
    _ok(lib.mifx_chain_set_transparency(c, u(4), None, u(0)))  # off is never refused
    # without the targets: the slice count and the layer count are refused first
    _said(lib, lib.mifx_chain_set_transparency(c, u(4), _slices(33), u(33)), INVALID_ARG, "mifx_chain_set_transparency: 33 slices are more than MIFX_OIT_MAX_SLICES (32)")
    for k in (0, 17):
        _said(lib, lib.mifx_chain_set_transparency(c, u(k), _slices(1), u(1)), INVALID_ARG, f"mifx_oit_create_check: layer_count {k} is outside 1 .. 16")
    _said(lib, lib.mifx_chain_set_transparency(c, u(4), _slices(1), u(1)), INVALID_ARG, NEEDS_TARGETS)
    desc = _desc()
    _ok(lib.mifx_chain_set_shade_output(c, ctypes.byref(desc), 0))  # the output stage without the targets is not enough
    _said(lib, lib.mifx_chain_set_transparency(c, u(4), _slices(1), u(1)), INVALID_ARG, NEEDS_TARGETS)
    _ok(lib.mifx_chain_set_shade_output(c, None, 1))
    _said(lib, lib.mifx_chain_set_transparency(c, u(4), _slices(2, (1, "material")), u(2)), INVALID_ARG,
          "mifx_chain_set_transparency: slice 1: base_color, normal, material and depth must not be null")
    _said(lib, lib.mifx_chain_set_transparency(c, u(4), _slices(2, (0, "depth")), u(2)), INVALID_ARG,
          "mifx_chain_set_transparency: slice 0: base_color, normal, material and depth must not be null")
    _ok(lib.mifx_chain_set_transparency(c, u(4), _slices(2), u(2)))
    # the targets going off under transparency, with a desc and without; a row band behind transparency
    _said(lib, lib.mifx_chain_set_shade_output(c, ctypes.byref(desc), 0), INVALID_ARG, TARGETS_GO_OFF)
    _said(lib, lib.mifx_chain_set_shade_output(c, None, 0), INVALID_ARG, TARGETS_GO_OFF)
    _said(lib, lib.mifx_chain_set_row_band(c, 16, 48, 4), INVALID_ARG, BAND_WITH_OUTPUT)
    _ok(lib.mifx_chain_set_shade_output(c, ctypes.byref(desc), 1))  # (the targets stay on: the desc may change)
    _ok(lib.mifx_chain_set_transparency(c, u(0), None, u(0)))
    _ok(lib.mifx_chain_set_shade_output(c, None, 0))
    _ok(lib.mifx_chain_set_row_band(c, 16, 48, 4))
    _ok(lib.mifx_chain_set_row_band(c, 0, 0, 0))


def test_transparency_in_the_native_storage_build(blank_chain):
    h4 = _h4()
    _said(h4, h4.mifx_chain_set_transparency(None, u(4), _slices(1), u(1)), INVALID_ARG, "mifx_chain_set_transparency: null chain")
    _ok(h4.mifx_chain_set_transparency(blank_chain, u(4), None, u(0)))
    for k, n in ((4, 1), (0, 1), (4, 33)):  # (before every other check)
        _said(h4, h4.mifx_chain_set_transparency(blank_chain, u(k), _slices(n), u(n)), NOT_IMPLEMENTED,
              "mifx_chain_set_transparency: the fused shade-and-blend is not part of the native-storage build yet")


def test_shade_target_refusals(mifx_lib, blank_chain):
    from diligentfx_amd import binding as B

    lib, c, out = mifx_lib, blank_chain, B.Image2D()
    for args in ((None, b"normal", ctypes.byref(out)), (c, None, ctypes.byref(out)), (c, b"normal", None)):
        _said(lib, lib.mifx_chain_get_shade_target(*args), INVALID_ARG, "mifx_chain_get_shade_target: null argument")
    _said(lib, lib.mifx_chain_get_shade_target(c, b"depth", ctypes.byref(out)), INVALID_ARG, "mifx_chain_get_shade_target: unknown target 'depth' (normal, base_color, material, ibl)")
    for targets in (0, 1):  # off; on, and no frame executed yet
        _ok(lib.mifx_chain_set_shade_output(c, None, targets))
        for name in ("normal", "base_color", "material", "ibl"):
            _said(lib, lib.mifx_chain_get_shade_target(c, name.encode(), ctypes.byref(out)), INVALID_ARG,
                  f"mifx_chain_get_shade_target: no '{name}' target (mifx_chain_set_shade_output with write_targets, and a frame executed)")


@pytest.mark.parametrize("args", [(0, 4, 0), (-1, 4, 0), (8, 4, 0), (0, 4, -1)])
def test_row_band_refuses_bad_arguments(mifx_lib, blank_chain, args):
    chain = None if args == (0, 4, 0) else blank_chain
    _said(mifx_lib, mifx_lib.mifx_chain_set_row_band(chain, *args), INVALID_ARG, "mifx_chain_set_row_band: bad argument")


def test_a_bad_desc_is_refused_before_the_row_band(mifx_lib, blank_chain):
    from diligentfx_amd import binding as B

    _ok(mifx_lib.mifx_chain_set_row_band(blank_chain, 16, 48, 4))
    _said(mifx_lib, mifx_lib.mifx_chain_set_shade_output(blank_chain, ctypes.byref(B.PBRShadeOutputDesc()), 1), INVALID_ARG,
          "mifx_chain_set_shade_output: output->renderer is null (the PBRRendererShaderParameters block of the frame)")
