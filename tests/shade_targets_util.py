"""Shared by the tests of the shade's G-buffer targets (mifx_pbr_shade_targets: test_gpu_shade_targets.py on the device, test_shade_targets_cpu.py on the host) and by the
generator of their fixture (tests/golden/make_golden_shade_targets.py): the cases, the frame and the fixture's loader.  The frame is the one of the sibling fixture
(shade_output_golden.npz) with exact values written into two of its planes -- see frame_inputs -- so tests/golden/shade_targets_golden.npz holds results only."""
import os

import numpy as np

import shade_output_util as S

F = np.float32
OUTPUTS = ("color", "normal", "base_color", "material", "ibl")
ANIM_FACTORS = (0.0, 0.4, 1.0)


def _case(name, **kw):
    c = S._case(name, cc_normal=1)
    c.update(kw)
    return c


def cases():
    """Every case runs on the one frame, with two shadow-mapped lights (and three unshadowed ones); background pixels are in every case."""
    cs = [_case("no_layers", flags=0), _case("all_layers"), _case("all_layers_no_clearcoat_normal", cc_normal=0), _case("clear_coat_alone", flags=1),
          _case("blend", alpha_mode=S.BLEND), _case("blend_no_layers", alpha_mode=S.BLEND, flags=0), _case("mask", alpha_mode=S.MASK)]
    for mode, tag in ((S.ANIM_NONE, "none"), (S.ANIM_ALWAYS, "always"), (S.ANIM_TRANSITIONING, "transitioning")):  # ALWAYS does not force the factor in the footer
        cs += [_case(f"anim_{tag}_f{str(f).replace('.', '')}", anim=mode, factor=f) for f in ANIM_FACTORS]
    cs += [_case("view_white_base_color", view=S.V["WHITE_BASE_COLOR"]), _case("view_roughness", view=S.V["ROUGHNESS"]),  # (no view but the white base colour changes a target)
           _case("unlit", unlit=1), _case("unlit_no_layers", unlit=1, flags=0),
           _case("everything", tm=S.TM_MODES["UNCHARTED2"], srgb=1, highlight=0.35, anim=S.ANIM_TRANSITIONING, factor=0.4, alpha_mode=S.BLEND)]
    return cs


def frame_inputs(G):
    """The frame of the fixture from the sibling fixture's (S.load_golden()): the same planes, with
      * base-colour alpha exactly 1, 0.5 and 0 in three column bands (elsewhere on both sides of the mask's cutoff, as there), and
      * a clear-coat factor of exactly 0 and exactly 1 in two row bands.
    The clear-coat normals are within 17 degrees of the base normal (layers_util.make_layers): normalize(lerp(...)) never sees a near-zero vector."""
    gn = {k: v.copy() for k, v in G["gn"].items()}
    planes = {k: v.copy() for k, v in G["planes"].items()}
    h, w = gn["depth"].shape
    for i, a in enumerate((1.0, 0.5, 0.0)):
        gn["base_color"][:, 8 + 6 * i: 14 + 6 * i, 3] = F(a)
    planes["clearcoat"][13:18, :, 0] = F(0.0)
    planes["clearcoat"][24:29, :, 0] = F(1.0)
    return gn, planes


def geometry(gn, c):
    geom = gn["depth"] < 1.0 - 1e-6
    if c["alpha_mode"] == S.MASK:
        geom = geom & ~(gn["base_color"][..., 3] < F(S.CUTOFF))
    return geom


def load_golden():
    """The sibling fixture's frame with frame_inputs applied, and tests/golden/shade_targets_golden.npz: per case the reference's five outputs, (h, w, 4) each"""
    from util import GOLDEN

    G = S.load_golden()
    G["gn"], G["planes"] = frame_inputs(G)
    z = np.load(os.path.join(GOLDEN, "shade_targets_golden.npz"))
    names = [str(n) for n in z["names"]]
    index = z["plane_index"]  # (case, output, channel) -> a (h, w) plane of `planes`: equal channel planes are stored once
    planes = z["planes"]
    G["out"] = {n: {o: np.ascontiguousarray(np.stack([planes[index[i, j, ch]] for ch in range(4)], -1)) for j, o in enumerate(OUTPUTS)} for i, n in enumerate(names)}
    G["strict_vs_contracted"] = float(z["strict_vs_contracted"])
    return G


def dump_frame(G, path):
    """The fixture's frame as the flat file tests/host_kernels/shade_targets_sanitize_main.cpp reads (the order is documented there)"""
    from layers_util import LAYER_ORDER

    gn, pl, ibl = G["gn"], G["planes"], G["ibl"]
    stack = np.stack(G["shadows"][0]).astype(F)
    infos = np.ascontiguousarray(G["shadows"][1], F).reshape(len(G["shadows"][1]), -1)
    raw = lambda b: np.frombuffer(bytes(b) + b"\0" * (-len(bytes(b)) % 4), F).reshape(1, -1)  # noqa: E731
    layers = [pl[k] if k != "transmission" else pl[k][..., 0] for k in LAYER_ORDER]
    items = [gn["base_color"], gn["normal"], gn["material"], gn["depth"], gn["emissive"], gn["occlusion"], G["motion"], G["mesh_normal"]] + layers + [
        ibl["lut"], G["albedo"], np.repeat(G["charlie"][..., None], 4, -1), ibl["irradiance"][0], stack.reshape(-1, stack.shape[2]), infos, raw(G["camera"]), raw(G["attribs"])] + list(
        ibl["prefiltered"])
    with open(path, "wb") as f:
        f.write(np.int32(len(items)).tobytes())
        for a in items:
            a = np.ascontiguousarray(a, F)
            a3 = a.reshape(a.shape[0], a.shape[1], -1)
            f.write(np.array(a3.shape, np.int32).tobytes())
            f.write(a3.tobytes())
