"""Cases of the material fetch (mifx_pbr_material_fetch), shared by the fixture's generator (tests/golden/make_golden_material_fetch.py) and the tests: every input is built
here from fixed seeds, the fixture (tests/golden/material_fetch_golden.npz) holds the reference's outputs only.

The head of the reference's pixel shader has discontinuities; the cases stay clear of them by construction, and the generator proves it by building every case twice
(strict and contracted) and asserting that the two agree:
  * the wrap of frac (atlas path): the texture coordinates are affine with offsets that keep pixel centres away from integers;
  * ceil(LOD) in the atlas margin: atlas cases have a nearly constant gradient whose level of detail lies well inside (k, k + 1);
  * the fade-out thresholds: gradients either well below the limit, well inside the band or well beyond twice the limit;
  * d != 0, NormalLen > 1e-5: texture coordinates and positions are never degenerate where a fragment is; mesh normals are unit or exactly zero (plane absent);
  * MicroNormal.z < 0: a three-channel normal map has b >= 0.8, the two-channel one b = 0."""
import ctypes
import os

import numpy as np

import grid_util as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "material_fetch_golden.npz")
F = np.float32
W0, H0 = 48, 28
SLOTS = ("BASE_COLOR", "PHYS_DESC", "NORMAL", "OCCLUSION", "EMISSIVE", "METALLIC", "ROUGHNESS", "CLEAR_COAT", "CLEAR_COAT_ROUGHNESS", "CLEAR_COAT_NORMAL", "SHEEN_COLOR",
         "SHEEN_ROUGHNESS", "ANISOTROPY", "IRIDESCENCE", "IRIDESCENCE_THICKNESS", "TRANSMISSION")
S = {n: i for i, n in enumerate(SLOTS)}
LAYER_CLEAR_COAT, LAYER_SHEEN, LAYER_ANISOTROPY, LAYER_IRIDESCENCE, LAYER_TRANSMISSION, ALL_LAYERS = 1, 2, 4, 8, 16, 31
FLAG_ATLAS, FLAG_TRANSFORM, FLAG_SRGB = 1, 2, 4
WRAP, CLAMP = 1, 3
# output planes: name -> channels stored (the other channels of a 4-channel plane are zero)
GBUFFER_OUT = (("base_color", 4), ("normal", 3), ("material", 4), ("emissive", 3), ("occlusion", 1))
LAYER_OUT = (("clearcoat", 2, LAYER_CLEAR_COAT), ("clearcoat_normal", 3, LAYER_CLEAR_COAT), ("sheen", 4, LAYER_SHEEN), ("anisotropy", 3, LAYER_ANISOTROPY),
             ("iridescence", 2, LAYER_IRIDESCENCE), ("transmission", 1, LAYER_TRANSMISSION))
IOR, ROTATION = 1.4, 0.6


def attribs(selector=0, wrap_u=WRAP, wrap_v=WRAP, slice=0.0, bias=(0.0, 0.0), m=(1.0, 0.0, 0.0, 1.0), atlas=(1.0, 1.0, 0.0, 0.0)):
    """PBRMaterialTextureAttribs as 12 four-byte words"""
    a = np.zeros(12, F)
    a[1:] = [slice, bias[0], bias[1], *m, *atlas]
    w = a.view(np.uint32).copy()
    w[0] = ((selector + 1) & 7) | (((wrap_u - 1) & 7) << 3) | (((wrap_v - 1) & 7) << 6)
    return w


def rotation(deg, sx, sy):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return (float(F(sx * c)), float(F(sx * s)), float(F(-sy * s)), float(F(sy * c)))


def material(maps=None, workflow=0, base_color_factor=(1, 1, 1, 1), emissive_factor=(1, 1, 1), normal_scale=1.0, cc_normal_scale=1.0, metallic=1.0, roughness=1.0, occlusion=1.0,
             clearcoat=(1.0, 1.0), sheen=(1, 1, 1, 1), anisotropy_strength=1.0, iridescence=(1.0, 100.0, 400.0), transmission=1.0, fallback=(1, 1, 1, 1)):
    """A material record as plain data: maps = {slot name: (texture index, attribs words)}"""
    return dict(maps=dict(maps or {}), workflow=workflow, base_color_factor=base_color_factor, emissive_factor=emissive_factor, normal_scale=normal_scale,
                cc_normal_scale=cc_normal_scale, metallic=metallic, roughness=roughness, occlusion=occlusion, clearcoat=clearcoat, sheen=sheen,
                anisotropy_strength=anisotropy_strength, iridescence=iridescence, transmission=transmission, fallback=fallback)


def material_words(m):
    """mifx_pbr_material (1008 bytes) as 252 four-byte words"""
    f = np.zeros(252, F)
    f[0:4] = m["base_color_factor"]
    f[4:7], f[7] = m["emissive_factor"], m["normal_scale"]
    f[8:11], f[11] = (1, 1, 1), m["cc_normal_scale"]
    f[14], f[15] = 0.5, m["metallic"]
    f[16], f[17], f[18], f[19] = m["roughness"], m["occlusion"], m["clearcoat"][0], m["clearcoat"][1]
    f[24:28] = m["sheen"]
    f[28:30] = (m["anisotropy_strength"], ROTATION)
    f[32:36] = (m["iridescence"][0], IOR, m["iridescence"][1], m["iridescence"][2])
    f[36] = m["transmission"]
    f[40:44] = m["fallback"]
    w = f.view(np.uint32).copy()
    w[12], w[13] = m["workflow"], 0
    idx = np.full(16, -1, np.int32)
    for s in range(16):
        w[44 + 12 * s:56 + 12 * s] = attribs(selector=-1)
    for name, (t, a) in m["maps"].items():
        w[44 + 12 * S[name]:56 + 12 * S[name]] = a
        idx[S[name]] = t
    w[236:252] = idx.view(np.uint32)
    return w


def random_chain(rng, w, h, slices, levels, kind="colour", dtype=F):
    """Independent random values per level (not a box filter: a wrong level shows)"""
    out = []
    for k in range(levels):
        shape = (slices, max(1, h >> k), max(1, w >> k), 4)
        t = rng.random(shape, dtype=F)
        if kind == "normal":       # xy in [0.3, 0.7], b in [0.8, 1]: z stays well above 0
            t[..., :2] = 0.3 + 0.4 * t[..., :2]
            t[..., 2] = 0.8 + 0.2 * t[..., 2]
        elif kind == "normal2":    # two channels: b = 0, z is rebuilt
            t[..., :2] = 0.3 + 0.4 * t[..., :2]
            t[..., 2] = 0.0
        elif kind == "colour":
            t = 0.05 + 0.9 * t
        if dtype == np.uint8:
            t = np.rint(t * 255.0).astype(np.uint8)
        out.append(np.ascontiguousarray(t))
    return out


def decoded(chain):
    """What the kernel reads out of a chain: RGBA8_UNORM is code / 255, correctly rounded"""
    return [m if m.dtype == F else (m.astype(F) / F(255.0)).astype(F) for m in chain]


def affine_uv(w, h, du, angle_deg, offset, bend=0.0):
    """uv = R(angle) * du * (x, y) + offset (+ a small quadratic term, so that the derivatives differ from quad to quad)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x + 0.5, y + 0.5
    c, s = np.cos(np.radians(angle_deg)), np.sin(np.radians(angle_deg))
    u = du * (c * x - s * y) + offset[0] + bend * du * 0.01 * x * y
    v = du * (s * x + c * y) + offset[1] + bend * du * 0.008 * (x * x - y * y) * 0.1
    return np.stack([u, v], -1).astype(F)


def frame(w=W0, h=H0, reversed_depth=False, seed=1, holes=True):
    """The interpolants every case starts from: a smooth surface (depth), unit mesh normals, vertex colours, a face plane of both signs"""
    cam = G.make_camera(w, h, eye=(0.3, 1.2, -4.0), at=(0.0, 0.0, 0.0), reversed_depth=reversed_depth)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 3.2 + 0.035 * x + 0.05 * y + 0.15 * np.sin(0.21 * x + 0.1) * np.cos(0.17 * y)
    depth = G.camera_z_to_depth(z, cam)
    far = F(cam[G.CAM_FAR_DEPTH])
    if holes and w > 8 and h > 8:
        depth[h - 6:h - 1, w - 9:w - 2] = far  # a block of background (it splits quads: odd bounds) ...
        depth[3, 5], depth[10, 17], depth[11, 18] = far, far, far  # ... and single pixels
    n = np.stack([0.3 * np.sin(0.13 * x + 0.2 * y), 0.25 * np.cos(0.11 * y - 0.07 * x), -1.0 + 0.0 * x], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normal = np.concatenate([n, np.zeros((h, w, 1))], -1).astype(F)
    color = np.stack([0.6 + 0.4 * np.sin(0.3 * x) ** 2, 0.5 + 0.5 * np.cos(0.2 * y) ** 2, 0.7 + 0.0 * x, 0.8 + 0.2 * np.sin(0.1 * x * y) ** 2], -1).astype(F)
    face = np.where(((x // 5).astype(int) + (y // 4).astype(int)) % 3 == 0, -1.0, 1.0).astype(F)
    flat = np.zeros((h, w, 4), F)
    flat[..., 2] = -1.0  # (a constant mesh normal for the cases that are not about normals: their normal plane is constant and packs to nothing in the fixture)
    return dict(camera=cam, depth=depth.astype(F), mesh_normal=normal, flat_normal=flat, color=color, face=face, reversed=reversed_depth, seed=seed)


def has_fragment(c):
    d = c["interp"]["depth"]
    bg = d < 1e-6 if c["reversed"] else d >= F(1.0 - 1e-6)
    ok = ~bg
    idx = c["interp"].get("material_index")
    if idx is not None:
        ok &= (idx >= 0) & (idx < len(c["materials"]))
    return ok


def case(name, fr, uv0=None, uv1=None, materials=(), textures=(), layers=0, flags=0, mip_bias=0.0, use=("flat_normal",), index=None):
    interp = {"depth": fr["depth"]}
    if uv0 is not None:
        interp["uv0"] = uv0
    if uv1 is not None:
        interp["uv1"] = uv1
    for k in use:
        interp["mesh_normal" if k == "flat_normal" else k] = fr[k]
    if index is not None:
        interp["material_index"] = index
    return dict(name=name, camera=fr["camera"], reversed=fr["reversed"], interp=interp, materials=list(materials), textures=list(textures), layers=layers, flags=flags,
                mip_bias=mip_bias)


def cases():
    out = []
    rng = np.random.default_rng(20240607)
    fr = frame()
    tex = [random_chain(rng, 16, 16, 2, 5) for _ in range(6)]                                      # 0..5: colour-like 16x16, 5 levels, 2 slices
    tex += [random_chain(rng, 16, 16, 2, 5, "normal"), random_chain(rng, 16, 16, 2, 5, "normal2"), random_chain(rng, 16, 16, 2, 5, "normal")]  # 6, 7, 8
    minified = affine_uv(W0, H0, 2.5 / 16, 12.0, (0.37, 0.21), bend=1.0)
    magnified = affine_uv(W0, H0, 0.3 / 16, -20.0, (0.13, 0.58), bend=1.0)
    uv1 = affine_uv(W0, H0, 1.3 / 16, 40.0, (0.71, 0.09), bend=1.0)
    base = lambda a=None, t=0: {"BASE_COLOR": (t, attribs(slice=1.0) if a is None else a)}  # noqa: E731
    # (a) base-colour map only, wrap: minified (a derivative of about 2.5 texels) and magnified
    out.append(case("a_minified", fr, uv0=minified, materials=[material(base())], textures=tex, flags=FLAG_SRGB))
    out.append(case("a_magnified", fr, uv0=magnified, materials=[material(base())], textures=tex))
    # (b) clamp in u, wrap in v, texture coordinates in [-1.5, 2.5]
    wide = affine_uv(W0, H0, 4.0 / 48, 0.0, (-1.5, -1.5))
    wide[..., 1] = (-1.5 + 4.0 * (np.arange(H0)[:, None] + 0.5) / H0 + 0.003 * np.arange(W0)[None, :]).astype(F)
    out.append(case("b_clamp_u_wrap_v", fr, uv0=wide, materials=[material(base(attribs(wrap_u=CLAMP, wrap_v=WRAP)))], textures=tex))
    # (c) a texture-coordinate transform: rotation 30 degrees, scale (2, 0.5), a bias
    out.append(case("c_transform", fr, uv0=magnified, materials=[material(base(attribs(m=rotation(30.0, 2.0, 0.5), bias=(0.3, -0.2))))], textures=tex, flags=FLAG_TRANSFORM))
    # (d) occlusion on UV1 and the rest on UV0; a present map whose selector is -1
    out.append(case("d_two_uv_sets", fr, uv0=minified, uv1=uv1, textures=tex, flags=FLAG_SRGB,
                    materials=[material({**base(), "OCCLUSION": (1, attribs(selector=1)), "EMISSIVE": (2, attribs(selector=-1)), "PHYS_DESC": (3, attribs())}, occlusion=0.8)]))
    # (e) a normal map with mesh normals and a face plane of both signs
    nm = lambda t=6, **kw: {"NORMAL": (t, attribs(**kw))}  # noqa: E731
    out.append(case("e_normal_map", fr, uv0=minified, materials=[material({**base(), **nm()})], textures=tex, use=("mesh_normal", "face")))
    # (f) a normal map with no mesh normals, fHandness +1 and -1
    for hn in (1.0, -1.0):
        f2 = dict(fr, camera=fr["camera"].copy())
        f2["camera"][16] = hn
        out.append(case(f"f_no_mesh_normals_handness{int(hn):+d}", f2, uv0=magnified, materials=[material({**base(), **nm()})], textures=tex, use=()))
    # (g) a two-channel normal map (b = 0, z rebuilt); NormalScale 0.5
    out.append(case("g_two_channel_normal_map", fr, uv0=magnified, materials=[material(nm(7))], textures=tex, use=("mesh_normal",)))
    out.append(case("g_normal_scale", fr, uv0=magnified, materials=[material(nm(6), normal_scale=0.5)], textures=tex, use=("mesh_normal",)))
    # (h) PHYS_DESC against separate METALLIC + ROUGHNESS
    out.append(case("h_phys_desc", fr, uv0=minified, materials=[material({"PHYS_DESC": (1, attribs()), "METALLIC": (2, attribs()), "ROUGHNESS": (3, attribs())}, metallic=0.9, roughness=1.3)],
                    textures=tex))
    out.append(case("h_metallic_roughness", fr, uv0=minified, materials=[material({"METALLIC": (2, attribs()), "ROUGHNESS": (3, attribs(slice=1.0))}, metallic=0.9, roughness=1.3)],
                    textures=tex))
    # (i) specular-glossiness with unit factors
    out.append(case("i_specular_glossiness", fr, uv0=minified, materials=[material({**base(), "PHYS_DESC": (1, attribs())}, workflow=1)], textures=tex))
    # (j) vertex colours; emissive with factors; fallback colour with no base map
    out.append(case("j_vertex_colours_emissive", fr, uv0=minified, textures=tex, use=("flat_normal", "color"), flags=FLAG_SRGB,
                    materials=[material({**base(), "EMISSIVE": (4, attribs())}, emissive_factor=(0.5, 2.0, 1.5), base_color_factor=(0.9, 0.8, 0.7, 0.6))]))
    out.append(case("j_fallback_colour", fr, uv0=minified, textures=tex, use=("flat_normal", "color"), materials=[material({}, fallback=(0.2, 0.4, 0.6, 0.8))]))
    # (k) mip bias +1.5 and -1
    out.append(case("k_mip_bias_plus", fr, uv0=minified, materials=[material(base())], textures=tex, mip_bias=1.5))
    out.append(case("k_mip_bias_minus", fr, uv0=minified, materials=[material(base())], textures=tex, mip_bias=-1.0))
    # (l) every layer map on, with a clear-coat normal map that has its own UV attribs; (m) the same scene from RGBA8 textures
    ident = dict(m=(1.0, 0.0, 0.0, 1.0))
    every = {"BASE_COLOR": (0, attribs(**ident)), "PHYS_DESC": (1, attribs(**ident)), "NORMAL": (6, attribs(**ident)), "OCCLUSION": (2, attribs(slice=1.0)),
             "EMISSIVE": (3, attribs()), "CLEAR_COAT": (4, attribs()), "CLEAR_COAT_ROUGHNESS": (5, attribs(slice=1.0)),
             "CLEAR_COAT_NORMAL": (8, attribs(selector=1, m=rotation(-25.0, 1.5, 0.8), bias=(0.1, 0.2))), "SHEEN_COLOR": (0, attribs(slice=1.0)), "SHEEN_ROUGHNESS": (1, attribs(slice=1.0)),
             "ANISOTROPY": (2, attribs()), "IRIDESCENCE": (3, attribs(slice=1.0)), "IRIDESCENCE_THICKNESS": (4, attribs(slice=1.0)), "TRANSMISSION": (5, attribs())}
    lm = material(every, emissive_factor=(1.2, 0.7, 0.4), normal_scale=0.8, cc_normal_scale=0.7, metallic=0.9, roughness=0.95, occlusion=0.9, clearcoat=(0.8, 0.6),
                  sheen=(0.9, 0.6, 0.3, 0.7), anisotropy_strength=0.75, iridescence=(0.85, 120.0, 380.0), transmission=0.4)
    out.append(case("l_every_layer", fr, uv0=magnified, uv1=uv1, materials=[lm], textures=tex, layers=ALL_LAYERS, flags=FLAG_TRANSFORM | FLAG_SRGB, use=("mesh_normal", "face")))
    rng8 = np.random.default_rng(77)
    tex8 = [random_chain(rng8, 16, 16, 2, 5, dtype=np.uint8) for _ in range(6)]
    tex8 += [random_chain(rng8, 16, 16, 2, 5, "normal", np.uint8), random_chain(rng8, 16, 16, 2, 5, "normal2", np.uint8), random_chain(rng8, 16, 16, 2, 5, "normal", np.uint8)]
    out.append(case("m_every_layer_rgba8", fr, uv0=magnified, uv1=uv1, materials=[lm], textures=tex8, layers=ALL_LAYERS, flags=FLAG_TRANSFORM | FLAG_SRGB, use=("mesh_normal", "face")))
    # (n) a 16x4 texture with 5 levels, and a 1x1 texture with 1 level
    odd = [random_chain(rng, 16, 4, 2, 5), random_chain(rng, 1, 1, 1, 1)]
    out.append(case("n_16x4_five_levels", fr, uv0=minified, materials=[material(base(attribs(slice=1.0), 0))], textures=odd))
    out.append(case("n_1x1_one_level", fr, uv0=minified, materials=[material(base(attribs(), 1))], textures=odd))
    # (o) three materials with an index plane that holds every index, a -1 and a material_count, over background and foreground depth; straddling quads stay in
    y, x = np.mgrid[0:H0, 0:W0]
    index = ((x // 7 + y // 5) % 3).astype(F)
    index[2, 3], index[2, 4], index[20, 30], index[21, 31] = -1.0, 3.0, -1.0, 3.0
    index[H0 - 4, W0 - 5], index[H0 - 3, W0 - 4] = -1.0, 3.0  # (inside the background block)
    three = [material({**base(), **nm()}), material({"BASE_COLOR": (2, attribs(selector=1)), "OCCLUSION": (3, attribs())}, base_color_factor=(0.7, 0.9, 1.0, 1.0)),
             material({"EMISSIVE": (4, attribs()), "PHYS_DESC": (5, attribs(slice=1.0))}, fallback=(0.3, 0.5, 0.2, 1.0), metallic=0.5)]
    out.append(case("o_three_materials", fr, uv0=minified, uv1=uv1, materials=three, textures=tex, index=index, use=("mesh_normal", "face")))
    # (p) frames 77x45, 2x1 and 1x1
    for w, h in ((77, 45), (2, 1), (1, 1)):
        fp = frame(w, h, holes=w > 8)
        out.append(case(f"p_frame_{w}x{h}", fp, uv0=affine_uv(w, h, 1.7 / 16, 12.0, (0.37, 0.21), bend=0.3), materials=[material(nm())], textures=tex, use=("mesh_normal",)))
    # ---- the atlas: 64x64 with 16x16 regions (a region is a quarter of the atlas along each axis), 5 levels
    atlas = [random_chain(rng, 64, 64, 2, 5), random_chain(rng, 64, 64, 2, 5, "normal")]
    region = lambda i, j, sx=1.0, sy=1.0: (0.25 * sx, 0.25 * sy, 0.25 * i + (0.25 if sx < 0 else 0.0), 0.25 * j + (0.25 if sy < 0 else 0.0))  # noqa: E731
    # gradient of sqrt(2) atlas texels: the level of detail is 0.5
    smooth = affine_uv(W0, H0, np.sqrt(2.0) / 16, 10.0, (0.3137, 0.1731), bend=0.05)
    ab = lambda i, j, t=0, **kw: {"BASE_COLOR": (t, attribs(atlas=region(i, j, kw.pop("sx", 1.0), kw.pop("sy", 1.0)), **kw))}  # noqa: E731
    out.append(case("q_atlas_wrap", fr, uv0=smooth, materials=[material(ab(1, 2))], textures=atlas, flags=FLAG_ATLAS))
    out.append(case("r_atlas_clamp", fr, uv0=smooth, materials=[material(ab(2, 1, wrap_u=CLAMP, wrap_v=CLAMP, slice=1.0))], textures=atlas, flags=FLAG_ATLAS | FLAG_SRGB))
    # (s) a gradient inside the fade-out band (limit 4 texels: 6) and one beyond twice the limit (10: the mean colour alone)
    out.append(case("s_atlas_fade_band", fr, uv0=affine_uv(W0, H0, 6.0 / 16, 10.0, (0.3137, 0.1731), bend=0.02), materials=[material(ab(3, 0))], textures=atlas, flags=FLAG_ATLAS))
    out.append(case("s_atlas_mean_colour", fr, uv0=affine_uv(W0, H0, 10.0 / 16, 10.0, (0.3137, 0.1731), bend=0.02), materials=[material(ab(3, 0))], textures=atlas, flags=FLAG_ATLAS))
    # (t) an upside-down and a mirrored region (negative scale)
    out.append(case("t_atlas_upside_down", fr, uv0=smooth, materials=[material(ab(0, 3, sy=-1.0))], textures=atlas, flags=FLAG_ATLAS))
    out.append(case("t_atlas_mirrored", fr, uv0=smooth, materials=[material(ab(1, 1, sx=-1.0))], textures=atlas, flags=FLAG_ATLAS))
    # (u) a normal map through the atlas
    out.append(case("u_atlas_normal_map", fr, uv0=smooth, materials=[material({**ab(1, 2), "NORMAL": (1, attribs(atlas=region(2, 2)))})], textures=atlas, flags=FLAG_ATLAS,
                    use=("mesh_normal", "face")))
    # reversed depth once
    out.append(case("reversed_depth", frame(reversed_depth=True), uv0=minified, materials=[material(nm())], textures=tex, use=("mesh_normal",)))
    return out


def layer_planes_written(c):
    """The layer planes a case's call writes"""
    cc_normal = any("CLEAR_COAT_NORMAL" in m["maps"] for m in c["materials"])
    return [n for n, _, bit in LAYER_OUT if (c["layers"] & bit) and (n != "clearcoat_normal" or cc_normal)]


def output_names(c):
    return [n for n, _ in GBUFFER_OUT] + layer_planes_written(c)


def load_golden():
    z = np.load(GOLDEN)
    names = [str(n) for n in z["names"]]
    return {n: {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")} for i, n in enumerate(names)}, float(z["strict_vs_contracted"])


def expected_plane(gold_case, name, channels):
    """A stored plane (channels first, to pack well) as the 4-channel / 1-channel plane the entry writes where a fragment is"""
    a = gold_case[name]
    if channels == 1 and name in ("occlusion", "transmission"):
        return a[0]
    full = np.zeros(a.shape[1:] + (4,), F)
    full[..., :a.shape[0]] = np.moveaxis(a, 0, -1)
    return full


def channels_of(name):
    return dict([(n, c) for n, c in GBUFFER_OUT] + [(n, c) for n, c, _ in LAYER_OUT])[name]


class HostTexture(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int), ("slices", ctypes.c_int), ("mips", ctypes.c_int), ("rgba8", ctypes.c_int),
                ("slice_pitch_bytes", ctypes.c_uint64)]


class HostPitchedPlane(ctypes.Structure):  # host_plane of tests/host_kernels/material_fetch_host.cpp
    _fields_ = [("data", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int), ("c", ctypes.c_int), ("pitch_bytes", ctypes.c_int)]


INTERPOLANTS = ("depth", "uv0", "uv1", "mesh_normal", "color", "face", "material_index")
ALL_OUTPUTS = ("base_color", "normal", "material", "emissive", "occlusion", "clearcoat", "clearcoat_normal", "sheen", "anisotropy", "iridescence", "transmission")
SENTINEL = F(-7.25)


def flat_textures(c):
    """A case's textures as the entry takes them: per texture one array (slices, texels of the chain, 4), float32 or uint8"""
    return [np.ascontiguousarray(np.concatenate([m.reshape(m.shape[0], -1, 4) for m in t], axis=1)) for t in c["textures"]]


def blank_outputs(c):
    """Every output plane of a case's call, holding the sentinel"""
    h, w = c["interp"]["depth"].shape
    return {n: np.full((h, w, 4) if channels_of(n) > 1 else (h, w), SENTINEL, F) for n in output_names(c)}


def run_on_host(lib, c):
    """The kernel's body, compiled for the host, over a case: the output planes (sentinel where nothing was stored)"""
    from diligentfx_amd import binding as B

    def plane(a):
        if a is None:
            return HostPitchedPlane(None, 0, 0, 0, 0)
        a = np.ascontiguousarray(a)
        keep.append(a)
        return HostPitchedPlane(a.ctypes.data, a.shape[1], a.shape[0], a.shape[2] if a.ndim == 3 else 1, 0)

    keep = []
    got = blank_outputs(c)
    P = (HostPitchedPlane * 7)(*[plane(c["interp"].get(k)) for k in INTERPOLANTS])
    O = (HostPitchedPlane * 11)(*[HostPitchedPlane(got[n].ctypes.data, got[n].shape[1], got[n].shape[0], 4 if got[n].ndim == 3 else 1, 0) if n in got else plane(None)
                                  for n in ALL_OUTPUTS])
    flat = flat_textures(c)
    T = (HostTexture * max(len(flat), 1))(*[HostTexture(f.ctypes.data, t[0].shape[2], t[0].shape[1], t[0].shape[0], len(t), int(f.dtype == np.uint8), f.strides[0])
                                            for f, t in zip(flat, c["textures"])])
    mats = np.ascontiguousarray(np.stack([material_words(m) for m in c["materials"]]))
    cam = B.camera_from_bytes(c["camera"].tobytes())
    rc = lib.mifx_host_material_fetch(P, O, mats.ctypes.data_as(ctypes.c_void_p), len(c["materials"]), T, len(flat), c["layers"], c["flags"], ctypes.c_float(c["mip_bias"]),
                                      ctypes.byref(cam), int(c["reversed"]))
    assert rc == 0
    return got


# ---- cases (v): the fetched planes through the existing shade (two lights and the IBL of tests/golden/layers_golden.npz)
SHADED = {"l_every_layer": "all", "o_three_materials": None}  # case -> the permutation of the reference's layered shade (None: the default shade)
# what the caller's planes hold where the fetch stores nothing (a pixel without a fragment whose depth is not the far plane is still shaded)
CALLER = {"base_color": (0.5, 0.5, 0.5, 1.0), "normal": (0.0, 0.0, -1.0, 0.0), "material": (0.5, 0.0, 0.0, 0.0), "emissive": (0.0, 0.0, 0.0, 0.0), "occlusion": 1.0,
          "clearcoat": (0.0, 0.5, 0.0, 0.0), "clearcoat_normal": (0.0, 0.0, -1.0, 0.0), "sheen": (0.0, 0.0, 0.0, 0.5), "anisotropy": (1.0, 0.0, 0.0, 0.0),
          "iridescence": (0.0, 100.0, 0.0, 0.0), "transmission": 0.0}


def shade_setup():
    """(IBL maps as numpy, the two sheen tables, mifx_pbr_shade_attribs with two lights) of the cases (v)"""
    from diligentfx_amd import binding as B
    from layers_util import load_layers_golden

    L = load_layers_golden()
    sa = B.PBRShadeAttribs()
    sa.IBLScale[:] = [1.0, 0.9, 1.1, 1.0]
    sa.OcclusionStrength, sa.EmissionScale, sa.PrefilteredCubeLastMip, sa.LightCount, sa.Workflow = 0.8, 1.2, float(len(L["ibl"]["prefiltered"]) - 1), 2, 0
    sa.Lights[0] = B.PBRLightAttribs(1, 0.0, 0.0, 0.0, 0.301511, -0.904534, 0.301511, -1, 3.0, 2.8, 2.5, 0.0, 0.0, 0.0, 0.0, 0.0)  # directional
    sa.Lights[1] = B.PBRLightAttribs(2, 0.5, 1.5, -2.0, 0.0, -1.0, 0.0, -1, 20.0, 25.0, 30.0, 0.0, 0.0, 0.0, 0.0, 0.0)             # point, no range
    return L["ibl"], L["albedo"], L["charlie"], sa


def planes_with_caller_texels(c, gold_case):
    """The reference-fetched planes of a case as full planes: the fixture's values where a fragment is, CALLER elsewhere"""
    frag = has_fragment(c)
    out = {}
    for name in output_names(c):
        p = expected_plane(gold_case, name, channels_of(name)).copy()
        p[~frag] = np.asarray(CALLER[name], F)
        out[name] = p
    return out
