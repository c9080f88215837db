"""The C ABI of the material fetch (mifx_pbr_material_fetch / mifx_pbr_material_fetch_check) against the built libraries, with no device: exports of both builds, struct
sizes, every refusal of include/mifx.h with a message that names the argument, a valid call, and the native-storage build's MIFX_ERR_NOT_IMPLEMENTED."""
import copy
import ctypes
import os

import numpy as np
import pytest

import material_fetch_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"fp32": os.path.join(ROOT, "diligentfx_amd", "libmifx.so"), "h4": os.path.join(ROOT, "diligentfx_amd", "libmifx_h4.so")}
INVALID_ARG, NOT_IMPLEMENTED = -1, -5
NEW_STRUCTS = {"texture_array": 40, "pbr_texture_attribs": 48, "pbr_material": 1008, "material_interpolants": 56, "material_fetch_desc": 48}


def load(build):
    from diligentfx_amd import binding as B

    if not os.path.exists(LIBS[build]):
        pytest.skip(f"{LIBS[build]} is not built")
    lib = B.declare_material_fetch(ctypes.CDLL(LIBS[build]))
    lib.mifx_last_error.restype = ctypes.c_char_p
    lib.mifx_sizeof.restype, lib.mifx_sizeof.argtypes = ctypes.c_uint32, [ctypes.c_char_p]
    return lib


class Call:
    """The arguments of one call, built from a case of the fixture without touching a device: the planes' addresses are made up (the checks never read them)"""

    def __init__(self, c, build="fp32"):
        from diligentfx_amd import binding as B

        self.c, self.B = c, B
        self.h, self.w = c["interp"]["depth"].shape
        self.f4 = B.FORMAT_F16X4 if build == "h4" else B.FORMAT_F32X4
        self.next = 0x10000000
        self.interp = {k: self.image(2 if k in ("uv0", "uv1") else 4 if k in ("mesh_normal", "color") else 1) for k in c["interp"]}
        self.out = {n: self.image(4 if M.channels_of(n) > 1 else 1) for n in M.output_names(c)}
        self.materials = [B.PBRMaterial.from_buffer_copy(M.material_words(m).tobytes()) for m in c["materials"]]
        self.textures = []
        for t in c["textures"]:
            texels = sum(m.shape[1] * m.shape[2] for m in t)
            ts = 4 if t[0].dtype == np.uint8 else 16
            self.textures.append(B.TextureArray(self.address(texels * ts * t[0].shape[0]), t[0].shape[2], t[0].shape[1], t[0].shape[0], len(t),
                                                B.NATIVE_FORMATS["RGBA8_UNORM" if ts == 4 else "RGBA32_FLOAT"], 0, texels * ts))
        self.layer_flags, self.flags, self.mip_bias = c["layers"], c["flags"], c["mip_bias"]
        self.camera = B.camera_from_bytes(c["camera"].tobytes())

    def address(self, size):
        a = self.next
        self.next += (size + 0xFFFF) & ~0xFFFF
        return a

    def image(self, channels, w=None, h=None):
        w, h = w or self.w, h or self.h
        B = self.B
        fmt, ts = {1: (B.FORMAT_F32, 4), 2: (B.FORMAT_F32X2, 8), 4: (self.f4, 8 if self.f4 == B.FORMAT_F16X4 else 16)}[channels]
        return B.Image2D(self.address(w * h * ts), w, h, w * ts, fmt)

    def args(self):
        B = self.B
        p = lambda d, k: ctypes.pointer(d[k]) if d.get(k) is not None else None  # noqa: E731
        self.keep = [B.MaterialInterpolants(*[p(self.interp, k) for k in M.INTERPOLANTS]),
                     (B.PBRMaterial * max(len(self.materials), 1))(*self.materials), (B.TextureArray * max(len(self.textures), 1))(*self.textures),
                     B.GBuffer(p(self.out, "base_color"), p(self.out, "normal"), p(self.out, "material"), None, p(self.out, "emissive"), p(self.out, "occlusion")),
                     B.PBRLayers(0, 0.0, 0.0, 0, *[p(self.out, k) for k in B.PBR_LAYER_PLANES])]
        desc = B.MaterialFetchDesc(self.keep[1], self.keep[2] if self.textures else None, len(self.materials), len(self.textures), self.layer_flags, self.flags, self.mip_bias,
                                   (ctypes.c_uint32 * 3)(0, 0, 0))
        self.keep.append(desc)
        return ctypes.byref(self.keep[0]), ctypes.byref(desc), ctypes.byref(self.camera), ctypes.byref(self.keep[3]), ctypes.byref(self.keep[4])

    def check(self, lib):
        status = lib.mifx_pbr_material_fetch_check(*self.args())
        return status, lib.mifx_last_error().decode()


BY_NAME = {c["name"]: c for c in M.cases()}


@pytest.mark.parametrize("build", ["fp32", "h4"])
def test_both_builds_export_both_entries_and_agree_on_the_structs(build):
    from diligentfx_amd import binding as B

    lib = load(build)
    assert hasattr(lib, "mifx_pbr_material_fetch") and hasattr(lib, "mifx_pbr_material_fetch_check")
    for name, size in NEW_STRUCTS.items():
        assert lib.mifx_sizeof(name.encode()) == size == ctypes.sizeof(B.SIZEOF_NAMES[name]), name
    assert ctypes.sizeof(B.PBRTextureAttribs) == 48 and B.PBR_TEXTURE_COUNT == 16 and B.PBR_TEXTURE_SLOTS == M.SLOTS


@pytest.mark.parametrize("build", ["fp32", "h4"])
@pytest.mark.parametrize("name", ["a_minified", "l_every_layer", "m_every_layer_rgba8", "o_three_materials", "u_atlas_normal_map", "j_fallback_colour", "p_frame_1x1"])
def test_a_valid_call_passes_the_check(build, name):
    status, message = Call(BY_NAME[name], build).check(load(build))
    assert status == 0, message


def refusals():
    """(what, the case it starts from, how the call is broken, words its message must hold)"""
    B_LAYER_IRIDESCENCE, B_LAYER_ANISOTROPY = 8, 4

    def two_materials(change, layers=0):
        def f(k):
            k.materials.append(copy.deepcopy(k.materials[0]))
            change(k.materials[1])
            k.layer_flags |= layers
            for n, _, bit in M.LAYER_OUT:
                if (layers & bit) and n not in k.out and n != "clearcoat_normal":
                    k.out[n] = k.image(4 if M.channels_of(n) > 1 else 1)
        return f

    def set_workflow(v):
        def f(m):
            m.basic.Workflow = v
        return f

    def unlit(k):
        k.materials[0].basic.Workflow = 2

    def spec_factor(k):
        k.materials[0].basic.SpecularFactor[1] = 0.5

    def ior(m):
        m.iridescence[1] = 1.7

    def rot(m):
        m.anisotropy[1] = 0.1

    def region(k):
        k.materials[0].textures[0].AtlasUVScaleAndBias[2] = 0.9  # 0.9 + 0.25 > 1

    def texture_index(k):
        k.materials[0].texture[2] = len(k.textures)

    def no_uv(k):
        k.interp.pop("uv0")

    def missized(k):
        k.out["normal"] = k.image(4, w=k.w + 1)

    def misformatted(k):
        k.interp["uv0"] = k.image(4)

    def alias_out(k):
        k.out["material"] = k.out["base_color"]

    def alias_in(k):
        k.out["occlusion"] = k.interp["depth"]

    def cc_normal_unwanted(k):
        k.layer_flags = 1
        k.out["clearcoat"], k.out["clearcoat_normal"] = k.image(4), k.image(4)

    def missing_layer_plane(k):
        k.out.pop("sheen")

    def texture_format(k):
        k.textures[0].format = 5

    def texture_mips(k):
        k.textures[0].mips = 6

    def texture_pitch(k):
        k.textures[0].slice_pitch_bytes = 16

    def no_depth(k):
        k.interp.pop("depth")

    def no_base_colour(k):
        k.out.pop("base_color")

    def bad_flags(k):
        k.flags = 8

    def bad_layers(k):
        k.layer_flags = 32

    return [
        ("mixed workflows", "a_minified", two_materials(set_workflow(1)), ["materials[1]", "Workflow"]),
        ("iridescence IOR differs", "a_minified", two_materials(ior, B_LAYER_IRIDESCENCE), ["materials[1]", "iridescence.IOR"]),
        ("anisotropy rotation differs", "a_minified", two_materials(rot, B_LAYER_ANISOTROPY), ["materials[1]", "anisotropy.Rotation"]),
        ("specular factors not 1", "i_specular_glossiness", spec_factor, ["materials[0]", "SpecularFactor"]),
        ("unlit", "a_minified", unlit, ["materials[0]", "UNLIT"]),
        ("texture index outside the table", "a_minified", texture_index, ["materials[0]", "texture[NORMAL]"]),
        ("atlas region outside [0, 1]", "q_atlas_wrap", region, ["textures[BASE_COLOR]", "AtlasUVScaleAndBias"]),
        ("map without UV planes", "a_minified", no_uv, ["texture[BASE_COLOR]", "uv0"]),
        ("mis-sized plane", "a_minified", missized, ["gbuffer->normal"]),
        ("mis-formatted plane", "a_minified", misformatted, ["interpolants->uv0"]),
        ("outputs alias", "a_minified", alias_out, ["gbuffer->material", "gbuffer->base_color"]),
        ("output aliases an interpolant", "a_minified", alias_in, ["gbuffer->occlusion", "interpolants->depth"]),
        ("clear-coat normal plane without a map", "a_minified", cc_normal_unwanted, ["layers->clearcoat_normal"]),
        ("layer on, plane missing", "l_every_layer", missing_layer_plane, ["layers->sheen"]),
        ("texture format", "a_minified", texture_format, ["textures[0].format"]),
        ("texture mips", "a_minified", texture_mips, ["textures[0].mips"]),
        ("texture slice pitch", "a_minified", texture_pitch, ["textures[0].slice_pitch_bytes"]),
        ("no depth", "a_minified", no_depth, ["interpolants->depth"]),
        ("no base-colour plane", "a_minified", no_base_colour, ["gbuffer->base_color"]),
        ("unknown flags", "a_minified", bad_flags, ["desc->flags"]),
        ("unknown layers", "a_minified", bad_layers, ["desc->layer_flags"]),
    ]


REFUSALS = refusals()


@pytest.mark.parametrize("build", ["fp32", "h4"])
@pytest.mark.parametrize("what,name,breakage,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_answers_invalid_arg_with_a_message_naming_the_argument(build, what, name, breakage, words):
    lib = load(build)
    k = Call(BY_NAME[name], build)
    assert k.check(lib)[0] == 0
    breakage(k)
    status, message = k.check(lib)
    assert status == INVALID_ARG, (what, status, message)
    for w in words:
        assert w in message, (what, w, message)


def test_the_entry_makes_the_same_checks_before_anything_else():
    """mifx_pbr_material_fetch refuses a broken call exactly as the check does, before it reads its context"""
    lib = load("fp32")
    k = Call(BY_NAME["a_minified"])
    k.materials[0].texture[2] = 99
    fake_ctx = ctypes.create_string_buffer(8192)
    assert lib.mifx_pbr_material_fetch(ctypes.cast(fake_ctx, ctypes.c_void_p), *k.args()) == INVALID_ARG
    assert "texture[NORMAL]" in lib.mifx_last_error().decode()
    assert lib.mifx_pbr_material_fetch(None, *Call(BY_NAME["a_minified"]).args()) == INVALID_ARG


def test_native_storage_build_answers_not_implemented():
    """The native-storage build exports the entry, makes the same checks and answers MIFX_ERR_NOT_IMPLEMENTED, as the shade's output stage does"""
    lib = load("h4")
    fake_ctx = ctypes.create_string_buffer(8192)  # (never read: the answer comes before the first use of the context)
    k = Call(BY_NAME["l_every_layer"], "h4")
    assert lib.mifx_pbr_material_fetch(ctypes.cast(fake_ctx, ctypes.c_void_p), *k.args()) == NOT_IMPLEMENTED
    assert "native-storage" in lib.mifx_last_error().decode()
    k.materials[0].texture[0] = 99
    assert lib.mifx_pbr_material_fetch(ctypes.cast(fake_ctx, ctypes.c_void_p), *k.args()) == INVALID_ARG
