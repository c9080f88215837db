"""The order in which the shade's launchers (diligentfx_amd/csrc/pbr.hip) refuse their arguments: a call with two faults is answered with the message of the check that comes
first.  The order is behaviour -- a caller reads mifx_last_error -- and the launchers share their checks, so a change to the sharing must not move it:

    1 unknown layer flag bits, 2 out_radiance, 4 the G-buffer planes (base_color, normal, material, depth, emissive, occlusion) and out_specular_ibl, 5 the lights,
    6 the shadow maps, 7 the layer planes (clear coat, sheen and its two tables, anisotropy, iridescence and its IOR, transmission), 8 the slice's color_alpha (OIT),
    9 the IBL: workflow, BRDF table, irradiance, prefiltered.

mifx_oit_shade_blend_check runs the layered launcher's whole sequence (steps 1, 4 - 9) and never touches a device: those cases need no GPU.  Steps 2 and 4's out_specular_ibl,
and the default shade's launcher, are reached through the device entries only, and those select the context's device (hipSetDevice) before they call the launcher: where
there is no device they answer MIFX_ERR_HIP and the launcher is never entered, so these cases carry the gpu mark.  They are called on a zero-filled context (as
tests/test_shade_output_abi.py calls its entry) and every call is refused in step 9 at the latest, in front of the launcher's first device call: nothing is launched,
allocated or copied.  The entries refuse a null `ibl` pointer themselves, so "no IBL" is a mifx_ibl with nothing in it, whose first refusal is the BRDF table's.
Frames are 4 x 3, tables 2 x 2; no pointer is ever read.  The messages are literals, as the library gave them before the launchers were taken apart."""
import ctypes

import pytest

W, H = 4, 3


class Call:
    """A call that would pass every check; a case breaks two things"""

    def __init__(self):
        from diligentfx_amd import binding as B

        self.B, self.keep = B, []
        self.gbuffer = dict(base_color=self.f4(), normal=self.f4(), material=self.f4(), depth=self.f1(), emissive=None, occlusion=None)
        self.layers = B.PBRLayers()
        self.alpha, self.out, self.spec, self.shadows = None, self.f4(), None, None
        self.camera, self.attribs = B.CameraAttribs(), B.PBRShadeAttribs()
        self.camera.fNearPlaneDepth, self.camera.fFarPlaneDepth = 0.0, 1.0
        self.lut = B.Image2D(0x3000, 2, 2, 2 * 8, B.FORMAT_F32X2)
        self.irr, self.pre = B.Cubemap(), B.Cubemap()
        self.irr.size, self.irr.mip_count, self.pre.size, self.pre.mip_count = 2, 1, 2, 2
        self.irr.mip_data[0], self.pre.mip_data[0], self.pre.mip_data[1] = 0x4000, 0x5000, 0x6000
        self.no_ibl = False

    def f1(self, w=W, h=H):
        return self.B.Image2D(0x1000, w, h, w * 4, self.B.FORMAT_F32)

    def f4(self, w=W, h=H):
        return self.B.Image2D(0x2000, w, h, w * 16, self.B.FORMAT_F32X4)

    def p(self, x):
        if x is None:
            return None
        self.keep.append(x)
        return ctypes.pointer(x)

    def layer(self, flag, **planes):
        self.layers.flags |= flag
        for name, image in planes.items():
            setattr(self.layers, name, self.p(image))

    def shadowed_light(self):
        self.attribs.LightCount = 1
        self.attribs.Lights[0].Type, self.attribs.Lights[0].ShadowMapIndex = 1, 0

    def shadow_maps(self, pcf):
        B = self.B
        maps = B.ShadowMapArray(0x7000, 2, 2, 1, 8, 16)
        self.shadows = B.PBRShadows(self.p(maps), self.p(B.PBRShadowMapInfo()), 1, pcf)

    def run(self, lib, entry):
        B = self.B
        g = B.GBuffer(*[self.p(self.gbuffer[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion")])
        ibl = B.IBL() if self.no_ibl else B.IBL(self.p(self.lut), self.p(self.irr), self.p(self.pre))
        cam, sa, sh = ctypes.byref(self.camera), ctypes.byref(self.attribs), self.p(self.shadows)
        if entry == "oit_check":
            s = B.TransparentSlice(g, self.p(self.layers), self.p(self.alpha))
            t = B.OITTargets(*[self.p(self.f4()) for _ in range(4)])
            rc = lib.mifx_oit_shade_blend_check(W, H, 0, ctypes.byref(s), None, cam, sa, ctypes.byref(ibl), sh, ctypes.byref(t))
        else:
            ctx, bg = ctypes.create_string_buffer(1 << 16), (ctypes.c_float * 4)()
            out, spec = self.p(self.out), self.p(self.spec)
            if entry == "layers":
                rc = lib.mifx_pbr_shade_execute_layers(ctx, ctypes.byref(g), ctypes.byref(self.layers), cam, sa, ctypes.byref(ibl), sh, bg, out, spec)
            elif entry == "shade":
                rc = lib.mifx_pbr_shade_execute(ctx, ctypes.byref(g), cam, sa, ctypes.byref(ibl), bg, out, spec)
            else:
                rc = lib.mifx_pbr_shade_execute_with_shadows(ctx, ctypes.byref(g), cam, sa, ctypes.byref(ibl), sh, bg, out, spec)
        return rc, lib.mifx_last_error().decode()


# ---- the faults, by the step that finds them
def flag_bits(c):
    c.layers.flags |= 1 << 9


def bad_out_radiance(c):
    c.out = c.f1()


def bad_base_color(c):
    c.gbuffer["base_color"] = c.f4(w=W + 1)


def depth_wrong_size(c):
    c.gbuffer["depth"] = c.f1(h=H + 2)


def bad_out_spec(c):
    c.spec = c.f4(w=W - 1)


def light_count_17(c):
    c.attribs.LightCount = 17


def shadowed_light_without_shadows(c):
    c.shadowed_light()


def pcf_size_4(c):
    c.shadowed_light()
    c.shadow_maps(4)


def bad_clearcoat(c):
    c.layer(c.B.PBR_LAYER_CLEAR_COAT, clearcoat=c.f4(h=H + 1))


def bad_sheen_lut(c):
    c.layer(c.B.PBR_LAYER_SHEEN, sheen=c.f4(), sheen_albedo_scaling_lut=c.B.Image2D(0x3000, 2, 2, 4, c.B.FORMAT_F32), preintegrated_charlie=c.B.Image2D(0x3000, 2, 2, 8, c.B.FORMAT_F32))


def bad_transmission(c):
    c.layer(c.B.PBR_LAYER_TRANSMISSION, transmission=c.f4())


def iridescence_ior_0(c):
    c.layer(c.B.PBR_LAYER_IRIDESCENCE, iridescence=c.f4())
    c.layers.iridescence_ior = 0.0


def bad_color_alpha(c):
    c.alpha = c.f1(w=W + 3)


def no_ibl(c):
    c.no_ibl = True


def unknown_workflow(c):
    c.attribs.Workflow = 7


def a_layer(c):  # mifx_pbr_shade_execute_layers hands an empty set to the default shade: a sound transmission plane keeps the call on the layered launcher
    c.layer(c.B.PBR_LAYER_TRANSMISSION, transmission=c.f1())


FLAGS = "layers: unknown flag bits 0x200"
OUT_RADIANCE = "out_radiance: format 1, expected 4"
DEPTH = "gbuffer.depth: size 4x5, expected 4x3"
SHADOWLESS = "light 0: ShadowMapIndex 0 needs `shadows` and an entry in shadow_maps"
SHADOWLESS_DEFAULT = "light 0: ShadowMapIndex 0 needs mifx_pbr_shade_execute_with_shadows and an entry in shadow_maps"
PCF = "shadows: PCF filter size 4 (2, 3, 5 or 7: PCF.fxh)"
CLEARCOAT = "layers.clearcoat: size 4x4, expected 4x3"
IOR = "layers.iridescence_ior 0"
COLOR_ALPHA = "slice color_alpha: size 7x3, expected 4x3"
NO_IBL = "brdf_lut: F32X2 or F32X4 image required"
WORKFLOW = "unknown PBR workflow 7"
OUT_SPEC = "out_specular_ibl: size 3x3, expected 4x3"

CASES = [
    # the layered launcher's whole sequence, no device anywhere: steps 1, 4 - 9
    ("oit_check", [flag_bits, bad_base_color], FLAGS),
    ("oit_check", [depth_wrong_size, light_count_17], DEPTH),
    ("oit_check", [shadowed_light_without_shadows, bad_clearcoat], SHADOWLESS),
    ("oit_check", [pcf_size_4, bad_sheen_lut], PCF),
    ("oit_check", [bad_clearcoat, bad_transmission], CLEARCOAT),
    ("oit_check", [iridescence_ior_0, no_ibl], IOR),
    ("oit_check", [bad_color_alpha, no_ibl], COLOR_ALPHA),
    ("oit_check", [bad_transmission, bad_color_alpha], "layers.transmission: format 4, expected 1"),
    ("oit_check", [no_ibl], NO_IBL),
    ("oit_check", [unknown_workflow], WORKFLOW),
    ("oit_check", [unknown_workflow, no_ibl], WORKFLOW),
    # launch_pbr_shade_layers through its entry: steps 1, 2, 4 - 7, and the IBL behind them
    ("layers", [flag_bits, bad_out_radiance], FLAGS),
    ("layers", [a_layer, bad_out_radiance, bad_base_color, no_ibl], OUT_RADIANCE),
    ("layers", [a_layer, depth_wrong_size, light_count_17, no_ibl], DEPTH),
    ("layers", [a_layer, bad_out_spec, light_count_17, no_ibl], OUT_SPEC),
    ("layers", [shadowed_light_without_shadows, bad_clearcoat, no_ibl], SHADOWLESS),
    ("layers", [pcf_size_4, bad_sheen_lut, no_ibl], PCF),
    ("layers", [bad_clearcoat, bad_transmission, no_ibl], CLEARCOAT),
    ("layers", [iridescence_ior_0, no_ibl], IOR),
    ("layers", [a_layer, unknown_workflow, no_ibl], WORKFLOW),
    ("layers", [a_layer, no_ibl], NO_IBL),
    # launch_pbr_shade through its two entries: out_radiance, steps 4 - 6, the IBL
    ("shade", [bad_out_radiance, bad_base_color, no_ibl], OUT_RADIANCE),
    ("shade", [depth_wrong_size, light_count_17, no_ibl], DEPTH),
    ("shade", [light_count_17, unknown_workflow, no_ibl], "LightCount 17 out of range"),
    ("shade", [shadowed_light_without_shadows, no_ibl], SHADOWLESS_DEFAULT),
    ("shade", [unknown_workflow, no_ibl], WORKFLOW),
    ("shade", [no_ibl], NO_IBL),
    ("shade_with_shadows", [pcf_size_4, unknown_workflow, no_ibl], PCF),
    ("shade_with_shadows", [bad_out_spec, pcf_size_4, no_ibl], OUT_SPEC),
]


@pytest.mark.parametrize("entry,faults,message", [pytest.param(e, fs, m, id=f"{e}-{'+'.join(f.__name__ for f in fs)}", marks=[] if e == "oit_check" else [pytest.mark.gpu])
                                                  for e, fs, m in CASES])
def test_the_earlier_check_answers(mifx_lib, entry, faults, message):
    c = Call()
    for fault in faults:
        fault(c)
    rc, err = c.run(mifx_lib, entry)
    print(f"{entry}: {rc} {err!r}")
    assert rc == -1 and err == message  # MIFX_ERR_INVALID_ARG


def test_each_fault_is_refused_on_its_own(mifx_lib):
    """Every fault the cases pair is a fault by itself (the pairs would prove nothing otherwise), and the call they break is accepted"""
    rc, err = Call().run(mifx_lib, "oit_check")
    assert rc == 0, err
    for fault in (flag_bits, bad_base_color, depth_wrong_size, light_count_17, shadowed_light_without_shadows, pcf_size_4, bad_clearcoat, bad_sheen_lut, bad_transmission,
                  iridescence_ior_0, bad_color_alpha, no_ibl, unknown_workflow):
        c = Call()
        fault(c)
        rc, err = c.run(mifx_lib, "oit_check")
        assert rc == -1 and err, fault.__name__


@pytest.mark.gpu
def test_the_faults_of_the_planes_the_shade_writes_are_refused_on_their_own(mifx_lib):
    for fault in (bad_out_radiance, bad_out_spec):  # (the OIT draw writes neither plane)
        c = Call()
        a_layer(c)
        fault(c)
        no_ibl(c)
        rc, err = c.run(mifx_lib, "layers")
        assert rc == -1 and err != NO_IBL, fault.__name__
