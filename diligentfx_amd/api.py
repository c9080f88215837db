"""Thin Python host mirror of the reference's pass interfaces on top of the C ABI (include/mifx.h).

Names follow the reference classes (PostFXContext, ScreenSpaceAmbientOcclusion, ScreenSpaceReflection,
TemporalAntiAliasing, Bloom) and their PrepareResources / Execute / Get*SRV protocol; tensors are torch CUDA
float32 tensors used purely as device-memory handles.  Every call goes through libmifx.so."""
import ctypes

import torch

from . import binding as B


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _view(desc: B.Image2D, device):
    """Wraps an effect-owned plane (mifx_image2d) as a torch tensor view without copying (valid until the next prepare)."""
    # channels, bytes per element, element type.  The native-storage build hands out float16 / uint8 (R8_UNORM) / int32 (one packed R11G11B10_FLOAT texel) / int16 (the
    # bits of an R16_UNORM code) views:
    # widen() below turns any of them into float32 values.
    c, eb, ts = {B.FORMAT_F32: (1, 4, "<f4"), B.FORMAT_F32X2: (2, 4, "<f4"), B.FORMAT_F32X4: (4, 4, "<f4"), B.FORMAT_F16X4: (4, 2, "<f2"), B.FORMAT_F16: (1, 2, "<f2"),
                 B.FORMAT_F16X2: (2, 2, "<f2"), B.FORMAT_U8: (1, 1, "|u1"), B.FORMAT_R11G11B10: (1, 4, "<i4"), B.FORMAT_U16: (1, 2, "<i2")}[desc.format]
    pitch_f = desc.pitch_bytes // eb
    n = pitch_f * desc.height

    class _Holder:  # __cuda_array_interface__ provider
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {"shape": (n,), "typestr": ts, "data": (desc.data, False), "version": 2}
    flat = torch.as_tensor(h, device=device)
    rows = flat.view(desc.height, pitch_f)[:, : desc.width * c]
    return rows.view(desc.height, desc.width) if c == 1 else rows.unflatten(1, (desc.width, c))


def widen(t):
    """float32 values of a plane view of any storage type (see _view): float16 -> float, uint8 -> / 255 (R8_UNORM), int32 -> the three unsigned small floats of
    an R11G11B10_FLOAT texel (H, W, 3), int16 -> / 65535 (the bits of an R16_UNORM code)."""
    if t.dtype == torch.uint8:   # (the quotient in float64, then rounded: the correctly rounded code / N whatever the device's float32 division does)
        return (t.double() / 255.0).float()
    if t.dtype == torch.int16:
        return ((t.int() & 0xFFFF).double() / 65535.0).float()
    if t.dtype == torch.int32:
        def ufloat(v, m):  # 5 exponent bits, m mantissa bits, no sign
            e, f = v >> m, (v & ((1 << m) - 1)).float()
            sub = f * (2.0 ** -(14 + m))
            nrm = torch.ldexp(1.0 + f * (2.0 ** -m), (e - 15).int())
            r = torch.where(e == 0, sub, nrm)
            return torch.where(e == 31, torch.where(f == 0, torch.full_like(r, float("inf")), torch.full_like(r, float("nan"))), r)
        v = t.long() & 0xFFFFFFFF
        return torch.stack([ufloat(v & 0x7FF, 6), ufloat((v >> 11) & 0x7FF, 6), ufloat(v >> 22, 5)], dim=-1)
    return t.float()


class PostFXContext:
    """== Diligent::PostFXContext (PostProcess/Common/interface/PostFXContext.hpp:48-263)."""

    def __init__(self, device=0, sobol_256d=None, scrambling_tile=None):
        self.lib = B.load()
        self.device = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        dev = B.DeviceDesc(self.device.index or 0, _stream_ptr(self.device))
        info = B.PostFXCreateInfo()
        self._keep = []
        if sobol_256d is not None:
            s = bytes(bytearray(sobol_256d))
            t = bytes(bytearray(scrambling_tile))
            assert len(s) == 256 and len(t) == 128 * 128 * 8
            sb, tb = ctypes.create_string_buffer(s, len(s)), ctypes.create_string_buffer(t, len(t))
            self._keep += [sb, tb]
            info.sobol_256d = ctypes.cast(sb, ctypes.c_void_p)
            info.scrambling_tile = ctypes.cast(tb, ctypes.c_void_p)
        self.handle = ctypes.c_void_p()
        B.check(self.lib.mifx_postfx_create(ctypes.byref(dev), ctypes.byref(info), ctypes.byref(self.handle)))
        self.frame = None

    def close(self):
        if self.handle:
            self.lib.mifx_postfx_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync_stream(self):
        B.check(self.lib.mifx_postfx_set_stream(self.handle, _stream_ptr(self.device)))

    def set_static_ibl(self, enable=True):
        """mifx_postfx_set_static_ibl: the IBL maps handed to the shade do not change from call to call (their apron copy is then made once)."""
        B.check(self.lib.mifx_postfx_set_static_ibl(self.handle, ctypes.c_int32(1 if enable else 0)))

    FEATURE_FLAG_REVERSED_DEPTH, FEATURE_FLAG_HALF_PRECISION_DEPTH, FEATURE_FLAG_TEMPORAL_UPSCALING = 1, 2, 4  # PostFXContext.hpp:53-57

    def prepare_resources(self, index, width, height, feature_flags=0, output_width=None, output_height=None):
        self.frame = B.FrameDesc(index, width, height, output_width or width, output_height or height)
        self.sync_stream()
        B.check(self.lib.mifx_postfx_prepare(self.handle, ctypes.byref(self.frame), feature_flags))

    def execute(self, curr_depth, prev_depth, motion, curr_camera: B.CameraAttribs, prev_camera: B.CameraAttribs):
        imgs = [B.image(curr_depth), B.image(prev_depth), B.image(motion)]
        a = B.PostFXRenderAttribs(ctypes.pointer(imgs[0]), ctypes.pointer(imgs[1]), ctypes.pointer(imgs[2]), ctypes.pointer(curr_camera),
                                  ctypes.pointer(prev_camera))
        self._inputs = (curr_depth, prev_depth, motion)
        B.check(self.lib.mifx_postfx_execute(self.handle, ctypes.byref(a)))

    def _get(self, fn, *args):
        d = B.Image2D()
        B.check(fn(self.handle, *args, ctypes.byref(d)))
        return _view(d, self.device)

    def get_reprojected_depth(self):
        return self._get(self.lib.mifx_postfx_get_reprojected_depth)

    def get_closest_motion_vectors(self):
        return self._get(self.lib.mifx_postfx_get_closest_motion)

    def get_previous_depth(self):
        return self._get(self.lib.mifx_postfx_get_previous_depth)

    def get_2d_blue_noise(self, dimension):
        return self._get(self.lib.mifx_postfx_get_blue_noise, ctypes.c_int32(dimension))

    # -- PostFXContext's public texture helpers (PostFXContext.hpp:114, 168-172)
    def get_supported_features(self):
        """PostFXContext::GetSupportedFeatures as a dict of the four capability flags."""
        f = (ctypes.c_int32 * 4)()
        B.check(self.lib.mifx_postfx_get_supported_features(self.handle, f))
        return dict(zip(("TransitionSubresources", "TextureSubresourceViews", "CopyDepthToColor", "ShaderBaseVertexOffset"), (bool(v) for v in f)))

    def clear_render_target(self, target, clear_color):
        """PostFXContext::ClearRenderTarget: every texel of `target` := clear_color (4 floats, one per channel)."""
        self.sync_stream()
        i = B.image(target)
        B.check(self.lib.mifx_postfx_clear_render_target(self.handle, ctypes.byref(i), (ctypes.c_float * 4)(*clear_color)))

    def copy_texture_depth(self, src, dst):
        self.sync_stream()
        s, d = B.image(src), B.image(dst)
        B.check(self.lib.mifx_postfx_copy_texture_depth(self.handle, ctypes.byref(s), ctypes.byref(d)))

    def copy_texture_color(self, src, dst):
        self.sync_stream()
        s, d = B.image(src), B.image(dst)
        B.check(self.lib.mifx_postfx_copy_texture_color(self.handle, ctypes.byref(s), ctypes.byref(d)))

    # -- stand-alone full-screen passes recorded on this context's stream
    def tone_map(self, hdr, attribs: B.ToneMappingAttribs, ave_log_lum, flags=0, out=None):
        """Full-screen ToneMap() (ToneMapping.fxh:87-226), see mifx_tonemap_execute."""
        if out is None:
            out = torch.empty_like(hdr)
        i, o = B.image(hdr), B.image(out)
        B.check(self.lib.mifx_tonemap_execute(self.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(attribs), ctypes.c_float(ave_log_lum),
                                              ctypes.c_uint32(flags)))
        return out

    def copy_frame(self, color, depth, camera: B.CameraAttribs, tone_mapping: B.ToneMappingAttribs, ave_log_lum, tonemap_flags=0, grid: "B.CoordinateGridAttribs | None" = None,
                   grid_feature_flags=0, out=None):
        """The copy-frame draw with the coordinate grid (mifx_copy_frame_render, Hydrogent/shaders/HnCopyFrame.psh:27-63): ToneMap, the grid and axes over the 3x3 depth
        range, optional sRGB.  grid None or no plane / axis flag: the plain tone map."""
        if out is None:
            out = torch.empty_like(color)
        c, o = B.image(color), B.image(out)
        d = B.image(depth) if depth is not None else None
        B.check(self.lib.mifx_copy_frame_render(self.handle, ctypes.byref(c), ctypes.byref(d) if d is not None else None, ctypes.byref(camera) if camera is not None else None,
                                                ctypes.byref(tone_mapping), ctypes.c_float(ave_log_lum), ctypes.c_uint32(tonemap_flags),
                                                ctypes.byref(grid) if grid is not None else None, ctypes.c_uint32(grid_feature_flags), ctypes.byref(o)))
        return out

    def tone_map_native(self, hdr, attribs: B.ToneMappingAttribs, ave_log_lum, fmt: str, flags=0, pitch_bytes=None):
        """ToneMap() stored in the target's own format (mifx_tonemap_execute_native): torch.uint8 (H, pitch_bytes), bit-identical to
        image_export(tone_map(...), fmt) without the fp32 intermediate."""
        raw, dst = _native_target(self, hdr.shape[0], hdr.shape[1], fmt, pitch_bytes, hdr.device)
        i = B.image(hdr)
        B.check(self.lib.mifx_tonemap_execute_native(self.handle, ctypes.byref(i), ctypes.byref(dst), ctypes.byref(attribs), ctypes.c_float(ave_log_lum),
                                                     ctypes.c_uint32(flags)))
        return raw


def _native_target(ctx, h, w, fmt, pitch_bytes, device):
    ts = ctx.lib.mifx_native_format_texel_size(ctypes.c_uint32(B.NATIVE_FORMATS[fmt]))
    pitch = pitch_bytes or w * ts
    raw = torch.zeros((h, pitch), dtype=torch.uint8, device=device)
    return raw, B.NativeImage(raw.data_ptr(), w, h, pitch, B.NATIVE_FORMATS[fmt])


class IBLResources:
    """Device-side IBL inputs (mifx_ibl): BRDF LUT (H,W,2|4), irradiance cube and prefiltered cube as lists of (6*s, s, 4) mips."""

    def __init__(self, lut, irradiance_mips, prefiltered_mips):
        self.lut, self.irr, self.pre = lut, list(irradiance_mips), list(prefiltered_mips)
        self._lut_img = B.image(lut)
        self._irr, self._pre = B.Cubemap(), B.Cubemap()
        for cm, mips in ((self._irr, self.irr), (self._pre, self.pre)):
            cm.size, cm.mip_count = mips[0].shape[1], len(mips)
            for i, m in enumerate(mips):
                assert m.is_contiguous() and m.dtype == torch.float32 and m.shape == (6 * (cm.size >> i), cm.size >> i, 4), (i, m.shape)
                cm.mip_data[i] = m.data_ptr()
        self.struct = B.IBL(ctypes.pointer(self._lut_img), ctypes.pointer(self._irr), ctypes.pointer(self._pre))


def _cubemap(mips):
    cm = B.Cubemap()
    cm.size, cm.mip_count = mips[0].shape[1], len(mips)
    for i, m in enumerate(mips):
        assert m.is_contiguous() and m.dtype == torch.float32 and m.shape == (6 * (cm.size >> i), cm.size >> i, 4), (i, m.shape)
        cm.mip_data[i] = m.data_ptr()
    return cm


def _spheremap(mips):
    sm = B.SphereMap()
    sm.height, sm.width, sm.mip_count = mips[0].shape[0], mips[0].shape[1], len(mips)
    for i, m in enumerate(mips):
        assert m.is_contiguous() and m.dtype == torch.float32 and m.shape[2] == 4
        sm.mip_data[i] = m.data_ptr()
    return sm


def ibl_from_sphere_map(ctx: "PostFXContext", sphere_mips, irradiance_size=64, prefiltered_size=256, diffuse_samples=8192, specular_samples=256):
    """PrecomputeCubemaps from an equirectangular environment map (ENV_MAP_TYPE_SPHERE): returns (irradiance cube, [prefiltered cube mips]); mip 0 of the
    prefiltered cube (roughness 0) is the equirect -> cube conversion."""
    env = _spheremap(sphere_mips)
    dev = sphere_mips[0].device
    irr = torch.empty(6 * irradiance_size, irradiance_size, 4, device=dev)
    B.check(ctx.lib.mifx_ibl_compute_irradiance_map_sphere(ctx.handle, ctypes.byref(env), ctypes.c_void_p(irr.data_ptr()), ctypes.c_uint32(irradiance_size),
                                                           ctypes.c_uint32(diffuse_samples)))
    levels = prefiltered_size.bit_length()
    pre = []
    for m in range(levels):
        s = prefiltered_size >> m
        o = torch.empty(6 * s, s, 4, device=dev)
        B.check(ctx.lib.mifx_ibl_prefilter_env_map_sphere(ctx.handle, ctypes.byref(env), ctypes.c_void_p(o.data_ptr()), ctypes.c_uint32(s),
                                                          ctypes.c_float(m / max(levels - 1, 1)), ctypes.c_uint32(specular_samples)))
        pre.append(o)
    torch.cuda.synchronize(dev)
    return irr, pre


def cube_box_mips(cube):
    """(6*n, n, 4) -> full mip chain by 2x2 box filtering (how an application prepares the environment map SRV)."""
    n = cube.shape[1]
    mips = [cube.contiguous()]
    faces = cube.view(6, n, n, 4)
    while n > 1:
        faces = faces.view(6, n // 2, 2, n // 2, 2, 4).mean(dim=(2, 4))
        n //= 2
        mips.append(faces.reshape(6 * n, n, 4).contiguous())
    return mips


def image_import(ctx: "PostFXContext", raw, width, fmt: str, channels=4):
    """mifx_image_import: `raw` = torch.uint8 (H, pitch_bytes) holding a linear-layout image in the native format `fmt` (binding.NATIVE_FORMATS)
    -> float32 tensor (H, W[, channels])."""
    assert raw.dtype == torch.uint8 and raw.dim() == 2 and raw.stride(1) == 1
    h = raw.shape[0]
    out = torch.empty((h, width) if channels == 1 else (h, width, channels), dtype=torch.float32, device=raw.device)
    src = B.NativeImage(raw.data_ptr(), width, h, raw.stride(0), B.NATIVE_FORMATS[fmt])
    d = B.image(out)
    B.check(ctx.lib.mifx_image_import(ctx.handle, ctypes.byref(src), ctypes.byref(d)))
    return out


def image_export(ctx: "PostFXContext", img, fmt: str, pitch_bytes=None):
    """mifx_image_export: float32 tensor (H, W[, C]) -> torch.uint8 (H, pitch_bytes) in the native format `fmt`."""
    h, w = img.shape[0], img.shape[1]
    ts = ctx.lib.mifx_native_format_texel_size(ctypes.c_uint32(B.NATIVE_FORMATS[fmt]))
    pitch = pitch_bytes or w * ts
    raw = torch.zeros((h, pitch), dtype=torch.uint8, device=img.device)
    dst = B.NativeImage(raw.data_ptr(), w, h, pitch, B.NATIVE_FORMATS[fmt])
    s = B.image(img)
    B.check(ctx.lib.mifx_image_export(ctx.handle, ctypes.byref(s), ctypes.byref(dst)))
    return raw


ENVMAP_OPTION_FLAG_CONVERT_OUTPUT_TO_SRGB, ENVMAP_OPTION_FLAG_COMPUTE_MOTION_VECTORS = 1, 2


def render_env_map(ctx: "PostFXContext", env_mips, depth, color, motion, camera: B.CameraAttribs, prev_camera: B.CameraAttribs, tone_mapping: B.ToneMappingAttribs = None,
                   average_log_lum=0.3, mip_level=1.0, alpha=0.0, scale=(1.0, 1.0, 1.0), options=ENVMAP_OPTION_FLAG_COMPUTE_MOTION_VECTORS):
    """EnvMapRenderer::Prepare + Render (mifx_envmap_render): the environment colour (and motion vectors) on every pixel at the far-plane depth of
    `color` / `motion`, in place. Defaults = Hydrogent's call (HnRenderEnvMapTask.cpp:165-219): tone mapping NONE, mip 1, alpha 0, motion vectors."""
    sphere = env_mips[0].shape[0] != 6 * env_mips[0].shape[1]  # a cube mip is (6 n, n, 4); anything else is an equirectangular map
    env = _spheremap(env_mips) if sphere else _cubemap(env_mips)
    tm = tone_mapping if tone_mapping is not None else B.ToneMappingAttribs.default(0)
    a = B.EnvMapRenderAttribs(None if sphere else ctypes.pointer(env), average_log_lum, mip_level, alpha, options, (ctypes.c_float * 3)(*scale),
                              ctypes.pointer(env) if sphere else None)
    d, c = B.image(depth), B.image(color)
    m = B.image(motion) if motion is not None else None
    B.check(ctx.lib.mifx_envmap_render(ctx.handle, ctypes.byref(a), ctypes.byref(tm), ctypes.byref(camera), ctypes.byref(prev_camera), ctypes.byref(d), ctypes.byref(c),
                                       ctypes.byref(m) if m is not None else None))
    return color, motion


def precompute_ibl(ctx: "PostFXContext", env_cube, lut_size=512, irradiance_size=64, prefiltered_size=256, lut_samples=512, diffuse_samples=8192,
                   specular_samples=256):
    """PBR_Renderer::PrecomputeBRDF + PrecomputeCubemaps on the GPU (mifx_ibl_*); defaults are the reference's (PBR_Renderer.hpp:298,477-480)."""
    dev = ctx.device
    env_mips = cube_box_mips(env_cube)
    env = _cubemap(env_mips)
    ctx.sync_stream()
    lut = torch.empty(lut_size, lut_size, 2, device=dev)
    li = B.image(lut)
    B.check(ctx.lib.mifx_ibl_precompute_brdf_lut(ctx.handle, ctypes.byref(li), ctypes.c_uint32(lut_samples)))
    irr = torch.empty(6 * irradiance_size, irradiance_size, 4, device=dev)
    B.check(ctx.lib.mifx_ibl_compute_irradiance_map(ctx.handle, ctypes.byref(env), ctypes.c_void_p(irr.data_ptr()), ctypes.c_uint32(irradiance_size),
                                                    ctypes.c_uint32(diffuse_samples)))
    levels = prefiltered_size.bit_length()
    pre = []
    for m in range(levels):
        s = prefiltered_size >> m
        o = torch.empty(6 * s, s, 4, device=dev)
        B.check(ctx.lib.mifx_ibl_prefilter_env_map(ctx.handle, ctypes.byref(env), ctypes.c_void_p(o.data_ptr()), ctypes.c_uint32(s),
                                                   ctypes.c_float(m / max(levels - 1, 1)), ctypes.c_uint32(specular_samples)))
        pre.append(o)
    torch.cuda.synchronize(dev)
    return IBLResources(lut, [irr], pre)


def pbr_shade(ctx: "PostFXContext", gbuffer: dict, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: IBLResources, background=(0.0, 0.0, 0.0, 0.0),
              out_radiance=None, out_specular_ibl=None, want_specular_ibl=True, shadows=None):
    """PBR shading entry (mifx_pbr_shade_execute). gbuffer: dict with base_color, normal, material, depth [, emissive, occlusion].
    shadows: (shadow_map float32 tensor (slices, H, W), infos = sequence of 24-float PBRShadowMapInfo rows, pcf_filter_size) -> mifx_pbr_shade_execute_with_shadows."""
    ref = gbuffer["depth"]
    h, w = ref.shape
    if out_radiance is None:
        out_radiance = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    if out_specular_ibl is None and want_specular_ibl:
        out_specular_ibl = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    imgs = {k: B.image(gbuffer[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion") if gbuffer.get(k) is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    g = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    o0 = B.image(out_radiance)
    o1 = B.image(out_specular_ibl) if out_specular_ibl is not None else None
    bg = (ctypes.c_float * 4)(*background)
    ctx.sync_stream()
    if shadows is not None:
        sm, infos, pcf = shadows
        assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
        arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
        rows = (B.PBRShadowMapInfo * len(infos))()
        for i, r in enumerate(infos):
            rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
        sh = B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf)
        B.check(ctx.lib.mifx_pbr_shade_execute_with_shadows(ctx.handle, ctypes.byref(g), ctypes.byref(camera), ctypes.byref(attribs), ctypes.byref(ibl.struct), ctypes.byref(sh), bg,
                                                            ctypes.byref(o0), ctypes.byref(o1) if o1 is not None else None))
        return out_radiance, out_specular_ibl
    B.check(ctx.lib.mifx_pbr_shade_execute(ctx.handle, ctypes.byref(g), ctypes.byref(camera), ctypes.byref(attribs), ctypes.byref(ibl.struct), bg, ctypes.byref(o0),
                                           ctypes.byref(o1) if o1 is not None else None))
    return out_radiance, out_specular_ibl


def pbr_shade_layers(ctx: "PostFXContext", gbuffer: dict, layers: dict, flags: int, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: IBLResources,
                     background=(0.0, 0.0, 0.0, 0.0), iridescence_ior=1.3, anisotropy_rotation=0.0, want_specular_ibl=True, shadows=None):
    """The shade with material layers (mifx_pbr_shade_execute_layers).  layers: dict of the planes of mifx_pbr_layers (binding.PBR_LAYER_PLANES) that the set `flags`
    (binding.PBR_LAYER_*) needs; optional planes may be missing.  shadows: as pbr_shade()."""
    ref = gbuffer["depth"]
    h, w = ref.shape
    out_radiance = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    out_specular_ibl = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype()) if want_specular_ibl else None
    imgs = {k: B.image(gbuffer[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion") if gbuffer.get(k) is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    g = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    limgs = {k: B.image(layers[k]) for k in B.PBR_LAYER_PLANES if layers.get(k) is not None}
    ly = B.PBRLayers(flags, iridescence_ior, anisotropy_rotation, 0, *[ctypes.pointer(limgs[k]) if k in limgs else None for k in B.PBR_LAYER_PLANES])
    o0 = B.image(out_radiance)
    o1 = B.image(out_specular_ibl) if out_specular_ibl is not None else None
    bg = (ctypes.c_float * 4)(*background)
    ctx.sync_stream()
    sh = None
    if shadows is not None:
        sm, infos, pcf = shadows
        assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
        arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
        rows = (B.PBRShadowMapInfo * len(infos))()
        for i, r in enumerate(infos):
            rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
        sh = B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf)
    B.check(ctx.lib.mifx_pbr_shade_execute_layers(ctx.handle, ctypes.byref(g), ctypes.byref(ly), ctypes.byref(camera), ctypes.byref(attribs), ctypes.byref(ibl.struct),
                                                  ctypes.byref(sh) if sh is not None else None, bg, ctypes.byref(o0), ctypes.byref(o1) if o1 is not None else None))
    return out_radiance, out_specular_ibl


def pbr_shade_output(ctx: "PostFXContext", gbuffer: dict, layers, flags: int, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: IBLResources, output: dict = None,
                     shadows=None, motion=None, mesh_normal=None, background=(0.0, 0.0, 0.0, 0.0), iridescence_ior=1.3, anisotropy_rotation=0.0, want_specular_ibl=True,
                     out_color=None, out_specular_ibl=None):
    """The shade with its output stage (mifx_pbr_shade_output): debug views, in-shader tone mapping, alpha modes, unlit, highlight, loading animation, sRGB.
    layers / flags: as pbr_shade_layers(), or None / 0 for no layer.  output: dict with `renderer` (binding.PBRRendererShaderParameters) and any of debug_view,
    tone_mapping_mode, loading_animation, alpha_mode, alpha_mask_cutoff, unlit, flags (the fields of mifx_pbr_shade_output_desc).  motion: F32X2 plane, mesh_normal: 4-channel
    plane, or None.  shadows: as pbr_shade().  Returns (color, specular_ibl)."""
    ref = gbuffer["depth"]
    h, w = ref.shape
    if out_color is None:
        out_color = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    if out_specular_ibl is None and want_specular_ibl:
        out_specular_ibl = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    imgs = {k: B.image(gbuffer[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion") if gbuffer.get(k) is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    g = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    ly = None
    if layers is not None and flags:
        limgs = {k: B.image(layers[k]) for k in B.PBR_LAYER_PLANES if layers.get(k) is not None}
        ly = B.PBRLayers(flags, iridescence_ior, anisotropy_rotation, 0, *[ctypes.pointer(limgs[k]) if k in limgs else None for k in B.PBR_LAYER_PLANES])
    output = dict(output or {})
    renderer = output.pop("renderer", None)
    mi = B.image(motion) if motion is not None else None
    ni = B.image(mesh_normal) if mesh_normal is not None else None
    desc = B.PBRShadeOutputDesc(ctypes.pointer(renderer) if renderer is not None else None, output.pop("debug_view", 0), output.pop("tone_mapping_mode", 0),
                                output.pop("loading_animation", 0), output.pop("alpha_mode", 0), output.pop("alpha_mask_cutoff", 0.5), int(output.pop("unlit", 0)),
                                output.pop("flags", 0), 0, ctypes.pointer(mi) if mi is not None else None, ctypes.pointer(ni) if ni is not None else None)
    assert not output, f"unknown fields of mifx_pbr_shade_output_desc: {sorted(output)}"
    o0 = B.image(out_color)
    o1 = B.image(out_specular_ibl) if out_specular_ibl is not None else None
    bg = (ctypes.c_float * 4)(*background)
    ctx.sync_stream()
    sh = None
    if shadows is not None:
        sm, infos, pcf = shadows
        assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
        arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
        rows = (B.PBRShadowMapInfo * len(infos))()
        for i, r in enumerate(infos):
            rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
        sh = B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf)
    B.check(ctx.lib.mifx_pbr_shade_output(ctx.handle, ctypes.byref(g), ctypes.byref(ly) if ly is not None else None, ctypes.byref(camera), ctypes.byref(attribs),
                                          ctypes.byref(ibl.struct), ctypes.byref(sh) if sh is not None else None, ctypes.byref(desc), bg, ctypes.byref(o0),
                                          ctypes.byref(o1) if o1 is not None else None))
    return out_color, out_specular_ibl


class TextureArray:
    """A Texture2DArray of the material fetch (mifx_texture_array) in device memory.  mips: the chain as a list of numpy arrays, level k of shape (slices, max(1, h >> k),
    max(1, w >> k), 4): float32 -> RGBA32_FLOAT, uint8 -> RGBA8_UNORM.  The levels of a slice are packed one behind the other."""

    def __init__(self, mips, device):
        import numpy as np

        mips = [np.ascontiguousarray(m) for m in mips]
        slices, h, w, c = mips[0].shape
        assert c == 4 and mips[0].dtype in (np.float32, np.uint8) and all(m.dtype == mips[0].dtype for m in mips)
        for k, m in enumerate(mips):
            assert m.shape == (slices, max(1, h >> k), max(1, w >> k), 4), f"level {k} is {m.shape}"
        self.mips_np = mips
        self.data = torch.from_numpy(np.concatenate([m.reshape(slices, -1, 4) for m in mips], axis=1)).to(device)
        fmt = B.NATIVE_FORMATS["RGBA8_UNORM" if mips[0].dtype == np.uint8 else "RGBA32_FLOAT"]
        self.struct = B.TextureArray(self.data.data_ptr(), w, h, slices, len(mips), fmt, 0, self.data.stride(0) * self.data.element_size())

    @classmethod
    def from_level0(cls, level0, device, mips=None):
        """The chain box-filtered from level 0 (slices, h, w, 4): each level averages the 2 x 2 (at an odd size: the first 2 * n) texels of the level above; uint8 levels are
        rounded to nearest.  mips: the number of levels (default: down to 1 x 1)."""
        import numpy as np

        level0 = np.asarray(level0)
        chain, cur = [level0], level0.astype(np.float32)
        while (mips is None or len(chain) < mips) and max(cur.shape[1], cur.shape[2]) > 1:
            h, w = max(1, cur.shape[1] // 2), max(1, cur.shape[2] // 2)
            ys, xs = (2 if cur.shape[1] > 1 else 1), (2 if cur.shape[2] > 1 else 1)
            cur = cur[:, :h * ys, :w * xs].reshape(cur.shape[0], h, ys, w, xs, 4).mean(axis=(2, 4), dtype=np.float32)
            chain.append(np.clip(np.rint(cur), 0, 255).astype(np.uint8) if level0.dtype == np.uint8 else cur)
        return cls(chain, device)


def Material(basic=None, textures=None, fallback_color=(1.0, 1.0, 1.0, 1.0), sheen=(1.0, 1.0, 1.0, 1.0), anisotropy=(1.0, 0.0, 0.0, 0.0), iridescence=(1.0, 1.3, 100.0, 400.0),
             transmission=(1.0, 0.0, 0.0, 0.0)) -> B.PBRMaterial:
    """One record of the material table (mifx_pbr_material).  basic: binding.PBRMaterialBasicAttribs (default: metallic-roughness, every factor 1); textures: dict
    slot (binding.PBR_TEXTURE_*) -> (index into the call's texture table, binding.PBRTextureAttribs or None for UV0 / wrap / slice 0); a slot that is missing has no map.
    sheen: (colour factor rgb, roughness factor); anisotropy: (strength, rotation); iridescence: (factor, IOR, thickness minimum, maximum); transmission: (factor)."""
    m = B.PBRMaterial()
    if basic is None:
        basic = B.PBRMaterialBasicAttribs((ctypes.c_float * 4)(1, 1, 1, 1), (ctypes.c_float * 3)(1, 1, 1), 1.0, (ctypes.c_float * 3)(1, 1, 1), 1.0, 0, 0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0,
                                          (ctypes.c_float * 4)(0, 0, 0, 0))
    m.basic = basic
    m.sheen[:], m.anisotropy[:], m.iridescence[:], m.transmission[:] = list(sheen), list(anisotropy), list(iridescence), list(transmission)
    m.fallback_color[:] = list(fallback_color)
    for s in range(B.PBR_TEXTURE_COUNT):
        m.texture[s] = -1
        m.textures[s] = B.PBRTextureAttribs.make(uv_selector=-1)
    for s, (index, attribs) in (textures or {}).items():
        m.texture[s] = index
        m.textures[s] = attribs if attribs is not None else B.PBRTextureAttribs.make()
    return m


MATERIAL_INTERPOLANTS = ("depth", "uv0", "uv1", "mesh_normal", "color", "face", "material_index")
_MATERIAL_LAYER_OUTPUTS = (("clearcoat", B.PBR_LAYER_CLEAR_COAT, 4), ("sheen", B.PBR_LAYER_SHEEN, 4), ("anisotropy", B.PBR_LAYER_ANISOTROPY, 4),
                           ("iridescence", B.PBR_LAYER_IRIDESCENCE, 4), ("transmission", B.PBR_LAYER_TRANSMISSION, 1))


def pbr_material_fetch(ctx: "PostFXContext", interpolants: dict, materials, textures, camera: B.CameraAttribs, layer_flags=0, flags=0, mip_bias=0.0, gbuffer: dict = None,
                       layers: dict = None, want_emissive=True, want_occlusion=True, check_only=False):
    """The material fetch (mifx_pbr_material_fetch): the head of the reference's pixel shader over interpolant planes.  interpolants: dict with `depth` and any of uv0, uv1,
    mesh_normal, color, face, material_index (MATERIAL_INTERPOLANTS); materials: sequence of binding.PBRMaterial (see Material()); textures: sequence of TextureArray.
    gbuffer / layers: planes to write into (a pixel without a fragment keeps their texels); planes that are missing are allocated zeroed.  Returns (gbuffer, layers): the dicts
    that pbr_shade_layers() and pbr_shade_output() take (gbuffer["depth"] is the interpolants' depth)."""
    depth = interpolants["depth"]
    h, w = depth.shape
    new = lambda c: torch.zeros((h, w, 4) if c == 4 else (h, w), device=depth.device, dtype=B.storage_dtype() if c == 4 else torch.float32)  # noqa: E731
    g, ly = dict(gbuffer or {}), dict(layers or {})
    for k in ("base_color", "normal", "material"):
        if g.get(k) is None:
            g[k] = new(4)
    if want_emissive and g.get("emissive") is None:
        g["emissive"] = new(4)
    if want_occlusion and g.get("occlusion") is None:
        g["occlusion"] = new(1)
    for k, bit, c in _MATERIAL_LAYER_OUTPUTS:
        if (layer_flags & bit) and ly.get(k) is None:
            ly[k] = new(c)
    if (layer_flags & B.PBR_LAYER_CLEAR_COAT) and ly.get("clearcoat_normal") is None and any(m.texture[B.PBR_TEXTURE_CLEAR_COAT_NORMAL] >= 0 for m in materials):
        ly["clearcoat_normal"] = new(4)
    iimgs = {k: B.image(interpolants[k]) for k in MATERIAL_INTERPOLANTS if interpolants.get(k) is not None}
    ip = B.MaterialInterpolants(*[ctypes.pointer(iimgs[k]) if k in iimgs else None for k in MATERIAL_INTERPOLANTS])
    gimgs = {k: B.image(g[k]) for k in ("base_color", "normal", "material", "emissive", "occlusion") if g.get(k) is not None}
    p = lambda k: ctypes.pointer(gimgs[k]) if k in gimgs else None  # noqa: E731
    gs = B.GBuffer(p("base_color"), p("normal"), p("material"), None, p("emissive"), p("occlusion"))
    limgs = {k: B.image(ly[k]) for k in B.PBR_LAYER_PLANES if ly.get(k) is not None}
    ls = B.PBRLayers(layer_flags, 0.0, 0.0, 0, *[ctypes.pointer(limgs[k]) if k in limgs else None for k in B.PBR_LAYER_PLANES])
    mats = (B.PBRMaterial * len(materials))(*materials)
    texs = (B.TextureArray * max(len(textures), 1))(*[t.struct for t in textures])
    desc = B.MaterialFetchDesc(mats, texs if textures else None, len(materials), len(textures), layer_flags, flags, mip_bias, (ctypes.c_uint32 * 3)(0, 0, 0))
    if check_only:
        B.check(ctx.lib.mifx_pbr_material_fetch_check(ctypes.byref(ip), ctypes.byref(desc), ctypes.byref(camera), ctypes.byref(gs), ctypes.byref(ls)))
        return None
    ctx.sync_stream()
    B.check(ctx.lib.mifx_pbr_material_fetch(ctx.handle, ctypes.byref(ip), ctypes.byref(desc), ctypes.byref(camera), ctypes.byref(gs), ctypes.byref(ls)))
    g["depth"] = depth
    return g, ly


PBR_TARGET_PLANES = ("normal", "base_color", "material", "ibl")


def pbr_shade_targets(ctx: "PostFXContext", gbuffer: dict, layers, flags: int, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: IBLResources, output: dict = None,
                      shadows=None, motion=None, mesh_normal=None, background=(0.0, 0.0, 0.0, 0.0), iridescence_ior=1.3, anisotropy_rotation=0.0, out_color=None, out_targets=None):
    """The shade with its output stage and the USD footer's G-buffer targets (mifx_pbr_shade_targets).  Arguments as pbr_shade_output(); output=None is the entry's NULL desc
    (view NONE, nothing on).  out_targets: dict of the four planes of PBR_TARGET_PLANES, or None.  Returns (color, normal, base_color, material, ibl)."""
    ref = gbuffer["depth"]
    h, w = ref.shape
    if out_color is None:
        out_color = torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype())
    if out_targets is None:
        out_targets = {k: torch.empty(h, w, 4, device=ref.device, dtype=B.storage_dtype()) for k in PBR_TARGET_PLANES}
    imgs = {k: B.image(gbuffer[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion") if gbuffer.get(k) is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    g = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    ly = None
    if layers is not None and flags:
        limgs = {k: B.image(layers[k]) for k in B.PBR_LAYER_PLANES if layers.get(k) is not None}
        ly = B.PBRLayers(flags, iridescence_ior, anisotropy_rotation, 0, *[ctypes.pointer(limgs[k]) if k in limgs else None for k in B.PBR_LAYER_PLANES])
    desc = None
    if output is not None:
        output = dict(output)
        renderer = output.pop("renderer", None)
        mi = B.image(motion) if motion is not None else None
        ni = B.image(mesh_normal) if mesh_normal is not None else None
        desc = B.PBRShadeOutputDesc(ctypes.pointer(renderer) if renderer is not None else None, output.pop("debug_view", 0), output.pop("tone_mapping_mode", 0),
                                    output.pop("loading_animation", 0), output.pop("alpha_mode", 0), output.pop("alpha_mask_cutoff", 0.5), int(output.pop("unlit", 0)),
                                    output.pop("flags", 0), 0, ctypes.pointer(mi) if mi is not None else None, ctypes.pointer(ni) if ni is not None else None)
        assert not output, f"unknown fields of mifx_pbr_shade_output_desc: {sorted(output)}"
    o0 = B.image(out_color)
    timgs = [B.image(out_targets[k]) for k in PBR_TARGET_PLANES]
    tg = B.PBRTargets(*[ctypes.pointer(i) for i in timgs])
    bg = (ctypes.c_float * 4)(*background)
    ctx.sync_stream()
    sh = None
    if shadows is not None:
        sm, infos, pcf = shadows
        assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
        arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
        rows = (B.PBRShadowMapInfo * len(infos))()
        for i, r in enumerate(infos):
            rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
        sh = B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf)
    B.check(ctx.lib.mifx_pbr_shade_targets(ctx.handle, ctypes.byref(g), ctypes.byref(ly) if ly is not None else None, ctypes.byref(camera), ctypes.byref(attribs),
                                           ctypes.byref(ibl.struct), ctypes.byref(sh) if sh is not None else None, ctypes.byref(desc) if desc is not None else None, bg,
                                           ctypes.byref(o0), ctypes.byref(tg)))
    return (out_color,) + tuple(out_targets[k] for k in PBR_TARGET_PLANES)


HYDROGENT_GBUFFER_FORMATS = {"base_color": "RGBA8_UNORM", "normal": "RGBA16_FLOAT", "material": "RG8_UNORM", "depth": "R32_FLOAT", "emissive": "RGBA16_FLOAT",
                             "occlusion": "R8_UNORM"}  # HnBeginFrameTask.cpp:63-69 (emissive / occlusion are not Hydrogent targets: same classes of format)


def pbr_shade_native(ctx: "PostFXContext", gbuffer: dict, width, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: IBLResources, background=(0.0, 0.0, 0.0, 0.0),
                     out_format="RGBA16_FLOAT", want_specular_ibl=True):
    """mifx_pbr_shade_execute_native. gbuffer: name -> (torch.uint8 (H, pitch_bytes) tensor, format name); returns the radiance (and IBL) targets as raw
    torch.uint8 (H, pitch) tensors of `out_format`."""
    h = gbuffer["depth"][0].shape[0]
    imgs = {k: B.NativeImage(t.data_ptr(), width, h, t.stride(0), B.NATIVE_FORMATS[f]) for k, (t, f) in gbuffer.items() if t is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    g = B.GBufferNative(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    dev = gbuffer["depth"][0].device
    raw0, o0 = _native_target(ctx, h, width, out_format, None, dev)
    raw1, o1 = _native_target(ctx, h, width, out_format, None, dev) if want_specular_ibl else (None, None)
    bg = (ctypes.c_float * 4)(*background)
    ctx.sync_stream()
    B.check(ctx.lib.mifx_pbr_shade_execute_native(ctx.handle, ctypes.byref(g), ctypes.byref(camera), ctypes.byref(attribs), ctypes.byref(ibl.struct), bg, ctypes.byref(o0),
                                                  ctypes.byref(o1) if o1 is not None else None))
    return raw0, raw1


def composite(ctx: "PostFXContext", color, specular_ibl, ssr, ssao, normal, base_color, material, lut, camera, ssr_scale=1.0, ssao_scale=1.0,
              tone_mapping=None, ave_log_lum=0.3, out=None):
    """SSR / SSAO composite (mifx_composite_execute), Hydrogent/shaders/HnPostProcess.psh:145-185."""
    if out is None:
        out = torch.empty_like(color)
    imgs = [B.image(t) for t in (color, specular_ibl, ssr, ssao, normal, base_color, material, lut)]
    a = B.CompositeAttribs(*[ctypes.pointer(i) for i in imgs], ctypes.pointer(camera), ssr_scale, ssao_scale,
                           ctypes.pointer(tone_mapping) if tone_mapping is not None else None, ave_log_lum)
    o = B.image(out)
    ctx.sync_stream()
    B.check(ctx.lib.mifx_composite_execute(ctx.handle, ctypes.byref(a), ctypes.byref(o)))
    return out


class CoordinateGridRenderer:
    """Components/CoordinateGridRenderer: the world-space grid planes and the X / Y / Z axes over a depth buffer (mifx_coordinate_grid_render)."""

    def __init__(self, ctx: "PostFXContext"):
        self.ctx = ctx

    def render(self, depth, camera: B.CameraAttribs, attribs: "B.CoordinateGridAttribs | None", feature_flags, color_target=None, raw=False):
        """CoordinateGridRenderer::Render.  color_target: blended in place (rgb; its alpha is left as it is).  raw: also return the shader's own RGBA as a float32
        (H, W, 4) tensor (the only output when there is no colour target)."""
        out = None
        if raw or color_target is None:
            out = torch.empty((depth.shape[0], depth.shape[1], 4), dtype=torch.float32, device=depth.device)
        d = B.image(depth)
        t = B.image(color_target) if color_target is not None else None
        o = B.image(out) if out is not None else None
        if o is not None:
            o.format = B.FORMAT_F32X4  # (fp32 texels in every build of the library)
        B.check(self.ctx.lib.mifx_coordinate_grid_render(self.ctx.handle, ctypes.byref(d), ctypes.byref(camera), ctypes.byref(attribs) if attribs is not None else None,
                                                         ctypes.c_uint32(feature_flags), ctypes.byref(t) if t is not None else None,
                                                         ctypes.byref(o) if o is not None else None))
        return out if out is not None else color_target


class ShadowMapManager:
    """Components/ShadowMapManager, the per-texel half: ConvertToFilterable (mifx_shadow_convert_to_filterable) and the look-up of Shadows.fxh for every pixel of a frame
    (mifx_shadow_map_filter).  Cascade distribution and shadow-map rendering stay with the rasteriser: the attribs are taken as given."""

    def __init__(self, ctx: "PostFXContext", shadow_mode=B.SHADOW_MODE_PCF, is_32bit_filterable=True):
        """ShadowMapManager::InitInfo::ShadowMode / Is32BitFilterableFmt (ShadowMapManager.cpp:98-102).  is_32bit_filterable=False: the filterable array is
        RG16_UNORM (VSM: int16 codes), RG16_FLOAT (EVSM2) or RGBA16_FLOAT (EVSM4), in both builds of the library."""
        if shadow_mode not in (B.SHADOW_MODE_PCF, B.SHADOW_MODE_VSM, B.SHADOW_MODE_EVSM2, B.SHADOW_MODE_EVSM4):
            raise ValueError(f"unknown shadow mode {shadow_mode}")
        self.ctx = ctx
        self.shadow_mode = shadow_mode
        self.is_32bit_filterable = bool(is_32bit_filterable)
        self.filterable = None

    def filterable_dtype(self):
        """The dtype of the filterable array's channels: float32, or float16 / int16 (the UNORM16 codes of VSM) for the 16-bit formats"""
        if self.is_32bit_filterable:
            return torch.float32
        return torch.int16 if self.shadow_mode == B.SHADOW_MODE_VSM else torch.float16

    def set_format_attribs(self, attribs: B.ShadowMapAttribs, filterable=None):
        """ShadowAttribs.bIs32BitEVSM for a 16-bit filterable array: 0, as ShadowMapManager.cpp:157 sets it for a format that is not RG32_FLOAT / RGBA32_FLOAT (the
        library refuses a 16-bit EVSM map with the flag set).  The format is that of `filterable`, the array actually handed over, or the manager's own when none is
        given.  With an fp32 array the caller's value is left alone: the flag then selects the exponent clamp only, and 0 with an fp32 map is a combination the
        library takes.  PCF has no filterable map: untouched."""
        narrow = (filterable.dtype != torch.float32) if filterable is not None else not self.is_32bit_filterable
        if narrow and self.shadow_mode != B.SHADOW_MODE_PCF:
            attribs.bIs32BitEVSM = 0
        return attribs

    @staticmethod
    def widen(filterable):
        """A filterable array read back as float32 values: float16 widens, the int16 codes of RG16_UNORM become code / 65535 (correctly rounded)"""
        if filterable.dtype == torch.int16:
            codes = (filterable.to(torch.int32) & 0xFFFF).to(torch.float64)
            return (codes / 65535.0).to(torch.float32)
        return filterable.to(torch.float32)

    def convert_to_filterable(self, shadow_map, attribs: B.ShadowMapAttribs, out=None):
        """ShadowMapManager::ConvertToFilterable.  shadow_map: float32 (slices, H, W).  Returns (and keeps) the filterable array, (slices, H, W, 2) for VSM /
        EVSM2 and (slices, H, W, 4) for EVSM4, of filterable_dtype() or the dtype of `out` (widen() reads a 16-bit one back as float32); PCF mode has none.  Into a
        16-bit array attribs.bIs32BitEVSM is set to 0 (set_format_attribs); into an fp32 one the attribs are used as given."""
        if self.shadow_mode == B.SHADOW_MODE_PCF:
            return None
        if out is None:
            out = torch.empty(tuple(shadow_map.shape) + (4 if self.shadow_mode == B.SHADOW_MODE_EVSM4 else 2,), dtype=self.filterable_dtype(), device=shadow_map.device)
        self.set_format_attribs(attribs, out)
        src, dst = B.shadow_map_array(shadow_map), B.filterable_shadow_map(out)
        self.ctx.sync_stream()
        B.check(self.ctx.lib.mifx_shadow_convert_to_filterable(self.ctx.handle, ctypes.byref(src), ctypes.byref(attribs), ctypes.c_uint32(self.shadow_mode), ctypes.byref(dst)))
        self.filterable = out
        return out

    def filter(self, ctx, depth, camera: B.CameraAttribs, attribs: B.ShadowMapAttribs, shadow_map=None, filterable_map=None, filter_across_cascades=False,
               best_cascade_search=False, cascade_info=False):
        """FilterShadowMap (PCF: reads shadow_map) / SampleFilterableShadowMap (reads filterable_map, by default the last result of convert_to_filterable) for every
        pixel of `depth`.  Returns the light amount (H, W), with cascade_info also the (H, W, 2) plane (float(iCascadeIdx), fNextCascadeBlendAmount)."""
        ctx = ctx or self.ctx
        light = torch.empty_like(depth)
        casc = torch.empty(tuple(depth.shape) + (2,), dtype=torch.float32, device=depth.device) if cascade_info else None
        params = B.ShadowFilterParams(self.shadow_mode, int(bool(filter_across_cascades)), int(bool(best_cascade_search)), 0)
        sm = B.shadow_map_array(shadow_map) if shadow_map is not None else None
        if filterable_map is None and self.shadow_mode != B.SHADOW_MODE_PCF:
            filterable_map = self.filterable
        if filterable_map is not None:
            self.set_format_attribs(attribs, filterable_map)
        fm = B.filterable_shadow_map(filterable_map) if filterable_map is not None else None
        d, o = B.image(depth), B.image(light)
        c = B.image(casc) if casc is not None else None
        ctx.sync_stream()
        B.check(ctx.lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(camera), ctypes.byref(attribs), ctypes.byref(params),
                                                   ctypes.byref(sm) if sm is not None else None, ctypes.byref(fm) if fm is not None else None, ctypes.byref(o),
                                                   ctypes.byref(c) if c is not None else None))
        return (light, casc) if cascade_info else light


def composite_selection(ctx: "PostFXContext", color, specular_ibl, ssr, ssao, normal, base_color, material, lut, camera, depth, selection_depth, closest_location,
                        selection: "B.SelectionAttribs", ssr_scale=1.0, ssao_scale=1.0, tone_mapping=None, ave_log_lum=0.3, out=None):
    """The composite with the selection tail (mifx_composite_execute_selection), Hydrogent/shaders/HnPostProcess.psh:145-185 + 211-241.  The outline colours of
    `selection` are used as given (ProcessSelection.hdr_colors converts them the way the reference's host does when TAA follows a tone-mapped frame)."""
    if out is None:
        out = torch.empty_like(color)
    imgs = [B.image(t) for t in (color, specular_ibl, ssr, ssao, normal, base_color, material, lut)]
    a = B.CompositeAttribs(*[ctypes.pointer(i) for i in imgs], ctypes.pointer(camera), ssr_scale, ssao_scale,
                           ctypes.pointer(tone_mapping) if tone_mapping is not None else None, ave_log_lum)
    si = [B.image(t) for t in (depth, selection_depth, closest_location)]
    inputs = B.SelectionCompositeInputs(*[ctypes.pointer(i) for i in si], ctypes.pointer(selection))
    o = B.image(out)
    ctx.sync_stream()
    B.check(ctx.lib.mifx_composite_execute_selection(ctx.handle, ctypes.byref(a), ctypes.byref(inputs), ctypes.byref(o)))
    return out


class ProcessSelection:
    """== Diligent::USD::HnProcessSelectionTask (Hydrogent/src/Tasks/HnProcessSelectionTask.cpp:302-369): the closest-selected-location plane (F32X2, the encoding of
    HnClosestSelectedLocation.fxh) by jump flooding a selection depth plane."""

    def __init__(self, ctx: "PostFXContext"):
        self.ctx, self.lib = ctx, ctx.lib
        self.handle = ctypes.c_void_p()
        B.check(self.lib.mifx_selection_create(ctx.handle, ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            self.lib.mifx_selection_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def execute(self, selection_depth, attribs: "B.SelectionAttribs"):
        d = B.image(selection_depth)
        self.ctx.sync_stream()
        return B.check(self.lib.mifx_selection_execute(self.handle, ctypes.byref(d), ctypes.byref(attribs)))

    def get_output(self):
        d = B.Image2D()
        B.check(self.lib.mifx_selection_get_output(self.handle, ctypes.byref(d)))
        return _view(d, self.ctx.device)

    @staticmethod
    def hdr_colors(attribs: "B.SelectionAttribs", tone_mapping: "B.ToneMappingAttribs | None", ave_log_lum):
        """A copy of `attribs` with the outline colours as HnPostProcessTask.cpp:843-850 hands them to the composite when TAA follows: ReverseExpToneMap of the rgb
        (fMiddleGray, AverageLogLum) when the tone mapping mode is not NONE, alpha as given."""
        out = B.SelectionAttribs.from_buffer_copy(bytes(attribs))
        if tone_mapping is not None and tone_mapping.iToneMappingMode != 0:
            lib = B.load()
            for name in ("outline_color", "occluded_outline_color"):
                src = getattr(attribs, name)
                ldr, hdr = (ctypes.c_float * 3)(*src[:3]), (ctypes.c_float * 3)()
                B.check(lib.mifx_reverse_exp_tone_map(ldr, ctypes.c_float(tone_mapping.fMiddleGray), ctypes.c_float(ave_log_lum), hdr))
                getattr(out, name)[:3] = list(hdr)
        return out


def _pbr_shadows(shadows):
    """mifx_pbr_shadows from (shadow_map float32 tensor (slices, H, W), infos, pcf_filter_size) as pbr_shade() takes it, or None; returns (struct or None, keep-alive)"""
    if shadows is None:
        return None, None
    sm, infos, pcf = shadows
    assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
    arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
    rows = (B.PBRShadowMapInfo * len(infos))()
    for i, r in enumerate(infos):
        rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
    return B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf), (arr, rows, sm)


def transparent_slice(s):
    """mifx_transparent_slice of one transparent draw.  s: dict with `gbuffer` (base_color, normal, material, depth [, emissive, occlusion]: the draw's own G-buffer, depth at
    the background value where it has no fragment) and optionally `layers` + `flags` [+ iridescence_ior, anisotropy_rotation] as pbr_shade_layers() takes them and
    `color_alpha`.  Returns (struct, keep-alive)."""
    g = s["gbuffer"]
    imgs = {k: B.image(g[k]) for k in ("base_color", "normal", "material", "depth", "emissive", "occlusion") if g.get(k) is not None}
    p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
    gb = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
    ly = limgs = None
    if s.get("layers") is not None and s.get("flags", 0):
        limgs = {k: B.image(s["layers"][k]) for k in B.PBR_LAYER_PLANES if s["layers"].get(k) is not None}
        ly = B.PBRLayers(s["flags"], s.get("iridescence_ior", 1.3), s.get("anisotropy_rotation", 0.0), 0, *[ctypes.pointer(limgs[k]) if k in limgs else None for k in B.PBR_LAYER_PLANES])
    alpha = B.image(s["color_alpha"]) if s.get("color_alpha") is not None else None
    return B.TransparentSlice(gb, ctypes.pointer(ly) if ly is not None else None, ctypes.pointer(alpha) if alpha is not None else None), (imgs, ly, limgs, alpha, s)


OIT_SLICE_PLANES = ("depth", "base_color", "material", "radiance", "specular_ibl", "color_alpha")  # the members of mifx_oit_slice, in order
OIT_TARGETS = ("color", "base_color", "material", "ibl")  # the members of mifx_oit_targets, in order


class OITResources:
    """== PBR_Renderer's OITResources (PBR_Renderer::CreateOITResources): K packed layers per pixel plus the tail, and the per-texel passes of the reference's layered
    order-independent transparency over them (include/mifx.h, "layered order-independent transparency").  A transparent draw is a slice: a dict with the planes of
    OIT_SLICE_PLANES (radiance / specular_ibl = what pbr_shade() returns for the slice's G-buffer; color_alpha optional; the layer entries read depth and base_color
    only).  targets: a dict with the four planes of OIT_TARGETS, blended in place."""

    def __init__(self, ctx: "PostFXContext", width, height, layer_count):
        self.ctx, self.lib = ctx, ctx.lib
        self.width, self.height, self.layer_count = width, height, layer_count
        self.plane_dtype = B.storage_dtype()  # the 4-channel texel of the library build: float32, or float16 (RGBA16_FLOAT) in the native-storage build
        self.handle = ctypes.c_void_p()
        B.check(self.lib.mifx_oit_create(ctx.handle, ctypes.c_uint32(width), ctypes.c_uint32(height), ctypes.c_uint32(layer_count), ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            self.lib.mifx_oit_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_targets(self):
        """The four targets of OIT_TARGETS, zeroed, in the 4-channel texel of the library build"""
        return {k: torch.zeros(self.height, self.width, 4, device=self.ctx.device, dtype=self.plane_dtype) for k in OIT_TARGETS}

    def to_planes(self, planes):
        """A slice or a set of targets with every 4-channel plane in the 4-channel texel of the library build (a float32 plane is rounded to binary16 in the
        native-storage build); the one-channel planes stay float32"""
        return {k: (v.to(self.plane_dtype).contiguous() if v is not None and v.dim() == 3 and v.shape[2] == 4 else v) for k, v in planes.items()}

    @staticmethod
    def _slices(slices):
        imgs = [{k: B.image(s[k]) for k in OIT_SLICE_PLANES if s.get(k) is not None} for s in slices]  # (kept alive by the caller's frame)
        arr = (B.OITSlice * max(len(slices), 1))(*[B.OITSlice(*[ctypes.pointer(m[k]) if k in m else None for k in OIT_SLICE_PLANES]) for m in imgs])
        return arr, imgs

    @staticmethod
    def _targets(targets):
        imgs = [B.image(targets[k]) for k in OIT_TARGETS]
        return B.OITTargets(*[ctypes.pointer(i) for i in imgs]), imgs

    def clear_layers(self):
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_clear_layers(self.handle))

    def update_layers(self, slice_, camera: B.CameraAttribs, opaque_depth=None):
        arr, keep = self._slices([slice_])
        od = B.image(opaque_depth) if opaque_depth is not None else None
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_update_layers(self.handle, arr, ctypes.byref(od) if od is not None else None, ctypes.byref(camera)))

    def apply_attenuation(self, targets):
        t, keep = self._targets(targets)
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_apply_attenuation(self.handle, ctypes.byref(t)))

    def blend(self, slice_, camera: B.CameraAttribs, targets, opaque_depth=None):
        arr, keep = self._slices([slice_])
        t, keep_t = self._targets(targets)
        od = B.image(opaque_depth) if opaque_depth is not None else None
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_blend(self.handle, arr, ctypes.byref(od) if od is not None else None, ctypes.byref(camera), ctypes.byref(t)))

    def shade_blend(self, slice_, camera: B.CameraAttribs, attribs: B.PBRShadeAttribs, ibl: "IBLResources", targets, opaque_depth=None, shadows=None):
        """One transparent draw shaded and blended in one launch (mifx_oit_shade_blend): slice_ as transparent_slice() takes it -- the draw's G-buffer, not shaded
        planes.  Equals pbr_shade_layers() on the slice (background 0) followed by blend(), bit for bit.  shadows: as pbr_shade()."""
        x, keep = transparent_slice(slice_)
        t, keep_t = self._targets(targets)
        od = B.image(opaque_depth) if opaque_depth is not None else None
        sh, keep_s = _pbr_shadows(shadows)
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_shade_blend(self.handle, ctypes.byref(x), ctypes.byref(od) if od is not None else None, ctypes.byref(camera), ctypes.byref(attribs),
                                              ctypes.byref(ibl.struct), ctypes.byref(sh) if sh is not None else None, ctypes.byref(t)))

    def build_layers(self, slices, camera: B.CameraAttribs, opaque_depth=None):
        arr, keep = self._slices(slices)
        od = B.image(opaque_depth) if opaque_depth is not None else None
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_build_layers(self.handle, arr, ctypes.c_uint32(len(slices)), ctypes.byref(od) if od is not None else None, ctypes.byref(camera)))

    def resolve(self, slices, camera: B.CameraAttribs, targets, opaque_depth=None):
        arr, keep = self._slices(slices)
        t, keep_t = self._targets(targets)
        od = B.image(opaque_depth) if opaque_depth is not None else None
        self.ctx.sync_stream()
        B.check(self.lib.mifx_oit_resolve(self.handle, arr, ctypes.c_uint32(len(slices)), ctypes.byref(od) if od is not None else None, ctypes.byref(camera), ctypes.byref(t)))

    def render(self, slices, targets, camera: B.CameraAttribs, opaque_depth=None):
        """HnBeginOITPassTask -> the transparent draws -> HnEndOITPassTask for up to binding.OIT_MAX_SLICES slices: build_layers, then resolve (the fused kernels, or the
        reference's sequence of launches: mifx_oit_set_fusion).  The targets are blended in place and returned."""
        self.build_layers(slices, camera, opaque_depth)
        self.resolve(slices, camera, targets, opaque_depth)
        return targets

    def get_layers(self):
        """The layers buffer as an int32 view (height, width, layer_count) of the uint32 words, valid until close()."""
        data, words = ctypes.c_void_p(), ctypes.c_uint64()
        B.check(self.lib.mifx_oit_get_layers(self.handle, ctypes.byref(data), ctypes.byref(words)))

        class _Holder:  # __cuda_array_interface__ provider
            pass

        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (words.value,), "typestr": "<i4", "data": (data.value, False), "version": 2}
        return torch.as_tensor(h, device=self.ctx.device).view(self.height, self.width, self.layer_count)

    def get_tail(self):
        """The tail plane (height, width, 2): the count in steps of 1 / 255, the transmittance product"""
        d = B.Image2D()
        B.check(self.lib.mifx_oit_get_tail(self.handle, ctypes.byref(d)))
        return _view(d, self.ctx.device)


def _export_history(fx, channel_shapes):
    """mifx_<effect>_export_history into fresh tensors of the prepared size; returns (*planes, frame_index)."""
    # (a plane of the prepared size; not the SSR output: inside a chain that plane may be deferred, mifx_ssr_run_deferred_cleanup)
    ref = fx.get_intermediate("hist_radiance") if fx._prefix == "ssr" else (fx._output() if fx._prefix != "taa" else fx._output(ctypes.c_int32(0)))
    h, w = ref.shape[0], ref.shape[1]
    planes = [torch.empty((h, w) + tuple(c), device=fx.ctx.device, dtype=B.plane_dtype(kind)) for c, kind in channel_shapes]
    imgs = [B.image(p) for p in planes]
    idx = ctypes.c_uint32(0)
    B.check(getattr(fx.lib, f"mifx_{fx._prefix}_export_history")(fx.handle, *[ctypes.byref(i) for i in imgs], ctypes.byref(idx)))
    return (*planes, idx.value)


def _import_history(fx, planes, frame_index):
    imgs = [B.image(p) for p in planes]
    B.check(getattr(fx.lib, f"mifx_{fx._prefix}_import_history")(fx.handle, *[ctypes.byref(i) for i in imgs], ctypes.c_uint32(frame_index)))


class _Effect:
    """Common PrepareResources / Execute / Get*SRV plumbing of the effect objects."""

    _prefix = None

    def __init__(self, ctx: PostFXContext):
        self.ctx, self.lib = ctx, ctx.lib
        self.handle = ctypes.c_void_p()
        B.check(getattr(self.lib, f"mifx_{self._prefix}_create")(ctx.handle, ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            getattr(self.lib, f"mifx_{self._prefix}_destroy")(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare_resources(self, feature_flags=0):
        B.check(getattr(self.lib, f"mifx_{self._prefix}_prepare")(self.handle, self.ctx.handle, ctypes.c_uint32(feature_flags)))

    def reset_history(self):
        B.check(getattr(self.lib, f"mifx_{self._prefix}_reset_history")(self.handle))

    def get_intermediate(self, name):
        d = B.Image2D()
        B.check(getattr(self.lib, f"mifx_{self._prefix}_get_intermediate")(self.handle, name.encode(), ctypes.byref(d)))
        return _view(d, self.ctx.device)

    def _output(self, *args):
        d = B.Image2D()
        B.check(getattr(self.lib, f"mifx_{self._prefix}_get_output")(self.handle, *args, ctypes.byref(d)))
        return _view(d, self.ctx.device)


class ScreenSpaceAmbientOcclusion(_Effect):
    """== Diligent::ScreenSpaceAmbientOcclusion (ScreenSpaceAmbientOcclusion.hpp:57-262)."""

    _prefix = "ssao"

    def execute(self, depth, normal, attribs: B.SSAOAttribs):
        i = [B.image(depth), B.image(normal)]
        ra = B.SSAORenderAttribs(self.ctx.handle, ctypes.pointer(i[0]), ctypes.pointer(i[1]), ctypes.pointer(attribs))
        return B.check(self.lib.mifx_ssao_execute(self.handle, ctypes.byref(ra)))

    def get_ambient_occlusion(self):
        return self._output()

    def set_fused_resolve(self, enable):
        """Test hook (mifx_debug_ssao_set_fused_resolve): A7 + A8 as one resolve over work lists (default) or as two full-frame passes."""
        B.check(self.lib.mifx_debug_ssao_set_fused_resolve(self.handle, ctypes.c_int32(1 if enable else 0)))

    def export_history(self):
        """(resolved AO, history length, frame index) the next frame would reproject (mifx_ssao_export_history)."""
        return _export_history(self, (((), "ao"), ((), "history_len")))

    def import_history(self, ao, history_length, frame_index):
        _import_history(self, (ao, history_length), frame_index)


class ScreenSpaceReflection(_Effect):
    """== Diligent::ScreenSpaceReflection (ScreenSpaceReflection.hpp:62-250)."""

    _prefix = "ssr"

    def execute(self, color, depth, normal, material, motion, attribs: B.SSRAttribs):
        i = [B.image(t) for t in (color, depth, normal, material, motion)]
        ra = B.SSRRenderAttribs(self.ctx.handle, *[ctypes.pointer(x) for x in i], ctypes.pointer(attribs))
        return B.check(self.lib.mifx_ssr_execute(self.handle, ctypes.byref(ra)))

    def get_ssr_radiance(self):
        return self._output()

    def set_clean_tiles(self, enable):
        """Test hook (mifx_debug_ssr_set_clean_tiles): R4 clears its targets only where an 8x8 tile needs it (default) or every texel outside the mask every frame."""
        B.check(self.lib.mifx_debug_ssr_set_clean_tiles(self.handle, ctypes.c_int32(1 if enable else 0)))

    def get_tile_flags(self):
        """(flags as an int array (tiles_y, tiles_x): 0 = the tile holds the cleared values in both ray planes, valid) (mifx_debug_ssr_get_tile_flags)."""
        tx, ty, valid = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int32(0)
        B.check(self.lib.mifx_debug_ssr_get_tile_flags(self.handle, None, ctypes.c_uint32(0), ctypes.byref(tx), ctypes.byref(ty), ctypes.byref(valid)))
        buf = (ctypes.c_uint32 * (tx.value * ty.value))()
        B.check(self.lib.mifx_debug_ssr_get_tile_flags(self.handle, buf, ctypes.c_uint32(len(buf)), ctypes.byref(tx), ctypes.byref(ty), ctypes.byref(valid)))
        return torch.tensor(list(buf), dtype=torch.int64).reshape(ty.value, tx.value), bool(valid.value)

    def export_history(self):
        """(accumulated radiance, variance, frame index) (mifx_ssr_export_history)."""
        return _export_history(self, (((4,), "colour"), ((), "variance")))

    def import_history(self, radiance, variance, frame_index):
        _import_history(self, (radiance, variance), frame_index)


class Bloom(_Effect):
    """== Diligent::Bloom (Bloom.hpp:58-150)."""

    _prefix = "bloom"

    def execute(self, color, attribs: B.BloomAttribs):
        i = B.image(color)
        ra = B.BloomRenderAttribs(self.ctx.handle, ctypes.pointer(i), ctypes.pointer(attribs))
        return B.check(self.lib.mifx_bloom_execute(self.handle, ctypes.byref(ra)))

    def get_bloom_texture(self):
        return self._output()


class DepthOfField(_Effect):
    """== Diligent::DepthOfField (PostProcess/DepthOfField/interface/DepthOfField.hpp:52-240)."""

    _prefix = "dof"
    FEATURE_FLAG_ENABLE_TEMPORAL_SMOOTHING, FEATURE_FLAG_ENABLE_KARIS_INVERSE = 1, 2

    def reset_history(self):
        """mifx_dof_reset_history (no reference counterpart): the temporal circle of confusion cleared as when the targets are created."""
        B.check(self.lib.mifx_dof_reset_history(self.handle))

    def execute(self, color, depth, attribs: B.DOFAttribs):
        i = [B.image(color), B.image(depth)]
        ra = B.DOFRenderAttribs(self.ctx.handle, ctypes.pointer(i[0]), ctypes.pointer(i[1]), ctypes.pointer(attribs))
        return B.check(self.lib.mifx_dof_execute(self.handle, ctypes.byref(ra)))

    def get_depth_of_field_texture(self):
        return self._output()

    def debug_set_last_pass(self, last_pass):
        B.check(self.lib.mifx_debug_dof_set_last_pass(self.handle, ctypes.c_uint32(last_pass)))

    @staticmethod
    def generate_kernel_points(ring_count, ring_density):
        import numpy as np

        out = (ctypes.c_float * 256)()
        n = ctypes.c_uint32(0)
        B.check(B.load().mifx_dof_generate_kernel_points(ctypes.c_int32(ring_count), ctypes.c_int32(ring_density), out, ctypes.c_uint32(128), ctypes.byref(n)))
        return np.array(out[:2 * n.value], np.float32).reshape(-1, 2)


class TemporalAntiAliasing(_Effect):
    """== Diligent::TemporalAntiAliasing (TemporalAntiAliasing.hpp:60-214)."""

    _prefix = "taa"
    FEATURE_FLAG_GAUSSIAN_WEIGHTING, FEATURE_FLAG_BICUBIC_FILTER, FEATURE_FLAG_YCOCG_COLOR_SPACE = 1, 2, 4

    def execute(self, color, attribs: B.TAAAttribs):
        i = B.image(color)
        ra = B.TAARenderAttribs(self.ctx.handle, ctypes.pointer(i), ctypes.pointer(attribs))
        return B.check(self.lib.mifx_taa_execute(self.handle, ctypes.byref(ra)))

    def get_accumulated_frame(self, is_prev_frame=False):
        return self._output(ctypes.c_int32(1 if is_prev_frame else 0))

    def export_history(self):
        """(accumulation buffer, frame index) (mifx_taa_export_history)."""
        return _export_history(self, (((4,), "colour"),))

    def import_history(self, color, frame_index):
        _import_history(self, (color,), frame_index)

    def set_history_skip(self, enable):
        """Test hook (mifx_debug_taa_set_history_skip): pixels whose history weight is exactly zero store their current colour without fetching the history (default) or run the whole body."""
        B.check(self.lib.mifx_debug_taa_set_history_skip(self.handle, ctypes.c_int32(1 if enable else 0)))

    @staticmethod
    def get_jitter_offset(frame_index, width, height):
        out = (ctypes.c_float * 2)()
        B.check(B.load().mifx_taa_get_jitter_offset(ctypes.c_uint32(frame_index), ctypes.c_uint32(width), ctypes.c_uint32(height), out))
        return out[0], out[1]


class AutoExposure:
    """Average scene luminance for ToneMap (mifx_autoexposure_*): the low-resolution luminance / mip chain / UpdateAverageLuminance sequence
    of the reference's light-scattering post-process (EpipolarLightScattering.cpp:2496-2506)."""

    def __init__(self, ctx: PostFXContext):
        self.ctx, self.lib = ctx, ctx.lib
        self.handle = ctypes.c_void_p()
        B.check(self.lib.mifx_autoexposure_create(ctx.handle, ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            self.lib.mifx_autoexposure_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def execute(self, scene_color, elapsed_time_s, light_adaptation=True):
        i = B.image(scene_color)
        B.check(self.lib.mifx_autoexposure_execute(self.handle, ctypes.byref(i), ctypes.c_float(elapsed_time_s), ctypes.c_int32(1 if light_adaptation else 0)))

    def reset(self, value=0.1):
        B.check(self.lib.mifx_autoexposure_reset(self.handle, ctypes.c_float(value)))

    def plane(self, name):
        d = B.Image2D()
        B.check(self.lib.mifx_autoexposure_get_plane(self.handle, name.encode(), ctypes.byref(d)))
        return _view(d, self.ctx.device)

    def average(self):
        """GetAverageSceneLuminance(): max(0.05, average); waits for the stream."""
        v = ctypes.c_float(0.0)
        B.check(self.lib.mifx_autoexposure_get_average(self.handle, ctypes.byref(v)))
        return v.value

    def tone_map(self, hdr, attribs: B.ToneMappingAttribs, flags=0, out=None):
        """ToneMap() with fAveLogLum read from the auto-exposure plane on the device."""
        if out is None:
            out = torch.empty_like(hdr)
        i, o = B.image(hdr), B.image(out)
        B.check(self.lib.mifx_tonemap_execute_auto(self.ctx.handle, ctypes.byref(i), ctypes.byref(o), ctypes.byref(attribs), self.handle, ctypes.c_uint32(flags)))
        return out


class Comm:
    """One rank's endpoint of the sharded chain (mifx_comm): RCCL over xGMI, or an in-process group for tests on one GPU."""

    COMM_ID_BYTES = 128

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    @staticmethod
    def unique_id() -> bytes:
        buf = (ctypes.c_uint8 * Comm.COMM_ID_BYTES)()
        B.check(B.load().mifx_comm_get_unique_id(buf))
        return bytes(buf)

    @classmethod
    def create(cls, ctx: "PostFXContext", uid: bytes, rank, world):
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * cls.COMM_ID_BYTES).from_buffer_copy(uid)
        B.check(ctx.lib.mifx_comm_create(ctx.handle, buf, ctypes.c_int32(rank), ctypes.c_int32(world), ctypes.byref(h)))
        return cls(ctx.lib, h)

    @classmethod
    def local_group(cls, ctx: "PostFXContext", world):
        arr = (ctypes.c_void_p * world)()
        B.check(ctx.lib.mifx_comm_create_local_group(ctx.handle, ctypes.c_int32(world), arr))
        return [cls(ctx.lib, ctypes.c_void_p(arr[i])) for i in range(world)]

    def info(self):
        r, w, k = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        B.check(self.lib.mifx_comm_get_info(self.handle, ctypes.byref(r), ctypes.byref(w), ctypes.byref(k)))
        return r.value, w.value, bool(k.value)

    def set_timing(self, enable):
        """mifx_comm_set_timing: bracket every exchange group of the frames that follow with timing events (read by stats())."""
        B.check(self.lib.mifx_comm_set_timing(self.handle, ctypes.c_int32(1 if enable else 0)))

    def stats(self):
        """mifx_comm_get_stats as a dict: what the endpoint is (ranks_in_communicator = ncclCommCount of the RCCL communicator), what it has moved since creation, and the
        exchange durations recorded since set_timing(True) (waits for those groups)."""
        st = B.CommStats()
        B.check(self.lib.mifx_comm_get_stats(self.handle, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in B.CommStats._fields_}

    def self_test(self, ctx: "PostFXContext", bytes_per_peer=1 << 16, timeout_ms=30000):
        """mifx_comm_self_test (collective): a known slab to and from every peer through the transport the frames use; raises MifxError with the transport's message."""
        B.check(self.lib.mifx_comm_self_test(self.handle, ctx.handle, ctypes.c_uint32(bytes_per_peer), ctypes.c_uint32(timeout_ms)))

    def close(self):
        if self.handle:
            self.lib.mifx_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class Chain:
    """The canonical caller of the hot path (== HnPostProcessTask, Hydrogent/src/Tasks/HnPostProcessTask.cpp:743-948):
    PBR shade -> PostFX prep -> SSR -> SSAO -> composite -> TAA -> Bloom -> ToneMap, one mifx_chain_execute per frame."""

    def __init__(self, device=0, sobol_256d=None, scrambling_tile=None):
        self.lib = B.load()
        self.device = torch.device("cuda", device) if not isinstance(device, torch.device) else device
        dev = B.DeviceDesc(self.device.index or 0, _stream_ptr(self.device))
        info = B.PostFXCreateInfo()
        self._keep = []
        if sobol_256d is not None:
            s, t = bytes(bytearray(sobol_256d)), bytes(bytearray(scrambling_tile))
            sb, tb = ctypes.create_string_buffer(s, len(s)), ctypes.create_string_buffer(t, len(t))
            self._keep += [sb, tb]
            info.sobol_256d, info.scrambling_tile = ctypes.cast(sb, ctypes.c_void_p), ctypes.cast(tb, ctypes.c_void_p)
        self.handle = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_create(ctypes.byref(dev), ctypes.byref(info), ctypes.byref(self.handle)))
        pf = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_get_postfx(self.handle, ctypes.byref(pf)))
        # a non-owning PostFXContext view (IBL precompute, stream updates)
        self.postfx = PostFXContext.__new__(PostFXContext)
        self.postfx.lib, self.postfx.device, self.postfx.handle, self.postfx._keep, self.postfx.frame = self.lib, self.device, pf, [], None
        self.postfx.close = lambda: None
        # per-frame attribs with the reference defaults; callers may edit them
        self.ssao_attribs, self.ssr_attribs = B.SSAOAttribs.default(), B.SSRAttribs.default()
        self.taa_attribs, self.bloom_attribs = B.TAAAttribs.default(), B.BloomAttribs.default()
        self.tone_mapping = B.ToneMappingAttribs.default(4)
        self.taa_flags = TemporalAntiAliasing.FEATURE_FLAG_BICUBIC_FILTER  # Hydrogent default (HnPostProcessTask.hpp:109)
        self.ave_log_lum, self.ssr_scale, self.ssao_scale = 0.3, 1.0, 1.0
        self.tonemap_flags = 1  # CONVERT_OUTPUT_TO_SRGB
        self.background = (0.02, 0.03, 0.05, 0.0)

    def close(self):
        if self.handle:
            self.lib.mifx_chain_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset_history(self):
        B.check(self.lib.mifx_chain_reset_history(self.handle))

    def bind_frame(self, frame_index, g: dict, ibl: "IBLResources", shade_attribs: B.PBRShadeAttribs, out):
        """Builds the mifx_chain_frame for a G-buffer dict (synth.make_frame layout). Returns an opaque object for execute()."""
        h, w = g["depth"].shape
        g = dict(g)
        for k in ("base_color", "normal", "material", "emissive"):  # 4-channel planes in the storage of this build (float16 with MIFX_STORAGE=h4; a no-op otherwise)
            if g.get(k) is not None and g[k].dtype != B.storage_dtype():
                g[k] = B.to_storage(g[k])
        imgs = {k: B.image(g[k]) for k in ("base_color", "normal", "material", "depth", "motion", "prev_depth")}
        for k in ("emissive", "occlusion"):
            if g.get(k) is not None:
                imgs[k] = B.image(g[k])
        p = lambda k: ctypes.pointer(imgs[k]) if k in imgs else None  # noqa: E731
        f = B.ChainFrame()
        f.frame = B.FrameDesc(frame_index, w, h, w, h)
        f.gbuffer = B.GBuffer(p("base_color"), p("normal"), p("material"), p("depth"), p("emissive"), p("occlusion"))
        f.motion, f.prev_depth = p("motion"), p("prev_depth")
        f.curr_camera, f.prev_camera = ctypes.pointer(g["camera"]), ctypes.pointer(g["prev_camera"])
        f.ibl, f.pbr = ctypes.pointer(ibl.struct), ctypes.pointer(shade_attribs)
        f.ssao, f.ssr = ctypes.pointer(self.ssao_attribs), ctypes.pointer(self.ssr_attribs)
        f.taa, f.bloom = ctypes.pointer(self.taa_attribs), ctypes.pointer(self.bloom_attribs)
        f.tone_mapping = ctypes.pointer(self.tone_mapping)
        f.ave_log_lum, f.ssr_scale, f.ssao_scale = self.ave_log_lum, self.ssr_scale, self.ssao_scale
        f.background[:] = list(self.background)
        f.taa_feature_flags, f.tonemap_flags = self.taa_flags, self.tonemap_flags
        o = B.image(out)
        return (f, o, imgs, g, ibl, shade_attribs, out)

    def execute(self, bound):
        B.check(self.lib.mifx_postfx_set_stream(self.postfx.handle, _stream_ptr(self.device)))
        self._last_bound = bound  # (effect_output("ssr") may have to run the deferred cleanup on this frame's depth / normal planes)
        return B.check(self.lib.mifx_chain_execute(self.handle, ctypes.byref(bound[0]), ctypes.byref(bound[1])))

    def execute_native(self, bound, fmt: str, pitch_bytes=None):
        """mifx_chain_execute_native: the frame in the copy-frame target's own format, torch.uint8 (H, pitch_bytes)."""
        out = bound[-1]
        raw, dst = _native_target(self.postfx, out.shape[0], out.shape[1], fmt, pitch_bytes, out.device)
        B.check(self.lib.mifx_postfx_set_stream(self.postfx.handle, _stream_ptr(self.device)))
        self._last_bound = bound
        B.check(self.lib.mifx_chain_execute_native(self.handle, ctypes.byref(bound[0]), ctypes.byref(dst)))
        return raw

    def set_auto_exposure(self, enable, elapsed_time_s=1.0 / 60.0, light_adaptation=True):
        """The final tone map takes fAveLogLum from the adapted average luminance of the Bloom output instead of self.ave_log_lum."""
        B.check(self.lib.mifx_chain_set_auto_exposure(self.handle, ctypes.c_int32(1 if enable else 0), ctypes.c_float(elapsed_time_s), ctypes.c_int32(1 if light_adaptation else 0)))
        self.auto_exposure = bool(enable)  # (sharded.py: the luminance rows are exchanged after phase 3)

    def effect_output(self, name):
        """Output plane of one of the chain's own effect objects: "ssao", "ssr", "taa", "bloom", "dof" (a view, valid until the next prepare)."""
        h = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_get_effect(self.handle, name.encode(), ctypes.byref(h)))
        if not h:
            raise ValueError(f"the chain has no '{name}' effect (not enabled)")
        d = B.Image2D()
        extra = (ctypes.c_int32(0),) if name == "taa" else ()
        if name == "ssr":
            if getattr(self, "_last_bound", None) is None:
                raise RuntimeError("Chain.effect_output('ssr'): no frame has been executed through this object yet (the deferred cleanup needs its depth / normal planes)")
            # the chain's composite evaluated the bilateral cleanup itself (MIFX_CHAIN_FUSE_SSR_CLEANUP_INTO_COMPOSITE): produce the plane from the frame just executed
            imgs = self._last_bound[2]
            normal = imgs["normal"]
            if getattr(self, "_shade_targets", False):  # (the passes behind the shade read the chain's normal target, the cleanup included)
                normal = B.Image2D()
                B.check(self.lib.mifx_chain_get_shade_target(self.handle, b"normal", ctypes.byref(normal)))
            B.check(self.lib.mifx_ssr_run_deferred_cleanup(h, ctypes.byref(imgs["depth"]), ctypes.byref(normal)))
        B.check(getattr(self.lib, f"mifx_{name}_get_output")(h, *extra, ctypes.byref(d)))
        return _view(d, self.device)

    FUSE_TONE_MAP_INTO_BLOOM, FUSE_SSR_MASK_INTO_SHADE, FUSE_SSR_CLEANUP_INTO_COMPOSITE, FUSE_SSAO_RESOLVE, FUSE_BLOOM_OUTPUT_ON_DEMAND, FUSE_COMPOSITE_INTO_TAA, FUSE_DEFAULT, FUSE_ALL, FUSE_EXPERIMENTAL, FUSE_EVERY_SWITCH = 1, 2, 4, 8, 16, 32, 31, 31, 32, 63

    def set_fusion_mask(self, mask):
        """mifx_chain_set_fusion_mask: every fusion switch of the chain (MIFX_CHAIN_FUSE_*; FUSE_DEFAULT = what a new chain has; the results are bit-identical either way)."""
        B.check(self.lib.mifx_chain_set_fusion_mask(self.handle, ctypes.c_uint32(mask)))

    def set_overlap(self, mode):
        """mifx_chain_set_overlap: 0 = one stream; 1 = PostFX prep + SSAO on a second stream beside the shade + SSR; 3 = three lanes (shade + prep + Hi-Z + SSAO | SSR +
        composite + TAA | Bloom) sliding across frames; 2 = also across frames (the next frame's prep +
        SSAO start as soon as this frame's TAA is done, under the Bloom pyramid) -- mode 2 requires that a frame's input planes are complete when execute is called;
        4 = the lanes of 3 with two frames in flight (the next frame's shade + SSAO beside this frame's SSR resolve / composite / TAA); 5 = 4 with the composite, TAA and depth
        of field on the Bloom lane (the next frame's ray march beside them)."""
        B.check(self.lib.mifx_chain_set_overlap(self.handle, ctypes.c_int32(int(mode))))

    def set_lane_edges(self, edges):
        """mifx_chain_set_lane_edges: "waiter<signal@frames,..." (mode 4: extra ordering between kernels of different lanes / frames; results do not depend on it)."""
        B.check(self.lib.mifx_chain_set_lane_edges(self.handle, (edges or "").encode()))

    def set_fusion(self, tone_map_into_bloom=True, ssr_mask_into_shade=True):
        """mifx_chain_set_fusion: pass fusion inside the chain (bit-identical results; on by default)."""
        B.check(self.lib.mifx_chain_set_fusion(self.handle, ctypes.c_int32(1 if tone_map_into_bloom else 0), ctypes.c_int32(1 if ssr_mask_into_shade else 0)))

    def effect(self, name):
        """Non-owning view of one of the chain's own effect objects ("ssao", "ssr", "taa", "bloom", "selection" once set_selection turned it on): intermediates,
        history export / import, the closest-selected-location plane."""
        cls = {"ssao": ScreenSpaceAmbientOcclusion, "ssr": ScreenSpaceReflection, "taa": TemporalAntiAliasing, "bloom": Bloom, "selection": ProcessSelection}[name]
        h = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_get_effect(self.handle, name.encode(), ctypes.byref(h)))
        fx = cls.__new__(cls)
        fx.ctx, fx.lib, fx.handle = self.postfx, self.lib, h
        fx.close = lambda: None  # the chain owns it
        return fx

    def set_effect_feature_flags(self, ssao_feature_flags=0, ssr_feature_flags=0):
        """FEATURE_FLAGS of the chain's SSAO / SSR objects (SSAO 2 = HALF_RESOLUTION, SSR 1 = PREVIOUS_FRAME)."""
        B.check(self.lib.mifx_chain_set_effect_feature_flags(self.handle, ctypes.c_uint32(ssao_feature_flags), ctypes.c_uint32(ssr_feature_flags)))

    def set_postfx_feature_flags(self, feature_flags):
        """PostFXContext::FEATURE_FLAGS of the chain's context (1 = FEATURE_FLAG_REVERSED_DEPTH)."""
        B.check(self.lib.mifx_chain_set_postfx_feature_flags(self.handle, ctypes.c_uint32(feature_flags)))

    def set_depth_of_field(self, attribs: "B.DOFAttribs | None", feature_flags=0):
        """DepthOfField::Execute between TAA and Bloom (HnPostProcessTask.cpp:899-909); None turns it off."""
        B.check(self.lib.mifx_chain_set_depth_of_field(self.handle, ctypes.byref(attribs) if attribs is not None else None, ctypes.c_uint32(feature_flags)))

    def set_material_layers(self, layers: "dict | None" = None, flags=0, iridescence_ior=1.3, anisotropy_rotation=0.0, shadows=None):
        """The chain's shade with material layers / shadow-mapped lights (mifx_chain_set_material_layers); arguments as pbr_shade_layers().  The tensors are kept alive here."""
        ly = sh = None
        self._layer_keep = (layers, shadows)
        if layers is not None and flags:
            imgs = {k: B.image(layers[k]) for k in B.PBR_LAYER_PLANES if layers.get(k) is not None}
            ly = B.PBRLayers(flags, iridescence_ior, anisotropy_rotation, 0, *[ctypes.pointer(imgs[k]) if k in imgs else None for k in B.PBR_LAYER_PLANES])
        if shadows is not None:
            sm, infos, pcf = shadows
            assert sm.dtype == torch.float32 and sm.dim() == 3 and sm.is_contiguous()
            arr = B.ShadowMapArray(sm.data_ptr(), sm.shape[2], sm.shape[1], sm.shape[0], sm.stride(1) * 4, sm.stride(0) * 4)
            rows = (B.PBRShadowMapInfo * len(infos))()
            for i, r in enumerate(infos):
                rows[i] = r if isinstance(r, B.PBRShadowMapInfo) else B.PBRShadowMapInfo.from_buffer_copy(r.astype("float32").tobytes())
            sh = B.PBRShadows(ctypes.pointer(arr), ctypes.cast(rows, ctypes.POINTER(B.PBRShadowMapInfo)), len(infos), pcf)
        B.check(self.lib.mifx_chain_set_material_layers(self.handle, ctypes.byref(ly) if ly is not None else None, ctypes.byref(sh) if sh is not None else None))

    def set_shade_output(self, desc: "dict | None" = None, targets=True, motion=None, mesh_normal=None):
        """The chain's shade with its output stage and, `targets`, the USD footer's G-buffer targets, which every later pass then reads (mifx_chain_set_shade_output).
        desc: the fields of mifx_pbr_shade_output_desc as pbr_shade_output() takes them, or None; set_shade_output(None, False) turns it off."""
        d = None
        self._output_keep = (motion, mesh_normal)
        if desc is not None:
            desc = dict(desc)
            renderer = desc.pop("renderer", None)
            mi = B.image(motion) if motion is not None else None
            ni = B.image(mesh_normal) if mesh_normal is not None else None
            d = B.PBRShadeOutputDesc(ctypes.pointer(renderer) if renderer is not None else None, desc.pop("debug_view", 0), desc.pop("tone_mapping_mode", 0),
                                     desc.pop("loading_animation", 0), desc.pop("alpha_mode", 0), desc.pop("alpha_mask_cutoff", 0.5), int(desc.pop("unlit", 0)), desc.pop("flags", 0), 0,
                                     ctypes.pointer(mi) if mi is not None else None, ctypes.pointer(ni) if ni is not None else None)
            assert not desc, f"unknown fields of mifx_pbr_shade_output_desc: {sorted(desc)}"
        B.check(self.lib.mifx_chain_set_shade_output(self.handle, ctypes.byref(d) if d is not None else None, ctypes.c_int32(1 if targets else 0)))
        self._shade_targets = bool(targets)

    def set_transparency(self, slices, layer_count=4):
        """Transparent draws in the chain (mifx_chain_set_transparency): every frame from now on builds `layer_count` OIT layers over `slices` (each as transparent_slice()
        takes it), attenuates the colour and the BaseColor / Material / IBL targets and shades and blends every slice behind the opaque shade.  Needs
        set_shade_output(..., targets=True).  None or an empty list turns it off.  The tensors are kept alive here (the library borrows them)."""
        if not slices:
            self._transparency_keep = None
            B.check(self.lib.mifx_chain_set_transparency(self.handle, ctypes.c_uint32(layer_count), None, ctypes.c_uint32(0)))
            return
        made = [transparent_slice(s) for s in slices]
        arr = (B.TransparentSlice * len(made))(*[m[0] for m in made])
        B.check(self.lib.mifx_chain_set_transparency(self.handle, ctypes.c_uint32(layer_count), arr, ctypes.c_uint32(len(made))))
        self._transparency_keep = [m[1] for m in made]

    def oit(self):
        """Non-owning view of the chain's OITResources (mifx_chain_get_effect "oit"); None until a frame ran with transparency on"""
        h = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_get_effect(self.handle, b"oit", ctypes.byref(h)))
        if not h:
            return None
        o = OITResources.__new__(OITResources)
        o.ctx, o.lib, o.handle, o.plane_dtype = self.postfx, self.lib, h, B.storage_dtype()
        o.close = lambda: None  # the chain owns it
        tail, data, words = B.Image2D(), ctypes.c_void_p(), ctypes.c_uint64()
        B.check(self.lib.mifx_oit_get_tail(h, ctypes.byref(tail)))
        B.check(self.lib.mifx_oit_get_layers(h, ctypes.byref(data), ctypes.byref(words)))
        o.width, o.height, o.layer_count = tail.width, tail.height, words.value // (tail.width * tail.height)
        return o

    def shade_target(self, name):
        """One of the chain's target planes ("normal", "base_color", "material", "ibl") as the last frame wrote it (mifx_chain_get_shade_target): a view."""
        d = B.Image2D()
        B.check(self.lib.mifx_chain_get_shade_target(self.handle, name.encode(), ctypes.byref(d)))
        return _view(d, self.device)

    def set_selection(self, attribs: "B.SelectionAttribs | None", selection_depth=None):
        """Selection highlighting (mifx_chain_set_selection): the jump flood of `selection_depth` and the composite's selection tail on every frame from now on; None
        turns it off.  The tensor is kept alive here (the library borrows it)."""
        if attribs is None:
            self._selection_keep = None
            B.check(self.lib.mifx_chain_set_selection(self.handle, None, None))
            return
        d = B.image(selection_depth)
        self._selection_keep = (selection_depth, attribs)
        B.check(self.lib.mifx_chain_set_selection(self.handle, ctypes.byref(attribs), ctypes.byref(d)))

    def set_coordinate_grid(self, attribs: "B.CoordinateGridAttribs | None", grid_feature_flags=0):
        """The coordinate grid and axes in the frame's last pass (mifx_chain_set_coordinate_grid; HnPostProcessTaskParams::Grid / GridFeatureFlags); None turns it off."""
        B.check(self.lib.mifx_chain_set_coordinate_grid(self.handle, ctypes.byref(attribs) if attribs is not None else None, ctypes.c_uint32(grid_feature_flags)))

    def auto_exposure_average(self):
        h = ctypes.c_void_p()
        B.check(self.lib.mifx_chain_get_auto_exposure(self.handle, ctypes.byref(h)))
        if not h:
            return None
        v = ctypes.c_float(0.0)
        B.check(self.lib.mifx_autoexposure_get_average(h, ctypes.byref(v)))
        return v.value

    # ---- row-band sharding with the exchanges inside the library (mifx_comm_* / mifx_chain_set_sharding / mifx_chain_execute_sharded)
    def set_sharding(self, comm: "Comm | None", row_cuts=None, max_motion_rows=0):
        if comm is None:
            B.check(self.lib.mifx_chain_set_sharding(self.handle, None, None, ctypes.c_int32(0)))
            return
        cuts = (ctypes.c_int32 * len(row_cuts))(*row_cuts)
        B.check(self.lib.mifx_chain_set_sharding(self.handle, comm.handle, cuts, ctypes.c_int32(max_motion_rows)))
        self._keep.append(comm)

    def execute_sharded(self, bound):
        B.check(self.lib.mifx_postfx_set_stream(self.postfx.handle, _stream_ptr(self.device)))
        self._last_bound = bound
        return B.check(self.lib.mifx_chain_execute_sharded(self.handle, ctypes.byref(bound[0]), ctypes.byref(bound[1])))

    def execute_band(self, bound):
        """mifx_chain_execute_band: the phases (and lanes) of execute_sharded for the band of set_row_band, exchanges left out -- one rank's compute side (tools)."""
        B.check(self.lib.mifx_postfx_set_stream(self.postfx.handle, _stream_ptr(self.device)))
        self._last_bound = bound
        return B.check(self.lib.mifx_chain_execute_band(self.handle, ctypes.byref(bound[0]), ctypes.byref(bound[1])))

    # ---- row-band sharding (mifx_chain_set_row_band / execute_phase / get_shard_info / get_shard_plane)
    def set_row_band(self, row_begin, row_end, max_motion_rows):
        B.check(self.lib.mifx_chain_set_row_band(self.handle, ctypes.c_int32(row_begin), ctypes.c_int32(row_end), ctypes.c_int32(max_motion_rows)))

    def execute_phase(self, bound, phase):
        B.check(self.lib.mifx_postfx_set_stream(self.postfx.handle, _stream_ptr(self.device)))
        self._last_bound = bound
        return B.check(self.lib.mifx_chain_execute_phase(self.handle, ctypes.byref(bound[0]), ctypes.byref(bound[1]), ctypes.c_int32(phase)))

    def shard_info(self, bound):
        info = B.ShardInfo()
        B.check(self.lib.mifx_chain_get_shard_info(self.handle, ctypes.byref(bound[0]), ctypes.byref(info)))
        return info

    def shard_plane_image(self, name):
        """The same plane as an image view (H, W[, C]) in its own texel type."""
        d = B.Image2D()
        B.check(self.lib.mifx_chain_get_shard_plane(self.handle, name.encode(), ctypes.byref(d)))
        return _view(d, self.device)

    def shard_plane(self, name):
        """Contiguous (height, pitch_floats) torch view (no copy) of one of the planes that move between ranks: a block of rows is one
        contiguous slab, padding included.  Valid until the next prepare that changes the size."""
        d = B.Image2D()
        B.check(self.lib.mifx_chain_get_shard_plane(self.handle, name.encode(), ctypes.byref(d)))
        pitch_f = d.pitch_bytes // 4

        class _Holder:
            pass

        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (d.height * pitch_f,), "typestr": "<f4", "data": (d.data, False), "version": 2}
        return torch.as_tensor(h, device=self.device).view(d.height, pitch_f)
