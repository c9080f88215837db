// api_oit.cpp -- C ABI of the layered order-independent transparency (include/mifx.h: mifx_oit_*): the argument checks of its entries and the sequencing of the six
// kernels, whose launchers are in oit.hip (mifx_oit_host.h), and of mifx_oit_shade_blend, one transparent draw shaded and blended by one kernel of pbr.hip.
#include "mifx_objects.h"
#include "mifx_oit_host.h"

using namespace mifx;

// The fused kernels are the default: 2.0 - 3.3 times faster than the sequence at 3840 x 2160, K = 4, L = 2 .. 8, both shapes at the device's copy rate for the bytes
// they move (profiles/oit_bench.json, tools/oit_bench.py; mifx_oit_set_fusion(0) is the sequence).
static bool g_oit_fusion = true;

namespace
{
mifx_status create_check(uint32_t width, uint32_t height, uint32_t layer_count, const char* who)
{
    MIFX_REQUIRE(layer_count >= 1u && layer_count <= uint32_t(MIFX_OIT_MAX_LAYERS), "%s: layer_count %u is outside 1 .. %d", who, layer_count, MIFX_OIT_MAX_LAYERS);
    MIFX_REQUIRE(width >= 1u && height >= 1u && width <= 16384u && height <= 16384u, "%s: %ux%u is empty or larger than 16384", who, width, height);
    return MIFX_OK;
}

struct OitFrameK
{
    OitSlicesK  tab;
    OitTargetsK targets;
    Img         opaque;
    OitCamK     cam;
};

// every argument check of the entries that take slices, an opaque depth, a camera or targets, for an object of w x h
mifx_status frame_check(uint32_t w, uint32_t h, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                        const mifx_oit_targets* targets, const char* who, OitFrameK& f)
{
    f = OitFrameK{};
    MIFX_REQUIRE(count <= uint32_t(MIFX_OIT_MAX_SLICES), "%s: %u slices are more than MIFX_OIT_MAX_SLICES (%d)", who, count, MIFX_OIT_MAX_SLICES);
    MIFX_REQUIRE(count == 0u || (slices != nullptr && camera != nullptr), "%s: null argument (slices, camera)", who);
    if (camera) f.cam = make_oitcamk(*camera);
    if (opaque_depth) MIFX_CHECK(to_img_wh(opaque_depth, MIFX_FORMAT_F32, w, h, "opaque_depth", f.opaque));
    Img im;
    for (uint32_t i = 0; i < count; ++i)
    {
        const mifx_oit_slice& s = slices[i];
        OitSliceK&            o = f.tab.s[i];
        MIFX_REQUIRE(s.depth != nullptr && s.base_color != nullptr, "%s: slice %u: depth and base_color must not be null", who, i);
        MIFX_CHECK(to_img_wh(s.depth, MIFX_FORMAT_F32, w, h, "slice depth", im));
        o.depth = im.p; o.pitchDepth = im.pitch;
        MIFX_CHECK(to_img_wh(s.base_color, MIFX_FORMAT_F32X4, w, h, "slice base_color", im));
        o.base = im.p; o.pitchBase = im.pitch;
        if (!targets) continue;
        MIFX_REQUIRE(s.material != nullptr && s.radiance != nullptr && s.specular_ibl != nullptr, "%s: slice %u: material, radiance and specular_ibl must not be null", who, i);
        MIFX_CHECK(to_img_wh(s.material, MIFX_FORMAT_F32X4, w, h, "slice material", im));
        o.material = im.p; o.pitchMaterial = im.pitch;
        MIFX_CHECK(to_img_wh(s.radiance, MIFX_FORMAT_F32X4, w, h, "slice radiance", im));
        o.radiance = im.p; o.pitchRadiance = im.pitch;
        MIFX_CHECK(to_img_wh(s.specular_ibl, MIFX_FORMAT_F32X4, w, h, "slice specular_ibl", im));
        o.ibl = im.p; o.pitchIbl = im.pitch;
        if (s.color_alpha)
        {
            MIFX_CHECK(to_img_wh(s.color_alpha, MIFX_FORMAT_F32, w, h, "slice color_alpha", im));
            o.alpha = im.p; o.pitchAlpha = im.pitch;
        }
    }
    f.tab.count = int(count);
    if (targets)
    {
        MIFX_REQUIRE(targets->color != nullptr && targets->base_color != nullptr && targets->material != nullptr && targets->ibl != nullptr, "%s: a target is null", who);
        MIFX_CHECK(to_img_wh(targets->color, MIFX_FORMAT_F32X4, w, h, "target color", f.targets.color));
        MIFX_CHECK(to_img_wh(targets->base_color, MIFX_FORMAT_F32X4, w, h, "target base_color", f.targets.base));
        MIFX_CHECK(to_img_wh(targets->material, MIFX_FORMAT_F32X4, w, h, "target material", f.targets.material));
        MIFX_CHECK(to_img_wh(targets->ibl, MIFX_FORMAT_F32X4, w, h, "target ibl", f.targets.ibl));
    }
    return MIFX_OK;
}

OitK make_oitk(const mifx_oit* o, const OitFrameK& f)
{
    OitK k{};
    k.layers = static_cast<unsigned char*>(o->layers);
    k.tail = static_cast<unsigned char*>(o->tail.data);
    k.opaque = f.opaque.p; k.opaquePitch = f.opaque.pitch;
    k.w = int(o->w); k.h = int(o->h); k.K = int(o->K); k.tailPitch = int(o->tail.pitch);
    k.cam = f.cam;
    return k;
}
mifx_status run_clear(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_clear_kernel");
    return launch_oit_clear(o->ctx->stream, make_oitk(o, f));
}
mifx_status run_update(mifx_oit* o, const OitFrameK& f, int slice)
{
    MifxKernelTimer timer(o->ctx, "oit_update_kernel");
    return launch_oit_update(o->ctx->stream, make_oitk(o, f), f.tab.s[slice]);
}
mifx_status run_attenuate(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_attenuate_kernel");
    return launch_oit_attenuate(o->ctx->stream, make_oitk(o, f), f.targets);
}
mifx_status run_blend(mifx_oit* o, const OitFrameK& f, int slice)
{
    MifxKernelTimer timer(o->ctx, "oit_blend_kernel");
    return launch_oit_blend(o->ctx->stream, make_oitk(o, f), f.tab.s[slice], f.targets);
}
mifx_status run_build(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_build_kernel");
    return launch_oit_build(o->ctx->stream, make_oitk(o, f), f.tab);
}
mifx_status run_resolve(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_resolve_kernel");
    return launch_oit_resolve(o->ctx->stream, make_oitk(o, f), f.tab, f.targets);
}
// mifx_oit_shade_blend and its check entry: the argument checks of frame_check (opaque depth, camera, targets; the slice's depth and base colour are the G-buffer's,
// checked with it) and of the layered shade (launch_oit_shade_blend: G-buffer, layers, lights, shadows, IBL), every plane of w x h; `o` == nullptr: the checks alone
mifx_status shade_blend(mifx_oit* o, uint32_t w, uint32_t h, uint32_t postfx_flags, const mifx_transparent_slice* slice, const mifx_image2d* opaque_depth,
                        const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* attribs, const mifx_ibl* ibl, const mifx_pbr_shadows* shadows, const mifx_oit_targets* targets,
                        const char* who)
{
    MIFX_REQUIRE(slice != nullptr && camera != nullptr && attribs != nullptr && ibl != nullptr && targets != nullptr, "%s: null argument", who);
#ifdef MIFX_STORAGE_H4
    (void)o; (void)w; (void)h; (void)postfx_flags; (void)opaque_depth; (void)shadows;
    ::mifx::set_error("%s: the fused shade-and-blend is not part of the native-storage build yet", who);
    return MIFX_ERR_NOT_IMPLEMENTED;
#else
    OitFrameK f;
    MIFX_CHECK(frame_check(w, h, nullptr, 0u, opaque_depth, camera, targets, who, f));
    const bool shadeReversed = (postfx_flags & MIFX_POSTFX_FEATURE_FLAG_REVERSED_DEPTH) != 0;
    MIFX_REQUIRE((f.cam.reversed != 0) == shadeReversed,
                 "%s: reversed depth disagrees: the camera says %s (fNearPlaneDepth %g, fFarPlaneDepth %g: what the OIT reads), the context's MIFX_POSTFX_FEATURE_FLAG_REVERSED_DEPTH "
                 "says %s (what the shade reads)",
                 who, f.cam.reversed ? "reversed" : "not reversed", double(camera->fNearPlaneDepth), double(camera->fFarPlaneDepth), shadeReversed ? "reversed" : "not reversed");
    if (o == nullptr)
    {
        OitK k{};
        k.w = int(w); k.h = int(h); k.cam = f.cam;
        IblApronCache none;
        return launch_oit_shade_blend(nullptr, none, k, f.targets, &slice->gbuffer, slice->layers, slice->color_alpha, *camera, *attribs, ibl, shadeReversed, shadows, true);
    }
    MIFX_HIP_CHECK(hipSetDevice(o->ctx->device));
    MifxKernelTimer timer(o->ctx, "oit_shade_blend_kernel"); // (includes the two cube-apron launches of the call, where the maps are not declared static)
    return launch_oit_shade_blend(o->ctx->stream, o->ctx->ibl_apron, make_oitk(o, f), f.targets, &slice->gbuffer, slice->layers, slice->color_alpha, *camera, *attribs, ibl, shadeReversed,
                                shadows, false);
#endif
}
} // namespace

extern "C" {

mifx_status mifx_oit_create_check(uint32_t width, uint32_t height, uint32_t layer_count) { return create_check(width, height, layer_count, "mifx_oit_create_check"); }

mifx_status mifx_oit_frame_check(uint32_t width, uint32_t height, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                                 const mifx_oit_targets* targets)
{
    OitFrameK f;
    MIFX_CHECK(create_check(width, height, 1u, "mifx_oit_frame_check"));
    return frame_check(width, height, slices, count, opaque_depth, camera, targets, "mifx_oit_frame_check", f);
}

int32_t mifx_oit_set_fusion(int32_t enable)
{
    const int32_t prev = g_oit_fusion ? 1 : 0;
    g_oit_fusion       = enable != 0;
    return prev;
}

// PBR_Renderer::CreateOITResources
mifx_status mifx_oit_create(mifx_postfx* ctx, uint32_t width, uint32_t height, uint32_t layer_count, mifx_oit** out)
{
    const char* who = "mifx_oit_create";
    MIFX_REQUIRE(ctx != nullptr && out != nullptr, "%s: null argument", who);
    MIFX_CHECK(create_check(width, height, layer_count, who));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    mifx_oit* o = new mifx_oit();
    o->ctx = ctx; o->w = width; o->h = height; o->K = layer_count;
    mifx_status st = o->tail.alloc(width, height, MIFX_FORMAT_F32X2);
    if (st >= 0 && hipMalloc(&o->layers, size_t(width) * height * layer_count * 4u) != hipSuccess)
    {
        set_error("%s: hipMalloc of %zu bytes for the layers failed", who, size_t(width) * height * layer_count * 4u);
        o->layers = nullptr;
        st        = MIFX_ERR_HIP;
    }
    if (st < 0)
    {
        delete o;
        return st;
    }
    *out = o;
    return MIFX_OK;
}

void mifx_oit_destroy(mifx_oit* oit) { delete oit; }

mifx_status mifx_oit_get_layers(mifx_oit* oit, void** out_data, uint64_t* out_words)
{
    MIFX_REQUIRE(oit != nullptr && out_data != nullptr && out_words != nullptr, "mifx_oit_get_layers: null argument");
    *out_data  = oit->layers;
    *out_words = uint64_t(oit->w) * oit->h * oit->K;
    return MIFX_OK;
}

mifx_status mifx_oit_get_tail(mifx_oit* oit, mifx_image2d* out)
{
    MIFX_REQUIRE(oit != nullptr && out != nullptr, "mifx_oit_get_tail: null argument");
    *out = oit->tail.desc();
    return MIFX_OK;
}

#define MIFX_OIT_RUN(...)                          \
    MIFX_HIP_CHECK(hipSetDevice(oit->ctx->device)); \
    __VA_ARGS__                                    \
    return MIFX_OK

// ClearOITLayers.csh, and the tail's clear value of HnBeginOITPassTask.cpp:139-144
mifx_status mifx_oit_clear_layers(mifx_oit* oit)
{
    const char* who = "mifx_oit_clear_layers";
    MIFX_REQUIRE(oit != nullptr, "%s: null object", who);
    OitFrameK f{};
    MIFX_OIT_RUN(MIFX_CHECK(run_clear(oit, f)););
}

// UpdateOITLayers.psh:54-109 with BS_UpdateOITTail (PBR_Renderer.cpp:1849-1865)
mifx_status mifx_oit_update_layers(mifx_oit* oit, const mifx_oit_slice* slice, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera)
{
    const char* who = "mifx_oit_update_layers";
    MIFX_REQUIRE(oit != nullptr && slice != nullptr && camera != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slice, 1u, opaque_depth, camera, nullptr, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_update(oit, f, 0)););
}

// ApplyOITAttenuation.psh with BS_OITAttenuation (PBR_Renderer.cpp:2309-2324)
mifx_status mifx_oit_apply_attenuation(mifx_oit* oit, const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_apply_attenuation";
    MIFX_REQUIRE(oit != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, nullptr, 0u, nullptr, nullptr, targets, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_attenuate(oit, f)););
}

// one transparent draw: RenderPBR.psh:388-418, :544-559, :632, USD_Renderer.cpp:122-167, the blend state of PBR_Renderer.cpp:2096-2127
mifx_status mifx_oit_blend(mifx_oit* oit, const mifx_oit_slice* slice, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera, const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_blend";
    MIFX_REQUIRE(oit != nullptr && slice != nullptr && camera != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slice, 1u, opaque_depth, camera, targets, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_blend(oit, f, 0)););
}

// one transparent draw, shaded and blended: the layered shade's body and the colour pass above in one launch (mifx_oit_shade.h)
mifx_status mifx_oit_shade_blend(mifx_oit* oit, const mifx_transparent_slice* slice, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                                 const mifx_pbr_shade_attribs* attribs, const mifx_ibl* ibl, const mifx_pbr_shadows* shadows, const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_shade_blend";
    MIFX_REQUIRE(oit != nullptr, "%s: null object", who);
    return shade_blend(oit, oit->w, oit->h, oit->ctx->flags, slice, opaque_depth, camera, attribs, ibl, shadows, targets, who);
}

mifx_status mifx_oit_shade_blend_check(uint32_t width, uint32_t height, uint32_t postfx_feature_flags, const mifx_transparent_slice* slice, const mifx_image2d* opaque_depth,
                                       const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* attribs, const mifx_ibl* ibl, const mifx_pbr_shadows* shadows,
                                       const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_shade_blend_check";
    MIFX_CHECK(create_check(width, height, 1u, who));
    return shade_blend(nullptr, width, height, postfx_feature_flags, slice, opaque_depth, camera, attribs, ibl, shadows, targets, who);
}

// clear_layers, then update_layers of every slice: one launch where a fused kernel exists for the layer count and the fusion is on
mifx_status mifx_oit_build_layers(mifx_oit* oit, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera)
{
    const char* who = "mifx_oit_build_layers";
    MIFX_REQUIRE(oit != nullptr, "%s: null object", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slices, count, opaque_depth, camera, nullptr, who, f));
    MIFX_OIT_RUN(
        if (g_oit_fusion && oit_has_fused_kernel(oit->K)) MIFX_CHECK(run_build(oit, f));
        else
        {
            MIFX_CHECK(run_clear(oit, f));
            for (uint32_t i = 0; i < count; ++i) MIFX_CHECK(run_update(oit, f, int(i)));
        });
}

// apply_attenuation, then blend of every slice
mifx_status mifx_oit_resolve(mifx_oit* oit, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                             const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_resolve";
    MIFX_REQUIRE(oit != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slices, count, opaque_depth, camera, targets, who, f));
    MIFX_OIT_RUN(
        if (g_oit_fusion && oit_has_fused_kernel(oit->K)) MIFX_CHECK(run_resolve(oit, f));
        else
        {
            MIFX_CHECK(run_attenuate(oit, f));
            for (uint32_t i = 0; i < count; ++i) MIFX_CHECK(run_blend(oit, f, int(i)));
        });
}

} // extern "C"
