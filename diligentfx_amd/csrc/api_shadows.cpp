// api_shadows.cpp -- C ABI of the cascaded shadow maps (include/mifx.h "cascaded shadow maps"): ShadowMapManager::ConvertToFilterable and the per-pixel look-up
// FilterShadowMap / SampleFilterableShadowMap.  The kernels and their launchers are in shadows.hip (mifx_shadows_host.h).
#include "mifx_objects.h"
#include "mifx_shadows_host.h"

using namespace mifx;

// The fused conversion kernel is built and tested (bit-identical), but no same-box A/B against the two launches has been measured yet: until one says it is faster,
// the two launches are the default (mifx_shadow_set_conversion_fusion, tools/shadows_bench.py).
static bool g_fuse_conversion = false;

static_assert(sizeof(mifx_cascade_attribs) == 64 && sizeof(mifx_shadow_map_attribs) == 1200, "CascadeAttribs / ShadowMapAttribs are byte-identical to the reference's");

static mifx_status to_shadow_arr(const mifx_shadow_map_array* m, const char* who, ShadowArrK& out)
{
    MIFX_REQUIRE(m->data != nullptr && m->width > 0 && m->height > 0 && m->slices > 0, "%s: shadow_map: empty array", who);
    MIFX_REQUIRE(m->width <= 16384u && m->height <= 16384u && m->slices <= 0x7FFFFFFFu, "%s: shadow_map: %ux%u is larger than 16384", who, m->width, m->height);
    MIFX_REQUIRE(m->pitch_bytes >= m->width * 4u && m->pitch_bytes <= 0x7FFFFFFFu && m->pitch_bytes % 4u == 0 && reinterpret_cast<uintptr_t>(m->data) % 4u == 0,
                 "%s: shadow_map: bad pitch %u / alignment for width %u", who, m->pitch_bytes, m->width);
    MIFX_REQUIRE(m->slice_pitch_bytes >= uint64_t(m->pitch_bytes) * m->height && m->slice_pitch_bytes % 4u == 0, "%s: shadow_map: bad slice pitch %llu", who,
                 static_cast<unsigned long long>(m->slice_pitch_bytes));
    out = ShadowArrK{static_cast<const unsigned char*>(m->data), int(m->width), int(m->height), int(m->slices), int(m->pitch_bytes), m->slice_pitch_bytes};
    return MIFX_OK;
}

// The formats of ShadowMapManager.cpp:98-102 per mode: the 32-bit one, or the 16-bit one that Is32BitFilterableFmt == false selects.  `texel` is the texel size of
// the format given.
static mifx_status to_filterable_arr(const mifx_filterable_shadow_map* m, const mifx_shadow_map_attribs* attribs, uint32_t mode, const char* who, FilterableArrK& out)
{
    const uint32_t fmt32 = mode == MIFX_SHADOW_MODE_EVSM4 ? MIFX_FORMAT_F32X4 : MIFX_FORMAT_F32X2;
    const uint32_t fmt16 = mode == MIFX_SHADOW_MODE_EVSM4 ? MIFX_FORMAT_F16X4 : mode == MIFX_SHADOW_MODE_EVSM2 ? MIFX_FORMAT_F16X2 : MIFX_FORMAT_U16X2;
    const int      ch    = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    MIFX_REQUIRE(m->data != nullptr && m->width > 0 && m->height > 0 && m->slices > 0, "%s: filterable map: empty array", who);
    MIFX_REQUIRE(m->format == fmt32 || m->format == fmt16, "%s: filterable map: shadow mode %u needs %s texels (or the 16-bit %s), got format %u", who, mode,
                 ch == 4 ? "MIFX_FORMAT_F32X4" : "MIFX_FORMAT_F32X2", ch == 4 ? "MIFX_FORMAT_F16X4" : mode == MIFX_SHADOW_MODE_EVSM2 ? "MIFX_FORMAT_F16X2" : "MIFX_FORMAT_U16X2", m->format);
    const bool narrow = m->format == fmt16;
    // exp(40 d) is not a binary16 value: a 16-bit EVSM map goes with the exponents clamped to 5.54 (GetEVSMExponents, Shadows.fxh:280-285; ShadowMapManager.cpp:157)
    MIFX_REQUIRE(!(narrow && mode != MIFX_SHADOW_MODE_VSM && attribs->bIs32BitEVSM != 0), "%s: filterable map: a 16-bit EVSM format (%u) needs bIs32BitEVSM == 0", who, m->format);
    const uint32_t texel = shadow_texel_bytes(narrow ? fmt16 : 0u, ch);
    MIFX_REQUIRE(m->width <= 16384u && m->height <= 16384u && m->slices <= 0x7FFFFFFFu, "%s: filterable map: %ux%u is larger than 16384", who, m->width, m->height);
    MIFX_REQUIRE(m->pitch_bytes >= m->width * texel && m->pitch_bytes <= 0x7FFFFFFFu && m->pitch_bytes % texel == 0 && reinterpret_cast<uintptr_t>(m->data) % texel == 0,
                 "%s: filterable map: bad pitch %u / alignment for width %u", who, m->pitch_bytes, m->width);
    MIFX_REQUIRE(m->slice_pitch_bytes >= uint64_t(m->pitch_bytes) * m->height && m->slice_pitch_bytes % texel == 0, "%s: filterable map: bad slice pitch %llu", who,
                 static_cast<unsigned long long>(m->slice_pitch_bytes));
    out = FilterableArrK{static_cast<unsigned char*>(m->data), int(m->width), int(m->height), int(m->slices), int(m->pitch_bytes), m->slice_pitch_bytes, narrow ? fmt16 : 0u};
    return MIFX_OK;
}

// every argument check of mifx_shadow_convert_to_filterable; nothing is dereferenced but the descriptors and the attribs
static mifx_status convert_check(const mifx_shadow_map_array* shadow_map, const mifx_shadow_map_attribs* attribs, uint32_t mode, const mifx_filterable_shadow_map* out, const char* who,
                                 ShadowArrK& src, FilterableArrK& dst, ShadowConvK& k)
{
    MIFX_REQUIRE(shadow_map != nullptr && attribs != nullptr && out != nullptr, "%s: null argument", who);
    MIFX_REQUIRE(mode >= MIFX_SHADOW_MODE_VSM && mode <= MIFX_SHADOW_MODE_EVSM4, "%s: shadow mode %u is not VSM (2), EVSM2 (3) or EVSM4 (4)", who, mode);
    MIFX_REQUIRE(attribs->iNumCascades >= 1 && attribs->iNumCascades <= MIFX_MAX_CASCADES, "%s: iNumCascades %d is outside 1 .. %d", who, attribs->iNumCascades, MIFX_MAX_CASCADES);
    MIFX_REQUIRE(int64_t(shadow_map->slices) == int64_t(attribs->iNumCascades), "%s: the shadow map has %u slices, iNumCascades is %d (inconsistent number of cascades)", who,
                 shadow_map->slices, attribs->iNumCascades);
    MIFX_CHECK(to_shadow_arr(shadow_map, who, src));
    MIFX_CHECK(to_filterable_arr(out, attribs, mode, who, dst));
    MIFX_REQUIRE(dst.w == src.w && dst.h == src.h && dst.slices == src.slices, "%s: the filterable map is %dx%dx%d, the shadow map %dx%dx%d", who, dst.w, dst.h, dst.slices, src.w, src.h,
                 src.slices);
    k = make_shadowconvk(*attribs, src.w, src.h);
    // A tap count is a loop count on the device.  Every finite radius up to MIFX_SHADOW_MAX_FILTER_RADIUS texels is taken, also one wider than the slice (the taps beyond
    // it read 0 and count in the total weight, as in the reference); one that is not a number, or beyond that, is refused.
    for (int i = 0; i < src.slices; ++i)
        MIFX_REQUIRE(std::isfinite(k.rH[i]) && std::isfinite(k.rV[i]) && k.rH[i] <= float(MIFX_SHADOW_MAX_FILTER_RADIUS) && k.rV[i] <= float(MIFX_SHADOW_MAX_FILTER_RADIUS),
                     "%s: cascade %d: filter radii %g x %g texels are not finite or exceed MIFX_SHADOW_MAX_FILTER_RADIUS (%d)", who, i, double(k.rH[i]), double(k.rV[i]),
                     MIFX_SHADOW_MAX_FILTER_RADIUS);
    return MIFX_OK;
}

// every argument check of mifx_shadow_map_filter
static mifx_status filter_check(const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_shadow_map_attribs* attribs, const mifx_shadow_filter_params* params,
                                const mifx_shadow_map_array* shadow_map, const mifx_filterable_shadow_map* filterable_map, const mifx_image2d* out_light_amount,
                                const mifx_image2d* out_cascade, const char* who, ShadowArrK& map, FilterableArrK& filterable, Img& d, Img& light, Img& cascade)
{
    MIFX_REQUIRE(depth != nullptr && camera != nullptr && attribs != nullptr && params != nullptr && out_light_amount != nullptr, "%s: null argument", who);
    const uint32_t mode = params->shadow_mode;
    MIFX_REQUIRE(mode >= MIFX_SHADOW_MODE_PCF && mode <= MIFX_SHADOW_MODE_EVSM4, "%s: shadow mode %u is outside 1 .. 4", who, mode);
    MIFX_REQUIRE(params->filter_across_cascades <= 1u && params->best_cascade_search <= 1u && params->reserved == 0u, "%s: the switches are 0 or 1, reserved is 0", who);
    MIFX_REQUIRE(attribs->iNumCascades >= 1 && attribs->iNumCascades <= MIFX_MAX_CASCADES, "%s: iNumCascades %d is outside 1 .. %d", who, attribs->iNumCascades, MIFX_MAX_CASCADES);
    map = ShadowArrK{};
    filterable = FilterableArrK{};
    if (mode == MIFX_SHADOW_MODE_PCF)
    {
        MIFX_REQUIRE(shadow_map != nullptr, "%s: SHADOW_MODE_PCF reads the shadow map, which is NULL", who);
        const int fs = attribs->iFixedFilterSize;
        MIFX_REQUIRE(fs <= 0 || fs == 2 || fs == 3 || fs == 5 || fs == 7, "%s: iFixedFilterSize %d: PCF_FILTER_SIZE is 2, 3, 5 or 7 (<= 0: the varying filter)", who, fs);
        MIFX_CHECK(to_shadow_arr(shadow_map, who, map));
        MIFX_REQUIRE(int64_t(map.slices) >= int64_t(attribs->iNumCascades), "%s: the shadow map has %d slices, iNumCascades is %d", who, map.slices, attribs->iNumCascades);
        // (the varying filter loops over the texels between bounds clamped to f4ShadowMapDim.xy: a loop count on the device)
        MIFX_REQUIRE(attribs->f4ShadowMapDim[0] == float(map.w) && attribs->f4ShadowMapDim[1] == float(map.h), "%s: f4ShadowMapDim.xy is %g x %g, the shadow map %dx%d", who,
                     double(attribs->f4ShadowMapDim[0]), double(attribs->f4ShadowMapDim[1]), map.w, map.h);
        if (fs <= 0)
            for (int i = 0; i < attribs->iNumCascades; ++i)
            {
                // FilterShadowCascade's f2FilterSize times the map size: the varying filter's footprint in texels, 2 x 2 of them per loop iteration
                const float fx = std::fabs(attribs->fFilterWorldSize * attribs->Cascades[i].f4LightSpaceScale[0] * 0.5f) * float(map.w);
                const float fy = std::fabs(attribs->fFilterWorldSize * attribs->Cascades[i].f4LightSpaceScale[1] * 0.5f) * float(map.h);
                MIFX_REQUIRE(fx <= float(MIFX_SHADOW_MAX_VARYING_PCF_TEXELS) && fy <= float(MIFX_SHADOW_MAX_VARYING_PCF_TEXELS),
                             "%s: cascade %d: the varying PCF filter covers %g x %g texels, not finite or more than MIFX_SHADOW_MAX_VARYING_PCF_TEXELS (%d)", who, i, double(fx), double(fy),
                             MIFX_SHADOW_MAX_VARYING_PCF_TEXELS);
            }
    }
    else
    {
        MIFX_REQUIRE(filterable_map != nullptr, "%s: shadow mode %u reads the filterable map, which is NULL", who, mode);
        MIFX_CHECK(to_filterable_arr(filterable_map, attribs, mode, who, filterable));
        MIFX_REQUIRE(int64_t(filterable.slices) >= int64_t(attribs->iNumCascades), "%s: the filterable map has %d slices, iNumCascades is %d", who, filterable.slices,
                     attribs->iNumCascades);
    }
    cascade = Img{};
    MIFX_CHECK(to_img(depth, MIFX_FORMAT_F32, "depth", d));
    MIFX_CHECK(to_img_wh(out_light_amount, MIFX_FORMAT_F32, depth->width, depth->height, "out_light_amount", light));
    if (out_cascade) MIFX_CHECK(to_img_wh(out_cascade, MIFX_FORMAT_F32X2, depth->width, depth->height, "out_cascade", cascade));
    return MIFX_OK;
}

extern "C" {

// BasicStructures.fxh:47-65: the DEFAULT_VALUEs
mifx_status mifx_shadow_map_default_attribs(mifx_shadow_map_attribs* out)
{
    MIFX_REQUIRE(out != nullptr, "mifx_shadow_map_default_attribs: null argument");
    mifx_shadow_map_attribs a{};
    a.fReceiverPlaneDepthBiasClamp = 10.0f;
    a.fFixedDepthBias              = 1e-5f;
    a.fCascadeTransitionRegion     = 0.1f;
    a.iMaxAnisotropy               = 4;
    a.fVSMBias                     = 1e-4f;
    a.fVSMLightBleedingReduction   = 0.0f;
    a.fEVSMPositiveExponent        = 40.0f;
    a.fEVSMNegativeExponent        = 5.0f;
    a.bIs32BitEVSM                 = 1;
    a.iFixedFilterSize             = 3;
    a.fFilterWorldSize             = 0.0f;
    *out = a;
    return MIFX_OK;
}

int32_t mifx_shadow_set_conversion_fusion(int32_t enable)
{
    const int32_t prev = g_fuse_conversion ? 1 : 0;
    g_fuse_conversion  = enable != 0;
    return prev;
}

mifx_status mifx_shadow_convert_check(const mifx_shadow_map_array* shadow_map, const mifx_shadow_map_attribs* attribs, uint32_t mode, const mifx_filterable_shadow_map* out)
{
    ShadowArrK     src;
    FilterableArrK dst;
    ShadowConvK    k;
    return convert_check(shadow_map, attribs, mode, out, "mifx_shadow_convert_check", src, dst, k);
}

// ShadowMapManager::ConvertToFilterable (ShadowMapManager.cpp:533-600)
mifx_status mifx_shadow_convert_to_filterable(mifx_postfx* ctx, const mifx_shadow_map_array* shadow_map, const mifx_shadow_map_attribs* attribs, uint32_t mode,
                                              const mifx_filterable_shadow_map* out)
{
    const char* who = "mifx_shadow_convert_to_filterable";
    MIFX_REQUIRE(ctx != nullptr, "%s: null context", who);
    ShadowArrK     src;
    FilterableArrK dst;
    ShadowConvK    k;
    MIFX_CHECK(convert_check(shadow_map, attribs, mode, out, who, src, dst, k));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    // which kernels run is decided here, so that the kernel-timing names say it (mifx_postfx_set_kernel_timing)
    const bool skipBlur = attribs->iFixedFilterSize == 2;
    bool       fits     = true;
    for (int i = 0; i < src.slices; ++i) fits = fits && shadow_filter_range(k.rH[i]) <= kShadowFusedMaxRange && shadow_filter_range(k.rV[i]) <= kShadowFusedMaxRange;
    const bool fused = !skipBlur && g_fuse_conversion && fits;
    MifxKernelTimer timer(ctx, skipBlur ? "shadow_convert_horz_kernel" : fused ? "shadow_convert_fused_kernel" : "shadow_convert_two_launch");
    return launch_shadow_convert(ctx->stream, ctx->shadow_scratch, src, dst, k, mode, skipBlur, fused);
}

mifx_status mifx_shadow_map_filter_check(const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_shadow_map_attribs* attribs, const mifx_shadow_filter_params* params,
                                         const mifx_shadow_map_array* shadow_map, const mifx_filterable_shadow_map* filterable_map, const mifx_image2d* out_light_amount,
                                         const mifx_image2d* out_cascade)
{
    ShadowArrK     map;
    FilterableArrK filterable;
    Img            d, light, cascade;
    return filter_check(depth, camera, attribs, params, shadow_map, filterable_map, out_light_amount, out_cascade, "mifx_shadow_map_filter_check", map, filterable, d, light, cascade);
}

// FilterShadowMap (Shadows.fxh:219-253) / SampleFilterableShadowMap (:350-384) per pixel
mifx_status mifx_shadow_map_filter(mifx_postfx* ctx, const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_shadow_map_attribs* attribs,
                                   const mifx_shadow_filter_params* params, const mifx_shadow_map_array* shadow_map, const mifx_filterable_shadow_map* filterable_map,
                                   const mifx_image2d* out_light_amount, const mifx_image2d* out_cascade)
{
    const char* who = "mifx_shadow_map_filter";
    MIFX_REQUIRE(ctx != nullptr, "%s: null context", who);
    ShadowArrK     map;
    FilterableArrK filterable;
    Img            d, light, cascade;
    MIFX_CHECK(filter_check(depth, camera, attribs, params, shadow_map, filterable_map, out_light_amount, out_cascade, who, map, filterable, d, light, cascade));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "shadow_filter_kernel");
    return launch_shadow_filter(ctx->stream, d, light, cascade, make_shadowlookupk(*camera, *attribs), map, filterable, params->shadow_mode, params->best_cascade_search != 0,
                                params->filter_across_cascades != 0);
}

} // extern "C"
