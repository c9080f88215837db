// api_grid.cpp -- C ABI of the coordinate grid and axes (include/mifx.h "coordinate grid and axes"): the stand-alone renderer (Components/CoordinateGridRenderer) and the
// copy-frame draw with the grid (Hydrogent/shaders/HnCopyFrame.psh).  The kernels and their launchers are in grid.hip (mifx_grid_host.h).
#include "mifx_objects.h"
#include "mifx_grid_host.h"

using namespace mifx;

static const uint32_t kGridKnownFlags = MIFX_COORDINATE_GRID_FEATURE_FLAG_CONVERT_TO_SRGB | kGridPlaneFlags | kGridAxisFlags;

mifx_status mifx::copy_frame_grid_run(mifx_postfx* ctx, const mifx_image2d* color, const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_tone_mapping_attribs* tm,
                                      float ave_log_lum, uint32_t tonemap_flags, mifx_autoexposure* ae, const mifx_coordinate_grid_attribs& grid, uint32_t grid_flags,
                                      const mifx_image2d* out, const char* who)
{
    MIFX_REQUIRE(ctx != nullptr && tm != nullptr && camera != nullptr && color != nullptr, "%s: null argument", who);
    MIFX_REQUIRE(tm->iToneMappingMode >= 0 && tm->iToneMappingMode <= MIFX_TONE_MAPPING_MODE_COMMERCE, "%s: unknown tone mapping mode %d", who, tm->iToneMappingMode);
    MIFX_REQUIRE((tonemap_flags & ~uint32_t(MIFX_TONEMAP_FLAG_CONVERT_OUTPUT_TO_SRGB)) == 0, "%s: unknown tone map flags 0x%x", who, tonemap_flags);
    MIFX_REQUIRE((grid_flags & ~kGridKnownFlags) == 0, "%s: unknown grid feature flags 0x%x", who, grid_flags);
    // (the average is written on the auto-exposure object's context stream and read here on ctx's, as for mifx_tonemap_execute_auto)
    MIFX_REQUIRE(ae == nullptr || ae->ctx == ctx || (ae->ctx->device == ctx->device && ae->ctx->stream == ctx->stream),
                 "%s: the auto-exposure object belongs to a context on another device / stream", who);
    Img  in, d, o;
    bool packed = false;
    MIFX_CHECK(to_img_hdr(color, "color", in, packed));
    MIFX_CHECK(to_img_wh(depth, MIFX_FORMAT_F32, color->width, color->height, "depth", d));
    MIFX_CHECK(to_img_wh(out, MIFX_FORMAT_F32X4, color->width, color->height, "out", o));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "copy_frame_grid_kernel");
    return launch_copy_frame_grid(ctx->stream, in, packed, d, win(o, ctx->needed_rows(o.h)), *tm, ae ? 1.0f : ave_log_lum, tonemap_flags,
                                  ae ? static_cast<const float*>(ae->average.data) : nullptr, make_gridcamk(*camera), grid, grid_flags & (kGridPlaneFlags | kGridAxisFlags));
}

extern "C" {

// CoordinateGridStructures.fxh:6-29: the DEFAULT_VALUEs
mifx_status mifx_coordinate_grid_default_attribs(mifx_coordinate_grid_attribs* out)
{
    MIFX_REQUIRE(out != nullptr, "mifx_coordinate_grid_default_attribs: null argument");
    static const mifx_coordinate_grid_attribs k = {{1.0f, 0.0f, 0.0f, 1.0f},    {0.0f, 1.0f, 0.0f, 1.0f},    {0.0f, 0.0f, 1.0f, 1.0f}, {0.40f, 0.15f, 0.15f, 1.0f},
                                                   {0.15f, 0.40f, 0.15f, 1.0f}, {0.15f, 0.15f, 0.40f, 1.0f}, 3.0f, 3.0f, 3.0f, 0.0f,
                                                   {0.4f, 0.4f, 0.4f, 1.0f},    {0.1f, 0.1f, 0.1f, 1.0f},    {1.0f, 1.0f, 1.0f, 0.0f}, {10.0f, 10.0f, 10.0f, 0.0f},
                                                   2.0f, 4.0f, 0.0001f, 0.0f};
    *out = k;
    return MIFX_OK;
}

// CoordinateGridRenderer::Render (CoordinateGridRenderer.cpp:221-284)
mifx_status mifx_coordinate_grid_render(mifx_postfx* ctx, const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_coordinate_grid_attribs* attribs, uint32_t feature_flags,
                                        const mifx_image2d* color_target, const mifx_image2d* out_grid)
{
    MIFX_REQUIRE(ctx != nullptr && depth != nullptr && camera != nullptr, "mifx_coordinate_grid_render: null argument");
    MIFX_REQUIRE(color_target != nullptr || out_grid != nullptr, "mifx_coordinate_grid_render: neither a colour target nor a raw output");
    MIFX_REQUIRE((feature_flags & ~(kGridKnownFlags | MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD)) == 0, "mifx_coordinate_grid_render: unknown feature flags 0x%x", feature_flags);
    const bool debug = (feature_flags & MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD) != 0;
    MIFX_REQUIRE(!debug || (color_target == nullptr && (feature_flags & kGridPlaneFlags) != 0 && attribs != nullptr),
                 "mifx_coordinate_grid_render: MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD needs a plane flag and writes the raw output only");
    if (attribs == nullptr) feature_flags = 0;
    Img d, target{}, raw{};
    MIFX_CHECK(to_img(depth, MIFX_FORMAT_F32, "depth", d));
    if (color_target) MIFX_CHECK(to_img_wh(color_target, MIFX_FORMAT_F32X4, depth->width, depth->height, "color_target", target));
    if (out_grid)
    {
        // (the shader's own result: fp32 texels also in the native-storage build, whose 4-channel planes are RGBA16_FLOAT)
        MIFX_REQUIRE(out_grid->data != nullptr && out_grid->format == MIFX_FORMAT_F32X4 && out_grid->width == depth->width && out_grid->height == depth->height,
                     "out_grid: a %ux%u MIFX_FORMAT_F32X4 image is needed", depth->width, depth->height);
        MIFX_REQUIRE(out_grid->pitch_bytes >= out_grid->width * 16u && out_grid->pitch_bytes % 16u == 0 && reinterpret_cast<uintptr_t>(out_grid->data) % 16u == 0 &&
                         uint64_t(out_grid->pitch_bytes) * out_grid->height <= 0xFFFFFFFFull,
                     "out_grid: bad pitch %u / alignment for width %u", out_grid->pitch_bytes, out_grid->width);
        raw = Img{static_cast<unsigned char*>(out_grid->data), int(out_grid->width), int(out_grid->height), int(out_grid->pitch_bytes), 0, 0};
    }
    const mifx_coordinate_grid_attribs none{};
    if ((feature_flags & (kGridPlaneFlags | kGridAxisFlags)) == 0)
    {
        feature_flags = 0; // alpha-0 texels: nothing to blend, the raw output cleared
        target        = Img{};
        if (raw.p == nullptr) return MIFX_OK;
    }
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "coordinate_grid_kernel");
    return launch_coordinate_grid(ctx->stream, win(d, ctx->needed_rows(d.h)), target, raw, make_gridcamk(*camera), attribs ? *attribs : none, feature_flags);
}

// the copy-frame draw of HnPostProcessTask.cpp:920-925 (HnCopyFrame.psh:27-63)
mifx_status mifx_copy_frame_render(mifx_postfx* ctx, const mifx_image2d* color, const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_tone_mapping_attribs* tone_mapping,
                                   float ave_log_lum, uint32_t tonemap_flags, const mifx_coordinate_grid_attribs* grid, uint32_t grid_feature_flags, const mifx_image2d* out)
{
    MIFX_REQUIRE((grid_feature_flags & ~kGridKnownFlags) == 0, "mifx_copy_frame_render: unknown grid feature flags 0x%x", grid_feature_flags);
    if (grid == nullptr || (grid_feature_flags & (kGridPlaneFlags | kGridAxisFlags)) == 0) return mifx_tonemap_execute(ctx, color, out, tone_mapping, ave_log_lum, tonemap_flags);
    return copy_frame_grid_run(ctx, color, depth, camera, tone_mapping, ave_log_lum, tonemap_flags, nullptr, *grid, grid_feature_flags, out, "mifx_copy_frame_render");
}

// HnPostProcessTaskParams::Grid / GridFeatureFlags (HnPostProcessTask.cpp:181, 397, 856)
mifx_status mifx_chain_set_coordinate_grid(mifx_chain* chain, const mifx_coordinate_grid_attribs* attribs, uint32_t grid_feature_flags)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_coordinate_grid: null chain");
    MIFX_REQUIRE((grid_feature_flags & ~kGridKnownFlags) == 0, "mifx_chain_set_coordinate_grid: unknown grid feature flags 0x%x", grid_feature_flags);
    if (attribs == nullptr || (grid_feature_flags & (kGridPlaneFlags | kGridAxisFlags)) == 0)
    {
        chain->has_grid = false;
        return MIFX_OK;
    }
    chain->grid_attribs = *attribs;
    chain->grid_flags   = grid_feature_flags;
    chain->has_grid     = true;
    return MIFX_OK;
}

} // extern "C"
