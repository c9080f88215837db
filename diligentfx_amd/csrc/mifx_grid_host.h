// mifx_grid_host.h -- host side of the coordinate grid (grid.hip, api_grid.cpp).
// The two launchers are defined beside their kernels in grid.hip and called by api_grid.cpp; the chain (api_chain.cpp) goes through copy_frame_grid_run.
#pragma once
#include "mifx_host.h"
#include "mifx_coordinate_grid.h"

struct mifx_postfx;
struct mifx_autoexposure;

namespace mifx
{
// coordinate_grid_kernel.  `rows`: the depth plane, its row window = the rows written.  target.p / raw.p may be null (not both); raw: true fp32 float4 texels in every build.
mifx_status launch_coordinate_grid(hipStream_t s, Img rows, Img target, Img raw, const GridCamK& cam, const mifx_coordinate_grid_attribs& a, uint32_t flags);
// copy_frame_grid_kernel; aveLum != null: the tone map's average from the device (the auto-exposure object's value), as launch_tonemap
mifx_status launch_copy_frame_grid(hipStream_t s, Img in, bool packedIn, Img depth, Img out, const mifx_tone_mapping_attribs& attr, float ave_log_lum, uint32_t tonemap_flags,
                                   const float* aveLum, const GridCamK& cam, const mifx_coordinate_grid_attribs& a, uint32_t grid_flags);

// mifx_copy_frame_render with the grid on; ae != null: fAveLogLum from the auto-exposure object (the chain's frame with both)
mifx_status copy_frame_grid_run(mifx_postfx* ctx, const mifx_image2d* color, const mifx_image2d* depth, const mifx_camera_attribs* camera, const mifx_tone_mapping_attribs* tm,
                                float ave_log_lum, uint32_t tonemap_flags, mifx_autoexposure* ae, const mifx_coordinate_grid_attribs& grid, uint32_t grid_flags, const mifx_image2d* out,
                                const char* who);
} // namespace mifx
