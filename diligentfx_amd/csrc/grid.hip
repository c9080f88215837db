// grid.hip -- the coordinate grid and axes: the stand-alone renderer (Components/src/CoordinateGridRenderer.cpp:221-284, Shaders/Common/private/CoordinateGridPS.psh:24-38)
// and the frame's copy-frame pass with the grid (Hydrogent/shaders/HnCopyFrame.psh:27-63).  The per-pixel body is mifx_coordinate_grid.h.  Streaming passes like
// tonemap.hip: one texel per lane, 64x4 blocks, the colour read once, the final image stored non-temporally.  The plane / axis flags are kernel arguments tested in
// wave-uniform branches (64 instantiations per tone-mapping mode otherwise); each plane's hit position and alpha live only inside its branch, so nothing is indexed
// dynamically and nothing spills (tests/test_kernel_resources.py).
#include "mifx_grid_host.h"
#include "mifx_tonemap.h"

namespace mifx
{
// depth: its row window is the launch's.  target / raw: null pointer = not written.
__global__ __launch_bounds__(256) void coordinate_grid_kernel(Img depth, Img target, Img raw, GridCamK cam, mifx_coordinate_grid_attribs a, uint32_t flags)
{
    int x, y;
    if (!pixel_xy(depth, x, y)) return;
    v4 g{0.0f, 0.0f, 0.0f, 0.0f};
    if (flags & (kGridPlaneFlags | kGridAxisFlags))
    {
        const float d = ld<float>(depth, x, y); // SampleDepth (CoordinateGridPS.psh:26): MinDepth = MaxDepth = the pixel's depth
        g = coordinate_grid_at(x, y, depth.w, depth.h, cam, d, d, a, flags);
        if ((flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_CONVERT_TO_SRGB) && !(flags & MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD)) g = mk4(linear_to_srgb(xyz(g)), g.w);
    }
    if (raw.p) *(MIFX_GLOBAL mifx_f4*)(raw.p + size_t(y) * raw.pitch + size_t(x) * 16u) = mifx_f4{g.x, g.y, g.z, g.w};
    if (target.p)
    {
        const v4 dst = ld<v4>(target, x, y);
        st<v4>(target, x, y, mk4(grid_blend(xyz(dst), g), dst.w));
    }
}

template <int MODE> __global__ __launch_bounds__(256) void copy_frame_grid_kernel(Img in, Img depth, Img out, ToneMapK tm, const float* aveLum, int srgb, GridCamK cam,
                                                                                  mifx_coordinate_grid_attribs a, uint32_t flags)
{
    int x, y;
    if (!pixel_xy(out, x, y)) return;
    if (aveLum) tm.aveLogLum = fmaxf(0.05f, *aveLum); // GetAverageSceneLuminance of the auto-exposure plane, as tonemap_kernel
    const v4 c = ld_hdr_once(in, x, y, tm.packedIn);
    v3 t = tone_map<MODE>(xyz(c), tm);
    // the depth range of the 3x3 neighbourhood (HnCopyFrame.psh:41-51): Load is not clamped, a texel outside the frame reads 0
    float minDepth = 1.0f, maxDepth = 0.0f;
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j)
        {
            const float d = ld_zero_f_nb(depth, x + i, y + j);
            minDepth = fminf(minDepth, d);
            maxDepth = fmaxf(maxDepth, d);
        }
    const v4 g = coordinate_grid_at(x, y, out.w, out.h, cam, minDepth, maxDepth, a, flags);
    t = grid_lerp(t, g);
    if (srgb) t = linear_to_srgb(t);
    st_v4_late<1>(out, x, y, mk4(t, c.w));
}

mifx_status launch_coordinate_grid(hipStream_t s, Img rows, Img target, Img raw, const GridCamK& cam, const mifx_coordinate_grid_attribs& a, uint32_t flags)
{
    const dim3 block(64, 4, 1);
    hipLaunchKernelGGL(coordinate_grid_kernel, grid2d(rows, block), block, 0, s, rows, target, raw, cam, a, flags);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}

mifx_status launch_copy_frame_grid(hipStream_t s, Img in, bool packedIn, Img depth, Img out, const mifx_tone_mapping_attribs& attr, float ave_log_lum, uint32_t tonemap_flags,
                                   const float* aveLum, const GridCamK& cam, const mifx_coordinate_grid_attribs& a, uint32_t grid_flags)
{
    ToneMapK tm = make_tonemapk(attr, ave_log_lum);
    tm.packedIn = packedIn ? 1 : 0;
    const dim3 block(64, 4, 1);
    const dim3 grid = grid2d(out, block);
    const int  srgb = (tonemap_flags & MIFX_TONEMAP_FLAG_CONVERT_OUTPUT_TO_SRGB) != 0 ? 1 : 0;
#define MIFX_CF_LAUNCH(M) hipLaunchKernelGGL((copy_frame_grid_kernel<M>), grid, block, 0, s, in, depth, out, tm, aveLum, srgb, cam, a, grid_flags)
    MIFX_TONEMAP_DISPATCH(attr.iToneMappingMode, MIFX_CF_LAUNCH)
#undef MIFX_CF_LAUNCH
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
} // namespace mifx
