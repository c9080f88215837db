// material.hip -- the material fetch (include/mifx.h "material fetch"): the kernel and its launcher (mifx_material_host.h).  The per-pixel body is mifx_material.h (the head
// of `main` of Shaders/PBR/private/RenderPBR.psh over interpolant planes, with the texture system written out); the argument checks, the tables and the two C entries
// are api_material.cpp.
//
// Shape.  One thread per pixel, blocks of 32 x 8: a wave is two rows of 32 pixels that start on an even row, so the four pixels of every 2x2 quad are lanes of one wave and
// the partners' interpolants (the body reads them itself: no cross-lane exchange, no LDS) come from lines the wave has touched already.  The kernel is a gather: up to 16
// maps a pixel, each 4 or 8 texels of 16 bytes (RGBA32_FLOAT) or 4 bytes (RGBA8_UNORM, one load a texel), addressed through the per-pixel material record.  Material
// records and texture descriptors are read from memory by index (they stay in the scalar / L1 caches: a frame has a handful): there is no private array indexed at
// run time, and the kernel uses no scratch (tests/test_kernel_resources.py).  The atlas permutation is a template parameter (USE_TEXTURE_ATLAS is a pipeline key in
// the reference too); the texture-coordinate transform, the colour conversion and the layer set are uniform run-time values.
#include "mifx_material_host.h"

namespace mifx
{
#ifndef MIFX_STORAGE_H4 // (the native-storage build has no material fetch yet: api_material.cpp)
template <bool ATLAS> __global__ __launch_bounds__(256) void material_fetch_kernel(MaterialFetchK k, CamK cam)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.depth.w || y >= k.depth.h) return;
    material_fetch_store<ATLAS>(x, y, k, cam);
}

mifx_status launch_material_fetch(hipStream_t s, const MaterialFetchK& k, const CamK& cam)
{
    const dim3 block(32, 8, 1), grid((uint32_t(k.depth.w) + 31u) / 32u, (uint32_t(k.depth.h) + 7u) / 8u, 1);
    if (k.flags & MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS) hipLaunchKernelGGL(material_fetch_kernel<true>, grid, block, 0, s, k, cam);
    else hipLaunchKernelGGL(material_fetch_kernel<false>, grid, block, 0, s, k, cam);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
#endif
} // namespace mifx
