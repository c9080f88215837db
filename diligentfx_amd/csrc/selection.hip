// selection.hip -- HnProcessSelectionTask (Hydrogent/src/Tasks/HnProcessSelectionTask.cpp:302-369): the closest-selected-location plane by jump flooding.  The
// per-pixel bodies: mifx_selection.h; the effect object and the C entry points: api_selection.cpp.
//
// The reference draws the init pass and then one full-screen pass per step (m_NumJFIterations = 3 at the default MaximumDistance 4: ranges 4, 2, 1), each reading and
// writing an RG32_FLOAT target: ~60 B/px over four passes.  Here the trailing steps whose summed reach fits a 7-pixel halo run in ONE launch: a 32 x 16 tile loads the
// selection depth of its (32 + 14) x (16 + 14) neighbourhood once, computes the init on the fly into LDS and runs the steps there, each on the part of the neighbourhood
// the following steps still read, and stores only the final texels (4 B in, 8 B out per pixel).  Steps of larger ranges (max_distance > 4) run one launch each in front of it,
// over the whole frame.  Outside the frame a tap reads 0 (invalid) at every step, as a Load out of bounds does in the reference.
#include "mifx_selection_host.h"

namespace mifx
{
constexpr int kJfTileW = 32, kJfTileH = 16, kJfThreads = 256;

// The trailing K steps (ranges 1 << (K - 1), ..., 1) of the jump flood for a 32 x 16 tile of rows from `rowBegin` on.  FROM_DEPTH: `src` is the selection depth (F32) and
// the init pass is evaluated while loading; otherwise `src` is the plane of the step before (F32X2).
template <bool FROM_DEPTH, int K>
__global__ __launch_bounds__(kJfThreads) void jump_flood_kernel(Img src, float clearDepth, Img out, int rowBegin, int rowEnd)
{
    constexpr int HALO = (1 << K) - 1;
    constexpr int RW = kJfTileW + 2 * HALO, RH = kJfTileH + 2 * HALO;
    __shared__ v2 buf[2][RH * RW];
    const int W = out.w, H = out.h;
    const int ox = int(blockIdx.x) * kJfTileW - HALO, oy = rowBegin + int(blockIdx.y) * kJfTileH - HALO; // frame position of LDS texel (0, 0)
    const int t  = int(threadIdx.x);
    for (int i = t; i < RW * RH; i += kJfThreads)
    {
        const int gx = ox + i % RW, gy = oy + i / RW;
        v2 v{0.0f, 0.0f};
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = FROM_DEPTH ? jf_init(gx, gy, ld<float>(src, gx, gy), clearDepth, W, H) : ld<v2>(src, gx, gy);
        buf[0][i] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k)
    {
        const int range = 1 << (K - 1 - k);
        const int m     = range - 1; // what the later steps still read beyond the tile
        const v2* in    = buf[k & 1];
        auto fetch = [&](int tx, int ty) __attribute__((always_inline)) { return in[(ty - oy) * RW + (tx - ox)]; };
        if (k + 1 < K)
        {
            v2*       dst = buf[(k + 1) & 1];
            const int w = kJfTileW + 2 * m, h = kJfTileH + 2 * m;
            for (int i = t; i < w * h; i += kJfThreads)
            {
                const int lx = HALO - m + i % w, ly = HALO - m + i / w;
                const int gx = ox + lx, gy = oy + ly;
                v2 v{0.0f, 0.0f};
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = jf_step(gx, gy, range, W, H, fetch);
                dst[ly * RW + lx] = v;
            }
            __syncthreads();
        }
        else
        {
            for (int i = t; i < kJfTileW * kJfTileH; i += kJfThreads)
            {
                const int gx = ox + HALO + i % kJfTileW, gy = oy + HALO + i / kJfTileW;
                if (gx < W && gy < rowEnd) st<v2>(out, gx, gy, jf_step(gx, gy, range, W, H, fetch));
            }
        }
    }
}

// One step of the jump flood over the whole frame (the leading steps of a large max_distance), reading `src` in global memory.
template <bool FROM_DEPTH>
__global__ __launch_bounds__(256) void jump_flood_step_kernel(Img src, float clearDepth, int range, Img out)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    const int W = out.w, H = out.h;
    if (x >= W || y >= H) return;
    auto fetch = [&](int tx, int ty) __attribute__((always_inline)) {
        return FROM_DEPTH ? jf_init(tx, ty, ld<float>(src, tx, ty), clearDepth, W, H) : ld<v2>(src, tx, ty);
    };
    st<v2>(out, x, y, jf_step(x, y, range, W, H, fetch));
}

mifx_status launch_jump_flood(hipStream_t s, Img selectionDepth, float clearDepth, int iterations, Img tmp0, Img tmp1, Img out, int rowBegin, int rowEnd)
{
    MIFX_REQUIRE(iterations >= 1 && iterations <= 24, "jump flood: %d steps", iterations);
    rowBegin = rowBegin < 0 ? 0 : rowBegin;
    rowEnd   = rowEnd > out.h ? out.h : rowEnd;
    const int fused = iterations < kJfFused ? iterations : kJfFused;
    const int lead  = iterations - fused;
    Img  src  = selectionDepth;
    bool from = true;
    for (int i = 0; i < lead; ++i) // SampleRange 1 << (n - 1 - i), larger than the fused launch's halo
    {
        const Img dst = (i & 1) ? tmp1 : tmp0;
        const dim3 block(64, 4, 1), grid = grid2d(dst.w, dst.h, block);
        const int  range = 1 << (iterations - 1 - i);
        if (from) hipLaunchKernelGGL(jump_flood_step_kernel<true>, grid, block, 0, s, src, clearDepth, range, dst);
        else hipLaunchKernelGGL(jump_flood_step_kernel<false>, grid, block, 0, s, src, clearDepth, range, dst);
        src  = dst;
        from = false;
    }
    if (rowEnd > rowBegin)
    {
        const dim3 grid((out.w + kJfTileW - 1) / kJfTileW, (rowEnd - rowBegin + kJfTileH - 1) / kJfTileH, 1), block(kJfThreads, 1, 1);
        if (!from) hipLaunchKernelGGL((jump_flood_kernel<false, kJfFused>), grid, block, 0, s, src, clearDepth, out, rowBegin, rowEnd);
        else if (fused == 3) hipLaunchKernelGGL((jump_flood_kernel<true, 3>), grid, block, 0, s, src, clearDepth, out, rowBegin, rowEnd);
        else if (fused == 2) hipLaunchKernelGGL((jump_flood_kernel<true, 2>), grid, block, 0, s, src, clearDepth, out, rowBegin, rowEnd);
        else hipLaunchKernelGGL((jump_flood_kernel<true, 1>), grid, block, 0, s, src, clearDepth, out, rowBegin, rowEnd);
    }
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
} // namespace mifx
