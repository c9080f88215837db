// selection.hip -- HnProcessSelectionTask (Hydrogent/src/Tasks/HnProcessSelectionTask.cpp:302-369): the closest-selected-location plane by jump flooding, and the
// C entry points of the selection outline (include/mifx.h: mifx_selection_*, mifx_composite_execute_selection) beside their kernels.  The per-pixel bodies:
// mifx_selection.h.
//
// The reference draws the init pass and then one full-screen pass per step (m_NumJFIterations = 3 at the default MaximumDistance 4: ranges 4, 2, 1), each reading and
// writing an RG32_FLOAT target: ~60 B/px over four passes.  Here the trailing steps whose summed reach fits a 7-pixel halo run in ONE launch: a 32 x 16 tile loads the
// selection depth of its (32 + 14) x (16 + 14) neighbourhood once, computes the init on the fly into LDS and runs the steps there, each on the part of the neighbourhood
// the following steps still read, and stores only the final texels (4 B in, 8 B out per pixel).  Steps of larger ranges (max_distance > 4) run one launch each in front of it,
// over the whole frame.  Outside the frame a tap reads 0 (invalid) at every step, as a Load out of bounds does in the reference.
#include "mifx_objects.h"
#include "mifx_selection_host.h"

struct mifx_selection // == HnProcessSelectionTask
{
    mifx_postfx* ctx = nullptr;
    mifx::Plane  out;    // closestSelectedLocationFinalTarget
    mifx::Plane  tmp[2]; // the leading steps' ping-pong planes (max_distance > 4)
};

namespace mifx
{
constexpr int kJfTileW = 32, kJfTileH = 16, kJfThreads = 256;
constexpr int kJfFused = 3; // steps of one launch: the reach 4 + 2 + 1 = 7 of the halo

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

mifx_status make_selectionk(const mifx_selection_composite_inputs& in, uint32_t W, uint32_t H, SelectionK& k)
{
    MIFX_REQUIRE(in.attribs != nullptr, "selection composite: attribs must not be null");
    MIFX_CHECK(to_img_wh(in.depth, MIFX_FORMAT_F32, W, H, "depth", k.depth));
    MIFX_CHECK(to_img_wh(in.selection_depth, MIFX_FORMAT_F32, W, H, "selection_depth", k.selectionDepth));
    MIFX_CHECK(to_img_wh(in.closest_location, MIFX_FORMAT_F32X2, W, H, "closest_location", k.closest));
    const mifx_selection_attribs& a = *in.attribs;
    MIFX_REQUIRE(a.outline_width > 0.0f, "selection composite: outline_width %g must be positive", double(a.outline_width));
    for (int i = 0; i < 3; ++i)
    {
        k.outline[i]  = a.outline_color[i];
        k.occluded[i] = a.occluded_outline_color[i];
    }
    k.desaturation = a.nonselection_desaturation;
    k.clearDepth   = a.clear_depth;
    k.outlineWidth = a.outline_width;
    return MIFX_OK;
}

// HnProcessSelectionTask::Execute for `sel`'s context on the rows that context needs
static mifx_status selection_run(mifx_selection* sel, const mifx_image2d* selectionDepth, const mifx_selection_attribs& a)
{
    mifx_postfx* ctx = sel->ctx;
    Img depth;
    MIFX_CHECK(to_img(selectionDepth, MIFX_FORMAT_F32, "selection_depth", depth));
    MIFX_REQUIRE(a.max_distance == a.max_distance, "mifx_selection_execute: max_distance is NaN");
    const uint32_t W = selectionDepth->width, H = selectionDepth->height;
    const int      n = jf_iterations(a.max_distance);
    MIFX_REQUIRE(n <= 24, "mifx_selection_execute: max_distance %g is beyond the frame sizes this library supports", double(a.max_distance));
    MIFX_CHECK(sel->out.alloc(W, H, MIFX_FORMAT_F32X2));
    if (n > kJfFused) MIFX_CHECK(sel->tmp[0].alloc(W, H, MIFX_FORMAT_F32X2));
    if (n > kJfFused + 1) MIFX_CHECK(sel->tmp[1].alloc(W, H, MIFX_FORMAT_F32X2));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    if (a.selection_id == 0) return sel->out.fill(ctx->stream, 0.0f); // nothing selected: the final target cleared to 0 (HnProcessSelectionTask.cpp:329-335)
    MifxKernelTimer timer(ctx, "jump_flood_kernel");
    const Rows rows = ctx->needed_rows(int(H));
    return launch_jump_flood(ctx->stream, depth, a.clear_depth, n, sel->tmp[0].view(), sel->tmp[1].view(), sel->out.view(), rows.b, rows.e);
}

static mifx_status hook_create(mifx_postfx* ctx, mifx_selection** out) { return mifx_selection_create(ctx, out); }
static void        hook_destroy(mifx_selection* sel) { mifx_selection_destroy(sel); }
static mifx_status hook_chain_composite(mifx_selection* sel, const mifx_selection_attribs& a, const mifx_image2d* selectionDepth, const mifx_composite_attribs& ca,
                                        const mifx_image2d* depth, const mifx_image2d* out, const SsrCleanupIn* r7)
{
    MIFX_CHECK(selection_run(sel, selectionDepth, a));
    const mifx_image2d closest = sel->out.desc();
    const mifx_selection_composite_inputs in{depth, selectionDepth, &closest, &a};
    SelectionK k;
    MIFX_CHECK(make_selectionk(in, out->width, out->height, k));
    mifx_postfx* ctx = sel->ctx;
    MifxKernelTimer timer(ctx, r7 ? "composite_ssr_cleanup_kernel" : "composite_kernel");
    const Rows rows = ctx->needed_rows(int(out->height));
    return launch_composite_selection(ctx->stream, ca, k, out, rows.b, rows.e, r7);
}
static const SelectionHooks kSelectionHooks{hook_create, hook_destroy, hook_chain_composite};
static const struct SelectionHooksInstaller
{
    SelectionHooksInstaller() { selection_hooks = &kSelectionHooks; }
} kSelectionHooksInstaller;
} // namespace mifx

using namespace mifx;

extern "C" {

mifx_status mifx_selection_create(mifx_postfx* ctx, mifx_selection** out)
{
    MIFX_REQUIRE(ctx != nullptr && out != nullptr, "mifx_selection_create: null argument");
    mifx_selection* sel = new mifx_selection();
    sel->ctx = ctx;
    *out = sel;
    return MIFX_OK;
}

void mifx_selection_destroy(mifx_selection* sel) { delete sel; }

mifx_status mifx_selection_execute(mifx_selection* sel, const mifx_image2d* selection_depth, const mifx_selection_attribs* attribs)
{
    MIFX_REQUIRE(sel != nullptr && selection_depth != nullptr && attribs != nullptr, "mifx_selection_execute: null argument");
    return selection_run(sel, selection_depth, *attribs);
}

mifx_status mifx_selection_get_output(mifx_selection* sel, mifx_image2d* out)
{
    MIFX_REQUIRE(sel != nullptr && out != nullptr, "mifx_selection_get_output: null argument");
    MIFX_REQUIRE(sel->out.data != nullptr, "mifx_selection_get_output: not executed yet");
    *out = sel->out.desc();
    return MIFX_OK;
}

mifx_status mifx_composite_execute_selection(mifx_postfx* ctx, const mifx_composite_attribs* attribs, const mifx_selection_composite_inputs* selection, const mifx_image2d* out)
{
    MIFX_REQUIRE(ctx != nullptr && attribs != nullptr && selection != nullptr && out != nullptr, "mifx_composite_execute_selection: null argument");
    SelectionK k;
    MIFX_CHECK(make_selectionk(*selection, out->width, out->height, k));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "composite_kernel");
    const Rows rows = ctx->needed_rows(int(out->height));
    return launch_composite_selection(ctx->stream, *attribs, k, out, rows.b, rows.e);
}

} // extern "C"
