// shadows.hip -- cascaded shadow maps: ShadowMapManager::ConvertToFilterable (Components/src/ShadowMapManager.cpp:533-600, Shaders/Shadows/private/ShadowConversions.fx)
// and the per-pixel look-up FilterShadowMap / SampleFilterableShadowMap (Shaders/Common/public/Shadows.fxh:219-253, 350-384).  The per-texel bodies are mifx_shadows.h.
//
// Conversion.  Bandwidth-bound: 4 B in, 8 or 16 B out per texel.  The reference draws twice per cascade through an intermediate array (a full extra write and read).
// shadow_convert_fused_kernel does both passes of a 64 x 16 tile in one launch, the cascade on the grid's z axis:
//   A  the depth texels of the tile plus its halo (up to 3 texels on every side: iFixedFilterSize 7) are read once and what the horizontal pass takes from each -- the
//      depth, or its exponential warps, which cost two expf and are otherwise evaluated once per TAP -- goes to LDS;
//   B  the horizontal pass of the tile's rows and of its vertical halo runs from LDS into LDS; a row outside the slice is 0, as a Load of the intermediate target is;
//   C  the vertical pass runs from LDS, one 8- or 16-byte store per texel.
// The arithmetic of each pass is the same template as in the two-launch kernels (shadow_horz / shadow_vert: weighted sums in the reference's tap order, divided by the total
// weight after each pass), the warps are the same function of the same texel, so the result equals the two-pass result bit for bit (tests/test_gpu_shadows.py).  LDS:
// 22 x 70 x NB + 22 x 64 x 2 NB floats = 34.8 KB for EVSM4, channel planes apart (consecutive lanes read consecutive words: no bank conflict).  A filter range above 3 in
// any cascade (a large fFilterWorldSize) takes the two launches through a scratch array held by the context (mifx_postfx::shadow_scratch), as does mifx_shadow_set_conversion_fusion(0); iFixedFilterSize == 2 is the
// horizontal kernel alone, straight into the target.
//
// Look-up.  One kernel, templated on SHADOW_MODE, BEST_CASCADE_SEARCH and FILTER_ACROSS_CASCADES; the PCF size is a wave-uniform branch.  8 x 8 pixels per wave
// (tiled_xy): the 2x2 quads and the PCF footprints of neighbouring pixels share cache lines.  The cascade index is per-pixel data: indexing the kernel-argument copy of
// the cascade table with a VGPR turns every member into a dependent vector load from the kernarg segment (mifx_device.h, stage_pyramid), so the block copies the table
// (512 bytes) to LDS once and a look-up is a ds_read; constant memory would serialise the same divergent index through the scalar cache.
#include "mifx_shadows_host.h"

#ifndef MIFX_STORAGE_H4
namespace mifx
{
constexpr int kTW = kShadowTileW, kTH = kShadowTileH, kR = kShadowFusedMaxRange;

template <int NB, bool EVSM> __global__ __launch_bounds__(256) void shadow_convert_horz_kernel(ShadowArrK src, FilterableArrK dst, ShadowConvK k)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y), s = int(blockIdx.z);
    if (x >= dst.w || y >= dst.h) return;
    float m[2 * NB];
    shadow_horz_texel<NB, EVSM>(src, s, x, y, k, m);
    st_moments<2 * NB>(dst, s, x, y, m);
}

template <int CH> __global__ __launch_bounds__(256) void shadow_convert_vert_kernel(FilterableArrK mid, FilterableArrK dst, ShadowConvK k)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y), s = int(blockIdx.z);
    if (x >= dst.w || y >= dst.h) return;
    float m[CH];
    shadow_vert_texel<CH>(mid, s, x, y, k, m);
    st_moments<CH>(dst, s, x, y, m);
}

// block (64, 4); grid (ceil(w / 64), ceil(h / 16), slices).  Every cascade's ranges are at most kShadowFusedMaxRange (the launcher's test).  The stages are
// mifx_shadows.h's shadow_tile_stage_a / _b / _c, which the host compilation walks serially.
template <int NB, bool EVSM> __global__ __launch_bounds__(256) void shadow_convert_fused_kernel(ShadowArrK src, FilterableArrK dst, ShadowConvK k)
{
    __shared__ float A[NB * kShadowTileRows * kShadowTileCols];
    __shared__ float B[2 * NB * kShadowTileRows * kShadowTileW];
    const ShadowTile tile = shadow_tile(k, int(blockIdx.z), int(blockIdx.x), int(blockIdx.y));
    const int        t    = int(threadIdx.y) * 64 + int(threadIdx.x);
    for (int i = t; i < kShadowTileRows * kShadowTileCols; i += 256) shadow_tile_stage_a<NB, EVSM>(i, tile, src, k, A);
    __syncthreads();
    for (int i = t; i < kShadowTileRows * kShadowTileW; i += 256) shadow_tile_stage_b<NB>(i, tile, src.h, A, B);
    __syncthreads();
    for (int q = 0; q < kShadowTileH / 4; ++q) shadow_tile_stage_c<NB>(int(threadIdx.x), int(threadIdx.y) + 4 * q, tile, dst, B);
}

template <int MODE, bool BEST, bool ACROSS> __global__ __launch_bounds__(256) void shadow_filter_kernel(Img depth, Img light, Img cascade, ShadowLookupK k, ShadowArrK map,
                                                                                                        FilterableArrK filterable)
{
    __shared__ mifx_cascade_attribs casc[MIFX_MAX_CASCADES];
    const unsigned t = threadIdx.x;
    if (t < sizeof(casc) / 4u) reinterpret_cast<float*>(casc)[t] = reinterpret_cast<const float*>(k.cascades)[t];
    __syncthreads();
    int x, y;
    if (!tiled_xy(light, x, y)) return;
    const FilteredShadow r = shadow_filter_at<MODE, BEST, ACROSS>(x, y, depth, k, casc, map, filterable);
    st<float>(light, x, y, r.lightAmount);
    if (cascade.p) GlobalAccess<v2>::store(cascade.p + size_t(y) * cascade.pitch + size_t(x) * 8u, v2{r.cascadeIdx, r.nextCascadeBlendAmount});
}

mifx_status launch_shadow_convert(hipStream_t s, DeviceScratch& scratch, const ShadowArrK& src, const FilterableArrK& dst, const ShadowConvK& k, uint32_t mode, bool skipBlur, bool fused)
{
    const dim3 block(64, 4, 1);
    const dim3 grid((src.w + 63) / 64, (src.h + 3) / 4, src.slices);
#define MIFX_SHADOW_BY_MODE(LAUNCH)                                 \
    switch (mode)                                                   \
    {                                                               \
        case MIFX_SHADOW_MODE_VSM: LAUNCH(1, false); break;         \
        case MIFX_SHADOW_MODE_EVSM2: LAUNCH(1, true); break;        \
        default: LAUNCH(2, true); break;                            \
    }
    if (skipBlur)
    {
#define MIFX_LAUNCH_H(NB, EVSM) hipLaunchKernelGGL((shadow_convert_horz_kernel<NB, EVSM>), grid, block, 0, s, src, dst, k)
        MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_H)
        MIFX_HIP_CHECK(hipGetLastError());
        return MIFX_OK;
    }
    bool fits = true;
    for (int i = 0; i < src.slices; ++i) fits = fits && shadow_filter_range(k.rH[i]) <= kR && shadow_filter_range(k.rV[i]) <= kR;
    if (fused && fits)
    {
        const dim3 tiles((src.w + kTW - 1) / kTW, (src.h + kTH - 1) / kTH, src.slices);
#define MIFX_LAUNCH_F(NB, EVSM) hipLaunchKernelGGL((shadow_convert_fused_kernel<NB, EVSM>), tiles, block, 0, s, src, dst, k)
        MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_F)
        MIFX_HIP_CHECK(hipGetLastError());
        return MIFX_OK;
    }
    const int      ch    = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    const unsigned pitch = unsigned(src.w) * 4u * unsigned(ch);
    const size_t   slice = size_t(pitch) * size_t(src.h), need = slice * size_t(src.slices);
    if (scratch.bytes < need) MIFX_HIP_CHECK(hipStreamSynchronize(s)); // (growing frees the old block)
    MIFX_CHECK(scratch.reserve(need));
    const FilterableArrK mid{static_cast<unsigned char*>(scratch.data), src.w, src.h, src.slices, int(pitch), slice};
#define MIFX_LAUNCH_HM(NB, EVSM) hipLaunchKernelGGL((shadow_convert_horz_kernel<NB, EVSM>), grid, block, 0, s, src, mid, k)
    MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_HM)
    MIFX_HIP_CHECK(hipGetLastError());
    if (ch == 4) hipLaunchKernelGGL((shadow_convert_vert_kernel<4>), grid, block, 0, s, mid, dst, k);
    else hipLaunchKernelGGL((shadow_convert_vert_kernel<2>), grid, block, 0, s, mid, dst, k);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}

mifx_status launch_shadow_filter(hipStream_t s, Img depth, Img light, Img cascade, const ShadowLookupK& k, const ShadowArrK& map, const FilterableArrK& filterable, uint32_t mode, bool best,
                                 bool across)
{
    const dim3 block(256, 1, 1);
    const dim3 grid((light.w + 31) / 32, (light.h + 7) / 8, 1);
#define MIFX_LAUNCH_L(M, B, A) hipLaunchKernelGGL((shadow_filter_kernel<M, B, A>), grid, block, 0, s, depth, light, cascade, k, map, filterable)
#define MIFX_LAUNCH_L_MODE(M)                                     \
    do                                                            \
    {                                                             \
        if (best && across) MIFX_LAUNCH_L(M, true, true);         \
        else if (best) MIFX_LAUNCH_L(M, true, false);             \
        else if (across) MIFX_LAUNCH_L(M, false, true);           \
        else MIFX_LAUNCH_L(M, false, false);                      \
    } while (0)
    switch (mode)
    {
        case MIFX_SHADOW_MODE_PCF: MIFX_LAUNCH_L_MODE(MIFX_SHADOW_MODE_PCF); break;
        case MIFX_SHADOW_MODE_VSM: MIFX_LAUNCH_L_MODE(MIFX_SHADOW_MODE_VSM); break;
        case MIFX_SHADOW_MODE_EVSM2: MIFX_LAUNCH_L_MODE(MIFX_SHADOW_MODE_EVSM2); break;
        default: MIFX_LAUNCH_L_MODE(MIFX_SHADOW_MODE_EVSM4); break;
    }
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
} // namespace mifx
#else  // MIFX_STORAGE_H4
// The native-storage build compiles no shadow kernels (its filterable formats, RG16 / RGBA16, are out of scope): the two launchers are these refusals, which
// mifx_shadow_convert_to_filterable and mifx_shadow_map_filter return once their arguments have passed every check.
namespace mifx
{
static mifx_status no_shadow_kernels(const char* who)
{
    set_error("%s: this build of the library has no shadow-map kernels (the native-storage build's filterable formats are not built)", who);
    return MIFX_ERR_NOT_IMPLEMENTED;
}
mifx_status launch_shadow_convert(hipStream_t, DeviceScratch&, const ShadowArrK&, const FilterableArrK&, const ShadowConvK&, uint32_t, bool, bool)
{
    return no_shadow_kernels("mifx_shadow_convert_to_filterable");
}
mifx_status launch_shadow_filter(hipStream_t, Img, Img, Img, const ShadowLookupK&, const ShadowArrK&, const FilterableArrK&, uint32_t, bool, bool)
{
    return no_shadow_kernels("mifx_shadow_map_filter");
}
} // namespace mifx
#endif // MIFX_STORAGE_H4
