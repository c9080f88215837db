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
// Formats.  The filterable array names its own texel format (FilterableArrK::fmt): fp32, or the reference's 16-bit RG16_UNORM / RG16_FLOAT / RGBA16_FLOAT -- a
// run-time choice in both builds of the library (ld_moments / st_moments branch on FilterableArrK::fmt; the kernels are instantiated per format and the
// launchers pick, so the branches fold: shadow_fixed_format).  With a 16-bit format the scratch array of the
// two launches has that format too (the horizontal result is rounded by its store, as the reference's intermediate target rounds it), and the fused kernel rounds
// stage B's results to the format's values before they go to LDS, which stays fp32: it still equals the two launches bit for bit.  Depth, light amount and the
// cascade plane are F32 / F32X2 in both builds, so the native-storage build compiles the same kernels.
//
// Look-up.  One kernel, templated on SHADOW_MODE, BEST_CASCADE_SEARCH and FILTER_ACROSS_CASCADES; the PCF size is a wave-uniform branch.  8 x 8 pixels per wave
// (tiled_xy): the 2x2 quads and the PCF footprints of neighbouring pixels share cache lines.  The cascade index is per-pixel data: indexing the kernel-argument copy of
// the cascade table with a VGPR turns every member into a dependent vector load from the kernarg segment (mifx_device.h, stage_pyramid), so the block copies the table
// (512 bytes) to LDS once and a look-up is a ds_read; constant memory would serialise the same divergent index through the scalar cache.
#include "mifx_shadows_host.h"

namespace mifx
{
constexpr int kTW = kShadowTileW, kTH = kShadowTileH, kR = kShadowFusedMaxRange;

// FMT: FilterableArrK::fmt of the target (and of the intermediate array) as a compile-time constant; the launchers pick the instantiation
template <int NB, bool EVSM, unsigned FMT> __global__ __launch_bounds__(256) void shadow_convert_horz_kernel(ShadowArrK src, FilterableArrK dst_, ShadowConvK k)
{
    const FilterableArrK dst = shadow_fixed_format<FMT>(dst_);
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y), s = int(blockIdx.z);
    if (x >= dst.w || y >= dst.h) return;
    float m[2 * NB];
    shadow_horz_texel<NB, EVSM>(src, s, x, y, k, m);
    st_moments<2 * NB>(dst, s, x, y, m);
}

template <int CH, unsigned FMT> __global__ __launch_bounds__(256) void shadow_convert_vert_kernel(FilterableArrK mid_, FilterableArrK dst_, ShadowConvK k)
{
    const FilterableArrK mid = shadow_fixed_format<FMT>(mid_), dst = shadow_fixed_format<FMT>(dst_); // (the intermediate target has the filterable map's own format)
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y), s = int(blockIdx.z);
    if (x >= dst.w || y >= dst.h) return;
    float m[CH];
    shadow_vert_texel<CH>(mid, s, x, y, k, m);
    st_moments<CH>(dst, s, x, y, m);
}

// block (64, 4); grid (ceil(w / 64), ceil(h / 16), slices).  Every cascade's ranges are at most kShadowFusedMaxRange (the launcher's test).  The stages are
// mifx_shadows.h's shadow_tile_stage_a / _b / _c, which the host compilation walks serially.
template <int NB, bool EVSM, unsigned FMT> __global__ __launch_bounds__(256) void shadow_convert_fused_kernel(ShadowArrK src, FilterableArrK dst_, ShadowConvK k)
{
    __shared__ float A[NB * kShadowTileRows * kShadowTileCols];
    __shared__ float B[2 * NB * kShadowTileRows * kShadowTileW];
    const FilterableArrK dst  = shadow_fixed_format<FMT>(dst_);
    const ShadowTile     tile = shadow_tile(k, int(blockIdx.z), int(blockIdx.x), int(blockIdx.y));
    const int            t    = int(threadIdx.y) * 64 + int(threadIdx.x);
    for (int i = t; i < kShadowTileRows * kShadowTileCols; i += 256) shadow_tile_stage_a<NB, EVSM>(i, tile, src, k, A);
    __syncthreads();
    for (int i = t; i < kShadowTileRows * kShadowTileW; i += 256) shadow_tile_stage_b<NB>(i, tile, src.h, A, B, FMT);
    __syncthreads();
    for (int q = 0; q < kShadowTileH / 4; ++q) shadow_tile_stage_c<NB>(int(threadIdx.x), int(threadIdx.y) + 4 * q, tile, dst, B);
}

template <int MODE, bool BEST, bool ACROSS, unsigned FMT> __global__ __launch_bounds__(256) void shadow_filter_kernel(Img depth, Img light, Img cascade, ShadowLookupK k, ShadowArrK map,
                                                                                                                      FilterableArrK filterable_)
{
    __shared__ mifx_cascade_attribs casc[MIFX_MAX_CASCADES];
    const FilterableArrK filterable = shadow_fixed_format<FMT>(filterable_);
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
    const bool narrow = dst.fmt != 0u; // (the entry has checked that a format other than fp32 is the mode's 16-bit one)
#define MIFX_SHADOW_BY_MODE(LAUNCH)                                                                          \
    switch (mode)                                                                                            \
    {                                                                                                        \
        case MIFX_SHADOW_MODE_VSM:                                                                           \
            if (narrow) LAUNCH(1, false, MIFX_FORMAT_U16X2);                                                 \
            else LAUNCH(1, false, 0u);                                                                       \
            break;                                                                                           \
        case MIFX_SHADOW_MODE_EVSM2:                                                                         \
            if (narrow) LAUNCH(1, true, MIFX_FORMAT_F16X2);                                                  \
            else LAUNCH(1, true, 0u);                                                                        \
            break;                                                                                           \
        default:                                                                                             \
            if (narrow) LAUNCH(2, true, MIFX_FORMAT_F16X4);                                                  \
            else LAUNCH(2, true, 0u);                                                                        \
            break;                                                                                           \
    }
    if (skipBlur)
    {
#define MIFX_LAUNCH_H(NB, EVSM, FMT) hipLaunchKernelGGL((shadow_convert_horz_kernel<NB, EVSM, FMT>), grid, block, 0, s, src, dst, k)
        MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_H)
        MIFX_HIP_CHECK(hipGetLastError());
        return MIFX_OK;
    }
    bool fits = true;
    for (int i = 0; i < src.slices; ++i) fits = fits && shadow_filter_range(k.rH[i]) <= kR && shadow_filter_range(k.rV[i]) <= kR;
    if (fused && fits)
    {
        const dim3 tiles((src.w + kTW - 1) / kTW, (src.h + kTH - 1) / kTH, src.slices);
#define MIFX_LAUNCH_F(NB, EVSM, FMT) hipLaunchKernelGGL((shadow_convert_fused_kernel<NB, EVSM, FMT>), tiles, block, 0, s, src, dst, k)
        MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_F)
        MIFX_HIP_CHECK(hipGetLastError());
        return MIFX_OK;
    }
    const int      ch    = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    const unsigned pitch = unsigned(src.w) * shadow_texel_bytes(dst.fmt, ch); // (the intermediate target has the filterable map's own format)
    const size_t   slice = size_t(pitch) * size_t(src.h), need = slice * size_t(src.slices);
    if (scratch.bytes < need) MIFX_HIP_CHECK(hipStreamSynchronize(s)); // (growing frees the old block)
    MIFX_CHECK(scratch.reserve(need));
    const FilterableArrK mid{static_cast<unsigned char*>(scratch.data), src.w, src.h, src.slices, int(pitch), slice, dst.fmt};
#define MIFX_LAUNCH_HM(NB, EVSM, FMT) hipLaunchKernelGGL((shadow_convert_horz_kernel<NB, EVSM, FMT>), grid, block, 0, s, src, mid, k)
    MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_HM)
    MIFX_HIP_CHECK(hipGetLastError());
#define MIFX_LAUNCH_V(NB, EVSM, FMT) hipLaunchKernelGGL((shadow_convert_vert_kernel<2 * NB, FMT>), grid, block, 0, s, mid, dst, k)
    MIFX_SHADOW_BY_MODE(MIFX_LAUNCH_V)
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}

mifx_status launch_shadow_filter(hipStream_t s, Img depth, Img light, Img cascade, const ShadowLookupK& k, const ShadowArrK& map, const FilterableArrK& filterable, uint32_t mode, bool best,
                                 bool across)
{
    const dim3 block(256, 1, 1);
    const dim3 grid((light.w + 31) / 32, (light.h + 7) / 8, 1);
    const bool narrow = filterable.fmt != 0u; // (the entry has checked that a format other than fp32 is the mode's 16-bit one)
#define MIFX_LAUNCH_L(M, B, A, F) hipLaunchKernelGGL((shadow_filter_kernel<M, B, A, F>), grid, block, 0, s, depth, light, cascade, k, map, filterable)
#define MIFX_LAUNCH_L_MODE(M, F)                                  \
    do                                                            \
    {                                                             \
        if (best && across) MIFX_LAUNCH_L(M, true, true, F);      \
        else if (best) MIFX_LAUNCH_L(M, true, false, F);          \
        else if (across) MIFX_LAUNCH_L(M, false, true, F);        \
        else MIFX_LAUNCH_L(M, false, false, F);                   \
    } while (0)
#define MIFX_LAUNCH_L_FORMAT(M, F16)          \
    do                                        \
    {                                         \
        if (narrow) MIFX_LAUNCH_L_MODE(M, F16); \
        else MIFX_LAUNCH_L_MODE(M, 0u);       \
    } while (0)
    switch (mode)
    {
        case MIFX_SHADOW_MODE_PCF: MIFX_LAUNCH_L_MODE(MIFX_SHADOW_MODE_PCF, 0u); break; // (reads no filterable map)
        case MIFX_SHADOW_MODE_VSM: MIFX_LAUNCH_L_FORMAT(MIFX_SHADOW_MODE_VSM, MIFX_FORMAT_U16X2); break;
        case MIFX_SHADOW_MODE_EVSM2: MIFX_LAUNCH_L_FORMAT(MIFX_SHADOW_MODE_EVSM2, MIFX_FORMAT_F16X2); break;
        default: MIFX_LAUNCH_L_FORMAT(MIFX_SHADOW_MODE_EVSM4, MIFX_FORMAT_F16X4); break;
    }
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
} // namespace mifx
