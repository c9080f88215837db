// TEST INFRASTRUCTURE ONLY.  The cascaded-shadow bodies (diligentfx_amd/csrc/mifx_shadows.h) compiled for the HOST (see layers_host.cpp for the method):
//   * ConvertToFilterable as the two passes through an intermediate array (what shadow_convert_horz_kernel / shadow_convert_vert_kernel do per texel);
//   * the look-up of every pixel of a frame (shadow_filter_kernel's body).
// Nothing in diligentfx_amd/ builds, loads or calls this.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include <vector>
#include "mifx.h"
#include "mifx_shadows.h"

using namespace mifx;

template <int NB, bool EVSM> static void convert(const ShadowArrK& src, const FilterableArrK& mid, const FilterableArrK& dst, const ShadowConvK& k, bool skipBlur)
{
    constexpr int CH = 2 * NB;
    const FilterableArrK& first = skipBlur ? dst : mid;
    for (int s = 0; s < src.slices; ++s)
    {
#pragma omp parallel for
        for (int y = 0; y < src.h; ++y)
            for (int x = 0; x < src.w; ++x)
            {
                float m[CH];
                shadow_horz_texel<NB, EVSM>(src, s, x, y, k, m);
                st_moments<CH>(first, s, x, y, m);
            }
        if (skipBlur) continue;
#pragma omp parallel for
        for (int y = 0; y < src.h; ++y)
            for (int x = 0; x < src.w; ++x)
            {
                float m[CH];
                shadow_vert_texel<CH>(mid, s, x, y, k, m);
                st_moments<CH>(dst, s, x, y, m);
            }
    }
}

// the fused kernel's stages, tile by tile (shadow_convert_fused_kernel: one block per tile and cascade, every stage complete before the next)
template <int NB, bool EVSM> static void convert_tiled(const ShadowArrK& src, const FilterableArrK& dst, const ShadowConvK& k)
{
    const int tx = (src.w + kShadowTileW - 1) / kShadowTileW, ty = (src.h + kShadowTileH - 1) / kShadowTileH;
#pragma omp parallel for collapse(2)
    for (int s = 0; s < src.slices; ++s)
        for (int by = 0; by < ty; ++by)
        {
            std::vector<float> A(size_t(NB) * kShadowTileRows * kShadowTileCols, -1.0f), B(size_t(2 * NB) * kShadowTileRows * kShadowTileW, -1.0f);
            for (int bx = 0; bx < tx; ++bx)
            {
                const ShadowTile t = shadow_tile(k, s, bx, by);
                for (int i = 0; i < kShadowTileRows * kShadowTileCols; ++i) shadow_tile_stage_a<NB, EVSM>(i, t, src, k, A.data());
                for (int i = 0; i < kShadowTileRows * kShadowTileW; ++i) shadow_tile_stage_b<NB>(i, t, src.h, A.data(), B.data());
                for (int ly = 0; ly < kShadowTileH; ++ly)
                    for (int lx = 0; lx < kShadowTileW; ++lx) shadow_tile_stage_c<NB>(lx, ly, t, dst, B.data());
            }
        }
}

template <int MODE> static void filter(const Img& depth, const ShadowLookupK& k, const ShadowArrK& map, const FilterableArrK& fm, bool best, bool across, float* light, float* cascade)
{
#pragma omp parallel for
    for (int y = 0; y < depth.h; ++y)
        for (int x = 0; x < depth.w; ++x)
        {
            FilteredShadow r;
            if (best && across) r = shadow_filter_at<MODE, true, true>(x, y, depth, k, k.cascades, map, fm);
            else if (best) r = shadow_filter_at<MODE, true, false>(x, y, depth, k, k.cascades, map, fm);
            else if (across) r = shadow_filter_at<MODE, false, true>(x, y, depth, k, k.cascades, map, fm);
            else r = shadow_filter_at<MODE, false, false>(x, y, depth, k, k.cascades, map, fm);
            const size_t i = size_t(y) * depth.w + x;
            light[i] = r.lightAmount;
            if (cascade) { cascade[2 * i] = r.cascadeIdx; cascade[2 * i + 1] = r.nextCascadeBlendAmount; }
        }
}

extern "C" {
// depth: slices x h x w floats, tightly packed; out: slices x h x w x (2 | 4) floats.  Returns 0, or -1 for a mode outside 2 .. 4.
int mifx_host_shadow_convert(const float* depth, int w, int h, int slices, const mifx_shadow_map_attribs* a, uint32_t mode, float* out)
{
    if (mode < MIFX_SHADOW_MODE_VSM || mode > MIFX_SHADOW_MODE_EVSM4) return -1;
    const int ch = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    std::vector<float> tmp(size_t(w) * h * slices * ch);
    const ShadowArrK     src{reinterpret_cast<const unsigned char*>(depth), w, h, slices, w * 4, static_cast<unsigned long long>(w) * h * 4u};
    const FilterableArrK mid{reinterpret_cast<unsigned char*>(tmp.data()), w, h, slices, w * 4 * ch, static_cast<unsigned long long>(w) * h * 4u * ch};
    const FilterableArrK dst{reinterpret_cast<unsigned char*>(out), w, h, slices, w * 4 * ch, static_cast<unsigned long long>(w) * h * 4u * ch};
    const ShadowConvK k    = make_shadowconvk(*a, w, h);
    const bool        skip = a->iFixedFilterSize == 2;
    if (mode == MIFX_SHADOW_MODE_VSM) convert<1, false>(src, mid, dst, k, skip);
    else if (mode == MIFX_SHADOW_MODE_EVSM2) convert<1, true>(src, mid, dst, k, skip);
    else convert<2, true>(src, mid, dst, k, skip);
    return 0;
}

// the same through the fused kernel's tile stages; -2 when a cascade's range exceeds what a tile holds (the library then takes the two launches), or for the size-2 filter
int mifx_host_shadow_convert_tiled(const float* depth, int w, int h, int slices, const mifx_shadow_map_attribs* a, uint32_t mode, float* out)
{
    if (mode < MIFX_SHADOW_MODE_VSM || mode > MIFX_SHADOW_MODE_EVSM4) return -1;
    const int ch = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    const ShadowArrK     src{reinterpret_cast<const unsigned char*>(depth), w, h, slices, w * 4, static_cast<unsigned long long>(w) * h * 4u};
    const FilterableArrK dst{reinterpret_cast<unsigned char*>(out), w, h, slices, w * 4 * ch, static_cast<unsigned long long>(w) * h * 4u * ch};
    const ShadowConvK k = make_shadowconvk(*a, w, h);
    if (a->iFixedFilterSize == 2) return -2;
    for (int i = 0; i < slices; ++i)
        if (shadow_filter_range(k.rH[i]) > kShadowFusedMaxRange || shadow_filter_range(k.rV[i]) > kShadowFusedMaxRange) return -2;
    if (mode == MIFX_SHADOW_MODE_VSM) convert_tiled<1, false>(src, dst, k);
    else if (mode == MIFX_SHADOW_MODE_EVSM2) convert_tiled<1, true>(src, dst, k);
    else convert_tiled<2, true>(src, dst, k);
    return 0;
}

// frame: H x W floats; map: slices x mh x mw floats (PCF) or x (2 | 4) floats (the other modes); light: H x W; cascade (may be null): H x W x 2
int mifx_host_shadow_filter(const float* frame, int W, int H, const mifx_camera_attribs* camera, const mifx_shadow_map_attribs* a, uint32_t mode, int across, int best,
                            const float* map, int mw, int mh, int slices, float* light, float* cascade)
{
    const Img           depth{reinterpret_cast<unsigned char*>(const_cast<float*>(frame)), W, H, W * 4, 0, 0};
    const ShadowLookupK k  = make_shadowlookupk(*camera, *a);
    const int           ch = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    ShadowArrK     sm{};
    FilterableArrK fm{};
    if (mode == MIFX_SHADOW_MODE_PCF) sm = ShadowArrK{reinterpret_cast<const unsigned char*>(map), mw, mh, slices, mw * 4, static_cast<unsigned long long>(mw) * mh * 4u};
    else fm = FilterableArrK{reinterpret_cast<unsigned char*>(const_cast<float*>(map)), mw, mh, slices, mw * 4 * ch, static_cast<unsigned long long>(mw) * mh * 4u * ch};
    switch (mode)
    {
        case MIFX_SHADOW_MODE_PCF: filter<MIFX_SHADOW_MODE_PCF>(depth, k, sm, fm, best != 0, across != 0, light, cascade); break;
        case MIFX_SHADOW_MODE_VSM: filter<MIFX_SHADOW_MODE_VSM>(depth, k, sm, fm, best != 0, across != 0, light, cascade); break;
        case MIFX_SHADOW_MODE_EVSM2: filter<MIFX_SHADOW_MODE_EVSM2>(depth, k, sm, fm, best != 0, across != 0, light, cascade); break;
        case MIFX_SHADOW_MODE_EVSM4: filter<MIFX_SHADOW_MODE_EVSM4>(depth, k, sm, fm, best != 0, across != 0, light, cascade); break;
        default: return -1;
    }
    return 0;
}
}
