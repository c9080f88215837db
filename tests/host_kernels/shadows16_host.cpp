// TEST INFRASTRUCTURE ONLY.  The cascaded-shadow bodies (diligentfx_amd/csrc/mifx_shadows.h) compiled for the HOST with a filterable array of any of its formats
// (FilterableArrK::fmt: 0 = fp32, MIFX_FORMAT_U16X2 / F16X2 / F16X4 = the 16-bit filterable formats) -- shadows_host.cpp's three entries with the format as an argument:
//   * ConvertToFilterable as the two passes through an intermediate array OF THE SAME FORMAT (what the two launches do per texel), or through the fused kernel's tile stages;
//   * the look-up of every pixel of a frame from an array of that format.
// Nothing in diligentfx_amd/ builds, loads or calls this.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include <vector>
#include "mifx.h"
#include "mifx_shadows.h"

using namespace mifx;

static FilterableArrK arr_of(void* p, int w, int h, int slices, int ch, unsigned fmt)
{
    const unsigned texel = shadow_texel_bytes(fmt, ch);
    return FilterableArrK{static_cast<unsigned char*>(p), w, h, slices, int(w * texel), static_cast<unsigned long long>(w) * h * texel, fmt};
}

template <int NB, bool EVSM> static void convert(const ShadowArrK& src, const FilterableArrK& mid, const FilterableArrK& dst, const ShadowConvK& k, bool skipBlur)
{
    constexpr int CH = 2 * NB;
    const FilterableArrK& first = skipBlur ? dst : mid;
    for (int s = 0; s < src.slices; ++s)
    {
        for (int y = 0; y < src.h; ++y)
            for (int x = 0; x < src.w; ++x)
            {
                float m[CH];
                shadow_horz_texel<NB, EVSM>(src, s, x, y, k, m);
                st_moments<CH>(first, s, x, y, m);
            }
        if (skipBlur) continue;
        for (int y = 0; y < src.h; ++y)
            for (int x = 0; x < src.w; ++x)
            {
                float m[CH];
                shadow_vert_texel<CH>(mid, s, x, y, k, m);
                st_moments<CH>(dst, s, x, y, m);
            }
    }
}

// the fused kernel's stages, tile by tile, the staging arrays poisoned beforehand
template <int NB, bool EVSM> static void convert_tiled(const ShadowArrK& src, const FilterableArrK& dst, const ShadowConvK& k)
{
    const int tx = (src.w + kShadowTileW - 1) / kShadowTileW, ty = (src.h + kShadowTileH - 1) / kShadowTileH;
    std::vector<float> A(size_t(NB) * kShadowTileRows * kShadowTileCols), B(size_t(2 * NB) * kShadowTileRows * kShadowTileW);
    for (int s = 0; s < src.slices; ++s)
        for (int by = 0; by < ty; ++by)
            for (int bx = 0; bx < tx; ++bx)
            {
                A.assign(A.size(), -1.0f);
                B.assign(B.size(), -1.0f);
                const ShadowTile t = shadow_tile(k, s, bx, by);
                for (int i = 0; i < kShadowTileRows * kShadowTileCols; ++i) shadow_tile_stage_a<NB, EVSM>(i, t, src, k, A.data());
                for (int i = 0; i < kShadowTileRows * kShadowTileW; ++i) shadow_tile_stage_b<NB>(i, t, src.h, A.data(), B.data(), dst.fmt);
                for (int ly = 0; ly < kShadowTileH; ++ly)
                    for (int lx = 0; lx < kShadowTileW; ++lx) shadow_tile_stage_c<NB>(lx, ly, t, dst, B.data());
            }
}

template <int MODE> static void filter(const Img& depth, const ShadowLookupK& k, const FilterableArrK& fm, bool best, bool across, float* light, float* cascade)
{
    const ShadowArrK none{};
    for (int y = 0; y < depth.h; ++y)
        for (int x = 0; x < depth.w; ++x)
        {
            FilteredShadow r;
            if (best && across) r = shadow_filter_at<MODE, true, true>(x, y, depth, k, k.cascades, none, fm);
            else if (best) r = shadow_filter_at<MODE, true, false>(x, y, depth, k, k.cascades, none, fm);
            else if (across) r = shadow_filter_at<MODE, false, true>(x, y, depth, k, k.cascades, none, fm);
            else r = shadow_filter_at<MODE, false, false>(x, y, depth, k, k.cascades, none, fm);
            const size_t i = size_t(y) * depth.w + x;
            light[i] = r.lightAmount;
            if (cascade) { cascade[2 * i] = r.cascadeIdx; cascade[2 * i + 1] = r.nextCascadeBlendAmount; }
        }
}

extern "C" {
// depth: slices x h x w floats; out: slices x h x w x (2 | 4) texel channels of `fmt` (4 bytes a channel for fmt 0, otherwise 2), tightly packed.  tiled != 0: the
// fused kernel's stages.  Returns 0; -1 for a mode outside 2 .. 4 or a format that is not the mode's; -2 (tiled) when a range exceeds what a tile holds or for the
// size-2 filter.
int mifx_host_shadow16_convert(const float* depth, int w, int h, int slices, const mifx_shadow_map_attribs* a, uint32_t mode, uint32_t fmt, void* out, int tiled)
{
    if (mode < MIFX_SHADOW_MODE_VSM || mode > MIFX_SHADOW_MODE_EVSM4) return -1;
    const uint32_t fmt16 = mode == MIFX_SHADOW_MODE_EVSM4 ? MIFX_FORMAT_F16X4 : mode == MIFX_SHADOW_MODE_EVSM2 ? MIFX_FORMAT_F16X2 : MIFX_FORMAT_U16X2;
    if (fmt != 0u && fmt != fmt16) return -1;
    const int ch = mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    std::vector<float> tmp(size_t(w) * h * slices * ch); // (large enough for either texel size)
    const ShadowArrK     src{reinterpret_cast<const unsigned char*>(depth), w, h, slices, w * 4, static_cast<unsigned long long>(w) * h * 4u};
    const FilterableArrK mid = arr_of(tmp.data(), w, h, slices, ch, fmt), dst = arr_of(out, w, h, slices, ch, fmt);
    const ShadowConvK    k    = make_shadowconvk(*a, w, h);
    const bool           skip = a->iFixedFilterSize == 2;
    if (tiled)
    {
        if (skip) return -2;
        for (int i = 0; i < slices; ++i)
            if (shadow_filter_range(k.rH[i]) > kShadowFusedMaxRange || shadow_filter_range(k.rV[i]) > kShadowFusedMaxRange) return -2;
        if (mode == MIFX_SHADOW_MODE_VSM) convert_tiled<1, false>(src, dst, k);
        else if (mode == MIFX_SHADOW_MODE_EVSM2) convert_tiled<1, true>(src, dst, k);
        else convert_tiled<2, true>(src, dst, k);
        return 0;
    }
    if (mode == MIFX_SHADOW_MODE_VSM) convert<1, false>(src, mid, dst, k, skip);
    else if (mode == MIFX_SHADOW_MODE_EVSM2) convert<1, true>(src, mid, dst, k, skip);
    else convert<2, true>(src, mid, dst, k, skip);
    return 0;
}

// frame: H x W floats; map: slices x mh x mw x (2 | 4) texel channels of `fmt`, tightly packed; light: H x W; cascade (may be null): H x W x 2
int mifx_host_shadow16_filter(const float* frame, int W, int H, const mifx_camera_attribs* camera, const mifx_shadow_map_attribs* a, uint32_t mode, int across, int best,
                              const void* map, uint32_t fmt, int mw, int mh, int slices, float* light, float* cascade)
{
    const Img            depth{reinterpret_cast<unsigned char*>(const_cast<float*>(frame)), W, H, W * 4, 0, 0};
    const ShadowLookupK  k  = make_shadowlookupk(*camera, *a);
    const FilterableArrK fm = arr_of(const_cast<void*>(map), mw, mh, slices, mode == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2, fmt);
    switch (mode)
    {
        case MIFX_SHADOW_MODE_VSM: filter<MIFX_SHADOW_MODE_VSM>(depth, k, fm, best != 0, across != 0, light, cascade); break;
        case MIFX_SHADOW_MODE_EVSM2: filter<MIFX_SHADOW_MODE_EVSM2>(depth, k, fm, best != 0, across != 0, light, cascade); break;
        case MIFX_SHADOW_MODE_EVSM4: filter<MIFX_SHADOW_MODE_EVSM4>(depth, k, fm, best != 0, across != 0, light, cascade); break;
        default: return -1;
    }
    return 0;
}

// what a store + load of the format does to each of n values (shadow_quantize), and the codes a store writes (2 bytes each)
void mifx_host_shadow16_quantize(const float* in, int n, uint32_t fmt, float* values)
{
    for (int i = 0; i < n; ++i) values[i] = shadow_quantize(fmt, in[i]);
}
}
