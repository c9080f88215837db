// mifx_shadows.h -- cascaded shadow maps, per texel: the bodies of the conversion kernels (Shaders/Shadows/private/ShadowConversions.fx: GetSampleWeight :24,
// VSMHorzPS :31, EVSMHorzPS :46, VertBlurPS :64) and of the look-up kernel (Shaders/Common/public/Shadows.fxh: GetDistanceToCascadeMargin :30, GetCascadeSamplingInfo
// :49, FindCascade :65, GetNextCascadeBlendAmount :114, ComputeReceiverPlaneDepthBias :148, FilterShadowCascade :179, FilterShadowMap :219, ChebyshevUpperBound :265,
// WarpDepthEVSM :288, SampleVSM / SampleEVSM :297-330, SampleFilterableShadowMap :350; Shaders/Common/public/PCF.fxh: FilterShadowMapFixedPCF :7,
// FilterShadowMapVaryingPCF :157), in a header so that the test suite can also compile it for the host (tests/host_kernels/shadows_host.cpp).
//
// Arithmetic.  Strict fp32 in the reference's operation order: no contraction (`#pragma clang fp contract(off)` in every body), IEEE division (plain `/`), libm expf.
// EVSM subtracts squared moments of magnitude e^80 (Variance = m2 - m1 * m1), a PCF sample compares a biased depth with a texel, and the receiver-plane bias divides
// by a determinant of derivatives: none of these tolerates a fused multiply-add or an approximate quotient.  fmin / fmax ignore a NaN operand as HLSL's min / max do:
// clamp(NaN, -c, c) = -c, which is what the receiver-plane bias of a pixel without derivatives (0 / 0) becomes.
//
// Conventions of this library (include/mifx.h, mifx_shadow_map_filter): position from the pixel's own depth, quad derivatives with the partners recomputed from
// their depth texels (a partner outside the frame = the pixel itself), background pixels lit, SampleGrad = bilinear clamped fetch of the only mip.
#pragma once
#include <cmath>
#include "mifx.h"
#include "mifx_device.h"

namespace mifx
{
constexpr int kShadowFusedMaxRange = 3; // the largest filter range (texels) whose halo the fused conversion kernel holds in LDS: iFixedFilterSize 7

// Texture2DArray<float>: the depth cascades
struct ShadowArrK
{
    const unsigned char* data;
    int                  w, h, slices, pitch;
    unsigned long long   slicePitch;
};
// the filterable array (or the intermediate target of the two-launch conversion): CH = 2 or 4 channels per texel.  fmt == 0: true fp32 channels (F32X2 / F32X4 by
// the channel count); otherwise one of the reference's 16-bit filterable formats (ShadowMapManager.cpp:98-102, Is32BitFilterableFmt == false): MIFX_FORMAT_U16X2
// (RG16_UNORM, VSM), MIFX_FORMAT_F16X2 (RG16_FLOAT, EVSM2), MIFX_FORMAT_F16X4 (RGBA16_FLOAT, EVSM4) -- 2 bytes a channel.  A load widens to fp32, a store converts
// the way a render-target write of the format does (mifx_device.h: unorm16_code, quantize_half); everything between stays fp32.  The branches on the
// field are uniform over a launch; the kernels fix it at compile time (shadow_fixed_format below), the host compilation of the test suite takes them as they are.
struct FilterableArrK
{
    unsigned char*     data;
    int                w, h, slices, pitch;
    unsigned long long slicePitch;
    unsigned           fmt;
};
MIFX_HD unsigned shadow_texel_bytes(unsigned fmt, int ch) { return (fmt ? 2u : 4u) * unsigned(ch); }
// what a store to the array followed by a load does to a value
MIFX_D float shadow_quantize(unsigned fmt, float v) { return fmt == 0u ? v : fmt == MIFX_FORMAT_U16X2 ? quantize_unorm16(v) : quantize_half(v); }
typedef unsigned short mifx_us2 __attribute__((ext_vector_type(2)));
template <int CH> MIFX_D void ld_moments(const FilterableArrK& a, int s, int x, int y, float (&m)[CH])
{
    const unsigned char* p = a.data + size_t(s) * a.slicePitch + size_t(y) * a.pitch + size_t(x) * shadow_texel_bytes(a.fmt, CH);
    if (a.fmt == 0u)
    {
        if (CH == 2)
        {
            const mifx_f2 t = *(const MIFX_GLOBAL mifx_f2*)p;
            m[0] = t.x; m[1] = t.y;
        }
        else
        {
            const mifx_f4 t = *(const MIFX_GLOBAL mifx_f4*)p;
            m[0] = t.x; m[1] = t.y; m[CH - 2] = t.z; m[CH - 1] = t.w;
        }
    }
    else if (CH == 2 && a.fmt == MIFX_FORMAT_U16X2)
    {
        const mifx_us2 t = *(const MIFX_GLOBAL mifx_us2*)p;
        m[0] = unorm16_value(float(t.x)); m[1] = unorm16_value(float(t.y));
    }
    else if (CH == 2)
    {
        const mifx_h2 t = *(const MIFX_GLOBAL mifx_h2*)p;
        m[0] = float(t.x); m[1] = float(t.y);
    }
    else
    {
        const mifx_h4 t = *(const MIFX_GLOBAL mifx_h4*)p;
        m[0] = float(t.x); m[1] = float(t.y); m[CH - 2] = float(t.z); m[CH - 1] = float(t.w);
    }
}
template <int CH> MIFX_D void st_moments(const FilterableArrK& a, int s, int x, int y, const float (&m)[CH])
{
    unsigned char* p = a.data + size_t(s) * a.slicePitch + size_t(y) * a.pitch + size_t(x) * shadow_texel_bytes(a.fmt, CH);
    if (a.fmt == 0u)
    {
        if (CH == 2) *(MIFX_GLOBAL mifx_f2*)p = mifx_f2{m[0], m[1]};
        else *(MIFX_GLOBAL mifx_f4*)p = mifx_f4{m[0], m[1], m[CH - 2], m[CH - 1]};
    }
    else if (CH == 2 && a.fmt == MIFX_FORMAT_U16X2)
        *(MIFX_GLOBAL mifx_us2*)p = mifx_us2{(unsigned short)(unsigned(unorm16_code(m[0]))), (unsigned short)(unsigned(unorm16_code(m[1])))};
    else if (CH == 2) *(MIFX_GLOBAL mifx_h2*)p = mifx_h2{_Float16(m[0]), _Float16(m[1])};
    else *(MIFX_GLOBAL mifx_h4*)p = mifx_h4{_Float16(m[0]), _Float16(m[1]), _Float16(m[CH - 2]), _Float16(m[CH - 1])};
}
// `a` with its format the compile-time constant FMT: the kernels are instantiated per format (the launcher picks by FilterableArrK::fmt), so the branches of
// ld_moments / st_moments fold away and the fp32 instantiation is the code it was before the 16-bit formats existed.  Left as run-time branches inside the tap
// loops they cost the fp32 two-launch conversion up to 13 %, taken once per kernel around the loops still 3 - 7 % on the one-tap horizontal kernel (same-box A/Bs
// against the parent commit).  a.fmt == FMT is expected: the entries accept a format other than fp32 only if it is the mode's 16-bit one
// (api_shadows.cpp to_filterable_arr), and the launchers pick FMT from a.fmt and the mode, so FMT is the one source of truth inside a kernel.
template <unsigned FMT> MIFX_D FilterableArrK shadow_fixed_format(const FilterableArrK& a)
{
    FilterableArrK k = a;
    k.fmt = FMT;
    return k;
}
// Load(int4(x, y, slice, 0)).r of the depth array: 0 outside the slice
MIFX_D float ld_shadow_depth_zero(const ShadowArrK& a, int s, int x, int y)
{
    if (unsigned(x) >= unsigned(a.w) || unsigned(y) >= unsigned(a.h)) return 0.0f;
    return *(const MIFX_GLOBAL float*)(a.data + size_t(s) * a.slicePitch + size_t(y) * a.pitch + size_t(x) * 4u);
}

// ------------------------------------------------------------------------------------------------ conversion
// ConversionAttribs of every cascade, as ShadowMapManager::ConvertToFilterable fills them in (:545-582); the exponents after GetEVSMExponents
struct ShadowConvK
{
    float rH[MIFX_MAX_CASCADES], rV[MIFX_MAX_CASCADES];
    float expPos, expNeg;
};
// GetEVSMExponents (Shadows.fxh:280-285)
inline void shadow_evsm_exponents(const mifx_shadow_map_attribs& a, float& pos, float& neg)
{
    const float maxExponent = a.bIs32BitEVSM ? 42.0f : 5.54f;
    pos = fminf(a.fEVSMPositiveExponent, maxExponent);
    neg = fminf(a.fEVSMNegativeExponent, maxExponent);
}
inline ShadowConvK make_shadowconvk(const mifx_shadow_map_attribs& a, int w, int h)
{
    ShadowConvK k{};
    const int iFilterRadius = (a.iFixedFilterSize - 1) / 2;
    for (int i = 0; i < MIFX_MAX_CASCADES; ++i)
    {
        if (a.iFixedFilterSize > 0) k.rH[i] = k.rV[i] = static_cast<float>(iFilterRadius);
        else
        {
            const float fNDCtoUVScale = 0.5f;
            const float fFilterWidth  = a.fFilterWorldSize * a.Cascades[i].f4LightSpaceScale[0] * fNDCtoUVScale;
            const float fFilterHeight = a.fFilterWorldSize * a.Cascades[i].f4LightSpaceScale[1] * fNDCtoUVScale;
            k.rH[i] = fFilterWidth / 2.f * static_cast<float>(w);
            k.rV[i] = fFilterHeight / 2.f * static_cast<float>(h);
        }
    }
    shadow_evsm_exponents(a, k.expPos, k.expNeg);
    return k;
}

MIFX_D float shadow_sample_weight(int x, float r) // GetSampleWeight
{
#pragma clang fp contract(off)
    const float fTexelMin = fmaxf(float(x), fminf(0.5f - r, 0.0f));
    const float fTexelMax = fminf(float(x) + 1.0f, fmaxf(0.5f + r, 1.0f));
    return fTexelMax - fTexelMin;
}
MIFX_HD int shadow_filter_range(float r) { return int(floorf(r + 0.5f)); }
// WarpDepthEVSM (Shadows.fxh:288-295)
MIFX_D v2 shadow_warp_evsm(float depth, float ePos, float eNeg)
{
#pragma clang fp contract(off)
    depth = 2.0f * depth - 1.0f;
    const float pos = expf(ePos * depth);
    const float neg = -expf(-eNeg * depth);
    return v2{pos, neg};
}
// What the horizontal pass takes from one depth texel, NB values: the depth (VSM), the positive warp (EVSM2), both warps (EVSM4).  Each contributes the moments
// (x, x * x), so the target has 2 * NB channels -- the reference's EVSM shader computes all four and an RG target keeps the first two.
template <int NB, bool EVSM> MIFX_D void shadow_base(float depth, const ShadowConvK& k, float (&x)[NB])
{
    if (!EVSM) x[0] = depth;
    else
    {
        const v2 w = shadow_warp_evsm(depth, k.expPos, k.expNeg);
        x[0] = w.x;
        if (NB == 2) x[NB - 1] = w.y;
    }
}
// VSMHorzPS / EVSMHorzPS: base(i, x) returns the NB values of the texel i columns to the right
template <int NB, class F> MIFX_D void shadow_horz(F base, float radius, float (&out)[2 * NB])
{
#pragma clang fp contract(off)
    float acc[2 * NB];
    for (int c = 0; c < 2 * NB; ++c) acc[c] = 0.0f;
    float     total = 0.0f;
    const int range = shadow_filter_range(radius);
    for (int i = -range; i <= range; ++i)
    {
        const float w = shadow_sample_weight(i, radius);
        float       x[NB];
        base(i, x);
#pragma unroll
        for (int b = 0; b < NB; ++b)
        {
            const float sq = x[b] * x[b];
            acc[2 * b]     = acc[2 * b] + x[b] * w;
            acc[2 * b + 1] = acc[2 * b + 1] + sq * w;
        }
        total = total + w;
    }
    for (int c = 0; c < 2 * NB; ++c) out[c] = acc[c] / total;
}
// VertBlurPS: src(i, m) returns the CH moments of the texel i rows below (0 outside the slice)
template <int CH, class F> MIFX_D void shadow_vert(F src, float radius, float (&out)[CH])
{
#pragma clang fp contract(off)
    float acc[CH];
    for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
    float     total = 0.0f;
    const int range = shadow_filter_range(radius);
    for (int i = -range; i <= range; ++i)
    {
        const float w = shadow_sample_weight(i, radius);
        float       m[CH];
        src(i, m);
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = acc[c] + m[c] * w;
        total = total + w;
    }
    for (int c = 0; c < CH; ++c) out[c] = acc[c] / total;
}
// the two passes straight from memory (the two-launch path and the host compilation)
template <int NB, bool EVSM> MIFX_D void shadow_horz_texel(const ShadowArrK& src, int s, int x, int y, const ShadowConvK& k, float (&out)[2 * NB])
{
    shadow_horz<NB>([&](int i, float (&b)[NB]) { shadow_base<NB, EVSM>(ld_shadow_depth_zero(src, s, x + i, y), k, b); }, k.rH[s], out);
}
template <int CH> MIFX_D void shadow_vert_texel(const FilterableArrK& mid, int s, int x, int y, const ShadowConvK& k, float (&out)[CH])
{
    shadow_vert<CH>(
        [&](int i, float (&m)[CH]) {
            if (unsigned(y + i) >= unsigned(mid.h))
                for (int c = 0; c < CH; ++c) m[c] = 0.0f;
            else ld_moments<CH>(mid, s, x, y + i, m);
        },
        k.rV[s], out);
}

// ---- both passes of one 64 x 16 tile through two staging arrays (LDS in shadow_convert_fused_kernel; the host compilation walks the same stages serially):
//   A[NB][kShadowTileRows][kShadowTileCols]  what the horizontal pass takes from every depth texel of the tile and its halo (kShadowFusedMaxRange texels on every side)
//   B[2 NB][kShadowTileRows][kShadowTileW]   the horizontal pass of the tile's rows and its vertical halo; a row outside the slice is 0, as a Load of the intermediate is
constexpr int kShadowTileW = 64, kShadowTileH = 16, kShadowTileRows = kShadowTileH + 2 * kShadowFusedMaxRange, kShadowTileCols = kShadowTileW + 2 * kShadowFusedMaxRange;
struct ShadowTile
{
    int   s, x0, y0;                    // cascade, the tile's first texel
    float rH, rV;
    int   rowLo, rowHi, colLo, colHi;   // the part of A / B that this cascade's ranges need
};
MIFX_D ShadowTile shadow_tile(const ShadowConvK& k, int s, int bx, int by)
{
    ShadowTile t;
    t.s = s; t.x0 = bx * kShadowTileW; t.y0 = by * kShadowTileH;
    t.rH = k.rH[s]; t.rV = k.rV[s];
    const int rangeH = min(max(shadow_filter_range(t.rH), 0), kShadowFusedMaxRange), rangeV = min(max(shadow_filter_range(t.rV), 0), kShadowFusedMaxRange);
    t.rowLo = kShadowFusedMaxRange - rangeV; t.rowHi = kShadowFusedMaxRange + kShadowTileH + rangeV;
    t.colLo = kShadowFusedMaxRange - rangeH; t.colHi = kShadowFusedMaxRange + kShadowTileW + rangeH;
    return t;
}
// element i of A, i < kShadowTileRows * kShadowTileCols
template <int NB, bool EVSM> MIFX_D void shadow_tile_stage_a(int i, const ShadowTile& t, const ShadowArrK& src, const ShadowConvK& k, float* A)
{
    const int r = i / kShadowTileCols, c = i - r * kShadowTileCols, gy = t.y0 + r - kShadowFusedMaxRange;
    if (r < t.rowLo || r >= t.rowHi || c < t.colLo || c >= t.colHi || unsigned(gy) >= unsigned(src.h)) return;
    float b[NB];
    shadow_base<NB, EVSM>(ld_shadow_depth_zero(src, t.s, t.x0 + c - kShadowFusedMaxRange, gy), k, b);
#pragma unroll
    for (int n = 0; n < NB; ++n) A[(n * kShadowTileRows + r) * kShadowTileCols + c] = b[n];
}
// element i of B, i < kShadowTileRows * kShadowTileW.  fmt: the target's FilterableArrK::fmt -- the reference's intermediate target has the filterable map's own
// format (ShadowMapManager.cpp:120-123), so the horizontal result takes the values that format keeps before the vertical pass reads it (B itself stays fp32)
template <int NB> MIFX_D void shadow_tile_stage_b(int i, const ShadowTile& t, int sliceH, const float* A, float* B, unsigned fmt = 0u)
{
    constexpr int CH = 2 * NB;
    const int r = i / kShadowTileW, c = i - r * kShadowTileW, gy = t.y0 + r - kShadowFusedMaxRange;
    if (r < t.rowLo || r >= t.rowHi) return;
    float m[CH];
    if (unsigned(gy) >= unsigned(sliceH))
    {
#pragma unroll
        for (int n = 0; n < CH; ++n) m[n] = 0.0f;
    }
    else
        shadow_horz<NB>(
            [&](int j, float (&b)[NB]) {
#pragma unroll
                for (int n = 0; n < NB; ++n) b[n] = A[(n * kShadowTileRows + r) * kShadowTileCols + c + kShadowFusedMaxRange + j];
            },
            t.rH, m);
#pragma unroll
    for (int n = 0; n < CH; ++n) B[(n * kShadowTileRows + r) * kShadowTileW + c] = shadow_quantize(fmt, m[n]);
}
// the texel (lx, ly) of the tile
template <int NB> MIFX_D void shadow_tile_stage_c(int lx, int ly, const ShadowTile& t, const FilterableArrK& dst, const float* B)
{
    constexpr int CH = 2 * NB;
    const int gx = t.x0 + lx, gy = t.y0 + ly;
    if (gx >= dst.w || gy >= dst.h) return;
    float o[CH];
    shadow_vert<CH>(
        [&](int j, float (&m)[CH]) {
#pragma unroll
            for (int n = 0; n < CH; ++n) m[n] = B[(n * kShadowTileRows + ly + kShadowFusedMaxRange + j) * kShadowTileW + lx];
        },
        t.rV, o);
    st_moments<CH>(dst, t.s, gx, gy, o);
}

// ------------------------------------------------------------------------------------------------ look-up
struct ShadowLookupK
{
    float vpi[16];                // camera mViewProjInv
    float w2l[16];                // mWorldToLightView
    float p22, p23, p32, p33;     // camera mProj
    float farDepth;               // camera fFarPlaneDepth
    float zEnd[MIFX_MAX_CASCADES];
    float dim[4];                 // f4ShadowMapDim
    int   numCascades;
    float biasClamp, fixedBias, transition, vsmBias, lightBleedingReduction;
    float expPos, expNeg;         // after GetEVSMExponents
    int   fixedFilterSize;
    float filterWorldSize;
    mifx_cascade_attribs cascades[MIFX_MAX_CASCADES];
};
inline ShadowLookupK make_shadowlookupk(const mifx_camera_attribs& c, const mifx_shadow_map_attribs& a)
{
    ShadowLookupK k{};
    for (int i = 0; i < 16; ++i) { k.vpi[i] = c.mViewProjInv[i]; k.w2l[i] = a.mWorldToLightView[i]; }
    k.p22 = c.mProj[10]; k.p23 = c.mProj[11]; k.p32 = c.mProj[14]; k.p33 = c.mProj[15];
    k.farDepth = c.fFarPlaneDepth;
    for (int i = 0; i < MIFX_MAX_CASCADES; ++i) { k.zEnd[i] = a.fCascadeCamSpaceZEnd[i]; k.cascades[i] = a.Cascades[i]; }
    for (int i = 0; i < 4; ++i) k.dim[i] = a.f4ShadowMapDim[i];
    k.numCascades = a.iNumCascades;
    k.biasClamp = a.fReceiverPlaneDepthBiasClamp; k.fixedBias = a.fFixedDepthBias; k.transition = a.fCascadeTransitionRegion;
    k.vsmBias = a.fVSMBias; k.lightBleedingReduction = a.fVSMLightBleedingReduction;
    shadow_evsm_exponents(a, k.expPos, k.expNeg);
    k.fixedFilterSize = a.iFixedFilterSize;
    k.filterWorldSize = a.fFilterWorldSize;
    return k;
}

// PosInLightViewSpace of the pixel (x, y) of a W x H frame whose depth texel is `depth` (the convention of include/mifx.h)
MIFX_D v3 shadow_pos_in_light_view(int x, int y, int W, int H, float depth, const ShadowLookupK& k)
{
#pragma clang fp contract(off)
    const float nx = 2.0f * ((float(x) + 0.5f) / float(W)) - 1.0f, ny = 1.0f - 2.0f * ((float(y) + 0.5f) / float(H));
    const float* M = k.vpi;
    const float cx = nx * M[0] + ny * M[4] + depth * M[8] + 1.0f * M[12];
    const float cy = nx * M[1] + ny * M[5] + depth * M[9] + 1.0f * M[13];
    const float cz = nx * M[2] + ny * M[6] + depth * M[10] + 1.0f * M[14];
    const float cw = nx * M[3] + ny * M[7] + depth * M[11] + 1.0f * M[15];
    const float wx = cx / cw, wy = cy / cw, wz = cz / cw;
    const float* L = k.w2l;
    return v3{wx * L[0] + wy * L[4] + wz * L[8] + 1.0f * L[12], wx * L[1] + wy * L[5] + wz * L[9] + 1.0f * L[13], wx * L[2] + wy * L[6] + wz * L[10] + 1.0f * L[14]};
}
MIFX_D float shadow_camera_z(float depth, const ShadowLookupK& k) // DepthToCameraZ (ShaderUtilities.fxh:24-39)
{
#pragma clang fp contract(off)
    return (k.p32 - depth * k.p33) / (depth * k.p23 - k.p22);
}

struct CascadeSamplingInfo
{
    int   idx;
    v2    uv;
    float depth;
    v3    scale;
    float minDistToMargin;
};
MIFX_D float shadow_distance_to_margin(v3 p, const float* margin) // GetDistanceToCascadeMargin, NDC_MIN_Z = 0: ZScale = 2
{
#pragma clang fp contract(off)
    const float dx = 1.0f - margin[0] - fabsf(p.x), dy = 1.0f - margin[1] - fabsf(p.y);
    const float dz = (p.z - (0.0f + margin[2])) * 2.0f;
    const float dw = (1.0f - margin[3] - p.z) * 2.0f;
    return fminf(fminf(dx, dy), fminf(dz, dw));
}
MIFX_D CascadeSamplingInfo shadow_cascade_sampling_info(const mifx_cascade_attribs* cascades, v3 pos, int idx) // GetCascadeSamplingInfo
{
#pragma clang fp contract(off)
    const mifx_cascade_attribs& c = cascades[idx];
    CascadeSamplingInfo si;
    si.scale = v3{c.f4LightSpaceScale[0], c.f4LightSpaceScale[1], c.f4LightSpaceScale[2]};
    const v3 p{pos.x * si.scale.x + c.f4LightSpaceScaledBias[0], pos.y * si.scale.y + c.f4LightSpaceScaledBias[1], pos.z * si.scale.z + c.f4LightSpaceScaledBias[2]};
    si.idx   = idx;
    si.uv    = v2{0.5f + 0.5f * p.x, 0.5f + -0.5f * p.y}; // NormalizedDeviceXYToTexUV
    si.depth = p.z;                                        // NormalizedDeviceZToDepth
    si.minDistToMargin = shadow_distance_to_margin(p, c.f4MarginProjSpace);
    return si;
}
// FindCascade.  The index is iNumCascades (or more: garbage in the unused entries of the last group of four, see include/mifx.h) when no cascade holds the point.
template <bool BEST> MIFX_D CascadeSamplingInfo shadow_find_cascade(const ShadowLookupK& k, const mifx_cascade_attribs* cascades, v3 pos, float camZ)
{
    CascadeSamplingInfo si{};
    int idx = 0;
    if (BEST)
    {
        while (idx < k.numCascades)
        {
            si = shadow_cascade_sampling_info(cascades, pos, idx);
            if (si.minDistToMargin > 0.0f) break;
            ++idx;
        }
    }
    else
    {
        const int groups = (k.numCascades + 3) / 4;
        for (int i = 0; i < 4 * groups; ++i) idx += k.zEnd[i] < camZ ? 1 : 0;
        if (idx < k.numCascades) si = shadow_cascade_sampling_info(cascades, pos, idx);
    }
    si.idx = idx;
    return si;
}
template <bool BEST> MIFX_D float shadow_next_cascade_blend(const ShadowLookupK& k, const mifx_cascade_attribs* cascades, float camZ, const CascadeSamplingInfo& si,
                                                            const CascadeSamplingInfo& next) // GetNextCascadeBlendAmount
{
#pragma clang fp contract(off)
    const float* se = cascades[si.idx].f4StartEndZ;
    float d = (se[1] - camZ) / (se[1] - se[0]);
    if (BEST) d = fmaxf(d, si.minDistToMargin);
    return saturate(1.0f - d / k.transition) * saturate(next.minDistToMargin / 0.01f);
}

// SampleCmpLevelZero of Sam_ComparisonLinearClamp: "reference < texel" over the clamped 2x2 footprint of the slice, blended with the bilinear weights
MIFX_D float shadow_sample_cmp(const ShadowArrK& a, float u, float v, int slice, float ref)
{
#pragma clang fp contract(off)
    const int   s  = clampi(slice, 0, a.slices - 1);
    const float fx = u * float(a.w) - 0.5f, fy = v * float(a.h) - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx = fx - x0f, wy = fy - y0f;
    const int   x0 = int(x0f), y0 = int(y0f);
    const int   xa = clampi(x0, 0, a.w - 1), xb = clampi(x0 + 1, 0, a.w - 1), ya = clampi(y0, 0, a.h - 1), yb = clampi(y0 + 1, 0, a.h - 1);
    const unsigned char* p = a.data + size_t(s) * a.slicePitch;
    const float t00 = *(const MIFX_GLOBAL float*)(p + size_t(ya) * a.pitch + size_t(xa) * 4u), t10 = *(const MIFX_GLOBAL float*)(p + size_t(ya) * a.pitch + size_t(xb) * 4u);
    const float t01 = *(const MIFX_GLOBAL float*)(p + size_t(yb) * a.pitch + size_t(xa) * 4u), t11 = *(const MIFX_GLOBAL float*)(p + size_t(yb) * a.pitch + size_t(xb) * 4u);
    float acc = 0.0f;
    acc = acc + (ref < t00 ? 1.0f : 0.0f) * ((1.0f - wx) * (1.0f - wy));
    acc = acc + (ref < t10 ? 1.0f : 0.0f) * (wx * (1.0f - wy));
    acc = acc + (ref < t01 ? 1.0f : 0.0f) * ((1.0f - wx) * wy);
    acc = acc + (ref < t11 ? 1.0f : 0.0f) * (wx * wy);
    return acc;
}
// SampleGrad of the filterable array (one mip): bilinear, clamped, the slice rounded to nearest
template <int CH> MIFX_D void shadow_sample_filterable(const FilterableArrK& a, float u, float v, int slice, float (&out)[CH])
{
#pragma clang fp contract(off)
    const int   s  = clampi(slice, 0, a.slices - 1);
    const float fx = u * float(a.w) - 0.5f, fy = v * float(a.h) - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float wx = fx - x0f, wy = fy - y0f;
    const int   x0 = int(x0f), y0 = int(y0f);
    const int   xa = clampi(x0, 0, a.w - 1), xb = clampi(x0 + 1, 0, a.w - 1), ya = clampi(y0, 0, a.h - 1), yb = clampi(y0 + 1, 0, a.h - 1);
    float t00[CH], t10[CH], t01[CH], t11[CH];
    ld_moments<CH>(a, s, xa, ya, t00); ld_moments<CH>(a, s, xb, ya, t10); ld_moments<CH>(a, s, xa, yb, t01); ld_moments<CH>(a, s, xb, yb, t11);
    const float w00 = (1.0f - wx) * (1.0f - wy), w10 = wx * (1.0f - wy), w01 = (1.0f - wx) * wy, w11 = wx * wy;
#pragma unroll
    for (int c = 0; c < CH; ++c)
    {
        float acc = 0.0f;
        acc = acc + t00[c] * w00;
        acc = acc + t10[c] * w10;
        acc = acc + t01[c] * w01;
        acc = acc + t11[c] * w11;
        out[c] = acc;
    }
}

// FilterShadowMapFixedPCF (PCF.fxh:7-153) with the receiver-plane depth bias
MIFX_D float shadow_fixed_pcf(const ShadowArrK& map, const float* dim, int size, v2 f2UV, int slice, float depth, v2 bias)
{
#pragma clang fp contract(off)
    const float DepthClamp = 1e-8f;
    if (size == 2) return shadow_sample_cmp(map, f2UV.x, f2UV.y, slice, fmaxf(depth, DepthClamp));
    const float uvx = f2UV.x * dim[0], uvy = f2UV.y * dim[1];
    float bx = floorf(uvx + 0.5f), by = floorf(uvy + 0.5f);
    const float s = uvx + 0.5f - bx, t = uvy + 0.5f - by;
    bx = (bx - 0.5f) * dim[2];
    by = (by - 0.5f) * dim[3];
    auto S = [&](float u, float v) { return shadow_sample_cmp(map, bx + u * dim[2], by + v * dim[3], slice, fmaxf(depth + (u * bias.x + v * bias.y), DepthClamp)); };
    float sum = 0.0f;
    if (size == 3)
    {
        const float uw0 = 3.0f - 2.0f * s, uw1 = 1.0f + 2.0f * s, u0 = (2.0f - s) / uw0 - 1.0f, u1 = s / uw1 + 1.0f;
        const float vw0 = 3.0f - 2.0f * t, vw1 = 1.0f + 2.0f * t, v0 = (2.0f - t) / vw0 - 1.0f, v1 = t / vw1 + 1.0f;
        sum = sum + uw0 * vw0 * S(u0, v0);
        sum = sum + uw1 * vw0 * S(u1, v0);
        sum = sum + uw0 * vw1 * S(u0, v1);
        sum = sum + uw1 * vw1 * S(u1, v1);
        return sum * 1.0f / 16.0f;
    }
    if (size == 5)
    {
        const float uw[3] = {4.0f - 3.0f * s, 7.0f, 1.0f + 3.0f * s}, vw[3] = {4.0f - 3.0f * t, 7.0f, 1.0f + 3.0f * t};
        const float u[3] = {(3.0f - 2.0f * s) / uw[0] - 2.0f, (3.0f + s) / uw[1], s / uw[2] + 2.0f};
        const float v[3] = {(3.0f - 2.0f * t) / vw[0] - 2.0f, (3.0f + t) / vw[1], t / vw[2] + 2.0f};
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < 3; ++i) sum = sum + uw[i] * vw[j] * S(u[i], v[j]);
        return sum * 1.0f / 144.0f;
    }
    if (size == 7)
    {
        const float uw[4] = {5.0f * s - 6.0f, 11.0f * s - 28.0f, -(11.0f * s + 17.0f), -(5.0f * s + 1.0f)};
        const float vw[4] = {5.0f * t - 6.0f, 11.0f * t - 28.0f, -(11.0f * t + 17.0f), -(5.0f * t + 1.0f)};
        const float u[4] = {(4.0f * s - 5.0f) / uw[0] - 3.0f, (4.0f * s - 16.0f) / uw[1] - 1.0f, -(7.0f * s + 5.0f) / uw[2] + 1.0f, -s / uw[3] + 3.0f};
        const float v[4] = {(4.0f * t - 5.0f) / vw[0] - 3.0f, (4.0f * t - 16.0f) / vw[1] - 1.0f, -(7.0f * t + 5.0f) / vw[2] + 1.0f, -t / vw[3] + 3.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) sum = sum + uw[i] * vw[j] * S(u[i], v[j]);
        return sum * 1.0f / 2704.0f;
    }
    return 0.0f;
}
// FilterShadowMapVaryingPCF (PCF.fxh:157-228)
MIFX_D float shadow_varying_pcf(const ShadowArrK& map, const float* dim, v2 f2UV, int slice, float depth, v2 bias, v2 filterSize)
{
#pragma clang fp contract(off)
    const float fsx = fmaxf(filterSize.x * dim[0], 1.0f), fsy = fmaxf(filterSize.y * dim[1], 1.0f);
    const float cx = f2UV.x * dim[0], cy = f2UV.y * dim[1];
    const float minx = clampf(cx - fsx / 2.0f, 0.0f, dim[0]), miny = clampf(cy - fsy / 2.0f, 0.0f, dim[1]);
    const float maxx = clampf(cx + fsx / 2.0f, 0.0f, dim[0]), maxy = clampf(cy + fsy / 2.0f, 0.0f, dim[1]);
    const int   sx = int(floorf(minx)), sy = int(floorf(miny)), ex = int(ceilf(maxx)), ey = int(ceilf(maxy));
    float TotalWeight = 0.0f, Sum = 0.0f;
    for (int x = sx; x < ex; x += 2)
    {
        const float U0    = float(x) + 0.5f;
        const float Left  = fmaxf(fminf(U0 + 0.5f, maxx) - fmaxf(U0 - 0.5f, minx), 0.0f);
        const float Right = fmaxf(fminf(U0 + 1.5f, maxx) - fmaxf(U0 + 0.5f, minx), 0.0f);
        const float dU    = Right / fmaxf(Right + Left, 1e-6f);
        const float HorzWeight = Right + Left;
        for (int y = sy; y < ey; y += 2)
        {
            const float V0     = float(y) + 0.5f;
            const float Bottom = fmaxf(fminf(V0 + 0.5f, maxy) - fmaxf(V0 - 0.5f, miny), 0.0f);
            const float Top    = fmaxf(fminf(V0 + 1.5f, maxy) - fmaxf(V0 + 0.5f, miny), 0.0f);
            const float dV     = Top / fmaxf(Bottom + Top, 1e-6f);
            const float VertWeight = Bottom + Top;
            const float u = U0 + dU, v = V0 + dV;
            const float Weight = HorzWeight * VertWeight;
            const float fDepth = fmaxf(depth + ((u - cx) * bias.x + (v - cy) * bias.y), 1e-8f);
            Sum = Sum + shadow_sample_cmp(map, u * dim[2], v * dim[3], slice, fDepth) * Weight;
            TotalWeight = TotalWeight + Weight;
        }
    }
    return TotalWeight > 0.0f ? Sum / TotalWeight : 1.0f;
}
// FilterShadowCascade (Shadows.fxh:179-209); F3NDC_XYZ_TO_UVD_SCALE = (0.5, -0.5, 1)
MIFX_D float shadow_filter_cascade_pcf(const ShadowLookupK& k, const ShadowArrK& map, v3 ddxPos, v3 ddyPos, CascadeSamplingInfo si)
{
#pragma clang fp contract(off)
    const v3 DX{ddxPos.x * si.scale.x * 0.5f, ddxPos.y * si.scale.y * -0.5f, ddxPos.z * si.scale.z * 1.0f};
    const v3 DY{ddyPos.x * si.scale.x * 0.5f, ddyPos.y * si.scale.y * -0.5f, ddyPos.z * si.scale.z * 1.0f};
    // ComputeReceiverPlaneDepthBias (:148-175)
    float bx = DY.y * DX.z - DX.y * DY.z;
    float by = -DY.x * DX.z + DX.x * DY.z;
    const float Det = (DX.x * DY.y) - (DX.y * DY.x);
    const float div = signf(Det) * fmaxf(fabsf(Det), 1e-10f);
    bx = bx / div;
    by = by / div;
    const float cx = fabsf((si.scale.z * 1.0f) / (si.scale.x * 0.5f)) * k.biasClamp, cy = fabsf((si.scale.z * 1.0f) / (si.scale.y * -0.5f)) * k.biasClamp;
    bx = fminf(fmaxf(bx, -cx), cx) * k.dim[2];
    by = fminf(fmaxf(by, -cy), cy) * k.dim[3];
    const float FractionalSamplingError = (1.0f * fabsf(bx) + 1.0f * fabsf(by)) + k.fixedBias;
    si.depth = si.depth - FractionalSamplingError;
    if (k.fixedFilterSize > 0) return shadow_fixed_pcf(map, k.dim, k.fixedFilterSize, si.uv, si.idx, si.depth, v2{bx, by});
    const v2 filterSize{fabsf(k.filterWorldSize * si.scale.x * 0.5f), fabsf(k.filterWorldSize * si.scale.y * -0.5f)};
    return shadow_varying_pcf(map, k.dim, si.uv, si.idx, si.depth, v2{bx, by}, filterSize);
}

// ChebyshevUpperBound with ReduceLightBleeding (Shadows.fxh:259-278)
MIFX_D float shadow_chebyshev(float m1, float m2, float mean, float minVariance, float lbr)
{
#pragma clang fp contract(off)
    float Variance = m2 - (m1 * m1);
    Variance = fmaxf(Variance, minVariance);
    const float d = mean - m1;
    float pMax = Variance / (Variance + (d * d));
    pMax = saturate((pMax - lbr) / (1.0f - lbr));
    return mean <= m1 ? 1.0f : pMax;
}
// SampleFilterableShadowCascade: SampleVSM (MODE 2) / SampleEVSM (MODE 3, 4)
template <int MODE> MIFX_D float shadow_sample_filterable_cascade(const ShadowLookupK& k, const FilterableArrK& map, const CascadeSamplingInfo& si)
{
#pragma clang fp contract(off)
    constexpr int CH = MODE == MIFX_SHADOW_MODE_EVSM4 ? 4 : 2;
    float occ[CH];
    if (MODE == MIFX_SHADOW_MODE_VSM)
    {
        shadow_sample_filterable<CH>(map, si.uv.x, si.uv.y, si.idx, occ);
        return shadow_chebyshev(occ[0], occ[1], si.depth, k.vsmBias, k.lightBleedingReduction);
    }
    const v2 warped = shadow_warp_evsm(si.depth, k.expPos, k.expNeg);
    shadow_sample_filterable<CH>(map, si.uv.x, si.uv.y, si.idx, occ);
    const float dsx = k.vsmBias * k.expPos * warped.x, dsy = k.vsmBias * k.expNeg * warped.y;
    float c = shadow_chebyshev(occ[0], occ[1], warped.x, dsx * dsx, k.lightBleedingReduction);
    if (MODE == MIFX_SHADOW_MODE_EVSM4) c = fminf(c, shadow_chebyshev(occ[CH - 2], occ[CH - 1], warped.y, dsy * dsy, k.lightBleedingReduction));
    return c;
}

struct FilteredShadow
{
    float lightAmount;
    float cascadeIdx; // float(iCascadeIdx)
    float nextCascadeBlendAmount;
};
// FilterShadowMap / SampleFilterableShadowMap at the pixel (x, y) of the frame `depth`.  cascades: ShadowLookupK::cascades where a per-pixel index is cheap to apply
// (LDS in the kernel).  The map that MODE does not read is not touched.
template <int MODE, bool BEST, bool ACROSS> MIFX_D FilteredShadow shadow_filter_at(int x, int y, const Img& depth, const ShadowLookupK& k, const mifx_cascade_attribs* cascades,
                                                                                   const ShadowArrK& map, const FilterableArrK& filterable)
{
#pragma clang fp contract(off)
    const float d = ld<float>(depth, x, y);
    FilteredShadow r{1.0f, float(k.numCascades), 0.0f};
    if (d == k.farDepth) return r; // background
    const v3 pos = shadow_pos_in_light_view(x, y, depth.w, depth.h, d, k);
    v3 ddxPos{0.0f, 0.0f, 0.0f}, ddyPos{0.0f, 0.0f, 0.0f};
    if (MODE == MIFX_SHADOW_MODE_PCF)
    {
        const int xp = (x ^ 1) < depth.w ? (x ^ 1) : x, yp = (y ^ 1) < depth.h ? (y ^ 1) : y;
        const v3  ph = shadow_pos_in_light_view(xp, y, depth.w, depth.h, ld<float>(depth, xp, y), k);
        const v3  pv = shadow_pos_in_light_view(x, yp, depth.w, depth.h, ld<float>(depth, x, yp), k);
        ddxPos = (x & 1) ? v3{pos.x - ph.x, pos.y - ph.y, pos.z - ph.z} : v3{ph.x - pos.x, ph.y - pos.y, ph.z - pos.z};
        ddyPos = (y & 1) ? v3{pos.x - pv.x, pos.y - pv.y, pos.z - pv.z} : v3{pv.x - pos.x, pv.y - pos.y, pv.z - pos.z};
    }
    const float camZ = shadow_camera_z(d, k);
    const CascadeSamplingInfo si = shadow_find_cascade<BEST>(k, cascades, pos, camZ);
    if (si.idx >= k.numCascades) return r;
    r.cascadeIdx = float(si.idx);
    auto filter = [&](const CascadeSamplingInfo& s) {
        if (MODE == MIFX_SHADOW_MODE_PCF) return shadow_filter_cascade_pcf(k, map, ddxPos, ddyPos, s);
        return shadow_sample_filterable_cascade<MODE == MIFX_SHADOW_MODE_PCF ? MIFX_SHADOW_MODE_VSM : MODE>(k, filterable, s);
    };
    r.lightAmount = filter(si);
    if (ACROSS && si.idx + 1 < k.numCascades)
    {
        const CascadeSamplingInfo next = shadow_cascade_sampling_info(cascades, pos, si.idx + 1);
        r.nextCascadeBlendAmount = shadow_next_cascade_blend<BEST>(k, cascades, camZ, si, next);
        float nextShadow = 1.0f;
        if (r.nextCascadeBlendAmount > 0.0f) nextShadow = filter(next);
        r.lightAmount = r.lightAmount + r.nextCascadeBlendAmount * (nextShadow - r.lightAmount); // lerp
    }
    return r;
}

} // namespace mifx
