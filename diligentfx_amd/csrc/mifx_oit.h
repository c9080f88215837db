// mifx_oit.h -- layered order-independent transparency, per pixel: the bodies of the kernels of oit.hip (Shaders/Common/public/OIT.fxh: PackOITLayer :1,
// GetOITLayerDepth :10, GetOITLayerTransmittance :15, GetOITLayerDataOffset :20, OIT_OPACITY_THRESHOLD :26; Shaders/PBR/private/OIT/ClearOITLayers.csh;
// UpdateOITLayers.psh:54-109 with the blend state BS_UpdateOITTail, PBR/src/PBR_Renderer.cpp:1849-1865; ApplyOITAttenuation.psh with BS_OITAttenuation,
// PBR_Renderer.cpp:2309-2324; GetOITTransmittance, Shaders/PBR/private/RenderPBR.psh:388-418, the transparent colour pass :544-559, :632, the USD footer
// PBR/src/USD_Renderer.cpp:122-167 and its blend state PBR_Renderer.cpp:2096-2127), in a header so that the test suite can also compile it for the host
// (tests/host_kernels/oit_host.cpp).
//
// Arithmetic.  Strict fp32 in the reference's operation order: no contraction, IEEE division (plain `/`).  A blend is dst = src * sf + dst * df, evaluated in that
// order with the factors the blend state names, also where a factor is 0 or 1.  The slice planes and the four targets are the build's 4-channel texel
// (GlobalAccess<v4>: float4, or RGBA16_FLOAT in the native-storage build, where a store rounds to binary16 as the reference's targets do); depth, colour alpha,
// the opaque depth and the tail are fp32 and the layers uint32 in both builds.
//
// The bodies take the pixel's K layer words through a pointer type: the words in HBM (the reference sequence: one launch per draw, as the reference's shaders) or
// a register array of compile-time size (the fused kernels, whose loops over the layers unroll).  Both run the same functions in the same order, so their results
// are the same bits.  The reference's InterlockedMin loop is a serial compare-and-swap chain here: a slice has at most one fragment per pixel and slices are
// applied in submission order, so no two invocations ever meet on a pixel's words.
#pragma once
#include <cmath>
#include "mifx.h"
#include "mifx_device.h"

namespace mifx
{
constexpr uint32_t kOitEmpty = 0xFFFFFFFFu;
constexpr float    kOitOpacityThreshold = 1.0f / 255.0f; // OIT_OPACITY_THRESHOLD, OIT.fxh:26

typedef uint32_t mifx_u2 __attribute__((ext_vector_type(2)));
typedef uint32_t mifx_u4 __attribute__((ext_vector_type(4)));

// S = +-1 of UpdateOITLayers.psh:57 and the reversed-depth test of :64 (RenderPBR.psh:552), from CameraAttribs::fNearPlaneDepth / fFarPlaneDepth
struct OitCamK
{
    float S;
    int   reversed;
};
inline OitCamK make_oitcamk(const mifx_camera_attribs& c) { return OitCamK{c.fNearPlaneDepth < c.fFarPlaneDepth ? 1.0f : -1.0f, c.fNearPlaneDepth > c.fFarPlaneDepth ? 1 : 0}; }

// one transparent draw (mifx_oit_slice): six planes of the frame's size; alpha may be null
struct OitSliceK
{
    const unsigned char *depth, *base, *material, *radiance, *ibl, *alpha;
    int pitchDepth, pitchBase, pitchMaterial, pitchRadiance, pitchIbl, pitchAlpha;
};
// The slice table of the fused kernels, a kernel argument: the loop index is wave-uniform, so a member is a scalar load from the kernarg segment (what is slow is a
// VGPR-indexed table: shadows.hip).  72 bytes a slice.
struct OitSlicesK
{
    OitSliceK s[MIFX_OIT_MAX_SLICES];
    int       count;
};
// the object's own buffers, the optional opaque depth and the camera
struct OitK
{
    unsigned char*       layers; // K words a pixel, pixel (x, y) at (y * w + x) * K: GetOITLayerDataOffset
    unsigned char*       tail;   // two floats a pixel: x = the count in steps of 1 / 255, y = the transmittance product
    const unsigned char* opaque; // F32 or null
    int                  w, h, K, tailPitch, opaquePitch;
    OitCamK              cam;
};
struct OitTargetsK
{
    Img color, base, material, ibl;
};

// ------------------------------------------------------------------------------------------------ OIT.fxh
MIFX_HD float oit_clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
MIFX_HD uint32_t oit_pack(float depth, float transmittance) // PackOITLayer
{
    const uint32_t D = uint32_t(oit_clamp01(depth) * 16777215.0f);
    const uint32_t T = uint32_t(oit_clamp01(transmittance) * 255.0f);
    return (D << 8u) | T;
}
MIFX_HD uint32_t oit_layer_depth(uint32_t layer) { return layer >> 8u; }
MIFX_HD float    oit_layer_transmittance(uint32_t layer) { return float(layer & 0xFFu) / 255.0f; }
MIFX_HD float    oit_blend(float src, float sf, float dst, float df) { return src * sf + dst * df; }

// Does the slice have a fragment at this pixel that passes the depth test?  Coverage: the shade's own background test (is_background, mifx_device.h: what
// mifx_pbr_shade_execute writes `background` for).  Depth test: UpdateOITLayers.psh:57-62, which the colour pass shares (the hardware's test there).
MIFX_HD bool oit_has_fragment(float depth, bool hasOpaque, float opaque, const OitCamK& cam)
{
    if (is_background(depth, cam.reversed != 0)) return false;
    return !(hasOpaque && depth * cam.S >= opaque * cam.S);
}
MIFX_HD float oit_fragment_depth(float depth, const OitCamK& cam) { return cam.reversed ? 1.0f - depth : depth; } // UpdateOITLayers.psh:64-67, RenderPBR.psh:552-555

// ------------------------------------------------------------------------------------------------ the K layers and the tail
// UpdateOITLayers.psh:71-107 and BS_UpdateOITTail (rgb One / One, alpha Zero / SrcAlpha) for one fragment of depth D (reversal applied) and opacity A
template <class P> MIFX_HD void oit_insert(P L, int K, v2& tail, float D, float A)
{
    uint32_t layer = kOitEmpty;
    if (A > kOitOpacityThreshold)
    {
        layer = oit_pack(D, 1.0f - A);
        for (int i = 0; i < K; ++i)
        {
            const uint32_t orig = L[i];
            L[i] = orig < layer ? orig : layer;          // InterlockedMin
            if (orig == kOitEmpty || orig == layer)      // empty space, or the layer matches another one exactly: the tail is not touched
            {
                layer = kOitEmpty;
                break;
            }
            layer = layer > orig ? layer : orig;         // what fell out goes on
        }
    }
    float srcR = 0.0f, srcA = 1.0f;
    if (layer != kOitEmpty)
    {
        srcR = 1.0f / 255.0f;
        srcA = oit_layer_transmittance(layer);
    }
    tail.x = oit_blend(srcR, 1.0f, tail.x, 1.0f);
    tail.y = oit_blend(srcA, 0.0f, tail.y, srcA);
}

// ApplyOITAttenuation.psh:27-45
template <class P> MIFX_HD float oit_total_transmittance(P L, int K, v2 tail)
{
    float T = 1.0f;
    int   layer = 0;
    for (; layer < K; ++layer)
    {
        const uint32_t dt = L[layer];
        if (dt == kOitEmpty) break;
        T *= oit_layer_transmittance(dt);
    }
    if (layer == K) T *= tail.y;
    return T;
}

// GetOITTransmittance, RenderPBR.psh:389-418
template <class P> MIFX_HD float oit_transmittance_at(P L, int K, v2 tail, float depth)
{
    const uint32_t D = uint32_t(depth * 16777215.0f);
    float          T = 1.0f;
    int            layer = 0;
    for (; layer < K; ++layer)
    {
        const uint32_t dt = L[layer];
        if (D <= oit_layer_depth(dt) + 1u) break; // "+1u helps to avoid precision issues"
        T *= oit_layer_transmittance(dt);
    }
    if (layer == K) T /= fmaxf(255.0f * tail.x, 1.0f); // the average contribution of all tail layers
    return T;
}

// ------------------------------------------------------------------------------------------------ the four targets
// BS_OITAttenuation on one target: the source is (0, 0, 0, T), every channel Zero / SrcAlpha
MIFX_HD void oit_attenuate(v4& dst, float T)
{
    dst.x = oit_blend(0.0f, 0.0f, dst.x, T);
    dst.y = oit_blend(0.0f, 0.0f, dst.y, T);
    dst.z = oit_blend(0.0f, 0.0f, dst.z, T);
    dst.w = oit_blend(T, 0.0f, dst.w, T);
}
// the transparent pass' blend state with OITLayerCount > 0: rgb One / One, alpha One / InvSrcAlpha
MIFX_HD void oit_blend_target(v4& dst, v4 src)
{
    dst.x = oit_blend(src.x, 1.0f, dst.x, 1.0f);
    dst.y = oit_blend(src.y, 1.0f, dst.y, 1.0f);
    dst.z = oit_blend(src.z, 1.0f, dst.z, 1.0f);
    dst.w = oit_blend(src.w, 1.0f, dst.w, 1.0f - src.w);
}
struct OitFragment
{
    v4    base, material, radiance, ibl;
    float colorAlpha; // OutColor.a
};
// RenderPBR.psh:547 and :632, the USD footer (USD_Renderer.cpp:122-124, :157-167) and the blend of the four outputs, for the transmittance T in front of the fragment
MIFX_HD void oit_blend_fragment(const OitFragment& f, float T, v4& color, v4& base, v4& material, v4& ibl)
{
    const float a = f.base.w;
    v4 out{f.radiance.x * a, f.radiance.y * a, f.radiance.z * a, f.colorAlpha};
    out.x *= T; out.y *= T; out.z *= T;
    const float mx = f.material.x * T, my = f.material.y * T;
    const float ix = f.ibl.x * T, iy = f.ibl.y * T, iz = f.ibl.z * T;
    const float bx = f.base.x * T, by = f.base.y * T, bz = f.base.z * T;
    oit_blend_target(color, out);
    oit_blend_target(base, v4{bx * a, by * a, bz * a, a});
    oit_blend_target(material, v4{mx * a, my * a, 0.0f, a});
    oit_blend_target(ibl, v4{ix * a, iy * a, iz * a, a});
}

// ------------------------------------------------------------------------------------------------ memory
MIFX_D unsigned char* oit_layers_at(const OitK& k, int x, int y) { return k.layers + (size_t(y) * size_t(k.w) + size_t(x)) * size_t(k.K) * 4u; }
MIFX_D unsigned char* oit_tail_at(const OitK& k, int x, int y) { return k.tail + size_t(y) * k.tailPitch + size_t(x) * 8u; }
// the K words of a pixel with the widest access K allows: pixel (x, y) starts at a multiple of 4 K bytes
template <int K> MIFX_D void oit_load_layers(const unsigned char* p, uint32_t (&L)[K])
{
    if (K % 4 == 0)
        for (int i = 0; i < K / 4; ++i)
        {
            const mifx_u4 t = *(const MIFX_GLOBAL mifx_u4*)(p + 16 * i);
            L[4 * i] = t.x; L[4 * i + 1] = t.y; L[4 * i + 2] = t.z; L[4 * i + 3] = t.w;
        }
    else if (K % 2 == 0)
        for (int i = 0; i < K / 2; ++i)
        {
            const mifx_u2 t = *(const MIFX_GLOBAL mifx_u2*)(p + 8 * i);
            L[2 * i] = t.x; L[2 * i + 1] = t.y;
        }
    else
        for (int i = 0; i < K; ++i) L[i] = *(const MIFX_GLOBAL uint32_t*)(p + 4 * i);
}
template <int K> MIFX_D void oit_store_layers(unsigned char* p, const uint32_t (&L)[K])
{
    if (K % 4 == 0)
        for (int i = 0; i < K / 4; ++i) *(MIFX_GLOBAL mifx_u4*)(p + 16 * i) = mifx_u4{L[4 * i], L[4 * i + 1], L[4 * i + 2], L[4 * i + 3]};
    else if (K % 2 == 0)
        for (int i = 0; i < K / 2; ++i) *(MIFX_GLOBAL mifx_u2*)(p + 8 * i) = mifx_u2{L[2 * i], L[2 * i + 1]};
    else
        for (int i = 0; i < K; ++i) *(MIFX_GLOBAL uint32_t*)(p + 4 * i) = L[i];
}
MIFX_D float oit_slice_depth(const OitSliceK& s, int x, int y) { return GlobalAccess<float>::load(s.depth + size_t(y) * s.pitchDepth + size_t(x) * 4u); }
// base_color.a alone: the float at +12 of the 16-byte texel; native-storage build: the half at +6 of the 8-byte texel
MIFX_D float oit_slice_opacity(const OitSliceK& s, int x, int y)
{
    const unsigned char* p = s.base + size_t(y) * s.pitchBase + size_t(x) * kV4Bytes;
#ifdef MIFX_STORAGE_H4
    return float(*(const MIFX_GLOBAL _Float16*)(p + 6u));
#else
    return GlobalAccess<float>::load(p + 12u);
#endif
}
MIFX_D float oit_opaque_at(const OitK& k, int x, int y) { return k.opaque ? GlobalAccess<float>::load(k.opaque + size_t(y) * k.opaquePitch + size_t(x) * 4u) : 0.0f; }
MIFX_D bool  oit_fragment_at(const OitK& k, float depth, float opaque) { return oit_has_fragment(depth, k.opaque != nullptr, opaque, k.cam); }
MIFX_D OitFragment oit_load_fragment(const OitSliceK& s, int x, int y)
{
    OitFragment f;
    f.base       = GlobalAccess<v4>::load(s.base + size_t(y) * s.pitchBase + size_t(x) * kV4Bytes);
    f.material   = GlobalAccess<v4>::load(s.material + size_t(y) * s.pitchMaterial + size_t(x) * kV4Bytes);
    f.radiance   = GlobalAccess<v4>::load(s.radiance + size_t(y) * s.pitchRadiance + size_t(x) * kV4Bytes);
    f.ibl        = GlobalAccess<v4>::load(s.ibl + size_t(y) * s.pitchIbl + size_t(x) * kV4Bytes);
    f.colorAlpha = s.alpha ? GlobalAccess<float>::load(s.alpha + size_t(y) * s.pitchAlpha + size_t(x) * 4u) : f.base.w;
    return f;
}

// ------------------------------------------------------------------------------------------------ one pixel of each kernel
// oit_clear_kernel: ClearOITLayers.csh, and the tail's clear value (0, 0, 0, 1) of HnBeginOITPassTask.cpp:139-144
MIFX_D void oit_px_clear(const OitK& k, int x, int y)
{
    MIFX_GLOBAL uint32_t* L = (MIFX_GLOBAL uint32_t*)oit_layers_at(k, x, y);
    for (int i = 0; i < k.K; ++i) L[i] = kOitEmpty;
    GlobalAccess<v2>::store(oit_tail_at(k, x, y), v2{0.0f, 1.0f});
}
// oit_update_kernel: one draw of UpdateOITLayers.psh
MIFX_D void oit_px_update(const OitK& k, const OitSliceK& s, int x, int y)
{
    const float depth = oit_slice_depth(s, x, y);
    if (!oit_fragment_at(k, depth, oit_opaque_at(k, x, y))) return;
    v2 tail = GlobalAccess<v2>::load(oit_tail_at(k, x, y));
    oit_insert((MIFX_GLOBAL uint32_t*)oit_layers_at(k, x, y), k.K, tail, oit_fragment_depth(depth, k.cam), oit_slice_opacity(s, x, y));
    GlobalAccess<v2>::store(oit_tail_at(k, x, y), tail);
}
// oit_attenuate_kernel: ApplyOITAttenuation.psh; T == 1 discards
MIFX_D void oit_px_attenuate(const OitK& k, const OitTargetsK& t, int x, int y)
{
    const float T = oit_total_transmittance((const MIFX_GLOBAL uint32_t*)oit_layers_at(k, x, y), k.K, GlobalAccess<v2>::load(oit_tail_at(k, x, y)));
    if (T == 1.0f) return;
    v4 c = ld<v4>(t.color, x, y), b = ld<v4>(t.base, x, y), m = ld<v4>(t.material, x, y), i = ld<v4>(t.ibl, x, y);
    oit_attenuate(c, T); oit_attenuate(b, T); oit_attenuate(m, T); oit_attenuate(i, T);
    st<v4>(t.color, x, y, c); st<v4>(t.base, x, y, b); st<v4>(t.material, x, y, m); st<v4>(t.ibl, x, y, i);
}
// the colour pass of one fragment against layers read through L
template <class P> MIFX_D void oit_blend_slice(P L, int K, v2 tail, const OitK& k, const OitSliceK& s, float depth, int x, int y, v4& c, v4& b, v4& m, v4& i)
{
    const OitFragment f = oit_load_fragment(s, x, y);
    float T = 1.0f;
    if (f.base.w > kOitOpacityThreshold) T = oit_transmittance_at(L, K, tail, oit_fragment_depth(depth, k.cam)); // RenderPBR.psh:549-557
    oit_blend_fragment(f, T, c, b, m, i);
}
// oit_blend_kernel: one transparent draw of the colour pass
MIFX_D void oit_px_blend(const OitK& k, const OitSliceK& s, const OitTargetsK& t, int x, int y)
{
    const float depth = oit_slice_depth(s, x, y);
    if (!oit_fragment_at(k, depth, oit_opaque_at(k, x, y))) return;
    v4 c = ld<v4>(t.color, x, y), b = ld<v4>(t.base, x, y), m = ld<v4>(t.material, x, y), i = ld<v4>(t.ibl, x, y);
    oit_blend_slice((const MIFX_GLOBAL uint32_t*)oit_layers_at(k, x, y), k.K, GlobalAccess<v2>::load(oit_tail_at(k, x, y)), k, s, depth, x, y, c, b, m, i);
    st<v4>(t.color, x, y, c); st<v4>(t.base, x, y, b); st<v4>(t.material, x, y, m); st<v4>(t.ibl, x, y, i);
}
// oit_build_kernel<K>: the clear and every draw's update with the K words and the tail in registers; the layers buffer is written, never read
template <int K> MIFX_D void oit_px_build(const OitK& k, const OitSlicesK& tab, int x, int y)
{
    uint32_t L[K];
#pragma unroll
    for (int i = 0; i < K; ++i) L[i] = kOitEmpty;
    v2 tail{0.0f, 1.0f};
    const float opaque = oit_opaque_at(k, x, y);
    for (int l = 0; l < tab.count; ++l)
    {
        const OitSliceK& s     = tab.s[l];
        const float      depth = oit_slice_depth(s, x, y);
        if (oit_fragment_at(k, depth, opaque)) oit_insert(L, K, tail, oit_fragment_depth(depth, k.cam), oit_slice_opacity(s, x, y));
    }
    oit_store_layers<K>(oit_layers_at(k, x, y), L);
    GlobalAccess<v2>::store(oit_tail_at(k, x, y), tail);
}
// oit_resolve_kernel<K>: the attenuation and every draw's colour pass with the layers, the tail and the four texels in registers; a pixel that nothing touches is
// not stored
template <int K> MIFX_D void oit_px_resolve(const OitK& k, const OitSlicesK& tab, const OitTargetsK& t, int x, int y)
{
    uint32_t L[K];
    oit_load_layers<K>(oit_layers_at(k, x, y), L);
    const v2 tail = GlobalAccess<v2>::load(oit_tail_at(k, x, y));
    v4 c = ld<v4>(t.color, x, y), b = ld<v4>(t.base, x, y), m = ld<v4>(t.material, x, y), i = ld<v4>(t.ibl, x, y);
    const float T      = oit_total_transmittance(L, K, tail);
    const float opaque = oit_opaque_at(k, x, y);
    bool touched = T != 1.0f;
    // quantize_v4: what the sequence's store + load between two draws does to a target texel (native-storage build: binary16; fp32 build: the identity)
    if (touched)
    {
        oit_attenuate(c, T); oit_attenuate(b, T); oit_attenuate(m, T); oit_attenuate(i, T);
        c = quantize_v4(c); b = quantize_v4(b); m = quantize_v4(m); i = quantize_v4(i);
    }
    for (int l = 0; l < tab.count; ++l)
    {
        const OitSliceK& s     = tab.s[l];
        const float      depth = oit_slice_depth(s, x, y);
        if (!oit_fragment_at(k, depth, opaque)) continue;
        oit_blend_slice(L, K, tail, k, s, depth, x, y, c, b, m, i);
        c = quantize_v4(c); b = quantize_v4(b); m = quantize_v4(m); i = quantize_v4(i);
        touched = true;
    }
    if (!touched) return;
    st<v4>(t.color, x, y, c); st<v4>(t.base, x, y, b); st<v4>(t.material, x, y, m); st<v4>(t.ibl, x, y, i);
}
} // namespace mifx
