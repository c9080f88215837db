// mifx_material.h -- the material fetch: the head of the reference's forward pixel shader (`main` of Shaders/PBR/private/RenderPBR.psh:424-457 and the fetches of
// GetSurfaceShadingInfo :299-359) over interpolant planes, with the texture system it reads through written out in software: the per-pixel body of material_fetch_kernel
// (material.hip) and of tests/host_kernels/material_fetch_host.cpp.  What it restates, each with its line numbers below:
//   RenderPBR.psh:80-136 (GetDefaultTextureAttribs, GetNormalMapUVInfo), :138-184 (ReadBaseLayerProperties up to PerturbNormal; GetSurfaceReflectance stays in the shade),
//   :186-297 (the fetches of the layer readers, with the clear coat's PerturbNormal :203-216), PBR_Textures.fxh:346-932 (GetVolumeThickness excluded), AtlasSampling.fxh:64-184
//   (the CalculateLevelOfDetail branch), PBR_Shading.fxh:144-199 (GetPerturbNormalInfo, non-GL; PerturbNormal), ShaderUtilities.fxh:43-69, PBR_Structures.fxh:245-275.
// The two contracts the reference leaves to the graphics API -- quad derivatives and the sampler -- are those of include/mifx.h ("material fetch").
//
// Strict fp32 under the policy of the bodies that are held to the reference bit for bit: operations in the shader's order, libm log2 / exp2 / pow, no contraction.
// No address depends on an unclamped input: texel coordinates are wrapped integers (a NaN, infinite or huge coordinate falls on texel 0 with weight 0), slice and level are
// clamped, the material index is range-checked.  Material records and texture descriptors are read from memory by index; nothing here is a private array indexed at run time.
#pragma once
#include "mifx.h"
#include "mifx_device.h"

namespace mifx
{
struct MaterialTexK // a mifx_texture_array as the kernel reads it (104 bytes)
{
    const unsigned char* data;
    unsigned long long   slicePitch;
    int                  w, h, slices, mips;
    unsigned             rgba8; // 1: RGBA8_UNORM (one 4-byte load a texel), 0: RGBA32_FLOAT
    unsigned             pad;
    unsigned             levelOffset[16]; // first texel of level k within a slice
};
// the descriptor of a texture that has passed the checks of the entries (api_material.cpp: sizes, format, at most 15 levels): the levels of a slice lie one behind the other
inline MaterialTexK make_material_texk(const mifx_texture_array& t)
{
    MaterialTexK o{};
    o.data = static_cast<const unsigned char*>(t.data);
    o.slicePitch = t.slice_pitch_bytes;
    o.w = int(t.width); o.h = int(t.height); o.slices = int(t.slices); o.mips = int(t.mips);
    o.rgba8 = t.format == MIFX_NATIVE_FORMAT_RGBA8_UNORM ? 1u : 0u;
    unsigned texels = 0;
    for (uint32_t l = 0; l < t.mips; ++l)
    {
        o.levelOffset[l] = texels;
        texels += ((t.width >> l) > 1u ? (t.width >> l) : 1u) * ((t.height >> l) > 1u ? (t.height >> l) : 1u);
    }
    return o;
}
struct MaterialFetchK
{
    Img depth, uv0, uv1, meshNormal, color, face, index; // p == nullptr: the permutation without it
    Img outBaseColor, outNormal, outMaterial, outEmissive, outOcclusion;
    Img outClearcoat, outClearcoatNormal, outSheen, outAnisotropy, outIridescence, outTransmission;
    const mifx_pbr_material* materials;
    const MaterialTexK*      textures;
    int      materialCount, textureCount;
    unsigned layers, flags; // MIFX_PBR_LAYER_*, MIFX_MATERIAL_FETCH_FLAG_*
    float    mipBias, handness;
    int      workflow;
};
struct MaterialFetchOut
{
    v4    baseColor, normal, material, emissive;
    float occlusion;
    v4    clearcoat, clearcoatNormal, sheen, anisotropy, iridescence;
    float transmission;
};

// ------------------------------------------------------------------------------------------------ the sampler (include/mifx.h, contract 2)
struct MaterialTexRef
{
    const MaterialTexK*  t;
    const unsigned char* slice;
    int                  w, h, mips;
    bool                 rgba8;
};
MIFX_D MaterialTexRef mat_tex_open(const MaterialFetchK& k, int index, float fSlice)
{
    const MaterialTexK* t = k.textures + index;
    MaterialTexRef r;
    r.t = t; r.w = t->w; r.h = t->h; r.mips = t->mips; r.rgba8 = t->rgba8 != 0u;
    const float s = fminf(fmaxf(floorf(fSlice + 0.5f), 0.0f), float(t->slices - 1)); // rounded to nearest, clamped (NaN -> 0)
    r.slice = t->data + static_cast<unsigned long long>(int(s)) * t->slicePitch;
    return r;
}
MIFX_D v4 mat_texel(const MaterialTexRef& r, unsigned levelBase, int lw, int x, int y)
{
    const unsigned i = levelBase + unsigned(y) * unsigned(lw) + unsigned(x);
    if (r.rgba8)
    {
        const unsigned t = *(const MIFX_GLOBAL unsigned*)(r.slice + size_t(i) * 4u);
        // c / 255 correctly rounded: q = c * fl(1 / 255) and one residual step (mifx_formats.h: unorm_to_float)
        const float rc = 1.0f / 255.0f;
        const float c0 = float(t & 0xffu), c1 = float((t >> 8) & 0xffu), c2 = float((t >> 16) & 0xffu), c3 = float(t >> 24);
        const float q0 = c0 * rc, q1 = c1 * rc, q2 = c2 * rc, q3 = c3 * rc;
        return v4{__builtin_fmaf(__builtin_fmaf(-q0, 255.0f, c0), rc, q0), __builtin_fmaf(__builtin_fmaf(-q1, 255.0f, c1), rc, q1),
                  __builtin_fmaf(__builtin_fmaf(-q2, 255.0f, c2), rc, q2), __builtin_fmaf(__builtin_fmaf(-q3, 255.0f, c3), rc, q3)};
    }
    return GlobalAccess<v4>::load(r.slice + size_t(i) * 16u);
}
// floor(coordinate) as a texel of a row of n under WRAP; ok = false (NaN, infinite, beyond 2^30): texel 0, and the caller drops the fractional weight
MIFX_D int mat_wrap(float f, int n, bool& ok)
{
    ok = fabsf(f) < 1073741824.0f;
    int i = ok ? int(f) : 0;
    i %= n;
    return i < 0 ? i + n : i;
}
MIFX_D v4 mat_bilinear(const MaterialTexRef& r, int level, v2 uv)
{
    const int      lw = max(r.w >> level, 1), lh = max(r.h >> level, 1);
    const unsigned base = r.t->levelOffset[level];
    const float fx = uv.x * float(lw) - 0.5f, fy = uv.y * float(lh) - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    bool okx, oky;
    const int x0 = mat_wrap(x0f, lw, okx), y0 = mat_wrap(y0f, lh, oky);
    const int x1 = x0 + 1 == lw ? 0 : x0 + 1, y1 = y0 + 1 == lh ? 0 : y0 + 1;
    const float wx = okx ? fx - x0f : 0.0f, wy = oky ? fy - y0f : 0.0f;
    // GetBilinearSamplingInfoUC (ShaderUtilities.fxh:139-141)
    v4 acc = mat_texel(r, base, lw, x0, y0) * ((1.0f - wx) * (1.0f - wy));
    acc = acc + mat_texel(r, base, lw, x1, y0) * (wx * (1.0f - wy));
    acc = acc + mat_texel(r, base, lw, x0, y1) * ((1.0f - wx) * wy);
    acc = acc + mat_texel(r, base, lw, x1, y1) * (wx * wy);
    return acc;
}
MIFX_D float mat_clamp_lod(const MaterialTexRef& r, float lod) { return fminf(fmaxf(lod, 0.0f), float(r.mips - 1)); } // (NaN -> 0)
MIFX_D float mat_lod(const MaterialTexRef& r, v2 dx, v2 dy, float bias)
{
    const v2    dim{float(r.w), float(r.h)};
    const float rho = fmaxf(length(dx * dim), length(dy * dim));
    return mat_clamp_lod(r, log2f(rho) + bias);
}
MIFX_D v4 mat_sample_level(const MaterialTexRef& r, v2 uv, float lod) // SampleLevel
{
    lod = mat_clamp_lod(r, lod);
    const int   l0 = int(floorf(lod)), l1 = l0 + 1 < r.mips ? l0 + 1 : l0;
    const float f  = lod - float(l0);
    const v4    a  = mat_bilinear(r, l0, uv);
    if (f == 0.0f || l1 == l0) return a;
    const v4 b = mat_bilinear(r, l1, uv);
    return a + (b - a) * f;
}

// ------------------------------------------------------------------------------------------------ quad derivatives (include/mifx.h, contract 1)
// The three pixels a fine derivative needs: the pixel, its partner along x (x ^ 1) and along y (y ^ 1), clamped to the frame.
struct MaterialQuad
{
    int  x, y, xp, yp;
    bool right, bottom; // the pixel is the right / bottom one of its pair
};
MIFX_D MaterialQuad mat_quad(int x, int y, int w, int h)
{
    MaterialQuad q;
    q.x = x; q.y = y;
    q.xp = min(x ^ 1, w - 1); q.yp = min(y ^ 1, h - 1);
    q.right = (x & 1) != 0; q.bottom = (y & 1) != 0;
    return q;
}
MIFX_D float mat_ddx(const MaterialQuad& q, float self, float px) { return q.right ? self - px : px - self; }
MIFX_D float mat_ddy(const MaterialQuad& q, float self, float py) { return q.bottom ? self - py : py - self; }
MIFX_D v2 mat_ddx(const MaterialQuad& q, v2 s, v2 p) { return v2{mat_ddx(q, s.x, p.x), mat_ddx(q, s.y, p.y)}; }
MIFX_D v2 mat_ddy(const MaterialQuad& q, v2 s, v2 p) { return v2{mat_ddy(q, s.x, p.x), mat_ddy(q, s.y, p.y)}; }
MIFX_D v3 mat_ddx(const MaterialQuad& q, v3 s, v3 p) { return v3{mat_ddx(q, s.x, p.x), mat_ddx(q, s.y, p.y), mat_ddx(q, s.z, p.z)}; }
MIFX_D v3 mat_ddy(const MaterialQuad& q, v3 s, v3 p) { return v3{mat_ddy(q, s.x, p.x), mat_ddy(q, s.y, p.y), mat_ddy(q, s.z, p.z)}; }

struct MaterialUVs { v2 uv0, uv1; }; // VSOut.UV0 / UV1 of one pixel
MIFX_D MaterialUVs mat_load_uvs(const MaterialFetchK& k, int x, int y)
{
    MaterialUVs r;
    r.uv0 = k.uv0.p ? ld<v2>(k.uv0, x, y) : v2{0.0f, 0.0f};
    r.uv1 = k.uv1.p ? ld<v2>(k.uv1, x, y) : v2{0.0f, 0.0f};
    return r;
}
struct MaterialQuadUVs { MaterialUVs s, px, py; };

// PBR_Structures.fxh:259-275
MIFX_D float    mat_uv_selector(unsigned packed) { return float(packed & 7u) - 1.0f; }
MIFX_D unsigned mat_wrap_u(unsigned packed) { return ((packed >> 3u) & 7u) + 1u; }
MIFX_D unsigned mat_wrap_v(unsigned packed) { return ((packed >> 6u) & 7u) + 1u; }
constexpr unsigned kWrapModeClamp = 3u; // TEXTURE_ADDRESS_CLAMP

struct MaterialTexAttribs // PBRMaterialTextureAttribs in registers
{
    unsigned packed;
    float    slice, uBias, vBias;
    v4       scaleRot, atlas;
};
MIFX_D MaterialTexAttribs mat_attribs(const mifx_pbr_material* m, int slot)
{
    const mifx_pbr_texture_attribs* a = m->textures + slot;
    return MaterialTexAttribs{a->PackedProps, a->TextureSlice, a->UBias, a->VBias,
                              v4{a->UVScaleAndRotation[0], a->UVScaleAndRotation[1], a->UVScaleAndRotation[2], a->UVScaleAndRotation[3]},
                              v4{a->AtlasUVScaleAndBias[0], a->AtlasUVScaleAndBias[1], a->AtlasUVScaleAndBias[2], a->AtlasUVScaleAndBias[3]}};
}
// GetDefaultTextureAttribs (RenderPBR.psh:80-92)
MIFX_D MaterialTexAttribs mat_default_attribs() { return MaterialTexAttribs{0u, 0.0f, 0.0f, 0.0f, v4{1.0f, 0.0f, 0.0f, 1.0f}, v4{1.0f, 1.0f, 0.0f, 0.0f}}; }

// SelectUV (PBR_Textures.fxh:346-357)
MIFX_D v2 mat_select_uv(const MaterialFetchK& k, const MaterialUVs& in, float selector)
{
    if (k.uv0.p && k.uv1.p) return in.uv0 + selector * (in.uv1 - in.uv0); // lerp(UV0, UV1, Selector)
    if (k.uv0.p) return in.uv0;
    if (k.uv1.p) return in.uv1;
    return v2{0.0f, 0.0f};
}
// TransformUV (:359-362): mul(UV, MatrixFromRows(xy, zw)) + (UBias, VBias)
MIFX_D v2 mat_transform_uv(v2 uv, const MaterialTexAttribs& a)
{
    return v2{uv.x * a.scaleRot.x + uv.y * a.scaleRot.z + a.uBias, uv.x * a.scaleRot.y + uv.y * a.scaleRot.w + a.vBias};
}
// the texture coordinate of a map at one pixel: SelectUV and, with ENABLE_TEXCOORD_TRANSFORM, TransformUV (:380-385, RenderPBR.psh:108-112)
MIFX_D v2 mat_map_uv(const MaterialFetchK& k, const MaterialUVs& in, const MaterialTexAttribs& a)
{
    v2 uv = mat_select_uv(k, in, mat_uv_selector(a.packed));
    if (k.flags & MIFX_MATERIAL_FETCH_FLAG_TEXCOORD_TRANSFORM) uv = mat_transform_uv(uv, a);
    return uv;
}
// the clamp of the non-atlas path (:412-420, :498-506)
MIFX_D v2 mat_clamp_uv(v2 uv, const MaterialTexAttribs& a, const MaterialTexRef& r)
{
    const unsigned wu = mat_wrap_u(a.packed), wv = mat_wrap_v(a.packed);
    if (wu == kWrapModeClamp || wv == kWrapModeClamp)
    {
        const v2 dim{float(r.w), float(r.h)};
        uv.x = wu == kWrapModeClamp ? clampf(uv.x, fdiv(0.5f, dim.x), 1.0f - fdiv(0.5f, dim.x)) : uv.x;
        uv.y = wv == kWrapModeClamp ? clampf(uv.y, fdiv(0.5f, dim.y), 1.0f - fdiv(0.5f, dim.y)) : uv.y;
    }
    return uv;
}
// the wrap of the atlas path (:390-391, RenderPBR.psh:125-126)
MIFX_D v2 mat_wrap_atlas_uv(v2 uv, const MaterialTexAttribs& a)
{
    return v2{mat_wrap_u(a.packed) == kWrapModeClamp ? saturate(uv.x) : fracf(uv.x), mat_wrap_v(a.packed) == kWrapModeClamp ? saturate(uv.y) : fracf(uv.y)};
}

// SampleTextureAtlas (AtlasSampling.fxh:64-184), the branch with CalculateLevelOfDetail.  smooth / smoothPx / smoothPy: f2SmoothUV at the pixel and its two partners.
MIFX_D v4 mat_sample_atlas(const MaterialTexRef& r, const MaterialQuad& q, v2 f2UV, v2 smooth, v2 smoothPx, v2 smoothPy, v2 dSmoothDx, v2 dSmoothDy, v4 region)
{
    const v2 regionSize{fabsf(region.x), fabsf(region.y)};                                              // :70
    const v2 regionOrg{fminf(region.z, region.z + region.x), fminf(region.w, region.w + region.y)};     // :71
    v2 dUVdx = dSmoothDx, dUVdy = dSmoothDy;                                                            // :73-74
    const v2 dim{float(r.w), float(r.h)};                                                               // :76-78
    const float gradX = fmaxf(length(dUVdx * dim), 1e-5f), gradY = fmaxf(length(dUVdy * dim), 1e-5f);   // :81-82
    const float maxGrad = fmaxf(gradX, gradY);                                                          // :83
    float lod = mat_lod(r, mat_ddx(q, smooth, smoothPx), mat_ddy(q, smooth, smoothPy), 0.0f);           // :89
    lod = fmaxf(lod, 0.0f);                                                                             // :101
    const float e = exp2f(ceilf(lod));
    const v2 lodMargin{fdiv(0.5f, dim.x) * e, fdiv(0.5f, dim.y) * e};                                   // :105
    const v2 gradMargin{0.5f * (fabsf(dUVdx.x) + fabsf(dUVdy.x)), 0.5f * (fabsf(dUVdx.y) + fabsf(dUVdy.y))}; // :120
    v2 margin = lodMargin + gradMargin;                                                                 // :122
    margin = v2{fminf(margin.x, regionSize.x * 0.5f), fminf(margin.y, regionSize.y * 0.5f)};            // :124
    const v2 uv{clampf(f2UV.x, regionOrg.x + margin.x, regionOrg.x + regionSize.x - margin.x),
                clampf(f2UV.y, regionOrg.y + margin.y, regionOrg.y + regionSize.y - margin.y)};         // :127-129
    float minRegionDim = fminf(dim.x * regionSize.x, dim.y * regionSize.y);                             // :146
    minRegionDim = fmaxf(minRegionDim, 1.0f);                                                           // :148
    const float smallestValidLevelDim = fmaxf(4.0f, 2.0f);                                              // :154 (fSmallestValidLevelDim 4, PBR_Textures.fxh:402)
    const float maxGradLimit = fdiv(minRegionDim, smallestValidLevelDim);                               // :155
    const float fadeout = saturate(fdiv(maxGrad - maxGradLimit, maxGradLimit));                         // :158 (IsNonFilterable false)
    v4 color = mk4(0.0f);
    if (fadeout < 1.0f)                                                                                 // :161-168
    {
        const float gradScale = fminf(1.0f, fdiv(maxGradLimit, fmaxf(maxGrad, 1e-5f)));
        dUVdx = dUVdx * gradScale;
        dUVdy = dUVdy * gradScale;
        color = mat_sample_level(r, uv, mat_lod(r, dUVdx, dUVdy, 0.0f)); // SampleGrad
    }
    if (fadeout > 0.0f)                                                                                 // :170-181
    {
        const float lastValidLod = log2f(maxGradLimit);
        const v4 mean = (mat_sample_level(r, v2{regionOrg.x + 0.25f * regionSize.x, regionOrg.y + 0.25f * regionSize.y}, lastValidLod) +
                         mat_sample_level(r, v2{regionOrg.x + 0.75f * regionSize.x, regionOrg.y + 0.25f * regionSize.y}, lastValidLod) +
                         mat_sample_level(r, v2{regionOrg.x + 0.25f * regionSize.x, regionOrg.y + 0.75f * regionSize.y}, lastValidLod) +
                         mat_sample_level(r, v2{regionOrg.x + 0.75f * regionSize.x, regionOrg.y + 0.75f * regionSize.y}, lastValidLod)) *
                        0.25f;
        color = color + fadeout * (mean - color); // lerp
    }
    return color;
}

// SampleTexture (PBR_Textures.fxh:364-429) of the map in `slot`, which the material has (texture[slot] >= 0) and the frame has texture coordinates for.
template <bool ATLAS>
MIFX_D v4 mat_sample_texture(const MaterialFetchK& k, const mifx_pbr_material* m, int slot, int texIndex, const MaterialQuad& q, const MaterialQuadUVs& in, v4 defaultValue)
{
    const MaterialTexAttribs a = mat_attribs(m, slot);
    if (!(mat_uv_selector(a.packed) >= 0.0f)) return defaultValue;                                      // :378
    const MaterialTexRef r = mat_tex_open(k, texIndex, a.slice);
    const v2 uv = mat_map_uv(k, in.s, a), uvPx = mat_map_uv(k, in.px, a), uvPy = mat_map_uv(k, in.py, a); // :380-385, at the pixel and its quad partners
    if constexpr (ATLAS)
    {
        const v2    wrapped = mat_wrap_atlas_uv(uv, a);                                                 // :390-391
        const float g = exp2f(k.mipBias);                                                               // :393
        const v2    sc{a.atlas.x, a.atlas.y};
        const v2    f2UV = wrapped * sc + v2{a.atlas.z, a.atlas.w};                                     // :396
        const v2    smooth = uv * sc * g, smoothPx = uvPx * sc * g, smoothPy = uvPy * sc * g;           // :397
        const v2    dSdx = mat_ddx(q, uv, uvPx) * sc * g, dSdy = mat_ddy(q, uv, uvPy) * sc * g;         // :398-399
        return mat_sample_atlas(r, q, f2UV, smooth, smoothPx, smoothPy, dSdx, dSdy, a.atlas);           // :400-406
    }
    else
    {
        const v2 c = mat_clamp_uv(uv, a, r), cPx = mat_clamp_uv(uvPx, a, r), cPy = mat_clamp_uv(uvPy, a, r); // :412-420
        return mat_sample_level(r, c, mat_lod(r, mat_ddx(q, c, cPx), mat_ddy(q, c, cPy), k.mipBias));    // :421 SampleBias
    }
}

// NormalMapUVInfo (RenderPBR.psh:94-101) with what SampleNormalTexture's implicit derivatives need: the coordinate at the quad partners
struct MaterialNormalUV
{
    float selector;
    v2    uv, smoothUV, dUVdx, dUVdy;
    v2    uvPx, uvPy;         // UVInfo.UV at the partners (the non-atlas path differentiates it after the clamp)
    v2    smoothPx, smoothPy; // UVInfo.SmoothUV at the partners (the atlas path's CalculateLevelOfDetail)
};
// GetNormalMapUVInfo (RenderPBR.psh:103-136)
template <bool ATLAS> MIFX_D MaterialNormalUV mat_normal_uv_info(const MaterialFetchK& k, const MaterialQuad& q, const MaterialQuadUVs& in, const MaterialTexAttribs& a)
{
    MaterialNormalUV n;
    n.selector = mat_uv_selector(a.packed);                                                             // :107
    n.uv   = mat_map_uv(k, in.s, a);                                                                    // :108-112
    n.uvPx = mat_map_uv(k, in.px, a);
    n.uvPy = mat_map_uv(k, in.py, a);
    n.smoothUV = n.uv; n.smoothPx = n.uvPx; n.smoothPy = n.uvPy;                                        // :114
    n.dUVdx = mat_ddx(q, n.uv, n.uvPx);                                                                 // :115
    n.dUVdy = mat_ddy(q, n.uv, n.uvPy);                                                                 // :116
    if constexpr (ATLAS)                                                                                // :118-133
    {
        const v2 sc{a.atlas.x, a.atlas.y}, bias{a.atlas.z, a.atlas.w};
        n.uv   = mat_wrap_atlas_uv(n.uv, a) * sc + bias;
        n.uvPx = mat_wrap_atlas_uv(n.uvPx, a) * sc + bias;
        n.uvPy = mat_wrap_atlas_uv(n.uvPy, a) * sc + bias;
        n.smoothUV = n.smoothUV * sc; n.smoothPx = n.smoothPx * sc; n.smoothPy = n.smoothPy * sc;
        n.dUVdx = n.dUVdx * sc;
        n.dUVdy = n.dUVdy * sc;
    }
    return n;
}
// SampleNormalTexture (PBR_Textures.fxh:459-513)
template <bool ATLAS>
MIFX_D v3 mat_sample_normal_texture(const MaterialFetchK& k, const MaterialTexAttribs& a, int texIndex, const MaterialQuad& q, const MaterialNormalUV& n)
{
    v3 sampled{0.5f, 0.5f, 1.0f};
    if (mat_uv_selector(a.packed) >= 0.0f)                                                              // :470-471
    {
        const MaterialTexRef r = mat_tex_open(k, texIndex, a.slice);
        if constexpr (ATLAS)
        {
            const float g = exp2f(k.mipBias);                                                           // :475
            sampled = xyz(mat_sample_atlas(r, q, n.uv, n.smoothUV * g, n.smoothPx * g, n.smoothPy * g, n.dUVdx * g, n.dUVdy * g, a.atlas)); // :477-488
        }
        else
        {
            const v2 c = mat_clamp_uv(n.uv, a, r), cPx = mat_clamp_uv(n.uvPx, a, r), cPy = mat_clamp_uv(n.uvPy, a, r); // :492-506
            sampled = xyz(mat_sample_level(r, c, mat_lod(r, mat_ddx(q, c, cPx), mat_ddy(q, c, cPy), k.mipBias)));     // :507
        }
    }
    return sampled;
}
// the tail of GetMicroNormal / GetClearcoatNormal (:537-544, :717-724)
MIFX_D v3 mat_unpack_normal(v3 n, float scale)
{
    n = n * mk3(2.0f) - mk3(1.0f);
    n.x *= scale; n.y *= scale;
    if (n.z < 0.0f) n.z = fsqrt(fmaxf(1.0f - (n.x * n.x + n.y * n.y), 0.0f)); // the texture does not contain the Z component of the normal
    return n;
}

// PerturbNormalInfo (PBR_Shading.fxh:144-150)
struct MaterialNormalInfo
{
    v3    dPosDx, dPosDy, normal;
    float face;
};
// TransformTangentSpaceNormalGrad (ShaderUtilities.fxh:43-69)
MIFX_D v3 mat_tangent_space_normal(v3 dPosDx, v3 dPosDy, v2 dUVdx, v2 dUVdy, v3 macroNormal, v3 tsNormal)
{
    const float d = dUVdx.x * dUVdy.y - dUVdy.x * dUVdx.y;
    if (d != 0.0f)
    {
        const v3 n = macroNormal;
        v3 t = (dUVdy.y * dPosDx - dUVdx.y * dPosDy) / d;
        t = normalize(t - n * dot(n, t));
        const v3 b = normalize(cross(t, n));
        const v3 r = normalize(tsNormal.x * t + tsNormal.y * b + tsNormal.z * n); // mul(TSNormal, MatrixFromRows(t, b, n))
        // (the one deviation, include/mifx.h: a frame that degenerates to a non-finite normal -- non-finite or overflowing gradients -- leaves the macro normal)
        return (fabsf(r.x) <= 3.0e38f && fabsf(r.y) <= 3.0e38f && fabsf(r.z) <= 3.0e38f) ? r : macroNormal;
    }
    return macroNormal;
}
// PerturbNormal (PBR_Shading.fxh:184-199)
MIFX_D v3 mat_perturb_normal(const MaterialNormalInfo& info, v2 dUVdx, v2 dUVdy, v3 tsNormal, bool hasUV)
{
    if (hasUV)
    {
        tsNormal.x *= info.face; tsNormal.y *= info.face;
        return mat_tangent_space_normal(info.dPosDx, info.dPosDy, dUVdx, dUVdy, info.normal, tsNormal);
    }
    return info.normal;
}
MIFX_D v3 mat_to_linear(const MaterialFetchK& k, v3 c) // TO_LINEAR (PBR_Shading.fxh:21-25): FastSRGBToLinear (SRGBUtilities.fxh:17-20) or nothing
{
    return (k.flags & MIFX_MATERIAL_FETCH_FLAG_SRGB_TO_LINEAR) ? v3{powf(c.x, 2.2f), powf(c.y, 2.2f), powf(c.z, 2.2f)} : c;
}
MIFX_D v3 mat_world_pos(const MaterialFetchK& k, const CamK& cam, int x, int y) // VSOut.WorldPos: InvProjectPosition of the depth, as the shade reconstructs Shading.Pos
{
    return inv_project_position(v3{(float(x) + 0.5f) * cam.ivw, (float(y) + 0.5f) * cam.ivh, ld<float>(k.depth, x, y)}, cam.viewProjInv);
}

// One pixel of the material fetch.  Returns false for a pixel without a fragment (far-plane depth, or a material index outside the table): nothing is stored for it.
template <bool ATLAS> MIFX_D bool material_fetch_pixel(int x, int y, const MaterialFetchK& k, const CamK& cam, MaterialFetchOut& o)
{
    const float depth = ld<float>(k.depth, x, y);
    if (is_background(depth, cam.reversedDepth != 0)) return false;
    int index = 0;
    if (k.index.p)
    {
        const float f = ld<float>(k.index, x, y);
        if (!(f >= 0.0f && f < float(k.materialCount))) return false; // (NaN included)
        index = int(f);
    }
    const mifx_pbr_material* m = k.materials + index;
    const bool hasUV = k.uv0.p != nullptr || k.uv1.p != nullptr; // USE_TEXCOORD0 || USE_TEXCOORD1
    const MaterialQuad q = mat_quad(x, y, k.depth.w, k.depth.h);
    MaterialQuadUVs in;
    in.s = mat_load_uvs(k, q.x, q.y); in.px = mat_load_uvs(k, q.xp, q.y); in.py = mat_load_uvs(k, q.x, q.yp);
    const float mipBias = k.mipBias;
    (void)mipBias;

    // ---- GetBaseColor (PBR_Textures.fxh:431-457) with PRIMITIVE.FallbackColor (RenderPBR.psh:424)
    const v4 fallback{m->fallback_color[0], m->fallback_color[1], m->fallback_color[2], m->fallback_color[3]};
    v4 baseColor = fallback;
    {
        const int t = m->texture[MIFX_PBR_TEXTURE_BASE_COLOR];
        if (t >= 0)
        {
            baseColor = hasUV ? mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_BASE_COLOR, t, q, in, fallback) : fallback;
            baseColor = mk4(mat_to_linear(k, xyz(baseColor)), baseColor.w);                             // :446
        }
        if (k.color.p) baseColor = baseColor * ld<v4>(k.color, x, y);                                   // :450-454
        baseColor = baseColor * v4{m->basic.BaseColorFactor[0], m->basic.BaseColorFactor[1], m->basic.BaseColorFactor[2], m->basic.BaseColorFactor[3]}; // :456
    }
    o.baseColor = baseColor;

    // ---- GetPerturbNormalInfo (PBR_Shading.fxh:152-179, RenderPBR.psh:426-433)
    MaterialNormalInfo info;
    {
        const v3 pos = mat_world_pos(k, cam, q.x, q.y), posPx = mat_world_pos(k, cam, q.xp, q.y), posPy = mat_world_pos(k, cam, q.x, q.yp);
        info.dPosDx = mat_ddx(q, pos, posPx);
        info.dPosDy = mat_ddy(q, pos, posPy);
        const bool front = k.face.p ? ld<float>(k.face, x, y) >= 0.0f : true;
        info.face = front ? 1.0f : -1.0f;
        const v3    meshNormal = k.meshNormal.p ? xyz(ld<v4>(k.meshNormal, x, y)) : mk3(0.0f);
        const float len = length(meshNormal);
        if (len > 1e-5f) info.normal = meshNormal / (len * info.face);
        else info.normal = normalize(cross(info.dPosDx, info.dPosDy)) * k.handness;
    }

    // ---- the normal maps' coordinates (RenderPBR.psh:435-457)
    const int  normalTex = hasUV ? m->texture[MIFX_PBR_TEXTURE_NORMAL] : -1;
    const bool clearCoat = (k.layers & MIFX_PBR_LAYER_CLEAR_COAT) != 0u;
    const int  ccNormalTex = (hasUV && clearCoat) ? m->texture[MIFX_PBR_TEXTURE_CLEAR_COAT_NORMAL] : -1;
    const MaterialTexAttribs normalAttribs = normalTex >= 0 ? mat_attribs(m, MIFX_PBR_TEXTURE_NORMAL) : mat_default_attribs();
    const MaterialNormalUV   nm = mat_normal_uv_info<ATLAS>(k, q, in, normalAttribs);

    // ---- ReadBaseLayerProperties (RenderPBR.psh:138-184)
    {
        v3 micro{0.5f, 0.5f, 1.0f};                                                                     // GetMicroNormal (PBR_Textures.fxh:515-545)
        if (normalTex >= 0) micro = mat_sample_normal_texture<ATLAS>(k, normalAttribs, normalTex, q, nm);
        const v3 tsNormal = mat_unpack_normal(micro, m->basic.NormalScale);
        o.normal = mk4(mat_perturb_normal(info, nm.dUVdx, nm.dUVdy, tsNormal, nm.selector >= 0.0f), 0.0f); // :175-179
    }
    {
        v4 physicalDesc = mk4(1.0f);                                                                    // GetPhysicalDesc (PBR_Textures.fxh:587-631)
        const int pd = hasUV ? m->texture[MIFX_PBR_TEXTURE_PHYS_DESC] : -1;
        if (m->texture[MIFX_PBR_TEXTURE_PHYS_DESC] >= 0)
        {
            if (pd >= 0) physicalDesc = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_PHYS_DESC, pd, q, in, mk4(1.0f));
        }
        else if (hasUV)
        {
            const int mt = m->texture[MIFX_PBR_TEXTURE_METALLIC], rt = m->texture[MIFX_PBR_TEXTURE_ROUGHNESS];
            if (mt >= 0) physicalDesc.z = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_METALLIC, mt, q, in, mk4(1.0f)).x;
            if (rt >= 0) physicalDesc.y = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_ROUGHNESS, rt, q, in, mk4(1.0f)).x;
        }
        if (k.workflow == MIFX_PBR_WORKFLOW_SPECULAR_GLOSSINESS)
            o.material = physicalDesc; // (the shade converts this plane from sRGB itself, RenderPBR.psh:157; the factors of :159-164 are 1: refused otherwise)
        else
            o.material = v4{saturate(physicalDesc.y * m->basic.RoughnessFactor), saturate(physicalDesc.z * m->basic.MetallicFactor), 0.0f, 0.0f}; // :169-170
    }
    // ---- GetOcclusion (PBR_Textures.fxh:547-563), GetEmissive (:565-585)
    if (k.outOcclusion.p)
    {
        float       occlusion = 1.0f;
        const int   t = hasUV ? m->texture[MIFX_PBR_TEXTURE_OCCLUSION] : -1;
        if (t >= 0) occlusion = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_OCCLUSION, t, q, in, mk4(1.0f)).x;
        o.occlusion = occlusion * m->basic.OcclusionFactor;
    }
    if (k.outEmissive.p)
    {
        v3 emissive = mk3(1.0f);
        if (m->texture[MIFX_PBR_TEXTURE_EMISSIVE] >= 0)
        {
            if (hasUV) emissive = xyz(mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_EMISSIVE, m->texture[MIFX_PBR_TEXTURE_EMISSIVE], q, in, mk4(1.0f)));
            emissive = mat_to_linear(k, emissive);                                                      // :578
        }
        o.emissive = v4{emissive.x * m->basic.EmissiveFactorR, emissive.y * m->basic.EmissiveFactorG, emissive.z * m->basic.EmissiveFactorB, 0.0f};
    }

    // ---- ReadClearcoatLayerProperties (RenderPBR.psh:186-220): the fetches and the layer's normal
    if (clearCoat)
    {
        float factor = 1.0f, roughness = 1.0f;
        const int ft = hasUV ? m->texture[MIFX_PBR_TEXTURE_CLEAR_COAT] : -1, rt = hasUV ? m->texture[MIFX_PBR_TEXTURE_CLEAR_COAT_ROUGHNESS] : -1;
        if (ft >= 0) factor = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_CLEAR_COAT, ft, q, in, mk4(1.0f)).x;               // GetClearcoatFactor (PBR_Textures.fxh:639-663)
        if (rt >= 0) roughness = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_CLEAR_COAT_ROUGHNESS, rt, q, in, mk4(1.0f)).y;  // GetClearcoatRoughness (:665-689)
        o.clearcoat = v4{factor * m->basic.ClearcoatFactor, roughness * m->basic.ClearcoatRoughnessFactor, 0.0f, 0.0f};
        if (k.outClearcoatNormal.p)
        {
            v3 normal = info.normal;                                                                    // :202
            if (ccNormalTex >= 0)                                                                       // :203-216
            {
                const MaterialTexAttribs ccAttribs = mat_attribs(m, MIFX_PBR_TEXTURE_CLEAR_COAT_NORMAL);
                const MaterialNormalUV   cn = mat_normal_uv_info<ATLAS>(k, q, in, ccAttribs);           // :448-452
                const v3 sampled = mat_sample_normal_texture<ATLAS>(k, ccAttribs, ccNormalTex, q, cn);  // GetClearcoatNormal (PBR_Textures.fxh:691-725)
                const v3 ts = mat_unpack_normal(sampled, m->basic.ClearcoatNormalScale);
                if (cn.selector >= 0.0f) normal = mat_perturb_normal(info, cn.dUVdx, cn.dUVdy, ts, true);
            }
            o.clearcoatNormal = mk4(normal, 0.0f);
        }
    }
    // ---- ReadSheenLayerProperties (:222-233)
    if (k.layers & MIFX_PBR_LAYER_SHEEN)
    {
        v3    color = mk3(1.0f);                                                                        // GetSheenColor (PBR_Textures.fxh:731-756)
        float roughness = 1.0f;                                                                         // GetSheenRoughness (:758-782)
        if (m->texture[MIFX_PBR_TEXTURE_SHEEN_COLOR] >= 0)
        {
            if (hasUV) color = xyz(mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_SHEEN_COLOR, m->texture[MIFX_PBR_TEXTURE_SHEEN_COLOR], q, in, mk4(1.0f)));
            color = mat_to_linear(k, color);                                                            // :746
        }
        const int rt = hasUV ? m->texture[MIFX_PBR_TEXTURE_SHEEN_ROUGHNESS] : -1;
        if (rt >= 0) roughness = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_SHEEN_ROUGHNESS, rt, q, in, mk4(1.0f)).w;
        o.sheen = v4{color.x * m->sheen.ColorFactorR, color.y * m->sheen.ColorFactorG, color.z * m->sheen.ColorFactorB, roughness * m->sheen.RoughnessFactor};
    }
    // ---- GetAnisotropy (PBR_Textures.fxh:788-815; RenderPBR.psh:260)
    if (k.layers & MIFX_PBR_LAYER_ANISOTROPY)
    {
        v3 a{1.0f, 0.5f, 1.0f};
        const int t = hasUV ? m->texture[MIFX_PBR_TEXTURE_ANISOTROPY] : -1;
        if (t >= 0) a = xyz(mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_ANISOTROPY, t, q, in, v4{1.0f, 0.5f, 1.0f, 1.0f}));
        o.anisotropy = v4{a.x * 2.0f - 1.0f, a.y * 2.0f - 1.0f, a.z * m->anisotropy.Strength, 0.0f};
    }
    // ---- GetIridescence, GetIridescenceThickness (PBR_Textures.fxh:821-872; RenderPBR.psh:242-243)
    if (k.layers & MIFX_PBR_LAYER_IRIDESCENCE)
    {
        float factor = 1.0f, thickness = 1.0f;
        const int ft = hasUV ? m->texture[MIFX_PBR_TEXTURE_IRIDESCENCE] : -1, tt = hasUV ? m->texture[MIFX_PBR_TEXTURE_IRIDESCENCE_THICKNESS] : -1;
        if (ft >= 0) factor = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_IRIDESCENCE, ft, q, in, mk4(1.0f)).x;
        if (tt >= 0) thickness = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_IRIDESCENCE_THICKNESS, tt, q, in, mk4(1.0f)).y;
        o.iridescence = v4{factor * m->iridescence.Factor, lerpf(m->iridescence.ThicknessMinimum, m->iridescence.ThicknessMaximum, thickness), 0.0f, 0.0f};
    }
    // ---- GetTransmission (PBR_Textures.fxh:878-902; RenderPBR.psh:348)
    if (k.layers & MIFX_PBR_LAYER_TRANSMISSION)
    {
        float transmission = 1.0f;
        const int t = hasUV ? m->texture[MIFX_PBR_TEXTURE_TRANSMISSION] : -1;
        if (t >= 0) transmission = mat_sample_texture<ATLAS>(k, m, MIFX_PBR_TEXTURE_TRANSMISSION, t, q, in, mk4(1.0f)).x;
        o.transmission = transmission * m->transmission.Factor;
    }
    return true;
}
// what the kernel does with a pixel: only a pixel with a fragment stores, only into the planes that are there
template <bool ATLAS> MIFX_D void material_fetch_store(int x, int y, const MaterialFetchK& k, const CamK& cam)
{
    MaterialFetchOut o;
    if (!material_fetch_pixel<ATLAS>(x, y, k, cam, o)) return;
    st<v4>(k.outBaseColor, x, y, o.baseColor);
    st<v4>(k.outNormal, x, y, o.normal);
    st<v4>(k.outMaterial, x, y, o.material);
    if (k.outEmissive.p) st<v4>(k.outEmissive, x, y, o.emissive);
    if (k.outOcclusion.p) st<float>(k.outOcclusion, x, y, o.occlusion);
    if (k.layers & MIFX_PBR_LAYER_CLEAR_COAT)
    {
        st<v4>(k.outClearcoat, x, y, o.clearcoat);
        if (k.outClearcoatNormal.p) st<v4>(k.outClearcoatNormal, x, y, o.clearcoatNormal);
    }
    if (k.layers & MIFX_PBR_LAYER_SHEEN) st<v4>(k.outSheen, x, y, o.sheen);
    if (k.layers & MIFX_PBR_LAYER_ANISOTROPY) st<v4>(k.outAnisotropy, x, y, o.anisotropy);
    if (k.layers & MIFX_PBR_LAYER_IRIDESCENCE) st<v4>(k.outIridescence, x, y, o.iridescence);
    if (k.layers & MIFX_PBR_LAYER_TRANSMISSION) st<float>(k.outTransmission, x, y, o.transmission);
}
} // namespace mifx
