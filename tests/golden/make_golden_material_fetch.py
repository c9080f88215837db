#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/material_fetch_golden.npz: what the REFERENCE's forward pixel shader fetches for the cases of tests/material_fetch_util.py --
the head of `main` of Shaders/PBR/private/RenderPBR.psh (lines 424-457) with GetDefaultTextureAttribs, GetNormalMapUVInfo, ReadBaseLayerProperties and the layer readers
(lines 80-297), through Shaders/PBR/private/PBR_Textures.fxh, Shaders/Common/public/AtlasSampling.fxh, GetPerturbNormalInfo / PerturbNormal of
Shaders/PBR/public/PBR_Shading.fxh and TransformTangentSpaceNormalGrad of Shaders/Common/public/ShaderUtilities.fxh -- compiled for the CPU from the reference tree where it lies,
one translation unit per permutation of USE_*_MAP, ENABLE_*, USE_TEXCOORD0 / 1, USE_VERTEX_NORMALS, USE_VERTEX_COLORS, USE_TEXTURE_ATLAS, ENABLE_TEXCOORD_TRANSFORM and
TEX_COLOR_CONVERSION_MODE.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, as for make_golden_grid.py); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_material_fetch.py

The shader text is read at generation time, rewritten by oracle/ref_prep.py into a temporary directory and compiled there through oracle/ref/hlsl_shim.h with the wrapper below,
which #includes the reference files by name and holds none of their text; the two line ranges of RenderPBR.psh are cut out at generation time.  Nothing compiled is kept: the
fixture holds data only (the reference's outputs; the inputs are rebuilt from fixed seeds by tests/material_fetch_util.py).

What the wrapper supplies, inside the permutation's own namespace, in place of the shim's zero-returning ddx(float2) / ddx(float3) -- the two contracts the reference leaves
to the graphics API (include/mifx.h, "material fetch"):
  * the vector derivatives on the shim's two-phase quad mechanism (phase 0 records the value of every lane of the 2x2 quad, phase 1 replays: ddx = right - left of the lane's
    row, ddy = bottom - top of its column); a lane outside the frame runs at the clamped pixel, so an odd last column / row gets a zero derivative;
  * a Texture2DArray with SampleBias, SampleGrad, SampleLevel, CalculateLevelOfDetail and GetDimensions: trilinear, WRAP, texel centres at (i + 0.5) / N, the weights of
    GetBilinearSamplingInfoUC, rho = max(|dUVdx * dim|, |dUVdy * dim|), lod = log2(rho) + bias clamped to [0, mips - 1], a + (b - a) * frac(lod).
A frame is run once per material over every pixel (a pixel's quad partners are evaluated with ITS material, as helper lanes are) and the results are merged by the index plane.
The planes hold, where a fragment is: base_color = GetBaseColor; normal = Base.Normal; material = PhysicalDesc.gb after RenderPBR.psh:169-170 (the two statements are restated
below: ReadBaseLayerProperties does not return them) or the sampled PhysicalDesc for specular-glossiness; emissive = GetEmissive; occlusion = GetOcclusion; clearcoat =
(GetClearcoatFactor, GetClearcoatRoughness); clearcoat_normal = ReadClearcoatLayerProperties().Normal; sheen = ReadSheenLayerProperties; anisotropy = GetAnisotropy;
iridescence = (GetIridescence, GetIridescenceThickness); transmission = GetTransmission.  Elsewhere they hold zero.

Every case is built twice: strict fp32 (the oracle's flags) and with -ffp-contract=fast -march=native.  The largest difference in the measure of util.assert_close must stay
within 0.5e-3 on every stored value ("move the case" otherwise): that is what entitles the device test to util.assert_close at its defaults with no outliers."""
import concurrent.futures
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_grid as MG  # noqa: E402  (the two flag sets)
import material_fetch_util as M  # noqa: E402
import ref_prep  # noqa: E402
import util  # noqa: E402

REFERENCE_ROOT = MG.REFERENCE_ROOT
F = np.float32
NOUT = 41  # floats a pixel: base colour 4, normal 4, material 4, emissive 4, occlusion 1, clear coat 4, its normal 4, sheen 4, anisotropy 4, iridescence 4, transmission 1

BODY = r"""
#include "ref_common.h"
#define PBR_MAX_LIGHTS 0
#define USE_IBL 0
#define ENABLE_SHADOWS 0
#define NUM_OIT_LAYERS 0
#define ENABLE_VOLUME 0
#define PBR_WORKFLOW_UNLIT 2 // PBR_Renderer.cpp:1409
#define PBR_NUM_TEXTURE_ATTRIBUTES 16
// the slots of mifx_pbr_material::textures (include/mifx.h); the first five are the defaults of PBR_Textures.fxh:8-26
#define MetallicTextureAttribId 5
#define RoughnessTextureAttribId 6
#define ClearCoatTextureAttribId 7
#define ClearCoatRoughnessTextureAttribId 8
#define ClearCoatNormalTextureAttribId 9
#define SheenColorTextureAttribId 10
#define SheenRoughnessTextureAttribId 11
#define AnisotropyTextureAttribId 12
#define IridescenceTextureAttribId 13
#define IridescenceThicknessTextureAttribId 14
#define TransmissionTextureAttribId 15
#define TEX_COLOR_CONVERSION_MODE_NONE 0
#define TEX_COLOR_CONVERSION_MODE_SRGB_TO_LINEAR 1
namespace hlsl { namespace MF_NS {
// ---- contract 1: vector derivatives on the shim's two-phase quad mechanism, with a record of their own
struct QuadRec { int idx = 0; float3 rec[4][512]; };
inline thread_local QuadRec g_quad;
inline float3 quad_deriv(const float3& v, bool is_y)
{
    ExecCtx& c = g_ctx;
    QuadRec& q = g_quad;
    if (c.quad_phase < 0) return float3(0.f, 0.f, 0.f);
    const int k = q.idx++;
    if (c.quad_phase == 0) { q.rec[c.quad_lane][k] = v; return float3(0.f, 0.f, 0.f); }
    const int l = c.quad_lane, row = l & 2, col = l & 1;
    return is_y ? q.rec[col + 2][k] - q.rec[col][k] : q.rec[row + 1][k] - q.rec[row][k];
}
inline float3 mf_ddx(const float3& v) { return quad_deriv(v, false); }
inline float3 mf_ddy(const float3& v) { return quad_deriv(v, true); }
inline float2 mf_ddx(const float2& v) { const float3 d = quad_deriv(float3(v.x, v.y, 0.f), false); return float2(d.x, d.y); }
inline float2 mf_ddy(const float2& v) { const float3 d = quad_deriv(float3(v.x, v.y, 0.f), true); return float2(d.x, d.y); }
// (argument-dependent lookup would find the shim's zero-returning overloads beside these: the reference's text reaches them under these names)
#define ddx mf_ddx
#define ddy mf_ddy
// (TransformUV: the shim has no float2x2)
struct float2x2 { float2 r[2]; };
inline float2x2 MatrixFromRows(const float2& a, const float2& b) { float2x2 m; m.r[0] = a; m.r[1] = b; return m; }
inline float2 mul(const float2& v, const float2x2& m) { return v.x * m.r[0] + v.y * m.r[1]; }
using ::hlsl::MatrixFromRows;
using ::hlsl::mul;

// ---- contract 2: the sampler
struct Texture2DArray
{
    const float* data = nullptr; // RGBA32_FLOAT (an RGBA8_UNORM texture arrives decoded: code / 255)
    int          w = 0, h = 0, slices = 0, mips = 0;
    size_t       slice_floats = 0;
    unsigned     level_offset[16] = {};
    void GetDimensions(float& W, float& H, float& N) const { W = float(w); H = float(h); N = float(slices); }
    const float* slice_of(float fSlice) const
    {
        const float s = std::fmin(std::fmax(std::floor(fSlice + 0.5f), 0.0f), float(slices - 1));
        return data + size_t(int(s)) * slice_floats;
    }
    static int wrap(float f, int n, bool& ok)
    {
        ok = std::fabs(f) < 1073741824.0f;
        int i = ok ? int(f) : 0;
        i %= n;
        return i < 0 ? i + n : i;
    }
    float4 texel(const float* s, int level, int lw, int x, int y) const
    {
        const float* p = s + (size_t(level_offset[level]) + size_t(y) * lw + x) * 4;
        return float4(p[0], p[1], p[2], p[3]);
    }
    float4 bilinear(const float* s, int level, const float2& uv) const
    {
        const int   lw = std::max(w >> level, 1), lh = std::max(h >> level, 1);
        const float fx = uv.x * float(lw) - 0.5f, fy = uv.y * float(lh) - 0.5f;
        const float x0f = std::floor(fx), y0f = std::floor(fy);
        bool okx, oky;
        const int x0 = wrap(x0f, lw, okx), y0 = wrap(y0f, lh, oky);
        const int x1 = x0 + 1 == lw ? 0 : x0 + 1, y1 = y0 + 1 == lh ? 0 : y0 + 1;
        const float wx = okx ? fx - x0f : 0.0f, wy = oky ? fy - y0f : 0.0f;
        float4 acc = texel(s, level, lw, x0, y0) * ((1.0f - wx) * (1.0f - wy));
        acc = acc + texel(s, level, lw, x1, y0) * (wx * (1.0f - wy));
        acc = acc + texel(s, level, lw, x0, y1) * ((1.0f - wx) * wy);
        acc = acc + texel(s, level, lw, x1, y1) * (wx * wy);
        return acc;
    }
    float clamp_lod(float lod) const { return std::fmin(std::fmax(lod, 0.0f), float(mips - 1)); }
    float lod_of(const float2& dx, const float2& dy, float bias) const
    {
        const float  fw = float(w), fh = float(h);
        const float2 dim(fw, fh);
        const float  rho = std::fmax(length(dx * dim), length(dy * dim));
        return clamp_lod(std::log2(rho) + bias);
    }
    float4 SampleLevel(const SamplerState&, const float3& uvs, float lod) const
    {
        const float* s = slice_of(uvs.z);
        lod = clamp_lod(lod);
        const int   l0 = int(std::floor(lod)), l1 = l0 + 1 < mips ? l0 + 1 : l0;
        const float f  = lod - float(l0);
        const float2 uv(uvs.x, uvs.y);
        const float4 a = bilinear(s, l0, uv);
        if (f == 0.0f || l1 == l0) return a;
        const float4 b = bilinear(s, l1, uv);
        return a + (b - a) * f;
    }
    float4 SampleGrad(const SamplerState& sm, const float3& uvs, const float2& dx, const float2& dy) const { return SampleLevel(sm, uvs, lod_of(dx, dy, 0.0f)); }
    float4 SampleBias(const SamplerState& sm, const float3& uvs, float bias) const
    {
        const float2 uv(uvs.x, uvs.y);
        const float2 dx = ddx(uv), dy = ddy(uv);
        return SampleLevel(sm, uvs, lod_of(dx, dy, bias));
    }
    float CalculateLevelOfDetail(const SamplerState&, const float2& uv) const
    {
        const float2 dx = ddx(uv), dy = ddy(uv);
        return lod_of(dx, dy, 0.0f);
    }
};

#include "ShaderDefinitions.fxh"
#include "BasicStructures.fxh"
#include "PostFX_Common.fxh"
#include "PBR_Shading.fxh"
#include "RenderPBR_Structures.fxh"
#if ENABLE_IRIDESCENCE
#include "Iridescence.fxh" // RenderPBR.psh:9-11
#endif
struct VSOutput // RenderPBR.psh:17-26
{
    float4 ClipPos;
    float3 WorldPos;
    float4 Color;
    float3 Normal;
    float2 UV0;
    float2 UV1;
};
#include "PBR_Textures.fxh" // RenderPBR.psh:43
static PBRFrameAttribs       g_Frame;     // RenderPBR.psh:45-48
static PBRPrimitiveAttribs   g_Primitive; // :50-57
#define PRIMITIVE g_Primitive
static PBRMaterialShaderInfo g_Material;  // :65-68
#include "RenderPBR_80_297.inc"
}}
using namespace hlsl;

namespace
{
struct TexDesc { const float* data; int w, h, slices, mips; unsigned long long slice_floats; };
struct MaterialRecord // == mifx_pbr_material (include/mifx.h)
{
    float basic[24], sheen[4], anisotropy[4], iridescence[4], transmission[4], fallback[4];
    float textures[16][12];
    int   texture[16];
};
void bind(MF_NS::Texture2DArray& t, const TexDesc* textures, int index)
{
    const TexDesc& d = textures[index];
    t.data = d.data; t.w = d.w; t.h = d.h; t.slices = d.slices; t.mips = d.mips; t.slice_floats = size_t(d.slice_floats);
    unsigned off = 0;
    for (int l = 0; l < d.mips; ++l)
    {
        t.level_offset[l] = off;
        off += unsigned(std::max(d.w >> l, 1)) * unsigned(std::max(d.h >> l, 1));
    }
}
}

// planes: null = the permutation without it (the unit was compiled for exactly the planes the case has); out: NOUT floats a pixel, every pixel of the frame
extern "C" int MF_ENTRY(const void* camera, const void* material, const TexDesc* textures, float mip_bias, int W, int H, const float* depth, const float* uv0, const float* uv1,
                        const float* mesh_normal, const float* color, const float* face, float* out)
{
    namespace mf = MF_NS;
    static_assert(sizeof(MaterialRecord) == 1008 && sizeof(mf::PBRMaterialTextureAttribs) == 48 && sizeof(mf::PBRMaterialBasicAttribs) == 96, "PBR_Structures.fxh");
    MaterialRecord m;
    std::memcpy(&m, material, sizeof(m));
    std::memset(&mf::g_Frame, 0, sizeof(mf::g_Frame));
    std::memcpy(&mf::g_Frame.Camera, camera, sizeof(mf::g_Frame.Camera));
    mf::g_Frame.Renderer.MipBias = mip_bias;
    std::memset(&mf::g_Primitive, 0, sizeof(mf::g_Primitive));
    mf::g_Primitive.FallbackColor = float4(m.fallback[0], m.fallback[1], m.fallback[2], m.fallback[3]);
    std::memcpy(&mf::g_Material.Basic, m.basic, 96);
    for (int i = 0; i < 16; ++i) std::memcpy(&mf::g_Material.Textures[i], m.textures[i], 48);
#if ENABLE_SHEEN
    std::memcpy(&mf::g_Material.Sheen, m.sheen, 16);
#endif
#if ENABLE_ANISOTROPY
    std::memcpy(&mf::g_Material.Anisotropy, m.anisotropy, 16);
#endif
#if ENABLE_IRIDESCENCE
    std::memcpy(&mf::g_Material.Iridescence, m.iridescence, 16);
#endif
#if ENABLE_TRANSMISSION
    std::memcpy(&mf::g_Material.Transmission, m.transmission, 16);
#endif
#if USE_COLOR_MAP
    bind(mf::g_BaseColorMap, textures, m.texture[0]);
#endif
#if USE_PHYS_DESC_MAP
    bind(mf::g_PhysicalDescriptorMap, textures, m.texture[1]);
#endif
#if USE_NORMAL_MAP
    bind(mf::g_NormalMap, textures, m.texture[2]);
#endif
#if USE_AO_MAP
    bind(mf::g_OcclusionMap, textures, m.texture[3]);
#endif
#if USE_EMISSIVE_MAP
    bind(mf::g_EmissiveMap, textures, m.texture[4]);
#endif
#if USE_METALLIC_MAP
    bind(mf::g_MetallicMap, textures, m.texture[5]);
#endif
#if USE_ROUGHNESS_MAP
    bind(mf::g_RoughnessMap, textures, m.texture[6]);
#endif
#if USE_CLEAR_COAT_MAP
    bind(mf::g_ClearCoatMap, textures, m.texture[7]);
#endif
#if USE_CLEAR_COAT_ROUGHNESS_MAP
    bind(mf::g_ClearCoatRoughnessMap, textures, m.texture[8]);
#endif
#if USE_CLEAR_COAT_NORMAL_MAP
    bind(mf::g_ClearCoatNormalMap, textures, m.texture[9]);
#endif
#if USE_SHEEN_COLOR_MAP
    bind(mf::g_SheenColorMap, textures, m.texture[10]);
#endif
#if USE_SHEEN_ROUGHNESS_MAP
    bind(mf::g_SheenRoughnessMap, textures, m.texture[11]);
#endif
#if USE_ANISOTROPY_MAP
    bind(mf::g_AnisotropyMap, textures, m.texture[12]);
#endif
#if USE_IRIDESCENCE_MAP
    bind(mf::g_IridescenceMap, textures, m.texture[13]);
#endif
#if USE_IRIDESCENCE_THICKNESS_MAP
    bind(mf::g_IridescenceThicknessMap, textures, m.texture[14]);
#endif
#if USE_TRANSMISSION_MAP
    bind(mf::g_TransmissionMap, textures, m.texture[15]);
#endif
    const mf::CameraAttribs& cam = mf::g_Frame.Camera;
#pragma omp parallel for schedule(dynamic, 2)
    for (int qy = 0; qy < (H + 1) / 2; ++qy)
        for (int qx = 0; qx < (W + 1) / 2; ++qx)
        {
            for (int phase = 0; phase < 2; ++phase)
                for (int lane = 0; lane < 4; ++lane)
                {
                    using namespace MF_NS;
                    const int lx = qx * 2 + (lane & 1), ly = qy * 2 + (lane >> 1);
                    const int x = std::min(lx, W - 1), y = std::min(ly, H - 1); // (a lane outside the frame runs at the clamped pixel)
                    g_ctx.discarded  = false;
                    g_ctx.quad_phase = phase;
                    g_ctx.quad_lane  = lane;
                    g_ctx.call_idx   = 0;
                    g_quad.idx       = 0;
                    const size_t p = size_t(y) * W + x;
                    mf::VSOutput VSOut;
                    VSOut.ClipPos  = float4(float(x) + 0.5f, float(y) + 0.5f, depth[p], 1.0f);
                    const float2 uv((float(x) + 0.5f) * cam.f4ViewportSize.z, (float(y) + 0.5f) * cam.f4ViewportSize.w);
                    VSOut.WorldPos = InvProjectPosition(float3(uv, depth[p]), cam.mViewProjInv); // as the shade reconstructs Shading.Pos
                    VSOut.Color    = color ? float4(color[4 * p], color[4 * p + 1], color[4 * p + 2], color[4 * p + 3]) : float4(1.f, 1.f, 1.f, 1.f);
                    VSOut.Normal   = mesh_normal ? float3(mesh_normal[4 * p], mesh_normal[4 * p + 1], mesh_normal[4 * p + 2]) : float3(0.f, 0.f, 0.f);
                    VSOut.UV0      = uv0 ? float2(uv0[2 * p], uv0[2 * p + 1]) : float2(0.f, 0.f);
                    VSOut.UV1      = uv1 ? float2(uv1[2 * p], uv1[2 * p + 1]) : float2(0.f, 0.f);
                    const bool IsFrontFace = face ? face[p] >= 0.0f : true;
#include "RenderPBR_main_424_457.inc"
                    const float3 View = normalize(g_Frame.Camera.f4Position.xyz - VSOut.WorldPos.xyz); // RenderPBR.psh:309
                    const BaseLayerShadingInfo Base = ReadBaseLayerProperties(VSOut, g_Material, BaseColor, NormalInfo, NMUVInfo, View); // :310
                    float4 PhysicalDesc = GetPhysicalDesc(VSOut, g_Material, g_Frame.Renderer.MipBias); // :148
                    float4 MaterialPlane = PhysicalDesc; // specular-glossiness: the sampled texel (the shade converts it, :157; factors 1)
                    if (g_Material.Basic.Workflow == PBR_WORKFLOW_METALLIC_ROUGHNESS)
                    {
                        PhysicalDesc.g = saturate(PhysicalDesc.g * g_Material.Basic.RoughnessFactor); // :169
                        PhysicalDesc.b = saturate(PhysicalDesc.b * g_Material.Basic.MetallicFactor);  // :170
                        MaterialPlane  = float4(PhysicalDesc.g, PhysicalDesc.b, 0.f, 0.f);
                    }
                    const float  Occlusion = GetOcclusion(VSOut, g_Material, g_Frame.Renderer.MipBias); // :311
                    const float3 Emissive  = GetEmissive(VSOut, g_Material, g_Frame.Renderer.MipBias);  // :312
                    float r[NOUT_FLOATS] = {};
                    auto put = [&](int at, const float4& v) { r[at] = v.x; r[at + 1] = v.y; r[at + 2] = v.z; r[at + 3] = v.w; };
                    put(0, BaseColor);
                    put(4, float4(Base.Normal, 0.f));
                    put(8, MaterialPlane);
                    put(12, float4(Emissive, 0.f));
                    r[16] = Occlusion;
#if ENABLE_CLEAR_COAT
                    {
                        const ClearcoatShadingInfo cc = ReadClearcoatLayerProperties(VSOut, g_Material, NormalInfo, ClearCoatNMUVInfo); // :320
                        put(17, float4(GetClearcoatFactor(VSOut, g_Material, g_Frame.Renderer.MipBias), GetClearcoatRoughness(VSOut, g_Material, g_Frame.Renderer.MipBias), 0.f, 0.f)); // :194-196
                        put(21, float4(cc.Normal, 0.f));
                    }
#endif
#if ENABLE_SHEEN
                    {
                        const SheenShadingInfo sh = ReadSheenLayerProperties(VSOut, g_Material); // :326
                        put(25, float4(sh.Color, sh.Roughness));
                    }
#endif
#if ENABLE_ANISOTROPY
                    put(29, float4(GetAnisotropy(VSOut, g_Material, g_Frame.Renderer.MipBias), 0.f)); // :260
#endif
#if ENABLE_IRIDESCENCE
                    put(33, float4(GetIridescence(VSOut, g_Material, g_Frame.Renderer.MipBias), GetIridescenceThickness(VSOut, g_Material, g_Frame.Renderer.MipBias), 0.f, 0.f)); // :242-243
#endif
#if ENABLE_TRANSMISSION
                    r[37] = GetTransmission(VSOut, g_Material, g_Frame.Renderer.MipBias); // :348
#endif
                    if (phase == 1 && lx < W && ly < H) std::memcpy(out + p * NOUT_FLOATS, r, sizeof(r));
                }
            g_ctx.quad_phase = -1;
        }
    return 0;
}
"""
# (where the planes sit in the record of a pixel)
OFFSETS = {"base_color": 0, "normal": 4, "material": 8, "emissive": 12, "occlusion": 16, "clearcoat": 17, "clearcoat_normal": 21, "sheen": 25, "anisotropy": 29, "iridescence": 33,
           "transmission": 37}
MAP_MACROS = ("USE_COLOR_MAP", "USE_PHYS_DESC_MAP", "USE_NORMAL_MAP", "USE_AO_MAP", "USE_EMISSIVE_MAP", "USE_METALLIC_MAP", "USE_ROUGHNESS_MAP", "USE_CLEAR_COAT_MAP",
              "USE_CLEAR_COAT_ROUGHNESS_MAP", "USE_CLEAR_COAT_NORMAL_MAP", "USE_SHEEN_COLOR_MAP", "USE_SHEEN_ROUGHNESS_MAP", "USE_ANISOTROPY_MAP", "USE_IRIDESCENCE_MAP",
              "USE_IRIDESCENCE_THICKNESS_MAP", "USE_TRANSMISSION_MAP")


def permutation(c, m):
    """The pipeline key of one material of a case"""
    maps = sum(1 << M.S[n] for n in m["maps"])
    i = c["interp"]
    return (maps, c["layers"], "uv0" in i, "uv1" in i, "mesh_normal" in i, "color" in i, c["flags"])


def unit_text(key, name):
    maps, layers, uv0, uv1, normals, colors, flags = key
    lines = [f"#define MF_NS mf_{name}", f"#define MF_ENTRY ref_mf_{name}", f"#define NOUT_FLOATS {NOUT}"]
    lines += [f"#define {n} {(maps >> s) & 1}" for s, n in enumerate(MAP_MACROS)]
    lines += ["#define USE_THICKNESS_MAP 0", f"#define USE_TEXCOORD0 {int(uv0)}", f"#define USE_TEXCOORD1 {int(uv1)}", f"#define USE_VERTEX_NORMALS {int(normals)}",
              f"#define USE_VERTEX_COLORS {int(colors)}", "#define USE_VERTEX_TANGENTS 0", f"#define USE_TEXTURE_ATLAS {int(bool(flags & M.FLAG_ATLAS))}",
              f"#define ENABLE_TEXCOORD_TRANSFORM {int(bool(flags & M.FLAG_TRANSFORM))}", f"#define TEX_COLOR_CONVERSION_MODE {int(bool(flags & M.FLAG_SRGB))}",
              f"#define ENABLE_CLEAR_COAT {layers & 1}", f"#define ENABLE_SHEEN {(layers >> 1) & 1}", f"#define ENABLE_ANISOTROPY {(layers >> 2) & 1}",
              f"#define ENABLE_IRIDESCENCE {(layers >> 3) & 1}", f"#define ENABLE_TRANSMISSION {(layers >> 4) & 1}", '#include "material_fetch_body.inc"']
    return "\n".join(lines) + "\n"


def prepare(tmp):
    """The reference's text, rewritten for the shim, in the temporary directory; the two line ranges of RenderPBR.psh"""
    assert ref_prep.main(REFERENCE_ROOT, tmp) == 0
    with open(os.path.join(REFERENCE_ROOT, "Shaders/PBR/private/RenderPBR.psh"), encoding="utf-8", errors="replace") as f:
        lines = f.read().splitlines()
    assert lines[79].startswith("PBRMaterialTextureAttribs GetDefaultTextureAttribs()") and lines[296] == "#endif" and lines[298].startswith("SurfaceShadingInfo GetSurfaceShadingInfo("), \
        "RenderPBR.psh:80-297 moved"
    assert lines[423].lstrip().startswith("float4 BaseColor = GetBaseColor(") and lines[456].strip() == "#   endif" and lines[458].lstrip().startswith("PBRMaterialBasicAttribs BasicAttribs"), \
        "RenderPBR.psh:424-457 moved"
    open(os.path.join(tmp, "RenderPBR_80_297.inc"), "w").write(ref_prep.transform("\n".join(lines[79:297]) + "\n"))
    open(os.path.join(tmp, "RenderPBR_main_424_457.inc"), "w").write(ref_prep.transform("\n".join(lines[423:457]) + "\n"))
    open(os.path.join(tmp, "material_fetch_body.inc"), "w").write(BODY)


def build(units, flags, tmp, tag):
    def cc(item):
        name, text = item
        src = os.path.join(tmp, f"{name}.cpp")
        if not os.path.exists(src):
            open(src, "w").write(text)
        obj = os.path.join(tmp, f"{name}_{tag}.o")
        r = subprocess.run(["g++", "-std=c++20", "-c"] + flags + ["-I", os.path.join(ROOT, "oracle", "ref"), "-I", tmp, "-o", obj, src], capture_output=True, text=True)
        if r.returncode != 0:
            lines = r.stderr.splitlines()
            for i, l in enumerate(lines):  # (the errors, each with the two lines behind it; the notes of a failed overload resolution fill pages)
                if "error:" in l:
                    sys.stderr.write("\n".join(lines[i:i + 3]) + "\n")
            raise RuntimeError(f"compiling {name} failed")
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(cc, units.items()))
    so = os.path.join(tmp, f"libmaterial_fetch_{tag}.so")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", so] + objs, check=True)
    return ctypes.CDLL(so)


class TexDesc(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("w", ctypes.c_int), ("h", ctypes.c_int), ("slices", ctypes.c_int), ("mips", ctypes.c_int), ("slice_floats", ctypes.c_uint64)]


def run_case(lib, c, keys):
    """The reference's planes of a case: one run per material over the whole frame, merged by the index plane; zero where no fragment is"""
    i = c["interp"]
    h, w = i["depth"].shape
    flat = [np.ascontiguousarray(np.concatenate([m.reshape(m.shape[0], -1) for m in M.decoded(t)], axis=1)) for t in c["textures"]]
    descs = (TexDesc * max(len(flat), 1))(*[TexDesc(f.ctypes.data, t[0].shape[2], t[0].shape[1], t[0].shape[0], len(t), f.shape[1]) for f, t in zip(flat, c["textures"])])
    keep = {k: np.ascontiguousarray(i[k]) for k in i}
    ptr = lambda k: keep[k].ctypes.data_as(ctypes.c_void_p) if k in keep else None  # noqa: E731
    index = i.get("material_index")
    merged = np.zeros((h, w, NOUT), F)
    for mi, m in enumerate(c["materials"]):
        out = np.zeros((h, w, NOUT), F)
        words = M.material_words(m)
        fn = getattr(lib, "ref_mf_" + keys[permutation(c, m)])
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 7
        rc = fn(c["camera"].ctypes.data, words.ctypes.data, ctypes.cast(descs, ctypes.c_void_p), c["mip_bias"], w, h, ptr("depth"), ptr("uv0"), ptr("uv1"), ptr("mesh_normal"),
                ptr("color"), ptr("face"), out.ctypes.data)
        assert rc == 0
        sel = np.ones((h, w), bool) if index is None else index.astype(np.int64) == mi
        merged[sel] = out[sel]
    merged[~M.has_fragment(c)] = 0.0
    return merged


def shade_cases(cs, fx):
    """Cases (v): what the existing reference shade (oracle/_ref: ref_pbr_shade_layers_all, ref_pbr_shade) makes of the reference-fetched planes"""
    import pyref
    from layers_util import BACKGROUND, LAYER_ORDER

    ref = pyref.ref_lib()
    assert ref is not None and ref.has("ref_pbr_shade_layers_all"), "oracle/_ref is not built: run build() of __graft_entry__.py where the reference tree is mounted"
    ibl, albedo, charlie, sa = M.shade_setup()
    luts = [np.repeat(albedo[..., None], 4, -1).copy(), np.repeat(charlie[..., None], 4, -1).copy()]
    for ci, c in enumerate(cs):
        if c["name"] not in M.SHADED:
            continue
        gold_case = {k[len(f"c{ci}_"):]: v for k, v in fx.items() if k.startswith(f"c{ci}_")}
        p = M.planes_with_caller_texels(c, gold_case)
        h, w = c["interp"]["depth"].shape
        rad, spec = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
        ins = [p["base_color"], p["normal"], p["material"], c["interp"]["depth"], p["emissive"], p["occlusion"], ibl["lut"], ibl["irradiance"], ibl["prefiltered"]]
        if M.SHADED[c["name"]] is None:
            ref.call("ref_pbr_shade", ins, [rad, spec], cam0=c["camera"].tobytes(), attribs=bytes(sa), fval=list(BACKGROUND))
        else:
            planes = {**{k: np.zeros((h, w, 4), F) for k in LAYER_ORDER}, **{k: p[k] for k in M.layer_planes_written(c)}}
            planes["transmission"] = np.ascontiguousarray(np.repeat(p["transmission"][..., None], 4, -1))  # (the checker reads x of a 4-channel plane)
            ref.call("ref_pbr_shade_layers_" + M.SHADED[c["name"]], ins + [[planes[k] for k in LAYER_ORDER], luts], [rad, spec], cam0=c["camera"].tobytes(), attribs=bytes(sa),
                     ival=[1, 0, 0, 0, 0, 0, 0, 0], fval=list(BACKGROUND) + [M.IOR, M.ROTATION])  # clear-coat normal map bound, no vertex tangents
        assert np.isfinite(rad).all() and np.isfinite(spec).all(), c["name"]
        print(f"{c['name']:34s} shaded: mean radiance {rad[M.has_fragment(c)][:, :3].mean():.4f}")
        fx[f"c{ci}_shaded_radiance"], fx[f"c{ci}_shaded_specular_ibl"] = np.ascontiguousarray(np.moveaxis(rad, -1, 0)), np.ascontiguousarray(np.moveaxis(spec, -1, 0))


def main():
    assert os.path.isdir(os.path.join(REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    cs = M.cases()
    keys = {}
    for c in cs:
        for m in c["materials"]:
            keys.setdefault(permutation(c, m), "p%02d" % len(keys))
    fx = {"names": np.array([c["name"] for c in cs])}
    worst = 0.0
    with tempfile.TemporaryDirectory(prefix="mifx_material_fetch_golden_") as tmp:
        prepare(tmp)
        units = {name: unit_text(key, name) for key, name in keys.items()}
        print(len(cs), "cases,", len(units), "permutations")
        strict, fast = build(units, MG.STRICT, tmp, "strict"), build(units, MG.CONTRACTED, tmp, "fast")
        for ci, c in enumerate(cs):
            a, b = run_case(strict, c, keys), run_case(fast, c, keys)
            assert np.isfinite(a).all(), c["name"]
            geom = M.has_fragment(c)
            diff = 0.0
            for name in M.output_names(c):
                o, n = OFFSETS[name], M.channels_of(name)
                diff = max(diff, float(util.rel_err(b[..., o:o + n], a[..., o:o + n]).max()))
                fx[f"c{ci}_{name}"] = np.ascontiguousarray(np.moveaxis(a[..., o:o + n], -1, 0))  # (channel planes: a constant channel packs to nothing)
            worst = max(worst, diff)
            print(f"{c['name']:34s} {a.shape[1]}x{a.shape[0]}  fragments {int(geom.sum()):5d}  mean base colour {a[geom][:, :3].mean():7.4f}  strict vs contracted: max rel {diff:.3e}")
            assert diff <= 0.5e-3, f"{c['name']}: the reference's own two builds differ by {diff:.3e} > 0.5e-3 -- move the case"
    fx["strict_vs_contracted"] = np.array(worst)
    shade_cases(cs, fx)
    path = os.path.join(HERE, "material_fetch_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes; largest strict-vs-contracted difference", worst)
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
