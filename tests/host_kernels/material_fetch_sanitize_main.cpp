// TEST INFRASTRUCTURE ONLY.  A stand-alone program around the host compilation of the material fetch's body (material_fetch_host.cpp), built by
// tests/test_material_fetch_cpu.py with -fsanitize=address,undefined for the host alone: the body over pitched, offset planes and over hostile interpolants -- NaN, +-inf,
// 1e30 and negative texture coordinates, a texture slice of 1e9, garbage in the index plane, a mip bias of +-100 -- with and without the atlas, from RGBA32_FLOAT and
// RGBA8_UNORM textures.  Every plane is its own heap allocation of exactly its size, so an access outside one is a report.  The program checks that every output texel is
// finite or untouched and that the padding of the pitched planes is untouched; prints one line a run and "ok <runs>".
#include "mifx.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

extern "C" {
struct host_plane { float* data; int w, h, c; int pitch_bytes; };
struct host_texture { const void* data; int w, h, slices, mips, rgba8; unsigned long long slice_pitch_bytes; };
int mifx_host_material_fetch(const host_plane* interpolants, const host_plane* outputs, const mifx_pbr_material* materials, int material_count, const host_texture* textures,
                             int texture_count, unsigned layer_flags, unsigned flags, float mip_bias, const mifx_camera_attribs* camera, int reversed_depth);
}

namespace
{
constexpr float kSentinel = -7.25f;
constexpr int   W = 23, H = 14, kPad = 3, kLead = 1; // a pitched plane: kLead texels before each row's view, kPad texels in all beside it
unsigned g_seed = 12345u;
float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return float(g_seed >> 8) * (1.0f / 16777216.0f); }

struct Plane
{
    std::unique_ptr<float[]> mem;
    int c = 0, rowFloats = 0;
    host_plane view{};
    void make(int channels, bool pitched, float fill)
    {
        c = channels;
        rowFloats = (W + (pitched ? kPad : 0)) * c;
        mem.reset(new float[size_t(rowFloats) * H]);
        for (int i = 0; i < rowFloats * H; ++i) mem[size_t(i)] = fill;
        view = host_plane{mem.get() + (pitched ? kLead * c : 0), W, H, c, rowFloats * 4};
    }
    float& at(int x, int y, int k) { return view.data[size_t(y) * rowFloats + size_t(x) * c + k]; }
    bool padding_is(float v) const
    {
        const long lead = view.data - mem.get();
        for (int y = 0; y < H; ++y)
            for (int i = 0; i < rowFloats; ++i)
                if ((i < lead || i >= lead + W * c) && mem[size_t(y) * rowFloats + i] != v) return false;
        return true;
    }
};
struct Texture
{
    std::unique_ptr<unsigned char[]> mem;
    host_texture desc{};
    void make(int w, int h, int slices, int mips, bool rgba8)
    {
        size_t texels = 0;
        for (int l = 0; l < mips; ++l) texels += size_t((w >> l) > 1 ? (w >> l) : 1) * size_t((h >> l) > 1 ? (h >> l) : 1);
        const size_t ts = rgba8 ? 4 : 16, bytes = texels * ts * size_t(slices);
        mem.reset(new unsigned char[bytes]);
        if (rgba8) for (size_t i = 0; i < bytes; ++i) mem[i] = static_cast<unsigned char>(rnd() * 255.0f);
        else { float* f = reinterpret_cast<float*>(mem.get()); for (size_t i = 0; i < bytes / 4; ++i) f[i] = 0.05f + 0.9f * rnd(); }
        desc = host_texture{mem.get(), w, h, slices, mips, rgba8 ? 1 : 0, texels * ts};
    }
};
mifx_pbr_texture_attribs attribs(int selector, unsigned wrapU, unsigned wrapV, float slice, const float* region)
{
    mifx_pbr_texture_attribs a{};
    a.PackedProps = unsigned(selector + 1) | ((wrapU - 1u) << 3) | ((wrapV - 1u) << 6);
    a.TextureSlice = slice;
    a.UBias = 0.1f; a.VBias = -0.2f;
    a.UVScaleAndRotation[0] = 1.7f; a.UVScaleAndRotation[1] = 0.5f; a.UVScaleAndRotation[2] = -0.4f; a.UVScaleAndRotation[3] = 0.6f;
    for (int i = 0; i < 4; ++i) a.AtlasUVScaleAndBias[i] = region[i];
    return a;
}
mifx_pbr_material material(int variant, int textureCount, float slice)
{
    mifx_pbr_material m{};
    for (int i = 0; i < 4; ++i) { m.basic.BaseColorFactor[i] = 1.0f; m.fallback_color[i] = 0.5f; }
    m.basic.EmissiveFactorR = m.basic.EmissiveFactorG = m.basic.EmissiveFactorB = 1.0f;
    m.basic.NormalScale = 0.8f; m.basic.ClearcoatNormalScale = 0.7f;
    m.basic.SpecularFactorR = m.basic.SpecularFactorG = m.basic.SpecularFactorB = 1.0f;
    m.basic.MetallicFactor = 0.9f; m.basic.RoughnessFactor = 1.1f; m.basic.OcclusionFactor = 0.9f; m.basic.ClearcoatFactor = 0.8f; m.basic.ClearcoatRoughnessFactor = 0.6f;
    m.sheen = {0.9f, 0.6f, 0.3f, 0.7f};
    m.anisotropy = {0.75f, 0.6f, 0.0f, 0.0f};
    m.iridescence = {0.85f, 1.4f, 120.0f, 380.0f};
    m.transmission = {0.4f, 0.0f, 0.0f, 0.0f};
    static const float regions[4][4] = {{0.25f, 0.25f, 0.25f, 0.5f}, {-0.25f, 0.25f, 0.75f, 0.0f}, {0.5f, -0.5f, 0.0f, 1.0f}, {1.0f, 1.0f, 0.0f, 0.0f}};
    for (int s = 0; s < MIFX_PBR_TEXTURE_COUNT; ++s)
    {
        const bool present = variant == 0 || (s % 3) != 1; // (the second material lacks every third map; PHYS_DESC is one of them: METALLIC and ROUGHNESS are read)
        m.texture[s]  = present ? (s + variant) % textureCount : -1;
        m.textures[s] = attribs((s + variant) % 3 == 2 ? 1 : ((s == MIFX_PBR_TEXTURE_OCCLUSION && variant) ? -1 : 0), (s & 1) ? 3u : 1u, (s & 2) ? 3u : 1u, slice, regions[(s + variant) % 4]);
    }
    return m;
}
mifx_camera_attribs camera()
{
    mifx_camera_attribs c{};
    c.f4Position[1] = 1.0f; c.f4Position[2] = -4.0f; c.f4Position[3] = 1.0f;
    c.f4ViewportSize[0] = float(W); c.f4ViewportSize[1] = float(H); c.f4ViewportSize[2] = 1.0f / float(W); c.f4ViewportSize[3] = 1.0f / float(H);
    c.fHandness = 1.0f;
    // an inverse view-projection that is affine in (x, y) and projective in depth
    const float inv[16] = {2.0f, 0.1f, 0.0f, 0.0f, 0.2f, 1.5f, 0.1f, 0.0f, 0.0f, 0.0f, 0.0f, -0.9f, 0.3f, 1.0f, 1.0f, 1.0f};
    std::memcpy(c.mViewProjInv, inv, sizeof(inv));
    return c;
}

int run(const char* what, bool pitched, bool hostile, unsigned flags, float mipBias, float slice)
{
    Plane in[7], out[11];
    const int inC[7] = {1, 2, 2, 4, 4, 1, 1}, outC[11] = {4, 4, 4, 4, 1, 4, 4, 4, 4, 4, 1};
    for (int i = 0; i < 7; ++i) in[i].make(inC[i], pitched, 0.0f);
    for (int i = 0; i < 11; ++i) out[i].make(outC[i], pitched, kSentinel);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[8] = {nan, inf, -inf, 1e30f, -1e30f, -3.75f, 123456.7f, -0.0f};
    const float badIndex[6] = {nan, -5.0f, 1e9f, inf, 2.0f, -1.0f};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
        {
            const bool background = (x * 7 + y * 3) % 11 == 0;
            in[0].at(x, y, 0) = background ? 1.0f : 0.3f + 0.02f * float(x) + 0.015f * float(y) + 0.01f * rnd();
            for (int k = 0; k < 2; ++k)
            {
                in[1].at(x, y, k) = 0.13f * float(x) - 0.07f * float(y) * float(k + 1) + 0.2f;
                in[2].at(x, y, k) = -0.4f + 0.31f * float(y) + 0.05f * float(x) * float(k);
            }
            if (hostile && (x + y) % 2 == 0)
            {
                in[1].at(x, y, (x / 2) % 2) = bad[(x + 3 * y) % 8];
                in[2].at(x, y, (y / 2) % 2) = bad[(5 * x + y) % 8];
            }
            in[3].at(x, y, 0) = 0.2f; in[3].at(x, y, 1) = -0.1f; in[3].at(x, y, 2) = (x % 5 == 0) ? 0.0f : -0.97f; in[3].at(x, y, 3) = 0.0f;
            if (x % 5 == 0) { in[3].at(x, y, 0) = 0.0f; in[3].at(x, y, 1) = 0.0f; } // (a zero mesh normal: the position gradients)
            for (int k = 0; k < 4; ++k) in[4].at(x, y, k) = 0.5f + 0.5f * rnd();
            in[5].at(x, y, 0) = (x + y) % 3 == 0 ? -1.0f : 1.0f;
            in[6].at(x, y, 0) = hostile && (x * 5 + y) % 4 == 0 ? badIndex[(x + y) % 6] : float((x / 3 + y / 2) % 2);
        }
    Texture tex[4];
    tex[0].make(16, 16, 2, 5, false);
    tex[1].make(13, 5, 3, 3, true); // not a power of two
    tex[2].make(64, 64, 1, 5, true);
    tex[3].make(1, 1, 1, 1, false);
    host_texture descs[4] = {tex[0].desc, tex[1].desc, tex[2].desc, tex[3].desc};
    const mifx_pbr_material materials[2] = {material(0, 4, slice), material(1, 4, -slice)};
    const mifx_camera_attribs cam = camera();
    host_plane ip[7], op[11];
    for (int i = 0; i < 7; ++i) ip[i] = in[i].view;
    for (int i = 0; i < 11; ++i) op[i] = out[i].view;
    if (mifx_host_material_fetch(ip, op, materials, 2, descs, 4, 31u, flags, mipBias, &cam, 0) != 0) return 1;
    long stored = 0, untouched = 0;
    for (int i = 0; i < 11; ++i)
    {
        if (!out[i].padding_is(kSentinel)) { std::printf("FAILED %s: the padding of output plane %d was written\n", what, i); return 1; }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int k = 0; k < outC[i]; ++k)
                {
                    const float v = out[i].at(x, y, k);
                    if (!std::isfinite(v)) { std::printf("FAILED %s: output plane %d holds a non-finite value at (%d, %d)\n", what, i, x, y); return 1; }
                    (v == kSentinel ? untouched : stored) += 1;
                }
    }
    for (int i = 0; i < 7; ++i)
        if (!in[i].padding_is(0.0f)) { std::printf("FAILED %s: an interpolant plane was written\n", what); return 1; }
    if (stored == 0 || untouched == 0) { std::printf("FAILED %s: %ld values stored, %ld untouched\n", what, stored, untouched); return 1; }
    std::printf("run %s: %ld values stored, %ld untouched\n", what, stored, untouched);
    return 0;
}
}

int main()
{
    const unsigned T = MIFX_MATERIAL_FETCH_FLAG_TEXCOORD_TRANSFORM, S = MIFX_MATERIAL_FETCH_FLAG_SRGB_TO_LINEAR, A = MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS;
    int runs = 0;
    struct { const char* what; bool pitched, hostile; unsigned flags; float bias, slice; } const all[] = {
        {"packed", false, false, S, 0.0f, 1.0f},
        {"pitched and offset", true, false, T | S, 0.5f, 1.0f},
        {"pitched and offset, atlas", true, false, A | T, -0.5f, 0.0f},
        {"hostile interpolants", true, true, T | S, 100.0f, 1e9f},
        {"hostile interpolants, mip bias -100", false, true, S, -100.0f, -1e9f},
        {"hostile interpolants, atlas", true, true, A | T | S, 100.0f, 1e9f},
        {"hostile interpolants, atlas, mip bias -100", false, true, A, -100.0f, std::numeric_limits<float>::quiet_NaN()},
    };
    for (const auto& r : all)
    {
        if (run(r.what, r.pitched, r.hostile, r.flags, r.bias, r.slice) != 0) return 1;
        ++runs;
    }
    std::printf("ok %d\n", runs);
    return 0;
}
