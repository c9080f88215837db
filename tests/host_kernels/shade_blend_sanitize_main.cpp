// TEST INFRASTRUCTURE ONLY.  A stand-alone program around tests/host_kernels/shade_blend_host.cpp for a host-only build with the address and undefined-behaviour
// sanitizers: it makes hash-made transparent draws of 5 x 3 and 67 x 35 on pitched planes (every plane an allocation of exactly its rows, the row padding filled with a
// sentinel), runs the host compilation of the shade-and-blend body over them inside its frame (clear, updates, attenuation, one pass per slice), checks the padding and
// prints a checksum of every target.  Never loaded into Python; the sanitizer's runtime is linked into the program itself.
#include "mifx.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
struct host_plane { float* data; int w, h, c; };
struct host_pitched { float* data; int pitch; };
struct host_tslice { host_pitched base, normal, material, depth, alpha; };
int mifx_host_transparency(int K, int W, int H, int L, const host_tslice* slices, host_pitched opaque, const host_plane* lut_plane, const host_plane* irradiance,
                           const host_plane* prefiltered, int pref_levels, const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, int reversed_depth, uint32_t* layers,
                           float* tail, const host_pitched* targets);
}

namespace
{
constexpr float kSentinel = 12345.0f;
uint32_t mix(uint32_t x)
{
    x = (x ^ (x >> 16)) * 0x7FEB352Du;
    x = (x ^ (x >> 15)) * 0x846CA68Bu;
    return x ^ (x >> 16);
}
float unit(uint32_t seed, uint32_t i) { return float(mix(i + mix(seed * 0x9E3779B1u)) >> 8) / 16777216.0f; }

// a plane of `c` floats a texel whose rows are `pad` floats longer than the texels need; the allocation ends with the last texel of the last row
struct Pitched
{
    int                W, H, c, pitchF;
    std::vector<float> v;
    Pitched(int w, int h, int ch, int pad) : W(w), H(h), c(ch), pitchF(w * ch + pad), v(size_t(h - 1) * (w * ch + pad) + size_t(w) * ch, kSentinel) {}
    float*       at(int x, int y) { return v.data() + size_t(y) * pitchF + size_t(x) * c; }
    host_pitched view() { return host_pitched{v.data(), pitchF * 4}; }
    bool padding_kept() const
    {
        for (int y = 0; y + 1 < H; ++y)
            for (int i = W * c; i < pitchF; ++i)
                if (v[size_t(y) * pitchF + i] != kSentinel) return false;
        return true;
    }
    double checksum()
    {
        double s = 0.0;
        for (int y = 0; y < H; ++y)
            for (int i = 0; i < W * c; ++i) s += double(*(at(0, y) + i));
        return s;
    }
};

int run(int W, int H, int K, int L, bool withOpaque, bool withAlpha)
{
    const uint32_t seed = uint32_t(W * 131 + H * 7 + K);
    // a camera at (0, 0, -5) looking at the unit cube the identity projection spans: positions are the texel's normalised device coordinates
    mifx_camera_attribs cam{};
    const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(cam.mView, id, 64); std::memcpy(cam.mProj, id, 64); std::memcpy(cam.mViewProj, id, 64); std::memcpy(cam.mViewInv, id, 64); std::memcpy(cam.mViewProjInv, id, 64);
    cam.f4Position[0] = 0.0f; cam.f4Position[1] = 0.0f; cam.f4Position[2] = -5.0f; cam.f4Position[3] = 1.0f;
    cam.f4ViewportSize[0] = float(W); cam.f4ViewportSize[1] = float(H); cam.f4ViewportSize[2] = 1.0f / float(W); cam.f4ViewportSize[3] = 1.0f / float(H);
    cam.fNearPlaneDepth = 0.0f; cam.fFarPlaneDepth = 1.0f;
    mifx_pbr_shade_attribs sa{};
    sa.IBLScale[0] = sa.IBLScale[1] = sa.IBLScale[2] = 1.0f;
    sa.OcclusionStrength = 1.0f; sa.EmissionScale = 1.0f; sa.PrefilteredCubeLastMip = 2.0f;
    sa.Workflow = MIFX_PBR_WORKFLOW_METALLIC_ROUGHNESS;
    sa.LightCount = 1;
    sa.Lights[0].Type = MIFX_PBR_LIGHT_TYPE_DIRECTIONAL;
    sa.Lights[0].DirectionX = 0.3f; sa.Lights[0].DirectionY = -0.8f; sa.Lights[0].DirectionZ = 0.52f;
    sa.Lights[0].IntensityR = sa.Lights[0].IntensityG = sa.Lights[0].IntensityB = 2.0f;
    sa.Lights[0].ShadowMapIndex = -1;
    // the look-ups: an 8 x 8 two-channel BRDF table, a 4^2 irradiance cube, a 4^2 prefiltered cube of three levels (faces stacked vertically, four floats a texel)
    std::vector<float> lutv(8 * 8 * 2), irrv(6 * 4 * 4 * 4);
    for (size_t i = 0; i < lutv.size(); ++i) lutv[i] = unit(seed + 1, uint32_t(i));
    for (size_t i = 0; i < irrv.size(); ++i) irrv[i] = unit(seed + 2, uint32_t(i));
    host_plane lut{lutv.data(), 8, 8, 2}, irr{irrv.data(), 4, 24, 4};
    std::vector<float> prefv[3];
    host_plane         pref[3];
    for (int l = 0; l < 3; ++l)
    {
        const int n = 4 >> l;
        prefv[l].resize(size_t(6) * n * n * 4);
        for (size_t i = 0; i < prefv[l].size(); ++i) prefv[l][i] = unit(seed + 3 + uint32_t(l), uint32_t(i)) * 2.0f;
        pref[l] = host_plane{prefv[l].data(), n, 6 * n, 4};
    }
    std::vector<Pitched> planes;
    planes.reserve(size_t(L) * 5 + 5);
    std::vector<host_tslice> slices(L);
    for (int l = 0; l < L; ++l)
    {
        const uint32_t s = seed + 100u * uint32_t(l + 1);
        Pitched base(W, H, 4, 12), normal(W, H, 4, 4), material(W, H, 4, 20), depth(W, H, 1, 5), alpha(W, H, 1, 3);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
            {
                const uint32_t i = uint32_t(y * W + x);
                const bool     covered = unit(s, i) < 0.6f;
                *depth.at(x, y) = covered ? 0.05f + 0.9f * unit(s + 1, i) : 1.0f;
                *alpha.at(x, y) = unit(s + 2, i);
                float n[3] = {unit(s + 3, i) * 2.0f - 1.0f, unit(s + 4, i) * 2.0f - 1.0f, -0.2f - unit(s + 5, i)};
                const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                for (int c = 0; c < 3; ++c) normal.at(x, y)[c] = n[c] / len;
                normal.at(x, y)[3] = 0.0f;
                for (int c = 0; c < 3; ++c) base.at(x, y)[c] = unit(s + 6 + uint32_t(c), i);
                base.at(x, y)[3] = unit(s + 9, i) < 0.1f ? 0.003f : 0.05f + 0.95f * unit(s + 10, i);
                material.at(x, y)[0] = 0.1f + 0.8f * unit(s + 11, i);
                material.at(x, y)[1] = unit(s + 12, i);
                material.at(x, y)[2] = material.at(x, y)[3] = 0.0f;
            }
        planes.push_back(std::move(base)); planes.push_back(std::move(normal)); planes.push_back(std::move(material)); planes.push_back(std::move(depth)); planes.push_back(std::move(alpha));
        Pitched* p = &planes[planes.size() - 5];
        slices[l] = host_tslice{p[0].view(), p[1].view(), p[2].view(), p[3].view(), withAlpha ? p[4].view() : host_pitched{nullptr, 0}};
    }
    Pitched opaque(W, H, 1, 7);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) *opaque.at(x, y) = 0.35f + 0.6f * unit(seed + 50, uint32_t(y * W + x));
    Pitched      tg[4] = {Pitched(W, H, 4, 8), Pitched(W, H, 4, 16), Pitched(W, H, 4, 4), Pitched(W, H, 4, 28)};
    host_pitched targets[4];
    for (int j = 0; j < 4; ++j)
    {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 4; ++c) tg[j].at(x, y)[c] = float((x * 3 + y * 5 + c * 7 + j) % 17) / 16.0f;
        targets[j] = tg[j].view();
    }
    std::vector<uint32_t> layers(size_t(W) * H * K, 0xDEADBEEFu);
    std::vector<float>    tail(size_t(W) * H * 2, -7.0f);
    const int rc = mifx_host_transparency(K, W, H, L, slices.data(), withOpaque ? opaque.view() : host_pitched{nullptr, 0}, &lut, &irr, pref, 3, &cam, &sa, 0, layers.data(), tail.data(),
                                          targets);
    if (rc != 0) return 3;
    for (Pitched& p : planes)
        if (!p.padding_kept()) return 4;
    if (!opaque.padding_kept()) return 4;
    std::printf("%dx%d K %d L %d opaque %d alpha %d:", W, H, K, L, int(withOpaque), int(withAlpha));
    for (Pitched& t : tg)
    {
        if (!t.padding_kept()) return 4;
        std::printf(" %.6f", t.checksum());
    }
    std::printf("\n");
    return 0;
}
} // namespace

int main()
{
    if (int rc = run(5, 3, 4, 3, true, true)) return rc;
    if (int rc = run(5, 3, 1, 3, false, false)) return rc;
    if (int rc = run(67, 35, 4, 3, true, true)) return rc;
    if (int rc = run(67, 35, 3, 2, false, false)) return rc;
    return 0;
}
