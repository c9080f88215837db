// TEST INFRASTRUCTURE ONLY.  A stand-alone program around tests/host_kernels/shade_targets_host.cpp for a host-only build with the address and undefined-behaviour sanitizers: it
// reads the fixture's frame from the file shade_targets_util.dump_frame wrote, runs the host compilation of the footer's body over it for a few descs, and prints a checksum
// of every output.  Never loaded into Python; the sanitizer's runtime is linked into the program itself.
#include "mifx.h"
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
struct host_plane { float* data; int w, h, c; };
int mifx_host_pbr_shade_targets(const host_plane* planes, const host_plane* layers, const host_plane* luts, const host_plane* irradiance, const host_plane* prefiltered, int pref_levels,
                                const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, const float* background, unsigned flags, float iridescence_ior,
                                float anisotropy_rotation, int reversed_depth, const host_plane* shadow_slices, int shadow_slice_count, const mifx_pbr_shadow_map_info* shadow_infos,
                                int shadow_info_count, int pcf_filter_size, const mifx_pbr_shade_output_desc* desc);
}

namespace
{
struct Blob
{
    int                h = 0, w = 0, c = 0;
    std::vector<float> v;
    host_plane plane() { return host_plane{v.empty() ? nullptr : v.data(), w, h, c}; }
};
bool read_blob(std::FILE* f, Blob& b)
{
    int hdr[3];
    if (std::fread(hdr, sizeof(int), 3, f) != 3 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0 || size_t(hdr[0]) * hdr[1] * hdr[2] > (1u << 26)) return false;
    b.h = hdr[0]; b.w = hdr[1]; b.c = hdr[2];
    b.v.resize(size_t(b.h) * b.w * b.c);
    return b.v.empty() || std::fread(b.v.data(), sizeof(float), b.v.size(), f) == b.v.size();
}
double checksum(const std::vector<float>& v)
{
    double s = 0.0;
    for (float x : v) s += double(x);
    return s;
}
}

// file: int32 count, then `count` planes (int32 h, w, c; floats):  0-7 base colour, normal, material, depth, emissive, occlusion, motion, mesh normal;  8-14 the layer planes in
// the order of layers_util.LAYER_ORDER;  15-17 BRDF table, albedo scaling, Charlie;  18 irradiance;  19 shadow slices (h = slices * rows);  20 shadow infos (24 floats a row);
// 21 camera and 22 shade attribs as raw floats;  23.. the prefiltered levels
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int count = 0;
    if (std::fread(&count, sizeof(int), 1, f) != 1 || count < 24 || count > 23 + 12) return 2;
    std::vector<Blob> b(count);
    for (Blob& x : b)
        if (!read_blob(f, x)) return 2;
    std::fclose(f);
    if (b[21].v.size() * 4 < sizeof(mifx_camera_attribs) || b[22].v.size() * 4 < sizeof(mifx_pbr_shade_attribs)) return 2;
    mifx_camera_attribs    cam;
    mifx_pbr_shade_attribs sa;
    std::memcpy(&cam, b[21].v.data(), sizeof(cam));
    std::memcpy(&sa, b[22].v.data(), sizeof(sa));
    const int H = b[3].h, W = b[3].w, levels = count - 23;
    const int slices = int(b[20].h), rows = b[19].h / (slices > 0 ? slices : 1);
    host_plane shadow{b[19].v.data(), b[19].w, rows, 1};
    std::vector<host_plane> pref;
    for (int l = 0; l < levels; ++l) pref.push_back(b[23 + l].plane());
    host_plane irr = b[18].plane();
    const float background[4] = {0.02f, 0.03f, 0.05f, 0.0f};
    mifx_pbr_renderer_shader_parameters r{};
    r.AverageLogLum = 0.35f; r.MiddleGray = 0.18f; r.WhitePoint = 3.0f; r.Time = 1.7f;
    r.HighlightColor[0] = 0.9f; r.HighlightColor[1] = 0.6f; r.HighlightColor[2] = 0.1f; r.HighlightColor[3] = 0.35f;
    r.LoadingAnimation.Factor = 0.4f; r.LoadingAnimation.WorldScale = 1.5f; r.LoadingAnimation.Speed = 0.9f;
    struct Run { unsigned flags; int tm, anim, alpha, view, unlit; bool ccNormal; };
    const Run runs[] = {{31u, 4, 2, 2, 0, 0, true}, {31u, 0, 1, 1, 19, 0, false}, {1u, 0, 0, 0, 0, 0, true}, {0u, 0, 2, 0, 0, 1, true}};
    for (const Run& run : runs)
    {
        std::vector<float> out[5];
        for (auto& o : out) o.assign(size_t(H) * W * 4, -1.0f);
        auto op = [&](int i) { return host_plane{out[i].data(), W, H, 4}; };
        host_plane planes[14] = {b[0].plane(), b[1].plane(), b[2].plane(), b[3].plane(), b[4].plane(), b[5].plane(), op(0), host_plane{nullptr, 0, 0, 0},
                                 b[6].plane(), b[7].plane(), op(1), op(2), op(3), op(4)};
        host_plane layers[7];
        for (int i = 0; i < 7; ++i) layers[i] = b[8 + i].plane();
        if (!run.ccNormal) layers[1] = host_plane{nullptr, 0, 0, 0};
        host_plane luts[3] = {b[15].plane(), b[16].plane(), b[17].plane()};
        mifx_pbr_shade_output_desc d{};
        d.renderer = &r; d.debug_view = run.view; d.tone_mapping_mode = run.tm; d.loading_animation = run.anim; d.alpha_mode = run.alpha; d.alpha_mask_cutoff = 0.5f;
        d.unlit = run.unlit; d.flags = run.tm ? 1u : 0u;
        const int rc = mifx_host_pbr_shade_targets(planes, layers, luts, &irr, pref.data(), levels, &cam, &sa, background, run.flags, 1.33f, 0.7f, 0, &shadow, slices,
                                                   reinterpret_cast<const mifx_pbr_shadow_map_info*>(b[20].v.data()), slices, 3, &d);
        if (rc != 0) return 3;
        std::printf("flags %2u tm %d anim %d alpha %d view %2d unlit %d:", run.flags, run.tm, run.anim, run.alpha, run.view, run.unlit);
        for (auto& o : out) std::printf(" %.6f", checksum(o));
        std::printf("\n");
    }
    return 0;
}
