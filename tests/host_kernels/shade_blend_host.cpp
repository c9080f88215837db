// TEST INFRASTRUCTURE ONLY.  The per-pixel body of oit_shade_blend_kernel (diligentfx_amd/csrc/mifx_oit_shade.h: one transparent draw shaded and blended) compiled for the
// HOST (see layers_host.cpp for the method), inside the frame the chain runs around it: oit_clear_kernel, one oit_update_kernel per slice, oit_attenuate_kernel, then one
// oit_px_shade_blend pass per slice.  What it is compared with is the composition of the two existing host compilations: layers_host.cpp shades every slice into two
// planes, oit_host.cpp runs the sequence on them.  Every plane is addressed through its own pitch, so a caller may hand in pitched views (shade_blend_sanitize_main.cpp).
// Nothing in diligentfx_amd/ builds, loads or calls this.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "mifx_oit_shade.h"

using namespace mifx;

extern "C" {
struct host_plane { float* data; int w, h, c; };
struct host_pitched { float* data; int pitch; }; // pitch in bytes
struct host_tslice { host_pitched base, normal, material, depth, alpha; }; // alpha.data may be null

// layers: H x W x K words, tail: H x W x 2 (both tightly packed, the object's own buffers); targets: colour, base colour, material, IBL, blended in place; opaque.data may be
// null; lut: the BRDF table (c = 2 or 4); cubes as layers_host.cpp takes them.  No material layers, no shadow maps: the empty set, as the end-to-end fixture shades.
// Returns 0, or -1 for a bad K / L.
int mifx_host_transparency(int K, int W, int H, int L, const host_tslice* slices, host_pitched opaque, const host_plane* lut_plane, const host_plane* irradiance,
                           const host_plane* prefiltered, int pref_levels, const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, int reversed_depth, uint32_t* layers,
                           float* tail, const host_pitched* targets)
{
    if (K < 1 || K > MIFX_OIT_MAX_LAYERS || L < 0 || L > MIFX_OIT_MAX_SLICES) return -1;
    auto bytes = [](const void* p) { return reinterpret_cast<unsigned char*>(const_cast<void*>(p)); };
    auto img   = [&](const host_pitched& p) { return p.data ? Img{bytes(p.data), W, H, p.pitch, 0, 0} : Img{}; };
    const OitK k{bytes(layers), bytes(tail), opaque.data ? bytes(opaque.data) : nullptr, W, H, K, W * 8, opaque.pitch, make_oitcamk(*camera)};
    const OitTargetsK t{img(targets[0]), img(targets[1]), img(targets[2]), img(targets[3])};
    const LutK lut{lut_plane->data, lut_plane->w, lut_plane->h, lut_plane->w * lut_plane->c, lut_plane->c};
    const ShadeK sk = make_shadek(*a, nullptr);
    const CamK cam = make_camk(*camera, reversed_depth != 0);
    const LayersK ly{};
    const ShadowK sh{};
    const v4* pref[12] = {};
    for (int l = 0; l < pref_levels && l < 12; ++l) pref[l] = reinterpret_cast<const v4*>(prefiltered[l].data);
    auto every_pixel = [&](auto&& px) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) px(x, y);
    };
    auto layer_slice = [&](const host_tslice& s) { return OitSliceK{bytes(s.depth.data), bytes(s.base.data), nullptr, nullptr, nullptr, nullptr, s.depth.pitch, s.base.pitch, 0, 0, 0, 0}; };
    every_pixel([&](int x, int y) { oit_px_clear(k, x, y); });
    for (int l = 0; l < L; ++l) every_pixel([&](int x, int y) { oit_px_update(k, layer_slice(slices[l]), x, y); });
    every_pixel([&](int x, int y) { oit_px_attenuate(k, t, x, y); });
    for (int l = 0; l < L; ++l)
    {
        const host_tslice&   s = slices[l];
        const OitShadeSliceK slice{img(s.base), img(s.normal), img(s.material), img(s.depth), Img{}, Img{}, img(s.alpha), 0, 0, s.alpha.data != nullptr};
        every_pixel([&](int x, int y) {
            oit_px_shade_blend<false, false>(k, slice, t, lut, reinterpret_cast<const v4*>(irradiance->data), irradiance->w, pref, prefiltered[0].w, pref_levels, cam, sk, ly, sh, x, y);
        });
    }
    return 0;
}

// One launch of oit_shade_blend_kernel on the launcher's own OitK / OitTargetsK, in place on the memory they name (tests/cpu_product/device.py: the handler of the
// host-only build), with every other input as mifx_host_pbr_shade_layers (layers_host.cpp) takes it -- tightly packed planes, the layer set a run-time mask as in the kernel.
// planes: base colour, normal, material (c = 4), depth (c = 1), emissive (c = 4) or null, occlusion (c = 1) or null, colour alpha (c = 1) or null.
int mifx_host_oit_shade_blend_launch(const OitK* k, const OitTargetsK* t, const host_plane* planes, const host_plane* layers, const host_plane* luts, const host_plane* irradiance,
                                     const host_plane* prefiltered, int pref_levels, const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, unsigned flags,
                                     float iridescence_ior, float anisotropy_rotation, int reversed_depth, const host_plane* shadow_slices, int shadow_slice_count,
                                     const mifx_pbr_shadow_map_info* shadow_infos, int shadow_info_count, int pcf_filter_size)
{
    auto img  = [](const host_plane& p) { return p.data ? Img{reinterpret_cast<unsigned char*>(p.data), p.w, p.h, p.w * p.c * 4, 0, 0} : Img{}; };
    auto lutk = [](const host_plane& p) { return LutK{p.data, p.w, p.h, p.w * p.c, p.c}; };
    const OitShadeSliceK slice{img(planes[0]), img(planes[1]), img(planes[2]), img(planes[3]), img(planes[4]), img(planes[5]), img(planes[6]),
                               planes[4].data != nullptr, planes[5].data != nullptr, planes[6].data != nullptr};
    LayersK ly{};
    set_layer_scalars(ly, flags, iridescence_ior, anisotropy_rotation);
    ly.clearcoat = img(layers[0]); ly.clearcoatNormal = img(layers[1]); ly.sheen = img(layers[2]); ly.anisotropy = img(layers[3]); ly.tangent = img(layers[4]);
    ly.iridescence = img(layers[5]); ly.transmission = img(layers[6]);
    ly.hasClearcoatNormal = layers[1].data != nullptr;
    ly.hasTangent = layers[4].data != nullptr;
    const LutK lut = lutk(luts[0]);
    if (luts[1].data) ly.albedoScaling = lutk(luts[1]);
    if (luts[2].data) ly.charlie = lutk(luts[2]);
    const ShadeK sk = make_shadek(*a, nullptr);
    const CamK cam = make_camk(*camera, reversed_depth != 0);
    ShadowK sh{};
    if (shadow_slices != nullptr)
    {
        sh.data = reinterpret_cast<const unsigned char*>(shadow_slices[0].data);
        sh.w = shadow_slices[0].w; sh.h = shadow_slices[0].h; sh.slices = shadow_slice_count; sh.pitch = sh.w * 4;
        sh.slicePitch = static_cast<unsigned long long>(sh.pitch) * sh.h;
        sh.pcf = pcf_filter_size;
        for (int i = 0; i < shadow_info_count && i < MIFX_PBR_MAX_SHADOW_MAPS; ++i) sh.info[i] = shadow_infos[i];
    }
    const v4* pref[12] = {};
    for (int l = 0; l < pref_levels && l < 12; ++l) pref[l] = reinterpret_cast<const v4*>(prefiltered[l].data);
    for (int y = 0; y < k->h; ++y)
        for (int x = 0; x < k->w; ++x)
        {
            if (shadow_slices != nullptr)
                oit_px_shade_blend<false, true>(*k, slice, *t, lut, reinterpret_cast<const v4*>(irradiance->data), irradiance->w, pref, prefiltered[0].w, pref_levels, cam, sk, ly, sh, x, y);
            else
                oit_px_shade_blend<false, false>(*k, slice, *t, lut, reinterpret_cast<const v4*>(irradiance->data), irradiance->w, pref, prefiltered[0].w, pref_levels, cam, sk, ly, sh, x, y);
        }
    return 0;
}
}
