// TEST INFRASTRUCTURE ONLY.  The per-pixel body of pbr_shade_layers_kernel (diligentfx_amd/csrc/mifx_pbr_layers.h), compiled for the HOST by the test suite so that the
// kernel's arithmetic can be compared with the reference (oracle/_ref) where there is no GPU: `hipcc --cuda-host-only`, with __device__ redefined to "host and device" so
// that the MIFX_D functions of the kernel headers become callable here.  This is the kernel's source, not a second implementation -- and not a product path: nothing in
// diligentfx_amd/ builds, loads or calls it (the product fails without its HIP library and a device).  What the host build does not show: the device's own division /
// square-root sequences (fdiv, fsqrt: plain IEEE operations here) and the device math library; the -m gpu tests do.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "mifx_pbr_layers.h"
#include <type_traits>

using namespace mifx;

extern "C" {
struct host_plane { float* data; int w, h, c; };
// planes: base colour, normal, material (c = 4), depth (c = 1), emissive (c = 4) or null, occlusion (c = 1) or null, out radiance, out specular IBL (c = 4) or null;
// layers: clear coat, clear-coat normal or null, sheen, anisotropy, tangent or null, iridescence (c = 4), transmission (c = 1); luts: BRDF (c = 2 or 4), albedo scaling, Charlie;
// cubes: faces of a level stacked vertically (6n x n, c = 4), irradiance level 0 and `pref_levels` levels of the prefiltered map; attribs = mifx_pbr_shade_attribs
int mifx_host_pbr_shade_layers(const host_plane* planes, const host_plane* layers, const host_plane* luts, const host_plane* irradiance, const host_plane* prefiltered, int pref_levels,
                               const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, const float* background, unsigned flags, float iridescence_ior,
                               float anisotropy_rotation, int reversed_depth, const host_plane* shadow_slices, int shadow_slice_count, const mifx_pbr_shadow_map_info* shadow_infos,
                               int shadow_info_count, int pcf_filter_size, int generic_instance) // generic_instance: the run-time-set instance whatever the set; shadow_slices: `shadow_slice_count` slices of one contiguous (slices, h, w) array, or null
{
    auto img = [](const host_plane& p) { return p.data ? Img{reinterpret_cast<unsigned char*>(p.data), p.w, p.h, p.w * p.c * 4, 0, 0} : Img{}; };
    auto lutk = [](const host_plane& p) { return LutK{p.data, p.w, p.h, p.w * p.c, p.c}; };
    const Img bc = img(planes[0]), nrm = img(planes[1]), mat = img(planes[2]), depth = img(planes[3]), emis = img(planes[4]), occ = img(planes[5]), outR = img(planes[6]), outS = img(planes[7]);
    LayersK ly{};
    set_layer_scalars(ly, flags, iridescence_ior, anisotropy_rotation);
    ly.clearcoat = img(layers[0]); ly.clearcoatNormal = img(layers[1]); ly.sheen = img(layers[2]); ly.anisotropy = img(layers[3]); ly.tangent = img(layers[4]);
    ly.iridescence = img(layers[5]); ly.transmission = img(layers[6]);
    ly.hasClearcoatNormal = layers[1].data != nullptr;
    ly.hasTangent = layers[4].data != nullptr;
    const LutK lut = lutk(luts[0]);
    if (luts[1].data) ly.albedoScaling = lutk(luts[1]);
    if (luts[2].data) ly.charlie = lutk(luts[2]);
    const ShadeK k = make_shadek(*a, background);
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
    // the instance the launcher would take for this set (launch_pbr_shade_layers, pbr.hip): each single layer and all five fold their branches at compile time
    auto run = [&](auto set_tag, auto shadow_tag) {
        constexpr unsigned SET = decltype(set_tag)::value;
        constexpr bool SHADOWS = decltype(shadow_tag)::value;
#pragma omp parallel for schedule(dynamic, 4)
        for (int y = 0; y < outR.h; ++y)
            for (int x = 0; x < outR.w; ++x)
            {
                v4 color, spec;
                pbr_shade_layers_pixel<false, SET, SHADOWS>(x, y, bc, nrm, mat, depth, emis, occ, lut, reinterpret_cast<const v4*>(irradiance->data), irradiance->w, pref, prefiltered[0].w,
                                                            pref_levels, cam, k, ly, emis.p != nullptr, occ.p != nullptr, sh, color, spec);
                st<v4>(outR, x, y, color);
                if (outS.p != nullptr) st<v4>(outS, x, y, spec);
            }
    };
    auto run_set = [&](auto set_tag) {
        if (shadow_slices != nullptr) run(set_tag, std::true_type{});
        else run(set_tag, std::false_type{});
    };
    switch (generic_instance ? 0xffffu : flags)
    {
        case 1u: run_set(std::integral_constant<unsigned, 1u>{}); break;
        case 2u: run_set(std::integral_constant<unsigned, 2u>{}); break;
        case 4u: run_set(std::integral_constant<unsigned, 4u>{}); break;
        case 8u: run_set(std::integral_constant<unsigned, 8u>{}); break;
        case 16u: run_set(std::integral_constant<unsigned, 16u>{}); break;
        case 31u: run_set(std::integral_constant<unsigned, 31u>{}); break;
        default: run_set(std::integral_constant<unsigned, kLayersRuntime>{}); break;
    }
    return 0;
}
}
