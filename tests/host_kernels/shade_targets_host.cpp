// TEST INFRASTRUCTURE ONLY.  The per-pixel body of pbr_shade_targets_kernel (diligentfx_amd/csrc/mifx_pbr_output.h: the layered shade, the output stage and the USD renderer's
// footer behind it -- PSOut.Color and the Normal / BaseColor / Material / IBL targets), compiled for the HOST by the test suite as shade_output_host.cpp compiles the output
// stage: `hipcc --cuda-host-only`, __device__ redefined to "host and device".  The kernel's source, not a second implementation, and not a product path.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "mifx_pbr_output.h"
#include <cmath>
#include <cstring>
#include <type_traits>

using namespace mifx;

extern "C" {
struct host_plane { float* data; int w, h, c; };
// planes: base colour, normal, material (c = 4), depth (c = 1), emissive (c = 4) or null, occlusion (c = 1) or null, out colour, (unused), motion (c = 2) or null,
//         mesh normal (c = 4) or null, then the four targets (c = 4): normal, base colour, material, IBL;
// layers, luts, cubes, shadows: as mifx_host_pbr_shade_layers (layers_host.cpp); flags = the layer set (0: none); desc: its `renderer` must be set, its planes are ignored
int mifx_host_pbr_shade_targets(const host_plane* planes, const host_plane* layers, const host_plane* luts, const host_plane* irradiance, const host_plane* prefiltered, int pref_levels,
                               const mifx_camera_attribs* camera, const mifx_pbr_shade_attribs* a, const float* background, unsigned flags, float iridescence_ior,
                               float anisotropy_rotation, int reversed_depth, const host_plane* shadow_slices, int shadow_slice_count, const mifx_pbr_shadow_map_info* shadow_infos,
                               int shadow_info_count, int pcf_filter_size, const mifx_pbr_shade_output_desc* desc)
{
    auto img = [](const host_plane& p) { return p.data ? Img{reinterpret_cast<unsigned char*>(p.data), p.w, p.h, p.w * p.c * 4, 0, 0} : Img{}; };
    auto lutk = [](const host_plane& p) { return LutK{p.data, p.w, p.h, p.w * p.c, p.c}; };
    const Img bc = img(planes[0]), nrm = img(planes[1]), mat = img(planes[2]), depth = img(planes[3]), emis = img(planes[4]), occ = img(planes[5]), outC = img(planes[6]);
    const Img tgN = img(planes[10]), tgB = img(planes[11]), tgM = img(planes[12]), tgI = img(planes[13]);
    const Img motion = img(planes[8]), meshNormal = img(planes[9]);
    LayersK ly{};
    ly.flags = flags;
    ly.iridescenceIor = iridescence_ior;
    ly.rotationCos = std::cos(anisotropy_rotation);
    ly.rotationSin = std::sin(anisotropy_rotation);
    ly.clearcoat = img(layers[0]); ly.clearcoatNormal = img(layers[1]); ly.sheen = img(layers[2]); ly.anisotropy = img(layers[3]); ly.tangent = img(layers[4]);
    ly.iridescence = img(layers[5]); ly.transmission = img(layers[6]);
    ly.hasClearcoatNormal = layers[1].data != nullptr;
    ly.hasTangent = layers[4].data != nullptr;
    const LutK lut = lutk(luts[0]);
    if (luts[1].data) ly.albedoScaling = lutk(luts[1]);
    if (luts[2].data) ly.charlie = lutk(luts[2]);
    ShadeK k{};
    k.iblScale[0] = a->IBLScale[0]; k.iblScale[1] = a->IBLScale[1]; k.iblScale[2] = a->IBLScale[2];
    k.occlusionStrength = a->OcclusionStrength; k.emissionScale = a->EmissionScale; k.prefilteredCubeLastMip = a->PrefilteredCubeLastMip;
    k.lightCount = a->LightCount; k.workflow = a->Workflow;
    for (int i = 0; i < a->LightCount; ++i) k.lights[i] = a->Lights[i];
    for (int i = 0; i < 4; ++i) k.background[i] = background[i];
    CamK cam{}; // make_camk (mifx_core.cpp)
    std::memcpy(cam.view.m, camera->mView, 64); std::memcpy(cam.proj.m, camera->mProj, 64); std::memcpy(cam.viewProj.m, camera->mViewProj, 64);
    std::memcpy(cam.viewInv.m, camera->mViewInv, 64); std::memcpy(cam.viewProjInv.m, camera->mViewProjInv, 64);
    for (int i = 0; i < 3; ++i) cam.pos[i] = camera->f4Position[i];
    cam.vw = camera->f4ViewportSize[0]; cam.vh = camera->f4ViewportSize[1]; cam.ivw = camera->f4ViewportSize[2]; cam.ivh = camera->f4ViewportSize[3];
    cam.reversedDepth = reversed_depth;
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
    // the constants of launch_pbr_shade_layers' output stage (pbr.hip)
    const mifx_pbr_shade_output_desc& d = *desc;
    const mifx_pbr_renderer_shader_parameters& r = *d.renderer;
    OutputK o{};
    o.debugView = d.debug_view; o.loadingAnimation = d.loading_animation; o.alphaMode = d.alpha_mode; o.unlit = d.unlit != 0;
    o.srgb = (d.flags & MIFX_PBR_SHADE_OUTPUT_FLAG_CONVERT_OUTPUT_TO_SRGB) != 0u;
    o.hasMotion = motion.p != nullptr; o.hasMeshNormal = meshNormal.p != nullptr;
    o.alphaMaskCutoff = d.alpha_mask_cutoff;
    o.tm = ToneMapK{r.MiddleGray, r.WhitePoint, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, r.AverageLogLum, 0};
    for (int i = 0; i < 4; ++i) o.highlight[i] = r.HighlightColor[i];
    o.time = r.Time; o.worldScale = r.LoadingAnimation.WorldScale; o.speed = r.LoadingAnimation.Speed;
    o.factor = d.loading_animation == MIFX_PBR_LOADING_ANIMATION_TRANSITIONING ? r.LoadingAnimation.Factor : 1.0f;
    for (int i = 0; i < 3; ++i) { o.color0[i] = r.LoadingAnimation.Color0[i]; o.color1[i] = r.LoadingAnimation.Color1[i]; }
    o.sceneNearZ = camera->fSceneNearZ; o.sceneFarZ = camera->fSceneFarZ;

    auto run = [&](auto tm_tag, auto shadow_tag) {
        constexpr int  TM = decltype(tm_tag)::value;
        constexpr bool SHADOWS = decltype(shadow_tag)::value;
#pragma omp parallel for schedule(dynamic, 4)
        for (int y = 0; y < outC.h; ++y)
            for (int x = 0; x < outC.w; ++x)
            {
                v4 color;
                ShadeTargets t;
                pbr_shade_targets_pixel<false, SHADOWS, TM>(x, y, bc, nrm, mat, depth, emis, occ, lut, reinterpret_cast<const v4*>(irradiance->data), irradiance->w, pref, prefiltered[0].w,
                                                            pref_levels, cam, k, ly, emis.p != nullptr, occ.p != nullptr, sh, o, r.LoadingAnimation.Factor, motion, meshNormal, color, t);
                st<v4>(outC, x, y, color);
                st<v4>(tgN, x, y, t.normal);
                st<v4>(tgB, x, y, t.baseColor);
                st<v4>(tgM, x, y, t.material);
                st<v4>(tgI, x, y, t.ibl);
            }
    };
#define MIFX_HOST_INSTANCE(TM)                                                              \
    if (shadow_slices != nullptr) run(std::integral_constant<int, TM>{}, std::true_type{}); \
    else run(std::integral_constant<int, TM>{}, std::false_type{})
    if (d.tone_mapping_mode < 0 || d.tone_mapping_mode > 11) return 1;
    MIFX_TONEMAP_DISPATCH(d.tone_mapping_mode, MIFX_HOST_INSTANCE)
#undef MIFX_HOST_INSTANCE
    return 0;
}
}
