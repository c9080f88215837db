// mifx_pbr_output.h -- the output stage of the reference's forward pixel shader: what `main` of Shaders/PBR/private/RenderPBR.psh does after ResolveLighting (:515-643) --
// in-shader tone mapping, alpha modes, the unlit workflow, the selection highlight, the debug views (:574-613 and GetDebugColor, Shaders/PBR/public/PBR_Shading.fxh:879-989),
// the loading animation (GetLoadingAnimationColor :361-386) and the sRGB output -- on the terms pbr_shade_layers_pixel hands back (mifx_pbr_layers.h: ShadeTerms).
//
// Not the timed path, under the policy of the layered shade: strict fp32, operations in the reference's order, libm sin / pow (the tone map is the existing tone_map<MODE> of
// mifx_tonemap.h).  The view, the animation mode and the alpha mode are uniform run-time values: one pipeline permutation each in the reference (PBR_Renderer.cpp:1414,1439,1479).
#pragma once
#include "mifx_pbr_layers.h"
#include "mifx_tonemap.h"

namespace mifx
{
struct OutputK
{
    int      debugView, loadingAnimation, alphaMode, unlit, srgb; // mifx_pbr_shade_output_desc
    int      hasMotion, hasMeshNormal;
    float    alphaMaskCutoff;
    ToneMapK tm;              // MiddleGray, WhitePoint, fLuminanceSaturation 1, AverageLogLum (RenderPBR.psh:533-540)
    float    highlight[4];    // g_Frame.Renderer.HighlightColor
    float    time, factor, worldScale, speed; // Renderer.Time, Renderer.LoadingAnimation (Factor: 1 for LOADING_ANIMATION_ALWAYS, :617-622)
    float    color0[3], color1[3];
    float    sceneNearZ, sceneFarZ; // g_Frame.Camera.fSceneNearZ / fSceneFarZ (:605-606)
};
// the block of a desc that has passed check_shade_output_desc (api_pbr.cpp: `renderer` is set); its two planes are the caller's to bind
inline OutputK make_outputk(const mifx_pbr_shade_output_desc& d, const mifx_camera_attribs& camera, bool hasMotion, bool hasMeshNormal)
{
    const mifx_pbr_renderer_shader_parameters& r = *d.renderer;
    OutputK o{};
    o.debugView = d.debug_view; o.loadingAnimation = d.loading_animation; o.alphaMode = d.alpha_mode; o.unlit = d.unlit != 0;
    o.srgb = (d.flags & MIFX_PBR_SHADE_OUTPUT_FLAG_CONVERT_OUTPUT_TO_SRGB) != 0u;
    o.hasMotion = hasMotion; o.hasMeshNormal = hasMeshNormal;
    o.alphaMaskCutoff = d.alpha_mask_cutoff;
    o.tm = ToneMapK{r.MiddleGray, r.WhitePoint, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, r.AverageLogLum, 0};
    for (int i = 0; i < 4; ++i) o.highlight[i] = r.HighlightColor[i];
    o.time = r.Time; o.worldScale = r.LoadingAnimation.WorldScale; o.speed = r.LoadingAnimation.Speed;
    o.factor = d.loading_animation == MIFX_PBR_LOADING_ANIMATION_TRANSITIONING ? r.LoadingAnimation.Factor : 1.0f; // RenderPBR.psh:617-622
    for (int i = 0; i < 3; ++i) { o.color0[i] = r.LoadingAnimation.Color0[i]; o.color1[i] = r.LoadingAnimation.Color1[i]; }
    o.sceneNearZ = camera.fSceneNearZ; o.sceneFarZ = camera.fSceneFarZ;
    return o;
}

// GetLoadingAnimationColor (RenderPBR.psh:361-386)
MIFX_D v4 loading_animation_color(v3 worldPos, float factor, const OutputK& o)
{
    const v3 c0{o.color0[0], o.color0[1], o.color0[2]}, c1{o.color1[0], o.color1[1], o.color1[2]};
    const v3 p = worldPos * o.worldScale;
    v3 d{p.x - floorf(p.x), p.y - floorf(p.y), p.z - floorf(p.z)}; // frac
    d = min3(d, mk3(1.0f) - d) * 2.0f;
    d = v3{sinf(fdiv(d.x * MIFX_PI, 2.0f)), sinf(fdiv(d.y * MIFX_PI, 2.0f)), sinf(fdiv(d.z * MIFX_PI, 2.0f))};
    const float dist = fdiv(dot(d, d), 3.0f);
    float weight = 1.0f - fabsf(sinf((dist + o.time * o.speed) * 2.0f * MIFX_PI));
    const float alpha = saturate(factor * 2.0f + weight - 1.0f);
    float shock = fmaxf(0.25f - fabsf(alpha - 0.25f), 0.0f) * 4.0f;
    shock *= shock;
    shock *= shock;
    weight = fmaxf(weight, shock);
    return mk4(lerp3(c0, c1, weight), alpha);
}

// GetDebugColor (PBR_Shading.fxh:879-989): a layer's view with the layer off, TEXCOORD0 / 1 and THICKNESS fall through to black (the permutations without ENABLE_* /
// USE_TEXCOORD* / ENABLE_VOLUME)
MIFX_D v3 debug_color(int view, unsigned set, const ShadeTerms& t)
{
    const bool clearCoat = (set & MIFX_PBR_LAYER_CLEAR_COAT) != 0u, sheen = (set & MIFX_PBR_LAYER_SHEEN) != 0u, aniso = (set & MIFX_PBR_LAYER_ANISOTROPY) != 0u;
    const bool irid = (set & MIFX_PBR_LAYER_IRIDESCENCE) != 0u, transm = (set & MIFX_PBR_LAYER_TRANSMISSION) != 0u;
    switch (view)
    {
        case MIFX_PBR_DEBUG_VIEW_OCCLUSION: return mk3(t.occlusion);
        case MIFX_PBR_DEBUG_VIEW_EMISSIVE: return t.emissive;
        case MIFX_PBR_DEBUG_VIEW_METALLIC: return mk3(t.metallic);
        case MIFX_PBR_DEBUG_VIEW_ROUGHNESS: return mk3(t.srf.perceptualRoughness);
        case MIFX_PBR_DEBUG_VIEW_DIFFUSE_COLOR: return t.srf.diffuse;
        case MIFX_PBR_DEBUG_VIEW_SPECULAR_COLOR: return t.srf.r0;
        case MIFX_PBR_DEBUG_VIEW_REFLECTANCE90: return t.srf.r90;
        case MIFX_PBR_DEBUG_VIEW_SHADING_NORMAL: return t.N * 0.5f + mk3(0.5f);
        case MIFX_PBR_DEBUG_VIEW_NDOTV: return mk3(t.NdotV);
        case MIFX_PBR_DEBUG_VIEW_PUNCTUAL_LIGHTING: return t.punctual;
        case MIFX_PBR_DEBUG_VIEW_DIFFUSE_IBL: return t.diffuseIBL;
        case MIFX_PBR_DEBUG_VIEW_SPECULAR_IBL: return t.specularIBL;
        case MIFX_PBR_DEBUG_VIEW_CLEAR_COAT: if (clearCoat) return t.clearcoatLighting; break;
        case MIFX_PBR_DEBUG_VIEW_CLEAR_COAT_FACTOR: if (clearCoat) return mk3(t.clearcoatFactor); break;
        case MIFX_PBR_DEBUG_VIEW_CLEAR_COAT_ROUGHNESS: if (clearCoat) return mk3(t.clearcoatRoughness); break;
        case MIFX_PBR_DEBUG_VIEW_CLEAR_COAT_NORMAL: if (clearCoat) return t.clearcoatNormal * 0.5f + mk3(0.5f); break;
        case MIFX_PBR_DEBUG_VIEW_SHEEN: if (sheen) return t.sheenLighting; break;
        case MIFX_PBR_DEBUG_VIEW_SHEEN_COLOR: if (sheen) return t.sheenColor; break;
        case MIFX_PBR_DEBUG_VIEW_SHEEN_ROUGHNESS: if (sheen) return mk3(t.sheenRoughness); break;
        case MIFX_PBR_DEBUG_VIEW_ANISOTROPY_STRENGTH: if (aniso) return mk3(t.anisotropyStrength); break;
        case MIFX_PBR_DEBUG_VIEW_ANISOTROPY_DIRECTION: if (aniso) return v3{t.anisotropyDirection.x * 0.5f + 0.5f, t.anisotropyDirection.y * 0.5f + 0.5f, 0.0f}; break;
        case MIFX_PBR_DEBUG_VIEW_IRIDESCENCE: if (irid) return t.iridescenceFresnel; break;
        case MIFX_PBR_DEBUG_VIEW_IRIDESCENCE_FACTOR: if (irid) return mk3(t.iridescenceFactor); break;
        case MIFX_PBR_DEBUG_VIEW_IRIDESCENCE_THICKNESS: if (irid) return mk3(fdiv(t.iridescenceThickness, 1200.0f)); break;
        case MIFX_PBR_DEBUG_VIEW_TRANSMISSION: if (transm) return mk3(t.transmission); break;
        default: break;
    }
    return mk3(0.0f);
}

// RenderPBR.psh:515-643 for a pixel that has a fragment.  lit: what pbr_shade_layers_pixel returned (ResolveLighting, BaseColor.a); motion / meshNormal: MotionVector (:564-571)
// and MeshNormal (:426-431), zero without their planes.  TM: TONE_MAPPING_MODE, 0 = ENABLE_TONE_MAPPING off.
template <int TM>
MIFX_D v4 shade_output_tail(const ShadeTerms& t, v4 lit, unsigned set, const OutputK& o, v2 motion, v3 meshNormal, const CamK& cam)
{
    const v4 base = t.baseColor;
    v4 out = lit;
    if ((set & MIFX_PBR_LAYER_TRANSMISSION) != 0u) out.w = 1.0f - t.transmission; // :515-523
    if (o.unlit) out = base;                                                       // :525-528
    if constexpr (TM != 0) out = mk4(tone_map<TM>(xyz(out), o.tm), out.w);         // :530-542
    if (o.alphaMode == MIFX_PBR_ALPHA_MODE_BLEND) out = mk4(xyz(out) * base.w, out.w); // :545-547
    out = mk4(lerp3(xyz(out), v3{o.highlight[0], o.highlight[1], o.highlight[2]}, o.highlight[3]), out.w); // :562
    switch (o.debugView) // :574-613
    {
        case MIFX_PBR_DEBUG_VIEW_NONE:
        case MIFX_PBR_DEBUG_VIEW_WHITE_BASE_COLOR: break; // (handled before the lighting)
        case MIFX_PBR_DEBUG_VIEW_BASE_COLOR: out = base; break;
        case MIFX_PBR_DEBUG_VIEW_TRANSPARENCY: out = v4{base.w, base.w, base.w, 1.0f}; break;
        case MIFX_PBR_DEBUG_VIEW_MESH_NORMAL: out = mk4(meshNormal * 0.5f + mk3(0.5f), out.w); break;
        case MIFX_PBR_DEBUG_VIEW_MOTION_VECTORS: out = v4{fsqrt(fabsf(motion.x)) * 5.0f, fsqrt(fabsf(motion.y)) * 5.0f, 0.0f, out.w}; break;
        case MIFX_PBR_DEBUG_VIEW_SCENE_DEPTH:
        {
            const float cameraZ = depth_to_camera_z(t.depth, cam.proj);
            const float range   = fmaxf(o.sceneFarZ - o.sceneNearZ, 1e-6f);
            const float rel     = saturate(fdiv(cameraZ - o.sceneNearZ, range));
            out = mk4(mk3(rel), out.w);
            break;
        }
        default: out = mk4(debug_color(o.debugView, set, t), out.w); break;
    }
    if (o.loadingAnimation != MIFX_PBR_LOADING_ANIMATION_NONE && o.factor > 0.0f) // :615-630
    {
        const v4 c = loading_animation_color(t.pos, o.factor, o);
        out = v4{lerpf(out.x, c.x, c.w), lerpf(out.y, c.y, c.w), lerpf(out.z, c.z, c.w), lerpf(out.w, 0.0f, c.w)};
    }
    if (o.alphaMode != MIFX_PBR_ALPHA_MODE_BLEND) out.w = 1.0f; // :633-637 (Transmittance of :632 is 1: the OIT transmittance is mifx_oit_blend's)
    if (o.srgb) out = v4{powf(out.x, 1.0f / 2.2f), powf(out.y, 1.0f / 2.2f), powf(out.z, 1.0f / 2.2f), out.w}; // FastLinearToSRGB (SRGBUtilities.fxh:40-43)
    return out;
}

// One pixel of the shade with its output stage: the body of pbr_shade_output_kernel (pbr.hip) and of tests/host_kernels/shade_output_host.cpp.
template <bool APRON, bool SHADOWS, int TM>
MIFX_D void pbr_shade_output_pixel(int x, int y, const Img& baseColor, const Img& normalTex, const Img& material, const Img& depthTex, const Img& emissive, const Img& occlusion,
                                   const LutK& lut, const v4* irradiance0, int irradianceSize, const v4* const* prefMips, int prefSize, int prefLevels, const CamK& cam,
                                   const ShadeK& k, const LayersK& ly, int hasEmissive, int hasAo, const ShadowK& sh, const OutputK& o, const Img& motionTex, const Img& meshNormalTex,
                                   v4& outColor, v4& outSpec)
{
    ShadeTerms t;
    t.maskTest        = o.alphaMode == MIFX_PBR_ALPHA_MODE_MASK;
    t.alphaMaskCutoff = o.alphaMaskCutoff;
    t.whiteBaseColor  = o.debugView == MIFX_PBR_DEBUG_VIEW_WHITE_BASE_COLOR;
    v4 lit;
    pbr_shade_layers_pixel<APRON, kLayersRuntime, SHADOWS, ShadeTerms>(x, y, baseColor, normalTex, material, depthTex, emissive, occlusion, lut, irradiance0, irradianceSize, prefMips,
                                                                       prefSize, prefLevels, cam, k, ly, hasEmissive, hasAo, sh, lit, outSpec, &t);
    if (t.background)
    {
        outColor = lit;
        return;
    }
    if (o.unlit) outSpec = mk4(mk3(0.0f), 1.0f); // (no lighting pass ran: SrfLighting keeps GetDefaultSurfaceLightingInfo, whose specular IBL is zero)
    const v2 motion     = o.hasMotion ? ld<v2>(motionTex, x, y) : v2{0.0f, 0.0f};
    const v3 meshNormal = o.hasMeshNormal ? xyz(ld<v4>(meshNormalTex, x, y)) : mk3(0.0f);
    outColor = shade_output_tail<TM>(t, lit, ly.flags, o, motion, meshNormal, cam);
}

// ---- the G-buffer targets of the USD renderer's footer (Hydrogent: the text USD_Renderer::GetUsdPbrPSMainSource builds behind `main`, PBR/src/USD_Renderer.cpp:85-168):
// what PSOut.Normal / BaseColor / Material / IBL receive, which the later passes of the frame (SSR, SSAO, the composite of HnPostProcess.psh:145-185) read.
struct ShadeTargets
{
    v4 normal, baseColor, material, ibl;
};
// The footer for a pixel that has a fragment.  t: the terms of the pixel; baseSpecularIBL: GetBaseLayerSpecularIBL (PBR_Shading.fxh:801-805), what the layered body returns as
// its specular-IBL output; animationFactor: g_Frame.Renderer.LoadingAnimation.Factor as it stands -- the footer does NOT force 1 for LOADING_ANIMATION_ALWAYS, unlike the colour
// (RenderPBR.psh:617).  An unlit material ran no lighting: SrfLighting keeps its default and both IBL getters return zero.
MIFX_D ShadeTargets shade_targets_footer(const ShadeFooterTerms& t, v3 baseSpecularIBL, unsigned set, const OutputK& o, float animationFactor)
{
    v3 normal = t.N;                                          // USD_Renderer.cpp:97  Shading.BaseLayer.Normal
    v2 materialData{t.srf.perceptualRoughness, t.metallic};   // :98
    v3 ibl  = o.unlit ? mk3(0.0f) : baseSpecularIBL;          // :99
    v3 base = xyz(t.baseColor);                               // BaseColor after RenderPBR.psh:467-471; the BLEND premultiply of :547 touches OutColor only
    if ((set & MIFX_PBR_LAYER_CLEAR_COAT) != 0u)              // :101-117
    {
        const float f = t.clearcoatFactor;
        normal       = normalize(lerp3(normal, t.clearcoatNormal, f));                                              // :108
        materialData = v2{lerpf(materialData.x, t.clearcoatRoughness, f), lerpf(materialData.y, 0.0f, f)};          // :109
        base         = lerp3(base, mk3(1.0f), f);                                                                   // :110
        ibl          = lerp3(ibl, o.unlit ? mk3(0.0f) : t.clearcoatIBL, f);                                         // :115 (GetClearcoatIBL, PBR_Shading.fxh:834-838)
    }
    if (o.loadingAnimation != MIFX_PBR_LOADING_ANIMATION_NONE)                                                      // :118-120
        materialData = v2{lerpf(materialData.x, 1.0f, animationFactor), lerpf(materialData.y, 0.0f, animationFactor)};
    const float transmittance = 1.0f; // (:122-124; NUM_OIT_LAYERS 0 -- the OIT transmittance is mifx_oit_blend's)
    materialData = v2{materialData.x * transmittance, materialData.y * transmittance};
    ibl          = ibl * transmittance;
    base         = base * transmittance;
    const float a = t.baseColor.w;
    ShadeTargets r;
    r.normal    = mk4(normal, 1.0f);                                        // :148 (not blended: the normal of the top layer)
    r.baseColor = mk4(base * a, a);                                         // :155
    r.material  = v4{materialData.x * a, materialData.y * a, 0.0f, a};      // :160
    r.ibl       = mk4(ibl * a, a);                                          // :165
    return r;
}
// One pixel of the shade with its output stage and the footer: the body of pbr_shade_targets_kernel (pbr.hip) and of tests/host_kernels/shade_targets_host.cpp.  A pixel without
// a fragment (background, or discarded by PBR_ALPHA_MODE_MASK) keeps what the caller's G-buffer holds -- there is no rasteriser: "not covered" is "what the plane had" -- and
// gets a zero IBL target, as out_specular_ibl does.
template <bool APRON, bool SHADOWS, int TM>
MIFX_D void pbr_shade_targets_pixel(int x, int y, const Img& baseColor, const Img& normalTex, const Img& material, const Img& depthTex, const Img& emissive, const Img& occlusion,
                                    const LutK& lut, const v4* irradiance0, int irradianceSize, const v4* const* prefMips, int prefSize, int prefLevels, const CamK& cam,
                                    const ShadeK& k, const LayersK& ly, int hasEmissive, int hasAo, const ShadowK& sh, const OutputK& o, float animationFactor, const Img& motionTex,
                                    const Img& meshNormalTex, v4& outColor, ShadeTargets& targets)
{
    // (pbr_shade_output_pixel with the footer's terms: the same statements, so that PSOut.Color is that entry's, bit for bit)
    ShadeFooterTerms t;
    t.maskTest        = o.alphaMode == MIFX_PBR_ALPHA_MODE_MASK;
    t.alphaMaskCutoff = o.alphaMaskCutoff;
    t.whiteBaseColor  = o.debugView == MIFX_PBR_DEBUG_VIEW_WHITE_BASE_COLOR;
    v4 lit, spec;
    pbr_shade_layers_pixel<APRON, kLayersRuntime, SHADOWS, ShadeFooterTerms>(x, y, baseColor, normalTex, material, depthTex, emissive, occlusion, lut, irradiance0, irradianceSize,
                                                                             prefMips, prefSize, prefLevels, cam, k, ly, hasEmissive, hasAo, sh, lit, spec, &t);
    if (t.background)
    {
        outColor          = lit;
        targets.normal    = ld<v4>(normalTex, x, y);
        targets.baseColor = ld<v4>(baseColor, x, y);
        targets.material  = ld<v4>(material, x, y);
        targets.ibl       = mk4(0.0f);
        return;
    }
    const v2 motion     = o.hasMotion ? ld<v2>(motionTex, x, y) : v2{0.0f, 0.0f};
    const v3 meshNormal = o.hasMeshNormal ? xyz(ld<v4>(meshNormalTex, x, y)) : mk3(0.0f);
    outColor = shade_output_tail<TM>(t, lit, ly.flags, o, motion, meshNormal, cam);
    targets  = shade_targets_footer(t, xyz(spec), ly.flags, o, animationFactor);
}
} // namespace mifx
