// mifx_oit_shade.h -- one transparent draw, shaded and blended, per pixel: the body of oit_shade_blend_kernel (pbr.hip; include/mifx.h: mifx_oit_shade_blend).  The
// reference's transparent draw is ONE pixel shader -- RenderPBR.psh `main` shades, multiplies by BaseColor.a (:547) and the transmittance in front of the fragment (:632),
// and the blend state adds the four outputs to the targets -- and so is this: the layered shade's body (mifx_pbr_layers.h: pbr_shade_layers_pixel, the set a run-time
// mask) followed by the colour pass of mifx_oit.h (oit_transmittance_at, oit_blend_fragment), both as they are, the shade's colour and specular IBL staying in registers.
// No arithmetic of its own: the result is what mifx_pbr_shade_execute_layers (background 0) into two planes and mifx_oit_blend on those planes give, bit for bit.
// In a header so that the test suite can also compile it for the host (tests/host_kernels/shade_blend_host.cpp).
#pragma once
#include "mifx_oit.h"
#include "mifx_pbr_layers.h"

namespace mifx
{
// the draw's own G-buffer (mifx_transparent_slice): depth holds the shade's background value where the draw has no fragment; emissive, occlusion and alpha may be absent
struct OitShadeSliceK
{
    Img baseColor, normal, material, depth, emissive, occlusion, alpha;
    int hasEmissive, hasAo, hasAlpha;
};

// APRON, SHADOWS: those of pbr_shade_layers_pixel.  A pixel without a fragment reads the slice's depth and the opaque depth and writes nothing; the targets are loaded
// only after the shade has finished, so its register budget is the shade's.
template <bool APRON, bool SHADOWS>
MIFX_D void oit_px_shade_blend(const OitK& k, const OitShadeSliceK& s, const OitTargetsK& t, const LutK& lut, const v4* irradiance0, int irradianceSize, const v4* const* prefMips,
                               int prefSize, int prefLevels, const CamK& cam, const ShadeK& sk, const LayersK& ly, const ShadowK& sh, int x, int y)
{
    const float depth = ld<float>(s.depth, x, y);
    if (!oit_fragment_at(k, depth, oit_opaque_at(k, x, y))) return;
    v4 color, spec;
    pbr_shade_layers_pixel<APRON, kLayersRuntime, SHADOWS>(x, y, s.baseColor, s.normal, s.material, s.depth, s.emissive, s.occlusion, lut, irradiance0, irradianceSize, prefMips, prefSize,
                                                           prefLevels, cam, sk, ly, s.hasEmissive, s.hasAo, sh, color, spec);
    OitFragment f;
    f.base       = ld<v4>(s.baseColor, x, y);
    f.material   = ld<v4>(s.material, x, y);
    f.radiance   = color;
    f.ibl        = spec;
    f.colorAlpha = s.hasAlpha ? ld<float>(s.alpha, x, y) : f.base.w;
    float T = 1.0f;
    if (f.base.w > kOitOpacityThreshold) // RenderPBR.psh:549-557, as oit_blend_slice
        T = oit_transmittance_at((const MIFX_GLOBAL uint32_t*)oit_layers_at(k, x, y), k.K, GlobalAccess<v2>::load(oit_tail_at(k, x, y)), oit_fragment_depth(depth, k.cam));
    v4 c = ld<v4>(t.color, x, y), b = ld<v4>(t.base, x, y), m = ld<v4>(t.material, x, y), i = ld<v4>(t.ibl, x, y);
    oit_blend_fragment(f, T, c, b, m, i);
    st<v4>(t.color, x, y, c); st<v4>(t.base, x, y, b); st<v4>(t.material, x, y, m); st<v4>(t.ibl, x, y, i);
}
} // namespace mifx
