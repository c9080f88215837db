// mifx_composite.h -- (M1) one pixel of the SSR / SSAO composite of the chain, Hydrogent/shaders/HnPostProcess.psh:145-185: the body of composite_kernel (composite.hip),
// in a header so that the test suite can also compile it for the host (tests/host_kernels/chain_host.cpp).
#pragma once
#include "mifx_pbr.h"
#include "mifx_effects.h"
#include "mifx_tonemap.h"
#include "mifx_ssr_cleanup.h"
#include "mifx_selection.h"

namespace mifx
{
// FUSE_R7: the reflection is SSR's bilateral cleanup (pass R7) evaluated here for this pixel from the effect's accumulated radiance / variance instead of a load of
// the plane R7 would have written -- this kernel is that plane's only consumer in the chain (mifx_ssr_cleanup.h; `ssr` is not read).  outW / outH: the size of the target.
// SELECTION: after the optional tone map, the selection tail of HnPostProcess.psh:211-241 (mifx_selection.h) with the planes and colours of `sel` (not read otherwise).
//
// FUSE_R7 fetches the inputs of the reflection term only where a reflection exists.  Outside the reflection mask R7 yields exactly (0, 0, 0, 0); inside it, a pixel whose
// every ray missed has refl.w == 0 exactly.  In both cases the term is (0 * k - sibl) * 0 * ssrScale, a zero, and the colour is passed through instead: outside the mask
// without one load of the block (64 B/px, the LUT taps, the arithmetic), inside it after R7 without specular IBL / base colour / material (48 B/px) and the LUT taps.
// That is the same float as adding the zero for every input except these corners:
//   (1) a colour component of -0.0 stays -0.0 where the sum gave +0.0 (the chain's shade starts its sum from +0 and cannot produce one);
//   (2) a non-finite value in specIBL / base colour / material / the LUT at such a pixel -- outside the mask also in the normal -- no longer turns it into NaN (inf * 0);
//   (3) inside the mask, a non-finite reflection colour with refl.w == 0 (s non-finite) no longer does either.
// A pixel with a reflection executes the same arithmetic on the same values in the same order.  Without FUSE_R7 (the stand-alone composite, which loads R7's plane) nothing
// is tested: it is the yardstick the fused instance is held to (tests/test_gpu_composite_skip.py, tests/test_host_kernel_composite_skip.py).
template <int TM_MODE, bool FUSE_R7, bool SELECTION = false>
MIFX_D void composite_pixel(v4& result, int x, int y, const Img& color, const Img& specIBL, const Img& ssr, const Img& ssao, const Img& normalTex, const Img& baseColor, const Img& material,
                          const LutK& lut, int outW, int outH, const CamK& cam, float ssrScaleAttr, float ssaoScaleAttr, const ToneMapK& tm, const SsrCleanupIn& r7,
                          const SelectionK& sel = SelectionK{})
{
    // (loads grouped by what they depend on: the colour -- whose alpha decides whether anything else is read -- with the reflection mask, which decides the same for the
    //  reflection; then every other plane of the pixel at once: unfused, all of them; fused, the normal beside the inputs of the cleanup, and behind the cleanup, where its
    //  weight is not zero, specular IBL / base colour / material at once; then the LUT taps, which need the roughness and the normal)
    v4 c = ld_once<v4>(color, x, y);
    const float maskValue = FUSE_R7 ? ld<mask_t>(r7.mask, x, y) : 1.0f;
    const float opacity  = c.w;
    const float ssrScale = ssrScaleAttr * opacity;
    const float ssaoScale = ssaoScaleAttr * opacity;
    const float ao = ssaoScale > 0.0f ? ld_once<ao_t>(ssao, x, y) : 1.0f;
    v3 rgb = xyz(c);
    if (FUSE_R7)
    {
        if (ssrScale > 0.0f && !(maskValue == 0.0f))
        {
            const v3 N = xyz(ld<v4>(normalTex, x, y));
            // (quantize_v4: what the store into the pass's 4-channel target and the load back from it do to the value -- nothing in the fp32 build, a binary16 rounding in
            //  the native-storage build, where the fused and the separate pass must still agree)
            const v4 refl = quantize_v4(ssr_bilateral_cleanup(x, y, N, maskValue, normalTex, r7, cam.proj, int(cam.vw), int(cam.vh)));
            if (!(refl.w == 0.0f))
            {
                const v4 sibl = ld_once<v4>(specIBL, x, y);
                const v4 bc   = ld_once<v4>(baseColor, x, y);
                const v4 mat  = ld_once<v4>(material, x, y);
#if defined(__HIP_DEVICE_COMPILE__)
                __builtin_amdgcn_sched_barrier(0); // (the three loads leave together: the scheduler otherwise sinks each to its first use, one round trip after the other)
#endif
                // (the term of the unfused branch below, on the same values in the same order)
                const SurfaceReflectance srf = surface_reflectance_mr(xyz(bc), saturate(mat.y), saturate(mat.x));
                // f2NormalizedXY of the pixel centre, depth 0.5 => a point on the view ray
                const v2 ndc{fdiv(2.0f * (float(x) + 0.5f), float(outW)) - 1.0f, 1.0f - fdiv(2.0f * (float(y) + 0.5f), float(outH))};
                const v4 wp   = mul(v4{ndc.x, ndc.y, 0.5f, 1.0f}, cam.viewProjInv);
                const v3 view = normalize(v3{cam.pos[0], cam.pos[1], cam.pos[2]} - xyz(wp) / wp.w);
                const IBLInfo ibl = ibl_sampling_info(srf, lut, N, view);
                const v3 s = specular_ibl_ggx(ibl, xyz(refl));
                rgb = rgb + (s - xyz(sibl)) * refl.w * ssrScale;
            }
        }
    }
    else if (ssrScale > 0.0f)
    {
        const v4 sibl = ld_once<v4>(specIBL, x, y);
        const v3 N    = xyz(ld<v4>(normalTex, x, y));
        const v4 bc   = ld_once<v4>(baseColor, x, y);
        const v4 mat  = ld_once<v4>(material, x, y);
        const v4 refl = ld<v4>(ssr, x, y);
        const SurfaceReflectance srf = surface_reflectance_mr(xyz(bc), saturate(mat.y), saturate(mat.x));
        // f2NormalizedXY of the pixel centre, depth 0.5 => a point on the view ray
        const v2 ndc{fdiv(2.0f * (float(x) + 0.5f), float(outW)) - 1.0f, 1.0f - fdiv(2.0f * (float(y) + 0.5f), float(outH))};
        const v4 wp   = mul(v4{ndc.x, ndc.y, 0.5f, 1.0f}, cam.viewProjInv);
        const v3 view = normalize(v3{cam.pos[0], cam.pos[1], cam.pos[2]} - xyz(wp) / wp.w);
        const IBLInfo ibl = ibl_sampling_info(srf, lut, N, view);
        const v3 s = specular_ibl_ggx(ibl, xyz(refl));
        rgb = rgb + (s - xyz(sibl)) * refl.w * ssrScale;
    }
    if (ssaoScale > 0.0f) rgb = rgb * lerpf(1.0f, ao, ssaoScale);
    if (TM_MODE != MIFX_TONE_MAPPING_MODE_NONE) rgb = tone_map<TM_MODE>(rgb, tm);
    if (SELECTION)
    {
        const float depth = ld<float>(sel.depth, x, y), selDepth = ld<float>(sel.selectionDepth, x, y);
        const v2    enc   = ld<v2>(sel.closest, x, y);
        rgb = selection_tail(rgb, x, y, outW, outH, depth, selDepth, enc, sel, [&](int lx, int ly, float& d, float& sd) __attribute__((always_inline)) {
            d  = ld<float>(sel.depth, lx, ly);
            sd = ld<float>(sel.selectionDepth, lx, ly);
        });
    }
    result = mk4(rgb, c.w);
}
} // namespace mifx
