// mifx_selection.h -- the selection outline of Hydrogent, per pixel: the body of the jump flood kernels and of the selection tail of composite_kernel (selection.hip,
// composite.hip), in a header so that the test suite can also compile it for the host (tests/host_kernels/selection_host.cpp).
//   * the closest-selected-location plane: HnProcessSelectionTask.cpp:302-369 with HnInitClosestSelectedLocation.psh (init) and HnUpdateClosestSelectedLocation.psh
//     (one jump-flood step), encoded as HnClosestSelectedLocation.fxh does;
//   * the composite's selection tail: HnPostProcess.psh:211-241 (desaturation of what is not selected, the outline).
// Every decision of the jump flood (which tap wins) depends on fp32 products and sums, so nothing here is contracted: with `#pragma clang fp contract(off)` in every
// body an fp32 restatement (tests/selection_util.py) reproduces the plane bit for bit.  The pragma is lexical: the bodies call no helper with a multiply-add.
#pragma once
#include <cmath>
#include "mifx_device.h"

namespace mifx
{
// HnClosestSelectedLocation.fxh: EncodeClosestSelectedLocation / DecodeClosestSelectedLocation
MIFX_D v2 jf_encode(v2 loc, bool valid)
{
#pragma clang fp contract(off)
    return valid ? v2{loc.x, loc.y * 0.5f + 0.5f} : v2{0.0f, 0.0f};
}
MIFX_D bool jf_decode(v2 enc, v2& loc)
{
#pragma clang fp contract(off)
    if (enc.y <= 0.25f)
    {
        loc = v2{0.0f, 0.0f};
        return false;
    }
    loc = v2{enc.x, enc.y * 2.0f - 1.0f};
    return true;
}

// HnInitClosestSelectedLocation.psh: the encoded location of the pixel (x, y) of a W x H frame whose selection depth is `selDepth`
MIFX_D v2 jf_init(int x, int y, float selDepth, float clearDepth, int W, int H)
{
#pragma clang fp contract(off)
    const bool selected = selDepth != clearDepth;
    // (f4PixelPos.xy / float2(Width, Height): IEEE division -- this value is the seed every later step compares against)
    const v2 loc{(float(x) + 0.5f) / float(W), (float(y) + 0.5f) / float(H)};
    return jf_encode(loc, selected);
}

// The texel a tap of HnUpdateClosestSelectedLocation.psh reads along one axis: Load(int(Pos + Offset * SampleRange)) with Pos = p + 0.5.  The float-to-int conversion
// truncates toward zero, so p + o * r = -1 (Pos - r = -0.5) reads texel 0 and p + o * r <= -2 lies outside the frame, as does anything >= n.  Returns -1 for outside.
MIFX_D int jf_tap(int p, int offset, int range, int n)
{
    int t = p + offset * range;
    t = t == -1 ? 0 : t;
    return (t < 0 || t >= n) ? -1 : t;
}

// One candidate of UpdateClosestLocation: `enc` is the texel the tap read (0 outside the frame = invalid).  best = ClosestDistance (1e10 at the start), strict <.
MIFX_D void jf_consider(v2 enc, int x, int y, float fW, float fH, v2& closest, bool& valid, float& best)
{
#pragma clang fp contract(off)
    v2 loc;
    if (!jf_decode(enc, loc)) return;
    const float dx = loc.x * fW - (float(x) + 0.5f);
    const float dy = loc.y * fH - (float(y) + 0.5f);
    const float d2 = dx * dx + dy * dy;
    if (d2 < best)
    {
        best    = d2;
        closest = loc;
        valid   = true;
    }
}

// One jump-flood step for the pixel (x, y) with SampleRange = `range`: the nine taps in the shader's order, `fetch(tx, ty)` returns the source texel (only called for
// texels inside the frame).
template <class Fetch> MIFX_D v2 jf_step(int x, int y, int range, int W, int H, Fetch fetch)
{
    v2    closest{0.0f, 0.0f};
    bool  valid = false;
    float best  = 1e10f;
    const float fW = float(W), fH = float(H);
#pragma unroll
    for (int oy = -1; oy <= 1; ++oy)
    {
        const int ty = jf_tap(y, oy, range, H);
#pragma unroll
        for (int ox = -1; ox <= 1; ++ox)
        {
            const int tx = jf_tap(x, ox, range, W);
            if (tx < 0 || ty < 0) continue; // (reads 0: decodes as invalid)
            jf_consider(fetch(tx, ty), x, y, fW, fH, closest, valid, best);
        }
    }
    return jf_encode(closest, valid);
}

// HnProcessSelectionTask::Sync (HnProcessSelectionTask.cpp:71): m_NumJFIterations; step i uses SampleRange = 1 << (n - 1 - i)
inline int jf_iterations(float maxDistance)
{
    const float d = maxDistance > 1.0f ? maxDistance : 1.0f;
    return int(std::ceil(std::log2(d))) + 1;
}

// What the composite's selection tail reads beside the composite's own inputs (PostProcessAttribs, HnPostProcessStructures.fxh): the outline colours as the shader
// receives them (the chain converts them with ReverseExpToneMap first, HnPostProcessTask.cpp:843-850).
struct SelectionK
{
    Img   depth, selectionDepth, closest; // F32, F32, F32X2 (the closest-selected-location plane)
    float outline[3], occluded[3];
    float desaturation, clearDepth, outlineWidth;
};

// HnPostProcess.psh:211-241 on the colour of the pixel (x, y) after the composite (and its optional tone map); W x H = the frame.  `depth` / `selDepth` / `enc`: the
// pixel's texels of the three planes (loaded by the caller beside its own loads); the two texels at the closest location are loaded here when the outline is drawn.
template <class Load> MIFX_D v3 selection_tail(v3 rgb, int x, int y, int W, int H, float depth, float selDepth, v2 enc, const SelectionK& k, Load loadDepths)
{
#pragma clang fp contract(off)
    const bool selected = depth != k.clearDepth && selDepth == depth;
    // Desaturate all unselected pixels
    const float desat = selected ? 0.0f : k.desaturation;
    const float lum   = rgb.x * 0.2126f + rgb.y * 0.7152f + rgb.z * 0.0722f;
    rgb = v3{rgb.x + desat * (lum - rgb.x), rgb.y + desat * (lum - rgb.y), rgb.z + desat * (lum - rgb.z)};
    v2 loc;
    if (jf_decode(enc, loc))
    {
        loc = v2{loc.x * float(W), loc.y * float(H)};
        const float dx = loc.x - (float(x) + 0.5f), dy = loc.y - (float(y) + 0.5f);
        const float dist = sqrtf(dx * dx + dy * dy);
        float outline = saturate(1.0f - dist / k.outlineWidth);
        outline = outline * (selDepth != k.clearDepth ? 0.0f : 1.0f);
        if (outline > 0.0f)
        {
            // Load(int3(ClosestSelectedLocation.xy, 0)): truncation; outside the frame a load reads 0
            const int lx = int(loc.x), ly = int(loc.y);
            float d = 0.0f, sd = 0.0f;
            if (lx >= 0 && lx < W && ly >= 0 && ly < H) loadDepths(lx, ly, d, sd);
            const bool  visible = d == sd;
            const v3    c{visible ? k.outline[0] : k.occluded[0], visible ? k.outline[1] : k.occluded[1], visible ? k.outline[2] : k.occluded[2]};
            rgb = v3{rgb.x + outline * (c.x - rgb.x), rgb.y + outline * (c.y - rgb.y), rgb.z + outline * (c.z - rgb.z)};
        }
    }
    return rgb;
}
} // namespace mifx
