#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/shadows_golden.npz: inputs and outputs of the REFERENCE's shadow conversion (Shaders/Shadows/private/ShadowConversions.fx
driven the way Components/src/ShadowMapManager.cpp:533-600 drives it) and of its cascaded look-up (Shaders/Common/public/Shadows.fxh with PCF.fxh), compiled for the CPU
from the reference tree where it lies.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, default /root/reference); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_shadows.py

The shader text is read at generation time, rewritten by oracle/ref_prep.py into a temporary directory and compiled there through oracle/ref/hlsl_shim.h with the small
wrappers below, which #include the reference files by name and hold none of their text; one translation unit per permutation of the SHADOW_MODE / PCF_FILTER_SIZE /
FILTER_ACROSS_CASCADES / BEST_CASCADE_SEARCH macros.  Nothing compiled is kept.  The fixture holds data only.

What the wrappers add (the conventions of include/mifx.h, mifx_shadow_map_filter, in the same fp32 order as diligentfx_amd/csrc/mifx_shadows.h):
  * Texture2DArray<float4>::SampleGrad: a bilinear, clamped fetch of the only mip in the slice rounded to nearest (an explicit specialisation of the shim's array);
  * the bare `Texture2DArray` of ShadowConversions.fx with Load(int4): 0 outside the slice;
  * the shader branch of ShadowMapAttribs::f4CascadeCamSpaceZEnd in the temporary copy of BasicStructures.fxh (same bytes: sizeof is 1200 either way);
  * position from depth, quad derivatives (a lane outside the frame is evaluated as its in-frame partner) and the background test.

Every case is built twice: strict fp32 (the oracle's flags) and with -ffp-contract=fast -march=native.  PCF cases store the share of pixels whose light amount differs by
more than 1e-3 between the two builds, the other look-ups the largest light-amount difference, the conversions the largest difference in the measure of
util.assert_close.  Where the two builds stay within 0.5e-3 and no pixel flips the tests use the project's contract; otherwise the stored budget is twice the measured
value, and the generator asserts a flipped share of at most 1e-3 and a tolerance below 0.02."""
import ctypes
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_grid as MG  # noqa: E402  (the prelude with run_quads, the two flag sets and the compile step)
import ref_prep  # noqa: E402
import shadows_util as S  # noqa: E402
import util  # noqa: E402

REFERENCE_ROOT = MG.REFERENCE_ROOT
F = np.float32

ARRAY_PRELUDE = r"""
namespace hlsl
{
// SampleGrad on the filterable array: one mip (ShadowMapManager.cpp:63), so the gradients select nothing: hl_sample_level's bilinear clamp fetch
template <> struct Texture2DArray_<float4>
{
    Image slice[32];
    int   slices = 0;
    float4 SampleGrad(const SamplerState&, const float3& uvs, const float2&, const float2&) const
    {
        int s = int(std::floor(uvs.z + 0.5f));
        s = s < 0 ? 0 : (s > slices - 1 ? slices - 1 : s);
        return hl_sample_level(slice[s], Sam_LinearClamp, uvs.x, uvs.y);
    }
};
// the bare Texture2DArray of ShadowConversions.fx
struct ConvArray
{
    Image slice[32];
    int   slices = 0;
    float4 Load(const int4& p) const { return (p.z < 0 || p.z >= slices) ? float4(0.f, 0.f, 0.f, 0.f) : hl_fetch(slice[p.z], p.x, p.y); }
};
}
"""


def lookup_unit(mode, across, best, pcf):
    tag = f"{mode}_{across}_{best}_{pcf}"
    pcf_macro = f"#define PCF_FILTER_SIZE {pcf}\n" if pcf > 0 else ""
    call = ("sl::FilterShadowMap(SA, sm, Sam_ComparisonLinearClamp, pos, dx, dy, camZ)" if mode == S.MODE_PCF
            else "sl::SampleFilterableShadowMap(SA, fm, Sam_LinearClamp, pos, dx, dy, camZ)")
    return MG.PRELUDE + ARRAY_PRELUDE + pcf_macro + f"""
#define SHADOW_MODE {mode}
#define FILTER_ACROSS_CASCADES {across}
#define BEST_CASCADE_SEARCH {best}
#define sl sl_{tag} // (one namespace per permutation: the units are linked into one library)
namespace hlsl {{ namespace sl {{
#include "ShaderDefinitions.fxh"
#include "BasicStructures.fxh"
#include "ShaderUtilities.fxh"
#include "FullScreenTriangleVSOutput.fxh"
#include "Shadows.fxh"
}}}}
extern "C" int ref_shadow_lookup_{tag}(const void* cam, const void* attribs, const float* frame, int W, int H, const float* map, int mw, int mh, int slices, int ch, float* light,
                                       float* cascade)
{{
    using namespace hlsl;
    static sl::CameraAttribs Cam;
    static sl::ShadowMapAttribs SA;
    std::memcpy(&Cam, cam, sizeof(Cam));
    std::memcpy(&SA, attribs, sizeof(SA));
    Texture2DArray_<float> sm;
    Texture2DArray_<float4> fm;
    sm.slices = fm.slices = slices;
    for (int s = 0; s < slices; ++s) sm.slice[s] = fm.slice[s] = Image{{map + size_t(s) * mw * mh * ch, mw, mh, ch}};
    run_quads<sl::FullScreenTriangleVSOutput>(W, H, 0, 0, W, H, [&](const sl::FullScreenTriangleVSOutput&, int lx, int ly, bool store) {{
        const int x = lx < W ? lx : W - 1, y = ly < H ? ly : H - 1; // a lane outside the frame is evaluated as its in-frame partner: the derivative is 0
        const float2 nxy = float2(2.0f * ((float(x) + 0.5f) / float(W)) - 1.0f, 1.0f - 2.0f * ((float(y) + 0.5f) / float(H)));
        const float depth = frame[size_t(y) * W + x];
        const float4 c = mul(float4(nxy, DepthToNormalizedDeviceZ(depth), 1.0f), Cam.mViewProjInv);
        const float3 world = c.xyz / c.w;
        const float3 pos = mul(float4(world, 1.0f), SA.mWorldToLightView).xyz;
        const float3 dx = float3(ddx(pos.x), ddx(pos.y), ddx(pos.z)), dy = float3(ddy(pos.x), ddy(pos.y), ddy(pos.z));
        if (!store) return;
        const float camZ = sl::DepthToCameraZ(depth, Cam.mProj);
        sl::FilteredShadow r;
        r.fLightAmount = 1.0f; r.iCascadeIdx = SA.iNumCascades; r.fNextCascadeBlendAmount = 0.0f;
        if (depth != Cam.fFarPlaneDepth) r = {call};
        const size_t i = size_t(ly) * W + lx;
        light[i] = r.fLightAmount; cascade[2 * i] = float(r.iCascadeIdx); cascade[2 * i + 1] = r.fNextCascadeBlendAmount;
    }});
    return int(sizeof(SA));
}}
"""


CONVERT_UNIT = MG.PRELUDE + ARRAY_PRELUDE + r"""
#define Texture2DArray ConvArray
namespace hlsl { namespace cv {
#include "ShaderDefinitions.fxh"
#include "ShadowConversions.fx"
}}
#undef Texture2DArray
// ShadowMapManager::ConvertToFilterable's loop (ShadowMapManager.cpp:547-598) with the radii given; out: slices x h x w x ch
extern "C" int ref_shadow_convert(const float* depth, int w, int h, int slices, const float* radii, float ePos, float eNeg, int is32, int evsm, int skipBlur, int ch, float* out)
{
    using namespace hlsl;
    std::vector<float> mid(size_t(w) * h * 4);
    for (int s = 0; s < slices; ++s)
    {
        cv::g_Attribs.iCascade              = s;
        cv::g_Attribs.fHorzFilterRadius     = radii[2 * s];
        cv::g_Attribs.fVertFilterRadius     = radii[2 * s + 1];
        cv::g_Attribs.fEVSMPositiveExponent = ePos;
        cv::g_Attribs.fEVSMNegativeExponent = eNeg;
        cv::g_Attribs.Is32BitEVSM           = is32 != 0;
        cv::g_tex2DShadowMap.slices = slices;
        for (int k = 0; k < slices; ++k) cv::g_tex2DShadowMap.slice[k] = Image{depth + size_t(k) * w * h, w, h, 1};
        float* dst = out + size_t(s) * w * h * ch;
        ref_fullscreen<cv::FullScreenTriangleVSOutput>(w, h, 0u, [&](cv::FullScreenTriangleVSOutput& vs, int x, int y) {
            const float4 m = evsm ? cv::EVSMHorzPS(vs) : cv::VSMHorzPS(vs);
            for (int k = 0; k < 4; ++k) mid[(size_t(y) * w + x) * 4 + k] = k < ch ? m.d[k] : 0.0f; // (the target keeps ch channels)
            if (skipBlur) for (int k = 0; k < ch; ++k) dst[(size_t(y) * w + x) * ch + k] = m.d[k];
        });
        if (skipBlur) continue;
        cv::g_tex2DShadowMap.slices   = 1;
        cv::g_tex2DShadowMap.slice[0] = Image{mid.data(), w, h, 4};
        ref_fullscreen<cv::FullScreenTriangleVSOutput>(w, h, 0u, [&](cv::FullScreenTriangleVSOutput& vs, int x, int y) {
            const float4 m = cv::VertBlurPS(vs);
            for (int k = 0; k < ch; ++k) dst[(size_t(y) * w + x) * ch + k] = m.d[k];
        });
    }
    return int(sizeof(cv::ConversionAttribs));
}
"""


def radii_of(A, w, h):
    """fHorzFilterRadius / fVertFilterRadius of every cascade as ShadowMapManager.cpp:545-579 computes them, in float32"""
    out = np.zeros((A.iNumCascades, 2), F)
    for i in range(A.iNumCascades):
        if A.iFixedFilterSize > 0:
            out[i] = F(int((A.iFixedFilterSize - 1) / 2))
        else:
            fw = F(F(F(A.fFilterWorldSize) * F(A.Cascades[i].f4LightSpaceScale[0])) * F(0.5))
            fh = F(F(F(A.fFilterWorldSize) * F(A.Cascades[i].f4LightSpaceScale[1])) * F(0.5))
            out[i] = [F(F(fw / F(2)) * F(w)), F(F(fh / F(2)) * F(h))]
    return out


def conversion_cases():
    cs = []
    for mode in (S.MODE_VSM, S.MODE_EVSM2, S.MODE_EVSM4):
        for fs in (2, 3, 5, 7):
            cs.append(dict(name=f"conv_13x9_m{mode}_f{fs}", w=13, h=9, n=1, mode=mode, over=dict(iFixedFilterSize=fs)))
    cs.append(dict(name="conv_13x9_m4_f3_16bit_clamp", w=13, h=9, n=1, mode=S.MODE_EVSM4, over=dict(iFixedFilterSize=3, bIs32BitEVSM=0)))
    cs.append(dict(name="conv_13x9_m3_f5_16bit_clamp", w=13, h=9, n=1, mode=S.MODE_EVSM2, over=dict(iFixedFilterSize=5, bIs32BitEVSM=0)))
    cs.append(dict(name="conv_13x9_m4_f5_above_clamp", w=13, h=9, n=1, mode=S.MODE_EVSM4, over=dict(iFixedFilterSize=5, fEVSMPositiveExponent=50.0, fEVSMNegativeExponent=45.0)))
    cs.append(dict(name="conv_50x38_m2_f5", w=50, h=38, n=3, mode=S.MODE_VSM, over=dict(iFixedFilterSize=5)))
    cs.append(dict(name="conv_50x38_m4_f7", w=50, h=38, n=3, mode=S.MODE_EVSM4, over=dict(iFixedFilterSize=7)))
    # world-sized filters: radius = fFilterWorldSize * scale * 0.25 * size, per cascade and axis: (2.6, 0.3), (1.2, 1.7), (3.4, 0.0)
    cs.append(dict(name="conv_50x38_m3_world", w=50, h=38, n=3, mode=S.MODE_EVSM2, over=dict(iFixedFilterSize=0, fFilterWorldSize=1.0), radii=((2.6, 0.3), (1.2, 1.7), (3.4, 0.0))))
    # ... and one beyond what the fused kernel's tile holds (range 4 across in cascade 1, 5 down in cascade 2)
    cs.append(dict(name="conv_50x38_m2_world_large", w=50, h=38, n=3, mode=S.MODE_VSM, over=dict(iFixedFilterSize=0, fFilterWorldSize=1.0), radii=((1.0, 2.0), (4.2, 0.6), (0.4, 5.3))))
    cs.append(dict(name="conv_260x70_m2_f3", w=260, h=70, n=2, mode=S.MODE_VSM, over=dict(iFixedFilterSize=3)))
    cs.append(dict(name="conv_260x70_m4_f7", w=260, h=70, n=2, mode=S.MODE_EVSM4, over=dict(iFixedFilterSize=7)))
    return cs


MAP_W, MAP_H = 64, 48


def lookup_cases():
    P, V, E2, E4 = S.MODE_PCF, S.MODE_VSM, S.MODE_EVSM2, S.MODE_EVSM4
    L = lambda name, mode, n, across, best, W=67, H=45, **over: dict(name=name, mode=mode, n=n, across=across, best=best, W=W, H=H, over=over)  # noqa: E731
    return [
        L("look_pcf3_n3", P, 3, 0, 0, iFixedFilterSize=3),
        L("look_pcf2_n3_across", P, 3, 1, 0, iFixedFilterSize=2, fCascadeTransitionRegion=0.3),
        L("look_pcf5_n5_across_best", P, 5, 1, 1, iFixedFilterSize=5),
        L("look_pcf7_n8_best", P, 8, 0, 1, iFixedFilterSize=7),
        L("look_pcf_varying_n3_across", P, 3, 1, 0, iFixedFilterSize=0, fFilterWorldSize=0.6, fCascadeTransitionRegion=0.3),
        L("look_pcf_varying_n1_best", P, 1, 0, 1, iFixedFilterSize=0, fFilterWorldSize=0.25),
        L("look_pcf3_n3_bias_clamp", P, 3, 0, 0, iFixedFilterSize=3, fReceiverPlaneDepthBiasClamp=0.01),
        L("look_vsm_n3", V, 3, 0, 0),
        L("look_vsm_n3_across_best_lbr", V, 3, 1, 1, fVSMLightBleedingReduction=0.3),
        L("look_evsm2_n3_across", E2, 3, 1, 0, fCascadeTransitionRegion=0.3),
        L("look_evsm2_n3_best_lbr", E2, 3, 0, 1, fVSMLightBleedingReduction=0.2),
        L("look_evsm4_n3_across_best", E4, 3, 1, 1),
        L("look_evsm4_n3_lbr", E4, 3, 0, 0, fVSMLightBleedingReduction=0.1),
        L("look_pcf3_n3_2x2", P, 3, 1, 0, W=2, H=2, iFixedFilterSize=3),
        L("look_pcf7_n3_1x1", P, 3, 0, 1, W=1, H=1, iFixedFilterSize=7),
        L("look_evsm4_n3_2x2", E4, 3, 1, 1, W=2, H=2),
        L("look_vsm_n3_1x1", V, 3, 0, 0, W=1, H=1),
    ]


# a flipped PCF pixel moves the light amount by at most one comparison sample's weight: the largest weight product over the normalisation (PCF.fxh:55-148)
PCF_CAP = {2: 1.0, 3: 9.0 / 16.0, 5: 49.0 / 144.0, 7: 784.0 / 2704.0, 0: 1.0}


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def run_convert(lib, A, depth, mode, radii):
    n, h, w = depth.shape
    ch = 4 if mode == S.MODE_EVSM4 else 2
    out = np.zeros((n, h, w, ch), F)
    r = np.ascontiguousarray(radii, F)
    size = lib.ref_shadow_convert(fp(depth), w, h, n, fp(r), ctypes.c_float(A.fEVSMPositiveExponent), ctypes.c_float(A.fEVSMNegativeExponent), int(A.bIs32BitEVSM),
                                  int(mode != S.MODE_VSM), int(A.iFixedFilterSize == 2), ch, fp(out))
    assert size == 24, size
    return out


def run_lookup(lib, c, cam, A, frame, arr):
    H, W = frame.shape
    light, casc = np.zeros((H, W), F), np.zeros((H, W, 2), F)
    pcf = A.iFixedFilterSize if (c["mode"] == S.MODE_PCF and A.iFixedFilterSize > 0) else 0
    fn = getattr(lib, f"ref_shadow_lookup_{c['mode']}_{c['across']}_{c['best']}_{pcf}")
    ch = 1 if arr.ndim == 3 else arr.shape[3]
    size = fn(cam.tobytes(), bytes(A), fp(frame), W, H, fp(arr), arr.shape[2], arr.shape[1], arr.shape[0], ch, fp(light), fp(casc))
    assert size == 1200, size
    return light, casc


def main():
    assert os.path.isdir(os.path.join(REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    conv, look = conversion_cases(), lookup_cases()
    units = {"convert": CONVERT_UNIT}
    for c in look:
        pcf = c["over"].get("iFixedFilterSize", 3) if c["mode"] == S.MODE_PCF else 0
        pcf = pcf if pcf > 0 else 0
        units[f"lookup_{c['mode']}_{c['across']}_{c['best']}_{pcf}"] = lookup_unit(c["mode"], c["across"], c["best"], pcf)
    fx = {"conv_names": np.array([c["name"] for c in conv]), "look_names": np.array([c["name"] for c in look])}
    with tempfile.TemporaryDirectory(prefix="mifx_shadows_golden_") as tmp:
        assert ref_prep.main(REFERENCE_ROOT, tmp) == 0
        with open(os.path.join(REFERENCE_ROOT, "Shaders/Shadows/private/ShadowConversions.fx"), encoding="utf-8", errors="replace") as f:
            open(os.path.join(tmp, "ShadowConversions.fx"), "w").write(ref_prep.transform(f.read()))
        # the shader branch of ShadowMapAttribs::f4CascadeCamSpaceZEnd (BasicStructures.fxh:38-42) in the temporary copy
        p = os.path.join(tmp, "BasicStructures.fxh")
        text, k = re.subn(r"#ifdef\s+__cplusplus(\s+float\s+fCascadeCamSpaceZEnd)", r"#if 0\1", open(p).read())
        assert k == 1
        open(p, "w").write(text)
        strict, fast = MG.build(units, MG.STRICT, tmp, "strict"), MG.build(units, MG.CONTRACTED, tmp, "fast")

        # ---- conversions
        for i, c in enumerate(conv):
            A = S.make_attribs(c["n"], c["w"], c["h"], **c["over"])
            for k, r in enumerate(c.get("radii", ())):  # scales that give the radii wanted: radius = fFilterWorldSize * scale * 0.25 * size
                A.Cascades[k].f4LightSpaceScale[0], A.Cascades[k].f4LightSpaceScale[1] = 4.0 * r[0] / c["w"], 4.0 * r[1] / c["h"]
            depth = S.periodic_slices(c["n"], c["w"], c["h"])
            radii = radii_of(A, c["w"], c["h"])
            a, b = run_convert(strict, A, depth, c["mode"], radii), run_convert(fast, A, depth, c["mode"], radii)
            assert np.isfinite(a).all(), c["name"]
            diff = float(util.rel_err(b, a).max())
            print(f"{c['name']:32s} radii {radii.reshape(-1)}  strict vs contracted: max rel {diff:.3e}")
            assert diff <= 0.5e-3, f"{c['name']}: the reference's own two builds differ by {diff:.3e}"
            q = f"v{i}_"
            fx[q + "attribs"], fx[q + "depth"], fx[q + "mode"], fx[q + "out"], fx[q + "radii"] = np.frombuffer(bytes(A), np.uint8), depth, np.array(c["mode"], np.uint32), a, radii
            fx[q + "strict_vs_contracted"] = np.array(diff)

        # ---- look-ups: one 8-slice depth array; the filterable arrays are the reference's conversion (3x3) of its first three slices (EVSM2 = the first two channels
        # of EVSM4: one shader)
        slices = S.shadow_slices(8, MAP_W, MAP_H)
        Aconv = S.make_attribs(3, MAP_W, MAP_H, iFixedFilterSize=3)
        r3 = radii_of(Aconv, MAP_W, MAP_H)
        vsm, evsm4 = run_convert(strict, Aconv, slices[:3].copy(), S.MODE_VSM, r3), run_convert(strict, Aconv, slices[:3].copy(), S.MODE_EVSM4, r3)
        fx["map_depth"], fx["map_vsm"], fx["map_evsm4"], fx["map_conv_attribs"] = slices, vsm, evsm4, np.frombuffer(bytes(Aconv), np.uint8)
        frames = {}
        for i, c in enumerate(look):
            cam = S.frame_camera(c["W"], c["H"])
            frame = S.frame_depth(cam, c["W"], c["H"])
            frames.setdefault((c["W"], c["H"]), (cam, frame))
            A = S.make_attribs(c["n"], MAP_W, MAP_H, **c["over"])
            arr = {S.MODE_PCF: slices[:c["n"]], S.MODE_VSM: vsm, S.MODE_EVSM2: np.ascontiguousarray(evsm4[..., :2]), S.MODE_EVSM4: evsm4}[c["mode"]]
            arr = np.ascontiguousarray(arr)
            (la, ca), (lb, cb) = run_lookup(strict, c, cam, A, frame, arr), run_lookup(fast, c, cam, A, frame, arr)
            assert np.isfinite(la).all() and np.isfinite(ca).all(), c["name"]
            d = np.abs(la.astype(np.float64) - lb)
            flipped, worst = float((d > 1e-3).mean()), float(d.max())
            idx = ca[..., 0]
            print(f"{c['name']:32s} {c['W']}x{c['H']} cascades {sorted(set(int(v) for v in idx.reshape(-1)))} lit {float((la > 0.99).mean()):.2f} dark {float((la < 0.01).mean()):.2f} "
                  f"blend>0 {float((ca[..., 1] > 0).mean()):.2f}  strict vs contracted: max {worst:.3e} flipped {flipped:.3e} index changes {int((ca[..., 0] != cb[..., 0]).sum())}")
            q = f"l{i}_"
            if worst <= 0.5e-3:
                tol, flip = 0.0, 0.0  # the project's contract (util.assert_close defaults, no outlier)
            elif c["mode"] == S.MODE_PCF:
                tol, flip = 0.0, 2.0 * flipped
                assert flipped <= 1e-3, f"{c['name']}: {flipped:.3e} of the pixels flip between the reference's own builds -- move the relief"
            else:
                tol, flip = 2.0 * worst, 0.0
                assert tol < 0.02, f"{c['name']}: the reference's own builds differ by {worst:.3e} -- raise fVSMBias"
            fx[q + "attribs"], fx[q + "frame_size"], fx[q + "params"] = np.frombuffer(bytes(A), np.uint8), np.array([c["W"], c["H"]], np.int32), np.array([c["mode"], c["across"], c["best"]], np.uint32)
            fx[q + "light"], fx[q + "cascade"] = la, ca
            fx[q + "tol"], fx[q + "flip_budget"], fx[q + "cap"] = np.array(tol), np.array(flip), np.array(PCF_CAP[max(A.iFixedFilterSize, 0)] if c["mode"] == S.MODE_PCF else 0.0)
            fx[q + "strict_vs_contracted"] = np.array([worst, flipped])
        for (W, H), (cam, frame) in frames.items():
            fx[f"camera_{W}x{H}"], fx[f"frame_{W}x{H}"] = cam, frame
    path = os.path.join(HERE, "shadows_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
