#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/oit_golden.npz: what the REFERENCE's layered order-independent transparency makes of the cases of tests/oit_util.py --
Shaders/PBR/private/OIT/ClearOITLayers.csh, UpdateOITLayers.psh and ApplyOITAttenuation.psh with Shaders/Common/public/OIT.fxh, and GetOITTransmittance of
Shaders/PBR/private/RenderPBR.psh, compiled for the CPU from the reference tree where it lies.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, default /root/reference); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_oit.py

The shader text is read at generation time, rewritten by oracle/ref_prep.py into a temporary directory and compiled there through oracle/ref/hlsl_shim.h with the small
wrappers below, which #include the reference files by name and hold none of their text.  Nothing compiled is kept.  The fixture holds data only: the inputs of a case
are regenerated from its description by tests/oit_util.py.

Compiled whole: OIT.fxh, ClearOITLayers.csh, ApplyOITAttenuation.psh.  UpdateOITLayers.psh: its `main` (lines 51-110), taken out of the text at generation time -- the
file's includes pull in the whole material system; the wrapper supplies g_Frame, the depth buffer (USE_MANUAL_DEPTH_TEST), the layers buffer and GetBaseColor as the
slice's texel.  RenderPBR.psh: its `main` cannot be compiled, so GetOITTransmittance (lines 389-418) is taken out of the text and the few lines around its call are
restated in the wrapper with their line numbers, as oracle/ref/ref_pl_body.inc does for the shade.

What the wrappers add (the conventions of include/mifx.h, "layered order-independent transparency"):
  * StructuredBuffer / RWStructuredBuffer<uint> and a serial InterlockedMin (one invocation at a time per pixel: a slice has one fragment per pixel);
  * stub files for the two `.generated` includes of ApplyOITAttenuation.psh (four colour outputs);
  * coverage (the shade's background test), the depth test of the colour pass (the rule of UpdateOITLayers.psh:57-62; no opaque depth = one at infinity);
  * the blend states, dst = src * sf + dst * df in fp32 in that order: BS_UpdateOITTail and BS_OITAttenuation (PBR/src/PBR_Renderer.cpp:1849-1865, 2309-2324) and the
    transparent pass' rgb One / One, alpha One / InvSrcAlpha (:2096-2127); the tail keeps fp32 (count, transmittance) and is cleared to (0, 1).

Every case is built twice: strict fp32 (the oracle's flags) and with -ffp-contract=fast -march=native.  The layers and the tail's count must be equal; the largest
difference of the tail's transmittance and of the targets, in the measure of util.assert_close, is stored and must stay within 0.5e-3: then the project's contract
(util.assert_close at its defaults) is the right bar for the device."""
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
import make_golden_grid as MG  # noqa: E402  (the two flag sets and the compile step)
import oit_util as O  # noqa: E402
import ref_prep  # noqa: E402
import util  # noqa: E402

REFERENCE_ROOT = MG.REFERENCE_ROOT
F = np.float32

PRELUDE = r"""
#include "ref_common.h"
#include <cstring>
#include <limits>
namespace hlsl
{
template <class T> struct StructuredBuffer   { const T* p = nullptr; const T& operator[](uint i) const { return p[i]; } };
template <class T> struct RWStructuredBuffer { T* p = nullptr; T& operator[](uint i) const { return p[i]; } };
// one invocation at a time per pixel
inline void InterlockedMin(uint& dest, uint value, uint& original) { original = dest; if (value < dest) dest = value; }
}
static int g_num_oit_layers = 0;
#define NUM_OIT_LAYERS g_num_oit_layers
static void bind_plane(hlsl::TexStorage& s, const float* data, int w, int h, int c)
{
    s.mips = 1;
    s.mip[0].data = data;
    s.mip[0].w = w; s.mip[0].h = h; s.mip[0].c = c;
}
// dst = src * sf + dst * df
static inline float blend(float src, float sf, float dst, float df) { return src * sf + dst * df; }
// the shade's background test (diligentfx_amd/csrc/mifx_device.h is_background)
static inline bool is_background(float depth, bool reversed) { return reversed ? depth < 1e-6f : depth >= (1.0f - 1e-6f); }
"""

CLEAR_UNIT = PRELUDE + r"""
namespace hlsl { namespace oit {
#include "ClearOITLayers.csh"
}}
extern "C" int ref_oit_clear(unsigned* layers, const void* cam, int W, int H, int K)
{
    using namespace hlsl;
    std::memcpy(&oit::g_Camera, cam, sizeof(oit::g_Camera));
    g_num_oit_layers = K;
    oit::g_rwOITLayers.p = layers;
    for (int y = 0; y < H + 3; ++y) // (threads beyond the frame, as a dispatch of whole groups has)
        for (int x = 0; x < W + 5; ++x) oit::main(uint3(uint(x), uint(y), 0u));
    return int(sizeof(oit::g_Camera));
}
"""

UPDATE_UNIT = PRELUDE + r"""
namespace hlsl { namespace oit {
#include "BasicStructures.fxh"
#include "OIT.fxh"
struct VSOutput { float4 ClipPos; };
struct RendererParams { float MipBias; };
struct FrameAttribs { CameraAttribs Camera; RendererParams Renderer; };
static FrameAttribs g_Frame;
struct PrimitiveAttribs { float4 FallbackColor; };
static PrimitiveAttribs g_Primitive;
#define PRIMITIVE g_Primitive
struct MaterialInfo { int unused; };
static MaterialInfo g_Material;
static float4 g_SliceBaseColor;
inline float4 GetBaseColor(const VSOutput&, const MaterialInfo&, float, const float4&) { return g_SliceBaseColor; }
#define USE_MANUAL_DEPTH_TEST 1
static Texture2D_<float> g_DepthBuffer;
static RWStructuredBuffer<uint> g_rwOITLayers;
struct PSOutput { float4 Color; };
#include "UpdateOITLayers_main.inc"
}}
// one draw; tail: H x W x 4 (count, -, -, transmittance); opaque may be null
extern "C" int ref_oit_update(unsigned* layers, float* tail, const float* depth, const float* base, const float* opaque, const void* cam, int W, int H, int K)
{
    using namespace hlsl;
    std::memcpy(&oit::g_Frame.Camera, cam, sizeof(oit::g_Frame.Camera));
    const bool reversed = oit::g_Frame.Camera.fNearPlaneDepth > oit::g_Frame.Camera.fFarPlaneDepth;
    const float S = oit::g_Frame.Camera.fNearPlaneDepth < oit::g_Frame.Camera.fFarPlaneDepth ? +1.0f : -1.0f;
    std::vector<float> none(size_t(W) * H, S * std::numeric_limits<float>::infinity()); // no opaque depth: one that no fragment reaches
    bind_plane(oit::g_DepthBuffer.s, opaque ? opaque : none.data(), W, H, 1);
    g_num_oit_layers = K;
    oit::g_rwOITLayers.p = layers;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
        {
            const size_t i = size_t(y) * W + x;
            if (is_background(depth[i], reversed)) continue; // the slice has no fragment here
            oit::VSOutput vs;
            vs.ClipPos = float4(float(x) + 0.5f, float(y) + 0.5f, depth[i], 1.0f);
            oit::g_SliceBaseColor = float4(base[4 * i], base[4 * i + 1], base[4 * i + 2], base[4 * i + 3]);
            g_ctx.discarded = false;
            const oit::PSOutput o = oit::main(vs, true);
            if (g_ctx.discarded) continue;
            float* t = tail + 4 * i; // BS_UpdateOITTail: rgb One / One, alpha Zero / SrcAlpha
            t[0] = blend(o.Color.x, 1.0f, t[0], 1.0f);
            t[1] = blend(o.Color.y, 1.0f, t[1], 1.0f);
            t[2] = blend(o.Color.z, 1.0f, t[2], 1.0f);
            t[3] = blend(o.Color.w, 0.0f, t[3], o.Color.w);
        }
    return int(sizeof(oit::g_Frame.Camera));
}
"""

ATTENUATE_UNIT = PRELUDE + r"""
#undef discard
#define discard do { ::hlsl::g_ctx.discarded = true; return; } while (0) // (the shim's returns a value; this main returns void)
namespace hlsl { namespace oit {
#include "ApplyOITAttenuation.psh"
}}
extern "C" int ref_oit_attenuate(const unsigned* layers, const float* tail, float* color, float* base, float* material, float* ibl, const void* cam, int W, int H, int K)
{
    using namespace hlsl;
    std::memcpy(&oit::g_Camera, cam, sizeof(oit::g_Camera));
    g_num_oit_layers = K;
    oit::g_OITLayers.p = layers;
    bind_plane(oit::g_OITTail.s, tail, W, H, 4);
    float* rt[4] = {color, base, material, ibl};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
        {
            oit::FullScreenTriangleVSOutput vs;
            vs.f4PixelPos = float4(float(x) + 0.5f, float(y) + 0.5f, 0.0f, 1.0f);
            g_ctx.discarded = false;
            oit::PSOutput o;
            oit::main(vs, o);
            if (g_ctx.discarded) continue;
            const float4 src[4] = {o.Color0, o.Color1, o.Color2, o.Color3};
            for (int k = 0; k < 4; ++k) // BS_OITAttenuation: every channel Zero / SrcAlpha
            {
                float* d = rt[k] + 4 * (size_t(y) * W + x);
                for (int c = 0; c < 4; ++c) d[c] = blend(src[k].d[c], 0.0f, d[c], src[k].w);
            }
        }
    return int(sizeof(oit::g_Camera));
}
"""

BLEND_UNIT = PRELUDE + r"""
namespace hlsl { namespace oit {
#include "BasicStructures.fxh"
#include "OIT.fxh"
struct FrameAttribs { CameraAttribs Camera; };
static FrameAttribs g_Frame;
static StructuredBuffer<uint> g_OITLayers;
static Texture2D_<float4> g_OITTail;
#include "RenderPBR_GetOITTransmittance.inc"
}}
static void blend_rt(float* d, const hlsl::float4& s) // the transparent pass with OITLayerCount > 0 (PBR_Renderer.cpp:2096-2127): rgb One / One, alpha One / InvSrcAlpha
{
    d[0] = blend(s.x, 1.0f, d[0], 1.0f);
    d[1] = blend(s.y, 1.0f, d[1], 1.0f);
    d[2] = blend(s.z, 1.0f, d[2], 1.0f);
    d[3] = blend(s.w, 1.0f, d[3], 1.0f - s.w);
}
// one transparent draw of the colour pass; alpha and opaque may be null
extern "C" int ref_oit_blend(const unsigned* layers, const float* tail, const float* depth, const float* base, const float* material, const float* radiance, const float* sibl,
                             const float* alpha, const float* opaque, float* color, float* tbase, float* tmaterial, float* tibl, const void* cam, int W, int H, int K)
{
    using namespace hlsl;
    std::memcpy(&oit::g_Frame.Camera, cam, sizeof(oit::g_Frame.Camera));
    const oit::CameraAttribs& Camera = oit::g_Frame.Camera;
    const bool reversed = Camera.fNearPlaneDepth > Camera.fFarPlaneDepth;
    g_num_oit_layers = K;
    oit::g_OITLayers.p = layers;
    bind_plane(oit::g_OITTail.s, tail, W, H, 4);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
        {
            const size_t i = size_t(y) * W + x;
            if (is_background(depth[i], reversed)) continue; // the slice has no fragment here
            if (opaque)                                      // the depth test: the rule of UpdateOITLayers.psh:57-62
            {
                const float S = Camera.fNearPlaneDepth < Camera.fFarPlaneDepth ? +1.0f : -1.0f;
                if (depth[i] * S >= opaque[i] * S) continue;
            }
            float4 BaseColor = float4(base[4 * i], base[4 * i + 1], base[4 * i + 2], base[4 * i + 3]); // RenderPBR.psh:424
            float3 OutRGB = float3(radiance[4 * i], radiance[4 * i + 1], radiance[4 * i + 2]);         // :514, the slice's shade
            const float OutA = alpha ? alpha[i] : BaseColor.w;                                         // :515-523
            float Transmittance = 1.0f;                                                                // :544
            OutRGB = OutRGB * BaseColor.w;                                                             // :547
            if (BaseColor.w > OIT_OPACITY_THRESHOLD)                                                   // :549
            {
                float D = depth[i];                                                                    // :551
                if (Camera.fNearPlaneDepth > Camera.fFarPlaneDepth) D = 1.0f - D;                      // :552-555
                Transmittance = oit::GetOITTransmittance(D, uint2(uint(x), uint(y)));                  // :556
            }
            OutRGB = OutRGB * Transmittance;                                                           // :632
            float2 MaterialData = float2(material[4 * i], material[4 * i + 1]);                        // USD_Renderer.cpp:98
            float3 IBL = float3(sibl[4 * i], sibl[4 * i + 1], sibl[4 * i + 2]);                        // :99
            MaterialData = MaterialData * Transmittance;                                               // :122
            IBL = IBL * Transmittance;                                                                 // :123
            float3 BaseRGB = float3(BaseColor.x, BaseColor.y, BaseColor.z) * Transmittance;            // :124
            blend_rt(color + 4 * i, float4(OutRGB.x, OutRGB.y, OutRGB.z, OutA));                       // :132
            const float3 b = BaseRGB * BaseColor.w;                                                    // :157
            blend_rt(tbase + 4 * i, float4(b.x, b.y, b.z, BaseColor.w));
            const float2 m = MaterialData * BaseColor.w;                                               // :162
            blend_rt(tmaterial + 4 * i, float4(m.x, m.y, 0.0f, BaseColor.w));
            const float3 l = IBL * BaseColor.w;                                                        // :167
            blend_rt(tibl + 4 * i, float4(l.x, l.y, l.z, BaseColor.w));
        }
    return int(sizeof(oit::g_Frame.Camera));
}
"""

# one namespace per unit: the units are linked into one library
UNITS = {name: f"#define oit {name}\n" + text for name, text in (("oit_clear", CLEAR_UNIT), ("oit_update", UPDATE_UNIT), ("oit_attenuate", ATTENUATE_UNIT), ("oit_blend", BLEND_UNIT))}


def prepare(tmp):
    """The reference's text, rewritten for the shim, in the temporary directory"""
    assert ref_prep.main(REFERENCE_ROOT, tmp) == 0

    def read(rel):
        with open(os.path.join(REFERENCE_ROOT, rel), encoding="utf-8", errors="replace") as f:
            return f.read()

    for name in ("ClearOITLayers.csh", "ApplyOITAttenuation.psh"):  # (ref_prep.main does not descend into Shaders/PBR/private/OIT)
        text = ref_prep.transform(read("Shaders/PBR/private/OIT/" + name))
        text = re.sub(r"\[\s*numthreads\s*\([^\]]*\)\s*\]", "", text)
        open(os.path.join(tmp, name), "w").write(text)
    body = ref_prep._extract_definition(ref_prep._strip_comments(read("Shaders/PBR/private/OIT/UpdateOITLayers.psh")), "PSOutput main(")
    open(os.path.join(tmp, "UpdateOITLayers_main.inc"), "w").write(ref_prep.transform(body))
    body = ref_prep._extract_definition(ref_prep._strip_comments(read("Shaders/PBR/private/RenderPBR.psh")), "float GetOITTransmittance(")
    open(os.path.join(tmp, "RenderPBR_GetOITTransmittance.inc"), "w").write(ref_prep.transform(body))
    # ApplyOITAttenuation.psh:13-19 and :56-59 describe what the renderer generates: one colour per render target, all of them OutColor
    open(os.path.join(tmp, "PSOutputStruct.generated"), "w").write("struct PSOutput { float4 Color0; float4 Color1; float4 Color2; float4 Color3; };\n")
    open(os.path.join(tmp, "PSMainFooter.generated"), "w").write("PSOut.Color0 = OutColor; PSOut.Color1 = OutColor; PSOut.Color2 = OutColor; PSOut.Color3 = OutColor;\n")


def up(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def run_case(lib, c, d):
    """(layers (H, W, K) uint32, tail (H, W, 2), targets (4, H, W, 4)) of the reference's sequence: clear, L updates, attenuation, L colour draws"""
    w, h, k, n = c["w"], c["h"], c["k"], c["l"]
    cam = np.ascontiguousarray(d["camera"], F).tobytes()
    layers = np.full((h, w, k), 0xDEADBEEF, np.uint32)
    assert lib.ref_oit_clear(up(layers), cam, w, h, k) == 576
    tail = np.zeros((h, w, 4), F)
    tail[..., 3] = 1  # HnBeginOITPassTask.cpp:139-144
    for i in range(n):
        assert lib.ref_oit_update(up(layers), fp(tail), fp(d["depth"][i]), fp(d["base"][i]), fp(d["opaque"]), cam, w, h, k) == 576
    t = [np.ascontiguousarray(d["targets"][j]).copy() for j in range(4)]
    assert lib.ref_oit_attenuate(up(layers), fp(tail), fp(t[0]), fp(t[1]), fp(t[2]), fp(t[3]), cam, w, h, k) == 576
    for i in range(n):
        alpha = None if d["alpha"] is None else d["alpha"][i]
        assert lib.ref_oit_blend(up(layers), fp(tail), fp(d["depth"][i]), fp(d["base"][i]), fp(d["material"][i]), fp(d["radiance"][i]), fp(d["ibl"][i]), fp(alpha), fp(d["opaque"]),
                                 fp(t[0]), fp(t[1]), fp(t[2]), fp(t[3]), cam, w, h, k) == 576
    return layers, np.ascontiguousarray(tail[..., [0, 3]]), np.stack(t)


def end_to_end(lib):
    """The end-to-end case (tests/oit_util.py e2e_inputs): the two slices shaded by the reference's own shade (oracle/_ref: RenderPBR.psh's lighting half), then the
    reference's OIT sequence over them."""
    import chain_util
    import pyref

    ref = pyref.ref_lib()
    assert ref is not None, "oracle/_ref is not built: run build() of __graft_entry__.py where the reference tree is mounted"
    ibl = chain_util.make_ibl(ref, "ref_")
    sa = chain_util.shade_attribs(len(ibl["prefiltered"]) - 1)
    e = O.e2e_inputs()
    h, w = O.E2E["h"], O.E2E["w"]
    rad, spec = np.zeros((2, h, w, 4), F), np.zeros((2, h, w, 4), F)
    for i, g in enumerate(e["gbuffers"]):
        ref.call("ref_pbr_shade", [g["base_color"], g["normal"], g["material"], g["depth"], None, None, ibl["lut"], ibl["irradiance"], ibl["prefiltered"]], [rad[i], spec[i]],
                 cam0=bytes(e["camera"]), attribs=bytes(sa), fval=[0.0, 0.0, 0.0, 0.0])
    assert np.isfinite(rad).all() and float(rad[..., :3].max()) > 0.1
    d = dict(depth=np.stack([g["depth"] for g in e["gbuffers"]]), base=np.stack([g["base_color"] for g in e["gbuffers"]]),
             material=np.stack([g["material"] for g in e["gbuffers"]]), radiance=rad, ibl=spec, alpha=None, opaque=None, targets=e["targets"],
             camera=np.frombuffer(bytes(e["camera"]), F))
    layers, tail, targets = run_case(lib, O.E2E, d)
    print(f"{O.E2E['name']:28s} layers in use {int((layers != 0xFFFFFFFF).sum()):6d}  texels changed {int((targets != e['targets']).any(-1).sum()):6d}")
    return layers, tail, targets


def main():
    assert os.path.isdir(os.path.join(REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    cs = O.cases()
    fx = {"names": np.array([c["name"] for c in cs])}
    with tempfile.TemporaryDirectory(prefix="mifx_oit_golden_") as tmp:
        prepare(tmp)
        strict, fast = MG.build(UNITS, MG.STRICT, tmp, "strict"), MG.build(UNITS, MG.CONTRACTED, tmp, "fast")
        for i, c in enumerate(cs):
            d = O.make_case(c)
            (la, ta, ga), (lb, tb, gb) = run_case(strict, c, d), run_case(fast, c, d)
            assert np.isfinite(ta).all() and np.isfinite(ga).all(), c["name"]
            assert np.array_equal(la, lb) and np.array_equal(ta[..., 0], tb[..., 0]), f"{c['name']}: the layers or the tail count differ between the reference's own builds"
            diff = max(float(util.rel_err(tb[..., 1], ta[..., 1]).max()), float(util.rel_err(gb, ga).max()))
            frags = int((la != 0xFFFFFFFF).sum())
            print(f"{c['name']:28s} layers in use {frags:6d}  tail pixels {int((ta[..., 0] > 0).sum()):5d}  texels changed {int((ga != d['targets']).any(-1).sum()):6d}  "
                  f"strict vs contracted: max rel {diff:.3e}")
            assert diff <= 0.5e-3, f"{c['name']}: the reference's own two builds differ by {diff:.3e} -- change the case"
            q = f"c{i}_"
            fx[q + "layers"], fx[q + "tail"], fx[q + "targets"], fx[q + "strict_vs_contracted"] = la, ta, ga, np.array(diff)
        fx["e2e_layers"], fx["e2e_tail"], fx["e2e_targets"] = end_to_end(strict)
    path = os.path.join(HERE, "oit_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
