#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/shadows16_golden.npz: the REFERENCE's shadow conversion and filterable look-ups with the 16-bit filterable formats
that ShadowMapManager.cpp:98-102 selects when Is32BitFilterableFmt is false -- RG16_UNORM (VSM), RG16_FLOAT (EVSM2), RGBA16_FLOAT (EVSM4), bIs32BitEVSM = 0
(:157: the exponents are clamped to 5.54, Shadows.fxh:280-285).

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, default /root/reference); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_shadows16.py

The cases' shapes, the look-up units, the inputs and the two flag sets are those of make_golden_shadows.py / make_golden_grid.py, imported as they are.  The
conversion wrapper below #includes ShadowConversions.fx by name at generation time and holds none of its text; between the two draws, and after the last, it does
what the targets of that format do to a value (the intermediate target has the filterable map's own format, ShadowMapManager.cpp:120-123):
    UNORM16   NaN -> 0, clamp to [0, 1], x 65535, + 0.5, truncate; a load returns code / 65535 (correctly rounded);
    binary16  round to nearest even, overflow -> infinity (integer arithmetic on the bits, written here).
The outputs are stored as CODES (uint16 / float16).  Look-up cases read the stored codes of the strict build, widened to fp32.

Both builds are run (strict fp32, and -ffp-contract=fast -march=native) under the rule of make_golden_shadows.py: a look-up whose two builds stay within 0.5e-3 with
no flipped pixel is held to the project's contract; otherwise its stored budget is twice the measured difference, and the generator asserts a flipped share of at
most 1e-3 and a tolerance below 0.02.  Conversion codes of the two builds may differ by one step of the format at most (asserted; the largest is stored)."""
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
import make_golden_grid as MG  # noqa: E402
import make_golden_shadows as MS  # noqa: E402
import ref_prep  # noqa: E402
import shadows_util as S  # noqa: E402

F = np.float32
FMT_U16X2, FMT_F16X2, FMT_F16X4 = 512, 64, 8  # MIFX_FORMAT_*
FMT_OF_MODE = {S.MODE_VSM: FMT_U16X2, S.MODE_EVSM2: FMT_F16X2, S.MODE_EVSM4: FMT_F16X4}

CONVERT16_UNIT = MG.PRELUDE + MS.ARRAY_PRELUDE + r"""
#define Texture2DArray ConvArray
namespace hlsl { namespace cv16 {
#include "ShaderDefinitions.fxh"
#include "ShadowConversions.fx"
}}
#undef Texture2DArray
#include <cstdint>
namespace
{
// a render-target write of R16_UNORM and the load of the code it wrote
uint16_t unorm16_code(float v)
{
    v = v != v ? 0.0f : (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v));
    volatile float s = v * 65535.0f; // (rounded before the addition also where the build contracts)
    return uint16_t(unsigned(s + 0.5f));
}
float unorm16_value(uint16_t c) { return float(double(c) / 65535.0); }
// fp32 -> binary16, round to nearest even, overflow -> infinity, NaN stays NaN; and back
uint16_t half_code(float f)
{
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return uint16_t(sign | 0x7E00u);
    if (a >= 0x47800000u) return uint16_t(sign | 0x7C00u); // >= 65536 (65520 .. 65536 rounds up to infinity below)
    if (a < 0x38800000u)                                   // below the smallest normal half: a multiple of 2^-24
    {
        if (a < 0x33000000u) return uint16_t(sign);        // < 2^-25 rounds to zero (2^-25 itself is a tie to even: zero)
        const int      e    = int(a >> 23);                // biased fp32 exponent, 102 .. 112
        const uint32_t m    = (a & 0x7FFFFFu) | 0x800000u;
        const int      sh   = 126 - e;                     // m * 2^(e - 150) / 2^-24 = m >> (126 - e)
        uint32_t       q    = m >> sh;
        const uint32_t rem  = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
        if (rem > half || (rem == half && (q & 1u))) ++q;
        return uint16_t(sign | q);
    }
    uint32_t       q   = (a - 0x38000000u) >> 13; // exponent rebias 127 -> 15, 10 mantissa bits
    const uint32_t rem = a & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ++q; // (a carry into the exponent is the right answer, up to 0x7C00 = infinity)
    return uint16_t(sign | q);
}
float half_value(uint16_t h)
{
    const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    float          v;
    if (e == 0) v = std::ldexp(float(m), -24);
    else if (e == 31) v = m ? std::nanf("") : INFINITY;
    else v = std::ldexp(float(m | 0x400u), int(e) - 25);
    return sign ? -v : v;
}
uint16_t code_of(float v, int unorm) { return unorm ? unorm16_code(v) : half_code(v); }
float    value_of(uint16_t c, int unorm) { return unorm ? unorm16_value(c) : half_value(c); }
}
// ShadowMapManager::ConvertToFilterable's loop (ShadowMapManager.cpp:547-598) with the radii given and both targets of a 16-bit format; out: slices x h x w x ch codes
extern "C" int ref_shadow_convert16(const float* depth, int w, int h, int slices, const float* radii, float ePos, float eNeg, int evsm, int skipBlur, int ch, int unorm, uint16_t* out)
{
    using namespace hlsl;
    std::vector<float> mid(size_t(w) * h * 4);
    for (int s = 0; s < slices; ++s)
    {
        cv16::g_Attribs.iCascade              = s;
        cv16::g_Attribs.fHorzFilterRadius     = radii[2 * s];
        cv16::g_Attribs.fVertFilterRadius     = radii[2 * s + 1];
        cv16::g_Attribs.fEVSMPositiveExponent = ePos;
        cv16::g_Attribs.fEVSMNegativeExponent = eNeg;
        cv16::g_Attribs.Is32BitEVSM           = false;
        cv16::g_tex2DShadowMap.slices = slices;
        for (int k = 0; k < slices; ++k) cv16::g_tex2DShadowMap.slice[k] = Image{depth + size_t(k) * w * h, w, h, 1};
        uint16_t* dst = out + size_t(s) * w * h * ch;
        ref_fullscreen<cv16::FullScreenTriangleVSOutput>(w, h, 0u, [&](cv16::FullScreenTriangleVSOutput& vs, int x, int y) {
            const float4 m = evsm ? cv16::EVSMHorzPS(vs) : cv16::VSMHorzPS(vs);
            for (int k = 0; k < 4; ++k) mid[(size_t(y) * w + x) * 4 + k] = k < ch ? value_of(code_of(m.d[k], unorm), unorm) : 0.0f; // (the target keeps ch channels of its format)
            if (skipBlur) for (int k = 0; k < ch; ++k) dst[(size_t(y) * w + x) * ch + k] = code_of(m.d[k], unorm);
        });
        if (skipBlur) continue;
        cv16::g_tex2DShadowMap.slices   = 1;
        cv16::g_tex2DShadowMap.slice[0] = Image{mid.data(), w, h, 4};
        ref_fullscreen<cv16::FullScreenTriangleVSOutput>(w, h, 0u, [&](cv16::FullScreenTriangleVSOutput& vs, int x, int y) {
            const float4 m = cv16::VertBlurPS(vs);
            for (int k = 0; k < ch; ++k) dst[(size_t(y) * w + x) * ch + k] = code_of(m.d[k], unorm);
        });
    }
    return int(sizeof(cv16::ConversionAttribs));
}
extern "C" void ref_half_codes(const float* in, int n, uint16_t* out) { for (int i = 0; i < n; ++i) out[i] = half_code(in[i]); }
"""


def conversion_cases():
    """The shapes of make_golden_shadows.conversion_cases() that exercise every path of the conversion, each in the three 16-bit formats: 13x9x1 with the size-2
    filter (the horizontal pass alone), 3 and 7 (the halo outside the slice on every side); 50x38x3 with the two world-radius sets (inside the fused kernel's range and
    beyond it); 260x70x2 (five tiles across, a width that is no multiple of 64)."""
    base = {c["name"]: c for c in MS.conversion_cases()}
    world, large = base["conv_50x38_m3_world"], base["conv_50x38_m2_world_large"]
    cs = []
    for mode in (S.MODE_VSM, S.MODE_EVSM2, S.MODE_EVSM4):
        for fs in (2, 3, 7):
            cs.append(dict(name=f"conv16_13x9_m{mode}_f{fs}", w=13, h=9, n=1, mode=mode, over=dict(iFixedFilterSize=fs)))
        cs.append(dict(name=f"conv16_50x38_m{mode}_world", w=50, h=38, n=3, mode=mode, over=dict(world["over"]), radii=world["radii"]))
        cs.append(dict(name=f"conv16_50x38_m{mode}_world_large", w=50, h=38, n=3, mode=mode, over=dict(large["over"]), radii=large["radii"]))
        cs.append(dict(name=f"conv16_260x70_m{mode}_f3", w=260, h=70, n=2, mode=mode, over=dict(iFixedFilterSize=3)))
    for c in cs:
        c["over"]["bIs32BitEVSM"] = 0
    return cs


def lookup_cases():
    """make_golden_shadows.lookup_cases() without the PCF ones (which read no filterable map), bIs32BitEVSM = 0"""
    cs = [dict(c, over=dict(c["over"], bIs32BitEVSM=0)) for c in MS.lookup_cases() if c["mode"] != S.MODE_PCF]
    assert {(c["W"], c["H"]) for c in cs} == {(67, 45), (2, 2), (1, 1)} and {c["mode"] for c in cs} == {S.MODE_VSM, S.MODE_EVSM2, S.MODE_EVSM4}
    return cs


def widen(codes, fmt):
    """float32 values of stored codes"""
    if fmt == FMT_U16X2:
        return (codes.astype(np.float64) / 65535.0).astype(F)
    return codes.astype(F)


def step_of(values, fmt):
    """One step of the format at each value: 1 / 65535, or the spacing of binary16 there"""
    if fmt == FMT_U16X2:
        return np.full(values.shape, 1.0 / 65535.0)
    return np.abs(np.spacing(np.asarray(values, np.float16))).astype(np.float64)


def run_convert16(lib, A, depth, mode, radii):
    n, h, w = depth.shape
    ch = 4 if mode == S.MODE_EVSM4 else 2
    out = np.zeros((n, h, w, ch), np.uint16)
    r = np.ascontiguousarray(radii, F)
    size = lib.ref_shadow_convert16(MS.fp(depth), w, h, n, MS.fp(r), ctypes.c_float(min(A.fEVSMPositiveExponent, 5.54)), ctypes.c_float(min(A.fEVSMNegativeExponent, 5.54)),
                                    int(mode != S.MODE_VSM), int(A.iFixedFilterSize == 2), ch, int(mode == S.MODE_VSM), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
    assert size == 24, size
    return out if mode == S.MODE_VSM else out.view(np.float16)


def main():
    assert os.path.isdir(os.path.join(MG.REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    conv, look = conversion_cases(), lookup_cases()
    units = {"convert16": CONVERT16_UNIT}
    for c in look:
        units[f"lookup_{c['mode']}_{c['across']}_{c['best']}_0"] = MS.lookup_unit(c["mode"], c["across"], c["best"], 0)
    fx = {"conv_names": np.array([c["name"] for c in conv]), "look_names": np.array([c["name"] for c in look])}
    with tempfile.TemporaryDirectory(prefix="mifx_shadows16_golden_") as tmp:
        assert ref_prep.main(MG.REFERENCE_ROOT, tmp) == 0
        with open(os.path.join(MG.REFERENCE_ROOT, "Shaders/Shadows/private/ShadowConversions.fx"), encoding="utf-8", errors="replace") as f:
            open(os.path.join(tmp, "ShadowConversions.fx"), "w").write(ref_prep.transform(f.read()))
        p = os.path.join(tmp, "BasicStructures.fxh")
        text, k = re.subn(r"#ifdef\s+__cplusplus(\s+float\s+fCascadeCamSpaceZEnd)", r"#if 0\1", open(p).read())
        assert k == 1
        open(p, "w").write(text)
        strict, fast = MG.build(units, MG.STRICT, tmp, "strict"), MG.build(units, MG.CONTRACTED, tmp, "fast")

        # the wrapper's binary16 rounding against numpy's, on every fp32 exponent around the half range and on ties
        probe = np.concatenate([np.linspace(-70000, 70000, 20001), 2.0 ** np.arange(-30, 17), (1.0 + 2.0 ** -11) * 2.0 ** np.arange(-26, 16), (1.0 + 3 * 2.0 ** -11) * 2.0 ** np.arange(-26, 16),
                                np.random.default_rng(0).standard_normal(20000) * 1e-5, [65519.99, 65520.0, 0.0, -0.0, np.inf]]).astype(F)
        codes = np.zeros(probe.size, np.uint16)
        strict.ref_half_codes(MS.fp(probe), probe.size, codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)))
        with np.errstate(over="ignore"):
            assert np.array_equal(codes, probe.astype(np.float16).view(np.uint16)), "the wrapper's binary16 rounding is not round-to-nearest-even"

        # ---- conversions
        for i, c in enumerate(conv):
            fmt = FMT_OF_MODE[c["mode"]]
            A = S.make_attribs(c["n"], c["w"], c["h"], **c["over"])
            for k, r in enumerate(c.get("radii", ())):
                A.Cascades[k].f4LightSpaceScale[0], A.Cascades[k].f4LightSpaceScale[1] = 4.0 * r[0] / c["w"], 4.0 * r[1] / c["h"]
            depth = S.periodic_slices(c["n"], c["w"], c["h"])
            radii = MS.radii_of(A, c["w"], c["h"])
            a, b = run_convert16(strict, A, depth, c["mode"], radii), run_convert16(fast, A, depth, c["mode"], radii)
            va, vb = widen(a, fmt), widen(b, fmt)
            assert np.isfinite(va).all(), c["name"]
            steps = float((np.abs(va.astype(np.float64) - vb) / step_of(va, fmt)).max())
            print(f"{c['name']:36s} radii {radii.reshape(-1)}  strict vs contracted: {int((a.view(np.uint16) != b.view(np.uint16)).sum())} of {a.size} codes differ, by at most {steps:.2f} steps")
            assert steps <= 1.0, f"{c['name']}: the reference's own two builds differ by {steps} steps of the format"
            q = f"v{i}_"
            fx[f"depth_{c['w']}x{c['h']}x{c['n']}"] = depth  # (one per shape: the three formats convert the same slices)
            fx[q + "attribs"], fx[q + "mode"], fx[q + "fmt"], fx[q + "out"], fx[q + "radii"] = (np.frombuffer(bytes(A), np.uint8), np.array(c["mode"], np.uint32), np.array(fmt, np.uint32),
                                                                                              a, radii)
            fx[q + "strict_vs_contracted_steps"] = np.array(steps)

        # ---- look-ups from the reference's 16-bit conversion (3x3) of the first three slices of make_golden_shadows' depth array
        slices = S.shadow_slices(8, MS.MAP_W, MS.MAP_H)[:3].copy()
        Aconv = S.make_attribs(3, MS.MAP_W, MS.MAP_H, iFixedFilterSize=3, bIs32BitEVSM=0)
        r3 = MS.radii_of(Aconv, MS.MAP_W, MS.MAP_H)
        maps = {m: run_convert16(strict, Aconv, slices, m, r3) for m in (S.MODE_VSM, S.MODE_EVSM2, S.MODE_EVSM4)}
        # stored once: the depth slices are shadows_golden.npz's map_depth[:3]; the RG16_FLOAT map is the first two channels of the RGBA16_FLOAT one (one shader, the
        # same rounding per channel)
        assert np.array_equal(slices, np.load(os.path.join(HERE, "shadows_golden.npz"))["map_depth"][:3])
        assert np.array_equal(maps[S.MODE_EVSM2].view(np.uint16), maps[S.MODE_EVSM4][..., :2].view(np.uint16))
        fx["map_conv_attribs"], fx["map_vsm"], fx["map_evsm4"] = np.frombuffer(bytes(Aconv), np.uint8), maps[S.MODE_VSM], maps[S.MODE_EVSM4]
        frames = {}
        for i, c in enumerate(look):
            cam = S.frame_camera(c["W"], c["H"])
            frame = S.frame_depth(cam, c["W"], c["H"])
            frames.setdefault((c["W"], c["H"]), (cam, frame))
            A = S.make_attribs(c["n"], MS.MAP_W, MS.MAP_H, **c["over"])
            arr = np.ascontiguousarray(widen(maps[c["mode"]], FMT_OF_MODE[c["mode"]]))
            (la, ca), (lb, cb) = MS.run_lookup(strict, c, cam, A, frame, arr), MS.run_lookup(fast, c, cam, A, frame, arr)
            assert np.isfinite(la).all() and np.isfinite(ca).all(), c["name"]
            d = np.abs(la.astype(np.float64) - lb)
            flipped, worst = float((d > 1e-3).mean()), float(d.max())
            changes = int((ca[..., 0] != cb[..., 0]).sum())
            print(f"{c['name']:32s} {c['W']}x{c['H']} lit {float((la > 0.99).mean()):.2f} dark {float((la < 0.01).mean()):.2f}  strict vs contracted: max {worst:.3e} flipped {flipped:.3e} "
                  f"index changes {changes}")
            assert changes == 0, c["name"]
            if worst <= 0.5e-3:
                tol = 0.0  # the project's contract (util.assert_close defaults, no outlier)
            else:
                tol = 2.0 * worst
                assert flipped <= 1e-3, f"{c['name']}: {flipped:.3e} of the pixels flip between the reference's own builds -- raise fVSMBias, move the depth ramp"
                assert tol < 0.02, f"{c['name']}: the reference's own builds differ by {worst:.3e} -- raise fVSMBias"
            q = f"l{i}_"
            fx[q + "attribs"], fx[q + "frame_size"], fx[q + "params"] = np.frombuffer(bytes(A), np.uint8), np.array([c["W"], c["H"]], np.int32), np.array([c["mode"], c["across"], c["best"]], np.uint32)
            fx[q + "light"], fx[q + "cascade"], fx[q + "tol"] = la, ca, np.array(tol)
            fx[q + "strict_vs_contracted"] = np.array([worst, flipped])
        for (W, H), (cam, frame) in frames.items():
            fx[f"camera_{W}x{H}"], fx[f"frame_{W}x{H}"] = cam, frame
    path = os.path.join(HERE, "shadows16_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200_000


if __name__ == "__main__":
    main()
