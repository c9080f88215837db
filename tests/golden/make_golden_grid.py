#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/grid_golden.npz: inputs and outputs of the REFERENCE's coordinate grid (Shaders/Common/private/CoordinateGridPS.psh with
Shaders/Common/public/CoordinateGrid.fxh) and of its copy-frame pass (Hydrogent/shaders/HnCopyFrame.psh), compiled for the CPU from the reference tree where it lies.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT, default /root/reference); never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_grid.py

The shader text is read at generation time, rewritten by oracle/ref_prep.py into a temporary directory and compiled there through oracle/ref/hlsl_shim.h with the small
wrappers below, which #include the reference files by name and hold none of their text; one translation unit per permutation (the COORDINATE_GRID_* / TONE_MAPPING_MODE /
CONVERT_OUTPUT_TO_SRGB macros are compile-time in the reference).  Nothing compiled is kept.  The fixture holds data only: camera bytes, depth, attribs, flags, colour and
the outputs.

fwidth(float2): the shim has scalar ddx / ddy only, so the wrapper supplies fwidth(float2) on the shim's own two-phase quad mechanism (phase 0 records the value of every
lane of the 2x2 quad, phase 1 replays: fine derivatives, ddx = right - left of the lane's row, ddy = bottom - top of its column).  A lane outside the frame (last column /
row of an odd-sized frame) runs at its own pixel centre, as a rasteriser's helper lane does.

Every case is built twice: strict fp32 (the oracle's flags) and with -ffp-contract=fast -march=native.  The small cases are held to 1e-3 / no outlier by the tests, so
the generator asserts that the reference alone keeps half of that between its two builds (0.5e-3) on every stored small case.  For the window of a 3840x2160 frame the
largest strict-versus-contracted difference is measured and twice that is stored as `window_tolerance`."""
import concurrent.futures
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_util as G  # noqa: E402
import ref_prep  # noqa: E402

REFERENCE_ROOT = os.environ.get("MIFX_REFERENCE_ROOT", "/root/reference")
STRICT = ["-O2", "-fPIC", "-fopenmp", "-fsingle-precision-constant", "-ffp-contract=off", "-fno-fast-math", "-w"]
CONTRACTED = ["-O2", "-fPIC", "-fopenmp", "-fsingle-precision-constant", "-ffp-contract=fast", "-march=native", "-fno-fast-math", "-w"]
F = np.float32

PRELUDE = r"""
#include "ref_common.h"
namespace hlsl
{
// fwidth(float2) on the shim's two-phase quad mechanism (g_ctx.quad_phase / quad_lane), with its own record (up to 16 calls per invocation)
struct GridQuadRec { int idx = 0; float2 rec[4][16]; };
inline thread_local GridQuadRec g_grid_quad;
inline float2 fwidth(const float2& v)
{
    ExecCtx& c = g_ctx;
    GridQuadRec& q = g_grid_quad;
    if (c.quad_phase < 0) return float2(0.f, 0.f);
    const int k = q.idx++;
    if (c.quad_phase == 0) { q.rec[c.quad_lane][k] = v; return float2(0.f, 0.f); }
    const int l = c.quad_lane, row = l & 2, col = l & 1;
    const float2 dx = q.rec[row + 1][k] - q.rec[row][k], dy = q.rec[col + 2][k] - q.rec[col][k];
    return float2(std::fabs(dx.x) + std::fabs(dy.x), std::fabs(dx.y) + std::fabs(dy.y));
}
}
// Runs `ps(vs, lx, ly, real)` over the window [x0, x0 + w) x [y0, y0 + h) (x0, y0 even) of a W x H frame, quad by quad in two phases; f4PixelPos is window-relative
// (the textures hold the window), f2NormalizedXY that of the frame.
template <class VSOUT, class PS> static void run_quads(int W, int H, int x0, int y0, int w, int h, PS&& ps)
{
    using namespace hlsl;
#pragma omp parallel for schedule(dynamic, 2)
    for (int qy = 0; qy < (h + 1) / 2; ++qy)
        for (int qx = 0; qx < (w + 1) / 2; ++qx)
        {
            for (int phase = 0; phase < 2; ++phase)
                for (int lane = 0; lane < 4; ++lane)
                {
                    const int lx = qx * 2 + (lane & 1), ly = qy * 2 + (lane >> 1), x = x0 + lx, y = y0 + ly;
                    VSOUT vs;
                    vs.f4PixelPos     = float4(float(lx) + 0.5f, float(ly) + 0.5f, 0.0f, 1.0f);
                    vs.f2NormalizedXY = float2(2.0f * ((float(x) + 0.5f) / float(W)) - 1.0f, 1.0f - 2.0f * ((float(y) + 0.5f) / float(H)));
                    vs.uInstID        = 0u;
                    g_ctx.discarded   = false;
                    g_ctx.quad_phase  = phase;
                    g_ctx.quad_lane   = lane;
                    g_ctx.call_idx    = 0;
                    g_grid_quad.idx   = 0;
                    ps(vs, lx, ly, phase == 1 && lx < w && ly < h);
                }
            g_ctx.quad_phase = -1;
        }
}
static void bind_plane(hlsl::TexStorage& s, const float* data, int w, int h, int c)
{
    s.mips = 1;
    s.mip[0].data = const_cast<float*>(data);
    s.mip[0].w = w; s.mip[0].h = h; s.mip[0].c = c;
}
"""


def flag_macros(flags, srgb_macro=None):
    m = {"COORDINATE_GRID_PLANE_YZ": G.FLAG_YZ, "COORDINATE_GRID_PLANE_XZ": G.FLAG_XZ, "COORDINATE_GRID_PLANE_XY": G.FLAG_XY, "COORDINATE_GRID_AXIS_X": G.FLAG_AXIS_X,
         "COORDINATE_GRID_AXIS_Y": G.FLAG_AXIS_Y, "COORDINATE_GRID_AXIS_Z": G.FLAG_AXIS_Z}
    s = "".join(f"#define {k} {1 if flags & v else 0}\n" for k, v in m.items())
    if srgb_macro:
        s += f"#define {srgb_macro} {1 if flags & G.FLAG_SRGB else 0}\n"
    return s


def render_unit(flags):
    """CoordinateGridPS.psh (ComputeGridAxesPS) for one FEATURE_FLAGS value"""
    return PRELUDE + flag_macros(flags, "COORDINATE_GRID_CONVERT_OUTPUT_TO_SRGB") + f"""
#define gg gg_{flags} // (one namespace per permutation: the units are linked into one library)
namespace hlsl {{ namespace gg {{
#include "ShaderDefinitions.fxh"
#include "CoordinateGridPS.psh"
}}}}
extern "C" int ref_grid_{flags}(const void* cam, const void* attribs, const float* depth, int W, int H, int x0, int y0, int w, int h, float* out)
{{
    using namespace hlsl;
    std::memcpy(&gg::g_Camera, cam, sizeof(gg::CameraAttribs));
    std::memcpy(&gg::g_GridAxesAttribs, attribs, sizeof(gg::CoordinateGridAttribs));
    bind_plane(gg::g_TextureDepth.s, depth, w, h, 1);
    run_quads<gg::FullScreenTriangleVSOutput>(W, H, x0, y0, w, h, [&](const gg::FullScreenTriangleVSOutput& vs, int lx, int ly, bool store) {{
        const float4 r = gg::ComputeGridAxesPS(vs);
        if (store) for (int k = 0; k < 4; ++k) out[(size_t(ly) * w + lx) * 4 + k] = r.d[k];
    }});
    return int(sizeof(gg::CoordinateGridAttribs));
}}
"""


def copy_unit(flags, mode, srgb):
    """HnCopyFrame.psh (main) for one permutation"""
    grid = "#define ENABLE_GRID 1\n" if flags & G.ALL else ""
    return PRELUDE + flag_macros(flags) + grid + f"""
#define TONE_MAPPING_MODE {mode}
#define CONVERT_OUTPUT_TO_SRGB {1 if srgb else 0}
#define PBR_MAX_LIGHTS 16
#define ENABLE_SHADOWS 0
#define USE_IBL 1
#define cf cf_{flags}_{mode}_{1 if srgb else 0} // (one namespace per permutation: the units are linked into one library)
namespace hlsl {{ namespace cf {{
#include "ShaderDefinitions.fxh"
#include "HnCopyFrame.psh"
}}}}
extern "C" int ref_copy_{flags}_{mode}_{1 if srgb else 0}(const void* cam, const void* post, const float* color, const float* depth, int W, int H, float* out)
{{
    using namespace hlsl;
    std::memset(&cf::g_Frame, 0, sizeof(cf::g_Frame));
    std::memcpy(&cf::g_Frame.Camera, cam, sizeof(cf::CameraAttribs));
    std::memcpy(&cf::g_Attribs, post, sizeof(cf::PostProcessAttribs));
    bind_plane(cf::g_ColorBuffer.s, color, W, H, 4);
    bind_plane(cf::g_Depth.s, depth, W, H, 1);
    run_quads<cf::FullScreenTriangleVSOutput>(W, H, 0, 0, W, H, [&](const cf::FullScreenTriangleVSOutput& vs, int lx, int ly, bool store) {{
        float4 c;
        cf::main(vs, c);
        if (store) for (int k = 0; k < 4; ++k) out[(size_t(ly) * W + lx) * 4 + k] = c.d[k];
    }});
    return int(sizeof(cf::PostProcessAttribs));
}}
"""


def scene_depth(cam, W, H, kind, seed):
    """A depth plane: the far plane with blocks of geometry at several camera-space distances (in front of and behind the grid planes)."""
    far = cam[G.CAM_FAR_DEPTH]
    d = np.full((H, W), far, F)
    if kind == "far":
        return d
    rng = np.random.default_rng(seed)
    for z in (2.0, 4.0, 7.0, 12.0, 30.0):
        x0, y0 = int(rng.integers(0, W - 4)), int(rng.integers(0, H - 4))
        w, h = int(rng.integers(4, max(5, W // 3))), int(rng.integers(4, max(5, H // 2)))
        d[y0:y0 + h, x0:x0 + w] = G.camera_z_to_depth(np.float64(z), cam)
    return d


def scene_color(W, H, seed):
    rng = np.random.default_rng(seed)
    c = (rng.integers(0, 1024, (H, W, 4)) / 256.0).astype(F)  # HDR values in [0, 4), a few bits each
    c[..., 3] = (rng.integers(0, 5, (H, W)) / 4.0).astype(F)
    return c


def post_process_attribs(tm_words, ave_log_lum, grid):
    """PostProcessAttribs (HnPostProcessStructures.fxh:4-21): 16 floats, ToneMappingAttribs (48 bytes), CoordinateGridAttribs (192 bytes)"""
    head = np.zeros(16, F)
    head[9] = ave_log_lum
    return head.tobytes() + tm_words.tobytes() + grid.tobytes()


def tone_mapping_words(mode):
    """ToneMappingAttribs with the reference's defaults and the mode given: 12 four-byte words"""
    w = np.zeros(12, np.uint32)
    w[0] = mode
    w[2:3] = np.array([0.18], F).view(np.uint32)
    w[4:6] = np.array([3.0, 1.0], F).view(np.uint32)
    w[8:12] = np.array([1.0, 1.0, 1.0, 0.0], F).view(np.uint32)
    return w


def copy_flags(i, srgb):
    """Where several planes or axes overlap their alphas add up beyond 1, lerp(colour, grid.rgb, grid.a) then leaves a negative colour and LinearToSRGB of it is NaN -- in the
    reference as in the product.  The sRGB cases therefore draw one plane and one axis (alpha <= 1: every stored value is finite); the linear ones draw everything."""
    if not srgb:
        return G.ALL if i % 2 else (G.FLAG_XZ | G.AXES)
    return (G.FLAG_XZ | G.FLAG_AXIS_X) if i % 2 else (G.FLAG_XY | G.FLAG_AXIS_Y)


def cases():
    A = dict(eye=(3.0, 2.5, -6.0), at=(0.0, 0.5, 0.0))
    out = []
    for name, flags in (("plane_yz", G.FLAG_YZ), ("plane_xz", G.FLAG_XZ), ("plane_xy", G.FLAG_XY), ("axis_x", G.FLAG_AXIS_X), ("axis_y", G.FLAG_AXIS_Y), ("axis_z", G.FLAG_AXIS_Z),
                        ("all", G.ALL), ("all_srgb", G.ALL | G.FLAG_SRGB)):
        out.append(dict(name=name, kind="render", W=64, H=36, cam=dict(**A), flags=flags, depth="far" if flags < 126 else "blocks"))
    out.append(dict(name="orthographic", kind="render", W=64, H=36, cam=dict(eye=(3.0, 4.0, -6.0), at=(0.0, 0.0, 0.0), ortho_height=9.0, near=0.1, far=50.0), flags=G.ALL, depth="blocks"))
    out.append(dict(name="reversed_depth", kind="render", W=64, H=36, cam=dict(**A, reversed_depth=True), flags=G.ALL, depth="blocks"))
    out.append(dict(name="geometry", kind="render", W=64, H=36, cam=dict(eye=(-4.0, 3.0, 5.0), at=(0.5, 0.0, 0.0)), flags=G.FLAG_XZ | G.AXES, depth="blocks"))
    out.append(dict(name="jitter", kind="render", W=64, H=36, cam=dict(**A, jitter=(0.74 / 64, -0.42 / 36)), flags=G.ALL, depth="blocks"))
    out.append(dict(name="odd_size", kind="render", W=77, H=45, cam=dict(**A), flags=G.ALL, depth="blocks"))
    out.append(dict(name="all_160x90", kind="render", W=160, H=90, cam=dict(eye=(2.0, 1.5, -3.0), at=(0.0, 0.0, 0.0)), flags=G.ALL, depth="blocks"))
    for i, mode in enumerate((0, 1, 4, 7, 8, 10)):  # NONE, EXP (the Reinhard family's shape), UNCHARTED2, ADAPTIVE_LOG (the logarithmic ones), AGX, PBR_NEUTRAL (and COMMERCE)
        for srgb in (False, True):
            out.append(dict(name=f"copy_mode{mode}_{'srgb' if srgb else 'linear'}", kind="copy", W=48, H=28, cam=dict(**A, jitter=(0.3 / 48, 0.2 / 28)), mode=mode, srgb=srgb,
                            flags=copy_flags(i, srgb), depth="blocks"))
    out.append(dict(name="window_4k", kind="window", W=3840, H=2160, x0=1800, y0=1500, w=96, h=54, cam=dict(**A), flags=G.FLAG_XZ | G.AXES, depth="far"))
    return out


def build(units, flags, tmp, tag):
    def cc(item):
        name, text = item
        src = os.path.join(tmp, f"{name}.cpp")
        if not os.path.exists(src):
            open(src, "w").write(text)
        obj = os.path.join(tmp, f"{name}_{tag}.o")
        r = subprocess.run(["g++", "-std=c++20", "-c"] + flags + ["-I", os.path.join(ROOT, "oracle", "ref"), "-I", tmp, "-o", obj, src], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-6000:])
            raise RuntimeError(f"compiling {name} failed")
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(cc, units.items()))
    so = os.path.join(tmp, f"libgrid_{tag}.so")
    subprocess.run(["g++", "-shared", "-fopenmp", "-o", so] + objs, check=True)
    return ctypes.CDLL(so)


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def run_case(lib, c, data):
    cam, attribs, depth = data["camera"], data["attribs"], data["depth"]
    if c["kind"] == "copy":
        post = post_process_attribs(data["tone_mapping"], data["ave_log_lum"], attribs)
        out = np.zeros((c["H"], c["W"], 4), F)
        n = getattr(lib, f"ref_copy_{c['flags']}_{c['mode']}_{1 if c['srgb'] else 0}")(cam.tobytes(), post, fp(data["color"]), fp(depth), c["W"], c["H"], fp(out))
        assert n == len(post), (n, len(post))
        return out
    x0, y0, w, h = (c["x0"], c["y0"], c["w"], c["h"]) if c["kind"] == "window" else (0, 0, c["W"], c["H"])
    out = np.zeros((h, w, 4), F)
    n = getattr(lib, f"ref_grid_{c['flags']}")(cam.tobytes(), attribs.tobytes(), fp(depth), c["W"], c["H"], x0, y0, w, h, fp(out))
    assert n == 192, n
    return out


def main():
    assert os.path.isdir(os.path.join(REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    cs = cases()
    units = {}
    for c in cs:
        if c["kind"] == "copy":
            units[f"copy_{c['flags']}_{c['mode']}_{int(c['srgb'])}"] = copy_unit(c["flags"], c["mode"], c["srgb"])
        else:
            units[f"grid_{c['flags']}"] = render_unit(c["flags"])
    fixture = {"names": np.array([c["name"] for c in cs])}
    with tempfile.TemporaryDirectory(prefix="mifx_grid_golden_") as tmp:
        assert ref_prep.main(REFERENCE_ROOT, tmp) == 0
        for rel in ("Hydrogent/shaders/HnCopyFrame.psh", "Hydrogent/shaders/HnPostProcessStructures.fxh"):
            with open(os.path.join(REFERENCE_ROOT, rel), encoding="utf-8", errors="replace") as f:
                open(os.path.join(tmp, os.path.basename(rel)), "w").write(ref_prep.transform(f.read()))
        strict, fast = build(units, STRICT, tmp, "strict"), build(units, CONTRACTED, tmp, "fast")
        for i, c in enumerate(cs):
            cam = G.make_camera(c["W"], c["H"], **c["cam"])
            w, h = (c["w"], c["h"]) if c["kind"] == "window" else (c["W"], c["H"])
            data = dict(camera=cam, attribs=G.default_attribs(), depth=scene_depth(cam, w, h, c["depth"], 100 + i))
            if c["kind"] == "copy":
                data.update(color=scene_color(w, h, 200 + i), tone_mapping=tone_mapping_words(c["mode"]), ave_log_lum=F(0.3))
            a, b = run_case(strict, c, data), run_case(fast, c, data)
            assert np.isfinite(a).all() and a[..., 3].max() > 0.05, c["name"]
            diff = float(np.abs(a - b).max())
            print(f"{c['name']:24s} {w}x{h} flags {c['flags']:3d}  strict vs contracted: max {diff:.3e}  covered {float((a[..., 3] > 0).mean()) if c['kind'] != 'copy' else -1:.3f}")
            if c["kind"] == "window":
                fixture["window_tolerance"] = np.array(2.0 * diff, np.float64)
                fixture["window_strict_vs_contracted"] = np.array(diff, np.float64)
            else:
                assert diff <= 0.5e-3, f"{c['name']}: the reference's own two builds differ by {diff:.3e} > 0.5e-3 -- shrink the case"
            p = f"c{i}_"
            fixture[p + "kind"] = np.array(c["kind"])
            fixture[p + "frame"] = np.array([c["W"], c["H"], c.get("x0", 0), c.get("y0", 0)], np.int32)
            fixture[p + "flags"] = np.array(c["flags"], np.uint32)
            fixture[p + "out"] = a
            for k, v in data.items():
                fixture[p + k] = np.asarray(v)
            if c["kind"] == "copy":
                fixture[p + "tonemap_flags"] = np.array(1 if c["srgb"] else 0, np.uint32)
    path = os.path.join(HERE, "grid_golden.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes; window_tolerance", float(fixture["window_tolerance"]))
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
