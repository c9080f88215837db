#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/shade_targets_golden.npz: what the REFERENCE's forward pixel shader with Hydrogent's footer behind it makes of the cases of
tests/shade_targets_util.py -- PSOut.Color, Normal, BaseColor, Material and IBL.  The footer is the text USD_Renderer::GetUsdPbrPSMainSource builds
(PBR/src/USD_Renderer.cpp:80-171): it is read out of that file at generation time -- the raw string between its opening `R"(` and closing `)"`, and the literals of the
`ss << "    PSOut.X = ...;"` statements around it -- rewritten by oracle/ref_prep.py and put behind the tail of `main` of RenderPBR.psh in the wrapper of
make_golden_shade_output.py, compiled once per pipeline permutation through oracle/ref/hlsl_shim.h.  Nothing of the reference's text is kept, here or in the fixture.

Run by hand where the reference tree is mounted (MIFX_REFERENCE_ROOT) and oracle/_ref is built; never by build(), smoke(), bench.py or a test:

    python tests/golden/make_golden_shade_targets.py

What the wrapper adds to the sibling's (the conventions of include/mifx.h, mifx_pbr_shade_targets):
  * UNSHADED 0 and PRIMITIVE.CustomData = 0 (MeshID is not an output of the entry); every USD_PSO_FLAG_ENABLE_*_OUTPUT on;
  * a pixel without a fragment (background, or discarded by the mask test) keeps the G-buffer's Normal / BaseColor / Material texel and gets a zero IBL;
  * ref_args has four outputs: Material and IBL share the fourth, eight channels wide.

The frame is the sibling fixture's with exact alpha and clear-coat factor bands (shade_targets_util.frame_inputs), so only results are stored, one (h, w) plane per distinct
channel.  Every case is built twice, strict fp32 and -ffp-contract=fast -march=native; the largest difference in the measure of util.assert_close is printed and stored."""
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
import make_golden_shade_output as MSO  # noqa: E402  (the wrapper of `main`'s tail, the permutation key, the unit text)
import pyref  # noqa: E402
import ref_prep  # noqa: E402
import shade_output_util as S  # noqa: E402
import shade_targets_util as T  # noqa: E402
import util  # noqa: E402

F = np.float32


def _sub(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def body():
    """The sibling's wrapper with the footer behind the tail and five outputs"""
    b = MSO.BODY
    b = _sub(b, "#define ENABLE_VOLUME 0\n", "#define ENABLE_VOLUME 0\n#define UNSHADED 0\n")
    b = _sub(b, "struct VSOutput { float4 ClipPos; float4 PrevClipPos; };\n",
             "struct VSOutput { float4 ClipPos; float4 PrevClipPos; };\n"
             "struct PSOutput { float4 Color, MeshID, MotionVec, Normal, BaseColor, Material, IBL; }; // (every USD_PSO_FLAG_ENABLE_*_OUTPUT, USD_Renderer.cpp:36-72)\n"
             "struct PrimitiveAttribs { float4 CustomData; };\n")
    b = _sub(b, "    const ref_img &o0 = a->out[0], &o1 = a->out[1];\n",
             "    const ref_img &o0 = a->out[0], &o1 = a->out[1], &o2 = a->out[2], &o3 = a->out[3]; // Color, Normal, BaseColor, Material | IBL (c = 8)\n"
             "    if (o3.c != 8) return 2;\n"
             "    auto store8 = [&](int x, int y, float4 m, float4 i) {\n"
             "        float* p = o3.data + (size_t(y) * o3.w + x) * 8;\n"
             "        p[0] = m.x; p[1] = m.y; p[2] = m.z; p[3] = m.w; p[4] = i.x; p[5] = i.y; p[6] = i.z; p[7] = i.w;\n"
             "    };\n"
             "    pbr::PrimitiveAttribs PRIMITIVE;\n"
             "    PRIMITIVE.CustomData = float4(0.f, 0.f, 0.f, 0.f);\n")
    b = _sub(b, "                if (o1.data) ref_store(o1, x, y, float4(0.f, 0.f, 0.f, 0.f));\n                continue;\n",
             "                ref_store(o1, x, y, pbr::g_Normal.Load(pc));\n"
             "                ref_store(o2, x, y, pbr::g_BaseColor.Load(pc));\n"
             "                store8(x, y, pbr::g_Material.Load(pc), float4(0.f, 0.f, 0.f, 0.f));\n"
             "                continue;\n")
    b = _sub(b, "            ref_store(o0, x, y, OutColor); // PSOut.Color = OutColor (:647)\n"
                "            if (o1.data) ref_store(o1, x, y, float4(pbr::GetBaseLayerSpecularIBL(Shading, SrfLighting), 1.0f));\n",
             '#include "USD_PSMainFooter.inc" // PSMainFooter.generated (RenderPBR.psh:645): USD_Renderer.cpp:80-168\n'
             "            ref_store(o0, x, y, PSOut.Color);\n"
             "            ref_store(o1, x, y, PSOut.Normal);\n"
             "            ref_store(o2, x, y, PSOut.BaseColor);\n"
             "            store8(x, y, PSOut.Material, PSOut.IBL);\n")
    return b


def footer_text():
    """The footer as GetUsdPbrPSMainSource assembles it with every output on: the string literals it streams into `ss`, in order, without the `return`"""
    with open(os.path.join(MSO.REFERENCE_ROOT, "PBR/src/USD_Renderer.cpp"), encoding="utf-8", errors="replace") as f:
        src = f.read()
    begin = src.index("std::stringstream ss;", src.index('PSMainInfo.OutputStruct = "#define PSOutput void'))
    src = src[begin:src.index("PSMainInfo.Footer = ss.str();", begin)]
    raw_open, raw_close = src.index('R"('), src.index(')";')
    assert 0 < raw_open < raw_close and src.count('R"(') == 1, "the footer's raw string moved"
    literal = re.compile(r'ss << "([^"\n]*)"')
    head = [m.group(1) for m in literal.finditer(src[:raw_open])]
    tail = [m.group(1) for m in literal.finditer(src[raw_close:])]
    assert head == ["    PSOutput PSOut;"] and tail[-1].strip() == "return PSOut;" and sum("PSOut." in t for t in tail) == 7, (head, tail)
    raw = src[raw_open + 3:raw_close]
    assert "Shading.Clearcoat.Factor" in raw and "LoadingAnimation.Factor" in raw and "Transmittance" in raw
    return "\n".join(head + [raw] + tail[:-1]) + "\n"


def prepare(tmp):
    MSO.prepare(tmp)
    open(os.path.join(tmp, "USD_PSMainFooter.inc"), "w").write(ref_prep.transform(footer_text()))
    open(os.path.join(tmp, "shade_targets_body.inc"), "w").write(body())


def run_case(lib, entry, c, d):
    from layers_util import LAYER_ORDER

    gn, ibl = d["gn"], d["ibl"]
    h, w = gn["depth"].shape
    color, normal, base, mi = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), np.zeros((h, w, 8), F)
    luts = [np.repeat(d["albedo"][..., None], 4, -1).copy(), np.repeat(d["charlie"][..., None], 4, -1).copy()]
    slices, infos = d["shadows"]
    lib.call(entry, [gn["base_color"], gn["normal"], gn["material"], gn["depth"], gn["emissive"], gn["occlusion"], ibl["lut"], ibl["irradiance"], ibl["prefiltered"],
                     [d["planes"][k] for k in LAYER_ORDER], luts, list(slices), np.ascontiguousarray(infos, F).reshape(1, -1), [d["motion"], d["mesh_normal"]]],
             [color, normal, base, mi], cam0=d["camera"], cam1=bytes(S.renderer_params(c)), attribs=bytes(d["attribs"]), ival=[c["cc_normal"], 1, c["alpha_mode"], c["unlit"], 0, 0, 0, 0],
             fval=list(S.BACKGROUND) + [S.IOR, S.ROTATION, S.CUTOFF])
    return dict(color=color, normal=normal, base_color=base, material=np.ascontiguousarray(mi[..., :4]), ibl=np.ascontiguousarray(mi[..., 4:]))


def main():
    assert os.path.isdir(os.path.join(MSO.REFERENCE_ROOT, "Shaders")), "the reference tree is not mounted"
    cs = T.cases()
    d = S.load_golden()
    d["gn"], d["planes"] = T.frame_inputs(d)
    keys = {}
    for c in cs:
        keys.setdefault(MSO.permutation(c), "p%02d" % len(keys))
    planes, lookup, index, worst = [], {}, np.zeros((len(cs), len(T.OUTPUTS), 4), np.int32), 0.0
    with tempfile.TemporaryDirectory(prefix="mifx_shade_targets_golden_") as tmp:
        prepare(tmp)
        units = {name: MSO.unit_text(key, name).replace("shade_output_body.inc", "shade_targets_body.inc") for key, name in keys.items()}
        print(len(cs), "cases,", len(units), "permutations")
        strict = pyref._Lib(MG.build(units, MG.STRICT, tmp, "strict")._name)
        fast = pyref._Lib(MG.build(units, MG.CONTRACTED, tmp, "fast")._name)
        for i, c in enumerate(cs):
            entry = "ref_so_" + keys[MSO.permutation(c)]
            a, b = run_case(strict, entry, c, d), run_case(fast, entry, c, d)
            diff = 0.0
            for j, o in enumerate(T.OUTPUTS):
                assert np.isfinite(a[o]).all(), (c["name"], o)
                diff = max(diff, float(util.rel_err(b[o], a[o]).max()))
                for ch in range(4):
                    p = np.ascontiguousarray(a[o][..., ch])
                    k = p.tobytes()
                    if k not in lookup:
                        lookup[k] = len(planes)
                        planes.append(p)
                    index[i, j, ch] = lookup[k]
            worst = max(worst, diff)
            geom = T.geometry(d["gn"], c)
            print(f"{c['name']:34s} material mean {a['material'][geom][:, :2].mean():7.4f}  ibl mean {a['ibl'][geom][:, :3].mean():7.4f}  strict vs contracted: max rel {diff:.3e}")
    print(f"largest difference between the reference's strict and contracted builds (util.rel_err): {worst:.3e}")
    geom = d["gn"]["depth"] < 1.0 - 1e-6
    al, cc = d["gn"]["base_color"][..., 3][geom], d["planes"]["clearcoat"][..., 0][geom]
    assert all((al == v).any() for v in (0.0, 0.5, 1.0)) and (cc == 0.0).any() and (cc == 1.0).any() and (~geom).any()
    path = os.path.join(HERE, "shade_targets_golden.npz")
    np.savez_compressed(path, names=np.array([c["name"] for c in cs]), planes=np.stack(planes), plane_index=index, strict_vs_contracted=np.array(worst))
    print(path, os.path.getsize(path), "bytes,", len(planes), "planes")
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
