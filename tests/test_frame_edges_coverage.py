"""Coverage guard (no GPU): every mifx_*_execute* entry point of include/mifx.h that takes a caller image -- directly or through its argument struct -- is run at
the boundary frame sizes (tests/test_gpu_frame_edges.py SIZE_MATRIX) and in every caller-plane layout (tests/test_gpu_plane_layouts.py LAYOUT_MATRIX), or is
listed below with the reason it is not.  A pass added to the ABI fails here until it has that coverage.  The same for the native-storage build: every such entry is run by
a section of tests/h4_checks.py (H4_MATRIX), or is listed in H4_EXCLUDED with the reason it is not."""
import ast
import os
import re

from util import ROOT

# entry point -> why it is not in the matrices
EXCLUDED = {
    "mifx_pbr_shade_execute_with_shadows": "the G-buffer and output addressing of mifx_pbr_shade_execute (the same kernel, one more shadow-map argument)",
    "mifx_pbr_shade_execute_layers": "the G-buffer and output addressing of mifx_pbr_shade_execute; the layer planes are held to the checker by test_gpu_pbr_layers.py",
    "mifx_pbr_shade_execute_frame_attribs": "mifx_pbr_shade_execute after a host-side conversion of the attribute block",
    "mifx_pbr_shade_execute_native": "native-format G-buffer planes (mifx_native_image), pitched by test_gpu_pbr.py::test_pbr_shade_on_native_gbuffer",
    "mifx_tonemap_execute_native": "mifx_tonemap_execute with a native-format target (mifx_native_image), pitched by test_formats.py",
    "mifx_chain_execute_native": "mifx_chain_execute with a native-format target (mifx_native_image), pitched by test_formats.py",
    "mifx_chain_execute_phase": "one row band of mifx_chain_execute's frame; test_gpu_sharded.py holds every band to the whole frame",
    "mifx_chain_execute_sharded": "row bands of mifx_chain_execute's frame over a communicator; test_gpu_sharded.py",
    "mifx_chain_execute_band": "one row band of mifx_chain_execute's frame without exchanges; test_gpu_sharded.py",
}


# The native-storage build (libmifx_h4.so: texels of 1, 2, 4 and 8 bytes) has its own table, tests/h4_checks.py H4_MATRIX: entry point -> the sections of that script that run
# it in that build.  entry point -> why no section does:
H4_EXCLUDED = {
    "mifx_composite_execute": "not run in this build: the chain's composite pass is the same pixel body (sections chain and edges against the checker, section fusion and "
                              "tests/test_gpu_composite_skip.py::test_native_storage_build across the fusion switches)",
    "mifx_composite_execute_selection": "not run in this build: mifx_composite_execute with the selection tail",
    "mifx_selection_execute": "fp32 planes in both builds; tests/test_gpu_selection.py::test_native_storage_build_gives_the_same_plane holds this build's plane to the fp32 build's",
    "mifx_pbr_shade_execute_with_shadows": "the G-buffer and output addressing of mifx_pbr_shade_execute_layers, which section layers runs with shadow maps",
    "mifx_pbr_shade_execute_frame_attribs": "mifx_pbr_shade_execute after a host-side conversion of the attribute block",
    "mifx_pbr_shade_execute_native": "native-format planes (mifx_native_image): their texel formats do not depend on the build",
    "mifx_tonemap_execute_native": "a native-format target (mifx_native_image): its texel format does not depend on the build",
    "mifx_chain_execute_native": "a native-format target (mifx_native_image); section grid checks that it is refused with the grid on",
    "mifx_chain_execute_phase": "one row band of mifx_chain_execute's frame; section sharded holds every band to the whole frame through mifx_chain_execute_sharded",
    "mifx_chain_execute_band": "one row band of mifx_chain_execute's frame without exchanges; as mifx_chain_execute_phase",
}


def _header():
    with open(os.path.join(ROOT, "include", "mifx.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def image_taking_executes():
    src = _header()
    structs = {m.group(2): m.group(1) for m in re.finditer(r"typedef struct \w*\s*\{(.*?)\}\s*(\w+)\s*;", src, flags=re.S)}
    holds = {"mifx_image2d"}
    for _ in range(4):  # structs that hold an image, or a struct that does
        holds |= {name for name, body in structs.items() if any(re.search(rf"\b{t}\b", body) for t in holds)}
    found = set()
    for m in re.finditer(r"MIFX_API\s+mifx_status\s+(mifx_\w*_execute\w*)\s*\((.*?)\)\s*;", src, flags=re.S):
        if any(re.search(rf"\b{t}\b", m.group(2)) for t in holds):
            found.add(m.group(1))
    return found


def _matrix(module, name):
    with open(os.path.join(ROOT, "tests", module)) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value), {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    raise AssertionError(f"{module} has no {name}")


def _h4_sections_run_by_the_suite():
    """The `section` values of tests/test_gpu_storage_h4.py::test_native_storage_build_against_the_format_emulating_checker"""
    with open(os.path.join(ROOT, "tests", "test_gpu_storage_h4.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "test_native_storage_build_against_the_format_emulating_checker":
            for d in node.decorator_list:
                if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize" and ast.literal_eval(d.args[0]) == "section":
                    return set(ast.literal_eval(d.args[1]))
    raise AssertionError("test_gpu_storage_h4.py: the parametrised section list was not found")


def test_every_image_pass_runs_in_the_native_storage_build():
    """H4_MATRIX of tests/h4_checks.py names, for every image-taking execute, the sections that run it in libmifx_h4.so; each named section exists and the suite runs it."""
    entries = image_taking_executes()
    matrix, functions = _matrix("h4_checks.py", "H4_MATRIX")
    run = _h4_sections_run_by_the_suite()
    assert set(H4_EXCLUDED) <= entries, f"stale exclusions: {sorted(set(H4_EXCLUDED) - entries)}"
    missing = sorted(entries - set(matrix) - set(H4_EXCLUDED))
    assert not missing, f"h4_checks.py: no H4_MATRIX entry for {missing} (run the pass in a section of the native-storage build, or add it to H4_EXCLUDED with a reason)"
    assert not set(matrix) & set(H4_EXCLUDED), f"both covered and excluded: {sorted(set(matrix) & set(H4_EXCLUDED))}"
    for entry, names in matrix.items():
        assert entry in entries, f"h4_checks.py: {entry} is not an image-taking execute of include/mifx.h"
        for s in names.split(", "):
            assert "section_" + s in functions, f"h4_checks.py: H4_MATRIX[{entry!r}] names section {s}, which the script does not define"
            assert s in run, f"H4_MATRIX[{entry!r}] names section {s}, which tests/test_gpu_storage_h4.py does not run"
    assert {"edges", "effects_thin"} <= {s for names in matrix.values() for s in names.split(", ")}  # (the boundary sizes are in the table)


def test_every_image_pass_has_edge_and_layout_coverage():
    entries = image_taking_executes()
    assert {"mifx_ssao_execute", "mifx_ssr_execute", "mifx_chain_execute", "mifx_tonemap_execute", "mifx_selection_execute"} <= entries  # (the parser sees them)
    assert set(EXCLUDED) <= entries, f"stale exclusions: {sorted(set(EXCLUDED) - entries)}"
    for module, name in (("test_gpu_frame_edges.py", "SIZE_MATRIX"), ("test_gpu_plane_layouts.py", "LAYOUT_MATRIX")):
        matrix, tests = _matrix(module, name)
        missing = sorted(entries - set(matrix) - set(EXCLUDED))
        assert not missing, f"{module}: no {name} entry for {missing} (add the pass to the matrix, or to EXCLUDED with a reason)"
        assert not set(matrix) & set(EXCLUDED), f"{module}: both covered and excluded: {sorted(set(matrix) & set(EXCLUDED))}"
        for entry, names in matrix.items():
            assert entry in entries, f"{module}: {entry} is not an image-taking execute of include/mifx.h"
            for t in names.split(", "):
                assert t in tests, f"{module}: {name}[{entry!r}] names {t}, which the module does not define"
