#!/usr/bin/env python3
"""Builds diligentfx_amd/libmifx.so (HIP kernels + host objects + C ABI) for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this runs in the GPU-less build container; the .so is built in-tree
(git-ignored, but it travels to the GPU box with the snapshot)."""
import concurrent.futures
import glob
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libmifx.so")
OUT_H4 = os.path.join(HERE, "libmifx_h4.so")  # the same sources with -DMIFX_STORAGE_H4: 4-channel planes stored as RGBA16_FLOAT (include/mifx.h: mifx_storage_mode)
OBJDIR = os.path.join(HERE, "build")
ARCH = "gfx950"

# fp32 throughout, with the reference's operation sequence: no FMA contraction, correctly rounded division / square root, libm sin / cos /
# log2 (they feed discontinuous decisions: texel and mip selection, ray-march tile crossings, GGX terms with catastrophic cancellation --
# measured: contraction alone moves 0.5-5 % of the R4 / R5 / A3 texels by more than 1e-3).  Only exp / pow use the hardware
# transcendentals (mifx_device.h m_exp / m_pow: smooth weights and the sRGB curve, ~1e-6 relative error).  -ffast-math is never used: the
# TAA colour clip relies on IEEE NaN propagation and NaN-ignoring fmin / fmax (TAA_ComputeTemporalAccumulation.fx:98-106).
# A source file may add flags with a first line `// MIFX_BUILD_FLAGS: ...`.
HIPCC_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
    "-fvisibility=hidden", "-fno-slp-vectorize",
    "-Wno-unused-result", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
] + os.environ.get("MIFX_HIPCC_EXTRA", "").split()


# Sources whose multiply-adds may fuse (-ffp-contract=fast on top of the flags above): kernels that are smooth functions of their inputs, where one rounding
# instead of two is the more accurate result and ~10 % fewer VALU instructions.  MIFX_FMA_SOURCES (comma-separated basenames, "all", or "none") overrides
# the list for A/B builds.
# Measured (profiles/r02_ab_fma_contraction.txt): pbr.hip -10 % on the shade, taa.hip -6 % on TAA, every GPU parity test unchanged.  Fusing
# ssao.hip / ssr_temporal.hip as well gains 2 % more on those kernels but pushes SSAO end-to-end and the SSR per-pass cases over their outlier budgets
# (history-rejection thresholds), and whole-file fusion of the march (ssr_trace.hip), R5 (ssr.hip) and A3 (ssao_ao.hip) moves rays / taps: those stay strict
# and fuse only the expressions that carry an explicit __builtin_fmaf / MIFX_FMA_BLOCK.
# Round 4: NONE by default.  The contraction of pbr.hip / taa.hip / composite.hip (and hand-fused multiply-adds in SSR's march step, ssr_trace.hip) bought
# 1.0 % of the 4K frame (1.721 -> 1.740 ms, 1.724 -> 1.733 ms, two A/B pairs on one box: profiles/r04_ab_nofma_vs_fast.txt) and cost every value-level deviation the parity
# suite could still see per pass: with it 2.5e-4 of the shade's radiance values, 1.6e-4 .. 8.7e-4 of TAA's (by flag set) and 1.4e-3 of the ray march's differ from the
# reference by more than 1e-3; without it not one value of any per-pass comparison of the shade, TAA, R4, R5, R7, Bloom, SSAO A3 .. A8 or depth of field does
# (profiles/r04_parity_outliers_strict_vs_fast.txt; the per-pass budgets in tests/ are 0 since).  The contract puts parity before speed.  The list below is what
# MIFX_FMA_SOURCES=default restores for an A/B build.
FMA_SOURCES_FAST = ("pbr.hip", "taa.hip", "composite.hip")
FMA_SOURCES = ()
# How a fused source is compiled.  pbr.hip / taa.hip: plain `fast` (the backend fuses every multiply-add it finds).  composite.hip holds code that must NOT be
# contracted beside code that may (SSR's bilateral cleanup inside the composite kernel, mifx_ssr_cleanup.h): `fast-honor-pragmas` contracts the same expressions
# through per-instruction flags and lets `#pragma clang fp contract(off)` exempt a block -- under plain `fast` the backend fuses across the pragma (checked on the
# ISA: the cleanup compiles to the same instructions as under -ffp-contract=off only with fast-honor-pragmas).
FMA_MODE = {"composite.hip": "fast-honor-pragmas"}


def fma_sources():
    v = os.environ.get("MIFX_FMA_SOURCES")
    if v is None:
        return set(FMA_SOURCES)
    if v == "default":
        return set(FMA_SOURCES_FAST)
    if v == "all":
        return {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip"))}
    return {n for n in v.split(",") if n and n != "none"}


def hipcc():
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found: libmifx.so cannot be built (there is no CPU fallback)")
    return p


def _digest(paths, extra):
    h = hashlib.sha1(extra.encode())
    for p in sorted(paths):
        h.update(p.encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False, verbose=False):
    """Both libraries: libmifx.so (fp32 planes, the parity contract) and libmifx_h4.so (RGBA16_FLOAT 4-channel planes). Returns the path of the first."""
    out = build_variant(OUT, OBJDIR, [], force, verbose)
    build_variant(OUT_H4, os.path.join(OBJDIR, "h4"), ["-DMIFX_STORAGE_H4=1"], force, verbose)
    return out


def build_variant(OUT, OBJDIR, defines, force=False, verbose=False):
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")))
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(ROOT, "include", "mifx.h")])
    os.makedirs(OBJDIR, exist_ok=True)
    live = {os.path.basename(s) + ".o" for s in srcs}
    for stale in glob.glob(os.path.join(OBJDIR, "*.o")):  # objects of sources that were renamed / removed
        if os.path.basename(stale) not in live:
            os.remove(stale)
    fma = fma_sources()
    hdr_digest = _digest(hdrs, " ".join(HIPCC_FLAGS + defines))
    cc = hipcc()

    def compile_one(src):
        obj = os.path.join(OBJDIR, os.path.basename(src) + ".o")
        stamp = obj + ".stamp"
        fused = os.path.basename(src) in fma
        dig = _digest([src], hdr_digest + ("+fma" if fused else ""))
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
            return obj, False
        extra = []
        first = open(src).readline()
        if first.startswith("// MIFX_BUILD_FLAGS:"):
            extra = first.split(":", 1)[1].split()
        if fused:
            extra = extra + ["-ffp-contract=" + FMA_MODE.get(os.path.basename(src), "fast")]
        cmd = [cc] + HIPCC_FLAGS + defines + extra + (["-x", "hip"] if src.endswith(".hip") else []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
            raise RuntimeError(f"hipcc failed on {os.path.basename(src)}")
        if verbose and r.stderr.strip():
            sys.stderr.write(r.stderr)
        open(stamp, "w").write(dig)
        return obj, True

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        results = list(ex.map(compile_one, srcs))
    objs = [o for o, _ in results]
    if any(changed for _, changed in results) or not os.path.exists(OUT) or force:
        cmd = [cc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
            raise RuntimeError("linking libmifx.so failed")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
