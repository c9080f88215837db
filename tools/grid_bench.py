#!/usr/bin/env python3
"""Timing of the coordinate grid at 3840x2160 (HIP events around repeated launches on the library's stream; medians over blocks):
  * the copy-frame pass (mifx_copy_frame_render) with the XZ plane + three axes, with all planes + axes, and with no grid, against mifx_tonemap_execute on the same
    input -- also with the PARENT commit's library, whose tone map is the yardstick;
  * the stand-alone renderer (mifx_coordinate_grid_render) blended into a colour target;
  * the chain (mifx_chain_execute, overlap mode 5) per frame with the grid off and on, and the parent's frame.

One process measures one library (MIFX_LIB_PATH selects it; --parent: a library without the grid entries, only the tone map and the chain are measured); run the two
alternately and combine:

    python tools/grid_bench.py --out a0.json;  MIFX_LIB_PATH=<parent>/libmifx.so python tools/grid_bench.py --parent --out p0.json;  ... a1.json, p1.json ...
    python tools/grid_bench.py --combine a0.json p0.json a1.json p1.json --out profiles/grid_bench_4k.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

W, H = 3840, 2160


def combine(paths, out):
    runs = [json.load(open(p)) for p in paths]
    res = {"width": W, "height": H, "device": runs[0].get("device"), "runs": len(runs), "method": "median over runs of per-run medians; libraries alternated process by process"}
    for lib in ("current", "parent"):
        keys = sorted({k for r in runs if r["library"] == lib for k in r if k.endswith(("_us", "_ms_per_frame"))})
        for k in keys:
            v = [r[k] for r in runs if r["library"] == lib and k in r]
            res[f"{lib}_{k}"] = statistics.median(v)
            res[f"{lib}_{k}_all"] = v
    line = json.dumps(res, indent=1)
    print(line)
    if out:
        open(out, "w").write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--combine", nargs="+")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out)

    import numpy as np
    import torch

    from diligentfx_amd import api, binding as B, synth

    def timed_us(fn):
        for _ in range(5):  # warm clocks and caches
            fn()
        torch.cuda.synchronize()
        blocks = []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            blocks.append(a.elapsed_time(b) * 1000.0 / args.iters)
        return statistics.median(blocks)

    tables = np.load(os.path.join(ROOT, "tests", "golden", "blue_noise_tables.npz"))
    res = {"library": "parent" if args.parent else "current", "device": torch.cuda.get_device_name(0)}
    ctx = api.PostFXContext(0)
    frames = [synth.make_frame(synth.Scene(), i, W, H, ctx.device) for i in range(2)]
    f = frames[0]
    hdr = synth.make_hdr_buffer(W, H, ctx.device)
    out = torch.empty_like(hdr)
    tm = B.ToneMappingAttribs.default(4)
    res["tonemap_us"] = timed_us(lambda: ctx.tone_map(hdr, tm, 0.3, 1, out=out))
    if not args.parent:
        grid = B.CoordinateGridAttribs.default()
        xz_axes, everything = 4 | 16 | 32 | 64, 2 | 4 | 8 | 16 | 32 | 64
        cf = lambda flags: timed_us(lambda: ctx.copy_frame(hdr, f["depth"], f["camera"], tm, 0.3, 1, grid, flags, out=out))  # noqa: E731
        res["copy_frame_xz_axes_us"] = cf(xz_axes)
        res["copy_frame_all_us"] = cf(everything)
        res["copy_frame_xz_only_us"] = cf(4)
        res["copy_frame_no_grid_us"] = cf(0)
        r = api.CoordinateGridRenderer(ctx)
        target = hdr.clone()
        res["grid_render_blend_xz_axes_us"] = timed_us(lambda: r.render(f["depth"], f["camera"], grid, xz_axes, color_target=target))
    ibl = api.precompute_ibl(ctx, synth.make_sky_cube(32, ctx.device), lut_size=64, irradiance_size=8, prefiltered_size=32, lut_samples=64, diffuse_samples=128,
                             specular_samples=32)
    sa = synth.make_lights()
    sa.PrefilteredCubeLastMip = float(len(ibl.pre) - 1)
    for name, on in (("chain_mode5_ms_per_frame", False),) + (() if args.parent else (("chain_mode5_grid_ms_per_frame", True),)):
        chain = api.Chain(0, tables["sobol_256d"], tables["scrambling_tile"])
        chain.set_overlap(5)
        if on:
            chain.set_coordinate_grid(B.CoordinateGridAttribs.default(), 4 | 16 | 32 | 64)
        ldr = torch.zeros(H, W, 4, device=ctx.device)
        bound = [chain.bind_frame(i, frames[i % 2], ibl, sa, ldr) for i in range(args.frames + 3)]
        per_frame = []
        for _ in range(3):
            for i in range(3):
                chain.execute(bound[i])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(3, args.frames + 3):
                chain.execute(bound[i])
            e1.record()
            torch.cuda.synchronize()
            per_frame.append(e0.elapsed_time(e1) / args.frames)
        res[name] = statistics.median(per_frame)
        chain.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
