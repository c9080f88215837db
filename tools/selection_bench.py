#!/usr/bin/env python3
"""Timing of the selection outline at 3840x2160 (HIP events around repeated launches on the library's stream, one JSON object on stdout):
  * the jump flood (mifx_selection_execute) at max_distance 4 (the default: one launch) and 32 (three leading steps + the fused launch);
  * the composite (mifx_composite_execute) against the selection composite (mifx_composite_execute_selection);
  * the chain (mifx_chain_execute, overlap mode 5) per frame with selection off and on.

    python tools/selection_bench.py [--iters N] [--frames N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from diligentfx_amd import api, binding as B, synth  # noqa: E402
import selection_util as S  # noqa: E402

W, H = 3840, 2160


def timed_us(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tables = np.load(os.path.join(ROOT, "tests", "golden", "blue_noise_tables.npz"))
    res = {"width": W, "height": H, "device": torch.cuda.get_device_name(0)}

    ctx = api.PostFXContext(0)
    f = synth.make_frame(synth.Scene(), 2, W, H, ctx.device)
    depth = f["depth"].cpu().numpy()
    sel_np = S.make_selection_depth(depth, np.random.default_rng(1), seeds=12, max_radius=120)
    sd = torch.from_numpy(sel_np).to(ctx.device)
    fx = api.ProcessSelection(ctx)
    for d in (4.0, 32.0):
        a = B.SelectionAttribs.default(selection_id=1)
        a.max_distance = d
        res[f"jump_flood_us_max_distance_{int(d)}"] = timed_us(lambda: fx.execute(sd, a), args.iters)
        res[f"jump_flood_launches_max_distance_{int(d)}"] = max(S.iterations(d) - 3, 0) + 1

    ibl = api.precompute_ibl(ctx, synth.make_sky_cube(32, ctx.device), lut_size=64, irradiance_size=8, prefiltered_size=32, lut_samples=64, diffuse_samples=128,
                             specular_samples=32)
    gen = torch.Generator(device="cpu").manual_seed(3)
    color = torch.cat([torch.rand(H, W, 3, generator=gen).to(ctx.device) * 3.0, f["base_color"][..., 3:4]], -1).contiguous()
    spec, ssr, ssao = torch.rand(H, W, 4, generator=gen).to(ctx.device), torch.rand(H, W, 4, generator=gen).to(ctx.device), torch.rand(H, W, generator=gen).to(ctx.device)
    out = torch.empty_like(color)
    cargs = (ctx, color, spec, ssr, ssao, f["normal"], f["base_color"], f["material"], ibl.lut, f["camera"])
    a = B.SelectionAttribs.default(selection_id=1)
    fx.execute(sd, a)
    closest = fx.get_output()
    res["composite_us"] = timed_us(lambda: api.composite(*cargs, 1.0, 1.0, out=out), args.iters)
    res["composite_selection_us"] = timed_us(lambda: api.composite_selection(*cargs, f["depth"], sd, closest, a, 1.0, 1.0, out=out), args.iters)
    fx.close()

    sa = synth.make_lights()
    sa.PrefilteredCubeLastMip = float(len(ibl.pre) - 1)
    frames = [synth.make_frame(synth.Scene(), i, W, H, ctx.device) for i in range(2)]
    for name, on in (("chain_mode5_ms_per_frame", False), ("chain_mode5_selection_ms_per_frame", True)):
        chain = api.Chain(0, tables["sobol_256d"], tables["scrambling_tile"])
        chain.set_overlap(5)
        if on:
            chain.set_selection(a, sd)
        ldr = torch.zeros(H, W, 4, device=ctx.device)
        bound = [chain.bind_frame(i, frames[i % 2], ibl, sa, ldr) for i in range(args.frames + 3)]
        for i in range(3):
            chain.execute(bound[i])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(3, args.frames + 3):
            chain.execute(bound[i])
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / args.frames
        chain.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
