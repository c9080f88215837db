#!/usr/bin/env python3
"""Timing of the shade's G-buffer targets at 3840 x 2160, all five layers, five lights of which two are shadow-mapped, in one process: HIP events around repeated calls on the
library's stream, at least 0.3 s of warm-up before every measurement, medians over blocks of about 0.05 s, the blocks of one job alternating.

  kernel: mifx_pbr_shade_targets against mifx_pbr_shade_output (identity case and everything on; every output plane allocated once), and beside them the time
          mifx_debug_stream_copy takes to write the bytes of the four added planes (64 B per pixel; the copy reads as many: the yardstick is generous);
  chain:  the chain with layers, targets off against targets on, in one stream and in overlap mode 5, for the identity desc and for highlight + TRANSITIONING at 0.4.

    python tools/shade_targets_bench.py --out profiles/shade_targets_bench.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
W, H = 3840, 2160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=float, default=0.3, help="seconds of warm-up before every measurement")
    ap.add_argument("--window", type=float, default=0.05, help="seconds per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per variant (alternating)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import chain_util
    import shade_output_util as S
    from diligentfx_amd import api, binding as B, synth
    from util import blue_noise_tables

    def warm(fns):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warm:
            for fn in fns:
                for _ in range(4):
                    fn()
            torch.cuda.synchronize()

    def calibrate(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(4):
            fn()
        b.record()
        torch.cuda.synchronize()
        return max(4, int(args.window / max(a.elapsed_time(b) / 4e3, 1e-7)))

    def timed_us(fns):
        """Blocks of the variants alternate after one warm-up over all of them; the median block of each, in microseconds per call"""
        warm(fns)
        iters = [calibrate(fn) for fn in fns]
        blocks = [[] for _ in fns]
        for _ in range(args.blocks):
            for k, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters[k]):
                    fn()
                b.record()
                torch.cuda.synchronize()
                blocks[k].append(a.elapsed_time(b) * 1000.0 / iters[k])
        return [statistics.median(v) for v in blocks]

    ctx = api.PostFXContext(0)
    ctx.set_static_ibl(True)
    dev = ctx.device
    ibl = api.precompute_ibl(ctx, synth.make_sky_cube(64, dev), lut_size=128, irradiance_size=16, prefiltered_size=128, lut_samples=128, diffuse_samples=256, specular_samples=64)
    sa = chain_util.shadowed_shade_attribs(len(ibl.pre) - 1)
    slices, infos = chain_util.make_shadow_inputs()
    shadows = (torch.from_numpy(np.stack(slices)).to(dev), infos, 3)
    f = synth.make_frame(synth.Scene(), 3, W, H, dev)
    g = {k: f[k] for k in ("base_color", "normal", "material", "depth")}
    gen = torch.Generator(device=dev).manual_seed(5)
    r = lambda *s: torch.rand(*s, device=dev, generator=gen)  # noqa: E731
    g["base_color"] = torch.cat([g["base_color"][..., :3], 0.05 + 0.9 * r(H, W, 1)], -1).contiguous()
    n = f["normal"][..., :3]
    t = r(H, W, 3) - 0.5
    t = t - n * (t * n).sum(-1, keepdim=True)
    z = torch.zeros(H, W, 1, device=dev)
    ang = 6.2831853 * r(H, W, 1)
    nrm = torch.nn.functional.normalize
    planes = {"clearcoat": torch.cat([r(H, W, 1), 0.05 + 0.95 * r(H, W, 1), z, z], -1), "clearcoat_normal": torch.cat([nrm(n + 0.3 * (r(H, W, 3) - 0.5), dim=-1), z], -1),
              "sheen": torch.cat([r(H, W, 3), 0.05 + 0.95 * r(H, W, 1)], -1), "anisotropy": torch.cat([torch.cos(ang), torch.sin(ang), r(H, W, 1), z], -1),
              "tangent": torch.cat([nrm(t, dim=-1), z], -1), "iridescence": torch.cat([r(H, W, 1), 100.0 + 300.0 * r(H, W, 1), z, z], -1), "transmission": r(H, W),
              "sheen_albedo_scaling_lut": 0.5 * r(32, 32), "preintegrated_charlie": 0.3 * r(32, 32)}
    planes = {k: v.contiguous() for k, v in planes.items()}
    kw = dict(background=S.BACKGROUND, iridescence_ior=S.IOR, anisotropy_rotation=S.ROTATION, shadows=shadows)
    new = lambda: torch.empty(H, W, 4, device=dev)  # noqa: E731
    out_color, out_spec = new(), new()
    out_targets = {k: new() for k in api.PBR_TARGET_PLANES}
    added_bytes = 4 * W * H * 16
    src, dst = torch.empty(added_bytes, dtype=torch.uint8, device=dev), torch.empty(added_bytes, dtype=torch.uint8, device=dev)
    copy = lambda: B.check(ctx.lib.mifx_debug_stream_copy(ctx.handle, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), ctypes.c_uint64(added_bytes)))  # noqa: E731
    cs = {c["name"]: c for c in S.cases()}
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H], "layers": S.ALL_LAYERS, "lights": int(sa.LightCount), "shadow_mapped_lights": 2,
           "method": f"median of {args.blocks} blocks of about {args.window} s each after {args.warm} s of warm-up; the blocks of one job alternate",
           "added_bytes_per_frame": added_bytes, "kernel": {}, "chain": {}}
    for key, c in (("identity", cs["none"]), ("everything", cs["everything"])):
        desc = S.output_desc_fields(c)
        base = lambda d=desc: api.pbr_shade_output(ctx, g, planes, S.ALL_LAYERS, f["camera"], sa, ibl, output=d, out_color=out_color, out_specular_ibl=out_spec, **kw)  # noqa: E731
        case = lambda d=desc: api.pbr_shade_targets(ctx, g, planes, S.ALL_LAYERS, f["camera"], sa, ibl, output=d, out_color=out_color, out_targets=out_targets, **kw)  # noqa: E731
        base_us, case_us, copy_us = timed_us([base, case, copy])
        res["kernel"][key] = {"shade_output_us": base_us, "shade_targets_us": case_us, "added_us": case_us - base_us, "stream_copy_of_added_bytes_us": copy_us,
                              "added_over_copy": (case_us - base_us) / copy_us}
    ctx.close()

    # the chain with layers, targets off against targets on, for two descs: the identity desc, and highlight + TRANSITIONING at 0.4 (whose footer raises the roughness the later
    # passes see: SSR's work depends on the planes it reads, so "on" against "off" is the cost of the planes plus whatever the other values change downstream)
    descs = {"identity": S.output_desc_fields(cs["none"]), "highlight_transitioning_04": S.output_desc_fields(dict(cs["none"], highlight=0.35, anim=S.ANIM_TRANSITIONING, factor=0.4))}
    sobol, tile = blue_noise_tables()
    for name, desc in descs.items():
        for mode in (0, 5):
            chains, fns = [], []
            for targets in (False, True):
                chain = api.Chain(0, sobol, tile)
                chain.postfx.set_static_ibl(True)
                chain.set_overlap(mode)
                chain.set_material_layers(planes, S.ALL_LAYERS, S.IOR, S.ROTATION, shadows=shadows)
                chain.set_shade_output(desc, targets)
                out = new()
                state = {"i": 0}

                def frame(chain=chain, out=out, state=state):
                    chain.execute(chain.bind_frame(state["i"], f, ibl, sa, out))
                    state["i"] += 1

                chains.append(chain)
                fns.append(frame)
            off_us, on_us = timed_us(fns)
            res["chain"].setdefault(name, {})[f"overlap_{mode}"] = {"targets_off_us": off_us, "targets_on_us": on_us, "added_us": on_us - off_us}
            torch.cuda.synchronize()
            for chain in chains:
                chain.close()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
