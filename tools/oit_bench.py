#!/usr/bin/env python3
"""Timing of the layered order-independent transparency (HIP events around repeated calls on the library's stream; at least 0.3 s of warm-up before every measurement,
medians over blocks of about 0.05 s, the blocks of an A/B pair alternating): 3840 x 2160, K = 4 layers, L = 2, 4 and 8 slices that cover every pixel, no opaque depth --
mifx_oit_build_layers and mifx_oit_resolve by the reference's sequence of launches (1 + L each) against the fused kernels (one launch each) in the same process
(mifx_oit_set_fusion), with the achieved bytes per second of each by the bytes its own shape moves per pixel

    sequence   build  4 K + 8 + L (2 * 4 K + 2 * 8 + 20)        resolve  128 + 4 K + 8 + L (128 + 68 + 4 K + 8)
    fused      build  L * 20 + 4 K + 8                          resolve  128 + L * 68 + 4 K + 8

beside the device's own copy rate measured in the same run.  Under MIFX_STORAGE=h4 (the native-storage build) the 4-channel planes are RGBA16_FLOAT: with the
texel size T = 8 instead of 16 the 20 / 68 / 128 above are 4 + T / 4 + 4 T / 8 T.

    python tools/oit_bench.py --out profiles/oit_bench.json
    MIFX_STORAGE=h4 python tools/oit_bench.py --out profiles/oit_bench_h4.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

W, H, K = 3840, 2160, 4
SLICES = (2, 4, 8)


def bytes_per_pixel(shape, what, n, k=K, t=16):
    """t: the size of a 4-channel texel, 16 (fp32 build) or 8 (native-storage build)"""
    if shape == "sequence":
        return 4 * k + 8 + n * (2 * 4 * k + 2 * 8 + 4 + t) if what == "build" else 8 * t + 4 * k + 8 + n * (8 * t + 4 * t + 4 + 4 * k + 8)
    return n * (4 + t) + 4 * k + 8 if what == "build" else 8 * t + n * (4 * t + 4) + 4 * k + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=float, default=0.3, help="seconds of warm-up before every measurement")
    ap.add_argument("--window", type=float, default=0.05, help="seconds per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per variant (alternating)")
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from diligentfx_amd import api, binding as B

    w, h = args.width, args.height

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

    def timed_us(variants):
        """variants: [(setup, fn)].  Blocks of the variants ALTERNATE (A B A B ...) after one warm-up over all of them; the median block of each, in microseconds per call."""
        for setup, fn in variants:
            setup()
            fn()
        warm([fn for _, fn in variants] if len(variants) == 1 else [lambda s=s_, f=f_: (s(), f()) for s_, f_ in variants])
        iters = []
        for setup, fn in variants:
            setup()
            iters.append(calibrate(fn))
        blocks = [[] for _ in variants]
        for _ in range(args.blocks):
            for k, (setup, fn) in enumerate(variants):
                setup()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters[k]):
                    fn()
                b.record()
                torch.cuda.synchronize()
                blocks[k].append(a.elapsed_time(b) * 1000.0 / iters[k])
        return [statistics.median(v) for v in blocks]

    nothing = lambda: None  # noqa: E731
    ctx = api.PostFXContext(0)
    ctx.sync_stream()
    lib = ctx.lib
    default_fusion = lib.mifx_oit_set_fusion(1)
    lib.mifx_oit_set_fusion(default_fusion)
    dtype4 = B.storage_dtype()  # the 4-channel texel of the library build
    texel = 8 if dtype4 == torch.float16 else 16
    res = {"device": torch.cuda.get_device_name(0), "frame": [w, h], "layers": K, "fusion_default": default_fusion, "storage_mode": int(lib.mifx_storage_mode()), "texel_bytes": texel,
           "method": f"median of {args.blocks} blocks of about {args.window} s each after {args.warm} s of warm-up; sequence and fused blocks alternate"}
    # the device's own copy rate on a buffer of one target's size (read + write)
    big = torch.empty(w * h * 4 * 4, dtype=torch.float32, device=ctx.device)
    dst = torch.empty_like(big)
    us, = timed_us([(nothing, lambda: dst.copy_(big))])
    res["copy_TBps"] = 2 * big.numel() * 4 / us / 1e6
    del big, dst

    gen = torch.Generator(device=ctx.device).manual_seed(1)
    rnd = lambda *shape: torch.rand(*shape, generator=gen, device=ctx.device, dtype=torch.float32)  # noqa: E731
    cam = B.CameraAttribs()
    cam.f4ViewportSize[:] = [w, h, 1.0 / w, 1.0 / h]
    cam.fNearPlaneDepth, cam.fFarPlaneDepth = 0.0, 1.0
    slices = []
    for _ in range(max(SLICES)):
        base = rnd(h, w, 4)
        base[..., 3] = 0.05 + 0.9 * base[..., 3]
        slices.append(dict(depth=0.05 + 0.9 * rnd(h, w), base_color=base.to(dtype4), material=rnd(h, w, 4).to(dtype4), radiance=rnd(h, w, 4).to(dtype4),
                           specular_ibl=rnd(h, w, 4).to(dtype4)))
    targets = {k: rnd(h, w, 4).to(dtype4) for k in api.OIT_TARGETS}
    oit = api.OITResources(ctx, w, h, K)
    px = w * h
    t_struct, keep_t = oit._targets(targets)
    for n in SLICES:
        # the descriptors are made once: a call is the C entry alone (no Python work between the launches of the sequence)
        arr, keep = oit._slices(slices[:n])
        build = lambda: B.check(lib.mifx_oit_build_layers(oit.handle, arr, n, None, ctypes.byref(cam)))  # noqa: E731
        resolve = lambda: B.check(lib.mifx_oit_resolve(oit.handle, arr, n, None, ctypes.byref(cam), ctypes.byref(t_struct)))  # noqa: E731
        for what, call in (("build", build), ("resolve", resolve)):
            build()  # (the resolve reads real layers)
            us_seq, us_fused = timed_us([(lambda: lib.mifx_oit_set_fusion(0), call), (lambda: lib.mifx_oit_set_fusion(1), call)])
            for shape, us in (("sequence", us_seq), ("fused", us_fused)):
                key = f"{what}_l{n}_{shape}"
                res[key + "_us"], res[key + "_bytes_per_pixel"], res[key + "_TBps"] = us, bytes_per_pixel(shape, what, n, t=texel), px * bytes_per_pixel(shape, what, n, t=texel) / us / 1e6
            res[f"{what}_l{n}_speedup"] = us_seq / us_fused
            lib.mifx_oit_set_fusion(default_fusion)
    oit.close()
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
