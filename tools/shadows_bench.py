#!/usr/bin/env python3
"""Timing of the cascaded shadow maps (HIP events around repeated launches on the library's stream; at least 0.3 s of warm-up before every measurement, medians over
blocks of about 0.05 s, the blocks of an A/B pair alternating):
  * mifx_shadow_convert_to_filterable on a 2048 x 2048 x 4 array, VSM / EVSM2 / EVSM4 at iFixedFilterSize 2, 3 and 7 -- the fused kernel against the two launches
    through a scratch array in the same process (mifx_shadow_set_conversion_fusion), with the achieved bytes per second by the algorithmic bytes of the conversion
    (4 B read + 8 or 16 B written per texel) beside the device's own copy rate measured in the same run (BASELINE.md section 5 records 5.41 - 5.77 TB/s);
  * mifx_shadow_map_filter at 3840 x 2160 for PCF 3x3, the varying PCF, VSM and EVSM4, without and with filtering across cascades.
--filterable-bits 16: the filterable array in the reference's 16-bit formats (RG16_UNORM / RG16_FLOAT / RGBA16_FLOAT, bIs32BitEVSM = 0: 4 B read + 4 or 8 B
written per texel); 32 (the default): fp32.  Both work in both builds of the library (MIFX_STORAGE=h4 selects the native-storage one).

    python tools/shadows_bench.py --out profiles/shadows_bench.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

MAP, CASCADES = 2048, 4
W, H = 3840, 2160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=float, default=0.3, help="seconds of warm-up before every measurement")
    ap.add_argument("--window", type=float, default=0.05, help="seconds per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per variant (alternating)")
    ap.add_argument("--filterable-bits", type=int, choices=(16, 32), default=32, help="the filterable array's format: fp32, or the reference's 16-bit formats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bits = args.filterable_bits

    import torch

    import shadows_util as S
    from diligentfx_amd import api, binding as B

    def warm(fns):
        """Run the calls in turn for at least --warm seconds of wall time: the shader clock ramps over tenths of a second, a handful of launches measures the ramp"""
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warm:
            for fn in fns:
                for _ in range(8):
                    fn()
            torch.cuda.synchronize()

    def calibrate(fn):
        """launches per timed block, so that a block lasts about --window seconds"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(8):
            fn()
        b.record()
        torch.cuda.synchronize()
        return max(8, int(args.window / max(a.elapsed_time(b) / 8e3, 1e-7)))

    def timed_us(variants):
        """variants: [(setup, fn)].  Blocks of the variants ALTERNATE (A B A B ...) after one warm-up over all of them, so that clock and temperature drift hits them
        alike; returns the median block of each, in microseconds per launch."""
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
    res = {"device": torch.cuda.get_device_name(0), "map": [MAP, MAP, CASCADES], "frame": [W, H], "filterable_bits": bits, "storage_mode": int(lib.mifx_storage_mode()), "method": f"median of {args.blocks} blocks of about {args.window} s each after {args.warm} s of warm-up; fused and two-launch blocks alternate"}
    # the device's own copy rate on a buffer of the EVSM4 target's size (read + write)
    big = torch.empty(MAP * MAP * CASCADES * 4, dtype=torch.float32, device=ctx.device)
    dst = torch.empty_like(big)
    us, = timed_us([(nothing, lambda: dst.copy_(big))])
    res["copy_TBps"] = 2 * big.numel() * 4 / us / 1e6
    del big, dst

    slices = torch.from_numpy(S.shadow_slices(CASCADES, MAP, MAP)).to(ctx.device)
    src = B.shadow_map_array(slices)
    filterable = {}
    default_fusion = lib.mifx_shadow_set_conversion_fusion(1)
    lib.mifx_shadow_set_conversion_fusion(default_fusion)
    res["fusion_default"] = default_fusion
    for mode, name in ((S.MODE_VSM, "vsm"), (S.MODE_EVSM2, "evsm2"), (S.MODE_EVSM4, "evsm4")):
        ch = 4 if mode == S.MODE_EVSM4 else 2
        dtype = torch.float32 if bits == 32 else (torch.int16 if mode == S.MODE_VSM else torch.float16)
        out = torch.empty((CASCADES, MAP, MAP, ch), dtype=dtype, device=ctx.device)
        dstm = B.filterable_shadow_map(out)
        nbytes = MAP * MAP * CASCADES * (4 + (bits // 8) * ch)
        for fs in (2, 3, 7):
            A = S.make_attribs(CASCADES, MAP, MAP, iFixedFilterSize=fs, bIs32BitEVSM=int(bits == 32))
            call = lambda: B.check(lib.mifx_shadow_convert_to_filterable(ctx.handle, ctypes.byref(src), ctypes.byref(A), ctypes.c_uint32(mode), ctypes.byref(dstm)))  # noqa: E731
            us_fused, us_two = timed_us([(lambda: lib.mifx_shadow_set_conversion_fusion(1), call), (lambda: lib.mifx_shadow_set_conversion_fusion(0), call)])
            for key, us in ((f"convert_{name}_f{fs}_fused", us_fused), (f"convert_{name}_f{fs}_two_launch", us_two)):
                res[key + "_us"], res[key + "_TBps"] = us, nbytes / us / 1e6
            lib.mifx_shadow_set_conversion_fusion(default_fusion)
            if fs == 3:
                call()
                torch.cuda.synchronize()
                filterable[mode] = out.clone()
    cam = S.frame_camera(W, H)
    frame = torch.from_numpy(S.frame_depth(cam, W, H)).to(ctx.device)
    cam_s = S.camera_struct(cam)
    light = torch.empty_like(frame)
    casc = torch.empty((H, W, 2), dtype=torch.float32, device=ctx.device)
    d, o, c = B.image(frame), B.image(light), B.image(casc)
    fms = {m: B.filterable_shadow_map(t) for m, t in filterable.items()}
    for name, mode, over in (("pcf3", S.MODE_PCF, dict(iFixedFilterSize=3)), ("pcf_varying", S.MODE_PCF, dict(iFixedFilterSize=0, fFilterWorldSize=0.05)), ("vsm", S.MODE_VSM, dict()),
                             ("evsm4", S.MODE_EVSM4, dict())):
        A = S.make_attribs(CASCADES, MAP, MAP, bIs32BitEVSM=int(bits == 32), **over)
        for across in (0, 1):
            p = B.ShadowFilterParams(mode, across, 0, 0)
            call = lambda: B.check(lib.mifx_shadow_map_filter(ctx.handle, ctypes.byref(d), ctypes.byref(cam_s), ctypes.byref(A), ctypes.byref(p),  # noqa: E731
                                                                  ctypes.byref(src) if mode == S.MODE_PCF else None, ctypes.byref(fms[mode]) if mode != S.MODE_PCF else None,
                                                                  ctypes.byref(o), ctypes.byref(c)))
            res[f"filter_{name}{'_across' if across else ''}_us"], = timed_us([(nothing, call)])
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
