#!/usr/bin/env python3
"""Times the stand-alone TemporalAntiAliasing kernel at 3840x2160 on an all-zero motion plane: the static camera, where the history skip (csrc/taa.hip) finds nothing
to skip and must not cost anything.  --motion frame keeps the synthetic frame's own motion instead.  Prints one JSON line: the median and the range of the launches'
durations (events on the effect's stream) after --warm-s seconds of device work.  MIFX_LIB_PATH selects another build of the library for an A/B run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--width", type=int, default=3840)
    p.add_argument("--height", type=int, default=2160)
    p.add_argument("--flags", type=int, default=2, help="TAA feature flags (2 = BICUBIC_FILTER, the chain's default)")
    p.add_argument("--launches", type=int, default=40)
    p.add_argument("--warm-s", type=float, default=0.3)
    p.add_argument("--motion", default="zero", choices=("zero", "frame"))
    p.add_argument("--history-skip", type=int, default=None, help="mifx_debug_taa_set_history_skip (default: as the object is created)")
    a = p.parse_args()
    import torch

    from diligentfx_amd import api, binding as B, synth

    ctx = api.PostFXContext(0)
    taa = api.TemporalAntiAliasing(ctx)
    if a.history_skip is not None:
        taa.set_history_skip(bool(a.history_skip))
    w, h = a.width, a.height
    f = synth.make_frame(synth.Scene(), 16, w, h, ctx.device)
    color = B.to_storage(torch.cat([f["base_color"][..., :3] * 2.0, f["base_color"][..., 3:4]], -1).contiguous())
    attribs = B.TAAAttribs.default()
    frame, times = 0, []

    def step(timed):
        nonlocal frame
        ctx.prepare_resources(frame, w, h)
        taa.prepare_resources(a.flags)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        if a.motion == "zero":
            ctx.get_closest_motion_vectors().zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        taa.execute(color, attribs)
        e1.record()
        if timed:
            times.append((e0, e1))
        frame += 1

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.warm_s or frame < 3:
        step(False)
        torch.cuda.synchronize()
    for _ in range(a.launches):
        step(True)
    torch.cuda.synchronize()
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in times]
    print(json.dumps({"tool": "taa_static_camera_timing", "lib": os.path.basename(os.path.dirname(B.LIB_PATH)) + "/" + os.path.basename(B.LIB_PATH), "width": w, "height": h,
                      "flags": a.flags, "motion": a.motion, "launches": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                      "max_us": round(max(us), 2)}))
    taa.close()
    ctx.close()


if __name__ == "__main__":
    main()
