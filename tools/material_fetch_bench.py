#!/usr/bin/env python3
"""Timing of the material fetch (mifx_pbr_material_fetch) at 3840 x 2160 in one job: the five base maps (base colour, physical descriptor, normal, occlusion, emissive) and
all sixteen maps with every layer on, each from RGBA8_UNORM and from RGBA32_FLOAT 2048 x 2048 textures with full mip chains (one texture a slot), minified by about 2 texels
a pixel and magnified (0.25), with the atlas (regions of a quarter of the texture along each axis) and without.  Every configuration is set beside mifx_debug_stream_copy
moving the same number of bytes as the configuration's PLANES (the interpolants it reads and the planes it writes: the copy is given half that many bytes, it reads and
writes each) -- the texels the kernel gathers are on top of that and not in the yardstick.  HIP events around repeated calls of the C entry on the library's stream (argument
structures built once), at least 0.3 s of warm-up before every pair, medians over alternating blocks of about 0.05 s (fetch, copy, fetch, copy ...).

    python tools/material_fetch_bench.py --out profiles/material_fetch_bench.json"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
W, H, TEX = 3840, 2160, 2048
BASE_SLOTS = (0, 1, 2, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=float, default=0.3, help="seconds of warm-up before every measurement")
    ap.add_argument("--window", type=float, default=0.05, help="seconds per timed block")
    ap.add_argument("--blocks", type=int, default=7, help="timed blocks per variant (alternating)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import grid_util as G
    from diligentfx_amd import api, binding as B

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
    ctx.sync_stream()
    dev = ctx.device
    gen = torch.Generator(device=dev).manual_seed(11)
    levels = TEX.bit_length()
    texels = sum(max(1, TEX >> k) ** 2 for k in range(levels))

    def texture_table(rgba8):
        data, structs = [], []
        for _ in range(B.PBR_TEXTURE_COUNT):
            t = (torch.randint(0, 256, (1, texels, 4), device=dev, dtype=torch.uint8, generator=gen) if rgba8
                 else torch.rand((1, texels, 4), device=dev, generator=gen))
            if not rgba8:
                t[..., 2] = 0.8 + 0.2 * t[..., 2]  # (a normal map's z stays above 0)
            data.append(t)
            structs.append(B.TextureArray(t.data_ptr(), TEX, TEX, 1, levels, B.NATIVE_FORMATS["RGBA8_UNORM" if rgba8 else "RGBA32_FLOAT"], 0, t.stride(0) * t.element_size()))
        return data, (B.TextureArray * len(structs))(*structs)

    tables = {False: texture_table(False), True: texture_table(True)}
    cam = B.camera_from_bytes(G.make_camera(W, H, eye=(0.3, 1.2, -4.0), at=(0.0, 0.0, 0.0)).tobytes())
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32) + 0.5, torch.arange(W, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
    z = 3.2 + 0.0004 * x + 0.0007 * y + 0.15 * torch.sin(0.0021 * x) * torch.cos(0.0017 * y)
    P = [float(v) for v in cam.mProj]
    depth = ((P[10] * z + P[14]) / (P[11] * z + P[15])).contiguous()
    depth[H // 3: H // 3 + 200, W // 4: W // 4 + 600] = 1.0  # some background
    nrm = torch.nn.functional.normalize(torch.stack([0.3 * torch.sin(0.0013 * x), 0.25 * torch.cos(0.0011 * y), -torch.ones_like(x)], -1), dim=-1)
    mesh_normal = torch.cat([nrm, torch.zeros(H, W, 1, device=dev)], -1).contiguous()
    uvs = {"minified_2_texels": 2.0 / TEX, "magnified_0.25_texels": 0.25 / TEX}
    uv = {k: torch.stack([d * (0.98 * x - 0.17 * y) + 0.37, d * (0.17 * x + 0.98 * y) + 0.21], -1).contiguous() for k, d in uvs.items()}
    # (in the atlas a region is a quarter of the texture along each axis: the same texel step a pixel needs four times the coordinate step)
    uv_atlas = {k: (v * 4.0).contiguous() for k, v in uv.items()}
    out4 = {n: torch.zeros(H, W, 4, device=dev) for n in ("base_color", "normal", "material", "emissive", "clearcoat", "clearcoat_normal", "sheen", "anisotropy", "iridescence")}
    out1 = {n: torch.zeros(H, W, device=dev) for n in ("occlusion", "transmission")}
    imgs = {k: B.image(v) for k, v in {**out4, **out1, "depth": depth, "mesh_normal": mesh_normal}.items()}
    p = lambda k: ctypes.pointer(imgs[k])  # noqa: E731
    gs = B.GBuffer(p("base_color"), p("normal"), p("material"), None, p("emissive"), p("occlusion"))
    ls = B.PBRLayers(0, 0.0, 0.0, 0, *[p(k) if k in imgs else None for k in B.PBR_LAYER_PLANES])
    src, dst = torch.empty(W * H * 96, device=dev, dtype=torch.uint8), torch.empty(W * H * 96, device=dev, dtype=torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "frame": [W, H], "textures": f"{TEX}x{TEX}, {levels} levels, one texture a slot",
           "method": f"median of {args.blocks} blocks of about {args.window} s each after {args.warm} s of warm-up; fetch and copy blocks alternate; the copy moves the bytes of "
                     "the planes the configuration reads and writes (texels not counted); with PHYS_DESC present METALLIC and ROUGHNESS are not read: 'sixteen maps' are 14 fetches",
           "configurations": {}}
    keep = []
    for maps, slots, layer_flags in (("five_base_maps", BASE_SLOTS, 0), ("sixteen_maps", tuple(range(B.PBR_TEXTURE_COUNT)), 31)):
        read_bytes = 4 + 8 + 16                                   # depth, uv0, mesh normal
        write_bytes = 16 * 4 + 4 + (16 * 5 + 4 if layer_flags else 0)
        copy_bytes = (read_bytes + write_bytes) * W * H // 2
        assert copy_bytes <= src.numel()
        copy = lambda n=copy_bytes: B.check(ctx.lib.mifx_debug_stream_copy(ctx.handle, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), ctypes.c_uint64(n)))  # noqa: E731
        for rgba8 in (True, False):
            for uv_name, uv_plane in uv.items():
                for atlas in (False, True):
                    region = (0.25, 0.25, 0.25, 0.5) if atlas else (1.0, 1.0, 0.0, 0.0)
                    m = api.Material(textures={s: (s, B.PBRTextureAttribs.make(atlas=region)) for s in slots})
                    uvi = B.image(uv_atlas[uv_name] if atlas else uv_plane)
                    keep.append(uvi)
                    ip = B.MaterialInterpolants(p("depth"), ctypes.pointer(uvi), None, p("mesh_normal"), None, None, None)
                    mats = (B.PBRMaterial * 1)(m)
                    desc = B.MaterialFetchDesc(mats, tables[rgba8][1], 1, B.PBR_TEXTURE_COUNT, layer_flags, B.MATERIAL_FETCH_FLAG_TEXTURE_ATLAS if atlas else 0, 0.0,
                                               (ctypes.c_uint32 * 3)(0, 0, 0))
                    keep += [ip, mats, desc]
                    fetch = lambda ip=ip, desc=desc: B.check(ctx.lib.mifx_pbr_material_fetch(ctx.handle, ctypes.byref(ip), ctypes.byref(desc), ctypes.byref(cam),  # noqa: E731
                                                                                              ctypes.byref(gs), ctypes.byref(ls)))
                    fetch_us, copy_us = timed_us([fetch, copy])
                    name = f"{maps}/{'rgba8' if rgba8 else 'rgba32f'}/{uv_name}/{'atlas' if atlas else 'no_atlas'}"
                    res["configurations"][name] = {"fetch_us": fetch_us, "stream_copy_us": copy_us, "ratio": fetch_us / copy_us, "plane_bytes_per_pixel": read_bytes + write_bytes,
                                                   "fetch_plane_gb_per_s": (read_bytes + write_bytes) * W * H / fetch_us / 1e3}
                    print(name, res["configurations"][name], flush=True)
    ctx.close()
    line = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
