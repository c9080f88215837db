"""Run in its own process with MIFX_STORAGE=h4 (tests/test_gpu_storage_h4.py does): the native-storage build of the library (libmifx_h4.so: the reference's own target
formats -- RGBA16_FLOAT colour planes, R8_UNORM ambient occlusion and roughness, R16_FLOAT variance / resolved depth / history length, RG16_FLOAT closest motion,
R11G11B10_FLOAT Bloom) against the checker with format emulation -- every image a reference pass writes goes through the rounding of its target format when it is stored
(oracle/pyref.py QuantizingLib), the inputs are the binary16 values the HIP side is given.  Prints what it measured; exits non-zero on the first violated bound."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import chain_util  # noqa: E402
import cpu_chain  # noqa: E402
import pyref  # noqa: E402
from diligentfx_amd import api, binding as B, synth  # noqa: E402
from util import assert_close, blue_noise_tables, to_np  # noqa: E402

MEASURE = bool(os.environ.get("MIFX_PARITY_MEASURE"))
# binary16 has 11 significant bits: one rounding step is 4.9e-4 relative, two values that agree to 1e-3 before the store can land two steps apart after it
RTOL = 2.5e-3
# R8_UNORM: values that agree to 1e-3 before the store can land one code apart (1 / 255)
AO_STEP = 1.02 / 255.0
# R11G11B10_FLOAT (Bloom levels and output, hence the final image): 6 / 6 / 5 mantissa bits -- one rounding step is 1.6 % (red, green) or 3.1 % (blue) of the value
RTOL_BLOOM = 3.3e-2


def q16(a):
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(np.float32)


def f32(t):
    return to_np(t.float())


def bloom_rgba(t):
    """Bloom's output plane of the native-storage build: packed R11G11B10_FLOAT texels (torch.int32 view) -> float32 (H, W, 4); the format has no alpha: reads as 1."""
    assert t.dtype == torch.int32, t.dtype
    rgb = to_np(api.widen(t))
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), np.float32)], axis=-1)


def setup():
    lib = B.load()
    assert lib.mifx_storage_mode() == 1 and B.storage_dtype() == torch.float16, "not the RGBA16_FLOAT storage build"
    plain = pyref.ref_lib() or pyref.oracle_lib()
    pfx = "ref_" if pyref.ref_lib() is not None else "oracle_"
    quant = pyref.QuantizingLib(plain)
    w, h = 224, 128
    sobol, tile = blue_noise_tables()
    chain = api.Chain(0, sobol, tile)
    dev = chain.device
    ibl_np = chain_util.make_ibl(plain, pfx)  # cube maps and the LUT stay fp32 in both builds
    ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]).to(dev), [torch.from_numpy(m).to(dev) for m in ibl_np["irradiance"]], [torch.from_numpy(m).to(dev) for m in ibl_np["prefiltered"]])
    cpu = cpu_chain.CpuChain(quant, pfx)
    sa = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    scene = synth.Scene()
    out = torch.zeros(h, w, 4, device=dev, dtype=torch.float16)
    return dict(lib=lib, plain=plain, pfx=pfx, quant=quant, w=w, h=h, sobol=sobol, tile=tile, chain=chain, dev=dev, ibl_np=ibl_np, ibl=ibl, cpu=cpu, sa=sa, scene=scene, out=out)


# outlier budgets of the chain at 224 x 128: round 2 measured radiance 6e-5, SSR 5.8e-3, TAA 3.2e-4, 2.3e-3 of the Bloom / final values not on the same code
# (profiles/r02_h4_parity.txt) with the contracting build; the build without contraction (round 4) has 0 everywhere over these six frames except <= 1.8e-5 of the values not on
# the same R11G11B10 code (profiles/r04_h4_parity.txt) -- the budgets below are a small multiple of that; MIFX_PARITY_MEASURE=1 reports without deciding
CHAIN_BUDGET = {"radiance": 5e-5, "ssr": 1e-3, "ssao": 2e-4, "taa": 1e-4, "bloom": 1e-4, "final": 1e-4}
CHAIN_BUDGET_EXACT = {"bloom": 5e-4, "final": 5e-4}  # values that did not land on the same R11G11B10 code


def as_count(fraction, n):
    """The budget `fraction` of `n` compared values as a whole number of values, rounded down, handed to assert_close as the fraction it compares with (half a value above
    the count: the comparison is between whole numbers of values either way)."""
    return (np.floor(fraction * n) + 0.5) / max(n, 1)


def chain_frames(S, chain, cpu, out, size, frames, counted=False, label="chain", after_frame=None, same_code=None):
    """`frames` frames of the chain at `size` against the checker with RGBA16_FLOAT stores: radiance, SSR, SSAO, TAA, Bloom and the final image of every frame, Bloom and the
    final image also on the same R11G11B10 code.  counted: the budgets are whole numbers of values (as_count: on a small frame a fraction of the values is less than one
    value, i.e. none), not fractions.  same_code: this frame size's own fraction for the two "same code" comparisons (the caller says why).  after_frame(frame, checker's
    planes): further checks on the frame the chain has just produced.  Returns the last frame's checker planes."""
    ibl_np, ibl, sa, scene, dev = (S[k] for k in ("ibl_np", "ibl", "sa", "scene", "dev"))
    w, h = size
    exact = CHAIN_BUDGET_EXACT if same_code is None else dict.fromkeys(CHAIN_BUDGET_EXACT, same_code)

    def allow(table, name, n):
        return 1.0 if MEASURE else (as_count(table[name], n) if counted else table[name])

    keep = {}
    for frame in range(frames):
        f = synth.make_frame(scene, frame, w, h, dev)
        chain.execute(chain.bind_frame(frame, f, ibl, sa, out))
        g = {k: to_np(v) for k, v in f.items() if isinstance(v, torch.Tensor)}
        for k in ("base_color", "normal", "material"):
            g[k] = q16(g[k])  # the checker reads the binary16 values the HIP side was given
        keep = {}
        want = chain_util.run_frame_inputs(cpu, g, bytes(f["camera"]), bytes(f["prev_camera"]), frame, ibl_np, sa, keep)
        got = f32(out)
        assert np.isfinite(got).all() and out.dtype == torch.float16
        res = {}
        n4, n1 = got.size, got.size // 4
        _, res["radiance"] = assert_close(f32(chain.shard_plane_image("radiance")), keep["radiance"], rtol=RTOL, max_outlier_frac=allow(CHAIN_BUDGET, "radiance", n4), what=f"radiance frame {frame}")
        _, res["ssr"] = assert_close(f32(chain.effect_output("ssr")), keep["ssr_out"], rtol=RTOL, max_outlier_frac=allow(CHAIN_BUDGET, "ssr", n4), what=f"SSR frame {frame}")
        _, res["ssao"] = assert_close(to_np(api.widen(chain.effect_output("ssao"))), keep["ssao_out"], max_outlier_frac=allow(CHAIN_BUDGET, "ssao", n1), abs_slack=AO_STEP, what=f"SSAO frame {frame}")
        _, res["taa"] = assert_close(f32(chain.effect_output("taa")), keep["taa_out"], rtol=RTOL, max_outlier_frac=allow(CHAIN_BUDGET, "taa", n4), what=f"TAA frame {frame}")
        # Bloom's levels and output are R11G11B10_FLOAT: the bound is one rounding step of the format; how many values landed on the very same code is reported beside it
        _, res["bloom"] = assert_close(bloom_rgba(chain.effect_output("bloom")), keep["bloom_out"], rtol=RTOL_BLOOM, max_outlier_frac=allow(CHAIN_BUDGET, "bloom", n4), what=f"Bloom frame {frame}")
        _, res["final"] = assert_close(got, want, rtol=RTOL_BLOOM, max_outlier_frac=allow(CHAIN_BUDGET, "final", n4), what=f"final image frame {frame}")
        _, res["bloom_same_code"] = assert_close(bloom_rgba(chain.effect_output("bloom")), keep["bloom_out"], rtol=RTOL, max_outlier_frac=allow(exact, "bloom", n4), what=f"Bloom frame {frame} (same code)")
        _, res["final_same_code"] = assert_close(got, want, rtol=RTOL, max_outlier_frac=allow(exact, "final", n4), what=f"final image frame {frame} (same code)")
        assert np.abs(got[..., :3] - want[..., :3]).mean() < 2e-3
        print(f"h4 {label} frame {frame}: outlier fractions " + " ".join(f"{k} {v:.2e}" for k, v in res.items()), flush=True)
        if after_frame is not None:
            after_frame(frame, keep)
    return keep


def packed_equals_half(postfx, packed, values):
    """The auto exposure and the tone map on a packed R11G11B10_FLOAT plane and on an RGBA16_FLOAT copy of its values (`values`: what the plane holds, float32 (H, W, 4),
    alpha 1): the same average, the same low-resolution luminance and the same frame, bit for bit -- the packed load is the only difference."""
    dev = packed.device
    as_half = torch.from_numpy(values).to(dev).half()  # (R11G11B10 values are exact in binary16)
    assert packed.dtype == torch.int32 and np.array_equal(f32(as_half), values)
    ae_p, ae_h = api.AutoExposure(postfx), api.AutoExposure(postfx)
    tm = B.ToneMappingAttribs.default(4)
    ldr_p, ldr_h, tm_p, tm_h = (torch.zeros_like(as_half) for _ in range(4))
    for ae, img, ldr, plain in ((ae_p, packed, ldr_p, tm_p), (ae_h, as_half, ldr_h, tm_h)):
        ae.reset(0.1)
        ae.execute(img, 0.5)
        ae.tone_map(img, tm, 1, out=ldr)
        postfx.tone_map(img, tm, 0.3, 1, out=plain)  # (mifx_tonemap_execute with the host's average)
    torch.cuda.synchronize()
    assert ae_p.average() == ae_h.average() and torch.equal(ldr_p, ldr_h), (ae_p.average(), ae_h.average())
    assert torch.equal(ae_p.plane("low_res_luminance"), ae_h.plane("low_res_luminance"))
    assert torch.equal(tm_p, tm_h), f"tone map on a packed plane vs on its values in RGBA16_FLOAT: {int((tm_p != tm_h).sum())} values differ"
    ae_p.close()
    ae_h.close()


def section_chain(S):
    lib, pfx, quant, w, h, chain, dev, ibl_np, ibl, cpu, sa, scene, out = (S[k] for k in ("lib", "pfx", "quant", "w", "h", "chain", "dev", "ibl_np", "ibl", "cpu", "sa", "scene", "out"))
    # 1. a 4-channel float32 image is refused, loudly
    f = synth.make_frame(scene, 0, w, h, dev)
    i32, o16 = B.image(f["base_color"]), B.image(out)
    import ctypes

    tm = B.ToneMappingAttribs.default(4)
    st = lib.mifx_tonemap_execute(chain.postfx.handle, ctypes.byref(i32), ctypes.byref(o16), ctypes.byref(tm), ctypes.c_float(0.3), ctypes.c_uint32(1))
    assert st == -1 and b"F16X4" in lib.mifx_last_error(), (st, lib.mifx_last_error())

    # 2. the chain, frame by frame, against the checker with RGBA16_FLOAT stores (chain_frames above: the budgets are fractions of the compared values here)
    chain_frames(S, chain, cpu, out, (w, h), 6)
    assert chain.effect_output("ssr").dtype == torch.float16 and chain.effect_output("ssao").dtype == torch.uint8 and chain.effect_output("bloom").dtype == torch.int32
    # the Bloom output is an R11G11B10_FLOAT plane (4 bytes per texel, Bloom.cpp:137); alpha reads as 1
    bo = bloom_rgba(chain.effect_output("bloom"))
    assert np.array_equal(pyref.store_r11g11b10(bo, alpha_reads_as=1.0), bo)
    # ... and the tone map takes it as it is: the stand-alone pass on the plane equals the tone map fused into Bloom's last pass
    import ctypes as C

    unfused = torch.zeros(h, w, 4, device=dev, dtype=torch.float16)
    bdesc, odesc = B.image(chain.effect_output("bloom")), B.image(unfused)
    f5 = synth.make_frame(scene, 5, w, h, dev)
    bound = chain.bind_frame(5, f5, ibl, sa, out)
    B.check(lib.mifx_tonemap_execute(chain.postfx.handle, C.byref(bdesc), C.byref(odesc), bound[0].tone_mapping, C.c_float(bound[0].ave_log_lum), C.c_uint32(bound[0].tonemap_flags)))
    torch.cuda.synchronize()
    assert torch.equal(unfused, out), f"tone map on the packed Bloom output vs the fused pass: {int((unfused != out).sum())} values differ"
    # ... and so does the auto exposure: the packed plane and an RGBA16_FLOAT copy of its values give the same average and the same tone-mapped frame
    packed_equals_half(chain.postfx, chain.effect_output("bloom"), bo)
    ao, hl, idx_ao = chain.effect("ssao").export_history()
    assert ao.dtype == torch.uint8 and hl.dtype == torch.float16
    chain.effect("ssao").import_history(ao, hl, idx_ao)
    # 3. a stored value is exactly representable: storing it again does not change it
    assert torch.equal(out, out.float().half())
    # 4. history export / import carry the binary16 planes
    col, idx = chain.effect("taa").export_history()
    assert col.dtype == torch.float16 and idx == 5
    chain.effect("taa").import_history(col, idx)


def section_fusion(S):
    w, h, sobol, tile, dev, ibl, sa, scene = (S[k] for k in ("w", "h", "sobol", "tile", "dev", "ibl", "sa", "scene"))
    # 4b. every fusion switch of the chain gives the same bits in this build too (the narrow stores round identically in every translation unit)
    fused, plain = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    plain.set_fusion_mask(0)
    oa, ob = torch.zeros(h, w, 4, device=dev, dtype=torch.float16), torch.zeros(h, w, 4, device=dev, dtype=torch.float16)
    for frame in range(4):
        f = synth.make_frame(scene, frame, w, h, dev)
        fused.execute(fused.bind_frame(frame, f, ibl, sa, oa))
        plain.execute(plain.bind_frame(frame, f, ibl, sa, ob))
        assert torch.equal(oa, ob), f"h4 fusion on / off: frame {frame}: {int((oa != ob).sum())} values differ"
        for name in ("roughness", "mask", "hist_radiance"):
            assert torch.equal(fused.effect("ssr").get_intermediate(name), plain.effect("ssr").get_intermediate(name)), name
        assert torch.equal(fused.effect_output("ssao"), plain.effect_output("ssao"))
    fused.close()
    plain.close()
    print("h4 fusion on / off: 4 frames bit-identical", flush=True)


def section_dof(S):
    pfx, quant, sobol, tile, dev, scene = (S[k] for k in ("pfx", "quant", "sobol", "tile", "dev", "scene"))
    # 5. depth of field (its eleven passes store five 4-channel targets) end to end against the format-emulating checker
    import test_gpu_dof as D

    ctx = api.PostFXContext(0, sobol, tile)
    dof = api.DepthOfField(ctx)
    attribs = B.DOFAttribs.default()
    attribs.MaxCircleOfConfusion, attribs.AlphaInterpolation = 0.02, 0.9
    e2e = cpu_chain.CpuChain(quant, pfx)
    w2, h2 = 256, 144
    for frame in (7, 8):
        f = synth.make_frame(scene, frame, w2, h2, dev)
        cam = D.lens_camera(f["camera"])
        color = D.hdr_colour(f, dev)
        ctx.prepare_resources(frame, w2, h2)
        dof.prepare_resources(1)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], cam, f["prev_camera"])
        dof.execute(B.to_storage(color), f["depth"], attribs)
        pf = {"frame": frame, "cam": bytes(cam), "closest_motion": f32(ctx.get_closest_motion_vectors())}
        want = e2e.dof(pf, q16(to_np(color)), to_np(f["depth"]), attribs, 1)
        got = bloom_rgba(dof.get_depth_of_field_texture())  # (an R11G11B10_FLOAT target, DepthOfField.cpp:281-289: a 4-byte plane since round 5)
        _, frac = assert_close(got, want, rtol=RTOL, max_outlier_frac=1.0 if MEASURE else 2e-4, what=f"depth of field frame {frame}")  # measured <= 2.7e-5 (profiles/r04_h4_parity.txt)
        print(f"h4 depth of field frame {frame}: outlier fraction {frac:.2e}", flush=True)
        assert dof.get_depth_of_field_texture().dtype == torch.int32
    dof.close()
    ctx.close()


def section_dof_chain(S):
    """Depth of field between TAA and Bloom in the native-storage build: its output is a 4-byte R11G11B10_FLOAT plane (round 5) that Bloom's prefilter and final pass read
    as such.  (a) the chain with depth of field against a second chain + stand-alone DOF + stand-alone Bloom on the packed plane (tests/test_gpu_dof.py: the chain's fused
    final pass and the stand-alone passes take the packed source); (b) Bloom on the packed plane == Bloom on an RGBA16_FLOAT plane holding the same values (every R11G11B10
    value is a binary16 value): the packed load is the only difference, the pyramid and the output are equal code for code."""
    sobol, tile, dev, scene, ibl, sa = (S[k] for k in ("sobol", "tile", "dev", "scene", "ibl", "sa"))
    import test_gpu_dof as D

    W, H = 320, 192
    a, b = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    da = B.DOFAttribs.default()
    da.MaxCircleOfConfusion = 0.02
    flags = api.DepthOfField.FEATURE_FLAG_ENABLE_TEMPORAL_SMOOTHING
    a.set_depth_of_field(da, flags)
    out_a, out_b = (torch.zeros(H, W, 4, device=dev, dtype=torch.float16) for _ in range(2))
    standalone = api.DepthOfField(b.postfx)
    for fi in range(3, 6):
        g = synth.make_frame(scene, fi, W, H, dev)
        D.lens_camera(g["camera"])
        a.execute(a.bind_frame(fi, g, ibl, sa, out_a))
        b.execute(b.bind_frame(fi, g, ibl, sa, out_b))
        torch.cuda.synchronize()
        taa_b = b.effect_output("taa")
        assert torch.equal(a.effect_output("taa"), taa_b)
        standalone.prepare_resources(flags)
        standalone.execute(taa_b, g["depth"], da)
        assert standalone.get_depth_of_field_texture().dtype == torch.int32 and torch.equal(standalone.get_depth_of_field_texture(), a.effect_output("dof"))
        bl = api.Bloom(b.postfx)
        bl.prepare_resources()
        bl.execute(standalone.get_depth_of_field_texture(), b.bloom_attribs)  # (the prefilter and the final up-sample on the packed plane)
        assert torch.equal(bl.get_bloom_texture(), a.effect_output("bloom"))  # (the chain's: produced on demand from the packed plane it kept)
        ldr = b.postfx.tone_map(bl.get_bloom_texture(), b.tone_mapping, b.ave_log_lum, b.tonemap_flags, out=torch.zeros_like(out_a))
        assert torch.equal(ldr, out_a), f"frame {fi}: the chain's fused final pass on the packed depth-of-field output differs from Bloom + ToneMap() on it"
        bl.close()
        assert not torch.equal(out_a, out_b)
    standalone.close()
    a.close()
    b.close()
    ctx = api.PostFXContext(0, sobol, tile)
    dof, bloom = api.DepthOfField(ctx), api.Bloom(ctx)
    attribs = B.DOFAttribs.default()
    attribs.MaxCircleOfConfusion = 0.02
    ba = B.BloomAttribs.default()
    w2, h2 = 320, 192
    for frame in (7, 8):
        f = synth.make_frame(scene, frame, w2, h2, dev)
        cam = D.lens_camera(f["camera"])
        ctx.prepare_resources(frame, w2, h2)
        dof.prepare_resources(1)
        bloom.prepare_resources()
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], cam, f["prev_camera"])
        dof.execute(B.to_storage(D.hdr_colour(f, dev)), f["depth"], attribs)
        packed = dof.get_depth_of_field_texture()
        assert packed.dtype == torch.int32
        bloom.execute(packed, ba)
        torch.cuda.synchronize()
        from_packed = {"out": bloom.get_bloom_texture().clone(), "down0": bloom.get_intermediate("down0").clone(), "up0": bloom.get_intermediate("up0").clone()}
        unpacked = B.to_storage(torch.from_numpy(bloom_rgba(packed)).to(dev))
        assert unpacked.dtype == torch.float16 and np.array_equal(to_np(unpacked.float())[..., :3], bloom_rgba(packed)[..., :3]), "an R11G11B10 value is a binary16 value"
        bloom.execute(unpacked, ba)
        torch.cuda.synchronize()
        assert torch.equal(bloom.get_intermediate("down0"), from_packed["down0"]) and torch.equal(bloom.get_intermediate("up0"), from_packed["up0"]), frame
        assert torch.equal(bloom.get_bloom_texture(), from_packed["out"]), f"frame {frame}: Bloom on the packed depth-of-field output differs from Bloom on the same values in RGBA16_FLOAT"
    print("h4 depth of field -> Bloom: the chain equals the stand-alone effects on the packed plane; packed and RGBA16_FLOAT sources give the same pyramid and output", flush=True)
    bloom.close()
    dof.close()
    ctx.close()


def section_dof_passes(S):
    """Depth of field pass by pass in the reference's target formats: the circle of confusion and its history R16_FLOAT, the separated / dilated / blurred one
    R16_UNORM, the colour targets RGBA16_FLOAT, the combined output R11G11B10_FLOAT values with alpha 1.  Every pass of the HIP side runs on the HIP side's own previous
    planes; the checker's pass runs on the same (widened) planes and stores through QuantizingLib."""
    import test_gpu_dof as D

    pfx, quant, plain, sobol, tile, dev, scene = (S[k] for k in ("pfx", "quant", "plain", "sobol", "tile", "dev", "scene"))
    ctx = api.PostFXContext(0, sobol, tile)
    dof = api.DepthOfField(ctx)
    U16 = 1.02 / 65535.0
    tables = cpu_chain.CpuChain(plain, pfx)
    for (w, h), flags, rings in (((256, 144), 3, (5, 7)), ((202, 118), 1, (3, 4)), ((100, 60), 0, (4, 6))):
        attribs = B.DOFAttribs.default()
        attribs.MaxCircleOfConfusion, attribs.AlphaInterpolation = 0.02, 0.9
        attribs.BokehKernelRingCount, attribs.BokehKernelRingDensity = rings
        temporal = bool(flags & 1)
        prev_temporal = np.zeros((h, w), np.float32)
        large, small, gauss = tables.dof_tables(*rings)
        worst = {}
        for frame in (7, 8, 9):
            f = synth.make_frame(scene, frame, w, h, dev)
            cam = D.lens_camera(f["camera"])
            color = B.to_storage(D.hdr_colour(f, dev))
            ctx.prepare_resources(frame, w, h)
            dof.prepare_resources(flags)
            ctx.execute(f["depth"], f["prev_depth"], f["motion"], cam, f["prev_camera"])
            motion = f32(ctx.get_closest_motion_vectors())
            names = ["coc", "dilation1", "dilation2", "dilation3", "dilation_blurred", "prefiltered0", "prefiltered1", "bokeh0", "bokeh1"] + (["coc_temporal"] if temporal else [])

            def read():
                return {n: to_np(api.widen(dof.get_intermediate(n))).copy() for n in names}

            dof.debug_set_last_pass(7)
            dof.execute(color, f["depth"], attribs)
            first = read()
            dof.debug_set_last_pass(0)
            dof.execute(color, f["depth"], attribs)
            torch.cuda.synchronize()
            second = read()
            got = bloom_rgba(dof.get_depth_of_field_texture())
            assert dof.get_depth_of_field_texture().dtype == torch.int32 and dof.get_intermediate("coc").dtype == torch.float16 and dof.get_intermediate("dilation3").dtype == torch.int16 and dof.get_intermediate("bokeh0").dtype == torch.float16
            cnp, dnp = f32(color), to_np(f["depth"])
            P = D.Passes(quant, pfx, bytes(cam), attribs, flags)

            def cmp(name, a, b, rtol=RTOL, slack=None, frac=0.0):
                worst[name] = max(worst.get(name, 0.0), assert_close(a, b, rtol=rtol, abs_slack=slack, max_outlier_frac=1.0 if MEASURE else frac, what=f"h4 DOF {name} frame {frame} {w}x{h}")[1])

            cmp("coc", first["coc"], P.coc(dnp))
            used = first["coc"]
            if temporal:
                cmp("coc_temporal", first["coc_temporal"], P.temporal(first["coc"], prev_temporal, motion))
                used = prev_temporal = first["coc_temporal"]
            lvl = P.separated(used)
            for k in (1, 2, 3):
                assert np.array_equal(first[f"dilation{k}"], P.dilation(lvl)), f"dilation{k}: a maximum of R16_UNORM values is bit-exact"
                lvl = first[f"dilation{k}"]
            cmp("dilation_blurred", first["dilation_blurred"], P.blur(first["dilation3"], gauss), slack=2.0 * U16)  # two stores: the horizontal pass and the vertical one
            n6, f6 = P.prefilter(cnp, used, first["dilation_blurred"])
            cmp("prefiltered near", first["prefiltered0"], n6)
            cmp("prefiltered far", first["prefiltered1"], f6)
            n7, f7 = P.bokeh_first(first["prefiltered0"], first["prefiltered1"], large, cnp)
            cmp("bokeh gather near", first["bokeh0"], n7)
            cmp("bokeh gather far", first["bokeh1"], f7, frac=2e-3)  # "a >= CoCFar" on interpolated binary16 alphas: a tap that ties up to rounding may flip
            n8, f8 = P.bokeh_second(first["bokeh0"], first["bokeh1"], small)
            cmp("bokeh fill near", second["prefiltered0"], n8)
            cmp("bokeh fill far", second["prefiltered1"], f8, frac=2e-3)
            n9, f9 = P.postfilter(second["prefiltered0"], second["prefiltered1"])
            cmp("postfilter near", second["bokeh0"], n9)
            cmp("postfilter far", second["bokeh1"], f9)
            want = P.combine(cnp, used, second["bokeh0"], second["bokeh1"])
            cmp("combined", got, want, rtol=RTOL_BLOOM)
            cmp("combined (same code)", got, want, frac=6e-3)
            assert np.array_equal(pyref.store_r11g11b10(got, alpha_reads_as=1.0), got), "the combined output holds R11G11B10 values, alpha 1"
        print(f"h4 DOF passes {w}x{h} flags {flags}: outlier fractions " + " ".join(f"{k} {v:.1e}" for k, v in worst.items() if v > 0.0) + " (others 0)", flush=True)
    dof.close()
    ctx.close()


def section_half_precision_depth(S):
    """FEATURE_FLAG_HALF_PRECISION_DEPTH of PostFXContext and ScreenSpaceAmbientOcclusion: the reference makes the reprojected / previous depth and SSAO's two
    depth pyramids R16_UNORM targets; the native-storage build gives those planes the values such targets keep.  PostFX decides the format when it creates the planes, i.e. on
    a change of the frame size, not of the flag (PostFXContext.cpp:246-247) -- the second step below checks that too."""
    pfx, plain, sobol, tile, dev, scene = (S[k] for k in ("pfx", "plain", "sobol", "tile", "dev", "scene"))
    quant = pyref.QuantizingLib(plain)
    ctx = api.PostFXContext(0, sobol, tile)
    ssao, taa = api.ScreenSpaceAmbientOcclusion(ctx), api.TemporalAntiAliasing(ctx)
    cpu = cpu_chain.CpuChain(quant, pfx, taa_flags=2)
    U16 = 1.02 / 65535.0
    # (frame, width, height, PostFX flags, planes hold R16_UNORM values?, SSAO flags)
    steps = [(0, 224, 128, 0, False, 0), (1, 224, 128, 2, False, 1), (2, 224, 128, 2, False, 1), (3, 208, 112, 2, True, 1), (4, 208, 112, 2, True, 1), (5, 208, 112, 2, True, 1),
             (6, 208, 112, 0, True, 0)]
    for frame, w, h, pflags, p16, sflags in steps:
        f = synth.make_frame(scene, frame, w, h, dev)
        color = B.to_storage((torch.from_numpy(np.random.default_rng(2000 + frame).random((h, w, 4)).astype(np.float32)) * 2.0).to(dev))
        sa, ta = B.SSAOAttribs.default(), B.TAAAttribs.default()
        ctx.prepare_resources(frame, w, h, feature_flags=pflags)
        ssao.prepare_resources(feature_flags=sflags)
        taa.prepare_resources(2)
        ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
        ssao.execute(f["depth"], B.to_storage(f["normal"]), sa)
        taa.execute(color, ta)
        quant.depth16["postfx"], quant.depth16["ssao"] = p16, bool(sflags & 1)
        g = {k: to_np(f[k]) for k in ("depth", "prev_depth", "motion", "normal")}
        g["normal"] = q16(g["normal"])
        keep = {}
        pf = cpu.postfx(frame, g["depth"], g["prev_depth"], g["motion"], bytes(f["camera"]), bytes(f["prev_camera"]), (sobol, tile))
        want_ao = cpu.ssao(pf, g["depth"], g["normal"], sa, keep, half_precision_depth=bool(sflags & 1))
        want_taa = cpu.taa(pf, f32(color), ta, None)
        prevd, reproj = to_np(ctx.get_previous_depth()), to_np(ctx.get_reprojected_depth())
        assert np.array_equal(prevd, pyref.store_unorm16(g["prev_depth"]) if p16 else g["prev_depth"]), f"previous depth frame {frame}"
        assert not p16 or np.array_equal(pyref.store_unorm16(reproj), reproj), "the reprojected depth holds R16_UNORM values"
        res = {}
        _, res["reprojected depth"] = assert_close(reproj, pf["reproj_depth"], abs_slack=U16 if p16 else None, max_outlier_frac=0.0, what=f"reprojected depth frame {frame}")
        if sflags & 1:
            for k in range(1, 5):
                got = to_np(ssao.get_intermediate(f"prefiltered_depth{k}"))
                assert np.array_equal(pyref.store_unorm16(got), got), f"prefiltered depth level {k} holds R16_UNORM values"
                _, res[f"prefiltered {k}"] = assert_close(got, keep["ssao_prefiltered_depth"][k], abs_slack=U16, max_outlier_frac=0.0, what=f"prefiltered depth level {k} frame {frame}")
        _, res["ssao"] = assert_close(to_np(api.widen(ssao.get_ambient_occlusion())), want_ao, abs_slack=AO_STEP, max_outlier_frac=1.0 if MEASURE else 2e-3, what=f"SSAO frame {frame}")
        _, res["taa"] = assert_close(f32(taa.get_accumulated_frame()), want_taa, rtol=RTOL, max_outlier_frac=1.0 if MEASURE else 2e-3, what=f"TAA frame {frame}")
        print(f"h4 half-precision depth frame {frame} ({w}x{h}, PostFX planes R16 {p16}, SSAO flag {sflags}): outlier fractions " + " ".join(f"{k} {v:.1e}" for k, v in res.items()), flush=True)
    # the flag changes results: the same frame with and without it differs in the AO (a check that the path is live, not a bound)
    for fx in (ssao, taa):
        fx.close()
    ctx.close()


def section_sharded(S):
    sobol, tile, dev, ibl, sa, scene = (S[k] for k in ("sobol", "tile", "dev", "ibl", "sa", "scene"))
    # 6. the sharded frame on binary16 planes: two in-process ranks (mifx_comm_create_local_group), band for band bit-identical to the unsharded chain
    import threading

    w3, h3 = 256, 512
    ref = api.Chain(0, sobol, tile)
    chains = [api.Chain(0, sobol, tile) for _ in range(2)]
    comms = api.Comm.local_group(chains[0].postfx, 2)
    cuts = [0, 240, h3]
    frames = [synth.make_frame(scene, i, w3, h3, dev) for i in range(3)]
    mm = int(max(float(fr["motion"][..., 1].abs().max()) for fr in frames) * 0.5 * h3) + 2
    outs = [torch.zeros(h3, w3, 4, device=dev, dtype=torch.float16) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    want = torch.zeros(h3, w3, 4, device=dev, dtype=torch.float16)
    for r in range(2):
        chains[r].set_sharding(comms[r], cuts, mm)
    errors = []
    for i, fr in enumerate(frames):
        ref.execute(ref.bind_frame(i, fr, ibl, sa, want))
        torch.cuda.synchronize()

        def run(r):
            try:
                with torch.cuda.stream(streams[r]):
                    chains[r].execute_sharded(chains[r].bind_frame(i, fr, ibl, sa, outs[r]))
                streams[r].synchronize()
            except Exception as e:  # noqa: BLE001
                errors.append((r, repr(e)))

        ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not errors, errors
        torch.cuda.synchronize()
        for r in range(2):
            assert torch.equal(outs[r][cuts[r]:cuts[r + 1]], want[cuts[r]:cuts[r + 1]]), f"h4 sharded frame {i}: band of rank {r} differs"
    for r in range(2):
        chains[r].set_sharding(None)
        comms[r].close()
        chains[r].close()
    ref.close()
    print("h4 sharded: 3 frames x 2 ranks bit-identical to the unsharded chain", flush=True)


def section_layers(S):
    """The shade with material layers in the native-storage build: the G-buffer's and the layers' 4-channel planes are RGBA16_FLOAT, the outputs too; the checker (the
    reference's permutation) reads the binary16 values and its output takes the store's rounding."""
    from layers_util import BACKGROUND, IOR, ROTATION, checker_result, make_case

    lib = pyref.ref_lib()
    if lib is None or not lib.has("ref_pbr_shade_layers_all_shadows3"):
        print("h4 section layers: no oracle/_ref with the layered permutations, skipped")
        return
    dev, ibl_np, ibl, chain = S["dev"], S["ibl_np"], S["ibl"], S["chain"]
    f, gn, sa, planes, albedo, charlie = make_case("all_shadows3", (224, 128), ibl_np, dev, shadowed=True)
    slices, infos = chain_util.make_shadow_inputs()
    for k in ("base_color", "normal", "material", "emissive"):
        gn[k] = q16(gn[k])
    planes = {k: (v if k == "transmission" else q16(v)) for k, v in planes.items()}
    g = {k: (B.to_storage(torch.from_numpy(v).to(dev)) if v.ndim == 3 else torch.from_numpy(v).to(dev)) for k, v in gn.items()}
    lp = {k: B.to_storage(torch.from_numpy(v).to(dev)) for k, v in planes.items() if k != "transmission"}
    lp["transmission"] = torch.from_numpy(np.ascontiguousarray(planes["transmission"][..., 0])).to(dev)
    lp["sheen_albedo_scaling_lut"], lp["preintegrated_charlie"] = torch.from_numpy(albedo).to(dev), torch.from_numpy(charlie).to(dev)
    sm = torch.from_numpy(np.stack(slices)).to(dev)
    rad, spec = api.pbr_shade_layers(chain.postfx, g, lp, 31, f["camera"], sa, ibl, background=BACKGROUND, iridescence_ior=IOR, anisotropy_rotation=ROTATION, shadows=(sm, infos, 3))
    assert rad.dtype == torch.float16 and spec.dtype == torch.float16
    wr, ws = checker_result(lib, "all_shadows3", True, f, gn, sa, planes, albedo, charlie, ibl_np, shadows=(slices, infos))
    budget = 1.0 if MEASURE else 5e-5
    _, a = assert_close(f32(rad), q16(wr), rtol=RTOL, max_outlier_frac=budget, what="layered shade, radiance (RGBA16_FLOAT)")
    _, b = assert_close(f32(spec), q16(ws), rtol=RTOL, max_outlier_frac=budget, what="layered shade, specular IBL (RGBA16_FLOAT)")
    print(f"h4 layers: outlier fractions radiance {a:.2e}, specular IBL {b:.2e}; {(f32(rad) == q16(wr)).mean():.4f} of the radiance values on the same binary16 code")


# ------------------------------------------------------------------------------------------------ boundary frame sizes
# Bloom's minimum and that plus one, ODD / COLLAPSE of tests/test_gpu_frame_edges.py, the size of test_chain_layouts_native_storage_build, the shade test's odd size
EDGE_CHAIN_SIZES = [(8, 8), (9, 8), (33, 17), (67, 37), (129, 65), (131, 77), (300, 12)]
# where the checker's SSR plane is not empty (6.3 / 10.3 / 11.3 % of its texels above 1e-3 in the fourth frame; it is empty at (8, 8), (33, 17) and (300, 12))
EDGE_CHAIN_SSR_SIZES = [(67, 37), (129, 65), (131, 77)]
# The one budget above the 224 x 128 fraction: the "same code" comparisons of Bloom's output and the final image at the two sizes below.  Measured on an MI355X
# (profiles/h4_edges_parity.txt): 33 x 17 up to 5 of 2244 values (2.2e-3), 300 x 12 up to 45 of 14400 (3.1e-3), against 1 and 7 that 5e-4 allows; every other comparison at every
# size is inside the 224 x 128 fraction.  They are rounding ties of the output pass alone: every pyramid level (down and up) is on the checker's chain's code at these frames, and for
# each offending value the checker's own unrounded result of the output pass, on the HIP side's own planes, lies within 2.5e-6 (relative) of the boundary between the two
# codes (bloom_passes_on_own_planes asserts that for every value of every frame: none is further than 1e-3).  In the frames concerned nothing of these two small frames passes
# Bloom's threshold: the checker's up0 is zero throughout, the output is TAA's binary16 colour itself, and 59 - 69 (33 x 17) and 377 - 412 (300 x 12) of those binary16 values lie
# EXACTLY on the boundary between two 6- or 5-bit codes (one mantissa pattern in 16 or 32).  The HIP pass loads the centre texel and rounds the tie to even; the checker's
# bilinear centre tap (weight 1 - O(1e-5), util.centre_tap_slack) lands just beside it on some of them.  5e-3 is what the fp32 suite grants the final
# image at these sizes (tests/test_gpu_frame_edges.py::test_chain_edges), the ceiling for this budget.
EDGE_SAME_CODE_BUDGET = {(33, 17): 5e-3, (300, 12): 5e-3}


def r11g11b10_codes_or_ties(got, unrounded, what):
    """`got`: an R11G11B10_FLOAT plane of the HIP side (values); `unrounded`: the checker's full-precision result of the same pass on the same inputs.  Every value must be the
    code `unrounded` rounds to -- or, where the checker's unrounded value lies within 1e-3 (relative, the contract's tolerance) of the boundary between two codes, the code on
    the other side of that boundary: two results that agree to 1e-3 cannot be asked to fall on the same side.  Returns (values on the neighbouring code, largest distance of
    such a value from its boundary)."""
    import format_ref

    ties, worst = 0, 0.0
    for c, m in ((0, 6), (1, 6), (2, 5)):
        g, u = got[..., c].astype(np.float32), unrounded[..., c].astype(np.float32)
        want_code = format_ref.float_to_ufloat(u, m).astype(np.int64)
        got_code = format_ref.float_to_ufloat(g, m).astype(np.int64)
        assert np.array_equal(format_ref.ufloat_to_float(got_code.astype(np.uint32), m), g), f"{what}: channel {c} holds values that are no R11G11B10 code"
        bad = got_code != want_code
        if bad.any():
            w = format_ref.ufloat_to_float(want_code.astype(np.uint32), m)
            assert MEASURE or (np.abs(got_code - want_code)[bad] == 1).all(), f"{what}: channel {c}: {int((np.abs(got_code - want_code) > 1).sum())} values more than one code away"
            boundary = 0.5 * (g[bad].astype(np.float64) + w[bad].astype(np.float64))
            dist = np.abs(u[bad].astype(np.float64) - boundary) / np.maximum(np.abs(u[bad].astype(np.float64)), 1e-30)
            assert MEASURE or float(dist.max()) <= 1e-3, f"{what}: channel {c}: a value on the neighbouring code although the checker's unrounded value is {float(dist.max()):.3e} from the boundary"
            ties, worst = ties + int(bad.sum()), max(worst, float(dist.max()))
    return ties, worst


def bloom_passes_on_own_planes(S, chain, what):
    """Every pass of the chain's Bloom on the HIP side's own planes (TAA's output, its own pyramid levels) against the checker's pass WITHOUT the store's rounding: each
    R11G11B10 value the HIP side stored is the code the checker's value rounds to, rounding ties apart (r11g11b10_codes_or_ties).  End to end (chain_frames) one tie in a small
    level moves every texel of the larger levels it is up-sampled into, so the share of values on another code grows on frames whose pyramid collapses early; pass by pass
    nothing is left to grow."""
    plain, pfx = S["plain"], S["pfx"]
    bloom = chain.effect("bloom")
    ab = bytes(chain.bloom_attribs)
    taa = f32(chain.effect_output("taa"))
    h, w = taa.shape[:2]
    tex_count = cpu_chain.compute_mip_levels_count(w // 2, h // 2)
    mips = int(np.float32(chain.bloom_attribs.Radius) * np.float32(tex_count))
    down = [bloom_rgba(bloom.get_intermediate(f"down{i}")) for i in range(mips)]
    up = [bloom_rgba(bloom.get_intermediate(f"up{i}")) for i in range(mips - 1)]
    ties, worst = 0, 0.0

    def hold(name, got, call):
        nonlocal ties, worst
        u = np.zeros_like(got)
        call(u)
        t, d = r11g11b10_codes_or_ties(got, u, f"{what} {name}")
        ties, worst = ties + t, max(worst, d)

    hold("prefilter", down[0], lambda u: plain.call(pfx + "bloom_prefilter", [taa], [u], attribs=ab))
    for i in range(1, mips):
        hold(f"down{i}", down[i], lambda u: plain.call(pfx + "bloom_downsample", [down[i - 1]], [u]))
    for i in range(mips - 1, 0, -1):
        src = up[i] if i != mips - 1 else down[i]
        hold(f"up{i - 1}", up[i - 1], lambda u: plain.call(pfx + "bloom_upsample", [down[i - 1], src], [u], attribs=ab, ival=[0]))
    hold("output", bloom_rgba(chain.effect_output("bloom")), lambda u: plain.call(pfx + "bloom_upsample", [taa, up[0]], [u], attribs=ab, ival=[3]))
    return mips, ties, worst


def section_edges(S):
    """The chain at the boundary frame sizes, four frames each, every effect's output against the format-emulating checker (chain_frames: the comparisons of section
    `chain`).  Partial 8x8 / 32x8 tiles, odd widths (an unpaired last column of the 1-, 2- and 4-byte planes), pyramid levels of one texel, Bloom's tail from its first level.
    The budgets are the fractions of section `chain` as whole numbers of values, rounded down: none on the small frames."""
    pfx, quant, sobol, tile, dev = (S[k] for k in ("pfx", "quant", "sobol", "tile", "dev"))
    for w, h in EDGE_CHAIN_SIZES:
        chain = api.Chain(0, sobol, tile)
        out = torch.zeros(h, w, 4, device=dev, dtype=torch.float16)
        def bloom_alone(frame, keep):
            mips, ties, worst = bloom_passes_on_own_planes(S, chain, f"edges {w}x{h} frame {frame} Bloom")
            bloom = chain.effect("bloom")
            off = [int((bloom_rgba(bloom.get_intermediate(f"{n}{i}"))[..., :3] != lv[..., :3]).sum()) for n in ("down", "up") for i, lv in enumerate(keep[f"bloom_{n}"])]
            print(f"h4 edges {w}x{h} frame {frame}: Bloom pass by pass on its own planes: {mips} levels, every value on the checker's code but {ties} rounding ties"
                  + (f" (the checker's unrounded value within {worst:.1e} of the code boundary)" if ties else "")
                  + f"; end to end, values on another code than the checker's chain per level, down0.. then up0..: {off}", flush=True)

        keep = chain_frames(S, chain, cpu_chain.CpuChain(quant, pfx), out, (w, h), 4, counted=True, label=f"edges {w}x{h}", after_frame=bloom_alone,
                            same_code=EDGE_SAME_CODE_BUDGET.get((w, h)))
        lit = float((keep["final"][..., :3].max(-1) > 0.02).mean())
        ssr_share = float((keep["ssr_out"][..., :3] > 1e-3).any(-1).mean())
        ao_share = float((keep["ssao_out"] < 0.99).mean())
        print(f"h4 edges {w}x{h}: checker's last frame: {lit:.3f} of the texels lit, SSR above 1e-3 on {ssr_share:.3f}, SSAO below 0.99 on {ao_share:.3f}", flush=True)
        assert lit > 0.5 and ao_share > 0.5, "the comparison went hollow"
        assert (w, h) not in EDGE_CHAIN_SSR_SIZES or ssr_share >= 0.03, f"{w}x{h}: the checker's SSR plane is all but empty ({ssr_share:.4f})"
        chain.close()


def effect_colour(f):
    """The colour input of tests/test_gpu_bloom_taa.py::taa_multi_frame"""
    return torch.cat([f["base_color"][..., :3] * 2.0 + 0.05 * f["normal"][..., :3].abs(), f["base_color"][..., 3:4]], -1).contiguous()


def section_effects_thin(S):
    """The effects alone below the chain's minimum frame (Bloom's 8 x 8): SSAO, SSR, TAA (flags 0 and 7) over three frames, the shade, and the tone map / auto exposure on a
    packed R11G11B10 plane, at the thin and odd sizes of tests/test_gpu_frame_edges.py.  Budgets: the fractions of section `chain` as whole numbers of values, rounded down
    (none at most of these sizes, as in the fp32 per-pass edge tests)."""
    import format_ref
    from test_gpu_frame_edges import THIN

    pfx, quant, sobol, tile, dev, ibl_np, ibl = (S[k] for k in ("pfx", "quant", "sobol", "tile", "dev", "ibl_np", "ibl"))
    scene = synth.Scene()
    bg = (0.02, 0.03, 0.05, 0.0)
    for w, h in THIN + [(33, 17), (65, 9)]:
        ctx = api.PostFXContext(0, sobol, tile)
        ssao, ssr, taa0, taa7 = api.ScreenSpaceAmbientOcclusion(ctx), api.ScreenSpaceReflection(ctx), api.TemporalAntiAliasing(ctx), api.TemporalAntiAliasing(ctx)
        cpu = {flags: cpu_chain.CpuChain(quant, pfx, taa_flags=flags) for flags in (0, 7)}  # (two histories of the checker's TAA; SSAO and SSR on the first)
        worst = {}

        def cmp(name, got, want, budget, **kw):
            n = np.asarray(want).size
            worst[name] = max(worst.get(name, 0.0), assert_close(got, want, max_outlier_frac=1.0 if MEASURE else as_count(budget, n), what=f"h4 thin {w}x{h} {name} frame {frame}", **kw)[1])

        for frame in range(3):
            f = synth.make_frame(scene, frame, w, h, dev)
            color, normal, material = (B.to_storage(t) for t in (effect_colour(f), f["normal"], f["material"]))
            ctx.prepare_resources(frame, w, h)
            ssao.prepare_resources()
            ssr.prepare_resources()
            taa0.prepare_resources(0)
            taa7.prepare_resources(7)
            ctx.execute(f["depth"], f["prev_depth"], f["motion"], f["camera"], f["prev_camera"])
            sa, ra, ta = B.SSAOAttribs.default(), B.SSRAttribs.default(), B.TAAAttribs.default()
            ssao.execute(f["depth"], normal, sa)
            ssr.execute(color, f["depth"], normal, material, f["motion"], ra)
            taa0.execute(color, ta)
            taa7.execute(color, ta)
            torch.cuda.synchronize()
            g = {k: to_np(f[k]) for k in ("depth", "prev_depth", "motion")}
            cn, nn, mn = f32(color), f32(normal), f32(material)  # the binary16 values the HIP side was given
            pf = {flags: c.postfx(frame, g["depth"], g["prev_depth"], g["motion"], bytes(f["camera"]), bytes(f["prev_camera"]), (sobol, tile)) for flags, c in cpu.items()}
            want_ssr = cpu[0].ssr(pf[0], cn, g["depth"], nn, mn, g["motion"], ra)
            got_ssr = f32(ssr.get_ssr_radiance())
            assert np.isfinite(got_ssr).all()
            cmp("SSAO", to_np(api.widen(ssao.get_ambient_occlusion())), cpu[0].ssao(pf[0], g["depth"], nn, sa), CHAIN_BUDGET["ssao"], abs_slack=AO_STEP)
            cmp("SSR", got_ssr, want_ssr, CHAIN_BUDGET["ssr"], rtol=RTOL)
            cmp("TAA flags 0", f32(taa0.get_accumulated_frame()), cpu[0].taa(pf[0], cn, ta), CHAIN_BUDGET["taa"], rtol=RTOL)
            cmp("TAA flags 7", f32(taa7.get_accumulated_frame()), cpu[7].taa(pf[7], cn, ta), CHAIN_BUDGET["taa"], rtol=RTOL)
        assert ssao.get_ambient_occlusion().dtype == torch.uint8 and ssr.get_ssr_radiance().dtype == torch.float16 and taa0.get_accumulated_frame().dtype == torch.float16
        # of the thin sizes only 3 x 97 has reflections (the checker's plane peaks at 1.41 there); the chain sizes of section `edges` cover SSR elsewhere
        assert (w, h) != (3, 97) or float(want_ssr[..., :3].max()) > 1e-3, "3x97: the checker's SSR plane is empty"
        for fx in (ssao, ssr, taa0, taa7):
            fx.close()
        # the shade (tests/test_gpu_pbr.py::pbr_shade with the emissive and occlusion planes), both outputs
        frame = 4
        f = synth.make_frame(scene, frame, w, h, dev)
        gen = torch.Generator(device="cpu").manual_seed(3)
        gb = {"base_color": B.to_storage(f["base_color"]), "normal": B.to_storage(f["normal"]), "material": B.to_storage(f["material"]), "depth": f["depth"],
              "emissive": B.to_storage((torch.rand(h, w, 4, generator=gen) * 0.3).to(dev)), "occlusion": (0.3 + 0.7 * torch.rand(h, w, generator=gen)).to(dev)}
        attribs = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
        attribs.OcclusionStrength, attribs.EmissionScale = 0.8, 1.5
        attribs.IBLScale[:] = [1.1, 0.9, 1.0, 1.0]
        attribs.Lights[attribs.LightCount] = B.PBRLightAttribs(3, 2.0, 6.0, -3.0, -0.2, -0.9, 0.3, -1, 40.0, 35.0, 30.0, 20.0 ** 4, 8.0, -6.8, 0.0, 0.0)  # a spot light: the third light type
        attribs.LightCount += 1
        rad, spec = api.pbr_shade(ctx, gb, f["camera"], attribs, ibl, background=bg)
        assert rad.dtype == torch.float16 and spec.dtype == torch.float16
        gn = {k: f32(v) for k, v in gb.items()}
        wr, ws = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        quant.call(pfx + "pbr_shade", [gn["base_color"], gn["normal"], gn["material"], gn["depth"], gn["emissive"], gn["occlusion"], ibl_np["lut"], ibl_np["irradiance"],
                                       ibl_np["prefiltered"]], [wr, ws], cam0=bytes(f["camera"]), attribs=bytes(attribs), fval=list(bg))
        assert np.isfinite(f32(rad)).all() and np.array_equal(wr, q16(wr))  # (the checker's outputs went through the RGBA16_FLOAT store)
        cmp("shade, radiance", f32(rad), wr, CHAIN_BUDGET["radiance"], rtol=RTOL)
        cmp("shade, specular IBL", f32(spec), ws, CHAIN_BUDGET["radiance"], rtol=RTOL)
        # mifx_tonemap_execute, mifx_tonemap_execute_auto and the auto exposure on a packed R11G11B10 plane of this size
        values = pyref.store_r11g11b10(to_np(synth.make_hdr_buffer(w, h, dev)), alpha_reads_as=1.0)
        packed = torch.from_numpy(format_ref.encode(values, "R11G11B10_FLOAT").view(np.int32).reshape(h, w).copy()).to(dev)
        assert np.array_equal(bloom_rgba(packed), values)
        packed_equals_half(ctx, packed, values)
        ctx.close()
        print(f"h4 thin {w}x{h}: outlier fractions " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "; packed plane == its RGBA16_FLOAT copy through tone map and auto exposure", flush=True)


def spacing16(a):
    """The distance from |a| to the next binary16 value above it (a: binary16 values as float32); NaN / infinity -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.spacing(np.abs(a).astype(np.float16)).astype(np.float32)
    return np.where(np.isfinite(s), s, np.float32(0))


def assert_within_tol_after_the_store(got, want32, tol, what):
    """`got` (an RGBA16_FLOAT plane's values) against q16(want32) where the fp32 test grants the absolute `tol`: two values within tol before the store are at most tol + one
    binary16 spacing apart after it.  NaN where the expected value is NaN, and only there; no value left out."""
    want = q16(want32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at {int((np.isnan(got) != np.isnan(want)).sum())} values where the other side has a number"
    ok = ~np.isnan(want)
    with np.errstate(invalid="ignore"):
        over = np.abs(got - want) - (np.float32(tol) + spacing16(want))
    assert np.isfinite(got[ok]).all() and float(over[ok].max(initial=-1.0)) <= 0.0, f"{what}: {int((over[ok] > 0).sum())} of {int(ok.sum())} values beyond {tol} + one binary16 spacing (worst by {float(over[ok].max()):.3e})"
    return float(np.abs(got - want)[ok].max(initial=0.0))


def same_bits(a, b):
    """Bit for bit (a NaN equals itself only bit-wise)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def section_grid(S):
    """The coordinate grid in the native-storage build: mifx_coordinate_grid_render (fp32 raw output, an RGBA16_FLOAT blend target), mifx_copy_frame_render (RGBA16_FLOAT and
    packed R11G11B10 colour inputs, an RGBA16_FLOAT frame) and the chain with the grid on.  References: the reference fixture tests/golden/grid_golden.npz and the product's
    per-pixel header compiled for the host (tests/test_grid_cpu.py holds it to the fixture), both fed the binary16 values the HIP side is given."""
    import shutil

    import grid_util as G
    import test_grid_cpu as C
    from test_gpu_grid import GRID_FLAGS, TOL, _attribs, _cam, _edge_inputs, _tm

    sobol, tile, dev, ibl, sa, scene = (S[k] for k in ("sobol", "tile", "dev", "ibl", "sa", "scene"))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed for the host compilation of mifx_coordinate_grid.h"
    host = C.build_host_lib(hipcc)
    ctx = api.PostFXContext(0, sobol, tile)
    renderer = api.CoordinateGridRenderer(ctx)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    golden = C.golden()

    def render_case(name, depth, cam, attribs, flags, want_raw, dst, blend_own_raw=False):
        raw = renderer.render(up(depth), _cam(cam), _attribs(attribs), flags, raw=True)
        assert raw.dtype == torch.float32
        got = to_np(raw)
        worst_raw = float(np.abs(got - want_raw).max())
        assert np.isfinite(got).all() and worst_raw <= TOL, f"{name}: raw output off by {worst_raw:.3e}"
        # blended into an RGBA16_FLOAT colour target as BS_AlphaBlend does on rgb; the target's alpha stays, bit for bit
        target = up(q16(dst)).half()
        before = target.clone()
        renderer.render(up(depth), _cam(cam), _attribs(attribs), flags, color_target=target, raw=False)
        torch.cuda.synchronize()
        worst = assert_within_tol_after_the_store(f32(target), G.blend(q16(dst), got if blend_own_raw else want_raw), TOL, f"{name}: blended target")
        assert same_bits(target[..., 3], before[..., 3]) and not same_bits(target, before), f"{name}: the target's alpha"
        print(f"h4 grid {name}: raw max {worst_raw:.3e}, blended RGBA16_FLOAT target max {worst:.3e}", flush=True)
        return got

    def copy_case(name, c):
        c = dict(c, color=q16(c["color"]))
        out = torch.zeros(c["depth"].shape + (4,), device=dev, dtype=torch.float16)
        ctx.copy_frame(up(c["color"]).half(), up(c["depth"]), _cam(c["camera"]), _tm(c["tone_mapping"]), float(c["ave_log_lum"]), int(c["tonemap_flags"]), _attribs(c["attribs"]),
                       c["flags"], out=out)
        torch.cuda.synchronize()
        worst = assert_within_tol_after_the_store(f32(out), C.host_copy_frame(host, c), TOL, f"{name}: copy frame")
        print(f"h4 grid {name}: copy frame max {worst:.3e}, NaN at {int(np.isnan(f32(out)).sum())} values (as the host compilation)", flush=True)

    for i, name in C.golden_cases(("render",)):
        c = C.case(golden, i)
        render_case(name, c["depth"], c["camera"], c["attribs"], c["flags"], c["out"], np.random.default_rng(i).uniform(0.0, 2.0, c["out"].shape).astype(np.float32))
    for i, name in C.golden_cases(("copy",)):
        copy_case(name, C.case(golden, i))
    # an odd size (partial 64x4 blocks, an unpaired last column of 8-byte texels): tests/test_gpu_grid.py::test_render_and_copy_frame_edges
    w, h = 33, 17
    cam, depth, color = _edge_inputs(w, h, w * 131 + h)
    a = G.default_attribs()
    render_case("33x17", depth, cam, a, G.ALL, C.host_render(host, depth, cam, a, G.ALL), color, blend_own_raw=True)  # (blended with the raw output it was held to, as there)
    words = np.frombuffer(bytes(B.ToneMappingAttribs.default(4)), np.uint32)
    copy_case("33x17", dict(color=color, depth=depth, camera=cam, tone_mapping=words, ave_log_lum=0.3, tonemap_flags=1, attribs=a, flags=G.FLAG_XZ | G.FLAG_AXIS_X))
    ctx.close()
    # the chain with the grid on: its frame is mifx_copy_frame_render on its own packed Bloom output, bit for bit
    # (tests/test_gpu_grid.py::test_chain_frame_equals_copy_frame_on_its_own_bloom_output, variant plain)
    w, h = 208, 120
    on, off = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    grid = B.CoordinateGridAttribs.default()
    on.set_coordinate_grid(grid, GRID_FLAGS)
    x, y, want = (torch.zeros(h, w, 4, device=dev, dtype=torch.float16) for _ in range(3))
    changed = False
    frames = [synth.make_frame(scene, i, w, h, dev) for i in range(4)]
    for i, f in enumerate(frames):
        on.execute(on.bind_frame(i, f, ibl, sa, x))
        off.execute(off.bind_frame(i, f, ibl, sa, y))
        torch.cuda.synchronize()
        bloom = on.effect_output("bloom")
        assert bloom.dtype == torch.int32 and torch.equal(bloom, off.effect_output("bloom")), i  # (everything in front of the last pass is what the chain computes without the grid)
        on.postfx.copy_frame(bloom, f["depth"], f["camera"], on.tone_mapping, on.ave_log_lum, on.tonemap_flags, grid, GRID_FLAGS, out=want)
        torch.cuda.synchronize()
        assert same_bits(x, want), (i, int((x.view(torch.int16) != want.view(torch.int16)).sum()))
        changed |= not same_bits(x, y)
    assert changed
    try:
        on.execute_native(on.bind_frame(0, frames[0], ibl, sa, x), "RGBA8_UNORM_SRGB")
        raise AssertionError("mifx_chain_execute_native with a grid was not refused")
    except B.MifxError:
        pass
    for k, (attribs, flags) in enumerate(((None, 0), (grid, GRID_FLAGS), (grid, G.FLAG_SRGB))):  # grid off again: the plain chain's output, bit for bit
        on.set_coordinate_grid(attribs, flags)
        on.execute(on.bind_frame(len(frames) + k, frames[-1], ibl, sa, x))
        off.execute(off.bind_frame(len(frames) + k, frames[-1], ibl, sa, y))
        torch.cuda.synchronize()
        assert same_bits(x, y) == (flags != GRID_FLAGS), k
    on.close()
    off.close()
    print("h4 grid: the chain's frame with the grid == mifx_copy_frame_render on its own packed Bloom output, 4 frames bit for bit", flush=True)


def section_envmap(S):
    """mifx_envmap_render into an RGBA16_FLOAT colour target (tests/test_gpu_pbr.py::test_envmap_background_parity): the background texels against the checker's colour
    rounded by the store, the fp32 motion vectors as in the fp32 build, everything else untouched."""
    from test_oracle_vs_ref import run_envmap

    plain, pfx, dev = S["plain"], S["pfx"], S["dev"]
    ctx = api.PostFXContext(0)
    env_mips = api.cube_box_mips(synth.make_sky_cube(32, dev).clamp(max=500.0))
    scale = (1.5, 1.0, 0.75)
    for w, h in ((208, 120), (33, 17)):
        f = synth.make_frame(synth.Scene(), 9, w, h, dev)
        inp = {"env": [to_np(m) for m in env_mips], "depth": to_np(f["depth"]), "cam": bytes(f["camera"]), "prev": bytes(f["prev_camera"])}
        bg = inp["depth"] >= 1.0
        assert 0.05 < bg.mean() < 0.95
        for mode, gamma, mip in ((0, 0, 1.0), (4, 1, 1.0)):
            color = torch.full((h, w, 4), -7.0, device=dev, dtype=torch.float16)
            motion = torch.full((h, w, 2), -7.0, device=dev)
            api.render_env_map(ctx, env_mips, f["depth"], color, motion, f["camera"], f["prev_camera"], B.ToneMappingAttribs.default(mode), 0.3, mip, 0.25, scale,
                               (api.ENVMAP_OPTION_FLAG_CONVERT_OUTPUT_TO_SRGB if gamma else 0) | api.ENVMAP_OPTION_FLAG_COMPUTE_MOTION_VECTORS)
            torch.cuda.synchronize()
            # (the reference is compiled for tone mapping NONE and Uncharted2 + gamma: both cases here)
            want_c, want_m = run_envmap(plain, pfx, inp, mode, gamma, mip, 0.25, scale)
            got_c, got_m = f32(color), to_np(motion)
            assert_close(got_c, q16(want_c), rtol=RTOL, what=f"h4 env map colour {w}x{h} mode {mode}")
            assert_close(got_m, want_m, atol=1e-6, what=f"h4 env map motion {w}x{h} mode {mode}")
            assert (got_c[~bg] == -7.0).all() and (got_m[~bg] == -7.0).all() and (got_c[bg][:, 3] == 0.25).all()
            print(f"h4 env map {w}x{h} mode {mode} gamma {gamma}: colour and motion of {int(bg.sum())} background texels agree, {(got_c[bg] == q16(want_c)[bg]).mean():.4f} of the colour values on the same binary16 code", flush=True)
    ctx.close()


# (entry point of include/mifx.h that takes a caller image, the sections above that run it in the native-storage build): the coverage guard
# tests/test_frame_edges_coverage.py reads this table
H4_MATRIX = {
    "mifx_postfx_execute": "effects_thin, half_precision_depth, dof",
    "mifx_ssao_execute": "effects_thin, half_precision_depth",
    "mifx_ssr_execute": "effects_thin",
    "mifx_taa_execute": "effects_thin, half_precision_depth",
    "mifx_bloom_execute": "dof_chain",
    "mifx_dof_execute": "dof, dof_passes, dof_chain",
    "mifx_pbr_shade_execute": "effects_thin",
    "mifx_pbr_shade_execute_layers": "layers",
    "mifx_autoexposure_execute": "effects_thin, chain",
    "mifx_tonemap_execute": "effects_thin, chain",
    "mifx_tonemap_execute_auto": "effects_thin, chain",
    "mifx_chain_execute": "edges, chain, fusion, grid",
    "mifx_chain_execute_sharded": "sharded",
}

SECTIONS = {"chain": section_chain, "fusion": section_fusion, "dof": section_dof, "dof_chain": section_dof_chain, "dof_passes": section_dof_passes, "half_precision_depth": section_half_precision_depth, "sharded": section_sharded, "layers": section_layers,
            "edges": section_edges, "effects_thin": section_effects_thin, "grid": section_grid, "envmap": section_envmap}


def main():
    names = sys.argv[1:] or list(SECTIONS)
    S = setup()
    for n in names:
        SECTIONS[n](S)
        print(f"h4 section {n} OK", flush=True)
    S["chain"].close()
    print("h4 checks OK")


if __name__ == "__main__":
    main()
