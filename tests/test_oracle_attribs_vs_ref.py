"""Non-default attribute blocks: every effect of the chain run by the hand-written oracle and by the reference build (oracle/_ref) with the attributes moved
away from the struct defaults the other tests use -- radii, thresholds, stability factors, channel / flag switches, all three SSAO algorithms and TAA
flag sets -- over several frames with history.  CPU only; this is part of the oracle's pin."""
import numpy as np
import pytest

import cpu_chain
from attrib_sets import BLOOM_SETS, DOF_SETS, SSAO_SETS, SSR_SETS, TAA_SETS, TONEMAP_SETS  # (the rows: tests/attrib_sets.py composes the chain-wide sets from them)
from util import assert_close, blue_noise_tables

W, H, FRAMES = 72, 48, (5, 6, 7)


def frames():
    import torch
    from diligentfx_amd import synth
    from diligentfx_amd.binding import as_bytes

    scene = synth.Scene()
    out = []
    for fi in FRAMES:
        f = synth.make_frame(scene, fi, W, H, torch.device("cpu"))
        g = {k: v.numpy() for k, v in f.items() if isinstance(v, torch.Tensor)}
        g["color"] = np.ascontiguousarray(np.concatenate([g["base_color"][..., :3] * 3.0 + 0.2 * np.abs(g["normal"][..., :3]), g["base_color"][..., 3:4]], -1).astype(np.float32))
        # roughness also in the blue channel, squared, for the RoughnessChannel / IsRoughnessPerceptual switches
        g["material_alt"] = np.ascontiguousarray(np.stack([g["material"][..., 1], g["material"][..., 1], g["material"][..., 0] ** 2, g["material"][..., 3]], -1).astype(np.float32))
        out.append((fi, g, as_bytes(f["camera"]), as_bytes(f["prev_camera"])))
    return out


def both(oracle, ref, run, **chain_kw):
    """run(chain, frame tuple, postfx outputs) -> array, on every frame with each library; yields (frame, oracle result, reference result)."""
    tables = blue_noise_tables()
    chains = [cpu_chain.CpuChain(oracle, "oracle_", **chain_kw), cpu_chain.CpuChain(ref, "ref_", **chain_kw)]
    for fr in frames():
        fi, g, cam, prev = fr
        res = []
        for c in chains:
            pf = c.postfx(fi, g["depth"], g["prev_depth"], g["motion"], cam, prev, tables)
            res.append(run(c, fr, pf))
        yield fi, res[0], res[1]




@pytest.mark.parametrize("algo,radius,falloff,mult,mipoff,temporal,spatial,thick", SSAO_SETS)
def test_ssao_attribute_sweep(oracle, ref, algo, radius, falloff, mult, mipoff, temporal, spatial, thick):
    from diligentfx_amd.binding import SSAOAttribs

    a = SSAOAttribs.default()
    a.EffectRadius, a.EffectFalloffRange, a.RadiusMultiplier, a.DepthMIPSamplingOffset = radius, falloff, mult, mipoff
    a.TemporalStabilityFactor, a.SpatialReconstructionRadius, a.BitmaskThickness = temporal, spatial, thick
    a.Algorithm = {"gtao": 0, "hbao": 1, "vbao": 2}[algo]
    a.AlphaInterpolation = 0.7
    for fi, x, y in both(oracle, ref, lambda c, fr, pf: c.ssao(pf, fr[1]["depth"], fr[1]["normal"], a), algorithm=algo):
        assert_close(x, y, rtol=2e-4, atol=1e-6, max_outlier_frac=4e-3, what=f"SSAO {algo} frame {fi}")
        assert 0.0 <= x.min() and x.max() <= 1.0 and x.std() > 0.01




@pytest.mark.parametrize("thick,thresh,mdm,perceptual,channel,trav,bias,radius,trad,tvar,sigma", SSR_SETS)
def test_ssr_attribute_sweep(oracle, ref, thick, thresh, mdm, perceptual, channel, trav, bias, radius, trad, tvar, sigma):
    from diligentfx_amd.binding import SSRAttribs

    a = SSRAttribs.default()
    a.DepthBufferThickness, a.RoughnessThreshold, a.MostDetailedMip, a.IsRoughnessPerceptual, a.RoughnessChannel = thick, thresh, mdm, perceptual, channel
    a.MaxTraversalIntersections, a.GGXImportanceSampleBias, a.SpatialReconstructionRadius = trav, bias, radius
    a.TemporalRadianceStabilityFactor, a.TemporalVarianceStabilityFactor, a.BilateralCleanupSpatialSigmaFactor = trad, tvar, sigma
    a.AlphaInterpolation = 0.6
    material = "material_alt" if channel else "material"
    hits = 0.0
    for fi, x, y in both(oracle, ref, lambda c, fr, pf: c.ssr(pf, fr[1]["color"], fr[1]["depth"], fr[1]["normal"], fr[1][material], fr[1]["motion"], a)):
        assert_close(x, y, rtol=2e-4, atol=1e-6, max_outlier_frac=6e-3, what=f"SSR frame {fi}")
        hits = max(hits, float((x[..., 3] > 0).mean()))
    assert hits > 0.005  # the sweep does produce reflections


@pytest.mark.parametrize("flags,stability,skip", TAA_SETS)
def test_taa_attribute_sweep(oracle, ref, flags, stability, skip):
    from diligentfx_amd.binding import TAAAttribs

    a = TAAAttribs.default()
    a.TemporalStabilityFactor, a.SkipRejection = stability, skip
    for fi, x, y in both(oracle, ref, lambda c, fr, pf: c.taa(pf, fr[1]["color"], a), taa_flags=flags):
        assert_close(x, y, rtol=2e-4, atol=1e-6, max_outlier_frac=2e-3, what=f"TAA flags {flags} frame {fi}")


@pytest.mark.parametrize("intensity,threshold,soft,radius,alpha", BLOOM_SETS)
def test_bloom_attribute_sweep(oracle, ref, intensity, threshold, soft, radius, alpha):
    from diligentfx_amd.binding import BloomAttribs

    a = BloomAttribs.default()
    a.Intensity, a.Threshold, a.SoftTreshold, a.Radius, a.AlphaInterpolation = intensity, threshold, soft, radius, alpha
    for fi, x, y in both(oracle, ref, lambda c, fr, pf: c.bloom(fr[1]["color"], a)):
        assert_close(x, y, rtol=2e-4, atol=1e-6, what=f"Bloom frame {fi}")
        assert (x[..., :3] >= 0).all()
    a.Radius = 0.3  # int(0.3 * 6 levels) = 1: refused here as in mifx_bloom_execute
    with pytest.raises(ValueError):
        cpu_chain.CpuChain(oracle, "oracle_").bloom(frames()[0][1]["color"], a)


SHADE_SETS = [  # (IBL scale rgb, occlusion strength, emission scale, emissive + occlusion planes, lights = "default" | "spots" | "none")
    ((0.5, 1.5, 0.8), 0.4, 2.0, True, "default"),
    ((1.0, 1.0, 1.0), 1.0, 0.0, False, "spots"),
    ((2.0, 0.0, 0.3), 0.0, 1.0, True, "none"),
]


@pytest.mark.parametrize("ibl_scale,occl_strength,emis_scale,planes,lights", SHADE_SETS)
def test_pbr_shade_and_composite_attribute_sweep(oracle, ref, ibl_scale, occl_strength, emis_scale, planes, lights):
    import chain_util
    from diligentfx_amd import binding as B

    ibl = chain_util.make_ibl(oracle, "oracle_")
    sa = chain_util.shade_attribs(len(ibl["prefiltered"]) - 1)
    sa.IBLScale[:] = [*ibl_scale, 1.0]
    sa.OcclusionStrength, sa.EmissionScale = occl_strength, emis_scale
    if lights == "none":
        sa.LightCount = 0
    elif lights == "spots":  # two spot lights with different cones, one point light with a short range, one directional
        sa.Lights[1] = B.PBRLightAttribs(3, 2.0, 9.0, -3.0, 0.0, -1.0, 0.1, -1, 40.0, 36.0, 30.0, 30.0 ** 4, 2.0, -1.2, 0.0, 0.0)
        sa.Lights[2] = B.PBRLightAttribs(3, -4.0, 6.0, 2.0, 0.3, -0.9, -0.2, -1, 10.0, 30.0, 50.0, 12.0 ** 4, 6.0, -5.0, 0.0, 0.0)
        sa.Lights[3] = B.PBRLightAttribs(2, 0.0, 1.5, 0.0, 0.0, -1.0, 0.0, -1, 8.0, 8.0, 2.0, 3.0 ** 4, 0.0, 0.0, 0.0, 0.0)
    fi, g, cam, prev = frames()[1]
    rng = np.random.default_rng(5)
    emissive = (rng.random((H, W, 4)) * 0.5).astype(np.float32) if planes else None
    occlusion = (0.3 + 0.7 * rng.random((H, W))).astype(np.float32) if planes else None
    outs = []
    for lib, prefix in ((oracle, "oracle_"), (ref, "ref_")):
        rad, spec = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        lib.call(prefix + "pbr_shade", [g["base_color"], g["normal"], g["material"], g["depth"], emissive, occlusion, ibl["lut"], ibl["irradiance"], ibl["prefiltered"]],
                 [rad, spec], cam0=cam, attribs=bytes(sa), fval=[0.1, 0.2, 0.3, 0.5])
        # the composite with non-unit SSR / SSAO scales on synthetic SSR / SSAO planes
        ssr = np.concatenate([rng.random((H, W, 3)) * 2.0, rng.random((H, W, 1))], -1).astype(np.float32) if not outs else outs[0][3]
        ssao = rng.random((H, W)).astype(np.float32) if not outs else outs[0][4]
        comp = np.zeros((H, W, 4), np.float32)
        lib.call(prefix + "composite", [rad, spec, ssr, ssao, g["normal"], g["base_color"], g["material"], ibl["lut"]], [comp], cam0=cam, fval=[0.6, 0.35])
        outs.append((rad, spec, comp, ssr, ssao))
    for k, what in enumerate(("radiance", "specular IBL", "composite")):
        assert_close(outs[0][k], outs[1][k], rtol=1e-5, atol=1e-7, what=f"{what} ({lights} lights)")
    assert np.isfinite(outs[0][0]).all() and outs[0][0][..., :3].max() > 0.1


@pytest.mark.parametrize("auto_exposure,middle_gray,white_point,lum_sat,ave_log_lum", TONEMAP_SETS)
def test_tonemap_attribute_sweep(oracle, ref, auto_exposure, middle_gray, white_point, lum_sat, ave_log_lum):
    """ToneMappingAttribs away from the defaults (ToneMappingStructures.fxh:24-52), every operator, with and without the sRGB conversion."""
    import struct

    rng = np.random.default_rng(3)
    img = np.concatenate([np.exp2(rng.uniform(-9, 7, (40, 56, 3))), rng.random((40, 56, 1))], -1).astype(np.float32)
    img[0, :3, :3] = [[0, 0, 0], [1e-12, 1e-12, 1e-12], [1e4, 2e4, 5e3]]
    for mode in range(12):
        attr = struct.pack("<iififfIIffff", mode, auto_exposure, middle_gray, 1, white_point, lum_sat, 0, 0, 1.2, 0.9, 1.1, 0.02)
        for srgb in (0, 1):
            a, b = np.zeros_like(img), np.zeros_like(img)
            oracle.call("oracle_tonemap", [img], [a], attribs=attr, fval=[ave_log_lum], ival=[srgb])
            ref.call("ref_tonemap", [img], [b], attribs=attr, fval=[ave_log_lum], ival=[srgb])
            assert_close(a, b, rtol=2e-6, atol=1e-7, what=f"tone map mode {mode} srgb {srgb}")


@pytest.mark.parametrize("max_coc,temporal,rings,density,alpha", DOF_SETS)
def test_dof_attribute_sweep(oracle, ref, max_coc, temporal, rings, density, alpha):
    """DepthOfFieldAttribs away from the defaults (DepthOfFieldStructures.fxh:31-56): circle-of-confusion limit, temporal stability, Octaweb kernel shape
    (the large-kernel table is regenerated: DepthOfField.cpp:799-809), interpolation alpha; temporal smoothing + Karis inverse on."""
    from diligentfx_amd.binding import DOFAttribs
    from test_oracle_vs_ref import dof_frames, flat, run_cpu_dof

    a = DOFAttribs.default()
    a.MaxCircleOfConfusion, a.TemporalStabilityFactor, a.BokehKernelRingCount, a.BokehKernelRingDensity, a.AlphaInterpolation = max_coc, temporal, rings, density, alpha
    fr = dof_frames(frames=(5, 6, 7), w=80, h=56)
    ka, kb = run_cpu_dof(oracle, "oracle_", fr, a, 3), run_cpu_dof(ref, "ref_", fr, a, 3)
    for fi, (x, y) in enumerate(zip(ka, kb)):
        for name in x:
            for lvl, (p, q) in enumerate(zip(flat(x[name]), flat(y[name]))):
                assert_close(p, q, rtol=1e-6, atol=1e-7, what=f"dof frame {fi} {name}[{lvl}]")
    assert np.abs(ka[-1]["dof_out"][..., :3] - fr[-1]["color"][..., :3]).max() > 0.02
