"""One table of attribute blocks away from the struct defaults (a plain helper module, no fixtures).

The rows are the ones tests/test_oracle_attribs_vs_ref.py pins the hand-written checker to the reference build on (that module takes them from here), so every value
a chain-wide set below uses has been run by both checkers.  SETS composes three chain-wide sets from them; apply() puts one on a chain object -- api.Chain, or the CPU
chain of oracle/cpu_chain.py, which tests/chain_util.py run_frame_inputs reads the same names from.  tests/test_attrib_sets_coverage.py holds the table to the structs."""
import struct

# (algorithm, radius, falloff, radius multiplier, mip offset, temporal, spatial radius, bitmask thickness)
SSAO_SETS = [
    ("gtao", 0.4, 0.3, 1.0, 2.0, 0.5, 2.0, 0.5),
    ("gtao", 2.5, 0.9, 2.0, 4.5, 0.97, 6.0, 0.5),
    ("hbao", 1.7, 0.615, 1.2, 3.3, 0.8, 4.0, 0.5),
    ("vbao", 1.3, 0.615, 1.457, 2.5, 0.9, 3.0, 0.15),
    ("vbao", 0.8, 0.4, 1.8, 3.3, 0.6, 5.0, 1.5),
    ("vbao", 1.2, 0.5, 1.3, 4.5, 0.85, 5.5, 0.25),  # a fractional reconstruction radius (the row windows take its ceil) with the largest mip offset
]
# (thickness, roughness threshold, most detailed mip, perceptual, channel, traversals, GGX bias, spatial radius, temporal rad, temporal var, sigma)
SSR_SETS = [
    (0.05, 0.35, 0, 1, 0, 64, 0.0, 2.0, 0.7, 0.5, 0.5),
    (0.01, 0.5, 1, 1, 1, 128, 0.6, 6.0, 0.95, 0.9, 1.4),
    (0.025, 0.15, 2, 0, 2, 24, 0.3, 4.0, 1.0, 0.9, 0.9),
    (0.1, 1.0, 0, 1, 0, 8, 1.0, 1.0, 0.2, 0.2, 0.2),
]
TAA_SETS = [(0, 0.5, 0), (1, 0.9375, 0), (2, 0.8, 1), (3, 0.99, 0), (4, 0.9, 0), (6, 0.9375, 0), (7, 0.7, 1)]  # (feature flags, stability, skip rejection)
BLOOM_SETS = [(0.6, 0.2, 0.5, 0.4, 1.0), (0.05, 2.0, 0.0, 1.0, 0.4), (1.0, 0.0, 1.0, 0.55, 0.9)]  # (intensity, threshold, soft threshold, radius, alpha)
TONEMAP_SETS = [(0, 0.18, 3.0, 1.0, 0.3), (1, 0.4, 1.5, 0.6, 0.05), (1, 0.09, 8.0, 1.7, 4.0)]  # (auto exposure, middle gray, white point, luminance saturation, ave log lum)
TONEMAP_AGX = (1.2, 0.9, 1.1, 0.02)  # AgX saturation, slope, power, offset of every tone-map row
DOF_SETS = [(0.005, 0.5, 3, 3, 1.0), (0.035, 0.99, 4, 5, 0.3), (0.015, 0.8, 2, 7, 0.65)]  # (max CoC, temporal, rings, density, alpha)
DOF_LENS = (12.0, 1.2, 135.0)  # fFocusDistance, fFStop, fFocalLength of the camera in a frame with depth of field (tests/test_gpu_sharded.py)


def tonemap_bytes(mode, row):
    """The ToneMappingAttribs block of a TONEMAP_SETS row (ToneMappingStructures.fxh:24-52)."""
    auto_exposure, middle_gray, white_point, lum_sat, _ = row
    return struct.pack("<iififfIIffff", mode, auto_exposure, middle_gray, 1, white_point, lum_sat, 0, 0, *TONEMAP_AGX)


def ssao_attribs(row):
    from diligentfx_amd.binding import SSAOAttribs

    algo, radius, falloff, mult, mipoff, temporal, spatial, thick = row
    a = SSAOAttribs.default()
    a.EffectRadius, a.EffectFalloffRange, a.RadiusMultiplier, a.DepthMIPSamplingOffset = radius, falloff, mult, mipoff
    a.TemporalStabilityFactor, a.SpatialReconstructionRadius, a.BitmaskThickness = temporal, spatial, thick
    a.Algorithm = {"gtao": 0, "hbao": 1, "vbao": 2}[algo]
    a.AlphaInterpolation = 0.7
    return a


def ssr_attribs(row):
    from diligentfx_amd.binding import SSRAttribs

    thick, thresh, mdm, perceptual, channel, trav, bias, radius, trad, tvar, sigma = row
    a = SSRAttribs.default()
    a.DepthBufferThickness, a.RoughnessThreshold, a.MostDetailedMip, a.IsRoughnessPerceptual, a.RoughnessChannel = thick, thresh, mdm, perceptual, channel
    a.MaxTraversalIntersections, a.GGXImportanceSampleBias, a.SpatialReconstructionRadius = trav, bias, radius
    a.TemporalRadianceStabilityFactor, a.TemporalVarianceStabilityFactor, a.BilateralCleanupSpatialSigmaFactor = trad, tvar, sigma
    a.AlphaInterpolation = 0.6
    return a


def taa_attribs(row):
    from diligentfx_amd.binding import TAAAttribs

    a = TAAAttribs.default()
    _, a.TemporalStabilityFactor, a.SkipRejection = row
    return a


def bloom_attribs(row):
    from diligentfx_amd.binding import BloomAttribs

    a = BloomAttribs.default()
    a.Intensity, a.Threshold, a.SoftTreshold, a.Radius, a.AlphaInterpolation = row
    return a


def dof_attribs(row):
    from diligentfx_amd.binding import DOFAttribs

    a = DOFAttribs.default()
    a.MaxCircleOfConfusion, a.TemporalStabilityFactor, a.BokehKernelRingCount, a.BokehKernelRingDensity, a.AlphaInterpolation = row
    return a


def tone_mapping(mode, row):
    from diligentfx_amd.binding import ToneMappingAttribs

    return ToneMappingAttribs.from_buffer_copy(tonemap_bytes(mode, row))


# The chain-wide sets.  Every attribute that sizes a row window of the sharded frame stands once below and once above its default: SSAO SpatialReconstructionRadius 2.0 /
# 6.0 (and the fractional 5.5), SSR SpatialReconstructionRadius 1.0 / 6.0, Bloom Radius 0.4 / 1.0 (and 0.55), depth-of-field MaxCircleOfConfusion 0.005 / 0.035.
#   narrow: every window below its default; SkipRejection with TAA flags 7; SSR / SSAO scales of the composite off 1
#   wide:   every window above its default, on half-resolution SSAO and SSR; roughness from channel 1, rays from mip 1; all Bloom levels
#   dof:    depth of field with flags 3 and a temporal stability of 0.99 on the widest circle of confusion; VBAO; linear roughness from channel 2, rays from mip 2;
#           the AgX operator with custom parameters (mode 9, the one that reads the four AgX fields)
# "ssao" / "ssr" / "taa" / "bloom" / "dof": index of the row above; "tone": (mode, TONEMAP_SETS row, CONVERT_OUTPUT_TO_SRGB); "half": HALF_RESOLUTION of SSAO and SSR
SETS = {
    "narrow": {"ssao": 0, "ssr": 3, "taa": 6, "bloom": 0, "tone": (7, 1, 0), "dof": 0, "dof_flags": 3, "half": False, "ssr_scale": 0.6, "ssao_scale": 0.35},
    "wide": {"ssao": 1, "ssr": 1, "taa": 3, "bloom": 1, "tone": (10, 2, 1), "dof": None, "dof_flags": 0, "half": True, "ssr_scale": 1.0, "ssao_scale": 1.0},
    "dof": {"ssao": 5, "ssr": 2, "taa": 4, "bloom": 2, "tone": (9, 1, 1), "dof": 1, "dof_flags": 3, "half": False, "ssr_scale": 1.0, "ssao_scale": 1.0},
}
NAMES = tuple(SETS)


def blocks(name):
    """The attribute blocks of a set: a dict with ssao_attribs, ssr_attribs, taa_attribs, bloom_attribs, tone_mapping, tonemap_flags, ave_log_lum, ssr_scale, ssao_scale,
    taa_flags, algorithm, half (bool), dof_attribs (or None), dof_flags."""
    s = SETS[name]
    mode, row, srgb = s["tone"]
    return {"ssao_attribs": ssao_attribs(SSAO_SETS[s["ssao"]]), "ssr_attribs": ssr_attribs(SSR_SETS[s["ssr"]]), "taa_attribs": taa_attribs(TAA_SETS[s["taa"]]),
            "bloom_attribs": bloom_attribs(BLOOM_SETS[s["bloom"]]), "tone_mapping": tone_mapping(mode, TONEMAP_SETS[row]), "tonemap_flags": srgb,
            "ave_log_lum": TONEMAP_SETS[row][4], "ssr_scale": s["ssr_scale"], "ssao_scale": s["ssao_scale"], "taa_flags": TAA_SETS[s["taa"]][0],
            "algorithm": SSAO_SETS[s["ssao"]][0], "half": s["half"], "dof_attribs": dof_attribs(DOF_SETS[s["dof"]]) if s["dof"] is not None else None,
            "dof_flags": s["dof_flags"]}


def apply(chain, name):
    """Puts the set on a chain object and returns its blocks.  api.Chain: the per-frame attribute fields bind_frame reads, the feature flags of its SSAO / SSR objects
    and depth of field.  The CPU chain (oracle/cpu_chain.py CpuChain): the same names as plain fields (chain_util.run_frame_inputs runs the frame from them).
    The frames of a run with a set go through frame(g, blocks) below (the lens of depth of field, the roughness in the channel the set reads)."""
    b = blocks(name)
    for k in ("ssao_attribs", "ssr_attribs", "taa_attribs", "bloom_attribs", "tone_mapping", "tonemap_flags", "ave_log_lum", "ssr_scale", "ssao_scale", "taa_flags"):
        setattr(chain, k, b[k])
    flags = 2 if b["half"] else 0
    if hasattr(chain, "set_effect_feature_flags"):
        chain.set_effect_feature_flags(ssao_feature_flags=flags, ssr_feature_flags=flags)
        chain.set_depth_of_field(b["dof_attribs"], b["dof_flags"])
    else:
        chain.algorithm, chain.ssao_flags, chain.ssr_flags = b["algorithm"], flags, flags
        chain.dof_attribs, chain.dof_flags = b["dof_attribs"], b["dof_flags"]
    return b


def frame(g, b):
    """A frame dict (synth.make_frame) made fit for the set with the blocks b, in place: prepare_frame below."""
    return prepare_frame(g, b["dof_attribs"] is not None, b["ssr_attribs"].RoughnessChannel)


def prepare_frame(g, dof, roughness_channel):
    """dof: the camera focused so that depth of field blurs the scene (DOF_LENS).  roughness_channel: the synthetic material plane is (roughness, metallic, 0, 0); a set
    that reads the roughness from channel 1 or 2 would find a mirror wherever there is a reflection, and SSR's reconstruction radius -- scaled by the roughness -- would be
    dead.  The roughness goes where the set reads it, as in the material plane of tests/test_oracle_attribs_vs_ref.py: copied into channel 1 (the shade takes it for the
    metallic factor there), squared into channel 2 (the sets that read channel 2 take it as linear roughness)."""
    if dof:
        g["camera"].fFocusDistance, g["camera"].fFStop, g["camera"].fFocalLength = DOF_LENS
    if roughness_channel == 1:
        g["material"][..., 1] = g["material"][..., 0]
    elif roughness_channel == 2:
        g["material"][..., 2] = g["material"][..., 0] ** 2
    return g
