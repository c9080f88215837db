"""Coverage guard (no GPU): every field of the attribute structs of diligentfx_amd/binding.py that a chain frame carries -- SSAO, SSR, TAA, Bloom, depth of field,
tone mapping -- is moved off the struct's default() by at least one chain-wide set of tests/attrib_sets.py, or is listed below with the reason it is not.  The equivalence
tests (fusion switches, stream modes, row bands, execute_band) run at those sets, so a field added to a struct fails here until a set moves it.  Also the rules the sets
are composed by: the attributes that size a row window stand below and above their defaults, with a fractional value among them."""
import math

import attrib_sets as A
from diligentfx_amd import binding as B

# struct -> key of attrib_sets.blocks() that holds it
STRUCTS = {B.SSAOAttribs: "ssao_attribs", B.SSRAttribs: "ssr_attribs", B.TAAAttribs: "taa_attribs", B.BloomAttribs: "bloom_attribs", B.DOFAttribs: "dof_attribs",
           B.ToneMappingAttribs: "tone_mapping"}

# (struct name, field) -> why no set moves it
EXCLUDED = {
    ("SSAOAttribs", "ResetAccumulation"): "a one-off request: set on every frame it would leave the temporal passes without a history; tests/test_gpu_host_sequence.py drives it",
    ("SSAOAttribs", "Padding0"): "padding", ("SSAOAttribs", "Padding1"): "padding",
    ("TAAAttribs", "ResetAccumulation"): "a one-off request, as SSAO's; tests/test_gpu_host_sequence.py drives it",
    ("TAAAttribs", "Padding0"): "padding",
    ("BloomAttribs", "Padding0"): "padding", ("BloomAttribs", "Padding1"): "padding", ("BloomAttribs", "Padding2"): "padding",
    ("DOFAttribs", "Padding0"): "padding", ("DOFAttribs", "Padding1"): "padding", ("DOFAttribs", "Padding2"): "padding",
    ("ToneMappingAttribs", "bAutoExposure"): "neither the reference's tone-map shader nor this library reads it (a shader macro of the reference's epipolar light scattering); "
                                            "the chain's auto exposure is mifx_chain_set_auto_exposure",
    ("ToneMappingAttribs", "bLightAdaptation"): "as bAutoExposure: the chain takes it as an argument of mifx_chain_set_auto_exposure",
    ("ToneMappingAttribs", "Padding0"): "padding", ("ToneMappingAttribs", "Padding1"): "padding",
}


def _value(x):
    return list(x) if hasattr(x, "__len__") else x


def test_every_attribute_field_is_moved_by_a_set():
    all_blocks = [A.blocks(n) for n in A.NAMES]
    fields = set()
    for cls, key in STRUCTS.items():
        default = cls.default()
        for field, _ in cls._fields_:
            fields.add((cls.__name__, field))
            moved = any(b[key] is not None and _value(getattr(b[key], field)) != _value(getattr(default, field)) for b in all_blocks)
            if (cls.__name__, field) in EXCLUDED:
                assert not moved, f"{cls.__name__}.{field} is moved by a set and excluded as well"
            else:
                assert moved, f"{cls.__name__}.{field}: no set of tests/attrib_sets.py moves it off the default (move it in a set, or add it to EXCLUDED with the reason)"
    assert set(EXCLUDED) <= fields, f"stale exclusions: {sorted(set(EXCLUDED) - fields)}"


def test_the_sets_follow_their_rules():
    """What the issue of the sets asks of the table."""
    blocks = {n: A.blocks(n) for n in A.NAMES}
    assert len(blocks) == 3

    def values(key, field):
        return [getattr(b[key], field) for b in blocks.values() if b[key] is not None]

    # every attribute that sizes a row window: once below, once above its default
    for cls, key, field, lo, hi in ((B.SSAOAttribs, "ssao_attribs", "SpatialReconstructionRadius", 2.0, 6.0), (B.SSRAttribs, "ssr_attribs", "SpatialReconstructionRadius", 1.0, 6.0),
                                    (B.BloomAttribs, "bloom_attribs", "Radius", 0.4, 1.0), (B.DOFAttribs, "dof_attribs", "MaxCircleOfConfusion", 0.005, 0.035)):
        v, d = values(key, field), getattr(cls.default(), field)
        assert any(math.isclose(x, lo, rel_tol=1e-6) for x in v) and any(math.isclose(x, hi, rel_tol=1e-6) for x in v) and lo < d < hi, (field, v, d)
    # a fractional value where a window takes a ceil: the reconstruction radius itself, and Bloom's level count Radius x levels
    assert any(x != math.floor(x) for x in values("ssao_attribs", "SpatialReconstructionRadius"))
    assert any((x * 9) != math.floor(x * 9) for x in values("bloom_attribs", "Radius"))
    assert any(b["taa_attribs"].SkipRejection == 1 and b["taa_flags"] != 0 for b in blocks.values())
    d = B.SSRAttribs.default()
    assert any((b["ssr_attribs"].RoughnessChannel != d.RoughnessChannel or b["ssr_attribs"].IsRoughnessPerceptual != d.IsRoughnessPerceptual) and b["ssr_attribs"].MostDetailedMip in (1, 2)
               for b in blocks.values())
    assert any(b["algorithm"] in ("hbao", "vbao") for b in blocks.values())
    t = B.ToneMappingAttribs.default(4)
    for n, b in blocks.items():
        m = b["tone_mapping"]
        assert m.iToneMappingMode != 4 and m.fMiddleGray != t.fMiddleGray and m.fWhitePoint != t.fWhitePoint and m.fLuminanceSaturation != t.fLuminanceSaturation, n
        assert b["taa_flags"] != 2 or b["taa_attribs"].SkipRejection, n  # (the chain's default TAA flags are 2)
    assert any(b["tonemap_flags"] == 1 for b in blocks.values()) and any(b["tonemap_flags"] == 0 for b in blocks.values())
    assert any(math.isclose(b["ssr_scale"], 0.6) and math.isclose(b["ssao_scale"], 0.35) for b in blocks.values())
    assert any(b["dof_attribs"] is not None and b["dof_flags"] == 3 and math.isclose(b["dof_attribs"].TemporalStabilityFactor, 0.99, rel_tol=1e-6) for b in blocks.values())
    assert any(b["half"] and math.isclose(b["ssr_attribs"].SpatialReconstructionRadius, 6.0) for b in blocks.values())


def test_the_sets_are_made_of_rows_the_checker_is_pinned_on():
    """tests/test_oracle_attribs_vs_ref.py parametrises over the very lists the sets index."""
    import test_oracle_attribs_vs_ref as T

    assert T.SSAO_SETS is A.SSAO_SETS and T.SSR_SETS is A.SSR_SETS and T.TAA_SETS is A.TAA_SETS and T.BLOOM_SETS is A.BLOOM_SETS
    assert T.TONEMAP_SETS is A.TONEMAP_SETS and T.DOF_SETS is A.DOF_SETS
    for s in A.SETS.values():
        assert 0 <= s["ssao"] < len(A.SSAO_SETS) and 0 <= s["ssr"] < len(A.SSR_SETS) and 0 <= s["taa"] < len(A.TAA_SETS) and 0 <= s["bloom"] < len(A.BLOOM_SETS)
        assert 0 <= s["tone"][1] < len(A.TONEMAP_SETS) and 0 <= s["tone"][0] < 12 and (s["dof"] is None or 0 <= s["dof"] < len(A.DOF_SETS))
