"""Row-band sharding (diligentfx_amd/sharded.py): N ranks emulated in one process on one GPU -- one chain object per rank, the exchanges
done by copying rows between the ranks' planes exactly as the RCCL calls would.  The rows each rank produces must equal the unsharded
chain's output bit for bit, frame after frame (histories included), and the planes that feed the next frame must be exact on band + halo."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 640, 768
MAX_MOTION_ROWS = 12
# (world, width, height): equal bands; 600x750 has odd pyramid levels (375 rows at level 1): the per-level kernels and uneven Bloom ownership
# the last two: FEATURE_FLAG_HALF_RESOLUTION of SSAO and SSR inside the row-band phases (round 3), even and odd half sizes
# "ae": auto exposure on -- the low-resolution luminance rows are exchanged after phase 3, phase 4 reduces them and tone-maps
SHAPES = [(2, 640, 768, None, 0), (3, 640, 768, None, 0), (4, 512, 1536, None, 0), (2, 600, 750, None, 0), (3, 640, 768, (0, 330, 520, 768), 0),  # (uneven bands)
          (3, 640, 768, None, 2), (2, 600, 750, (0, 350, 750), 2), (3, 640, 768, None, "ae"), (2, 600, 750, (0, 350, 750), "ae"),
          (4, 640, 768, (0, 340, 372, 410, 768), 0),  # two bands of 32 / 38 rows: thinner than every history halo, ghost rows come from two ranks away
          (3, 640, 768, None, "dof"), (2, 600, 750, (0, 350, 750), "dof"),  # depth of field (temporal smoothing + Karis weights) between TAA and Bloom
          (3, 640, 768, (0, 330, 520, 768), "layers"),  # mifx_chain_set_material_layers: all five layers + two shadow-mapped lights in the shade and in the SSR hit fetch
          (3, 640, 768, (0, 376, 392, 768), 0),  # a band of 16 rows (the band setters take any non-empty band): its whole halo comes from its neighbours
          # the chain-wide attribute sets of tests/attrib_sets.py ("set NAME"): every attribute that sizes a row window below / above its default ("wide": on half resolution)
          (3, 640, 768, (0, 330, 520, 768), "set narrow"), (2, 600, 750, (0, 350, 750), "set wide"), (3, 640, 768, (0, 330, 520, 768), "set dof"),
          (3, 160, 192, (0, 70, 130, 192), "set narrow")]  # Bloom Radius 0.4 of 7 levels: a pyramid of two levels is not split (gather_level -1), both Bloom phases run it whole


class LocalComm:
    """The exchanges of sharded.py over the planes of all emulated ranks at once."""

    def __init__(self, sharded):
        self.sh = sharded
        self.n = len(sharded)

    def band(self, r):
        return self.sh[r].band

    def allgather_rows(self, name):
        planes = [s.chain.shard_plane(name) for s in self.sh]
        for r in range(self.n):
            b, e = self.band(r)
            for q in range(self.n):
                if q != r:
                    planes[q][b:e].copy_(planes[r][b:e])

    def gather_owned_rows(self, name, infos):
        planes = [s.chain.shard_plane(name) for s in self.sh]
        owned = [(i.own_begin, i.own_end) for i in infos]
        # the rows owned by the ranks must tile the level exactly
        assert owned[0][0] == 0 and owned[-1][1] == planes[0].shape[0] and all(owned[i][1] == owned[i + 1][0] for i in range(self.n - 1)), owned
        for r, (b, e) in enumerate(owned):
            for q in range(self.n):
                if q != r:
                    planes[q][b:e].copy_(planes[r][b:e])

    def gather_luminance_rows(self, infos):
        planes = [s.chain.shard_plane("ae_low_res") for s in self.sh]
        owned = [(i.ae_begin, i.ae_end) for i in infos]
        assert owned[0][0] == 0 and owned[-1][1] == 64 and all(owned[i][1] == owned[i + 1][0] for i in range(self.n - 1)), owned
        for r, (b, e) in enumerate(owned):
            for q in range(self.n):
                if q != r and e > b:
                    planes[q][b:e].copy_(planes[r][b:e])

    def exchange_halos(self, name, halos):
        planes = [s.chain.shard_plane(name) for s in self.sh]
        H = planes[0].shape[0]
        for q in range(self.n):
            b, e = self.band(q)
            h = halos[q]
            for lo, hi in ((max(b - h, 0), b), (e, min(e + h, H))):  # every ghost row from the rank that owns it (the neighbour, or the rank beyond a thin neighbour)
                for r in range(self.n):
                    rb, re = self.band(r)
                    s0, s1 = max(lo, rb), min(hi, re)
                    if r != q and s1 > s0:
                        planes[q][s0:s1].copy_(planes[r][s0:s1])


def history_mismatch(chain, ref_chain, info, b, e, H=H, W=W):
    """Names of the history planes of `chain` that differ from the unsharded chain's on the rows [b - halo, e + halo)."""
    from diligentfx_amd.sharded import HISTORY_PLANES

    bad = []
    for name, field in HISTORY_PLANES:
        halo = getattr(info, field)
        got, want = chain.shard_plane(name), ref_chain.shard_plane(name)
        lo, hi = max(b - halo, 0), min(e + halo, H)
        cols = W * (4 if name in ("taa_history", "ssr_history_radiance") else 1)  # the row padding up to the pitch is never written
        if not torch.equal(got[lo:hi, :cols], want[lo:hi, :cols]):
            bad.append(name)
    return bad


def bloom_is_unsplit(chain, W, H):
    """Bloom::ComputeMipCount for the chain's Radius at this size gives no level beyond the one the ranks would gather (level 1): every rank builds the pyramid whole."""
    import cpu_chain

    return int(np.float32(chain.bloom_attribs.Radius) * np.float32(cpu_chain.compute_mip_levels_count(W // 2, H // 2))) <= 2


def run_sharded_frame(sharded, comm, bounds, skip=(), unsplit_bloom=False, before_history_exchange=None):
    """unsplit_bloom: the caller expects a Bloom pyramid too short to split (every rank builds it whole: gather_level -1, nothing to gather).
    before_history_exchange: called with the infos when every phase has run and no ghost row of a history plane has been replaced yet."""
    from diligentfx_amd.sharded import HISTORY_PLANES

    for s, b in zip(sharded, bounds):
        s.phase(b, 0)
    for s, b in zip(sharded, bounds):
        s.phase(b, 1)
    for s, b in zip(sharded, bounds):
        s.phase(b, 2)
    infos = [s.chain.shard_info(b) for s, b in zip(sharded, bounds)]
    assert all((i.gather_level < 0) == unsplit_bloom for i in infos), [i.gather_level for i in infos]
    if "bloom" not in skip and not unsplit_bloom:
        comm.gather_owned_rows("bloom_gather", infos)
    for s, b in zip(sharded, bounds):
        s.phase(b, 3)
    if getattr(sharded[0].chain, "auto_exposure", False):
        if "luminance" not in skip:
            comm.gather_luminance_rows(infos)
        for s, b in zip(sharded, bounds):
            s.phase(b, 4)
    if before_history_exchange:
        before_history_exchange(infos)
    if "history" not in skip:
        for name, field in HISTORY_PLANES:
            common = max(getattr(i, field) for i in infos)  # both sides of an exchange move the same number of rows
            comm.exchange_halos(name, [common] * len(infos))
    return infos


@pytest.mark.parametrize("world,W,H,cuts,half", SHAPES)
def test_sharded_chain_equals_unsharded(mifx_lib, world, W, H, cuts, half):
    import chain_util
    from diligentfx_amd import api, synth
    from diligentfx_amd.sharded import ShardedChain
    from util import blue_noise_tables

    sobol, tile = blue_noise_tables()
    dev = torch.device("cuda", 0)
    scene = synth.Scene()
    ref_chain = api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(ref_chain.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32,
                             lut_samples=32, diffuse_samples=32, specular_samples=16)
    shade = chain_util.shade_attribs(len(ibl.pre) - 1)
    ranks = [api.Chain(0, sobol, tile) for _ in range(world)]
    attrib_set = half[4:] if str(half).startswith("set ") else None
    ae, dof, layers, half = half == "ae", half == "dof", half == "layers", 0 if half in ("ae", "dof", "layers") or attrib_set else half
    if layers:
        shade = chain_util.shadowed_shade_attribs(len(ibl.pre) - 1)
        slices, infos_np = chain_util.make_shadow_inputs()
        shadow_maps = torch.from_numpy(np.stack(slices)).to(dev)
    for c in ranks + [ref_chain]:
        if attrib_set:  # (feature flags and depth of field included)
            import attrib_sets

            blocks = attrib_sets.apply(c, attrib_set)
            continue
        c.set_effect_feature_flags(ssao_feature_flags=half, ssr_feature_flags=half)  # 2 = FEATURE_FLAG_HALF_RESOLUTION of both effects
        if ae:
            c.set_auto_exposure(True, elapsed_time_s=0.25)
        if dof:
            from diligentfx_amd import binding as B

            da = B.DOFAttribs.default()
            da.MaxCircleOfConfusion = 0.02
            c.set_depth_of_field(da, 3)
    sharded = [ShardedChain(c, H, r, world, MAX_MOTION_ROWS, cuts) for r, c in enumerate(ranks)]
    comm = LocalComm(sharded)
    out_ref = torch.zeros(H, W, 4, device=dev)
    outs = [torch.full((H, W, 4), -1.0, device=dev) for _ in range(world)]
    prev = None
    for fi in range(16, 22):
        g = synth.make_frame(scene, fi, W, H, dev)
        if dof:
            g["camera"].fFocusDistance, g["camera"].fFStop, g["camera"].fFocalLength = 12.0, 1.2, 135.0
        if attrib_set:
            attrib_sets.frame(g, blocks)
        if layers:  # new planes every frame, whole on every rank like the G-buffer
            from layers_util import IOR, ROTATION, make_layers

            planes, albedo, charlie = make_layers(g["normal"].cpu().numpy(), seed=fi)
            lp = {k: torch.from_numpy(v).to(dev) for k, v in planes.items()}
            lp["transmission"] = lp["transmission"][..., 0].contiguous()
            lp["sheen_albedo_scaling_lut"], lp["preintegrated_charlie"] = torch.from_numpy(albedo).to(dev), torch.from_numpy(charlie).to(dev)
            for c in ranks + [ref_chain]:
                c.set_material_layers(lp, 31, IOR, ROTATION, shadows=(shadow_maps, infos_np, 3))
        m = g["motion"]
        assert float(m[..., 1].abs().max()) * 0.5 * H < MAX_MOTION_ROWS, "the synthetic motion exceeds the declared reprojection reach"
        ref_chain.execute(ref_chain.bind_frame(fi, g, ibl, shade, out_ref))
        bounds = [c.bind_frame(fi, g, ibl, shade, o) for c, o in zip(ranks, outs)]
        infos = run_sharded_frame(sharded, comm, bounds, unsplit_bloom=bloom_is_unsplit(ref_chain, W, H))
        torch.cuda.synchronize()
        for r, s in enumerate(sharded):
            b, e = s.band
            same = torch.equal(outs[r][b:e], out_ref[b:e])
            if not same:
                d = (outs[r][b:e] != out_ref[b:e]).any(dim=-1).nonzero()
                rows = (d[:, 0] + b).unique()
                pytest.fail(f"frame {fi} rank {r}/{world}: {d.shape[0]} pixels differ, rows {rows[:12].tolist()} (band {b}..{e}, info "
                            f"{[(f, getattr(infos[r], f)) for f, _ in infos[r]._fields_]})")
            if ae:  # one average on every rank, the unsharded chain's to the bit
                assert s.chain.auto_exposure_average() == ref_chain.auto_exposure_average(), (fi, r)
            # the rank really worked on its band only: rows of the output outside the band were never written
            assert bool((outs[r][:b] == -1.0).all()) and bool((outs[r][e:] == -1.0).all())
            # what the next frame will read of the histories (band + halo) is exact
            bad = history_mismatch(s.chain, ref_chain, infos[r], b, e, H, W)
            assert not bad, f"frame {fi} rank {r}/{world}: history planes differ on band + halo: {bad}"
        prev = g
    assert prev is not None and np.isfinite(out_ref.cpu().numpy()).all()
    for c in ranks + [ref_chain]:
        c.close()


SWEEP = 32  # bands [H / 3 + k, 2 H / 3 + k), k = 0 .. 31: two whole periods of the 16-row alignment of SSAO's window on both edges


def shard_info_controls(dev, attrib_set, W, H, make_ibl, on_frame=None, on_chain=None):
    """Control of mifx_chain_get_shard_info at a set of tests/attrib_sets.py, one attribute at a time: the chain object with the whole set against a second one with the
    same set and ONE attribute back at its default, so that nothing else (depth of field above all, which widens every window) stands in the way, over SWEEP interior
    bands moved row by row -- SSAO's window is aligned to 16 rows, which takes up the 2 rows of the radius on most bands and not on all.
      SSAO SpatialReconstructionRadius -> halo_ssao: never on the other side of the default's, and beyond it on at least one band;
      depth of field                   -> halo_taa, halo_ssr, halo_ssao: larger on every band than without it;
      Bloom Radius                     -> gather_level -1 where the pyramid is too short to split (bloom_is_unsplit), against 1 at the default; otherwise neither the
                                          gathered level nor the rows a rank owns of it move -- they are functions of the band alone (mifx_bloom::make_plan) -- and that is held;
      SSR SpatialReconstructionRadius  -> nothing: R6 / R7 read a fixed number of rows (mifx_ssr::accum_rows), halo_ssr is the same with the default radius.
    (also run by tests/cpu_product/run.py `controls` on the CPU build of the host code)"""
    import attrib_sets
    import chain_util
    from diligentfx_amd import api, binding as B, synth
    from util import blue_noise_tables

    sobol, tile = blue_noise_tables()
    blocks = attrib_sets.blocks(attrib_set)
    variants = {"set": lambda c: None,
                "ssao radius": lambda c: setattr(c.ssao_attribs, "SpatialReconstructionRadius", B.SSAOAttribs.default().SpatialReconstructionRadius),
                "ssr radius": lambda c: setattr(c.ssr_attribs, "SpatialReconstructionRadius", B.SSRAttribs.default().SpatialReconstructionRadius),
                "bloom radius": lambda c: setattr(c.bloom_attribs, "Radius", B.BloomAttribs.default().Radius)}
    if blocks["dof_attribs"] is not None:
        variants["depth of field"] = lambda c: c.set_depth_of_field(None)
    g = attrib_sets.frame(synth.make_frame(synth.Scene(), 19, W, H, dev), blocks)
    if on_frame:
        on_frame(g)
    if on_chain:
        on_chain(blocks)
    out = torch.zeros(H, W, 4, device=dev)
    info, ibl = {}, None
    for name, reset in variants.items():
        c = api.Chain(0, sobol, tile)
        if ibl is None:
            ibl, n_pre = make_ibl(c)
            shade = chain_util.shade_attribs(n_pre - 1)
        attrib_sets.apply(c, attrib_set)
        reset(c)
        c.set_row_band(H // 3, 2 * H // 3, MAX_MOTION_ROWS)
        c.execute_phase(c.bind_frame(19, g, ibl, shade, out), 0)  # (mifx_chain_get_shard_info wants the frame's resources prepared)
        rows = []
        for k in range(SWEEP):
            c.set_row_band(H // 3 + k, 2 * H // 3 + k, MAX_MOTION_ROWS)
            rows.append(c.shard_info(c.bind_frame(19, g, ibl, shade, out)))
        info[name] = {f: [getattr(i, f) for i in rows] for f, _ in rows[0]._fields_}
        c.close()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    full = info["set"]
    plan = ("gather_level", "own_begin", "own_end")
    unsplit = bloom_is_unsplit(type("Set", (), blocks), W, H)
    print(f"set {attrib_set} {W}x{H}: gather_level {sorted(set(full['gather_level']))} | {sorted(set(info['bloom radius']['gather_level']))} at the default Bloom radius")
    if unsplit:  # every rank builds Bloom whole, so every window in front of it is the whole frame: only Bloom's own radius can show, and it does
        assert set(full["gather_level"]) == {-1} and set(info["bloom radius"]["gather_level"]) == {1}
        assert all(full == info[name] for name in info if name != "bloom radius")
        return
    assert set(full["gather_level"]) == {1} and all(full[f] == info["bloom radius"][f] for f in plan)
    # SSAO's radius
    radius, default = blocks["ssao_attribs"].SpatialReconstructionRadius, B.SSAOAttribs.default().SpatialReconstructionRadius
    sign = 1 if radius > default else -1
    diff = [sign * (a - b) for a, b in zip(full["halo_ssao"], info["ssao radius"]["halo_ssao"])]
    print(f"set {attrib_set} {W}x{H}: halo_ssao at radius {radius} minus at {default}, bands +0 .. +{SWEEP - 1}: {[sign * d for d in diff]}")
    assert min(diff) >= 0 and max(diff) > 0, (attrib_set, full["halo_ssao"], info["ssao radius"]["halo_ssao"])
    assert all(full[f] == info["ssao radius"][f] for f in full if f != "halo_ssao")
    # depth of field
    if "depth of field" in info:
        for f in ("halo_taa", "halo_ssr", "halo_ssao"):
            assert all(a > b for a, b in zip(full[f], info["depth of field"][f])), (attrib_set, f, full[f], info["depth of field"][f])
    # SSR's radius
    assert full == info["ssr radius"]


@pytest.mark.parametrize("attrib_set", ["narrow", "wide", "dof"])
def test_attribute_sets_move_every_effect_and_the_row_windows(mifx_lib, attrib_set):
    """Control of the cases "set NAME" above: a case must not pass because its attributes were dead.  On the unsharded chain the output of every effect (and the frame)
    differs from the default-attribute run of the same frames; SSR's resolve gathers taps (its reconstruction radius is scaled by the roughness: the roughness is
    where the set reads it).  mifx_shard_info follows the attributes that size a row window, one at a time: shard_info_controls, at the size of the set's case and --
    "narrow" -- at 160x192, where Bloom's pyramid is too short to split."""
    import attrib_sets
    import chain_util
    from diligentfx_amd import api, synth
    from util import blue_noise_tables

    world, W, H, cuts = next((s[0], s[1], s[2], s[3]) for s in SHAPES if s[4] == "set " + attrib_set)  # (the first case of the set: the sizes of the issue)
    sobol, tile = blue_noise_tables()
    dev = torch.device("cuda", 0)
    scene = synth.Scene()
    moved, plain = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(plain.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32,
                             lut_samples=32, diffuse_samples=32, specular_samples=16)
    shade = chain_util.shade_attribs(len(ibl.pre) - 1)
    blocks = attrib_sets.apply(moved, attrib_set)
    outs = {c: torch.zeros(H, W, 4, device=dev) for c in (moved, plain)}
    for fi in range(16, 19):
        g = attrib_sets.frame(synth.make_frame(scene, fi, W, H, dev), blocks)  # (both chains on the same planes: only the attributes differ)
        for c in (moved, plain):
            c.execute(c.bind_frame(fi, g, ibl, shade, outs[c]))
        torch.cuda.synchronize()
        assert not torch.equal(outs[moved], outs[plain]), fi
        for fx in ("ssao", "ssr", "taa", "bloom"):
            a, b = moved.effect_output(fx), plain.effect_output(fx)
            assert float((a != b).float().mean()) > 0.01, (fx, fi)
    if blocks["dof_attribs"] is not None:
        assert float((moved.effect_output("dof") != moved.effect_output("taa")).float().mean()) > 0.01
    # the roughness where the set reads it: reflecting texels with a roughness of 0.05 and more, whose resolve gathers taps over the set's radius
    rough, mask = moved.effect("ssr").get_intermediate("roughness"), moved.effect("ssr").get_intermediate("mask")
    assert float(((rough > 0.05) & (mask > 0)).float().mean()) > 0.01
    for c in (moved, plain):
        c.close()
    for w, h in [(W, H)] + ([(160, 192)] if attrib_set == "narrow" else []):
        shard_info_controls(dev, attrib_set, w, h, _band_ibl(dev))


@pytest.mark.parametrize("skip", ["bloom", "history", "luminance", "history at set wide"])
def test_every_exchange_is_needed(mifx_lib, skip):
    """Control: leaving out any one of the exchanges must change the result (otherwise the equality test above proves nothing).  "at set NAME": with that set of
    tests/attrib_sets.py on every chain object."""
    import chain_util
    from diligentfx_amd import api, synth
    from diligentfx_amd.sharded import ShardedChain
    from util import blue_noise_tables

    world = 2
    skip, _, attrib_set = skip.partition(" at set ")
    sobol, tile = blue_noise_tables()
    dev = torch.device("cuda", 0)
    scene = synth.Scene()
    ref_chain = api.Chain(0, sobol, tile)
    ibl = api.precompute_ibl(ref_chain.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32,
                             lut_samples=32, diffuse_samples=32, specular_samples=16)
    shade = chain_util.shade_attribs(len(ibl.pre) - 1)
    ranks = [api.Chain(0, sobol, tile) for _ in range(world)]
    if attrib_set:
        import attrib_sets

        for c in ranks + [ref_chain]:
            blocks = attrib_sets.apply(c, attrib_set)
    if skip == "luminance":
        for c in ranks + [ref_chain]:
            c.set_auto_exposure(True, elapsed_time_s=0.25)
    sharded = [ShardedChain(c, H, r, world, MAX_MOTION_ROWS) for r, c in enumerate(ranks)]
    comm = LocalComm(sharded)
    out_ref = torch.zeros(H, W, 4, device=dev)
    outs = [torch.full((H, W, 4), -1.0, device=dev) for _ in range(world)]
    differs = False
    for fi in range(16, 20):
        g = synth.make_frame(scene, fi, W, H, dev)
        if attrib_set:
            attrib_sets.frame(g, blocks)
        ref_chain.execute(ref_chain.bind_frame(fi, g, ibl, shade, out_ref))
        infos = run_sharded_frame(sharded, comm, [c.bind_frame(fi, g, ibl, shade, o) for c, o in zip(ranks, outs)], skip=(skip,))
        torch.cuda.synchronize()
        differs = differs or any(not torch.equal(outs[r][s.band[0]:s.band[1]], out_ref[s.band[0]:s.band[1]]) for r, s in enumerate(sharded))
        # (a missing history exchange reaches the band only after ghost / motion frames; the planes the next frame reads show it at once)
        differs = differs or any(history_mismatch(s.chain, ref_chain, infos[r], *s.band) for r, s in enumerate(sharded))
    assert differs, f"dropping the {skip} exchange went unnoticed"
    for c in ranks + [ref_chain]:
        c.close()



def band_against_phases(dev, overlap, ae, make_ibl, W=W, H=H, cuts=(0, 250, 520, H), on_frame=None, attrib_set=None, on_chain=None):
    """(also run by tests/cpu_product/run.py `band` on the CPU build of the host code)  attrib_set: a set of tests/attrib_sets.py on both chain objects; on_chain is then
    called with the set's blocks."""
    import os

    import chain_util
    from diligentfx_amd import api, synth
    from diligentfx_amd.sharded import HISTORY_PLANES, ShardedChain
    from util import blue_noise_tables

    sobol, tile = blue_noise_tables()
    scene = synth.Scene()
    a, b = api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)
    ibl, n_pre = make_ibl(a)
    shade = chain_util.shade_attribs(n_pre - 1)
    blocks = None
    for c in (a, b):
        if ae:
            c.set_auto_exposure(True, elapsed_time_s=0.25)
        if attrib_set:
            import attrib_sets

            blocks = attrib_sets.apply(c, attrib_set)
    if blocks is not None:
        if on_chain:
            on_chain(blocks)
        inner, on_frame = on_frame, lambda g: (attrib_sets.frame(g, blocks), inner(g) if inner else None)  # (the lens of depth of field, the roughness where the set reads it)
    # Two whole frames first, on both objects: without the exchanges the ghost rows and the other ranks' rows of the gathered Bloom level are never written, and a fresh
    # device allocation holds anything -- afterwards both objects hold the same values there (both slots of every history plane included).
    scratch = torch.zeros(H, W, 4, device=dev)
    for fi in (14, 15):
        g = synth.make_frame(scene, fi, W, H, dev)
        for c in (a, b):
            if on_frame:
                on_frame(g)
            c.execute(c.bind_frame(fi, g, ibl, shade, scratch))
    sa, sb = ShardedChain(a, H, 1, 3, MAX_MOTION_ROWS, cuts), ShardedChain(b, H, 1, 3, MAX_MOTION_ROWS, cuts)
    b.set_overlap(overlap)
    frames = [synth.make_frame(scene, fi, W, H, dev) for fi in range(16, 21)]
    outs_a = [torch.full((H, W, 4), -1.0, device=dev) for _ in frames]
    outs_b = [torch.full((H, W, 4), -1.0, device=dev) for _ in frames]
    for k, g in enumerate(frames):
        if on_frame:
            on_frame(g)
        bound = a.bind_frame(16 + k, g, ibl, shade, outs_a[k])
        for phase in range(ShardedChain.PHASES):
            sa.phase(bound, phase)
    bounds_b = [b.bind_frame(16 + k, g, ibl, shade, outs_b[k]) for k, g in enumerate(frames)]
    # Round 6: a rank of mifx_chain_execute_sharded prefilters only the rows of Bloom's level 0 it owns and receives the few rows beside its band's edges (csrc/api_comm.cpp,
    # mifx_bloom::halo_level0); the phases driven one by one have no such exchange and produce those rows themselves, so the row windows in front of Bloom differ by 9 rows.
    # The equality below is about the phase machinery and the lanes: with the switch off both sides compute the same windows.  (The exchange itself is held to the
    # unsharded frame by the group tests: test_comm.py, the in-process groups below, tests/cpu_product/run.py local_group.)
    before = os.environ.get("MIFX_SHARD_BLOOM_HALO")
    os.environ["MIFX_SHARD_BLOOM_HALO"] = "0"
    try:
        for g, bound in zip(frames, bounds_b):  # no synchronisation in between: the lanes of consecutive frames overlap
            if on_frame:
                on_frame(g)
            b.execute_band(bound)
    finally:
        if before is None:
            del os.environ["MIFX_SHARD_BLOOM_HALO"]
        else:
            os.environ["MIFX_SHARD_BLOOM_HALO"] = before
    if dev.type == "cuda":
        torch.cuda.synchronize()
    lo, hi = sb.band
    for k in range(len(frames)):
        assert torch.equal(outs_a[k][lo:hi], outs_b[k][lo:hi]), f"frame {k}: execute_band differs from the phases"
        assert bool((outs_b[k][:lo] == -1.0).all()) and bool((outs_b[k][hi:] == -1.0).all())
    for name, _ in HISTORY_PLANES:
        assert torch.equal(a.shard_plane(name), b.shard_plane(name)), name
    if ae:
        assert a.auto_exposure_average() == b.auto_exposure_average()
    for c in (a, b):
        c.close()


@pytest.mark.parametrize("overlap,ae,attrib_set", [(0, False, None), (2, False, None), (2, True, None), (3, False, None), (3, True, None), (3, True, "wide"), (2, False, "dof")],
                         ids=["0-False", "2-False", "2-True", "3-False", "3-True", "3-True-wide", "2-False-dof"])
def test_execute_band_is_the_phases_without_the_exchanges(mifx_lib, overlap, ae, attrib_set):
    """mifx_chain_execute_band (what tools/shard_cost.py and TiledChain.calibrate_cuts time): one rank's band through the phases -- and with overlap >= 2 the two lanes across
    frames -- of mifx_chain_execute_sharded, exchanges left out.  Against a second chain object on the same band driven phase by phase: the band's rows of every frame and all five
    history planes (whole: both hold the same stale ghost rows) are equal bit for bit, frames queued back to back.  "wide" / "dof": at those sets of tests/attrib_sets.py."""
    dev = torch.device("cuda", 0)
    band_against_phases(dev, overlap, ae, _band_ibl(dev), attrib_set=attrib_set)


@pytest.mark.parametrize("overlap,ae", [(0, False), (3, True)])
def test_execute_band_on_cuts_at_multiples_of_16(mifx_lib, overlap, ae):
    """test_execute_band_is_the_phases_without_the_exchanges with band cuts on multiples of 16 rows (0, 256, 512, 768): the rows a band's pyramid levels start on then fall
    on the levels' own block boundaries, which the cuts above (0, 250, 520, 768) never do."""
    dev = torch.device("cuda", 0)
    band_against_phases(dev, overlap, ae, _band_ibl(dev), cuts=(0, 256, 512, H))


def _band_ibl(dev):
    from diligentfx_amd import api, synth

    def make_ibl(chain):
        ibl = api.precompute_ibl(chain.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32,
                                 lut_samples=32, diffuse_samples=32, specular_samples=16)
        return ibl, len(ibl.pre)

    return make_ibl


def test_empty_row_band_is_refused(mifx_lib):
    """The thinnest band the chain takes is one row (tests above: 16); an empty or inverted band is a clean INVALID_ARG, before any launch."""
    from diligentfx_amd import api, binding as B
    from util import blue_noise_tables

    sobol, tile = blue_noise_tables()
    c = api.Chain(0, sobol, tile)
    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        c.set_row_band(40, 39, MAX_MOTION_ROWS)
    with pytest.raises(B.MifxError, match="INVALID_ARG"):
        c.set_row_band(-1, 16, MAX_MOTION_ROWS)
    c.close()


def _fake_rccl(tmp_path):
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = "/opt/rocm"
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "rccl", "rccl.h")):
        pytest.skip("g++ or the RCCL headers are missing")
    fake = tmp_path / "librccl_fake.so"
    r = subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "fake_rccl", "fake_rccl.cpp"),
                        "-o", str(fake), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lrt", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return root, str(fake)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["selftest", "selftest_absent", "selftest_mismatch"])
def test_comm_self_test_and_its_error_paths(tmp_path, mifx_lib, mode):
    """mifx_comm_self_test over the RCCL branch with three processes (the stand-in transport): all ranks -> every rank verifies the slabs of both peers; a rank that never
    posts -> the others get MIFX_ERR_COMM with the transport's message instead of a hang; a rank that announces another slab size -> its peers are told so.  What
    bench.py --gpus N runs before it trusts the communicator with a frame."""
    import os
    import subprocess
    import sys

    root, fake = _fake_rccl(tmp_path)
    env = dict(os.environ, MIFX_RCCL_PATH=fake, HSA_ENABLE_IPC_MODE_LEGACY="0", MIFX_FAKE_RCCL_TIMEOUT="3")
    idfile, world = str(tmp_path / "unique_id"), 3
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "rccl_branch_worker.py"), str(k), str(world), idfile, "64", "64", "0", mode], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for k in range(world)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=180)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for k, (rc, o, e) in enumerate(outs):
        assert rc == 0, (k, rc, o[-3000:], e[-1200:])
        if mode == "selftest":
            assert "self test OK" in o, (k, o, e[-800:])
        elif mode == "selftest_absent":
            assert ("stayed away" in o) if k == world - 1 else ("self test FAILED" in o and "MIFX_ERR_COMM" in o), (k, o, e[-800:])
        else:  # rank 0 sends 4096 bytes where 8192 are expected, and expects 4096 where 8192 arrive: every rank that talks to it is refused
            assert "self test FAILED" in o and "MIFX_ERR_COMM" in o, (k, o, e[-800:])

@pytest.mark.parametrize("world,W,H,lanes", [(2, 640, 768, 2), (2, 640, 768, 3), (4, 640, 768, 3), (8, 512, 1536, 2)])
def test_rccl_branch_with_several_processes(tmp_path, mifx_lib, world, W, H, lanes):
    """The RCCL branch of mifx_chain_execute_sharded (csrc/api_comm.cpp: ncclCommInitRank, grouped ncclSend / ncclRecv) with N > 1 ranks: N processes on this one GPU,
    each joining the communicator through mifx_comm_create and running its band; RCCL itself refuses two ranks on one device, so the library loads the stand-in of
    tests/fake_rccl (hipIpc + a shared-memory mailbox behind the same eight entry points) through MIFX_RCCL_PATH.  Every rank compares its band of every frame and its
    history planes on band + halo with the unsharded chain, bit for bit (tests/rccl_branch_worker.py)."""
    import os
    import shutil
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = "/opt/rocm"
    if shutil.which("g++") is None or not os.path.exists(os.path.join(rocm, "include", "rccl", "rccl.h")):
        pytest.skip("g++ or the RCCL headers are missing")
    fake = tmp_path / "librccl_fake.so"
    r = subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), os.path.join(root, "tests", "fake_rccl", "fake_rccl.cpp"),
                        "-o", str(fake), "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lrt", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, MIFX_RCCL_PATH=str(fake), HSA_ENABLE_IPC_MODE_LEGACY="0", MIFX_SHARD_OVERLAP=str(lanes))  # (mifx_chain_set_overlap of every rank's chain: two or three lanes)
    idfile = str(tmp_path / "unique_id")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "rccl_branch_worker.py"), str(k), str(world), idfile, str(W), str(H), "3"], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for k in range(world)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=240)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for k, (rc, o, e) in enumerate(outs):
        assert rc == 0 and "bit-identical to the unsharded chain" in o and "is_rccl 1" in o, (k, rc, o[-3000:], e[-1200:])
