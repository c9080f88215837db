"""R4 clears its two targets only where an 8x8 tile needs it (csrc/ssr_trace.hip "clean tiles"): bit identity with the march that always clears.

Two ScreenSpaceReflection objects on one PostFXContext are fed the same inputs frame by frame: `ref` with the switch off (mifx_debug_ssr_set_clean_tiles 0: every texel
outside the reflection mask gets its zeros every frame, the behaviour before the tile words existed) and `dut` as created.  After every frame both ray planes, R5's three
targets, the current history slot and the output are compared bit for bit (as integers: no tolerance, NaN-safe), and the tile words of `dut` are read back and held to their
invariant: word 0 => every texel of the tile, inside the plane, is 0 in both ray planes.  The reflection mask is steered through the roughness channel of the material
(the depth is kept off the far plane, so the roughness alone decides)."""
import pytest
import torch

from util import blue_noise_tables

pytestmark = pytest.mark.gpu

ROUGH_OUT, ROUGH_IN = 0.8, 0.05  # RoughnessThreshold is 0.2
PLANES = ("ray_radiance", "ray_dir_pdf", "res_radiance", "res_variance", "res_depth", "hist_radiance", "hist_variance")
# a block of reflective texels that shifts by 3 pixels per frame (tiles go clean -> dirty -> clean, some partly masked), an empty and a full mask and per-pixel noise in between
SEQUENCE = ("move0", "move1", "move2", "zero", "move3", "one", "move4", "random", "move5", "zero", "random")


def bits(t):
    return t.contiguous().view(torch.int32)


def tile_any(b):
    """(h, w) bool -> (ceil(h / 8), ceil(w / 8)) bool: the 8x8 tile, within the plane, holds a True."""
    h, w = b.shape
    p = torch.zeros((h + 7) // 8 * 8, (w + 7) // 8 * 8, dtype=torch.bool, device=b.device)
    p[:h, :w] = b
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).permute(0, 2, 1, 3).reshape(p.shape[0] // 8, p.shape[1] // 8, 64).any(-1)


def roughness(kind, w, h, dev):
    r = torch.full((h, w), ROUGH_OUT, device=dev)
    if kind.startswith("move"):
        t = int(kind[4:])
        x0, y0, bw, bh = 2 + 3 * t, 1, max(2, w // 4), max(2, h // 2)
        r[y0:y0 + bh, x0:x0 + bw] = ROUGH_IN
    elif kind == "one":
        r[...] = ROUGH_IN
    elif kind == "random":
        g = torch.Generator(device="cpu").manual_seed(w * 1000 + h)
        r = (0.2 + 0.2 * (torch.rand(h, w, generator=g) - 0.5)).to(dev)
    return r


class Pair:
    def __init__(self):
        from diligentfx_amd import api, binding as B, synth

        sobol, tile = blue_noise_tables()
        self.api, self.synth = api, synth
        self.ctx = api.PostFXContext(0, sobol, tile)
        self.ref, self.dut = api.ScreenSpaceReflection(self.ctx), api.ScreenSpaceReflection(self.ctx)
        self.ref.set_clean_tiles(False)
        self.attribs = B.SSRAttribs.default()
        self.scene = synth.Scene()
        self.index = 0
        self.mask_tiles = []  # per frame: which tiles hold a texel of the mask R4 ran under

    def frame(self, kind, w, h, flags=0, what="", switched_off=False):
        """One frame through both objects; compares everything and checks the tile words (switched_off: `dut` always clears as well, its words are stale and must say so).
        Returns the tile words of `dut`."""
        dev = self.ctx.device
        f = self.synth.make_frame(self.scene, self.index, w, h, dev)
        depth, prev_depth = f["depth"].clamp(max=0.9995).contiguous(), f["prev_depth"].clamp(max=0.9995).contiguous()
        material = f["material"].clone()
        material[..., 0] = roughness(kind, w, h, dev)
        color = (f["base_color"] * (0.5 + f["normal"][..., 1:2].clamp(0, 1)) + 0.05).contiguous()
        self.ctx.prepare_resources(self.index, w, h)
        for fx in (self.ref, self.dut):
            fx.prepare_resources(feature_flags=flags)
        self.ctx.execute(depth, prev_depth, f["motion"], f["camera"], f["prev_camera"])
        for fx in (self.ref, self.dut):
            fx.execute(color, depth, f["normal"], material, f["motion"], self.attribs)
        self.index += 1
        where = f"{what} frame {self.index - 1} ({kind}, {w}x{h}, flags {flags})"
        for name in PLANES:
            a, b = self.ref.get_intermediate(name), self.dut.get_intermediate(name)
            assert torch.equal(bits(a), bits(b)), f"{where}: {name} differs in {int((bits(a) != bits(b)).sum())} values"
        assert torch.equal(bits(self.ref.get_ssr_radiance()), bits(self.dut.get_ssr_radiance())), f"{where}: output differs"
        # the invariant itself
        words, valid = self.dut.get_tile_flags()
        if switched_off:
            assert not valid, f"{where}: the words count as valid while the march always clears"
            return words
        rr, rd = self.dut.get_intermediate("ray_radiance"), self.dut.get_intermediate("ray_dir_pdf")
        dirty = tile_any(((bits(rr) != 0) | (bits(rd) != 0)).any(-1)).cpu()
        assert words.shape == dirty.shape and valid, f"{where}: {tuple(words.shape)} words for {tuple(dirty.shape)} tiles, valid={valid}"
        assert not bool((dirty & (words == 0)).any()), f"{where}: {int((dirty & (words == 0)).sum())} tiles are marked clean and hold non-zero texels"
        # ... and no word stays set over a tile without a mask texel (a march that never skips would satisfy the invariant too)
        mask = self.ref.get_intermediate("mask_half" if flags & 2 else "mask") != 0
        assert mask.shape == rr.shape[:2]
        mt = tile_any(mask).cpu()
        assert not bool(((words != 0) & ~mt).any()), f"{where}: words set over tiles outside the mask"
        assert not self.ref.get_tile_flags()[1], "the object that always clears claims valid words"
        self.mask_tiles.append(mt)
        return words

    def close(self):
        for o in (self.ref, self.dut, self.ctx):
            o.close()


def run_sequence(w, h, flags=0):
    p = Pair()
    partly = False
    for kind in SEQUENCE:
        p.frame(kind, w, h, flags)
        m = p.ref.get_intermediate("mask_half" if flags & 2 else "mask") != 0
        partly = partly or bool((tile_any(m) & tile_any(~m)).any())
    # not vacuous: some tile was dirty, then wholly outside the mask -- the march had to clear it -- and then stayed outside (nothing to store); a tile was partly masked
    t = p.mask_tiles
    assert any(bool((t[i - 1] & ~t[i]).any()) for i in range(1, len(t))), "no tile went dirty -> clean"
    assert any(bool((~t[i - 1] & t[i]).any()) for i in range(1, len(t))), "no tile went clean -> dirty"
    assert any(bool((~t[i - 1] & ~t[i]).any()) for i in range(1, len(t))) or t[0].numel() == 1, "no tile stayed clean"
    assert partly, "no partly masked tile"
    p.close()


@pytest.mark.parametrize("size", [(67, 45), (40, 24), (5, 3)])
def test_clean_tiles_bit_identical_under_a_moving_mask(mifx_lib, size):
    """Edge tiles in both directions (67x45), in none (40x24), a plane smaller than one tile (5x3)."""
    run_sequence(*size)


@pytest.mark.parametrize("flags", [1, 2, 3])
def test_clean_tiles_ray_permutations(mifx_lib, flags):
    """FEATURE_FLAG_PREVIOUS_FRAME (1), the half-resolution ray pass (2: 20x12 ray planes under the half-size mask) and both."""
    run_sequence(40, 24, flags)


def test_clean_tiles_survive_what_invalidates_them(mifx_lib):
    """In the middle of a sequence: a history reset, a prepare that toggles half resolution and back, a frame size change and back, the switch itself -- the whole-plane frame
    after each is compared like every other."""
    p = Pair()
    w, h = 40, 24
    for kind in ("move0", "zero", "move1"):
        p.frame(kind, w, h)
    for fx in (p.ref, p.dut):
        fx.reset_history()
    p.frame("zero", w, h, what="after reset_history")
    p.frame("move2", w, h)
    p.frame("one", w, h, flags=2, what="half resolution on")
    p.frame("zero", w, h, flags=2)
    p.frame("zero", w, h, what="half resolution off")  # new planes, nothing inside the mask: every texel must still be cleared
    p.frame("move3", w, h)
    p.frame("one", 67, 45, what="another size")
    p.frame("zero", w, h, what="the size back")
    p.frame("move4", w, h)
    p.dut.set_clean_tiles(False)
    p.frame("zero", w, h, what="switch off", switched_off=True)
    p.frame("random", w, h, what="switch off", switched_off=True)
    p.dut.set_clean_tiles(True)
    p.frame("zero", w, h, what="switch on again")
    p.frame("move5", w, h)
    p.close()


def test_clean_tiles_really_skip_and_really_rebuild(mifx_lib):
    """The stores are gone where the words say clean, and only there: sentinels written into the ray planes of `dut` behind its back survive a frame whose mask is empty
    (nothing was stored), and are cleared by the frame after the words were declared stale (mifx_debug_ssr_set_clean_tiles)."""
    p = Pair()
    w, h = 40, 24
    p.frame("move0", w, h)
    words = p.frame("zero", w, h)
    assert not bool(words.any())
    rr, rd = p.dut.get_intermediate("ray_radiance"), p.dut.get_intermediate("ray_dir_pdf")
    rr.fill_(7.0)
    rd.fill_(-3.0)
    with pytest.raises(AssertionError, match="ray_radiance differs"):
        p.frame("zero", w, h)  # trusted: not one store
    assert bool((rr == 7.0).all()) and bool((rd == -3.0).all())
    p.dut.set_clean_tiles(True)  # "the words are stale"
    p.frame("zero", w, h)  # rebuilt: everything cleared and compared
    assert not bool(rr.any()) and not bool(rd.any())
    p.close()


def test_clean_tiles_after_a_row_band_frame_of_the_chain(mifx_lib):
    """A row-band execute of the chain (mifx_chain_execute_band: R4 over a row window, the sharded hit fetch behind it) writes the ray planes without the words: the whole
    frames after it are compared between a chain whose SSR object always clears and one as created -- the frame itself, the ray planes, the words' invariant."""
    import chain_util
    from diligentfx_amd import api, synth

    dev = torch.device("cuda", 0)
    sobol, tile = blue_noise_tables()
    W, H = 320, 384
    scene = synth.Scene()
    chains = [api.Chain(0, sobol, tile), api.Chain(0, sobol, tile)]
    chains[0].effect("ssr").set_clean_tiles(False)
    ibls = [api.precompute_ibl(c.postfx, synth.make_sky_cube(32, dev).clamp(max=200.0), lut_size=32, irradiance_size=8, prefiltered_size=32, lut_samples=32, diffuse_samples=32,
                               specular_samples=16) for c in chains]
    shade = chain_util.shade_attribs(len(ibls[0].pre) - 1)
    outs = [torch.zeros(H, W, 4, device=dev) for _ in chains]

    def whole(fi):
        g = synth.make_frame(scene, fi, W, H, dev)
        for c, ibl, o in zip(chains, ibls, outs):
            c.execute(c.bind_frame(fi, g, ibl, shade, o))
        torch.cuda.synchronize()
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"frame {fi}: the chains' frames differ"
        a, b = chains[0].effect("ssr"), chains[1].effect("ssr")
        for name in ("ray_radiance", "ray_dir_pdf", "hist_radiance", "hist_variance"):
            assert torch.equal(bits(a.get_intermediate(name)), bits(b.get_intermediate(name))), f"frame {fi}: {name}"
        words, valid = b.get_tile_flags()
        dirty = tile_any(((bits(b.get_intermediate("ray_radiance")) != 0) | (bits(b.get_intermediate("ray_dir_pdf")) != 0)).any(-1)).cpu()
        assert valid and not bool((dirty & (words == 0)).any()) and bool((words == 0).any()), f"frame {fi}"

    for fi in (14, 15, 16):
        whole(fi)
    g = synth.make_frame(scene, 17, W, H, dev)
    for c, ibl, o in zip(chains, ibls, outs):
        c.set_row_band(128, 256, 12)
        c.execute_band(c.bind_frame(17, g, ibl, shade, o))
        c.set_row_band(0, 0, 0)
    torch.cuda.synchronize()
    assert not chains[1].effect("ssr").get_tile_flags()[1], "the words still count as valid after a row-band frame"
    for fi in (18, 19):
        whole(fi)
    for c in chains:
        c.close()
