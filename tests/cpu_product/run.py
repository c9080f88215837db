"""TEST INFRASTRUCTURE ONLY.  Runs scenarios of the DEVICE tests (tests/test_gpu_host_sequence.py: the effect objects driven through the C ABI, compared with oracle/cpu_chain.py)
on the CPU build of the product's host code (tests/cpu_product/build.py) with the reference's shaders standing in for the kernels (tests/cpu_product/device.py).

    MIFX_LIB_PATH=tests/cpu_product/_build/libmifx_cpu.so python tests/cpu_product/run.py scenarios | dof | chain | random FIRST LAST | chain_random FIRST LAST | order | order_features [PART] | feature_values [PART] | trace [PART OF A NAME] | lane_errors | ...

(started by tests/test_cpu_product.py in a process of its own: the Python mirror diligentfx_amd/api.py is used as it is, with three of its device plumbing points replaced
here -- the stream handle, the device of the tensors, the view of an effect-owned plane -- so that torch CPU tensors stand for device memory.)"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE]

import numpy as np  # noqa: E402
import torch  # noqa: E402

assert os.environ.get("MIFX_LIB_PATH", "").endswith("libmifx_cpu.so"), "run with MIFX_LIB_PATH pointing at tests/cpu_product/_build/libmifx_cpu.so"

import device as cpu_device  # noqa: E402
import pyref  # noqa: E402
from diligentfx_amd import api, binding as B  # noqa: E402


def install():
    lib = B.load()
    ref = pyref.ref_lib()
    assert ref is not None, "oracle/_ref is needed"
    dev = cpu_device.Device(ref, "ref_")
    cb_type = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(cpu_device.Call))
    cb = cb_type(dev.launch)
    lib.mifx_cpu_set_launch_callback(cb)
    dev._keep = cb
    # ---- the three plumbing points of api.py
    api._stream_ptr = lambda device: ctypes.c_void_p(0)
    torch.cuda.synchronize = lambda *a, **k: None
    init = api.PostFXContext.__init__

    def cpu_init(self, device=0, *a, **k):
        init(self, torch.device("cpu"), *a, **k)

    api.PostFXContext.__init__ = cpu_init
    execute = api.PostFXContext.execute

    def noting_execute(self, curr_depth, prev_depth, motion, curr_camera, prev_camera):
        dev.cam, dev.prev_cam = bytes(curr_camera), bytes(prev_camera)  # (the reference's shaders read the whole CameraAttribs block: device.py)
        return execute(self, curr_depth, prev_depth, motion, curr_camera, prev_camera)

    api.PostFXContext.execute = noting_execute
    chain_init, chain_execute = api.Chain.__init__, api.Chain.execute

    def cpu_chain_init(self, device=0, *a, **k):
        chain_init(self, torch.device("cpu"), *a, **k)

    def noting_chain_execute(self, bound):
        dev.cam, dev.prev_cam = bytes(bound[3]["camera"]), bytes(bound[3]["prev_camera"])
        return chain_execute(self, bound)

    api.Chain.__init__, api.Chain.execute = cpu_chain_init, noting_chain_execute
    dof_execute = api.DepthOfField.execute

    def noting_dof_execute(self, color, depth, attribs):
        dev.dof_attribs = bytes(attribs)  # (the launchers of depth of field carry scalars of the block: device.py)
        return dof_execute(self, color, depth, attribs)

    api.DepthOfField.execute = noting_dof_execute

    def host_view(desc, device):
        c, eb, ts = {B.FORMAT_F32: (1, 4, "<f4"), B.FORMAT_F32X2: (2, 4, "<f4"), B.FORMAT_F32X4: (4, 4, "<f4")}[desc.format]
        pitch_f = desc.pitch_bytes // eb
        flat = np.ctypeslib.as_array((ctypes.c_float * (pitch_f * desc.height)).from_address(desc.data))
        rows = torch.from_numpy(flat).view(desc.height, pitch_f)[:, : desc.width * c]
        return rows.view(desc.height, desc.width) if c == 1 else rows.unflatten(1, (desc.width, c))

    api._view = host_view

    def host_shard_plane(self, name):
        d = B.Image2D()
        B.check(self.lib.mifx_chain_get_shard_plane(self.handle, name.encode(), ctypes.byref(d)))
        pitch_f = d.pitch_bytes // 4
        return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * (pitch_f * d.height)).from_address(d.data))).view(d.height, pitch_f)

    api.Chain.shard_plane = host_shard_plane
    return dev


# the kernels of this run ARE the checker's shaders: what the device tests hold to 1e-3 must be equal here, bit for bit -- a difference is a difference of sequencing
def exact(got, want, what="", **_):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = np.array_equal(got, want, equal_nan=True)
    assert same, f"{what}: {(got != want).mean():.3e} of the values differ (max {np.nanmax(np.abs(got - want)):.3e})"
    return None, 0.0


def chain_random(lib, seed, exact, steps=14):
    """A random sequence through mifx_chain_execute: resizes, frame-index moves, history resets, TAA flag sets, half-resolution SSR / SSAO, the AO algorithm, and -- what the
    checker has no notion of -- the fusion mask and the stream-overlap mode changing from frame to frame.  Every frame equals the CPU chain (tests/chain_util.py) exactly."""
    import chain_util
    import cpu_chain
    import pyref
    from diligentfx_amd import synth
    from util import blue_noise_tables

    rng = np.random.default_rng(7000 + seed)
    sobol, tile = blue_noise_tables()
    ref = pyref.ref_lib()
    chain = api.Chain(0, sobol, tile)
    ibl_np = chain_util.make_ibl(ref, "ref_")
    ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]])
    cpu = cpu_chain.CpuChain(ref, "ref_")
    scene = synth.Scene()
    sa = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    sizes = [(96, 64), (80, 48), (70, 36), (112, 72)]
    w, h = sizes[0]
    idx, cam_pos = int(rng.integers(0, 40)), int(rng.integers(0, 30))
    for step in range(steps):
        if rng.random() < 0.2:
            w, h = sizes[int(rng.integers(len(sizes)))]
        idx += int(rng.choice([1, 1, 1, 1, 0, 2, 5, -1]))
        idx = max(idx, 0)
        cam_pos += 1
        if rng.random() < 0.15:
            chain.reset_history()
            cpu.reset_history()
        taa_flags = int(rng.choice([2, 2, 2, 0, 5, 7]))
        chain.taa_flags = cpu.taa_flags = taa_flags
        algo = int(rng.choice([0, 0, 1, 2]))
        chain.ssao_attribs.Algorithm = algo
        cpu.algorithm = ("gtao", "hbao", "vbao")[algo]
        chain.set_fusion_mask(int(rng.integers(0, 64)))
        chain.set_overlap(int(rng.integers(0, 6)))  # (4 / 5: the planes between the lanes alternate between two sets)
        f = synth.make_frame(scene, cam_pos, w, h, torch.device("cpu"))
        out = torch.zeros(h, w, 4)
        chain.execute(chain.bind_frame(idx, f, ibl, sa, out))
        g = {k: v.numpy() for k, v in f.items() if isinstance(v, torch.Tensor)}
        sattr = type(chain.ssao_attribs).from_buffer_copy(bytes(chain.ssao_attribs))
        want = run_cpu_frame(cpu, chain_util, g, bytes(f["camera"]), bytes(f["prev_camera"]), idx, ibl_np, sa, sattr)
        exact(np.ascontiguousarray(out.numpy()), want, what=f"chain sequence {seed} step {step} (frame {idx}, {w}x{h}, TAA {taa_flags}, algorithm {algo})")
    chain.close()


SHARD_CASES = [(2, 160, 192, None, 0), (3, 160, 192, (0, 70, 130, 192), 0), (4, 128, 256, None, 0), (2, 150, 186, (0, 90, 186), 0), (3, 160, 192, None, 2),
               (4, 160, 192, (0, 85, 93, 103, 192), 0),  # two bands of 8 and 10 rows: thinner than every history halo, ghost rows come from two ranks away
               (3, 160, 192, None, "dof"), (2, 150, 186, (0, 90, 186), "dof"),  # depth of field (temporal + Karis) between TAA and Bloom
               (4, 64, 640, None, "wide ao"),  # a tall frame and an effect radius of 8: taps of every pyramid level, bands + reaches well inside the frame -- the per-level store
               #                                 windows of SSAO's depth pyramid (api_ssao.cpp) bind (with an eighth of the reach this case fails)
               # the chain-wide attribute sets of tests/attrib_sets.py: every attribute that sizes a row window below ("narrow") and above its default ("wide": on half-resolution
               # SSAO / SSR and an odd half size; "dof": the widest circle of confusion, a fractional SSAO radius).  "narrow" twice: at 160x192 Bloom builds two levels only and
               # is not split (gather_level -1), at 64x640 it builds three
               (3, 160, 192, (0, 70, 130, 192), "set narrow"), (2, 150, 186, (0, 90, 186), "set wide"), (3, 160, 192, (0, 70, 130, 192), "set dof"), (4, 64, 640, None, "set narrow"),
               (3, 160, 192, (0, 70, 130, 192), "set wide at full resolution")]  # (the radii of "wide" in the full-resolution windows: mifx_ssr::march_rows without half_rows)


def sharded_case(lib, case, frames=4, max_motion_rows=12, skip=()):
    """Row-band sharding on the CPU product: N chain objects, each running the phases of mifx_chain_execute_phase on its band, the exchanges done by copying rows between their
    planes (tests/test_gpu_sharded.py LocalComm) -- against one unsharded chain object.  The launch handlers write only the row windows the product hands them, so a pass that
    reads rows no producer computed shows up as a difference: the bands' rows and the history planes on band + halo must be EQUAL.  (The shade handler writes whole frames and the
    hit fetch is a no-op: device.py.)"""
    import chain_util
    import test_gpu_sharded as S
    from diligentfx_amd import synth
    from diligentfx_amd.sharded import ShardedChain
    from util import blue_noise_tables

    world, W, H, cuts, half = SHARD_CASES[case]
    sobol, tile = blue_noise_tables()
    ref = pyref.ref_lib()
    ibl_np = chain_util.make_ibl(ref, "ref_")
    ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]])
    shade = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    ref_chain = api.Chain(0, sobol, tile)
    ranks = [api.Chain(0, sobol, tile) for _ in range(world)]
    attrib_set, _, full = half[4:].partition(" at full resolution") if str(half).startswith("set ") else (None, "", "")
    dof, wide, half = half == "dof", half == "wide ao", 0 if half in ("dof", "wide ao") or attrib_set else half
    for c in ranks + [ref_chain]:
        if attrib_set:
            import attrib_sets

            blocks = attrib_sets.apply(c, attrib_set)
            if full:
                c.set_effect_feature_flags(ssao_feature_flags=0, ssr_feature_flags=0)
            if blocks["dof_attribs"] is not None:
                DEVICE.dof_attribs = bytes(blocks["dof_attribs"])
            continue
        c.set_effect_feature_flags(ssao_feature_flags=half, ssr_feature_flags=half)
        if wide:
            c.ssao_attribs.EffectRadius = 8.0
        if dof:
            da = B.DOFAttribs.default()
            da.MaxCircleOfConfusion = 0.02
            c.set_depth_of_field(da, 3)
            DEVICE.dof_attribs = bytes(da)
    sharded = [ShardedChain(c, H, r, world, max_motion_rows, cuts) for r, c in enumerate(ranks)]
    comm = S.LocalComm(sharded)
    scene = synth.Scene()
    out_ref = torch.zeros(H, W, 4)
    outs = [torch.full((H, W, 4), -1.0) for _ in range(world)]
    for fi in range(16, 16 + frames):
        g = synth.make_frame(scene, fi, W, H, torch.device("cpu"))
        assert float(g["motion"][..., 1].abs().max()) * 0.5 * H < max_motion_rows
        if dof:
            g["camera"].fFocusDistance, g["camera"].fFStop, g["camera"].fFocalLength = 12.0, 1.2, 135.0
        if attrib_set:
            attrib_sets.frame(g, blocks)  # (the lens of depth of field, the roughness in the channel the set reads)
        DEVICE.cam, DEVICE.prev_cam = bytes(g["camera"]), bytes(g["prev_camera"])
        ref_chain.execute(ref_chain.bind_frame(fi, g, ibl, shade, out_ref))
        bounds = [c.bind_frame(fi, g, ibl, shade, o) for c, o in zip(ranks, outs)]
        DEVICE.composite_rows.clear()

        def effect_windows(_infos):
            # What the equality of the bands cannot see: the windows downstream of the composite carry spare rows (one per Bloom level), so a row window of SSAO or SSR
            # that is a few rows short spoils rows of the composite which never reach the band.  The composite launch of every rank names the rows it reads (the ranks run
            # their phases in order, one launch each); on those rows the resolved AO must be the unsharded chain's, and R6's radiance and variance on the rows R7 reads
            # inside the composite (3 more either side: api_ssr.cpp w6) -- before the halo exchange replaces the ghost rows with their owners'.
            assert len(DEVICE.composite_rows) == world, DEVICE.composite_rows
            for r, (c, (b, e)) in enumerate(zip(ranks, DEVICE.composite_rows)):
                assert b <= sharded[r].band[0] and sharded[r].band[1] <= e, (r, b, e, sharded[r].band)
                for name, reach, cols in (("ssao_history_ao", 0, W), ("ssr_history_radiance", 3, 4 * W), ("ssr_history_variance", 3, W)):
                    lo, hi = max(b - reach, 0), min(e + reach, H)
                    got, want = c.shard_plane(name)[lo:hi, :cols], ref_chain.shard_plane(name)[lo:hi, :cols]
                    rows = (got != want).any(-1).nonzero().flatten() + lo
                    assert rows.numel() == 0, (f"case {case} frame {fi} rank {r}/{world}: {name} differs from the unsharded chain's on rows {rows[:8].tolist()} .. {int(rows[-1])} of the "
                                               f"rows {lo} .. {hi} the composite reads (band {sharded[r].band})")

        infos = S.run_sharded_frame(sharded, comm, bounds, skip=skip, unsplit_bloom=S.bloom_is_unsplit(ref_chain, W, H), before_history_exchange=effect_windows)
        for r, sc in enumerate(sharded):
            b, e = sc.band
            assert torch.equal(outs[r][b:e], out_ref[b:e]), f"case {case} frame {fi} rank {r}/{world}: rows {(outs[r][b:e] != out_ref[b:e]).any(-1).any(-1).nonzero()[:8].flatten().tolist()} of the band differ"
            written = ((outs[r] != -1.0).any(-1).any(-1)).nonzero().flatten()
            assert bool((outs[r][:b] == -1.0).all()) and bool((outs[r][e:] == -1.0).all()), f"case {case} rank {r}: band {b}..{e}, rows written {int(written.min())}..{int(written.max())}"
            bad = S.history_mismatch(sc.chain, ref_chain, infos[r], b, e, H, W)
            assert not bad, f"case {case} frame {fi} rank {r}/{world}: history planes differ on band + halo: {bad}"
    for c in ranks + [ref_chain]:
        c.close()


GROUP_CASES = [(2, 160, 192, None, ""), (3, 160, 192, (0, 60, 130, 192), ""), (4, 128, 256, None, ""), (2, 160, 192, None, "half resolution"),
               (4, 160, 192, (0, 84, 92, 102, 192), "thin bands"), (3, 160, 192, (0, 60, 130, 192), "depth of field"),
               (3, 160, 192, (0, 60, 130, 192), "three lanes"),  # mifx_chain_set_overlap 3: the event requests of the SSAO lane (streams do nothing here: the host logic)
               # the chain-wide attribute sets of tests/attrib_sets.py (as in SHARD_CASES), here with Bloom's level-0 halo exchange and the gathered last level of SSAO's pyramid
               (3, 160, 192, (0, 60, 130, 192), "set narrow"), (2, 150, 186, (0, 90, 186), "set wide"), (3, 160, 192, (0, 60, 130, 192), "set dof"), (4, 64, 640, None, "set narrow")]


def local_group_case(lib, case, frames=4, auto_exposure=False):
    """mifx_chain_execute_sharded with the in-library communicator of one process (mifx_comm_create_local_group: csrc/api_comm.cpp -- the same code that decides which rows
    go to whom for the RCCL transport, with a copy in place of ncclSend / ncclRecv): one thread per rank, against the unsharded chain object, for equality
    (tests/test_comm.py::test_sharded_execute_in_process_group on the CPU build)."""
    import threading

    import chain_util
    from diligentfx_amd import synth
    from util import blue_noise_tables

    if case >= 100:  # a random configuration (round 6: the level-4 gather with its compute windows; bands that own no row of the last level; frames not divisible by 16)
        import random

        rng = random.Random(case)
        world = rng.randint(2, 6)
        w, h = rng.choice([(160, 192), (128, 256), (96, 320), (176, 208), (144, 240), (150, 200)])
        inner = sorted(rng.sample(range(4, h - 3), world - 1))
        cuts = (0, *inner, h) if rng.random() < 0.8 else None
        mode = rng.choice(["", "", "three lanes", "three lanes", "half resolution"])
    else:
        world, w, h, cuts, mode = GROUP_CASES[case]
    cuts = list(cuts) if cuts else [h * r // world for r in range(world + 1)]
    sobol, tile = blue_noise_tables()
    ibl_np = chain_util.make_ibl(pyref.ref_lib(), "ref_")
    ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]])
    sa = chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    ref = api.Chain(0, sobol, tile)
    chains = [api.Chain(0, sobol, tile) for _ in range(world)]
    scene = synth.Scene()
    fr = [synth.make_frame(scene, 16 + i, w, h, torch.device("cpu")) for i in range(frames)]
    for c in chains + [ref]:
        if mode == "half resolution":
            c.set_effect_feature_flags(ssao_feature_flags=2, ssr_feature_flags=2)
        if mode == "depth of field":
            da = B.DOFAttribs.default()
            da.MaxCircleOfConfusion = 0.02
            c.set_depth_of_field(da, 3)
            DEVICE.dof_attribs = bytes(da)
        if mode.startswith("set "):
            import attrib_sets

            blocks = attrib_sets.apply(c, mode[4:])
            if blocks["dof_attribs"] is not None:
                DEVICE.dof_attribs = bytes(blocks["dof_attribs"])
        if auto_exposure:
            c.set_auto_exposure(True)
    if mode.startswith("set "):
        for f in fr:
            attrib_sets.frame(f, blocks)
    if mode == "depth of field":
        for f in fr:
            f["camera"].fFocusDistance, f["camera"].fFStop, f["camera"].fFocalLength = 12.0, 1.2, 135.0
    max_motion = int(max(float(f["motion"][..., 1].abs().max()) for f in fr) * 0.5 * h) + 2
    comms = api.Comm.local_group(chains[0].postfx, world)
    outs = [torch.zeros(h, w, 4) for _ in range(world)]
    for r in range(world):
        assert comms[r].info() == (r, world, False)
        chains[r].set_sharding(comms[r], cuts, max_motion)
        if mode == "three lanes":
            chains[r].set_overlap(3)
    want = torch.zeros(h, w, 4)
    for i, f in enumerate(fr):
        DEVICE.cam, DEVICE.prev_cam = bytes(f["camera"]), bytes(f["prev_camera"])
        ref.execute(ref.bind_frame(16 + i, f, ibl, sa, want))
        errors = []

        def run(r):
            try:
                chains[r].execute_sharded(chains[r].bind_frame(16 + i, f, ibl, sa, outs[r]))
            except Exception as e:  # noqa: BLE001
                errors.append((r, repr(e)))

        threads = [threading.Thread(target=run, args=(r,), name=f"rank {r}") for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(300)
        assert not errors and not any(t.is_alive() for t in threads), errors
        for r in range(world):
            assert torch.equal(outs[r][cuts[r]:cuts[r + 1]], want[cuts[r]:cuts[r + 1]]), f"case {case} frame {i}: the band of rank {r} differs from the unsharded frame (world {world}, {w}x{h}, cuts {cuts}, {mode!r})"
        for name in ("taa_history", "ssr_history_radiance", "ssr_history_variance", "ssao_history_ao", "ssao_history_len"):
            full = ref.shard_plane(name)
            for r in range(world):
                lo, hi = max(cuts[r] - 8, 0), min(cuts[r + 1] + 8, h)
                assert torch.equal(chains[r].shard_plane(name)[lo:hi], full[lo:hi]), f"case {case} frame {i}: {name} of rank {r}"
    stats = [comms[r].stats() for r in range(world)]
    infos = [chains[r].shard_info(chains[r].bind_frame(16 + frames - 1, fr[-1], ibl, sa, outs[r])) for r in range(world)]
    for r in range(world):
        chains[r].set_sharding(None)
        comms[r].close()
        chains[r].close()
    ref.close()
    return stats, infos


CONFIGS = {  # the feature configurations of run.py `order_features` (the switches of order_run's `cfg`)
    "a": dict(output=True, targets=True),
    "b": dict(output=True, targets=True, transparency=True),
    "c": dict(output=True, targets=True, transparency=True, unfused=True),
    "d": dict(selection=True, grid=True, auto_exposure=True),  # (+ depth of field: order_run's own switch)
    "e": dict(output=True, targets=True, transparency=True, layers=True, selection=True, grid=True, auto_exposure=True),
}
CONFIG_NAMES = {"a": "shade output + targets", "b": "a + transparency, fused", "c": "a + transparency, unfused", "d": "selection + grid + depth of field + auto exposure",
                "e": "b + layers + shadows + selection + grid + depth of field + auto exposure"}


class Features:
    """The chain features a configuration of order_run switches on, with the planes the chain borrows for them, made for one frame size.  cfg: output (the shade's output
    stage with a desc), targets (write_targets), layers (all five material layers and two shadow-mapped lights), transparency (two slices, K = 4, the second with all five
    layers and a color_alpha plane), unfused (mifx_chain_set_transparency_fusion 0 for the run), selection, grid, auto_exposure."""

    def __init__(self, cfg):
        self.cfg = dict(cfg)
        self.layer_count, self.slice_count = 4, 2

    def shade_attribs(self, last_mip):
        import chain_util

        return (chain_util.shadowed_shade_attribs if self.cfg.get("layers") else chain_util.shade_attribs)(last_mip)

    def layers(self, normal, seed):
        """All five layers as Chain.set_material_layers / transparent_slice take them, for the frame size of `normal`"""
        from layers_util import make_layers

        planes, albedo, charlie = make_layers(np.ascontiguousarray(normal), seed=seed)
        dev = {k: torch.from_numpy(v) for k, v in planes.items()}
        dev["transmission"] = dev["transmission"][..., 0].contiguous()
        dev["sheen_albedo_scaling_lut"], dev["preintegrated_charlie"] = torch.from_numpy(albedo), torch.from_numpy(charlie)
        return dev

    def slices(self, w, h, normal):
        import oit_util
        import transparency_util as T
        from layers_util import IOR, ROTATION

        s = T.e2e_slices() if (w, h) == (24, 16) else T.make_slices(dict(name="order", w=w, h=h, k=4, l=2, reversed=False, opaque=True, alpha=True, seed=4242))
        out = [dict(gbuffer={k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in gb.items()}) for gb in s["gbuffers"][:2]]
        alpha = s["alpha"][1] if s["alpha"] is not None else (np.float32(0.2) + np.float32(0.6) * oit_util.field(77, h, w))
        out[1].update(layers=self.layers(normal, 11), flags=31, iridescence_ior=IOR, anisotropy_rotation=ROTATION, color_alpha=torch.from_numpy(np.ascontiguousarray(alpha, np.float32)))
        return out

    def apply(self, chain, frame, what=None):
        """Switches the configuration's features on for the size of `frame` (a synth frame); what: only these switches"""
        import chain_util
        import grid_util
        from layers_util import IOR, ROTATION
        from shade_output_util import _case, output_desc_fields

        on = lambda k: self.cfg.get(k) and (what is None or k in what)  # noqa: E731
        h, w = frame["depth"].shape
        if on("layers"):
            slices, infos = chain_util.make_shadow_inputs()
            chain.set_material_layers(self.layers(frame["normal"].numpy(), 5), 31, IOR, ROTATION, shadows=(torch.from_numpy(np.stack(slices)), infos, 3))
        if on("output") or on("targets"):
            chain.set_shade_output(output_desc_fields(_case("chain")) if self.cfg.get("output") else None, bool(self.cfg.get("targets")))
        if on("transparency"):
            chain.set_transparency(self.slices(w, h, frame["normal"].numpy())[: self.slice_count], self.layer_count)
        if on("selection"):
            sel = torch.ones(h, w)
            sel[h // 4: h // 2, w // 4: w // 2] = frame["depth"][h // 4: h // 2, w // 4: w // 2]
            a = B.SelectionAttribs.default(selection_id=5)
            a.nonselection_desaturation = 0.5
            chain.set_selection(a, sel)
        if on("grid"):
            chain.set_coordinate_grid(B.CoordinateGridAttribs.default(), grid_util.FLAG_XZ | grid_util.AXES)
        if on("auto_exposure"):
            chain.set_auto_exposure(True, 1.0 / 60.0, True)


def mid_run_sequence(i, chain, feat, frame):
    """The fixed sequence of switches of tests/transparency_util.py mid_run_state, applied in front of frame i where the state changes (the chain starts with the shade's
    output stage and targets on; the resize at frame 7 is the caller's: order_run's resize_at)."""
    import transparency_util as T

    targets, count, k, _ = state = T.mid_run_state(i)
    if i == 0 or state[:3] == T.mid_run_state(i - 1)[:3]:
        return
    if not targets:
        chain.set_transparency(None)
        chain.set_shade_output(None, False)
        return
    feat.slice_count, feat.layer_count = count, k
    if not T.mid_run_state(i - 1)[0]:
        feat.apply(chain, frame, ("output", "targets"))
    if count:
        feat.apply(chain, frame, ("transparency",))
    else:
        chain.set_transparency(None)


PLANES = ("normal", "base_color", "material", "ibl")
MID_RUN_FRAMES = 10  # (tests/transparency_util.py MID_RUN_FRAMES: the sequence ends with two frames of everything back on)


def order_run(lib, mode, mask, frames=7, band=None, drop_wait=None, dof=False, size=(96, 64), track=None, reset_at=None, edges=None, fail_at=None, fail="taa", outs=None, cfg=None,
              sequence=None, resize_at=None, check=True, planes=None, first_frame=16):
    """One chain object, `frames` frames queued without a host synchronisation in between (as bench.py queues them), under tests/cpu_product/order.py: returns the LaneOrder
    with its findings and the index range of the hipStreamWaitEvent calls of the last frame.  band = (y0, y1): mifx_chain_execute_band on that row band instead.
    track: a LaneOrder of the caller's (call_trace below); reset_at: reset_history before that frame; edges: mifx_chain_set_lane_edges; fail_at: the `fail` launch of that frame
    fails (device.py fail_next), and `outs` receives every frame's output, or the error its execute raised.
    cfg: the feature switches of Features (CONFIGS); sequence(i, chain, features, frame): switches in front of frame i, the chain starting with the shade output and targets
    alone; resize_at = (i, (w, h)): the frames from i on have that size; check off: no order check, the values alone; planes: receives the four target planes of every frame
    (where the shade writes them)."""
    import chain_util
    import order as O
    from diligentfx_amd import synth
    from util import blue_noise_tables

    W, H = size
    sobol, tile = blue_noise_tables()
    ibl_np = chain_util.make_ibl(pyref.ref_lib(), "ref_")
    ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]])
    feat = Features(cfg) if cfg is not None else None
    shade = feat.shade_attribs(len(ibl_np["prefiltered"]) - 1) if feat else chain_util.shade_attribs(len(ibl_np["prefiltered"]) - 1)
    scene = synth.Scene()
    sizes = [size if resize_at is None or i < resize_at[0] else resize_at[1] for i in range(frames)]
    fr = [synth.make_frame(scene, first_frame + i, sizes[i][0], sizes[i][1], torch.device("cpu")) for i in range(frames)]
    track = track or O.LaneOrder()
    track.drop_wait = drop_wait
    DEVICE.names.clear()  # (plane names by address: an address is used again after a resize, a re-created object, another run)
    cb = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)(track.runtime)
    if check:
        lib.mifx_cpu_set_runtime_callback(cb)
        cpu_device.TRACK = track
    fusion = lib.mifx_chain_set_transparency_fusion(0 if feat and feat.cfg.get("unfused") else 1)
    try:
        chain = api.Chain(0, sobol, tile)
        if feat:
            feat.apply(chain, fr[0], ("output", "targets") if sequence else None)
        if dof:
            da = B.DOFAttribs.default()
            da.MaxCircleOfConfusion = 0.02
            chain.set_depth_of_field(da, 3)
            DEVICE.dof_attribs = bytes(da)
            for f in fr:
                f["camera"].fFocusDistance, f["camera"].fFStop, f["camera"].fFocalLength = 12.0, 1.2, 135.0
        chain.set_fusion_mask(mask)
        if band:
            chain.set_row_band(band[0], band[1], 12)
        chain.set_overlap(mode)
        if edges:
            chain.set_lane_edges(edges)
        out = torch.zeros(H, W, 4)
        last = (0, 0)
        for i, f in enumerate(fr):
            if i == reset_at:
                chain.reset_history()
            if sequence:
                sequence(i, chain, feat, f)
            if sizes[i] != (W, H):
                W, H = sizes[i]
                out = torch.zeros(H, W, 4)
            DEVICE.cam, DEVICE.prev_cam = bytes(f["camera"]), bytes(f["prev_camera"])
            DEVICE.fail_next = fail if i == fail_at else None
            if i == fail_at and hasattr(track, "note"):
                track.note("the failing frame begins", "", ())
            w0 = track.waits
            b = chain.bind_frame(first_frame + i, f, ibl, shade, out)
            try:
                (chain.execute_band if band else chain.execute)(b)
            except B.MifxError as e:
                if i != fail_at:
                    raise
                out = str(e)
                if hasattr(track, "note"):
                    track.note("the failing frame returns", "", ())
            if outs is not None:
                outs.append(out if isinstance(out, str) else out.clone())
            if planes is not None:
                planes.append({p: chain.shade_target(p).clone() for p in PLANES} if getattr(chain, "_shade_targets", False) else None)
            out = torch.zeros(H, W, 4) if isinstance(out, str) else out
            last = (w0, track.waits)
        chain.set_overlap(0)
        chain.close()
    finally:
        lib.mifx_chain_set_transparency_fusion(fusion)
        cpu_device.TRACK = None
        lib.mifx_cpu_set_runtime_callback(ctypes.cast(None, ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)))
    return track, last


def call_trace(check_order=True):
    """order.py's LaneOrder that also writes down what the host code asks of the runtime, per calling thread (by thread name): event records, stream waits, host
    synchronisations, asynchronous copies / fills and launches (name + stream), as tuples in `calls[thread]`.  Streams and events are numbered by first appearance in the
    thread's own sequence; creations and destructions are left out (a creation makes the address a new handle).  check_order off: the trace alone (ranks on threads)."""
    import threading

    import order as O

    names = {O.RT_EVENT_RECORD: ("record", "es"), O.RT_STREAM_WAIT: ("wait", "se"), O.RT_STREAM_SYNC: ("stream sync", "s"), O.RT_EVENT_SYNC: ("event sync", "e"),
             O.RT_WRITE: ("write", "-s"), O.RT_READ: ("read", "-s")}

    class CallTrace(O.LaneOrder):
        def __init__(self):
            super().__init__()
            self.calls, self.ids, self.lock = {}, {}, threading.Lock()

        def note(self, what, kinds, handles, n=None):
            with self.lock:
                ids = self.ids.setdefault(threading.current_thread().name, {})
                args = []
                for k, h in zip(kinds, handles):
                    if k != "-":
                        if (k, h) not in ids:
                            ids[k, h] = ids[k] = ids.get(k, -1) + 1  # (ids[k]: the last number given to a handle of that kind)
                        args.append(f"{k}{ids[k, h]}")
                self.calls.setdefault(threading.current_thread().name, []).append((what, *args) + ((n,) if n is not None else ()))

        def runtime(self, op, a, b, n):
            if op in (O.RT_STREAM_CREATE, O.RT_EVENT_CREATE):
                with self.lock:
                    for ids in self.ids.values():
                        ids.pop(("s" if op == O.RT_STREAM_CREATE else "e", a or 0), None)
            elif op in names:
                self.note(names[op][0], names[op][1], (a or 0, b or 0), n if op in (O.RT_WRITE, O.RT_READ) else None)
            if check_order:
                super().runtime(op, a, b, n)

        def begin_launch(self, stream, name):
            self.note("launch " + name, "s", (stream,))
            if check_order:
                super().begin_launch(stream, name)

        def access(self, img, write):
            if check_order:
                super().access(img, write)

    return CallTrace()


def event_trace():
    """order.py's LaneOrder that also notes, for every hipStreamWaitEvent (by its index in the run), which launch preceded the record of the event it waits for on the
    recording stream: `wait_after[k]` = "<launch> on <the stream, numbered by first appearance>" -- how run.py order_features tells the waits of a frame apart."""
    import order as O

    class EventTrace(O.LaneOrder):
        def __init__(self):
            super().__init__()
            self.last_launch, self.event_after, self.wait_after, self.stream_ids = {}, {}, {}, {}

        def runtime(self, op, a, b, n):
            a0, b0 = a or 0, b or 0
            if op == O.RT_EVENT_RECORD:
                sid = self.stream_ids.setdefault(b0, len(self.stream_ids))
                self.event_after[a0] = f"{self.last_launch.get(b0, 'nothing')} on stream {sid}"
            elif op == O.RT_STREAM_WAIT:
                self.wait_after[self.waits] = self.event_after.get(b0, "an event never recorded")
            super().runtime(op, a, b, n)

        def begin_launch(self, stream, name):
            self.stream_ids.setdefault(stream, len(self.stream_ids))
            self.last_launch[stream] = name
            super().begin_launch(stream, name)

    return EventTrace()


def trace_configurations(lib):
    """What run.py `trace` runs: (name, function of a CallTrace) for every frame path of the chain -- mifx_chain_execute in every stream mode with the default fusions, all and
    none (reset_history before frame 4: the lanes fork again; depth of field on for one mask per mode; modes 4 and 5 once more with lane edges), mifx_chain_execute_band, the shade stage's
    features (CONFIGS a, b, c, e in modes 0, 2, 5), mifx_chain_execute_sharded over the in-library group (per rank), and the synchronous five-plane exchange with the luminance gather, with and without Bloom's level-0 halos."""
    import order as O

    rt_type = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)

    def group(t, case, env, **kw):
        cb = rt_type(t.runtime)
        lib.mifx_cpu_set_runtime_callback(cb)
        cpu_device.TRACK = t
        os.environ.update(env)
        try:
            local_group_case(lib, case, **kw)
        finally:
            for k in env:
                del os.environ[k]
            cpu_device.TRACK = None
            lib.mifx_cpu_set_runtime_callback(ctypes.cast(None, rt_type))

    edges = "ssao_compute_ao_kernel<ssr_intersection_kernel@1,taa_kernel<pbr_shade_ssr_mask_kernel@0"
    out = []
    for m in range(6):
        for j, k in enumerate((31, 63, 0)):
            dof = j == m % 3
            out.append((f"execute, overlap {m}, fusion mask {k}{', depth of field' if dof else ''}", lambda t, m=m, k=k, dof=dof: order_run(lib, m, k, dof=dof, track=t, reset_at=4)))
    for m in (4, 5):
        out.append((f"execute, overlap {m}, lane edges", lambda t, m=m: order_run(lib, m, 31, track=t, reset_at=4, edges=edges)))
    for m in (0, 2, 3):
        out.append((f"execute_band (20, 44), overlap {m}", lambda t, m=m: order_run(lib, m, 31, band=(20, 44), track=t)))
    # the shade stage's features (CONFIGS of order_features): one stream, the two streams where SSAO waits for the shade's targets (evShade), the deepest lanes
    for name in "abce":
        for m in (0, 2, 5):
            out.append((f"execute, shade features {name} ({CONFIG_NAMES[name]}), overlap {m}", lambda t, m=m, name=name: order_run(lib, m, 31, frames=5, dof=name == "e", track=t, cfg=CONFIGS[name])))
    # (not here: mifx_chain_execute_band with layers and shadows on -- the layered hit fetch.  device.py runs launch_pbr_shade_layers for unsharded frames only and refuses
    #  the launch with a hit list; tests/test_gpu_sharded.py, case "layers", runs it on the device)
    for case in range(len(GROUP_CASES)):
        out.append((f"execute_sharded, group case {case} {GROUP_CASES[case]}", lambda t, case=case: group(t, case, {})))
    sync = {"MIFX_SHARD_ASYNC_HALOS": "0"}
    out.append(("execute_sharded, group case 1, auto exposure, synchronous halos", lambda t: group(t, 1, sync, auto_exposure=True)))
    out.append(("execute_sharded, group case 1, auto exposure, synchronous halos, no Bloom level-0 halo", lambda t: group(t, 1, dict(sync, MIFX_SHARD_BLOOM_HALO="0"), auto_exposure=True)))
    return [(name, fn, "execute_sharded" not in name) for name, fn in out]


def lane_error(lib, mode, band, fail="taa"):
    """Frames 0 - 2 under order.py with the `fail` launch of frame 1 failing (taa: late in the frame, on whichever lane the mode runs it; postfx_prep in modes 1 and 2: on the
    side stream, between the fork and the frame's own join -- the window in which the parent left the context's stream unordered): the execute returns the launcher's status; between the failing launch and the return every lane
    the frame used gets a record and the context's stream (handle 0) a wait for it; frame 2 has no unordered pair and equals the frame 2 of a one-stream chain object given
    the same failure (the failed frame leaves TAA's history unwritten: the CPU chain has no such state)."""
    t, outs, want = call_trace(), [], []
    order_run(lib, mode, 31, frames=3, band=band, track=t, fail_at=1, fail=fail, outs=outs)
    order_run(lib, 0, 31, frames=3, band=band, fail_at=1, fail=fail, outs=want)
    assert isinstance(outs[1], str) and outs[1].startswith("MIFX_ERR_HIP") and outs[1] == want[1], (outs[1], want[1])
    calls = t.calls["MainThread"]
    begin, fail, end = ([c[0] for c in calls].index(what) for what in ("the failing frame begins", f"launch {fail} (fails)", "the failing frame returns"))
    main = f"s{t.ids['MainThread']['s', 0]}"
    used = {a for c in calls[begin:fail] for a in c[1:] if str(a).startswith("s")} - {main}
    assert len(used) == (3 if band else 1 if mode <= 2 else 2), (mode, band, used)
    after = calls[fail + 1:end]
    for lane in sorted(used):
        events = [(i, c[1]) for i, c in enumerate(after) if c[0] == "record" and c[2] == lane]
        assert any(("wait", main, e) in after[i + 1:] for i, e in events), f"overlap {mode}{', band' if band else ''}: after the failing launch, lane {lane} is not joined: {after}"
    assert not t.findings, t.describe()[:6]
    assert torch.equal(outs[2], want[2]) and torch.equal(outs[0], want[0]), f"overlap {mode}: frame 2 differs from the one-stream chain's after the same failure"
    return len(used), len(after)


def run_cpu_frame(cpu, chain_util, g, cam, prev, frame_index, ibl, sa, ssao_attribs):
    """chain_util.run_frame_inputs with the SSAO attributes of the frame (the algorithm changes from frame to frame here)."""
    from diligentfx_amd import binding as B
    from util import blue_noise_tables

    h, w = g["depth"].shape
    radiance, spec_ibl = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    cpu.call("pbr_shade", [g["base_color"], g["normal"], g["material"], g["depth"], None, None, ibl["lut"], ibl["irradiance"], ibl["prefiltered"]], [radiance, spec_ibl], cam0=cam,
             attribs=bytes(sa), fval=[0.02, 0.03, 0.05, 0.0])
    pf = cpu.postfx(frame_index, g["depth"], g["prev_depth"], g["motion"], cam, prev, blue_noise_tables())
    ssr = cpu.ssr(pf, radiance, g["depth"], g["normal"], g["material"], g["motion"], B.SSRAttribs.default(), None)
    ssao = cpu.ssao(pf, g["depth"], g["normal"], ssao_attribs, None)
    comp = np.zeros((h, w, 4), np.float32)
    cpu.call("composite", [radiance, spec_ibl, ssr, ssao, g["normal"], g["base_color"], g["material"], ibl["lut"]], [comp], cam0=cam, fval=[1.0, 1.0])
    taa = cpu.taa(pf, comp, B.TAAAttribs.default(), None)
    bloom = cpu.bloom(taa, B.BloomAttribs.default(), None)
    final = np.zeros((h, w, 4), np.float32)
    cpu.call("tonemap", [bloom], [final], attribs=bytes(B.ToneMappingAttribs.default(4)), fval=[0.3], ival=[1])
    return final


DEVICE = None


def main():
    global DEVICE
    dev = DEVICE = install()
    import test_gpu_host_sequence as T

    T.assert_close = exact
    T.to_np = lambda t: np.ascontiguousarray(t.detach().cpu().numpy())  # (a CPU tensor's numpy() is a view of the pitched plane: the device tests get a tight copy)
    what = sys.argv[1] if len(sys.argv) > 1 else "scenarios"
    lib = B.load()
    if what == "scenarios":
        names = sys.argv[2:] or list(T.SCENARIOS)
        for n in names:
            T.test_host_objects_follow_the_reference_sequencing(lib, n)
            print(f"cpu product: scenario OK: {n}", flush=True)
    elif what == "chain":
        import test_gpu_chain as C

        C.assert_close = exact
        C.to_np = T.to_np
        for fn in (sys.argv[2:] or ["test_chain_vs_cpu_chain", "test_chain_reversed_depth"]):
            getattr(C, fn)(lib)
            print(f"cpu product: scenario OK: chain {fn}", flush=True)
    elif what == "chain_sets":
        # mifx_chain_execute with each chain-wide attribute set of tests/attrib_sets.py on the chain object and on the CPU chain (tests/test_gpu_chain.py
        # test_chain_vs_cpu_chain_at_attribute_sets, for equality): an attribute block, feature flag or depth-of-field setting that the host code does not pass on shows here
        import attrib_sets
        import test_gpu_chain as C

        C.assert_close = exact
        C.to_np = T.to_np
        for name in attrib_sets.NAMES:
            da = attrib_sets.blocks(name)["dof_attribs"]
            DEVICE.dof_attribs = bytes(da) if da is not None else None
            C.chain_vs_cpu_chain(frames=4, attrib_set=name)
            print(f"cpu product: scenario OK: chain at set {name}", flush=True)
    elif what == "arguments":
        # the argument checks of round 5's entries, which need a chain object (the CPU build has one without a GPU)
        from util import blue_noise_tables

        sobol, tile = blue_noise_tables()
        chain = api.Chain(0, sobol, tile)

        def refused(fn, *a):
            try:
                fn(*a)
            except B.MifxError as e:
                return "MIFX_ERR_INVALID_ARG" in str(e) or "INVALID" in str(e)
            return False

        for good in ("", "ssao_compute_ao_kernel<ssr_intersection_kernel@1", "a<b@0,c<d@3,", None):
            chain.set_lane_edges(good)
        for bad in ("a<b", "a@1", "<b@1", "a<@1", "a<b@", "a<b@4", "a<b@-1", "nonsense"):
            assert refused(chain.set_lane_edges, bad), bad
        for mode in range(6):
            chain.set_overlap(mode)
        assert refused(chain.set_overlap, 6) and refused(chain.set_overlap, -1)
        chain.set_fusion_mask(api.Chain.FUSE_EVERY_SWITCH)
        chain.set_fusion_mask(api.Chain.FUSE_DEFAULT)
        assert refused(chain.set_fusion_mask, 64)
        chain.close()
        print("cpu product: scenario OK: arguments of the round-5 entries", flush=True)
    elif what == "layers":
        import test_gpu_pbr_layers as L

        L.assert_close = exact
        L.to_np = T.to_np
        import chain_util

        L.test_chain_with_material_layers(lib, chain_util.make_ibl(pyref.ref_lib(), "ref_"))
        print("cpu product: scenario OK: chain with material layers", flush=True)
    elif what == "sharded":
        for case in range(int(sys.argv[2]), int(sys.argv[3])):
            sharded_case(lib, case)
            print(f"cpu product: sharded case OK: {case}", flush=True)
        for skip in ("bloom", "history"):  # the comparison can see a missing row: without one of the two exchanges the bands differ (cf. test_every_exchange_is_needed)
            try:
                sharded_case(lib, 0, skip=(skip,))
            except AssertionError:
                print(f"cpu product: without the {skip} exchange the bands differ, as they must", flush=True)
            else:
                raise SystemExit(f"the banded run did not notice the missing {skip} exchange")
    elif what == "order":
        # the order of the lanes (order.py): no pair of conflicting accesses of two streams without a happens-before edge, in every stream mode of the chain, with the default
        # fusions, all of them and none, with depth of field, and for one rank's band under the sharded frame's lanes; then the control: every wait of a steady-state frame
        # dropped in turn -- the ones whose absence the handlers' planes can show must be found
        cases = [(m, k, None, False) for m in (0, 1, 2, 3, 4, 5) for k in (31, 63, 0)] + [(3, 31, None, True), (4, 31, None, True), (5, 31, None, True)] + [(m, 31, (16, 48), False) for m in (0, 2, 3)]
        for mode, mask, band, dof in cases:
            t, last = order_run(lib, mode, mask, band=band, dof=dof)
            assert t.launches > 50, t.launches
            assert not t.findings, (mode, mask, band, dof, t.describe()[:6])
            print(f"cpu product: order OK: overlap {mode}, fusion mask {mask}{', band ' + str(band) if band else ''}{', depth of field' if dof else ''}: {t.launches} launches, "
                  f"{t.waits} waits ({last[1] - last[0]} in the last frame), no unordered pair", flush=True)
        for mode, band, dof in ((1, None, False), (2, None, False), (3, None, False), (4, None, False), (5, None, False), (3, None, True), (5, None, True), (2, (16, 48), False), (3, (16, 48), False)):
            base, last = order_run(lib, mode, 31, band=band, dof=dof)
            needed, silent = [], []
            for k in range(*last):
                t, _ = order_run(lib, mode, 31, band=band, dof=dof, drop_wait=k)
                (needed if t.findings else silent).append(k - last[0])
            assert needed, f"overlap {mode}: no dropped wait was noticed -- the check sees nothing"
            print(f"cpu product: order control: overlap {mode}{', band' if band else ''}{', depth of field' if dof else ''}: of the {last[1] - last[0]} waits of a steady-state frame, dropping "
                  f"{len(needed)} leaves an unordered pair {needed}; {len(silent)} are implied by others or guard what this configuration does not touch {silent}", flush=True)
    elif what == "order_features":
        # the order of the lanes with the chain's newer features on (CONFIGS a - e): the shade's output stage and targets, the transparent draws fused and unfused, the
        # selection outline, the coordinate grid, auto exposure, material layers with shadow maps -- five frames queued without a host synchronisation, every stream mode;
        # a, b and e also with no fusion and every fusion; the fixed sequence of switches in modes 3 - 5; then the control on a, b and d.  argv[2]: which part
        part = sys.argv[2] if len(sys.argv) > 2 else "all"
        if part in ("cases", "all"):
            for name in "abcde":
                for mode in range(6):
                    for mask in ((31, 0, 63) if name in "abe" else (31,)):
                        t, last = order_run(lib, mode, mask, frames=5, dof=name in "de", cfg=CONFIGS[name])
                        assert t.launches > 50, t.launches
                        assert not t.findings, (name, mode, mask, t.describe()[:6], [DEVICE.names.get(f[1]) for f in t.findings[:6]])
                        print(f"cpu product: feature order OK: {name} ({CONFIG_NAMES[name]}), overlap {mode}, fusion mask {mask}: {t.launches} launches, {t.waits} waits "
                              f"({last[1] - last[0]} in the last frame), no unordered pair", flush=True)
        if part in ("sequence", "all"):
            for mode in (3, 4, 5):
                t, _ = order_run(lib, mode, 31, frames=MID_RUN_FRAMES, cfg=CONFIGS["b"], sequence=mid_run_sequence, resize_at=(7, (80, 48)))
                assert not t.findings, (mode, t.describe()[:6], [DEVICE.names.get(f[1]) for f in t.findings[:6]])
                assert all(DEVICE.log.count(n) for n in ("oit_build", "oit_attenuate", "oit_shade_blend", "pbr_shade_output", "pbr_shade"))
                print(f"cpu product: feature order OK: the sequence of switches, overlap {mode}: {t.launches} launches, {t.waits} waits, no unordered pair", flush=True)
        if part.startswith("control") or part == "all":
            # every wait of the last (steady-state) frame dropped in turn; the waits are told apart by the launch that preceded the record of their event on its stream
            names = part[7:] or "abd"
            for name in names:
                for mode in range(1, 6):
                    kw = dict(frames=5, dof=name == "d", cfg=CONFIGS[name])
                    base = event_trace()
                    _, last = order_run(lib, mode, 31, track=base, **kw)
                    assert not base.findings
                    needed, silent, found_by = [], [], {}
                    for k in range(*last):
                        t, _ = order_run(lib, mode, 31, drop_wait=k, **kw)
                        (needed if t.findings else silent).append(k - last[0])
                        found_by[f"{k - last[0]}, for the event recorded behind {base.wait_after[k]}"] = sorted({DEVICE.names.get(f[1], "another plane") for f in t.findings})
                    assert needed, f"{name}, overlap {mode}: no dropped wait was noticed -- the check sees nothing"
                    print(f"cpu product: feature order control: {name}, overlap {mode}: of the {last[1] - last[0]} waits of a steady-state frame, dropping {len(needed)} leaves an "
                          f"unordered pair {needed}; {len(silent)} are implied by others or guard what this configuration does not touch {silent}", flush=True)
                    for after, planes in found_by.items():
                        print(f"    wait {after}: {', '.join(planes) if planes else 'not found'}", flush=True)
                    if mode <= 2 and name in "ab":  # SSAO on the side stream reads the Normal target the shade writes on the context's stream
                        shade = [a for a in found_by if a.split(" behind ")[1].split(" on ")[0] in ("pbr_shade_output", "oit_shade_blend", "oit_blend")]
                        assert len(shade) == 1 and "target: normal" in found_by[shade[0]], (name, mode, found_by)
                        print(f"cpu product: feature order control: {name}, overlap {mode}: the side stream's wait for evShade is needed: {found_by[shade[0]]}", flush=True)
                    if mode >= 3 and name == "b":  # lane X behind lane S (evPrep, recorded behind SSR's depth hierarchy on S): through what the shade and the OIT passes write
                        prep = [a for a in found_by if " behind ssr_hiz_pyramid" in a]
                        hit = [p for a in prep for p in found_by[a] if p == "radiance" or p.startswith("target: ")]
                        assert prep and hit, (name, mode, found_by)
                        print(f"cpu product: feature order control: {name}, overlap {mode}: lane X's wait for evPrep is needed through {sorted(set(hit))}", flush=True)
    elif what == "feature_values":
        # sequencing equalities of the chain's newer features on this build (the same code runs on both sides of every comparison: bit for bit), on the frames of
        # tests/test_gpu_transparency.py ChainCase at 24x16 and one more
        import chain_util
        import cpu_chain
        from diligentfx_amd import synth
        from layers_util import IOR, ROTATION
        from shade_output_util import _case, output_desc_fields
        from util import blue_noise_tables

        W, H, N = 24, 16, 4
        bits = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731

        def run(name, mode, mask):
            outs, planes = [], []
            order_run(lib, mode, mask, frames=N, dof=name == "e", size=(W, H), cfg=CONFIGS[name], check=False, outs=outs, planes=planes, first_frame=0)
            return outs, planes

        part = sys.argv[2] if len(sys.argv) > 2 else "all"
        one_stream = {}
        for name in "be":
            if part not in ("modes", "all"):
                break
            want = one_stream[name] = run(name, 0, 31)
            n = 0
            for mode in range(6):
                for mask in (31, 0, 63):
                    if (mode, mask) == (0, 31):
                        continue
                    got = run(name, mode, mask)
                    for i in range(N):
                        assert bits(got[0][i], want[0][i]), f"{name}, overlap {mode}, fusion mask {mask}, frame {i}: out_ldr differs from one stream with the default mask"
                        for p in PLANES:
                            assert bits(got[1][i][p], want[1][i][p]), f"{name}, overlap {mode}, fusion mask {mask}, frame {i}: target {p} differs from one stream with the default mask"
                    n += 1
            print(f"cpu product: feature values OK: {name} ({CONFIG_NAMES[name]}): {n} combinations of overlap mode and fusion mask equal one stream with the default mask, "
                  f"{N} frames, out_ldr and four targets", flush=True)
        if len(one_stream) == 2:  # (e is another picture than b: what it adds is in the frame)
            assert not bits(one_stream["b"][0][N - 1], one_stream["e"][0][N - 1]), "configuration e gives the picture of configuration b"
        ref = pyref.ref_lib()
        ibl_np = chain_util.make_ibl(ref, "ref_")
        ibl = api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]])
        last = len(ibl_np["prefiltered"]) - 1
        scene = synth.Scene()
        fr = [synth.make_frame(scene, i, W, H, torch.device("cpu")) for i in range(N)]
        feat = Features(CONFIGS["b"])
        slices = feat.slices(W, H, fr[0]["normal"].numpy())
        ctx = api.PostFXContext(0, *blue_noise_tables())
        if part in ("entries", "all"):
            # the chain with configuration b against the public entries run outside it, per frame: all four targets; its out_ldr against oracle/cpu_chain.py fed the entries'
            # planes and colour (tests/test_gpu_shade_targets.py test_chain_against_the_reference_passes_on_the_entrys_planes, here for equality)
            outs, planes = one_stream.get("b") or run("b", 0, 31)
            sa = feat.shade_attribs(last)
            oit = api.OITResources(ctx, W, H, 4)
            cpu = cpu_chain.CpuChain(ref, "ref_")
            for i, f in enumerate(fr):
                gdev = {k: f[k] for k in ("base_color", "normal", "material", "depth")}
                color, normal, base, material, ibl_t = api.pbr_shade_targets(ctx, gdev, None, 0, f["camera"], sa, ibl, output=output_desc_fields(_case("chain")),
                                                                             background=(0.02, 0.03, 0.05, 0.0))
                untouched = base.clone()
                t = dict(color=color, base_color=base, material=material, ibl=ibl_t)
                oit.build_layers([dict(depth=x["gbuffer"]["depth"], base_color=x["gbuffer"]["base_color"]) for x in slices], f["camera"], f["depth"])
                oit.apply_attenuation(t)
                for x in slices:
                    oit.shade_blend(x, f["camera"], sa, ibl, t, f["depth"])
                assert not torch.equal(untouched, base)  # (something was blended)
                for p, want in (("normal", normal), ("base_color", base), ("material", material), ("ibl", ibl_t)):
                    assert bits(planes[i][p], want), f"frame {i}: the chain's target {p} differs from the public entries'"
                g = {k: np.ascontiguousarray(v.numpy()) for k, v in f.items() if isinstance(v, torch.Tensor)}
                g["emissive"] = g["occlusion"] = None
                g["normal"], g["base_color"], g["material"] = (np.ascontiguousarray(x.numpy()) for x in (normal, base, material))
                shade = lambda gg, cam, a, c=color, s=ibl_t: (np.ascontiguousarray(c.numpy()), np.ascontiguousarray(s.numpy()))  # noqa: E731
                want = chain_util.run_frame_inputs(cpu, g, bytes(f["camera"]), bytes(f["prev_camera"]), i, ibl_np, sa, shade=shade)
                exact(np.ascontiguousarray(outs[i].numpy()), want, what=f"frame {i}: the chain's out_ldr against the CPU chain on the entries' planes and colour")
            oit.close()
            print(f"cpu product: feature values OK: b equals the public entries outside the chain on four targets and the CPU chain fed their planes on out_ldr, {N} frames", flush=True)
        if part in ("entry", "all"):
            # mifx_oit_shade_blend on this build (it used to be refused here) against mifx_pbr_shade_execute_layers + mifx_oit_blend: one slice without layers, one with all
            # five and a color_alpha plane, without and with two shadow-mapped lights
            import oit_util

            f = fr[1]
            sm_np, infos = chain_util.make_shadow_inputs()
            start = oit_util.e2e_inputs()["targets"]
            for shadows, sa in ((None, chain_util.shade_attribs(last)), ((torch.from_numpy(np.stack(sm_np)), infos, 3), chain_util.shadowed_shade_attribs(last))):
                oit = api.OITResources(ctx, W, H, 4)
                sets = [{k: torch.from_numpy(start[j].copy()) for j, k in enumerate(api.OIT_TARGETS)} for _ in range(2)]
                oit.build_layers([dict(depth=x["gbuffer"]["depth"], base_color=x["gbuffer"]["base_color"]) for x in slices], f["camera"], f["depth"])
                for t in sets:
                    oit.apply_attenuation(t)
                for x in slices:
                    g = x["gbuffer"]
                    rad, spec = api.pbr_shade_layers(ctx, g, x.get("layers") or {}, x.get("flags", 0), f["camera"], sa, ibl, background=(0.0, 0.0, 0.0, 0.0), iridescence_ior=IOR,
                                                     anisotropy_rotation=ROTATION, shadows=shadows)
                    two = dict(depth=g["depth"], base_color=g["base_color"], material=g["material"], radiance=rad, specular_ibl=spec)
                    if x.get("color_alpha") is not None:
                        two["color_alpha"] = x["color_alpha"]
                    oit.blend(two, f["camera"], sets[0], f["depth"])
                    oit.shade_blend(x, f["camera"], sa, ibl, sets[1], f["depth"], shadows=shadows)
                changed = sum(int((sets[1][k] != torch.from_numpy(start[j])).any(-1).sum()) for j, k in enumerate(api.OIT_TARGETS))
                assert changed > W * H  # (blended, not merely attenuated: every target of most texels)
                for k in api.OIT_TARGETS:
                    assert bits(sets[0][k], sets[1][k]), f"mifx_oit_shade_blend, {'two shadow-mapped lights' if shadows else 'no shadow maps'}: target {k} differs from shade + blend"
                oit.close()
            print("cpu product: feature values OK: the host-only build runs mifx_oit_shade_blend: equal to mifx_pbr_shade_execute_layers + mifx_oit_blend, without and with shadow maps", flush=True)
        ctx.close()
    elif what == "trace":
        # every stream / event call and launch of every frame path, per calling thread: diffed between two builds of the host code (a refactor keeps it identical)
        for name, fn, check in trace_configurations(lib):
            if len(sys.argv) > 2 and sys.argv[2] not in name:
                continue
            t = call_trace(check)
            fn(t)
            for thread in sorted(t.calls):
                print(f"== {name} | {thread}: {len(t.calls[thread])} calls")
                print("\n".join(" ".join(str(a) for a in c) for c in t.calls[thread]), flush=True)
    elif what == "lane_errors":
        for mode, band, fail in ((5, None, "taa"), (3, None, "taa"), (2, None, "taa"), (3, (16, 48), "taa"), (1, None, "postfx_prep"), (2, None, "postfx_prep")):
            lanes, calls = lane_error(lib, mode, band, fail)
            print(f"cpu product: lane error OK: overlap {mode}{', band' if band else ''}, {fail} fails: {lanes} lane(s) joined in the {calls} runtime calls after the failing launch; frame 2 ordered and equal", flush=True)
    elif what == "auto_exposure":
        # the auto-exposure handlers of device.py under mifx_chain_execute_sharded: three ranks, the luminance rows gathered, the five history planes exchanged at the end of
        # the frame (MIFX_SHARD_ASYNC_HALOS=0) -- bands and histories equal the unsharded chain object's, whose average comes from the one-launch handler
        os.environ["MIFX_SHARD_ASYNC_HALOS"] = "0"
        local_group_case(lib, 1, auto_exposure=True)
        print("cpu product: in-library group OK: auto exposure, synchronous halos", flush=True)
    elif what == "order_random":
        # the random chain sequences (sizes, frame indices, resets, flag sets, the fusion mask and the stream mode changing from frame to frame) under order.py: what the
        # library queues on the context's stream between frames -- history fills of a reset, re-allocations of a resize -- against the lanes of the frames around it
        import order as O

        rt_type = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)
        for seed in range(int(sys.argv[2]), int(sys.argv[3])):
            track = O.LaneOrder()
            cb = rt_type(track.runtime)
            lib.mifx_cpu_set_runtime_callback(cb)
            cpu_device.TRACK = track
            try:
                chain_random(lib, seed, exact)
            finally:
                cpu_device.TRACK = None
                lib.mifx_cpu_set_runtime_callback(ctypes.cast(None, rt_type))
            assert not track.findings, (seed, track.describe()[:8])
            print(f"cpu product: order OK: chain sequence {seed}: {track.launches} launches, {track.waits} waits, no unordered pair", flush=True)
    elif what == "band":
        # mifx_chain_execute_band against the phases driven one by one (tests/test_gpu_sharded.py band_against_phases), one stream and two lanes
        import chain_util
        import test_gpu_sharded as S

        def make_ibl(_chain):
            ibl_np = chain_util.make_ibl(pyref.ref_lib(), "ref_")
            return api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]]), len(ibl_np["prefiltered"])

        def on_frame(g):
            DEVICE.cam, DEVICE.prev_cam = bytes(g["camera"]), bytes(g["prev_camera"])

        def on_chain(blocks):
            DEVICE.dof_attribs = bytes(blocks["dof_attribs"]) if blocks["dof_attribs"] is not None else None

        for overlap, attrib_set in ((0, None), (2, None), (3, None), (3, "narrow"), (3, "wide"), (2, "dof")):
            S.band_against_phases(torch.device("cpu"), overlap, False, make_ibl, W=160, H=192, cuts=(0, 60, 130, 192), on_frame=on_frame, attrib_set=attrib_set, on_chain=on_chain)
            print(f"cpu product: execute_band OK: overlap {overlap}{', set ' + attrib_set if attrib_set else ''}", flush=True)
    elif what == "controls":
        # mifx_chain_get_shard_info follows each attribute that sizes a row window, one attribute at a time (tests/test_gpu_sharded.py shard_info_controls), at the sizes of the
        # device test: host code only
        import chain_util
        import test_gpu_sharded as S

        def make_ibl(_chain):
            ibl_np = chain_util.make_ibl(pyref.ref_lib(), "ref_")
            return api.IBLResources(torch.from_numpy(ibl_np["lut"]), [torch.from_numpy(m) for m in ibl_np["irradiance"]], [torch.from_numpy(m) for m in ibl_np["prefiltered"]]), len(ibl_np["prefiltered"])

        def on_frame(g):
            DEVICE.cam, DEVICE.prev_cam = bytes(g["camera"]), bytes(g["prev_camera"])

        def on_chain(blocks):
            DEVICE.dof_attribs = bytes(blocks["dof_attribs"]) if blocks["dof_attribs"] is not None else None

        for name, w, h in (("narrow", 640, 768), ("narrow", 160, 192), ("wide", 600, 750), ("dof", 640, 768)):
            S.shard_info_controls(torch.device("cpu"), name, w, h, make_ibl, on_frame=on_frame, on_chain=on_chain)
            print(f"cpu product: shard info controls OK: set {name} at {w}x{h}", flush=True)
    elif what == "local_group":
        for case in range(int(sys.argv[2]), int(sys.argv[3])):
            local_group_case(lib, case)
            print(f"cpu product: in-library group OK: {case}", flush=True)
    elif what == "bloom_halo":
        # Round 6, Bloom's level 0 with halos (csrc/api_comm.cpp): the exchange really runs -- one more group per frame -- and buys what it is for: shorter history halos,
        # fewer bytes per frame in total; MIFX_SHARD_BLOOM_HALO=0 (read per frame) is round 5's frame.  Both frames equal the unsharded chain (local_group_case asserts that).
        frames = 2
        os.environ["MIFX_SHARD_BLOOM_HALO"] = "0"
        off, info_off = local_group_case(lib, 1, frames=frames)
        os.environ["MIFX_SHARD_BLOOM_HALO"] = "1"
        on, info_on = local_group_case(lib, 1, frames=frames)
        for a, b, ia, ib in zip(off, on, info_off, info_on):
            assert b["groups"] == a["groups"] + frames, (a, b)
            assert b["bytes_sent"] < a["bytes_sent"] and b["bytes_received"] < a["bytes_received"], (a, b)
            assert ib.halo_taa < ia.halo_taa and ib.halo_ssr < ia.halo_ssr and ib.halo_ssao <= ia.halo_ssao, ((ia.halo_taa, ia.halo_ssr, ia.halo_ssao), (ib.halo_taa, ib.halo_ssr, ib.halo_ssao))
        print(f"cpu product: Bloom level-0 halo OK: groups per frame {off[0]['groups'] // frames} -> {on[0]['groups'] // frames}, bytes sent by rank 1 per frame "
              f"{off[1]['bytes_sent'] // frames} -> {on[1]['bytes_sent'] // frames}, TAA halo {info_off[1].halo_taa} -> {info_on[1].halo_taa} rows", flush=True)
    elif what == "sharded_random":
        for seed in range(int(sys.argv[2]), int(sys.argv[3])):
            rng = np.random.default_rng(9000 + seed)
            world = int(rng.integers(2, 6))
            W, H = [(160, 192), (150, 186), (128, 256), (176, 208), (96, 320)][int(rng.integers(5))]
            inner = np.sort(rng.choice(np.arange(6, H - 6), size=world - 1, replace=False))
            cuts = (0, *[int(c) for c in inner], H) if rng.random() < 0.7 or H % world else None  # (equal bands need a height the ranks divide)
            opt = [0, 0, 2, "dof"][int(rng.integers(4))]
            SHARD_CASES.append((world, W, H, cuts, opt))
            sharded_case(lib, len(SHARD_CASES) - 1, frames=int(rng.integers(2, 5)), max_motion_rows=max(12, H // 16))
            print(f"cpu product: sharded sequence OK: {seed} (world {world}, {W}x{H}, cuts {cuts}, option {opt})", flush=True)
    elif what == "chain_random":
        for seed in range(int(sys.argv[2]), int(sys.argv[3])):
            chain_random(lib, seed, exact)
            print(f"cpu product: chain sequence OK: {seed}", flush=True)
    elif what == "material_fetch":
        # mifx_pbr_material_fetch (api_material.cpp) as shipped: ONE context through a sequence of fixture cases -- the same tables twice, other and larger tables, back
        # again, a 1x1 frame -- each call into sentinel-filled planes, against the same compiled body run on the case's own arrays (material_fetch_util.run_on_host): both
        # sides execute one body, so a difference is a difference of the host code -- the descriptors, which tables the context holds, when it uploads them
        import material_fetch_util as M
        import test_gpu_material_fetch as F
        from util import blue_noise_tables

        host = cpu_device.host_lib("material_fetch_host")
        by_name = {c["name"]: c for c in M.cases()}
        sequence = ("a_minified", "a_minified", "o_three_materials", "m_every_layer_rgba8", "a_minified", "p_frame_1x1")
        ctx = api.PostFXContext(0)
        inputs = {name: F.device_inputs(by_name[name], ctx.device) for name in set(sequence)}  # (made once a case: a repeated case hands the entry the very same tables)
        syncs = []
        rt_type = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)
        cb = rt_type(lambda op, a, b, n: syncs.append(step) if op == 7 else None)  # (RT_STREAM_SYNC of stub_device.cpp: the wait in front of an upload)
        lib.mifx_cpu_set_runtime_callback(cb)
        start = len(dev.log)
        for step, name in enumerate(sequence):
            c = by_name[name]
            interp, mats, textures = inputs[name]
            g, ly = F.caller_planes(c, ctx.device)
            g, ly = api.pbr_material_fetch(ctx, interp, mats, textures, B.camera_from_bytes(c["camera"].tobytes()), layer_flags=c["layers"], flags=c["flags"], mip_bias=c["mip_bias"],
                                           gbuffer=g, layers=ly)
            got = {**{k: v for k, v in g.items() if k != "depth"}, **ly}
            want = M.run_on_host(host, c)
            assert set(got) == set(want) == set(M.output_names(c)), (name, sorted(got), sorted(want))
            frag = M.has_fragment(c)
            for k, t in got.items():
                a = np.ascontiguousarray(t.numpy())
                assert np.array_equal(a.view(np.uint32), want[k].view(np.uint32)), f"call {step} ({name}), {k}: {(a.view(np.uint32) != want[k].view(np.uint32)).mean():.3e} of the words differ"
                assert (a[~frag] == M.SENTINEL).all() and (frag.all() or (a[frag] != M.SENTINEL).any()), (step, name, k)
        lib.mifx_cpu_set_runtime_callback(ctypes.cast(None, rt_type))
        assert dev.log[start:] == ["material_fetch"] * len(sequence), dev.log[start:]
        # the context waits for its stream and uploads exactly where the tables differ from the call before: not for the repeated case (call 1)
        assert syncs == [s for s in range(len(sequence)) if s == 0 or sequence[s] != sequence[s - 1]], syncs
        ctx.close()

        def refusal(ctx, c, mats=None):
            interp, m, textures = F.device_inputs(c, ctx.device)
            try:
                api.pbr_material_fetch(ctx, interp, mats(m, textures) if mats else m, textures, B.camera_from_bytes(c["camera"].tobytes()), flags=c["flags"])
            except B.MifxError as e:
                return str(e)
            return "MIFX_OK"

        c = by_name["a_minified"]
        chain = api.Chain(0, *blue_noise_tables())
        chain.set_row_band(4, 12, 0)
        got = refusal(chain.postfx, c)
        assert got == "MIFX_ERR_INVALID_ARG: mifx_pbr_material_fetch: not available inside a row band", got
        chain.close()

        def outside(m, textures):
            m[0].texture[B.PBR_TEXTURE_BASE_COLOR] = len(textures)
            return m

        ctx = api.PostFXContext(0)
        got = refusal(ctx, c, outside)
        assert got == f"MIFX_ERR_INVALID_ARG: mifx_pbr_material_fetch: desc->materials[0].texture[BASE_COLOR] = {len(c['textures'])} is outside the texture table of {len(c['textures'])} entries", got
        ctx.close()
        assert dev.log[start:] == ["material_fetch"] * len(sequence)  # (a refused call launches nothing)
        print(f"cpu product: scenario OK: the host-only build runs mifx_pbr_material_fetch: one context, {len(sequence)} calls ({', '.join(sequence)}) equal the body on each "
              "case's own arrays bit for bit; refused inside a row band and for a texture index outside the table", flush=True)
    elif what == "unhandled":
        # a launcher without a handler in device.py fails loudly: the shadow maps' host code is linked and runs up to its first launch
        import shadows_util

        ctx = api.PostFXContext(0)
        mgr = api.ShadowMapManager(ctx, B.SHADOW_MODE_VSM)
        try:
            mgr.convert_to_filterable(torch.full((1, 8, 8), 0.5), shadows_util.make_attribs(1, 8, 8))
            got = "MIFX_OK"
        except B.MifxError as e:
            got = str(e)
        assert got.startswith("MIFX_ERR_NOT_IMPLEMENTED") and "launch_shadow_convert" in got, got
        ctx.close()
        print("cpu product: scenario OK: the first launch of the shadow-map conversion is refused by name", flush=True)
    elif what == "dof":
        T.test_depth_of_field_follows_the_reference_sequencing(lib)
        print("cpu product: scenario OK: depth of field", flush=True)
    elif what == "random":
        for seed in range(int(sys.argv[2]), int(sys.argv[3])):
            T.test_random_sequences_through_the_c_abi(lib, seed)
            print(f"cpu product: random sequence OK: {seed}", flush=True)
    print("cpu product: done; launches:", len(dev.log))


if __name__ == "__main__":
    main()
