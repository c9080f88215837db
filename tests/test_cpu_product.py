"""The product's HOST code on the CPU: diligentfx_amd/csrc/api_*.cpp + mifx_core.cpp exactly as they ship, linked with a stand-in for the HIP runtime and with launchers that
run the reference's own shaders (oracle/_ref) for each pass (tests/cpu_product/).  The effect objects are then driven through the C ABI by the very functions of the device test
(tests/test_gpu_host_sequence.py) and compared with oracle/cpu_chain.py -- whose sequencing tests/test_host_sequence_vs_ref.py holds to the executed reference host classes --
for EQUALITY: the arithmetic on both sides is the same shader code, so any difference is a difference of sequencing (ping-pong slots, reset rules, alpha, clears, what a resize
or a flag change re-creates).  SURVEY 8a rows C0 / A0 / R0 / T0 / B0, on the product's side.  Test infrastructure: nothing under diligentfx_amd/ builds or loads any of it."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cpu_lib():
    import importlib.util

    import pyref

    if pyref.ref_lib() is None:
        pytest.skip("needs oracle/_ref (the reference's shaders stand in for the kernels)")
    spec = importlib.util.spec_from_file_location("_cpu_product_build", os.path.join(HERE, "cpu_product", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    lib = m.build()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


def run(cpu_lib, *args, timeout=900, **extra_env):
    env = dict(os.environ, MIFX_LIB_PATH=cpu_lib, **extra_env)
    env.pop("MIFX_STORAGE", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "cpu_product", "run.py"), *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "cpu product: done" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_the_launcher_stubs_are_what_the_generator_prints():
    """Everything below the "the launchers" marker of stub_device.cpp is the output of gen_stubs.py for the current mifx_host.h / mifx_*_host.h: a launcher added or changed
    in a header cannot miss the stub file."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "cpu_product", "gen_stubs.py")], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = open(os.path.join(HERE, "cpu_product", "stub_device.cpp")).read().splitlines(keepends=True)
    marker = [i for i, line in enumerate(lines) if line.startswith("// ---") and "the launchers" in line]
    assert len(marker) == 1, marker
    assert "".join(lines[marker[0] + 1:]) == r.stdout, "stub_device.cpp: re-run tests/cpu_product/gen_stubs.py and paste its output below the marker"
    assert r.stdout.count("mifx_status launch_") >= 70  # (the 56 launchers of mifx_host.h and the fourteen of the mifx_*_host.h headers)
    assert "mifx_status launch_oit_shade_blend(" in r.stdout and "mifx_status launch_material_fetch(" in r.stdout


def test_the_shadow_map_conversion_is_linked_and_refused_at_its_first_launch(cpu_lib):
    """A launcher without a handler in device.py fails loudly.  The host code of the shadow maps (api_shadows.cpp) is part of the CPU build and runs up to its first launch:
    mifx_shadow_convert_to_filterable of an 8 x 8 map with one cascade passes its argument checks and answers MIFX_ERR_NOT_IMPLEMENTED with launch_shadow_convert in
    mifx_last_error.  (The shade's output stage, OIT, the selection outline and the coordinate grid were refused this way until their handlers were written.)"""
    assert "cpu product: scenario OK: the first launch of the shadow-map conversion is refused by name" in run(cpu_lib, "unhandled")


def test_host_objects_on_the_cpu_equal_the_reference_sequencing(cpu_lib):
    out = run(cpu_lib, "scenarios")
    assert out.count("cpu product: scenario OK") >= 7, out


def test_depth_of_field_on_the_cpu_equals_the_reference_sequencing(cpu_lib):
    """TAA -> depth of field -> Bloom over ten steps (temporal CoC ping-pong, flag changes that re-create the targets, kernel changes, a resize)."""
    assert "cpu product: scenario OK: depth of field" in run(cpu_lib, "dof")


def test_random_sequences_on_the_cpu_product(cpu_lib):
    """Random sequences of 30 steps (resizes, frame-index moves, feature flags of every effect, AO algorithm, bokeh kernel, reversed depth, Bloom radius, resets, effects left
    out) -- the sequences of tests/test_gpu_host_sequence.py::test_random_sequences_through_the_c_abi, here compared for equality.  More seeds:
    MIFX_LIB_PATH=tests/cpu_product/_build/libmifx_cpu.so python tests/cpu_product/run.py random FIRST LAST."""
    out = run(cpu_lib, "random", "11", "13", timeout=1500)
    assert out.count("cpu product: random sequence OK") == 2, out


def test_the_chain_object_on_the_cpu_equals_the_cpu_chain(cpu_lib):
    """mifx_chain_execute -- the entry bench.py times -- with its default fusions (the shade writing SSR's mask planes, R7 inside the composite, the tone map inside Bloom's last
    pass): six frames and the replay after reset_history, plain and reversed depth, equal to the checker's chain bit for bit (the device test allows 5e-3 of the values to differ:
    flipped rays; here both sides run the same shaders, so nothing may)."""
    out = run(cpu_lib, "chain")
    assert out.count("cpu product: scenario OK: chain") == 2, out


def test_the_chain_object_at_the_attribute_sets_equals_the_cpu_chain(cpu_lib):
    """mifx_chain_execute with each chain-wide set of tests/attrib_sets.py (every attribute block off its defaults, half-resolution SSAO / SSR, depth of field) on the
    chain object and on the CPU chain: four frames equal bit for bit, so every block, flag and scale reaches its pass as the checker's chain hands it on."""
    out = run(cpu_lib, "chain_sets")
    assert out.count("cpu product: scenario OK: chain at set") == 3, out


def test_the_pipelined_chain_on_the_cpu_equals_the_cpu_chain(cpu_lib):
    """mifx_chain_set_overlap 4 (two frames in flight: the planes between lane S and lane X alternate between two sets, traded with the effect objects' own at the start of
    every frame) over the same frames, with lane edges set: which set a kernel is handed is host logic, so it shows here; the stream ordering does not (streams do nothing
    in this build: tests/test_gpu_chain.py holds that on the device)."""
    out = run(cpu_lib, "chain", MIFX_CHAIN_OVERLAP="4", MIFX_LANE_EDGES="ssao_compute_ao_kernel<ssr_intersection_kernel@1,taa_kernel<pbr_shade_ssr_mask_kernel@0")
    assert out.count("cpu product: scenario OK: chain") == 2, out
    out = run(cpu_lib, "chain", MIFX_CHAIN_OVERLAP="5")  # (round 6: mode 4 with the composite, TAA and depth of field on the Bloom lane)
    assert out.count("cpu product: scenario OK: chain") == 2, out


def test_argument_checks_of_the_round_5_entries(cpu_lib):
    """mifx_chain_set_lane_edges (well-formed and malformed lists), mifx_chain_set_overlap (0 .. 4), mifx_chain_set_fusion_mask (bit 5, refused beyond): on the CPU build's chain object."""
    assert "cpu product: scenario OK: arguments of the round-5 entries" in run(cpu_lib, "arguments")


def test_execute_band_on_the_cpu_equals_the_phases(cpu_lib):
    """mifx_chain_execute_band (api_comm.cpp execute_sharded_impl without a communicator: one stream, two lanes, three lanes requested) against mifx_chain_execute_phase 0 .. 4
    on a second chain object with the same band: band rows and histories equal, nothing written outside the band.  Three lanes and two once more at the chain-wide
    attribute sets of tests/attrib_sets.py (narrow / wide on three lanes, depth of field on two)."""
    out = run(cpu_lib, "band", timeout=900)
    assert out.count("cpu product: execute_band OK") == 6 and all(f"set {n}" in out for n in ("narrow", "wide", "dof")), out


def test_the_order_of_the_lanes_has_no_unordered_pair(cpu_lib):
    """tests/cpu_product/order.py: the stand-in runtime keeps a vector clock per stream and event, the launch handlers report the planes they read and write, and every pair of
    conflicting accesses of two streams must have a happens-before edge.  mifx_chain_execute in every stream mode (0 - 4) with the default fusions, all and none, with depth of
    field; mifx_chain_execute_band under the sharded frame's two and three lanes; seven frames queued without a host synchronisation.  Control: every hipStreamWaitEvent of a
    steady-state frame dropped in turn -- each is either noticed or (one, without depth of field) guards a plane that configuration does not write."""
    out = run(cpu_lib, "order", timeout=1500)
    assert out.count("cpu product: order OK") == 24 and out.count("cpu product: order control") == 9, out  # (round 6: + mode 5 -- the composite / TAA on the Bloom lane)
    assert "overlap 3, depth of field: of the 5 waits of a steady-state frame, dropping 5 leaves an unordered pair" in out, out
    assert "overlap 3, band: of the 7 waits of a steady-state frame, dropping 7 leaves an unordered pair" in out, out  # (the SSAO lane and the depth-hierarchy lane)


def test_a_failing_launch_leaves_the_context_stream_behind_every_lane(cpu_lib):
    """The error path of the lanes (mifx_objects.h LaneJoin): modes 5, 3 and 2 of mifx_chain_execute and mifx_chain_execute_band under three lanes, frames 0 - 2 at 96x64 under
    order.py, the `taa` launch of frame 1 failing (the launch callback's return value is the launcher's status).  The execute returns that error; between the failing launch and
    the return every lane the frame used gets an event record and the context's stream a wait for it; frame 2 has no unordered pair and equals frame 2 of a one-stream chain
    object given the same failure (tests/cpu_product/run.py lane_error).  Modes 1 and 2 once more with the `postfx_prep` launch failing: on the side stream, between the fork
    and the frame's own join through evPrep / evSsao -- the window in which the context's stream used to be left unordered."""
    assert run(cpu_lib, "lane_errors").count("cpu product: lane error OK") == 6


def test_auto_exposure_in_the_sharded_frame_on_the_cpu(cpu_lib):
    """mifx_chain_execute_sharded with auto exposure on and the halos exchanged at the end of the frame (MIFX_SHARD_ASYNC_HALOS=0), three ranks of the in-library group: the
    luminance rows of every band are gathered and reduced on every rank -- bands and history planes equal the unsharded chain object's, whose average luminance comes from
    the one-launch path (tests/cpu_product/device.py: the low-resolution luminance is the reference's pass, the mip chain and the blend are restated there)."""
    assert "cpu product: in-library group OK: auto exposure" in run(cpu_lib, "auto_exposure")


def test_random_chain_sequences_keep_the_lanes_ordered(cpu_lib):
    """The random sequences of test_random_sequences_through_the_chain_object_on_the_cpu (sizes, frame indices, history resets, flag sets, the fusion mask and the stream mode
    changing from frame to frame) under order.py: the fills and re-allocations the library queues on the context's stream between frames against the lanes around them."""
    out = run(cpu_lib, "order_random", "0", "4", timeout=1500)
    assert out.count("cpu product: order OK: chain sequence") == 4, out


def test_random_sequences_through_the_chain_object_on_the_cpu(cpu_lib):
    """mifx_chain_execute over random sequences in which, beside sizes, frame indices, resets, TAA flag sets and the AO algorithm, the FUSION MASK and the stream-overlap mode
    change from frame to frame (tests/cpu_product/run.py chain_random): every frame equals the CPU chain."""
    out = run(cpu_lib, "chain_random", "0", "3", timeout=1500)
    assert out.count("cpu product: chain sequence OK") == 3, out


def test_the_chain_with_material_layers_on_the_cpu(cpu_lib):
    """mifx_chain_set_material_layers: four frames with all five layers and two shadow-mapped lights equal the CPU chain whose shade is the reference's permutation; switched off
    again, the chain equals one that never had layers (tests/test_gpu_pbr_layers.py::test_chain_with_material_layers, for equality)."""
    assert "cpu product: scenario OK: chain with material layers" in run(cpu_lib, "layers")


def test_row_bands_on_the_cpu_product(cpu_lib):
    """Row-band sharding of the chain (mifx_chain_execute_phase) on the CPU build: 2, 3 and 4 chain objects on equal and uneven bands (down to 8 rows: thinner than the history halos), odd pyramid
    sizes, half-resolution SSAO / SSR, depth of field, the exchanges done by copying rows between their planes -- the bands' rows equal the unsharded chain object's, rows outside a band are never written, the history
    planes are equal on band + halo.  The launch handlers write only the row window each launcher was given, so a pass reading rows nobody computed would show; the run also drops
    each of the two exchanges once and must see the bands differ.
    Cases 9 - 13: the chain-wide attribute sets of tests/attrib_sets.py -- every attribute that sizes a row window (SSAO and SSR SpatialReconstructionRadius, Bloom Radius,
    depth of field's MaxCircleOfConfusion) below and above its default, half-resolution SSAO / SSR with the wide radii, a Bloom pyramid too short to split.  Every
    case also holds the resolved AO and SSR's accumulated radiance / variance to the unsharded chain's on ALL rows the band's composite reads, before the halo exchange: the
    windows behind the composite carry spare rows, so the bands alone do not show a window of SSAO or SSR that is a row or two short (SSR's taps stay a row or
    two inside the ceil(radius) + 1 rows its windows allow them: a window of its ray march that is 2 rows short changes no texel)."""
    out = run(cpu_lib, "sharded", "0", "14", timeout=2400)  # (case 8: the store windows of SSAO's depth pyramid levels bind)
    assert out.count("cpu product: sharded case OK") == 14 and out.count("exchange the bands differ, as they must") == 2, out


def test_shard_info_follows_each_attribute_that_sizes_a_row_window(cpu_lib):
    """mifx_chain_get_shard_info at the three sets of tests/attrib_sets.py, against the same set with one attribute back at its default, over 32 interior bands moved row by row
    (tests/test_gpu_sharded.py shard_info_controls, here on the CPU build of the host code): halo_ssao follows SSAO's SpatialReconstructionRadius (on the bands where the 16-row
    alignment of the window does not take up its 2 rows), all three halos follow depth of field, Bloom's Radius turns the gather off where the pyramid has two levels and moves
    neither the gathered level nor the owned rows otherwise, SSR's radius moves nothing."""
    assert run(cpu_lib, "controls").count("cpu product: shard info controls OK") == 4


def test_execute_sharded_with_the_in_library_group_on_the_cpu(cpu_lib):
    """mifx_chain_execute_sharded over the communicator of one process (csrc/api_comm.cpp: the code that decides which rows travel to whom for the RCCL transport as well, with a
    copy in place of ncclSend / ncclRecv), one thread per rank: 2, 3 and 4 ranks, half resolution, 8-row bands whose ghost rows come from two ranks away, depth of field -- bands and
    history planes equal the unsharded chain object's (tests/test_comm.py::test_sharded_execute_in_process_group on the CPU build)."""
    out = run(cpu_lib, "local_group", "0", "11", timeout=2400)  # (case 6: mifx_chain_set_overlap 3, the SSAO lane's event requests; 7 - 10: the sets of tests/attrib_sets.py)
    assert out.count("cpu product: in-library group OK") == 11, out


def test_blooms_level_0_halo_exchange_runs_and_shortens_the_history_halos(cpu_lib):
    """Round 6 (csrc/api_comm.cpp, mifx_bloom::halo_level0): in a sharded frame a rank prefilters the rows of Bloom's level 0 it owns and receives the rows beside its band's edges.
    Three ranks on uneven bands, the switch off and on (MIFX_SHARD_BLOOM_HALO, read per frame): one more exchange group per frame, fewer bytes per frame in total, shorter history
    halos reported by mifx_chain_get_shard_info -- and both frames equal the unsharded chain object's bit for bit."""
    assert "cpu product: Bloom level-0 halo OK" in run(cpu_lib, "bloom_halo", timeout=900)


CONFIGURATIONS = ("a", "b", "c", "d", "e")  # tests/cpu_product/run.py CONFIGS


def test_the_order_of_the_lanes_with_the_newer_features_has_no_unordered_pair(cpu_lib):
    """tests/cpu_product/order.py over the features that run inside mifx_chain_execute since the plain chain was order-checked -- a: the shade's output stage with a desc and
    its G-buffer targets; b: a + two transparent slices, K = 4, one with all five layers and a color_alpha plane, the fused launch; c: the same unfused; d: selection
    outline + coordinate grid + depth of field + auto exposure; e: b + material layers + two shadow-mapped lights + everything of d.  Five frames at 96x64 queued without a
    host synchronisation (modes 4 / 5 take their two-frames-in-flight path more than once), every overlap mode 0 - 5; a, b and e also with no fusion and every fusion.
    The handlers report every plane through view() / store() and the OIT layer words, the tail and the auto-exposure average as raw buffers: no pair of conflicting
    accesses of two streams without a happens-before edge."""
    out = run(cpu_lib, "order_features", "cases", timeout=1500)
    for name in CONFIGURATIONS:
        for mode in range(6):
            for mask in ((31, 0, 63) if name in "abe" else (31,)):
                assert sum(1 for line in out.splitlines() if line.startswith(f"cpu product: feature order OK: {name} (") and f"overlap {mode}, fusion mask {mask}:" in line
                           and line.endswith("no unordered pair")) == 1, (name, mode, mask, out)
    assert out.count("cpu product: feature order OK") == 66, out


def test_switching_the_features_mid_run_keeps_the_lanes_ordered(cpu_lib):
    """Ten frames in modes 3, 4 and 5 under order.py, the chain starting with the shade output and targets: transparency on at frame 2, one slice instead of two at 3,
    another layer_count at 4 (the OIT object is destroyed and re-created: hipFree), transparency off at 5, mifx_chain_set_shade_output(NULL, 0) at 6, a resize to 80x48 at
    7, everything back on at 8 -- no unordered pair; every kind of launch the sequence is about did run."""
    out = run(cpu_lib, "order_features", "sequence", timeout=900)
    assert out.count("cpu product: feature order OK: the sequence of switches") == 3 and all(f"the sequence of switches, overlap {m}:" in out for m in (3, 4, 5)), out


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_a_dropped_wait_is_found_with_the_newer_features_on(cpu_lib, name):
    """The control of the check above: in every mode 1 - 5 each hipStreamWaitEvent of the fifth (steady-state) frame is ignored in turn; per mode at least one drop leaves an
    unordered pair.  With write_targets on (a, b) in modes 1 and 2 the side stream's wait for evShade -- the event recorded behind the shade, or behind the last transparent
    draw -- is among them, found on the Normal target SSAO reads; with transparency on (b) in modes 3 - 5 the wait of lane X for evPrep is found through the radiance or a
    target plane, not only through the prep pass's planes.  The run prints which planes each dropped wait was found on."""
    out = run(cpu_lib, "order_features", "control" + name, timeout=1500)
    lines = out.splitlines()
    for mode in range(1, 6):
        head = [ln for ln in lines if ln.startswith(f"cpu product: feature order control: {name}, overlap {mode}: of the ")]
        assert len(head) == 1 and " dropping 0 leaves" not in head[0], (mode, out)
    if name in "ab":
        for mode in (1, 2):
            assert any(ln.startswith(f"cpu product: feature order control: {name}, overlap {mode}: the side stream's wait for evShade is needed") and "target: normal" in ln
                       for ln in lines), (mode, out)
    if name == "b":
        for mode in (3, 4, 5):
            assert any(ln.startswith(f"cpu product: feature order control: {name}, overlap {mode}: lane X's wait for evPrep is needed through") and
                       ("radiance" in ln or "target: " in ln) for ln in lines), (mode, out)


def test_the_newer_features_equal_one_stream_in_every_mode_on_the_cpu(cpu_lib):
    """Configurations b and e on the frames of tests/test_gpu_transparency.py ChainCase at 24x16 (and one more): every overlap mode 0 - 5 with fusion masks 31, 0 and 63
    equals one stream with the default mask over four frames, bit for bit, on out_ldr and the four target planes.  Streams do nothing in this build; which plane set a kernel
    is handed in modes 4 / 5 (the targets joined the double-buffered set) is host logic and shows here."""
    out = run(cpu_lib, "feature_values", "modes", timeout=1500)
    assert out.count("17 combinations of overlap mode and fusion mask equal one stream with the default mask, 4 frames, out_ldr and four targets") == 2, out


def test_the_chain_with_transparency_equals_the_public_entries_on_the_cpu(cpu_lib):
    """Configuration b against mifx_pbr_shade_targets, mifx_oit_build_layers, mifx_oit_apply_attenuation and one mifx_oit_shade_blend per slice with the frame's depth, run
    outside the chain on the same build: the four targets per frame, bit for bit; and the chain's out_ldr against oracle/cpu_chain.py fed those planes and that colour --
    the radiance the chain blends the transparent colour into, which no entry reads back, is held through the picture made from it."""
    assert "cpu product: feature values OK: b equals the public entries outside the chain on four targets and the CPU chain fed their planes on out_ldr, 4 frames" in run(
        cpu_lib, "feature_values", "entries", timeout=900)


def test_the_host_only_build_runs_the_shade_blend_entry(cpu_lib):
    """launch_oit_shade_blend is one of the generated stand-ins now (it used to be reached through a pointer nothing installed here, and the entry was refused): on this
    build mifx_oit_shade_blend equals mifx_pbr_shade_execute_layers + mifx_oit_blend on all four targets, for a slice without layers and one with all five and a color_alpha
    plane, without and with two shadow-mapped lights."""
    assert "cpu product: feature values OK: the host-only build runs mifx_oit_shade_blend" in run(cpu_lib, "feature_values", "entry", timeout=900)



def test_the_host_only_build_runs_the_material_fetch_entry(cpu_lib):
    """mifx_pbr_material_fetch (api_material.cpp; its launcher is one of the generated stand-ins) as shipped, on ONE context through six fixture cases: the same tables twice,
    other and larger tables, the first again, a 1x1 frame.  Every call's output planes equal the same compiled body run on the case's own arrays bit for bit, sentinels kept
    where no fragment is; the context waits for its stream and uploads exactly where the tables differ from the call before.  Inside a row band and with a texture index
    outside the table the entry answers with the status and the message it always had."""
    assert "cpu product: scenario OK: the host-only build runs mifx_pbr_material_fetch" in run(cpu_lib, "material_fetch", timeout=900)
