// api_chain.cpp -- the canonical caller of the hot path: one frame of
//   PBR shade -> PostFX prep -> SSR -> SSAO -> composite -> TAA -> Bloom -> ToneMap
// in the order of HnPostProcessTask::Prepare / Execute (Hydrogent/src/Tasks/HnPostProcessTask.cpp:671-682, 743-948).
// SSR reads the un-composited scene colour of the current frame (FEATURE_FLAG_PREVIOUS_FRAME off), tone mapping is applied by the
// final copy-frame pass because TAA is on (HnPostProcessTask.cpp:172, :920-927).  Everything is recorded on the context stream.
#include "mifx_objects.h"
#include "mifx_selection_host.h"
#include "mifx_grid_host.h"
#include <cstdlib>
#include <cmath>
#include <string>

using namespace mifx;

mifx_chain::~mifx_chain()
{
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    if (halo_stream) (void)hipStreamSynchronize(halo_stream);
    if (ctx) ctx->pending_joins.clear();
    for (hipEvent_t e : {evFork, evPrep, evSsao, evPrepConsumed, evBloomDone, evJoinS, evJoinX, evAfterP1, evAfterP2, evHaloSsao, evHaloRest, evXEnd[0], evXEnd[1], evHiz, evJoinH, evSsrDone, evShade})
        if (e) (void)hipEventDestroy(e);
    for (auto& kv : signals)
        for (hipEvent_t e : kv.second.ev)
            if (e) (void)hipEventDestroy(e);
    if (ctx) ctx->kernel_hook = nullptr;
    if (halo_stream) (void)hipStreamDestroy(halo_stream);
    if (side) (void)hipStreamDestroy(side);
    if (lane_x) (void)hipStreamDestroy(lane_x);
    if (lane_h) (void)hipStreamDestroy(lane_h);
    mifx::chain_detach_comm(this);
    mifx_selection_destroy(selection);
    mifx_oit_destroy(shade.oit);
    mifx_autoexposure_destroy(auto_exposure);
    mifx_bloom_destroy(bloom);
    mifx_dof_destroy(dof);
    mifx_taa_destroy(taa);
    mifx_ssr_destroy(ssr);
    mifx_ssao_destroy(ssao);
    mifx_postfx_destroy(ctx);
}

void mifx_chain::join_halos()
{
    // Only the context's stream is ordered behind the exchange here.  A lanes frame that follows (sharded or not, overlap >= 2) runs its first phases on the side
    // streams and, while chain_lanes_continue() holds, starts them behind the previous frame's events alone -- with the pending flags cleared nothing would order those
    // streams behind the ghost rows still arriving on halo_stream.  So the next frame forks every lane from the context's stream again.
    if (halo_ssao_pending || halo_rest_pending) prep_consumed = false;
    if (halo_ssao_pending) (void)hipStreamWaitEvent(ctx->stream, evHaloSsao, 0);
    if (halo_rest_pending) (void)hipStreamWaitEvent(ctx->stream, evHaloRest, 0);
    halo_ssao_pending = halo_rest_pending = false;
    ctx->pending_joins.clear();
}

extern "C" {

mifx_status mifx_chain_create(const mifx_device_desc* dev, const mifx_postfx_create_info* info, mifx_chain** out)
{
    MIFX_REQUIRE(dev != nullptr && out != nullptr, "mifx_chain_create: null argument");
    *out = nullptr;
    mifx_chain* c = new mifx_chain();
    mifx_status st = mifx_postfx_create(dev, info, &c->ctx);
    if (st >= 0) st = mifx_ssao_create(c->ctx, &c->ssao);
    if (st >= 0) c->ssao->alias_output = true; // the chain reads the AO of the frame it just executed: history_ao[curr] is the output (mifx_objects.h)
    if (st >= 0) st = mifx_ssr_create(c->ctx, &c->ssr);
    if (st >= 0) st = mifx_taa_create(c->ctx, &c->taa);
    if (st >= 0) st = mifx_bloom_create(c->ctx, &c->bloom);
    if (st < 0)
    {
        delete c;
        return st;
    }
    if (const char* e = std::getenv("MIFX_CHAIN_OVERLAP")) c->overlap = std::atoi(e) < 0 ? 0 : std::atoi(e) > 5 ? 5 : std::atoi(e);
    if (const char* e = std::getenv("MIFX_LANE_EDGES")) (void)mifx_chain_set_lane_edges(c, e); // (a malformed list is reported by the call itself when made directly)
    if (const char* e = std::getenv("MIFX_SHARD_ASYNC_HALOS")) c->async_halos = std::atoi(e) != 0;
    *out = c;
    return MIFX_OK;
}

void mifx_chain_destroy(mifx_chain* chain) { delete chain; }

mifx_status mifx_chain_get_postfx(mifx_chain* chain, mifx_postfx** out)
{
    MIFX_REQUIRE(chain != nullptr && out != nullptr, "mifx_chain_get_postfx: null argument");
    *out = chain->ctx;
    return MIFX_OK;
}

mifx_status mifx_chain_get_effect(mifx_chain* chain, const char* name, void** out)
{
    MIFX_REQUIRE(chain != nullptr && name != nullptr && out != nullptr, "mifx_chain_get_effect: null argument");
    const std::string n = name;
    if (n == "ssao") *out = chain->ssao;
    else if (n == "ssr") *out = chain->ssr;
    else if (n == "taa") *out = chain->taa;
    else if (n == "bloom") *out = chain->bloom;
    else if (n == "dof") *out = chain->dof; // NULL until mifx_chain_set_depth_of_field enabled it
    else if (n == "selection") *out = chain->selection; // NULL until mifx_chain_set_selection turned it on
    else if (n == "oit") *out = chain->shade.oit;       // NULL until a frame ran with mifx_chain_set_transparency on
    else
    {
        set_error("mifx_chain_get_effect: unknown effect '%s'", name);
        return MIFX_ERR_INVALID_ARG;
    }
    return MIFX_OK;
}

mifx_status mifx_chain_reset_history(mifx_chain* chain)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_reset_history: null argument");
    chain->prep_consumed = false; // (the fills below are queued on the context stream: the next frame's lanes fork from it again)
    chain->join_halos();
    MIFX_CHECK(mifx_ssao_reset_history(chain->ssao));
    MIFX_CHECK(mifx_ssr_reset_history(chain->ssr));
    if (chain->dof) MIFX_CHECK(mifx_dof_reset_history(chain->dof)); // (the temporal circle of confusion: cleared as at creation -- the reference has no reset for it)
    if (chain->auto_exposure) MIFX_CHECK(mifx_autoexposure_reset(chain->auto_exposure, 0.1f)); // (the adapted average luminance back at the reference's start value)
    return mifx_taa_reset_history(chain->taa);
}

// The chain's transparent draws take the fused launch (mifx_chain_set_transparency_fusion; the measurement behind the default: DESIGN.md section 4)
static bool g_transparency_fusion = true;

// mifx_chain_set_transparency: HnBeginOITPassTask, the transparent draws and HnEndOITPassTask directly behind the opaque shade, on its stream.  The layers are built over
// the slices' depth and opacity against the frame's depth, the opaque colour and the BaseColor / Material / IBL targets are attenuated, then every slice is shaded and
// blended in submission order -- one launch per slice, or (fusion off) the layered shade into the chain's two slice planes and mifx_oit_blend.
static mifx_status chain_transparency(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* radiance)
{
    mifx_chain::ShadeStage& sh = chain->shade;
    const uint32_t          n  = uint32_t(sh.transparent.size());
    const mifx_oit_targets  tg = sh.oit_targets(radiance);
    const mifx_image2d      rad = sh.slice_radiance.desc(), spec = sh.slice_specular_ibl.desc();
    mifx_oit_slice          slices[MIFX_OIT_MAX_SLICES];
    for (uint32_t i = 0; i < n; ++i)
    {
        const mifx_transparent_slice& s = sh.transparent[i].s;
        // (the two shaded planes exist in the unfused path only, and only mifx_oit_blend reads them)
        slices[i] = mifx_oit_slice{s.gbuffer.depth, s.gbuffer.base_color, s.gbuffer.material, g_transparency_fusion ? nullptr : &rad, g_transparency_fusion ? nullptr : &spec, s.color_alpha};
    }
    MIFX_CHECK(mifx_oit_build_layers(sh.oit, slices, n, f->gbuffer.depth, f->curr_camera));
    MIFX_CHECK(mifx_oit_apply_attenuation(sh.oit, &tg));
    const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t i = 0; i < n; ++i)
    {
        const mifx_transparent_slice& s = sh.transparent[i].s;
        if (g_transparency_fusion)
        {
            MIFX_CHECK(mifx_oit_shade_blend(sh.oit, &s, f->gbuffer.depth, f->curr_camera, f->pbr, f->ibl, sh.shadows(), &tg));
            continue;
        }
        MIFX_CHECK(mifx_pbr_shade_execute_layers(chain->ctx, &s.gbuffer, &sh.transparent[i].layers.v, f->curr_camera, f->pbr, f->ibl, sh.shadows(), zero, &rad, &spec));
        MIFX_CHECK(mifx_oit_blend(sh.oit, &slices[i], f->gbuffer.depth, f->curr_camera, &tg));
    }
    return MIFX_OK;
}

// Which shade the frame takes, decided here alone from the chain and the frame: the shade, the sharded frame's hit fetch and the choice of the planes behind the shade ask here or
// ask the stage (mifx_chain::ShadeStage).  Plain: mifx_pbr_shade_execute; PlainWithMask: with SSR's roughness / reflection-mask planes as a by-product (fuse_ssr_mask: pass R2
// reads the same material and depth texels and nothing else); Layered: mifx_chain_set_material_layers (no by-product: SSR runs R2 itself); Output: mifx_chain_set_shade_output, to
// the end of the pixel shader's `main` (no by-product either); OutputTargets: and the USD footer's four targets, which the passes behind the shade then read, with the transparent draws
enum class Shade { Plain, PlainWithMask, Layered, Output, OutputTargets };
static Shade chain_shade_kind(const mifx_chain* chain, const mifx_chain_frame* f)
{
    const mifx_chain::ShadeStage& sh = chain->shade;
    if (sh.output_stage()) return sh.targets_on ? Shade::OutputTargets : Shade::Output;
    if (sh.layers().flags != 0u || sh.shadows() != nullptr) return Shade::Layered;
    return !chain->fuse_ssr_mask || f->ssr->RoughnessChannel > 3u ? Shade::Plain : Shade::PlainWithMask;
}

// The forward shade of the frame.  With a row band the shade runs on the rows of the composite; the R2 by-product is needed on the rows of the ray march, a few rows
// more: the shade then covers those (+3 % of its rows against a pass over the material and depth planes), and mifx_ssr_execute finds the planes done for this frame.
static mifx_status chain_shade(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* radiance, const mifx_image2d* spec)
{
    mifx_postfx*            ctx  = chain->ctx;
    mifx_ssr*               ssr  = chain->ssr;
    mifx_chain::ShadeStage& sh   = chain->shade;
    const Shade             kind = chain_shade_kind(chain, f);
    const int               H    = int(radiance->height);
    const bool              wide = kind == Shade::PlainWithMask && !ctx->band.empty(); // (the by-product on the rows of the ray march)
    sh.shaded_rows  = wide ? mifx_ssr::march_rows(*f->ssr, ctx->needed_rows(H), H, (chain->ssr_flags & MIFX_SSR_FEATURE_FLAG_HALF_RESOLUTION) != 0) : ctx->needed_rows(H);
    sh.shaded_frame = f->frame.Index;
    switch (kind)
    {
    case Shade::Plain: return mifx_pbr_shade_execute(ctx, &f->gbuffer, f->curr_camera, f->pbr, f->ibl, f->background, radiance, spec);
    case Shade::Layered: return mifx_pbr_shade_execute_layers(ctx, &f->gbuffer, &sh.layers(), f->curr_camera, f->pbr, f->ibl, sh.shadows(), f->background, radiance, spec);
    case Shade::Output: return mifx_pbr_shade_output(ctx, &f->gbuffer, &sh.layers(), f->curr_camera, f->pbr, f->ibl, sh.shadows(), sh.output_desc(), f->background, radiance, spec);
    case Shade::OutputTargets:
    {
        const mifx_pbr_targets tg = sh.pbr_targets(); // (`spec` is the IBL target: chain_frame_planes)
        MIFX_CHECK(mifx_pbr_shade_targets(ctx, &f->gbuffer, &sh.layers(), f->curr_camera, f->pbr, f->ibl, sh.shadows(), sh.output_desc(), f->background, radiance, &tg));
        return sh.transparent.empty() ? MIFX_OK : chain_transparency(chain, f, radiance);
    }
    case Shade::PlainWithMask: break;
    }
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    SsrMaskOut r2{ssr->roughness.view(), ssr->mask.view(), f->ssr->RoughnessThreshold, f->ssr->IsRoughnessPerceptual, f->ssr->RoughnessChannel, 1};
    MifxKernelTimer timer(ctx, "pbr_shade_ssr_mask_kernel"); // (includes the two cube-apron launches of the call)
    MIFX_CHECK(launch_pbr_shade(ctx->stream, ctx->ibl_apron, &f->gbuffer, *f->curr_camera, *f->pbr, f->ibl, f->background, radiance, spec, sh.shaded_rows.b, sh.shaded_rows.e,
                                (ctx->flags & MIFX_POSTFX_FEATURE_FLAG_REVERSED_DEPTH) != 0, nullptr, &r2));
    ssr->mask_provided_for = f->frame.Index;
    return MIFX_OK;
}

// The chain has ONE material plane, which the shade, SSR (pass R2) and the composite all read as the USD G-buffer's Material target (PerceptualRoughness, Metallic:
// USD_Renderer.cpp:98).  A specular-glossiness shade would read the same plane as PhysicalDesc (specular colour + glossiness) and SSR / the composite would then take
// their roughness from the specular-colour channels: refused.  A caller with specular-glossiness inputs shades with mifx_pbr_shade_execute and hands the chain's
// other effects the plane mifx_pbr_specgloss_to_material produces.
// (with the check that every attribs pointer is there: what each entry that takes a frame asks of it; `entry` = its name)
static mifx_status chain_check_frame(const mifx_chain_frame* f, const char* entry)
{
    MIFX_REQUIRE(f->curr_camera && f->prev_camera && f->ibl && f->pbr && f->ssao && f->ssr && f->taa && f->bloom && f->tone_mapping,
                 "%s: every attribs pointer of mifx_chain_frame must be set", entry);
    MIFX_REQUIRE(f->pbr->Workflow == MIFX_PBR_WORKFLOW_METALLIC_ROUGHNESS,
                 "mifx_chain_execute: Workflow %d: the chain's material plane is the metallic-roughness Material target (see mifx_pbr_specgloss_to_material)", f->pbr->Workflow);
    return MIFX_OK;
}

// mifx_chain_set_selection: HnProcessSelectionTask's jump flood, then the composite with the selection tail of HnPostProcess.psh:211-241, both on the composite's stream and rows.
// TAA follows the composite in the chain, so a tone-mapped frame gets the outline colours in HDR: ReverseExpToneMap(colour, fMiddleGray, AverageLogLum), alpha as given
// (HnPostProcessTask.cpp:843-850).
static mifx_status chain_selection_composite(mifx_chain* chain, const mifx_chain_frame* f, const mifx_composite_attribs& ca, const mifx_image2d* comp, const SsrCleanupIn* r7)
{
    mifx_selection_attribs a = chain->selection_attribs;
    if (f->tone_mapping != nullptr && f->tone_mapping->iToneMappingMode != MIFX_TONE_MAPPING_MODE_NONE)
    {
        MIFX_CHECK(mifx_reverse_exp_tone_map(chain->selection_attribs.outline_color, f->tone_mapping->fMiddleGray, f->ave_log_lum, a.outline_color));
        MIFX_CHECK(mifx_reverse_exp_tone_map(chain->selection_attribs.occluded_outline_color, f->tone_mapping->fMiddleGray, f->ave_log_lum, a.occluded_outline_color));
    }
    return selection_chain_composite(chain->selection, a, &chain->selection_depth, ca, f->gbuffer.depth, comp, r7);
}

// The Normal / BaseColor / Material planes the passes behind the shade read: the caller's G-buffer, or -- mifx_chain_set_shade_output with targets -- the planes the shade's
// footer wrote this frame (USD_Renderer.cpp:148-160: in Hydrogent these ARE the G-buffer the post-process reads).  Depth and motion are always the caller's.
struct ChainGBuffer
{
    const mifx_image2d *normal, *base_color, *material;
};
static ChainGBuffer chain_gbuffer(const mifx_chain* chain, const mifx_chain_frame* f)
{
    if (chain_shade_kind(chain, f) == Shade::OutputTargets) return {&chain->shade.target_desc[0], &chain->shade.target_desc[1], &chain->shade.target_desc[2]};
    return {f->gbuffer.normal, f->gbuffer.base_color, f->gbuffer.material};
}
// The chain's colour planes of this frame: radiance, the composite's specular IBL (the IBL target with targets on), the composite
struct ChainPlanes
{
    mifx_image2d radiance, spec, comp;
};
static ChainPlanes chain_frame_planes(mifx_chain* chain)
{
    mifx_chain::ShadeStage& sh = chain->shade;
    if (sh.targets_on) sh.frame_targets();
    return {chain->radiance.desc(), sh.targets_on ? sh.target_desc[3] : chain->specular_ibl.desc(), chain->composite.desc()};
}

// The composite draw (HnPostProcess.psh:145-185).  With fuse_ssr_cleanup the kernel evaluates SSR's last pass (R7, the bilateral cleanup) for its own pixel from the
// effect's accumulated radiance instead of reading the plane R7 would have written (mifx_ssr::run stopped after R6: mifx_ssr::Request::defer_cleanup).
// With fuse_composite_taa on top of that (round 5) nothing is launched here: the TAA kernel of this frame evaluates the composite for the texels of its colour tile
// (taa.hip) -- the request is left in `hand` and given to mifx_taa::run by chain_taa below.  Not on TAA's placeholder frame (a copy of the plane).
// `hand` is a local of the scope that calls both steps: the image descriptors its attribs point to are that scope's locals and the frame's.
struct CompositeHandOver
{
    mifx_composite_attribs  attribs{}; // what chain_composite would have launched
    mifx::TaaFusedComposite fused{nullptr, nullptr};
};
static mifx_status chain_composite(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* radiance, const mifx_image2d* spec, const mifx_image2d* ssao_out,
                                   const mifx_image2d* comp, CompositeHandOver& hand)
{
    mifx_postfx* ctx = chain->ctx;
    mifx_ssr*    ssr = chain->ssr;
    mifx_image2d ssr_out{};
    const bool fused = ssr->cleanup_pending; // (set by an execute that deferred the pass)
    if (!fused) MIFX_CHECK(mifx_ssr_get_output(ssr, &ssr_out));
    const ChainGBuffer gb = chain_gbuffer(chain, f);
    mifx_composite_attribs ca{radiance, spec, fused ? radiance /* not read */ : &ssr_out, ssao_out, gb.normal, gb.base_color, gb.material, f->ibl->brdf_lut,
                              f->curr_camera, f->ssr_scale, f->ssao_scale, nullptr, f->ave_log_lum};
    if (chain->has_selection) return chain_selection_composite(chain, f, ca, comp, fused ? &ssr->cleanup_in : nullptr); // (a pass of its own, also with fuse_composite_taa)
    if (!fused) return mifx_composite_execute(ctx, &ca, comp);
    if (chain->fuse_composite_taa && chain->taa->technique_ready)
    {
        hand.attribs = ca;
        hand.fused   = mifx::TaaFusedComposite{&hand.attribs, &ssr->cleanup_in};
        return MIFX_OK;
    }
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "composite_ssr_cleanup_kernel");
    const Rows rows = ctx->needed_rows(int(comp->height));
    return launch_composite(ctx->stream, ca, comp, rows.b, rows.e, &ssr->cleanup_in);
}
// TemporalAntiAliasing::Execute on the jittered composite (:871-897) -- on the plane, or with the composite evaluated in place (above)
static mifx_status chain_taa(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* comp, const CompositeHandOver& hand)
{
    // a selected prim other than the previous frame's resets the accumulation (HnProcessSelectionTask.cpp:293-300)
    mifx_taa_attribs taa_attribs{};
    if (chain->has_selection && f->taa != nullptr)
    {
        taa_attribs = *f->taa;
        if (chain->selection_attribs.selection_id != chain->last_selection_id) taa_attribs.ResetAccumulation = 1;
        chain->last_selection_id = chain->selection_attribs.selection_id;
    }
    mifx_taa_render_attribs ta{chain->ctx, comp, chain->has_selection && f->taa != nullptr ? &taa_attribs : f->taa};
    return chain->taa->run(&ta, hand.fused.attribs ? &hand.fused : nullptr);
}

// DepthOfField::Execute on the TAA output (:899-909; m_UseDOF requires TAA, :654), on the rows the context needs: `taa_out` becomes its output
static mifx_status chain_depth_of_field(mifx_chain* chain, const mifx_chain_frame* f, mifx_image2d* taa_out)
{
    if (!chain->dof) return MIFX_OK;
    MIFX_CHECK(mifx_dof_prepare(chain->dof, chain->ctx, chain->dof_flags));
    mifx_dof_render_attribs da{chain->ctx, taa_out, f->gbuffer.depth, &chain->dof_attribs};
    MIFX_CHECK(mifx_dof_execute(chain->dof, &da));
    return mifx_dof_get_output(chain->dof, taa_out);
}

// The frame's last draw, the copy-frame pass on the Bloom output (HnPostProcessTask.cpp:920-926): ToneMap (+ sRGB) into the target's own format, with the coordinate grid
// (mifx_chain_set_coordinate_grid, HnCopyFrame.psh:27-63: on the G-buffer depth and the frame's camera, on the rows the context needs -- whole-frame pixel coordinates and a
// depth plane every rank holds whole, so a row band equals the rows of the unsharded frame), or plain.  With auto exposure on, fAveLogLum is the adapted average luminance.
static mifx_status chain_copy_frame(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* bloom_out, const mifx_image2d* out_ldr, const mifx_native_image* out_native)
{
    mifx_postfx* ctx = chain->ctx;
    if (out_native != nullptr)
    {
        // the copy-frame target in its own format (the swap chain's in the reference): the conversion is the tail of the tone-map kernel
        MIFX_REQUIRE(chain->auto_exposure == nullptr, "mifx_chain_execute_native: not combined with auto exposure");
        MIFX_REQUIRE(!chain->has_grid, "mifx_chain_execute_native: not combined with the coordinate grid");
        return mifx_tonemap_execute_native(ctx, bloom_out, out_native, f->tone_mapping, f->ave_log_lum, f->tonemap_flags);
    }
    if (chain->has_grid)
        return copy_frame_grid_run(ctx, bloom_out, f->gbuffer.depth, f->curr_camera, f->tone_mapping, f->ave_log_lum, f->tonemap_flags, chain->auto_exposure, chain->grid_attribs,
                                   chain->grid_flags, out_ldr, "mifx_chain_execute");
    if (chain->auto_exposure) return mifx_tonemap_execute_auto(ctx, bloom_out, out_ldr, f->tone_mapping, chain->auto_exposure, f->tonemap_flags);
    return mifx_tonemap_execute(ctx, bloom_out, out_ldr, f->tone_mapping, f->ave_log_lum, f->tonemap_flags);
}

// Bloom::Execute on the TAA (or depth-of-field) output (HnPostProcessTask.cpp:911-918) and the copy-frame draw
static mifx_status chain_bloom_and_tone_map(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d& taa_out, const mifx_image2d* out_ldr, const mifx_native_image* out_native,
                                            hipEvent_t between)
{
    mifx_postfx* ctx = chain->ctx;
    mifx_image2d bloom_out;
    mifx_bloom_render_attribs ba{ctx, &taa_out, f->bloom};
    // With a plain fp32 target and a constant average luminance the copy-frame ToneMap() (:920-926) is the tail of Bloom's final up-sample: the Bloom output
    // is written as always, the LDR frame in the same pass (bit-identical to the two passes; the "tonemap" stage time is then part of "bloom").
    // (with the coordinate grid the frame's last pass is the copy-frame draw with the grid, which reads the Bloom output and the depth: not fused either)
    const bool fuse_tone_map = out_native == nullptr && chain->auto_exposure == nullptr && chain->fuse_tone_map && !chain->has_grid;
    const mifx_bloom::FusedToneMap ftm{out_ldr, f->tone_mapping, f->ave_log_lum, f->tonemap_flags, chain->fuse_bloom_output};
    MIFX_REQUIRE(chain->bloom->prepared, "mifx_chain_execute: bloom resources are not prepared");
    MIFX_CHECK(chain->bloom->run(&ba, 0, fuse_tone_map ? &ftm : nullptr, mifx_bloom::Request{}));
    if (between) MIFX_HIP_CHECK(hipEventRecord(between, ctx->stream));
    if (fuse_tone_map) return MIFX_OK; // (the frame is written; the Bloom output plane on demand, mifx_bloom::run_deferred_output)
    MIFX_CHECK(mifx_bloom_get_output(chain->bloom, &bloom_out));
    if (out_native == nullptr && chain->auto_exposure) MIFX_CHECK(mifx_autoexposure_execute(chain->auto_exposure, &bloom_out, chain->ae_elapsed, chain->ae_adapt ? 1 : 0));
    return chain_copy_frame(chain, f, &bloom_out, out_ldr, out_native);
}

// HnPostProcessTask::Prepare: per-frame PrepareResources in the order PostFX, SSAO, SSR, TAA, Bloom (:671-682), then the chain's own planes
extern "C++" mifx_status mifx::chain_prepare_resources(mifx_chain* chain, const mifx_chain_frame* f)
{
    mifx_postfx* ctx = chain->ctx;
    const uint32_t W = f->frame.Width, H = f->frame.Height;
    MIFX_CHECK(mifx_postfx_prepare(ctx, &f->frame, chain->postfx_flags));
    MIFX_CHECK(mifx_ssao_prepare(chain->ssao, ctx, chain->ssao_flags));
    MIFX_CHECK(mifx_ssr_prepare(chain->ssr, ctx, chain->ssr_flags));
    MIFX_CHECK(mifx_taa_prepare(chain->taa, ctx, f->taa_feature_flags));
    MIFX_CHECK(mifx_bloom_prepare(chain->bloom, ctx, 0));
    MIFX_CHECK(chain->radiance.alloc(W, H, MIFX_FORMAT_F32X4));
    MIFX_CHECK(chain->specular_ibl.alloc(W, H, MIFX_FORMAT_F32X4));
    MIFX_CHECK(chain->composite.alloc(W, H, MIFX_FORMAT_F32X4));
    mifx_chain::ShadeStage& sh = chain->shade;
    if (sh.targets_on)
        for (mifx::Plane& p : sh.targets) MIFX_CHECK(p.alloc(W, H, MIFX_FORMAT_F32X4)); // (once per size; freed with the chain)
    if (!sh.transparent.empty())
    {
        // every refusal of the frame's transparent draws before its first launch: the planes of every slice against the frame's size, what mifx_oit_shade_blend refuses
        MIFX_REQUIRE(sh.targets_on && chain->band.empty(), "mifx_chain_execute: transparency needs mifx_chain_set_shade_output with write_targets and no row band");
        sh.frame_targets();
        const mifx_image2d     radiance = chain->radiance.desc();
        const mifx_oit_targets tg       = sh.oit_targets(&radiance);
        for (const mifx::KeptTransparentSlice& t : sh.transparent)
            MIFX_CHECK(mifx_oit_shade_blend_check(W, H, ctx->flags, &t.s, f->gbuffer.depth, f->curr_camera, f->pbr, f->ibl, sh.shadows(), &tg));
        if (sh.oit == nullptr || sh.oit->w != W || sh.oit->h != H || sh.oit->K != sh.oit_layer_count)
        {
            mifx_oit_destroy(sh.oit); // (hipFree waits for the kernels that still read it)
            sh.oit = nullptr;
            MIFX_CHECK(mifx_oit_create(ctx, W, H, sh.oit_layer_count, &sh.oit));
        }
        if (!g_transparency_fusion)
        {
            MIFX_CHECK(sh.slice_radiance.alloc(W, H, MIFX_FORMAT_F32X4));
            MIFX_CHECK(sh.slice_specular_ibl.alloc(W, H, MIFX_FORMAT_F32X4));
        }
    }
    return MIFX_OK;
}

// The render attribs of PostFX prep, SSR and SSAO for this frame (`radiance`: the caller's descriptor of the shaded colour, which SSR reads)
struct FrameAttribs
{
    mifx_postfx_render_attribs pa;
    mifx_ssr_render_attribs    sr;
    mifx_ssao_render_attribs   sa;
};
static FrameAttribs chain_frame_attribs(const mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* radiance)
{
    mifx_postfx* ctx = chain->ctx;
    const ChainGBuffer gb = chain_gbuffer(chain, f);
    return {{f->gbuffer.depth, f->prev_depth, f->motion, f->curr_camera, f->prev_camera},
            {ctx, radiance, f->gbuffer.depth, gb.normal, gb.material, f->motion, f->ssr},
            {ctx, f->gbuffer.depth, gb.normal, f->ssao}};
}

// Creates the chain's extra streams and events on first use.
extern "C++" mifx_status mifx::chain_make_lanes(mifx_chain* chain, int lanes)
{
    if (!chain->side)
    {
        // (a stream priority for the second stream was measured: lowest 1.713-1.723 ms, highest 1.728-1.736 ms, default 1.701-1.703 ms per 4K frame in mode 2)
        MIFX_HIP_CHECK(hipStreamCreateWithFlags(&chain->side, hipStreamNonBlocking));
        for (hipEvent_t* e : {&chain->evFork, &chain->evPrep, &chain->evSsao, &chain->evPrepConsumed, &chain->evJoinS, &chain->evShade}) MIFX_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    if (lanes >= 3 && !chain->lane_x)
    {
        MIFX_HIP_CHECK(hipStreamCreateWithFlags(&chain->lane_x, hipStreamNonBlocking));
        for (hipEvent_t* e : {&chain->evBloomDone, &chain->evJoinX, &chain->evXEnd[0], &chain->evXEnd[1], &chain->evSsrDone}) MIFX_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    if (lanes >= 4 && !chain->lane_h)
    {
        MIFX_HIP_CHECK(hipStreamCreateWithFlags(&chain->lane_h, hipStreamNonBlocking));
        for (hipEvent_t* e : {&chain->evHiz, &chain->evJoinH}) MIFX_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return MIFX_OK;
}

// Whether the lanes of this frame may start behind the previous frame's events alone: the previous frame recorded them, and the library queued nothing on the context
// stream since (history fills of a reset or of a re-allocating prepare, history imports, a new stream: mifx_postfx::stream_epoch).  Otherwise every lane is ordered
// behind the context stream once.
static bool chain_lanes_continue(mifx_chain* chain)
{
    const bool cont = chain->prep_consumed && chain->seen_epoch == chain->ctx->stream_epoch;
    chain->prep_consumed = false; // (set again by a frame that got as far as recording the event: an error return leaves it off)
    return cont;
}
extern "C++" mifx_status mifx::chain_fork_lanes(mifx_chain* chain, std::initializer_list<LaneEvent> lanes, bool across_frames)
{
    const bool cont = chain_lanes_continue(chain) && across_frames; // (in this order: a frame that may not continue clears prep_consumed as well)
    if (!cont) MIFX_HIP_CHECK(hipEventRecord(chain->evFork, chain->ctx->stream));
    for (const LaneEvent& l : lanes)
        if (l.lane != nullptr && (!cont || l.ev != nullptr)) MIFX_HIP_CHECK(hipStreamWaitEvent(l.lane, cont ? l.ev : chain->evFork, 0));
    return MIFX_OK;
}

// mifx_chain_set_overlap 3: one frame as three lanes that slide against each other across frames.  The frame's kernels fall into three resource classes --
//   lane S (side stream):    PBR shade (+ R2), PostFX prep, Hi-Z (R1), SSAO A2 .. A8      vector-ALU bound (shade, A3) + their small pyramids
//   lane X (second stream):  SSR R4 .. R6, composite (+ R7), TAA, depth of field          latency / bandwidth bound (the ray march waits 73 % of its cycles)
//   lane M (context stream): Bloom pyramid + final pass (+ tone map)                     ~15 small dependent launches
// -- and a lane only waits for what it reads:  X for the Hi-Z of S (hence shade + prep), the composite for S's SSAO, M for X's TAA / depth of field; the next frame's S for
// this frame's last reader of the planes S overwrites (= the end of X), the next frame's X follows this frame's X in stream order, and before TAA it waits for the
// previous frame's Bloom (the reader of the accumulation buffer / depth-of-field output it is about to overwrite).  So the ray march of frame N runs beside A3 of
// frame N (both need wave slots of every SIMD: the march leaves the ALUs idle, A3 fills them), and the Bloom pyramid of frame N beside the shade of frame N + 1.
// Same kernels, same arguments, same results as one stream; the input contract is that of mode 2 (a frame's input planes are complete when execute is called).
// The context stream ends the frame behind all three lanes: work queued on it after the call sees the whole frame.
//
// mifx_chain_set_overlap 4 (round 5): the same lanes with TWO frames in flight.  In mode 3 lane S of frame N + 1 waits for the end of lane X of frame N, so R5, R6, the
// composite and TAA of every frame -- 0.46 ms of mostly bandwidth-bound work -- run with nothing beside them (profiles/r04_overlap_stats_v17.txt: one kernel in flight
// 67 % of the time).  Here S of frame N + 1 waits for the end of X of frame N - 1 and so runs beside X of frame N.  What S writes and X reads -- radiance, specular IBL,
// SSR's roughness / mask / depth hierarchy, the PostFX planes and the blue noise -- exists twice: the chain trades those planes with its `shadow` set at the start of
// every frame (kernels already queued hold the old addresses by value; the effect objects allocate, fill and hand out "their" planes as always).  Everything else is
// either private to a lane (stream order) or a ping-pong by FrameDesc.Index, which is two deep already -- provided the indices are consecutive: a frame whose index
// does not follow its predecessor's waits for the end of X of the previous frame like mode 3.
static void chain_swap_shadow(mifx_chain* chain)
{
    mifx_postfx* ctx = chain->ctx;
    mifx_ssr*    ssr = chain->ssr;
    mifx_chain::Shadow& sh = chain->shadow;
    chain->radiance.swap(sh.radiance);
    chain->specular_ibl.swap(sh.specular_ibl);
    if (chain->shade.targets_on)
        for (int i = 0; i < 4; ++i) chain->shade.targets[i].swap(sh.targets[i]);
    ctx->reproj_depth.swap(sh.reproj_depth);
    ctx->closest_motion.swap(sh.closest_motion);
    ctx->noise_xy.swap(sh.noise_xy);
    ctx->noise_zw.swap(sh.noise_zw);
    ctx->prev_depth16.swap(sh.prev_depth16);
    ssr->roughness.swap(sh.roughness);
    ssr->mask.swap(sh.mask);
    for (int k = 0; k < mifx_ssr::kMips; ++k) ssr->hiz[k].swap(sh.hiz[k]);
    ssr->hiz_slab.swap(sh.hiz_slab);
}
// the shadow set mirrors the geometry of the live one (after the frame's prepare calls)
static mifx_status chain_prepare_shadow(mifx_chain* chain)
{
    mifx_postfx* ctx = chain->ctx;
    mifx_ssr*    ssr = chain->ssr;
    mifx_chain::Shadow& sh = chain->shadow;
    MIFX_CHECK(sh.radiance.alloc_like(chain->radiance));
    MIFX_CHECK(sh.specular_ibl.alloc_like(chain->specular_ibl));
    if (chain->shade.targets_on)
        for (int i = 0; i < 4; ++i) MIFX_CHECK(sh.targets[i].alloc_like(chain->shade.targets[i]));
    MIFX_CHECK(sh.reproj_depth.alloc_like(ctx->reproj_depth));
    MIFX_CHECK(sh.closest_motion.alloc_like(ctx->closest_motion));
    MIFX_CHECK(sh.noise_xy.alloc_like(ctx->noise_xy));
    MIFX_CHECK(sh.noise_zw.alloc_like(ctx->noise_zw));
    MIFX_CHECK(sh.prev_depth16.alloc_like(ctx->prev_depth16));
    MIFX_CHECK(sh.roughness.alloc_like(ssr->roughness));
    MIFX_CHECK(sh.mask.alloc_like(ssr->mask));
    if (sh.hiz[0].data == nullptr || sh.hiz[0].w != ssr->hiz[0].w || sh.hiz[0].h != ssr->hiz[0].h) MIFX_CHECK(mifx::ssr_alloc_hiz(ssr->w, ssr->h, sh.hiz, sh.hiz_slab));
    return MIFX_OK;
}

// MIFX_LANE_EDGES / mifx_chain_set_lane_edges: at the launch site of a named kernel (mifx_postfx::kernel_hook, called by MifxKernelTimer on the lane's stream)
//   end:   record "kernel `name` of frame seq is done" when an edge names it as a signal
//   begin: wait for the signals of the edges that name it as the waiter, if that frame recorded them
static void chain_kernel_hook(mifx_chain* chain, const char* name, bool begin)
{
    const hipStream_t s = chain->ctx->stream;
    for (const mifx_chain::Edge& e : chain->edges)
    {
        if (begin && e.waiter == name)
        {
            auto it = chain->signals.find(e.signal);
            if (it == chain->signals.end() || chain->seq < uint64_t(e.delta)) continue;
            const uint64_t want = chain->seq - uint64_t(e.delta);
            if (it->second.seq[want & 3u] == want) (void)hipStreamWaitEvent(s, it->second.ev[want & 3u], 0);
        }
        else if (!begin && e.signal == name)
        {
            mifx_chain::Signal& sg = chain->signals[e.signal];
            hipEvent_t& ev = sg.ev[chain->seq & 3u];
            if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) continue;
            if (sg.seq[chain->seq & 3u] == chain->seq) continue; // (one record per frame: the first launch of that name)
            if (hipEventRecord(ev, s) == hipSuccess) sg.seq[chain->seq & 3u] = chain->seq;
        }
    }
}

// mifx_chain_set_overlap 5 (round 6): mode 4 with the frame's bandwidth-bound tail -- the composite, TAA, depth of field -- on lane M in front of Bloom instead of at the end
// of lane X.  In mode 4 the march of frame N + 1 follows TAA of frame N in stream order, so the composite and TAA still run with little beside them (profiles/
// r06_overlap_stats_v11.txt: 49 % and 42 % of their time alone); here lane X of a frame is R4 .. R6 only, and the next frame's march runs beside this frame's composite and TAA:
//   S  shade, prep, Hi-Z, SSAO   |   X  R4, R5, R6   |   M  composite (+ R7), TAA, depth of field, Bloom, tone map        (0.67 / 0.52 / 0.51 ms of kernels at 4K)
// What the composite and TAA read of lanes S and X is either double-buffered already (mode 4's shadow set: radiance, specular IBL, roughness, mask, the PostFX planes) or a
// ping-pong by FrameDesc.Index (SSR's and SSAO's histories: frame N + 1 writes the other slot, frame N + 2 -- whose lane S waits for this frame's TAA -- the same one).
static mifx_status chain_execute_lanes(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* out_ldr, const mifx_native_image* out_native, int mode)
{
    const bool pipelined = mode >= 4, late = mode >= 5;
    mifx_postfx*      ctx = chain->ctx;
    const hipStream_t M   = ctx->stream;
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MIFX_CHECK(chain_make_lanes(chain, 3));
    const hipStream_t S = chain->side, X = chain->lane_x;
    if (pipelined)
    {
        MIFX_CHECK(chain_prepare_shadow(chain));
        chain_swap_shadow(chain); // this frame's set = the one the frame before the previous frame used
    }
    const auto [radiance, spec, comp] = chain_frame_planes(chain);
    LaneJoin join{chain, M, {S, chain->evJoinS}, {X, chain->evJoinX}}; // (the regular path joins through evSsao -> evPrepConsumed)
    const uint64_t k = chain->seq;
    // lane S continues behind the last reader of what it overwrites: the end of lane X of the previous frame -- or, two frames in flight, of the frame before that one
    const bool deep = pipelined && k >= 2 && f->frame.Index == chain->last_index + 1u;
    MIFX_CHECK(chain_fork_lanes(chain, {{S, deep ? chain->evXEnd[k & 1u] : chain->evPrepConsumed}, {X, nullptr}})); // (evXEnd[k & 1] still holds frame k - 2's record)
    if (pipelined && !chain->edges.empty()) ctx->kernel_hook = [chain](const char* name, bool begin) { chain_kernel_hook(chain, name, begin); };
    const auto [pa, sr, sa] = chain_frame_attribs(chain, f, &radiance);
    // lane S: shade, prep
    ctx->stream = S;
    MIFX_CHECK(chain_shade(chain, f, &radiance, &spec));
    MIFX_CHECK(mifx_postfx_execute(ctx, &pa));
    // lane X: SSR, its depth hierarchy on S (X waits for evPrep behind it, i.e. for the shade, the prep pass and the hierarchy)
    // (round 5, measured and not kept: the prep pass and the hierarchy -- 68 us of streaming over the inputs -- on a fourth stream beside the shade, as the sharded frame does
    //  with its whole-frame hierarchy: 1.6358 against 1.6418 ms over three alternating pairs of runs on one box, inside the noise; order-checked by tests/cpu_product/order.py)
    ctx->stream = X;
    // (mode 5 with R7 as a pass of its own -- fusion bit 2 off: R7 of this frame overwrites the SSR output plane the PREVIOUS frame's composite, now on lane M, may still be
    //  reading; found by tests/cpu_product/order.py.  That configuration waits for the previous frame's composite / TAA here; with R7 inside the composite there is no such plane)
    if (late && !chain->fuse_ssr_cleanup) MIFX_HIP_CHECK(hipStreamWaitEvent(X, chain->evPrepConsumed, 0));
    MIFX_CHECK(chain->ssr->run(&sr, mifx_ssr::Request{chain->fuse_ssr_cleanup, S, chain->evPrep}));
    // lane S: SSAO
    ctx->stream = S;
    MIFX_CHECK(mifx_ssao_execute(chain->ssao, &sa));
    MIFX_HIP_CHECK(hipEventRecord(chain->evSsao, S));
    // lane X (mode 5: lane M, behind this frame's SSR): composite, TAA, depth of field
    const hipStream_t T = late ? M : X;
    if (late)
    {
        MIFX_HIP_CHECK(hipEventRecord(chain->evSsrDone, X));
        MIFX_HIP_CHECK(hipStreamWaitEvent(M, chain->evSsrDone, 0));
    }
    ctx->stream = T;
    MIFX_HIP_CHECK(hipStreamWaitEvent(T, chain->evSsao, 0));
    mifx_image2d ssao_out, taa_out;
    CompositeHandOver hand;
    MIFX_CHECK(mifx_ssao_get_output(chain->ssao, &ssao_out));
    MIFX_CHECK(chain_composite(chain, f, &radiance, &spec, &ssao_out, &comp, hand));
    if (!late) MIFX_HIP_CHECK(hipStreamWaitEvent(X, chain->evBloomDone, 0)); // (recorded by the previous frame; never recorded = no wait.  Mode 5: the previous Bloom is earlier on this stream)
    MIFX_CHECK(chain_taa(chain, f, &comp, hand));
    MIFX_CHECK(mifx_taa_get_output(chain->taa, 0, &taa_out));
    MIFX_CHECK(chain_depth_of_field(chain, f, &taa_out));
    MIFX_HIP_CHECK(hipEventRecord(chain->evPrepConsumed, T));
    if (pipelined) MIFX_HIP_CHECK(hipEventRecord(chain->evXEnd[k & 1u], T));
    // lane M: Bloom, tone map
    ctx->stream = M;
    if (!late) MIFX_HIP_CHECK(hipStreamWaitEvent(M, chain->evPrepConsumed, 0));
    join.joined = true;
    MIFX_CHECK(chain_bloom_and_tone_map(chain, f, taa_out, out_ldr, out_native, nullptr));
    MIFX_HIP_CHECK(hipEventRecord(chain->evBloomDone, M));
    chain->seen_epoch    = ctx->stream_epoch;
    chain->prep_consumed = true;
    chain->timed         = false;
    chain->last_index    = f->frame.Index;
    if (pipelined) ++chain->seq;
    return MIFX_OK;
}

static mifx_status chain_execute_impl(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* out_ldr, const mifx_native_image* out_native)
{
    MIFX_REQUIRE(chain != nullptr && f != nullptr && (out_ldr != nullptr) != (out_native != nullptr), "mifx_chain_execute: null argument");
    MIFX_CHECK(chain_check_frame(f, "mifx_chain_execute"));
    mifx_postfx* ctx = chain->ctx;
    MIFX_CHECK(mifx::chain_prepare_resources(chain, f));
    if (chain->overlap >= 3 && !chain->profiling) return chain_execute_lanes(chain, f, out_ldr, out_native, chain->overlap);
    const auto [radiance, spec, comp] = chain_frame_planes(chain);
    int stage = 0;
    auto mark = [&]() -> mifx_status {
        if (chain->profiling) MIFX_HIP_CHECK(hipEventRecord(chain->ev[stage], ctx->stream));
        ++stage;
        return MIFX_OK;
    };
    MIFX_CHECK(mark());

    const auto [pa, sr, sa] = chain_frame_attribs(chain, f, &radiance);
    const bool        two  = chain->overlap && !chain->profiling;
    const hipStream_t main = ctx->stream;
    if (two) MIFX_CHECK(chain_make_lanes(chain, 2));
    // (the regular path joins through evPrep / evSsao; it says so in front of Bloom, as the three lanes do: an error return after the fork leaves `main` behind the side stream)
    LaneJoin join{chain, main, {two ? chain->side : nullptr, chain->evJoinS}};
    if (two)
    {
        // Two dependency chains:  shade -> SSR (needs the radiance and the prep outputs)   |   prep -> SSAO (depth / normals only).
        // The second one is recorded on the side stream; the launch stream joins before the composite.  Same kernels, same results.
        // Across frames (overlap 2; the caller guarantees that the frame's input planes are complete when execute is called): the side stream does not wait for the
        // previous frame's Bloom and tone map, only for its last reader of what prep and SSAO overwrite (the PostFX planes and the blue noise: SSR, TAA, depth of field),
        // so that the next frame's prep + SSAO fill the GPU under the small launches of the Bloom pyramid.
        // (Measured and dropped: the PostFX planes double-buffered so that the second stream may run a whole frame ahead, beside this frame's ray march and TAA
        //  instead of its Bloom: 1.744 vs 1.742 ms; Bloom and the tone map of the frame on the second stream as well, so that both streams are busy all the time:
        //  1.706 / 1.720 vs 1.708 / 1.704 ms.  The gain of running two kernels at once saturates at ~5.6 %, which is also what two whole chains on two streams reach
        //  (tools/exp_two_chains.py).  tools/overlap_stats.py shows what runs beside what: profiles/r03_overlap_stats.txt.)
        // (only while nothing else was queued on the context stream in between -- a reset's or a re-allocating prepare's history fills, an import: chain_lanes_continue)
        MIFX_CHECK(chain_fork_lanes(chain, {{chain->side, chain->evPrepConsumed}}, chain->overlap >= 2));
        // (with the shade's targets on, SSAO reads the normal target: the shade is then queued first and SSAO waits for it; prep still runs beside it)
        const bool ssao_reads_shade = chain_shade_kind(chain, f) == Shade::OutputTargets;
        if (ssao_reads_shade)
        {
            MIFX_CHECK(chain_shade(chain, f, &radiance, &spec));
            MIFX_HIP_CHECK(hipEventRecord(chain->evShade, main));
        }
        ctx->stream = chain->side;
        MIFX_CHECK(mifx_postfx_execute(ctx, &pa));
        MIFX_HIP_CHECK(hipEventRecord(chain->evPrep, chain->side));
        if (ssao_reads_shade) MIFX_HIP_CHECK(hipStreamWaitEvent(chain->side, chain->evShade, 0));
        MIFX_CHECK(mifx_ssao_execute(chain->ssao, &sa));
        MIFX_HIP_CHECK(hipEventRecord(chain->evSsao, chain->side));
        ctx->stream = main;
        if (!ssao_reads_shade) MIFX_CHECK(chain_shade(chain, f, &radiance, &spec)); // (measured: the shade on the side stream as well, in front of prep, changes nothing: 1.747 vs 1.751 ms)
        MIFX_HIP_CHECK(hipStreamWaitEvent(main, chain->evPrep, 0));
        MIFX_CHECK(chain->ssr->run(&sr, mifx_ssr::Request{chain->fuse_ssr_cleanup}));
        MIFX_HIP_CHECK(hipStreamWaitEvent(main, chain->evSsao, 0));
        stage += 4;
    }
    else
    {
        // forward shade (stands in for HnRenderRprimsTask: SceneColor + the IBL target of the USD G-buffer)
        MIFX_CHECK(chain_shade(chain, f, &radiance, &spec));
        MIFX_CHECK(mark());
        // PostFXContext::Execute (:788-809)
        MIFX_CHECK(mifx_postfx_execute(ctx, &pa));
        MIFX_CHECK(mark());
        // ScreenSpaceReflection::Execute (:811-822)
        MIFX_CHECK(chain->ssr->run(&sr, mifx_ssr::Request{chain->fuse_ssr_cleanup}));
        MIFX_CHECK(mark());
        // ScreenSpaceAmbientOcclusion::Execute (:824-832)
        MIFX_CHECK(mifx_ssao_execute(chain->ssao, &sa));
        MIFX_CHECK(mark());
    }
    mifx_image2d ssao_out, taa_out;
    CompositeHandOver hand;
    MIFX_CHECK(mifx_ssao_get_output(chain->ssao, &ssao_out));
    // composite draw (:834-869), no tone mapping while TAA is on
    MIFX_CHECK(chain_composite(chain, f, &radiance, &spec, &ssao_out, &comp, hand));
    MIFX_CHECK(mark());
    // TemporalAntiAliasing::Execute on the jittered composite (:871-897)
    MIFX_CHECK(chain_taa(chain, f, &comp, hand));
    MIFX_CHECK(mifx_taa_get_output(chain->taa, 0, &taa_out));
    MIFX_CHECK(mark());
    MIFX_CHECK(chain_depth_of_field(chain, f, &taa_out));
    chain->prep_consumed = false;
    if (chain->overlap >= 2 && !chain->profiling && chain->evPrepConsumed)
    {
        MIFX_HIP_CHECK(hipEventRecord(chain->evPrepConsumed, ctx->stream));
        chain->seen_epoch    = ctx->stream_epoch;
        chain->prep_consumed = true;
    }
    MIFX_CHECK(mark());
    join.joined = true;
    MIFX_CHECK(chain_bloom_and_tone_map(chain, f, taa_out, out_ldr, out_native, chain->profiling ? chain->ev[stage] : nullptr)); // (the stage mark between the two)
    ++stage;
    MIFX_CHECK(mark());
    chain->timed = chain->profiling;
    return MIFX_OK;
}

extern "C" mifx_status mifx_chain_execute(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* out_ldr)
{
    MIFX_REQUIRE(out_ldr != nullptr, "mifx_chain_execute: null output");
    if (chain != nullptr && (chain->halo_ssao_pending || chain->halo_rest_pending)) chain->join_halos(); // (an unsharded frame after sharded ones writes whole history planes)
    return chain_execute_impl(chain, f, out_ldr, nullptr);
}
extern "C" mifx_status mifx_chain_execute_native(mifx_chain* chain, const mifx_chain_frame* f, const mifx_native_image* out_native)
{
    MIFX_REQUIRE(out_native != nullptr, "mifx_chain_execute_native: null output");
    MIFX_REQUIRE(chain == nullptr || !chain->has_grid, "mifx_chain_execute_native: not combined with the coordinate grid (mifx_chain_set_coordinate_grid)");
    if (chain != nullptr && (chain->halo_ssao_pending || chain->halo_rest_pending)) chain->join_halos();
    return chain_execute_impl(chain, f, nullptr, out_native);
}

// ------------------------------------------------------------------------------------------------ row-band sharding
namespace
{
struct ShardRows
{
    Rows band, taa, comp, prep; // rows of the final image owned; rows TAA / composite (= shade, SSR, SSAO outputs) / PostFX prep are computed on
    Rows post;                  // rows of Bloom's input (the TAA output, or the depth-of-field output computed from it) that Bloom and the final pass read
    Rows need;                  // rows of the Bloom output computed: the band, plus one row either side when auto exposure samples it (bilinear footprints
                                // of the low-resolution luminance rows this rank writes, mifx_autoexposure::sample_rows)
};
// Reaches: Bloom's fine levels read the TAA output on mifx_bloom::Plan::taa; TAA reads the 3x3 neighbourhood of the composite; SSAO and SSR
// derive their internal windows from the rows of their output (api_ssao.cpp, api_ssr.cpp) and need the prep outputs on the largest of them
// (<= 1 + radius 4 + 1 + 48 + 15 alignment (mifx_ssao::kWindowAlign; 31 until round 5) + 1 rows beyond the composite rows: 96 is checked by both effects against prep_rows).
} // namespace
extern "C++" bool mifx::shard_bloom_halo_enabled() // MIFX_SHARD_BLOOM_HALO=0: round 5's frame (every rank produces the level-0 rows it reads)
{
    // (read per frame, not once: tests/test_gpu_sharded.py holds mifx_chain_execute_band to the phases driven one by one, which have no such exchange, in the same process
    //  as the tests of the exchange)
    const char* e = std::getenv("MIFX_SHARD_BLOOM_HALO");
    return e == nullptr || std::atoi(e) != 0;
}
namespace
{
ShardRows shard_rows(const mifx_chain* chain, const mifx_chain_frame* f, Rows band, bool halo_level0)
{
    const int H = int(f->frame.Height);
    ShardRows r;
    r.band = rows_clip(band, H);
    r.need = chain->auto_exposure ? rows_expand(r.band, 1, H) : r.band;
    const mifx_bloom::Plan p = chain->bloom->make_plan(r.band, r.need, chain->bloom->mip_count(*f->bloom), halo_level0);
    r.post = p.G >= 0 ? rows_hull(p.taa, r.need) : Rows{0, H};
    r.taa  = r.post;
    // depth of field sits between TAA and Bloom: its output on r.post needs the TAA output on the colour rows of mifx_dof::windows (bokeh gather and fill radii)
    if (chain->dof) r.taa = mifx_dof::windows(chain->dof_attribs, r.post, int(f->frame.Width), H).colour;
    r.comp = rows_expand(r.taa, 1, H);
    r.prep = rows_expand(r.comp, 96, H);
    // (its colour-independent passes -- CoC, temporal CoC, dilation, blur -- run whole on every rank: the temporal CoC reads the closest motion vectors of the whole frame)
    if (chain->dof && (chain->dof_flags & MIFX_DOF_FEATURE_FLAG_ENABLE_TEMPORAL_SMOOTHING)) r.prep = Rows{0, H};
    return r;
}
} // namespace

extern "C" mifx_status mifx_chain_set_row_band(mifx_chain* chain, int32_t row_begin, int32_t row_end, int32_t max_motion_rows)
{
    MIFX_REQUIRE(chain != nullptr && row_begin >= 0 && row_end >= row_begin && max_motion_rows >= 0, "mifx_chain_set_row_band: bad argument");
    MIFX_REQUIRE(row_end == row_begin || !chain->shade.output_stage(),
                 "mifx_chain_set_row_band: a row band (or sharding) is not combined with mifx_chain_set_shade_output: the sharded hit fetch has no output stage or footer");
    chain->band       = Rows{row_begin, row_end}; // {0, 0} switches sharding off
    chain->max_motion = max_motion_rows;
    chain->ctx->band  = chain->band;
    chain->ctx->max_motion = max_motion_rows;
    if (chain->band.empty()) chain->ctx->need = Rows{0, 0};
    return MIFX_OK;
}

// One frame in four phases; between them the caller exchanges planes with the other ranks (diligentfx_amd/sharded.py: ShardedChain):
//   phase 0: PBR shade on the composite rows
//   phase 1: PostFX prep, SSAO
//   phase 2: SSR, composite, TAA, Bloom fine levels        -> "bloom_gather": every rank contributes the rows it owns, all ranks get the level
//            (the rays of SSR hit anywhere in the frame: the colour at a hit outside the rows of phase 0 is shaded on the spot -- no radiance exchange)
//   phase 3: Bloom coarse levels + up-sampling, tone map   -> halo exchange of the five history planes for the next frame
// With auto exposure on, phase 3 ends with this rank's rows of the low-resolution luminance ("ae_low_res", rows ae_begin..ae_end of mifx_shard_info) instead of
// the tone map; those rows are all-gathered and
//   phase 4: luminance reduction + adaptation (the same 64x64 values in the same order on every rank: the average is bit-identical), tone map
// follows (without auto exposure phase 4 does nothing).
// (SSAO before SSR: the reference runs SSR first, but the two effects only share read-only inputs.)
// `req`: what mifx_chain_execute_sharded asks of this one call (mifx_objects.h); empty for a caller that drives the phases itself.
extern "C++" mifx_status mifx::chain_execute_phase(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* out_ldr, int32_t phase, const ChainPhaseRequest& req)
{
    MIFX_REQUIRE(chain != nullptr && f != nullptr && out_ldr != nullptr && phase >= 0 && phase <= 4, "mifx_chain_execute_phase: bad argument");
    MIFX_REQUIRE(!chain->band.empty(), "mifx_chain_execute_phase: no row band set (mifx_chain_set_row_band)");
    MIFX_REQUIRE(!chain->shade.output_stage(), "mifx_chain_execute_phase: a row band is not combined with mifx_chain_set_shade_output (the sharded hit fetch has no output stage or footer)");
    MIFX_CHECK(chain_check_frame(f, "mifx_chain_execute_phase"));
    mifx_postfx* ctx = chain->ctx;
    if (phase == 0) MIFX_CHECK(mifx::chain_prepare_resources(chain, f));
    const mifx_image2d radiance = chain->radiance.desc(), spec = chain->specular_ibl.desc(), comp = chain->composite.desc();
    const ShardRows r = shard_rows(chain, f, chain->band, req.bloom.halo_level0);
    struct NeedGuard // the row request is per call: never leave one behind for a later whole-frame call
    {
        mifx_postfx* c;
        ~NeedGuard() { c->need = Rows{0, 0}; }
    } guard{ctx};
    if (phase == 0)
    {
        ctx->need = r.comp;
        return chain_shade(chain, f, &radiance, &spec);
    }
    mifx_image2d ssao_out, taa_out, bloom_out;
    mifx_bloom_render_attribs ba{ctx, nullptr, f->bloom};
    const auto [pa, sr, sa] = chain_frame_attribs(chain, f, &radiance);
    // A history-halo exchange of the previous sharded frame that is still travelling (mifx_chain_execute_sharded, async_halos) is joined where this frame first reads the
    // plane -- also for a caller that mixes mifx_chain_execute_sharded frames with phases of its own.
    if (phase == 1 && chain->halo_ssao_pending)
    {
        MIFX_HIP_CHECK(hipStreamWaitEvent(ctx->stream, chain->evHaloSsao, 0)); // A5 reprojects into the ghost rows of last frame's AO / history length
        chain->halo_ssao_pending = false;
    }
    if (phase == 2 && chain->halo_rest_pending)
    {
        MIFX_HIP_CHECK(hipStreamWaitEvent(ctx->stream, chain->evHaloRest, 0)); // R6 and TAA reproject into the ghost rows of last frame's SSR / TAA histories
        chain->halo_rest_pending = false;
    }
    if (phase == 1)
    {
        ctx->need = r.prep;
        MIFX_CHECK(mifx_postfx_execute(ctx, &pa));
        if (req.sig_after_prep) MIFX_HIP_CHECK(hipEventRecord(req.sig_after_prep, ctx->stream)); // (the sharded frame's SSAO lane: SSR on the other lane waits for this)
        ctx->need = r.comp;
        return chain->ssao->run(&sa, req.ssao);
    }
    if (phase == 2)
    {
        ctx->need = r.comp;
        // No exchange of the shaded radiance: the ray march records where every ray hit, and the hit fetch loads the colour from the rows this rank shaded in
        // phase 0 or shades the hit pixel itself (the G-buffer and the IBL maps are whole on every rank; same kernel body, bit-identical colour).
        if (chain->shade.shaded_rows.empty() || chain->shade.shaded_frame != f->frame.Index)
        {
            set_error("mifx_chain_execute_phase: phase 2 of frame %u before its phase 0 (the hit fetch needs the rows that phase shaded)", f->frame.Index);
            return MIFX_ERR_INVALID_OP;
        }
        mifx_ssr::Request ssr_req{chain->fuse_ssr_cleanup, req.hiz_stream, req.hiz_done};
        ssr_req.after_trace = [chain, f, ctx, radiance, kind = chain_shade_kind(chain, f)](Img rays, Img coords) -> mifx_status {
            const mifx_chain::ShadeStage& sh       = chain->shade;
            const bool                    reversed = (ctx->flags & MIFX_POSTFX_FEATURE_FLAG_REVERSED_DEPTH) != 0;
            MIFX_HIP_CHECK(hipSetDevice(ctx->device));
            MifxKernelTimer timer(ctx, "pbr_hit_fetch_kernel");
            if (kind != Shade::Layered) // (the hit pixels take the permutation that shaded the frame; a row band has no output stage)
                return launch_pbr_hit_fetch(ctx->stream, ctx->ibl_apron, &f->gbuffer, *f->curr_camera, *f->pbr, f->ibl, f->background, rays, coords, &radiance, sh.shaded_rows.b, sh.shaded_rows.e, reversed);
            const LayeredHitFetch hit{rays, coords, sh.shaded_rows.b, sh.shaded_rows.e};
            return launch_pbr_shade_layers(ctx->stream, ctx->ibl_apron, &f->gbuffer, sh.layers(), *f->curr_camera, *f->pbr, f->ibl, f->background, &radiance, nullptr, 0, 0, reversed, sh.shadows(), &hit);
        };
        ssr_req.hit_local_rows = chain->shade.shaded_rows; // (R4 loads the colour of a hit in these rows itself; only the others go through the fetch)
        MIFX_CHECK(chain->ssr->run(&sr, ssr_req));
        if (req.wait_before_composite) MIFX_HIP_CHECK(hipStreamWaitEvent(ctx->stream, req.wait_before_composite, 0)); // (the end of SSAO on its lane)
        CompositeHandOver hand;
        MIFX_CHECK(mifx_ssao_get_output(chain->ssao, &ssao_out));
        MIFX_CHECK(chain_composite(chain, f, &radiance, &spec, &ssao_out, &comp, hand));
        ctx->need = r.taa;
        MIFX_CHECK(chain_taa(chain, f, &comp, hand));
        MIFX_CHECK(mifx_taa_get_output(chain->taa, 0, &taa_out));
        ctx->need = r.post; // (depth of field, on the rows Bloom reads of its output)
        MIFX_CHECK(chain_depth_of_field(chain, f, &taa_out));
        ctx->need = r.need;
        ba.color  = &taa_out;
        return chain->bloom->run(&ba, 1, nullptr, req.bloom);
    }
    mifx_autoexposure* ae = chain->auto_exposure;
    if (phase == 4)
    {
        if (!ae) return MIFX_OK;
        MIFX_HIP_CHECK(hipSetDevice(ctx->device));
        MIFX_CHECK(launch_autoexposure_reduce(ctx->stream, ae->low_res.view(), static_cast<float*>(ae->average.data), chain->ae_elapsed, chain->ae_adapt ? 1 : 0));
        MIFX_CHECK(mifx_bloom_get_output(chain->bloom, &bloom_out));
        ctx->need = r.band;
        return chain_copy_frame(chain, f, &bloom_out, out_ldr, nullptr);
    }
    MIFX_CHECK(mifx_taa_get_output(chain->taa, 0, &taa_out));
    if (chain->dof) MIFX_CHECK(mifx_dof_get_output(chain->dof, &taa_out)); // (computed in phase 2)
    ctx->need = r.need;
    ba.color  = &taa_out;
    const bool fuse_tone_map = chain->fuse_tone_map && ae == nullptr && !chain->has_grid;
    const mifx_bloom::FusedToneMap ftm{out_ldr, f->tone_mapping, f->ave_log_lum, f->tonemap_flags, chain->fuse_bloom_output};
    MIFX_CHECK(chain->bloom->run(&ba, 2, fuse_tone_map ? &ftm : nullptr, req.bloom));
    if (fuse_tone_map) return MIFX_OK;
    MIFX_CHECK(mifx_bloom_get_output(chain->bloom, &bloom_out));
    if (ae)
    {
        Img  color;
        bool packed = false;
        MIFX_CHECK(to_img_hdr(&bloom_out, "bloom output", color, packed));
        const Rows rows = mifx_autoexposure::sample_rows(r.band, int(f->frame.Height));
        return launch_autoexposure_rows(ctx->stream, color, ae->low_res.view(), rows.b, rows.e, packed);
    }
    return chain_copy_frame(chain, f, &bloom_out, out_ldr, nullptr); // (no auto exposure here: the grid or the plain tone map)
}
extern "C" mifx_status mifx_chain_execute_phase(mifx_chain* chain, const mifx_chain_frame* f, const mifx_image2d* out_ldr, int32_t phase)
{
    return mifx::chain_execute_phase(chain, f, out_ldr, phase, mifx::ChainPhaseRequest{});
}

// What the caller has to move between the phases: planes (valid after the phase that writes them) and row counts.
extern "C" mifx_status mifx_chain_get_shard_info(mifx_chain* chain, const mifx_chain_frame* f, mifx_shard_info* out)
{
    MIFX_REQUIRE(chain != nullptr && f != nullptr && out != nullptr && f->bloom && f->ssao && f->ssr, "mifx_chain_get_shard_info: null argument");
    MIFX_REQUIRE(!chain->band.empty() && chain->bloom->prepared, "mifx_chain_get_shard_info: set a row band and run phase 0 first");
    // (a chain whose frames run through mifx_chain_execute_sharded exchanges Bloom's level-0 halos and so needs shorter history halos: report what that frame uses)
    *out = mifx::chain_shard_info(chain, f, chain->band, chain->comm != nullptr && mifx::shard_bloom_halo_enabled());
    return MIFX_OK;
}

// Bloom's row plan of any band of the frame (mifx_chain_execute_sharded: which rows of level 0 a rank produces and which it reads, for the halo exchange of that level)
extern "C++" mifx_bloom::Plan mifx::chain_bloom_plan(const mifx_chain* chain, const mifx_chain_frame* f, Rows band, bool halo_level0)
{
    const ShardRows r = shard_rows(chain, f, band, halo_level0);
    return chain->bloom->make_plan(r.band, r.need, chain->bloom->mip_count(*f->bloom), halo_level0);
}

// the same for any band of the frame: the rows a rank owning `band` has to receive (mifx_chain_execute_sharded derives every rank's needs from
// the cuts, so that both sides of an exchange move the same rows without a round of communication)
extern "C++" mifx_shard_info mifx::chain_shard_info(const mifx_chain* chain, const mifx_chain_frame* f, Rows band, bool halo_level0)
{
    mifx_shard_info out{};
    const int H = int(f->frame.Height);
    const ShardRows r = shard_rows(chain, f, band, halo_level0);
    const mifx_bloom::Plan p = chain->bloom->make_plan(r.band, r.band, chain->bloom->mip_count(*f->bloom), halo_level0);
    const int m = chain->max_motion;
    auto ghost = [&](Rows w) { const int lo = r.band.b - w.b, hi = w.e - r.band.e; return lo > hi ? lo : hi; };
    // rows a pass reads of its history = its row window grown by the reprojection reach and the filter support
    const bool centredTaps = int(f->curr_camera->f4ViewportSize[0]) == int(f->frame.Width) && int(f->curr_camera->f4ViewportSize[1]) == H && f->frame.Width % 16u == 0u &&
                             f->frame.Height % 16u == 0u && !(chain->ssao_flags & MIFX_SSAO_FEATURE_FLAG_HALF_RESOLUTION); // as in mifx_ssao_execute
    const Rows ssao5 = mifx_ssao::accum_rows(*f->ssao, r.comp, H, centredTaps); // A5's rows for the composite rows: the effect's own window (w5 of mifx_ssao_execute)
    const Rows ssr6  = mifx_ssr::accum_rows(r.comp, H);                          // R6's rows for the composite rows: the effect's own window (w6 of mifx_ssr_execute)
    out.band_begin = r.band.b; out.band_end = r.band.e;
    out.halo_taa   = ghost(r.taa) + m + 3;   // Catmull-Rom history taps: +-2 texels around the reprojected position
    out.halo_ssr   = ghost(ssr6) + 2 * m + 2; // incident and hit-point reprojection, bilinear
    out.halo_ssao  = ghost(ssao5) + m + 2;
    out.gather_level = p.G;
    out.own_begin = p.own.b; out.own_end = p.own.e;
    const Rows ae = chain->auto_exposure ? mifx_autoexposure::sample_rows(r.band, H) : Rows{0, 0};
    out.ae_begin = ae.b; out.ae_end = ae.e;
    return out;
}

extern "C" mifx_status mifx_chain_get_shard_plane(mifx_chain* chain, const char* name, mifx_image2d* out)
{
    MIFX_REQUIRE(chain != nullptr && name != nullptr && out != nullptr, "mifx_chain_get_shard_plane: null argument");
    chain->join_halos(); // (what the caller queues on the context's stream next sees the planes with their halos received)
    const std::string n = name;
    const uint32_t ci = chain->ctx->frame.Index & 1u; // the planes the last executed frame wrote
    const Plane* p = nullptr;
    if (n == "radiance") p = &chain->radiance;
    else if (n == "bloom_gather") p = chain->bloom->prepared && int(chain->bloom->down.size()) > mifx_bloom::kGatherLevel ? chain->bloom->down[mifx_bloom::kGatherLevel] : nullptr;
    else if (n == "taa_history") p = &chain->taa->accum[ci];
    else if (n == "ssr_history_radiance") p = &chain->ssr->hist_radiance[ci];
    else if (n == "ssr_history_variance") p = &chain->ssr->hist_variance[ci];
    else if (n == "ssao_history_ao") p = &chain->ssao->history_ao[ci];
    else if (n == "ssao_history_len") p = &chain->ssao->history_len[ci];
    else if (n == "ae_low_res") p = chain->auto_exposure ? &chain->auto_exposure->low_res : nullptr;
    MIFX_REQUIRE(p != nullptr && p->data != nullptr, "mifx_chain_get_shard_plane: unknown or unallocated plane '%s'", name);
    *out = p->desc();
    return MIFX_OK;
}

mifx_status mifx_chain_set_auto_exposure(mifx_chain* chain, int32_t enable, float elapsed_time_s, int32_t light_adaptation)
{
    MIFX_REQUIRE(chain != nullptr && elapsed_time_s >= 0.0f, "mifx_chain_set_auto_exposure: bad argument");
    if (enable && !chain->auto_exposure) MIFX_CHECK(mifx_autoexposure_create(chain->ctx, &chain->auto_exposure));
    if (!enable && chain->auto_exposure)
    {
        mifx_autoexposure_destroy(chain->auto_exposure);
        chain->auto_exposure = nullptr;
    }
    chain->ae_elapsed = elapsed_time_s;
    chain->ae_adapt   = light_adaptation != 0;
    return MIFX_OK;
}

mifx_status mifx_chain_set_depth_of_field(mifx_chain* chain, const mifx_dof_attribs* attribs, uint32_t feature_flags)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_depth_of_field: null chain");
    if (chain->bloom) chain->bloom->output_deferred = false; // (a deferred Bloom output would read the depth-of-field output plane that is about to go / to change)
    if (attribs == nullptr)
    {
        mifx_dof_destroy(chain->dof);
        chain->dof = nullptr;
        return MIFX_OK;
    }
    MIFX_REQUIRE((feature_flags & ~3u) == 0, "mifx_chain_set_depth_of_field: unknown feature flags 0x%x", feature_flags);
    if (!chain->dof) MIFX_CHECK(mifx_dof_create(chain->ctx, &chain->dof));
    chain->dof_attribs = *attribs;
    chain->dof_flags   = feature_flags;
    return MIFX_OK;
}

mifx_status mifx_chain_set_selection(mifx_chain* chain, const mifx_selection_attribs* attribs, const mifx_image2d* selection_depth)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_selection: null chain");
    if (attribs == nullptr)
    {
        chain->has_selection     = false;
        chain->last_selection_id = 0; // (turning selection off forgets the selected prim)
        return MIFX_OK;
    }
    MIFX_REQUIRE(selection_depth != nullptr && selection_depth->data != nullptr, "mifx_chain_set_selection: the selection depth image is missing");
    MIFX_REQUIRE(attribs->outline_width > 0.0f, "mifx_chain_set_selection: outline_width %g must be positive", double(attribs->outline_width));
    if (chain->selection == nullptr) MIFX_CHECK(mifx_selection_create(chain->ctx, &chain->selection));
    chain->selection_attribs = *attribs;
    chain->selection_depth   = *selection_depth;
    chain->has_selection     = true;
    return MIFX_OK;
}

mifx_status mifx_chain_set_material_layers(mifx_chain* chain, const mifx_pbr_layers* layers, const mifx_pbr_shadows* shadows)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_material_layers: null chain");
    if (shadows != nullptr)
        MIFX_REQUIRE(shadows->shadow_map != nullptr && shadows->shadow_map_count <= MIFX_PBR_MAX_SHADOW_MAPS && (shadows->shadow_map_count == 0 || shadows->shadow_maps != nullptr),
                     "mifx_chain_set_material_layers: bad shadows block");
    chain->shade.kept_layers.keep(layers != nullptr && layers->flags != 0u ? layers : nullptr);
    chain->shade.kept_shadows.keep(shadows);
    return MIFX_OK;
}

mifx_status mifx_chain_set_shade_output(mifx_chain* chain, const mifx_pbr_shade_output_desc* output, int32_t write_targets)
{
    // (no device call: every refusal is an argument check)
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_shade_output: null chain");
    if (output != nullptr)
    {
        MIFX_CHECK(mifx::check_shade_output_desc("mifx_chain_set_shade_output", output));
        MIFX_REQUIRE(output->tone_mapping_mode == 0,
                     "mifx_chain_set_shade_output: tone_mapping_mode %d: the chain tone-maps at its own end (HnPostProcessTask runs the renderer without ENABLE_TONE_MAPPING)",
                     output->tone_mapping_mode);
        MIFX_REQUIRE((output->flags & MIFX_PBR_SHADE_OUTPUT_FLAG_CONVERT_OUTPUT_TO_SRGB) == 0u,
                     "mifx_chain_set_shade_output: CONVERT_OUTPUT_TO_SRGB: the chain converts at its own end (the copy-frame pass)");
    }
    const bool on = output != nullptr || write_targets != 0;
    MIFX_REQUIRE(!on || chain->band.empty(),
                 "mifx_chain_set_shade_output: not combined with a row band or sharding (mifx_chain_set_row_band / _set_sharding): the sharded hit fetch has no output stage or footer");
    MIFX_REQUIRE(write_targets != 0 || chain->shade.transparent.empty(),
                 "mifx_chain_set_shade_output: write_targets goes off while mifx_chain_set_transparency is on: the transparent draws blend into the chain's own target planes "
                 "(turn transparency off first)");
#ifdef MIFX_STORAGE_H4
    if (on)
    {
        ::mifx::set_error("mifx_chain_set_shade_output: the shade's output stage and its footer are not part of the native-storage build yet");
        return MIFX_ERR_NOT_IMPLEMENTED;
    }
#endif
    chain->shade.kept_output.keep(output);
    chain->shade.targets_on = write_targets != 0;
    chain->prep_consumed = false; // (which planes the lanes trade and read changes: the next frame forks from the context stream once)
    return MIFX_OK;
}

mifx_status mifx_chain_set_transparency(mifx_chain* chain, uint32_t layer_count, const mifx_transparent_slice* slices, uint32_t count)
{
    // (no device call: every refusal is an argument check)
    const char* who = "mifx_chain_set_transparency";
    MIFX_REQUIRE(chain != nullptr, "%s: null chain", who);
    if (slices == nullptr || count == 0u) // off: the chain launches what it launched before
    {
        chain->shade.transparent.clear();
        return MIFX_OK;
    }
#ifdef MIFX_STORAGE_H4
    (void)layer_count;
    ::mifx::set_error("%s: the fused shade-and-blend is not part of the native-storage build yet", who);
    return MIFX_ERR_NOT_IMPLEMENTED;
#else
    MIFX_REQUIRE(count <= uint32_t(MIFX_OIT_MAX_SLICES), "%s: %u slices are more than MIFX_OIT_MAX_SLICES (%d)", who, count, MIFX_OIT_MAX_SLICES);
    MIFX_CHECK(mifx_oit_create_check(1u, 1u, layer_count));
    MIFX_REQUIRE(chain->shade.targets_on,
                 "%s: needs mifx_chain_set_shade_output with write_targets: the transparent draws blend into the chain's own BaseColor / Material / IBL planes (without "
                 "them base colour and material are the caller's const planes)", who);
    // (a row band needs no check of its own: mifx_chain_set_shade_output and mifx_chain_set_row_band refuse each other, in either order)
    for (uint32_t i = 0; i < count; ++i)
    {
        const mifx_gbuffer& g = slices[i].gbuffer;
        MIFX_REQUIRE(g.base_color != nullptr && g.normal != nullptr && g.material != nullptr && g.depth != nullptr, "%s: slice %u: base_color, normal, material and depth must not be null",
                     who, i);
    }
    std::vector<mifx::KeptTransparentSlice> copy(count);
    for (uint32_t i = 0; i < count; ++i) copy[i].keep(slices[i]);
    chain->shade.transparent.swap(copy);
    chain->shade.oit_layer_count = layer_count;
    return MIFX_OK;
#endif
}

int32_t mifx_chain_set_transparency_fusion(int32_t enable)
{
    const int32_t prev    = g_transparency_fusion ? 1 : 0;
    g_transparency_fusion = enable != 0;
    return prev;
}

mifx_status mifx_chain_get_shade_target(mifx_chain* chain, const char* name, mifx_image2d* out)
{
    MIFX_REQUIRE(chain != nullptr && name != nullptr && out != nullptr, "mifx_chain_get_shade_target: null argument");
    static const char* const names[4] = {"normal", "base_color", "material", "ibl"};
    for (int i = 0; i < 4; ++i)
        if (std::string(name) == names[i])
        {
            MIFX_REQUIRE(chain->shade.targets_on && chain->shade.targets[i].data != nullptr,
                         "mifx_chain_get_shade_target: no '%s' target (mifx_chain_set_shade_output with write_targets, and a frame executed)", name);
            *out = chain->shade.targets[i].desc();
            return MIFX_OK;
        }
    set_error("mifx_chain_get_shade_target: unknown target '%s' (normal, base_color, material, ibl)", name);
    return MIFX_ERR_INVALID_ARG;
}

mifx_status mifx_chain_set_effect_feature_flags(mifx_chain* chain, uint32_t ssao_feature_flags, uint32_t ssr_feature_flags)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_effect_feature_flags: null chain");
    MIFX_REQUIRE((ssao_feature_flags & ~3u) == 0 &&
                     (ssr_feature_flags & ~(uint32_t(MIFX_SSR_FEATURE_FLAG_PREVIOUS_FRAME) | uint32_t(MIFX_SSR_FEATURE_FLAG_HALF_RESOLUTION))) == 0,
                 "mifx_chain_set_effect_feature_flags: SSAO 0x%x / SSR 0x%x: unknown flag", ssao_feature_flags, ssr_feature_flags);
    chain->ssao_flags = ssao_feature_flags;
    chain->ssr_flags  = ssr_feature_flags;
    return MIFX_OK;
}

mifx_status mifx_chain_set_postfx_feature_flags(mifx_chain* chain, uint32_t feature_flags)
{
    MIFX_REQUIRE(chain != nullptr && (feature_flags & ~7u) == 0, "mifx_chain_set_postfx_feature_flags: unknown flag 0x%x", feature_flags);
    // (FEATURE_FLAG_TEMPORAL_UPSCALING: the chain has no up-scaler between TAA and Bloom -- neither has HnPostProcessTask -- so Bloom accepts the TAA output only
    //  when FrameDesc.OutputWidth x OutputHeight equals Width x Height; a different output size is refused by mifx_bloom_execute with the sizes in the message)
    chain->postfx_flags = feature_flags;
    return MIFX_OK;
}

mifx_status mifx_chain_get_auto_exposure(mifx_chain* chain, mifx_autoexposure** out)
{
    MIFX_REQUIRE(chain != nullptr && out != nullptr, "mifx_chain_get_auto_exposure: null argument");
    *out = chain->auto_exposure;
    return MIFX_OK;
}

mifx_status mifx_chain_set_fusion(mifx_chain* chain, int32_t tone_map_into_bloom, int32_t ssr_mask_into_shade)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_fusion: null chain");
    chain->fuse_tone_map = tone_map_into_bloom != 0;
    chain->fuse_ssr_mask = ssr_mask_into_shade != 0;
    return MIFX_OK;
}

mifx_status mifx_chain_set_fusion_mask(mifx_chain* chain, uint32_t mask)
{
    MIFX_REQUIRE(chain != nullptr && (mask & ~uint32_t(MIFX_CHAIN_FUSE_EVERY_SWITCH)) == 0, "mifx_chain_set_fusion_mask: bad argument (mask 0x%x)", mask);
    chain->fuse_tone_map    = (mask & MIFX_CHAIN_FUSE_TONE_MAP_INTO_BLOOM) != 0;
    chain->fuse_ssr_mask    = (mask & MIFX_CHAIN_FUSE_SSR_MASK_INTO_SHADE) != 0;
    chain->fuse_ssr_cleanup = (mask & MIFX_CHAIN_FUSE_SSR_CLEANUP_INTO_COMPOSITE) != 0;
    chain->ssao->fused_resolve = (mask & MIFX_CHAIN_FUSE_SSAO_RESOLVE) != 0;
    chain->fuse_bloom_output   = (mask & MIFX_CHAIN_FUSE_BLOOM_OUTPUT_ON_DEMAND) != 0;
    chain->fuse_composite_taa  = (mask & MIFX_CHAIN_FUSE_COMPOSITE_INTO_TAA) != 0;
    return MIFX_OK;
}

mifx_status mifx_chain_set_overlap(mifx_chain* chain, int32_t enable)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_overlap: null chain");
    MIFX_REQUIRE(enable >= 0 && enable <= 5, "mifx_chain_set_overlap: %d (0 off, 1 inside a frame, 2 across frames, 3 three lanes across frames, 4 three lanes with two frames in flight, 5 = 4 with the composite and TAA on the Bloom lane)", enable);
    if (chain->overlap != enable) chain->prep_consumed = false; // (a change of the mode: the next frame forks from the context stream once)
    chain->overlap = enable;
    return MIFX_OK;
}

// "waiter<signal@delta,...": see mifx.h.  An empty or NULL list removes every edge.
mifx_status mifx_chain_set_lane_edges(mifx_chain* chain, const char* edges)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_lane_edges: null chain");
    std::vector<mifx_chain::Edge> parsed;
    const std::string list = edges ? edges : "";
    size_t pos = 0;
    while (pos < list.size())
    {
        size_t stop = list.find(',', pos);
        if (stop == std::string::npos) stop = list.size();
        const std::string item = list.substr(pos, stop - pos);
        pos = stop + 1;
        if (item.empty()) continue;
        const size_t lt = item.find('<'), at = item.find('@');
        MIFX_REQUIRE(lt != std::string::npos && lt > 0 && at != std::string::npos && at > lt + 1 && at + 1 < item.size(),
                     "mifx_chain_set_lane_edges: '%s' is not of the form waiter<signal@frames", item.c_str());
        const int d = std::atoi(item.c_str() + at + 1);
        MIFX_REQUIRE(d >= 0 && d <= 3, "mifx_chain_set_lane_edges: '%s': 0 .. 3 frames back", item.c_str());
        parsed.push_back(mifx_chain::Edge{item.substr(0, lt), item.substr(lt + 1, at - lt - 1), d});
    }
    chain->edges.swap(parsed);
    chain->prep_consumed = false; // (the next frame forks from the context stream once)
    return MIFX_OK;
}

mifx_status mifx_chain_set_profiling(mifx_chain* chain, int32_t enable)
{
    MIFX_REQUIRE(chain != nullptr, "mifx_chain_set_profiling: null argument");
    MIFX_HIP_CHECK(hipSetDevice(chain->ctx->device));
    if (enable)
        for (auto& e : chain->ev)
            if (!e) MIFX_HIP_CHECK(hipEventCreate(&e));
    chain->profiling = enable != 0;
    chain->timed     = false;
    return MIFX_OK;
}

mifx_status mifx_chain_get_stage_times(mifx_chain* chain, float out_ms[MIFX_CHAIN_STAGE_COUNT])
{
    MIFX_REQUIRE(chain != nullptr && out_ms != nullptr, "mifx_chain_get_stage_times: null argument");
    if (!chain->timed)
    {
        set_error("mifx_chain_get_stage_times: enable profiling and execute a frame first");
        return MIFX_ERR_INVALID_OP;
    }
    MIFX_HIP_CHECK(hipEventSynchronize(chain->ev[MIFX_CHAIN_STAGE_COUNT]));
    for (int i = 0; i < MIFX_CHAIN_STAGE_COUNT; ++i) MIFX_HIP_CHECK(hipEventElapsedTime(&out_ms[i], chain->ev[i], chain->ev[i + 1]));
    return MIFX_OK;
}

} // extern "C"
