// api_selection.cpp -- C ABI of the selection outline (include/mifx.h: mifx_selection_*, mifx_composite_execute_selection) and the chain's composite with selection on:
// HnProcessSelectionTask::Execute (Hydrogent/src/Tasks/HnProcessSelectionTask.cpp:302-369), then the selection tail of HnPostProcess.psh:211-241.  The kernels and their
// launchers are in selection.hip and composite.hip (mifx_selection_host.h).
#include "mifx_objects.h"
#include "mifx_selection_host.h"

using namespace mifx;

// the SelectionK of a composite: planes checked against the W x H target, colours as given
static mifx_status make_selectionk(const mifx_selection_composite_inputs& in, uint32_t W, uint32_t H, SelectionK& k)
{
    MIFX_REQUIRE(in.attribs != nullptr, "selection composite: attribs must not be null");
    MIFX_CHECK(to_img_wh(in.depth, MIFX_FORMAT_F32, W, H, "depth", k.depth));
    MIFX_CHECK(to_img_wh(in.selection_depth, MIFX_FORMAT_F32, W, H, "selection_depth", k.selectionDepth));
    MIFX_CHECK(to_img_wh(in.closest_location, MIFX_FORMAT_F32X2, W, H, "closest_location", k.closest));
    const mifx_selection_attribs& a = *in.attribs;
    MIFX_REQUIRE(a.outline_width > 0.0f, "selection composite: outline_width %g must be positive", double(a.outline_width));
    for (int i = 0; i < 3; ++i)
    {
        k.outline[i]  = a.outline_color[i];
        k.occluded[i] = a.occluded_outline_color[i];
    }
    k.desaturation = a.nonselection_desaturation;
    k.clearDepth   = a.clear_depth;
    k.outlineWidth = a.outline_width;
    return MIFX_OK;
}

// HnProcessSelectionTask::Execute for `sel`'s context on the rows that context needs
static mifx_status selection_run(mifx_selection* sel, const mifx_image2d* selectionDepth, const mifx_selection_attribs& a)
{
    mifx_postfx* ctx = sel->ctx;
    Img depth;
    MIFX_CHECK(to_img(selectionDepth, MIFX_FORMAT_F32, "selection_depth", depth));
    MIFX_REQUIRE(a.max_distance == a.max_distance, "mifx_selection_execute: max_distance is NaN");
    const uint32_t W = selectionDepth->width, H = selectionDepth->height;
    const int      n = jf_iterations(a.max_distance);
    MIFX_REQUIRE(n <= 24, "mifx_selection_execute: max_distance %g is beyond the frame sizes this library supports", double(a.max_distance));
    MIFX_CHECK(sel->out.alloc(W, H, MIFX_FORMAT_F32X2));
    if (n > kJfFused) MIFX_CHECK(sel->tmp[0].alloc(W, H, MIFX_FORMAT_F32X2));
    if (n > kJfFused + 1) MIFX_CHECK(sel->tmp[1].alloc(W, H, MIFX_FORMAT_F32X2));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    if (a.selection_id == 0) return sel->out.fill(ctx->stream, 0.0f); // nothing selected: the final target cleared to 0 (HnProcessSelectionTask.cpp:329-335)
    MifxKernelTimer timer(ctx, "jump_flood_kernel");
    const Rows rows = ctx->needed_rows(int(H));
    return launch_jump_flood(ctx->stream, depth, a.clear_depth, n, sel->tmp[0].view(), sel->tmp[1].view(), sel->out.view(), rows.b, rows.e);
}

mifx_status mifx::selection_chain_composite(mifx_selection* sel, const mifx_selection_attribs& a, const mifx_image2d* selectionDepth, const mifx_composite_attribs& ca,
                                            const mifx_image2d* depth, const mifx_image2d* out, const SsrCleanupIn* r7)
{
    MIFX_CHECK(selection_run(sel, selectionDepth, a));
    const mifx_image2d closest = sel->out.desc();
    const mifx_selection_composite_inputs in{depth, selectionDepth, &closest, &a};
    SelectionK k;
    MIFX_CHECK(make_selectionk(in, out->width, out->height, k));
    mifx_postfx* ctx = sel->ctx;
    MifxKernelTimer timer(ctx, r7 ? "composite_ssr_cleanup_kernel" : "composite_kernel");
    const Rows rows = ctx->needed_rows(int(out->height));
    return launch_composite_selection(ctx->stream, ca, k, out, rows.b, rows.e, r7);
}

extern "C" {

mifx_status mifx_selection_create(mifx_postfx* ctx, mifx_selection** out)
{
    MIFX_REQUIRE(ctx != nullptr && out != nullptr, "mifx_selection_create: null argument");
    mifx_selection* sel = new mifx_selection();
    sel->ctx = ctx;
    *out = sel;
    return MIFX_OK;
}

void mifx_selection_destroy(mifx_selection* sel) { delete sel; }

mifx_status mifx_selection_execute(mifx_selection* sel, const mifx_image2d* selection_depth, const mifx_selection_attribs* attribs)
{
    MIFX_REQUIRE(sel != nullptr && selection_depth != nullptr && attribs != nullptr, "mifx_selection_execute: null argument");
    return selection_run(sel, selection_depth, *attribs);
}

mifx_status mifx_selection_get_output(mifx_selection* sel, mifx_image2d* out)
{
    MIFX_REQUIRE(sel != nullptr && out != nullptr, "mifx_selection_get_output: null argument");
    MIFX_REQUIRE(sel->out.data != nullptr, "mifx_selection_get_output: not executed yet");
    *out = sel->out.desc();
    return MIFX_OK;
}

mifx_status mifx_composite_execute_selection(mifx_postfx* ctx, const mifx_composite_attribs* attribs, const mifx_selection_composite_inputs* selection, const mifx_image2d* out)
{
    MIFX_REQUIRE(ctx != nullptr && attribs != nullptr && selection != nullptr && out != nullptr, "mifx_composite_execute_selection: null argument");
    SelectionK k;
    MIFX_CHECK(make_selectionk(*selection, out->width, out->height, k));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    MifxKernelTimer timer(ctx, "composite_kernel");
    const Rows rows = ctx->needed_rows(int(out->height));
    return launch_composite_selection(ctx->stream, *attribs, k, out, rows.b, rows.e);
}

} // extern "C"
