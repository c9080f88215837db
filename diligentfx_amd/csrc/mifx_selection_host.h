// mifx_selection_host.h -- host side of the selection outline (selection.hip, composite.hip).
// The launchers and the C entry points live beside the kernels, in the .hip translation units; the chain (api_chain.cpp) reaches what it needs through
// `selection_hooks`, which selection.hip fills in at load time.  A build of the host objects without the kernels leaves it null, and the chain then refuses
// selection with MIFX_ERR_NOT_IMPLEMENTED (nothing else changes).
#pragma once
#include "mifx_host.h"
#include "mifx_selection.h"

namespace mifx
{
// the jump flood (selection.hip): from the selection depth to `out` (F32X2), steps of the ranges 1 << (n - 1 - i); `tmp` holds the planes of the leading steps that do
// not fit the fused launch's halo.  rows [rowBegin, rowEnd) of `out` are written (the leading steps always cover the whole frame).
mifx_status launch_jump_flood(hipStream_t s, Img selectionDepth, float clearDepth, int iterations, Img tmp0, Img tmp1, Img out, int rowBegin, int rowEnd);
// the composite with the selection tail (composite.hip); r7 as for launch_composite
mifx_status launch_composite_selection(hipStream_t s, const mifx_composite_attribs& a, const SelectionK& sel, const mifx_image2d* out, int row_begin, int row_end,
                                       const SsrCleanupIn* r7 = nullptr);
// the SelectionK of a composite: planes checked against the W x H target, colours as given
mifx_status make_selectionk(const mifx_selection_composite_inputs& in, uint32_t W, uint32_t H, SelectionK& k);

struct SelectionHooks
{
    mifx_status (*create)(mifx_postfx* ctx, mifx_selection** out);
    void (*destroy)(mifx_selection* sel);
    // the chain's composite of one frame with selection on: the jump flood, then the selection composite on the rows the context needs (r7: SSR's cleanup in place)
    mifx_status (*chain_composite)(mifx_selection* sel, const mifx_selection_attribs& attribs, const mifx_image2d* selectionDepth, const mifx_composite_attribs& ca,
                                   const mifx_image2d* depth, const mifx_image2d* out, const SsrCleanupIn* r7);
};
extern const SelectionHooks* selection_hooks; // (api_chain.cpp; null without selection.hip)
} // namespace mifx
