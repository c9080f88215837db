// mifx_selection_host.h -- host side of the selection outline (selection.hip, composite.hip, api_selection.cpp).
// The two launchers are defined beside their kernels; the effect object's sequencing and the C entry points are in api_selection.cpp, which the chain
// (api_chain.cpp) calls directly.
#pragma once
#include "mifx_host.h"
#include "mifx_selection.h"

namespace mifx
{
constexpr int kJfFused = 3; // jump-flood steps of the one tiled launch: the reach 4 + 2 + 1 = 7 of its halo; the steps before it need the `tmp` planes

// the jump flood (selection.hip): from the selection depth to `out` (F32X2), steps of the ranges 1 << (n - 1 - i); `tmp` holds the planes of the leading steps that do
// not fit the fused launch's halo.  rows [rowBegin, rowEnd) of `out` are written (the leading steps always cover the whole frame).
mifx_status launch_jump_flood(hipStream_t s, Img selectionDepth, float clearDepth, int iterations, Img tmp0, Img tmp1, Img out, int rowBegin, int rowEnd);
// the composite with the selection tail (composite.hip); r7 as for launch_composite
mifx_status launch_composite_selection(hipStream_t s, const mifx_composite_attribs& a, const SelectionK& sel, const mifx_image2d* out, int row_begin, int row_end,
                                       const SsrCleanupIn* r7 = nullptr);
// the chain's composite of one frame with selection on: the jump flood, then the selection composite on the rows the context needs (r7: SSR's cleanup in place)
mifx_status selection_chain_composite(mifx_selection* sel, const mifx_selection_attribs& attribs, const mifx_image2d* selectionDepth, const mifx_composite_attribs& ca,
                                      const mifx_image2d* depth, const mifx_image2d* out, const SsrCleanupIn* r7);
} // namespace mifx
