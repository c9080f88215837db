// mifx_oit_host.h -- the launchers of the layered order-independent transparency (oit.hip), one per kernel (oit.hip; launch_oit_shade_blend: pbr.hip), called by api_oit.cpp.  Both builds compile the same kernels.
#pragma once
#include "mifx_host.h"
#include "mifx_oit.h"

namespace mifx
{
// the layer counts the fused pair (launch_oit_build: clear + every update; launch_oit_resolve: attenuation + every blend) is instantiated for; any other takes the sequence
constexpr bool oit_has_fused_kernel(uint32_t K) { return K == 1 || K == 2 || K == 3 || K == 4 || K == 8; }
mifx_status launch_oit_clear(hipStream_t s, const OitK& k);
mifx_status launch_oit_update(hipStream_t s, const OitK& k, const OitSliceK& slice);
mifx_status launch_oit_attenuate(hipStream_t s, const OitK& k, const OitTargetsK& targets);
mifx_status launch_oit_blend(hipStream_t s, const OitK& k, const OitSliceK& slice, const OitTargetsK& targets);
mifx_status launch_oit_build(hipStream_t s, const OitK& k, const OitSlicesK& tab);
mifx_status launch_oit_resolve(hipStream_t s, const OitK& k, const OitSlicesK& tab, const OitTargetsK& targets);
// One transparent draw shaded and blended by one kernel (pbr.hip: the kernel is the layered shade's body with the OIT colour pass behind it, so it lives beside the shade's
// kernels and shares their argument checks and IBL copies).  `g`: the draw's G-buffer, of the frame size of `k`; layers == nullptr: the empty set.
// check_only: the argument checks alone -- nothing is launched, no device call is made (`s`, `iblApron` and the buffers of `k` are not touched).
mifx_status launch_oit_shade_blend(hipStream_t s, IblApronCache& iblApron, const OitK& k, const OitTargetsK& targets, const mifx_gbuffer* g, const mifx_pbr_layers* layers,
                                   const mifx_image2d* color_alpha, const mifx_camera_attribs& camera, const mifx_pbr_shade_attribs& a, const mifx_ibl* ibl, bool reversedDepth,
                                   const mifx_pbr_shadows* shadows, bool check_only);
} // namespace mifx
