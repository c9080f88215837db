// mifx_oit_shade_launch.h -- the launcher of oit_shade_blend_kernel (pbr.hip: the kernel is the layered shade's body with the OIT colour pass behind it, so it lives beside
// the shade's kernels and shares their argument checks and IBL copies), called by api_oit.cpp.
//
// How the host code reaches it -- a debt, not a design (DESIGN.md section 4 "Transparency in the chain", section 7 item 3).  The launcher belongs in mifx_oit_host.h,
// called directly.  The host sources (csrc/*.cpp) are also linked WITHOUT the device objects by the host-only build of the test suite, against generated stand-ins for
// exactly the launchers of mifx_host.h / mifx_*_host.h; the change that added this launcher left that file as it was, so api_oit.cpp cannot name the launcher: pbr.hip
// puts its address into g_launch_oit_shade_blend when the library is loaded, and a build without pbr.hip leaves the pointer null -- mifx_oit_shade_blend then returns
// MIFX_ERR_NOT_IMPLEMENTED and names the launcher.  There is no other path to the kernel and no fall-back: a library without it refuses the call.
#pragma once
#include "mifx_host.h"
#include "mifx_oit.h"

namespace mifx
{
// `g`: the draw's G-buffer, of the frame size of `k`; layers == nullptr: the empty set.
// check_only: the argument checks alone -- nothing is launched, no device call is made (`s`, `iblApron` and the buffers of `k` are not touched).
mifx_status launch_oit_shade_blend(hipStream_t s, IblApronCache& iblApron, const OitK& k, const OitTargetsK& targets, const mifx_gbuffer* g, const mifx_pbr_layers* layers,
                                   const mifx_image2d* color_alpha, const mifx_camera_attribs& camera, const mifx_pbr_shade_attribs& a, const mifx_ibl* ibl, bool reversedDepth,
                                   const mifx_pbr_shadows* shadows, bool check_only);
extern decltype(&launch_oit_shade_blend) g_launch_oit_shade_blend; // api_oit.cpp; null until pbr.hip's initialiser has run
} // namespace mifx
