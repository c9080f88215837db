// mifx_oit_host.h -- the launchers of the layered order-independent transparency (oit.hip), one per kernel, called by api_oit.cpp.  Both builds compile the same kernels.
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
} // namespace mifx
