// mifx_material_host.h -- the launcher of the material fetch (material.hip), called by api_material.cpp.  The fp32 build alone has the kernel: the native-storage build
// answers MIFX_ERR_NOT_IMPLEMENTED behind its argument checks.
#pragma once
#include "mifx_host.h"
#include "mifx_material.h"

namespace mifx
{
// material_fetch_kernel<atlas> over k.depth.w x k.depth.h; the atlas permutation is MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS of k.flags
mifx_status launch_material_fetch(hipStream_t s, const MaterialFetchK& k, const CamK& cam);
} // namespace mifx
