// mifx_shadows_host.h -- the launchers of the cascaded shadow maps (shadows.hip), called by api_shadows.cpp.
// Both builds of the library compile the same kernels: the filterable array names its own format (FilterableArrK::fmt), every other plane is F32 / F32X2.
#pragma once
#include "mifx_host.h"
#include "mifx_shadows.h"

namespace mifx
{
// ConvertToFilterable for all cascades.  mode: MIFX_SHADOW_MODE_VSM / EVSM2 / EVSM4; skipBlur: iFixedFilterSize == 2 (the horizontal kernel alone); fused: the LDS-tile
// kernel (the caller has checked that every range fits); otherwise two launches through `scratch`, the calling context's own block on its own device
mifx_status launch_shadow_convert(hipStream_t s, DeviceScratch& scratch, const ShadowArrK& src, const FilterableArrK& dst, const ShadowConvK& k, uint32_t mode, bool skipBlur, bool fused);
// shadow_filter_kernel<mode, best, across>; cascade.p may be null
mifx_status launch_shadow_filter(hipStream_t s, Img depth, Img light, Img cascade, const ShadowLookupK& k, const ShadowArrK& map, const FilterableArrK& filterable, uint32_t mode, bool best,
                                 bool across);
} // namespace mifx
