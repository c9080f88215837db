// oit.hip -- layered order-independent transparency over G-buffer slices (include/mifx.h "layered order-independent transparency"): the six kernels and their
// launchers (mifx_oit_host.h; launch_oit_shade_blend, the seventh, is in pbr.hip beside the shade it contains).  The per-pixel bodies are mifx_oit.h; the effect object, the argument checks, the sequencing and the C entries are api_oit.cpp.
//
// Two shapes built from the same bodies:
//   the reference's sequence, one launch each: oit_clear_kernel (ClearOITLayers.csh), oit_update_kernel (one draw of UpdateOITLayers.psh: reads and writes the pixel's K
//   words and the tail), oit_attenuate_kernel (ApplyOITAttenuation.psh), oit_blend_kernel (one transparent draw of the colour pass: reads the K words and the tail, reads
//   and writes the four 16-byte targets) -- 1 + L + 1 + L launches for L draws, L * (2 * 4 K + 16 + 20) bytes a pixel to build and 128 + L * (128 + 68 + 4 K + 8) to resolve;
//   fused: oit_build_kernel<K> keeps the K words and the tail in registers over all L slices and stores them once (L * 20 + 4 K + 8 bytes a pixel),
//   oit_resolve_kernel<K> loads the words, the tail and each target once, attenuates, blends the L slices in order and stores each target once (128 + L * 68 + 4 K + 8).
// One thread per pixel, 64 consecutive pixels of a row per wave: a wave's access to a 16-byte target is 1 KB contiguous, to the K words 256 K bytes contiguous.  The
// slice table of the fused kernels is a kernel argument indexed by the (wave-uniform) loop counter: scalar loads.  Measured (profiles/oit_bench.json): every kernel runs
// at the device's copy rate for the bytes its shape moves (5.3 - 5.8 TB/s beside a copy at 5.3), so the fused pair's gain is the bytes it does not move.  Streaming
// passes, but no non-temporal hints and no row walk: no A/B of either has been measured here.
//
// Native-storage build (-DMIFX_STORAGE_H4).  The same kernels: the slice planes and the four targets are the build's 4-channel texel, RGBA16_FLOAT (8 bytes: the
// 16 / 128 above become 8 / 64; a slice's opacity is the half at +6), as the reference's targets are; depth, colour alpha and the opaque depth stay F32, the tail
// F32X2, the layers uint32.  A blend is evaluated in fp32 and its store rounds to binary16, once per draw in the sequence; oit_resolve_kernel rounds the four texels
// in registers at the same points (quantize_v4, the identity in the fp32 build), so it still equals the sequence bit for bit while it loads and stores each target
// once (tests/h4_checks_shadows_oit.py).
#include "mifx_oit_host.h"

namespace mifx
{
__global__ __launch_bounds__(256) void oit_clear_kernel(OitK k)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_clear(k, x, y);
}
__global__ __launch_bounds__(256) void oit_update_kernel(OitK k, OitSliceK s)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_update(k, s, x, y);
}
__global__ __launch_bounds__(256) void oit_attenuate_kernel(OitK k, OitTargetsK t)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_attenuate(k, t, x, y);
}
__global__ __launch_bounds__(256) void oit_blend_kernel(OitK k, OitSliceK s, OitTargetsK t)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_blend(k, s, t, x, y);
}
template <int K> __global__ __launch_bounds__(256) void oit_build_kernel(OitK k, OitSlicesK tab)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_build<K>(k, tab, x, y);
}
template <int K> __global__ __launch_bounds__(256) void oit_resolve_kernel(OitK k, OitSlicesK tab, OitTargetsK t)
{
    const int x = int(blockIdx.x * blockDim.x + threadIdx.x), y = int(blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= k.w || y >= k.h) return;
    oit_px_resolve<K>(k, tab, t, x, y);
}

static dim3 oit_block() { return dim3(64, 4, 1); }
static dim3 oit_grid(const OitK& k) { return dim3((uint32_t(k.w) + 63u) / 64u, (uint32_t(k.h) + 3u) / 4u, 1); }
#define MIFX_LAUNCH_END()              \
    MIFX_HIP_CHECK(hipGetLastError()); \
    return MIFX_OK

mifx_status launch_oit_clear(hipStream_t s, const OitK& k)
{
    hipLaunchKernelGGL(oit_clear_kernel, oit_grid(k), oit_block(), 0, s, k);
    MIFX_LAUNCH_END();
}
mifx_status launch_oit_update(hipStream_t s, const OitK& k, const OitSliceK& slice)
{
    hipLaunchKernelGGL(oit_update_kernel, oit_grid(k), oit_block(), 0, s, k, slice);
    MIFX_LAUNCH_END();
}
mifx_status launch_oit_attenuate(hipStream_t s, const OitK& k, const OitTargetsK& targets)
{
    hipLaunchKernelGGL(oit_attenuate_kernel, oit_grid(k), oit_block(), 0, s, k, targets);
    MIFX_LAUNCH_END();
}
mifx_status launch_oit_blend(hipStream_t s, const OitK& k, const OitSliceK& slice, const OitTargetsK& targets)
{
    hipLaunchKernelGGL(oit_blend_kernel, oit_grid(k), oit_block(), 0, s, k, slice, targets);
    MIFX_LAUNCH_END();
}
// the fused pair: the instance for the layer count (oit_has_fused_kernel: the caller has asked it)
#define MIFX_OIT_BY_K(KERNEL) (k.K == 1 ? KERNEL<1> : k.K == 2 ? KERNEL<2> : k.K == 3 ? KERNEL<3> : k.K == 4 ? KERNEL<4> : KERNEL<8>)
mifx_status launch_oit_build(hipStream_t s, const OitK& k, const OitSlicesK& tab)
{
    hipLaunchKernelGGL(MIFX_OIT_BY_K(oit_build_kernel), oit_grid(k), oit_block(), 0, s, k, tab);
    MIFX_LAUNCH_END();
}
mifx_status launch_oit_resolve(hipStream_t s, const OitK& k, const OitSlicesK& tab, const OitTargetsK& targets)
{
    hipLaunchKernelGGL(MIFX_OIT_BY_K(oit_resolve_kernel), oit_grid(k), oit_block(), 0, s, k, tab, targets);
    MIFX_LAUNCH_END();
}
} // namespace mifx
