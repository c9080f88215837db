// TEST INFRASTRUCTURE ONLY.  The order-independent-transparency bodies (diligentfx_amd/csrc/mifx_oit.h) compiled for the HOST in fp32, as oit_host.cpp compiles them,
// with the reference's sequence cut into its draws: the layers (the clear and every update), the attenuation, ONE colour draw.  The caller rounds the four targets
// to binary16 between the calls, which is what the RGBA16_FLOAT targets of the native-storage build do at every store (tests/oit16_util.py emulate()).
// Nothing in diligentfx_amd/ builds, loads or calls this.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "mifx.h"
#include "mifx_oit.h"

using namespace mifx;

namespace
{
unsigned char* bytes(const void* p) { return reinterpret_cast<unsigned char*>(const_cast<void*>(p)); }
OitK make_k(int K, int W, int H, const float* opaque, const mifx_camera_attribs* camera, const uint32_t* layers, const float* tail)
{
    return OitK{bytes(layers), bytes(tail), opaque ? bytes(opaque) : nullptr, W, H, K, W * 8, W * 4, make_oitcamk(*camera)};
}
OitSliceK make_slice(int W, const float* depth, const float* base, const float* material, const float* radiance, const float* ibl, const float* alpha)
{
    return OitSliceK{bytes(depth), bytes(base), bytes(material), bytes(radiance), bytes(ibl), alpha ? bytes(alpha) : nullptr, W * 4, W * 16, W * 16, W * 16, W * 16, W * 4};
}
OitTargetsK make_targets(int W, int H, float* targets)
{
    OitTargetsK t{};
    Img*        im[4] = {&t.color, &t.base, &t.material, &t.ibl};
    for (int j = 0; j < 4; ++j) *im[j] = Img{bytes(targets + size_t(4) * j * W * H), W, H, W * 16, 0, 0};
    return t;
}
bool bad(int K, int L) { return K < 1 || K > MIFX_OIT_MAX_LAYERS || L < 0 || L > MIFX_OIT_MAX_SLICES; }
} // namespace

extern "C" {
// planes tightly packed, slice l of depth / base follows slice l - 1; layers: H x W x K words, tail: H x W x 2
int mifx_host_oit16_layers(int K, int W, int H, int L, const float* depth, const float* base, const float* opaque, const mifx_camera_attribs* camera, uint32_t* layers, float* tail)
{
    if (bad(K, L)) return -1;
    const OitK   k = make_k(K, W, H, opaque, camera, layers, tail);
    const size_t n = size_t(W) * H;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) oit_px_clear(k, x, y);
    for (int l = 0; l < L; ++l)
    {
        const OitSliceK s = make_slice(W, depth + l * n, base + 4 * l * n, nullptr, nullptr, nullptr, nullptr);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) oit_px_update(k, s, x, y);
    }
    return 0;
}
// targets: 4 x H x W x 4 (colour, base colour, material, IBL), attenuated in place
int mifx_host_oit16_attenuate(int K, int W, int H, const mifx_camera_attribs* camera, const uint32_t* layers, const float* tail, float* targets)
{
    if (bad(K, 0)) return -1;
    const OitK        k = make_k(K, W, H, nullptr, camera, layers, tail);
    const OitTargetsK t = make_targets(W, H, targets);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) oit_px_attenuate(k, t, x, y);
    return 0;
}
// one transparent draw of the colour pass, blended in place
int mifx_host_oit16_blend(int K, int W, int H, const float* depth, const float* base, const float* material, const float* radiance, const float* ibl, const float* alpha,
                          const float* opaque, const mifx_camera_attribs* camera, const uint32_t* layers, const float* tail, float* targets)
{
    if (bad(K, 0)) return -1;
    const OitK        k = make_k(K, W, H, opaque, camera, layers, tail);
    const OitSliceK   s = make_slice(W, depth, base, material, radiance, ibl, alpha);
    const OitTargetsK t = make_targets(W, H, targets);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) oit_px_blend(k, s, t, x, y);
    return 0;
}
}
