// TEST INFRASTRUCTURE ONLY.  The order-independent-transparency bodies (diligentfx_amd/csrc/mifx_oit.h) compiled for the HOST (see layers_host.cpp for the method):
//   * the reference's sequence, pixel by pixel in launch order: oit_clear_kernel, one oit_update_kernel per slice, oit_attenuate_kernel, one oit_blend_kernel per slice;
//   * the fused kernels' pixel programs (oit_build_kernel<K>, oit_resolve_kernel<K>), the layers buffer poisoned beforehand.
// Nothing in diligentfx_amd/ builds, loads or calls this.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include <vector>
#include "mifx.h"
#include "mifx_oit.h"

using namespace mifx;

namespace
{
struct Frame
{
    OitK        k;
    OitSlicesK  tab;
    OitTargetsK t;
};
unsigned char* bytes(const void* p) { return reinterpret_cast<unsigned char*>(const_cast<void*>(p)); }

// planes tightly packed: depth / alpha / opaque W floats a row, the 4-channel planes 4 W; slice l of a plane array follows slice l - 1
Frame make_frame(int K, int W, int H, int L, const float* depth, const float* base, const float* material, const float* radiance, const float* ibl, const float* alpha,
                 const float* opaque, const mifx_camera_attribs* camera, uint32_t* layers, float* tail, float* targets)
{
    Frame f{};
    f.k = OitK{bytes(layers), bytes(tail), opaque ? bytes(opaque) : nullptr, W, H, K, W * 8, W * 4, make_oitcamk(*camera)};
    const size_t n = size_t(W) * H;
    for (int l = 0; l < L; ++l)
        f.tab.s[l] = OitSliceK{bytes(depth + l * n), bytes(base + 4 * l * n), bytes(material + 4 * l * n), bytes(radiance + 4 * l * n), bytes(ibl + 4 * l * n),
                               alpha ? bytes(alpha + l * n) : nullptr, W * 4, W * 16, W * 16, W * 16, W * 16, W * 4};
    f.tab.count = L;
    Img* im[4] = {&f.t.color, &f.t.base, &f.t.material, &f.t.ibl};
    for (int j = 0; j < 4; ++j) *im[j] = Img{bytes(targets + 4 * j * n), W, H, W * 16, 0, 0};
    return f;
}

template <class PX> void every_pixel(int W, int H, PX&& px)
{
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) px(x, y);
}

template <int K> void fused(const Frame& f)
{
    every_pixel(f.k.w, f.k.h, [&](int x, int y) { oit_px_build<K>(f.k, f.tab, x, y); });
    every_pixel(f.k.w, f.k.h, [&](int x, int y) { oit_px_resolve<K>(f.k, f.tab, f.t, x, y); });
}
} // namespace

extern "C" {
// layers: H x W x K words, tail: H x W x 2, targets: 4 x H x W x 4 (colour, base colour, material, IBL; blended in place).  Returns 0, or -1 for a bad K / L.
int mifx_host_oit_sequence(int K, int W, int H, int L, const float* depth, const float* base, const float* material, const float* radiance, const float* ibl, const float* alpha,
                           const float* opaque, const mifx_camera_attribs* camera, uint32_t* layers, float* tail, float* targets)
{
    if (K < 1 || K > MIFX_OIT_MAX_LAYERS || L < 0 || L > MIFX_OIT_MAX_SLICES) return -1;
    const Frame f = make_frame(K, W, H, L, depth, base, material, radiance, ibl, alpha, opaque, camera, layers, tail, targets);
    every_pixel(W, H, [&](int x, int y) { oit_px_clear(f.k, x, y); });
    for (int l = 0; l < L; ++l) every_pixel(W, H, [&](int x, int y) { oit_px_update(f.k, f.tab.s[l], x, y); });
    every_pixel(W, H, [&](int x, int y) { oit_px_attenuate(f.k, f.t, x, y); });
    for (int l = 0; l < L; ++l) every_pixel(W, H, [&](int x, int y) { oit_px_blend(f.k, f.tab.s[l], f.t, x, y); });
    return 0;
}

// the same through the fused kernels' pixel programs; -2 for a layer count without a fused kernel (the library then takes the sequence)
int mifx_host_oit_fused(int K, int W, int H, int L, const float* depth, const float* base, const float* material, const float* radiance, const float* ibl, const float* alpha,
                        const float* opaque, const mifx_camera_attribs* camera, uint32_t* layers, float* tail, float* targets)
{
    if (K < 1 || K > MIFX_OIT_MAX_LAYERS || L < 0 || L > MIFX_OIT_MAX_SLICES) return -1;
    const Frame f = make_frame(K, W, H, L, depth, base, material, radiance, ibl, alpha, opaque, camera, layers, tail, targets);
    switch (K)
    {
        case 1: fused<1>(f); break;
        case 2: fused<2>(f); break;
        case 3: fused<3>(f); break;
        case 4: fused<4>(f); break;
        case 8: fused<8>(f); break;
        default: return -2;
    }
    return 0;
}

// One launch of oit.hip on the launcher's own arguments, in place on the memory they name, every pixel in order (tests/cpu_product/device.py: the handlers of the
// host-only build).  which: 0 oit_clear_kernel, 1 oit_update_kernel, 2 oit_attenuate_kernel, 3 oit_blend_kernel, 4 oit_build_kernel<K>, 5 oit_resolve_kernel<K>;
// the arguments a launch does not take are null.  Returns 0; -1 for an unknown launch; -2 for a fused launch at a layer count without a fused kernel.
int mifx_host_oit_launch(int which, const OitK* k, const OitSliceK* slice, const OitSlicesK* tab, const OitTargetsK* t)
{
    const int W = k->w, H = k->h;
    switch (which)
    {
        case 0: every_pixel(W, H, [&](int x, int y) { oit_px_clear(*k, x, y); }); return 0;
        case 1: every_pixel(W, H, [&](int x, int y) { oit_px_update(*k, *slice, x, y); }); return 0;
        case 2: every_pixel(W, H, [&](int x, int y) { oit_px_attenuate(*k, *t, x, y); }); return 0;
        case 3: every_pixel(W, H, [&](int x, int y) { oit_px_blend(*k, *slice, *t, x, y); }); return 0;
        case 4:
        case 5: break;
        default: return -1;
    }
#define MIFX_HOST_OIT_FUSED(K)                                                                      \
    case K:                                                                                         \
        if (which == 4) every_pixel(W, H, [&](int x, int y) { oit_px_build<K>(*k, *tab, x, y); });  \
        else every_pixel(W, H, [&](int x, int y) { oit_px_resolve<K>(*k, *tab, *t, x, y); });       \
        return 0;
    switch (k->K)
    {
        MIFX_HOST_OIT_FUSED(1)
        MIFX_HOST_OIT_FUSED(2)
        MIFX_HOST_OIT_FUSED(3)
        MIFX_HOST_OIT_FUSED(4)
        MIFX_HOST_OIT_FUSED(8)
        default: return -2;
    }
#undef MIFX_HOST_OIT_FUSED
}

// PackOITLayer and the two unpackers, for the test of the packing itself
uint32_t mifx_host_oit_pack(float depth, float transmittance) { return oit_pack(depth, transmittance); }
float    mifx_host_oit_layer_transmittance(uint32_t layer) { return oit_layer_transmittance(layer); }
}
