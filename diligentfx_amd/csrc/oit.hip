// oit.hip -- layered order-independent transparency over G-buffer slices (include/mifx.h "layered order-independent transparency"): the kernels, and -- unlike the
// other effects -- the C ABI entries that sequence them.  The per-pixel bodies are mifx_oit.h.
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
//
// Why the entries are here and not in an api_oit.cpp: the launcher declarations of mifx_host.h / mifx_*_host.h are mirrored by a generated block of the CPU product
// build's stand-in (tests/cpu_product/stub_device.cpp), which a change of this kind does not regenerate; the entries therefore call the kernels directly.  Moving
// them out is a follow-up for whoever regenerates that block.
#include "mifx_objects.h"
#include "mifx_oit.h"

using namespace mifx;

struct mifx_oit
{
    mifx_postfx* ctx = nullptr;
    uint32_t     w = 0, h = 0, K = 0;
    void*        layers = nullptr; // w * h * K words
    mifx::Plane  tail;             // F32X2
    ~mifx_oit()
    {
        if (layers) (void)hipFree(layers);
    }
};

// The fused kernels are the default: 2.0 - 3.3 times faster than the sequence at 3840 x 2160, K = 4, L = 2 .. 8, both shapes at the device's copy rate for the bytes
// they move (profiles/oit_bench.json, tools/oit_bench.py; mifx_oit_set_fusion(0) is the sequence).
static bool g_oit_fusion = true;

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
} // namespace mifx

namespace
{
constexpr bool oit_has_fused_kernel(uint32_t K) { return K == 1 || K == 2 || K == 3 || K == 4 || K == 8; }

mifx_status create_check(uint32_t width, uint32_t height, uint32_t layer_count, const char* who)
{
    MIFX_REQUIRE(layer_count >= 1u && layer_count <= uint32_t(MIFX_OIT_MAX_LAYERS), "%s: layer_count %u is outside 1 .. %d", who, layer_count, MIFX_OIT_MAX_LAYERS);
    MIFX_REQUIRE(width >= 1u && height >= 1u && width <= 16384u && height <= 16384u, "%s: %ux%u is empty or larger than 16384", who, width, height);
    return MIFX_OK;
}

struct OitFrameK
{
    OitSlicesK  tab;
    OitTargetsK targets;
    Img         opaque;
    OitCamK     cam;
};

// every argument check of the entries that take slices, an opaque depth, a camera or targets, for an object of w x h
mifx_status frame_check(uint32_t w, uint32_t h, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                        const mifx_oit_targets* targets, const char* who, OitFrameK& f)
{
    f = OitFrameK{};
    MIFX_REQUIRE(count <= uint32_t(MIFX_OIT_MAX_SLICES), "%s: %u slices are more than MIFX_OIT_MAX_SLICES (%d)", who, count, MIFX_OIT_MAX_SLICES);
    MIFX_REQUIRE(count == 0u || (slices != nullptr && camera != nullptr), "%s: null argument (slices, camera)", who);
    if (camera) f.cam = make_oitcamk(*camera);
    if (opaque_depth) MIFX_CHECK(to_img_wh(opaque_depth, MIFX_FORMAT_F32, w, h, "opaque_depth", f.opaque));
    Img im;
    for (uint32_t i = 0; i < count; ++i)
    {
        const mifx_oit_slice& s = slices[i];
        OitSliceK&            o = f.tab.s[i];
        MIFX_REQUIRE(s.depth != nullptr && s.base_color != nullptr, "%s: slice %u: depth and base_color must not be null", who, i);
        MIFX_CHECK(to_img_wh(s.depth, MIFX_FORMAT_F32, w, h, "slice depth", im));
        o.depth = im.p; o.pitchDepth = im.pitch;
        MIFX_CHECK(to_img_wh(s.base_color, MIFX_FORMAT_F32X4, w, h, "slice base_color", im));
        o.base = im.p; o.pitchBase = im.pitch;
        if (!targets) continue;
        MIFX_REQUIRE(s.material != nullptr && s.radiance != nullptr && s.specular_ibl != nullptr, "%s: slice %u: material, radiance and specular_ibl must not be null", who, i);
        MIFX_CHECK(to_img_wh(s.material, MIFX_FORMAT_F32X4, w, h, "slice material", im));
        o.material = im.p; o.pitchMaterial = im.pitch;
        MIFX_CHECK(to_img_wh(s.radiance, MIFX_FORMAT_F32X4, w, h, "slice radiance", im));
        o.radiance = im.p; o.pitchRadiance = im.pitch;
        MIFX_CHECK(to_img_wh(s.specular_ibl, MIFX_FORMAT_F32X4, w, h, "slice specular_ibl", im));
        o.ibl = im.p; o.pitchIbl = im.pitch;
        if (s.color_alpha)
        {
            MIFX_CHECK(to_img_wh(s.color_alpha, MIFX_FORMAT_F32, w, h, "slice color_alpha", im));
            o.alpha = im.p; o.pitchAlpha = im.pitch;
        }
    }
    f.tab.count = int(count);
    if (targets)
    {
        MIFX_REQUIRE(targets->color != nullptr && targets->base_color != nullptr && targets->material != nullptr && targets->ibl != nullptr, "%s: a target is null", who);
        MIFX_CHECK(to_img_wh(targets->color, MIFX_FORMAT_F32X4, w, h, "target color", f.targets.color));
        MIFX_CHECK(to_img_wh(targets->base_color, MIFX_FORMAT_F32X4, w, h, "target base_color", f.targets.base));
        MIFX_CHECK(to_img_wh(targets->material, MIFX_FORMAT_F32X4, w, h, "target material", f.targets.material));
        MIFX_CHECK(to_img_wh(targets->ibl, MIFX_FORMAT_F32X4, w, h, "target ibl", f.targets.ibl));
    }
    return MIFX_OK;
}

OitK make_oitk(const mifx_oit* o, const OitFrameK& f)
{
    OitK k{};
    k.layers = static_cast<unsigned char*>(o->layers);
    k.tail = static_cast<unsigned char*>(o->tail.data);
    k.opaque = f.opaque.p; k.opaquePitch = f.opaque.pitch;
    k.w = int(o->w); k.h = int(o->h); k.K = int(o->K); k.tailPitch = int(o->tail.pitch);
    k.cam = f.cam;
    return k;
}
dim3 oit_block() { return dim3(64, 4, 1); }
dim3 oit_grid(const mifx_oit* o) { return dim3((o->w + 63u) / 64u, (o->h + 3u) / 4u, 1); }

mifx_status run_clear(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_clear_kernel");
    hipLaunchKernelGGL(oit_clear_kernel, oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f));
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
mifx_status run_update(mifx_oit* o, const OitFrameK& f, int slice)
{
    MifxKernelTimer timer(o->ctx, "oit_update_kernel");
    hipLaunchKernelGGL(oit_update_kernel, oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f), f.tab.s[slice]);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
mifx_status run_attenuate(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_attenuate_kernel");
    hipLaunchKernelGGL(oit_attenuate_kernel, oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f), f.targets);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
mifx_status run_blend(mifx_oit* o, const OitFrameK& f, int slice)
{
    MifxKernelTimer timer(o->ctx, "oit_blend_kernel");
    hipLaunchKernelGGL(oit_blend_kernel, oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f), f.tab.s[slice], f.targets);
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
#define MIFX_OIT_BY_K(LAUNCH)        \
    switch (o->K)                    \
    {                                \
        case 1: LAUNCH(1); break;    \
        case 2: LAUNCH(2); break;    \
        case 3: LAUNCH(3); break;    \
        case 4: LAUNCH(4); break;    \
        default: LAUNCH(8); break;   \
    }
mifx_status run_build(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_build_kernel");
#define MIFX_LAUNCH_BUILD(K) hipLaunchKernelGGL((oit_build_kernel<K>), oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f), f.tab)
    MIFX_OIT_BY_K(MIFX_LAUNCH_BUILD)
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
mifx_status run_resolve(mifx_oit* o, const OitFrameK& f)
{
    MifxKernelTimer timer(o->ctx, "oit_resolve_kernel");
#define MIFX_LAUNCH_RESOLVE(K) hipLaunchKernelGGL((oit_resolve_kernel<K>), oit_grid(o), oit_block(), 0, o->ctx->stream, make_oitk(o, f), f.tab, f.targets)
    MIFX_OIT_BY_K(MIFX_LAUNCH_RESOLVE)
    MIFX_HIP_CHECK(hipGetLastError());
    return MIFX_OK;
}
} // namespace

extern "C" {

mifx_status mifx_oit_create_check(uint32_t width, uint32_t height, uint32_t layer_count) { return create_check(width, height, layer_count, "mifx_oit_create_check"); }

mifx_status mifx_oit_frame_check(uint32_t width, uint32_t height, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                                 const mifx_oit_targets* targets)
{
    OitFrameK f;
    MIFX_CHECK(create_check(width, height, 1u, "mifx_oit_frame_check"));
    return frame_check(width, height, slices, count, opaque_depth, camera, targets, "mifx_oit_frame_check", f);
}

int32_t mifx_oit_set_fusion(int32_t enable)
{
    const int32_t prev = g_oit_fusion ? 1 : 0;
    g_oit_fusion       = enable != 0;
    return prev;
}

// PBR_Renderer::CreateOITResources
mifx_status mifx_oit_create(mifx_postfx* ctx, uint32_t width, uint32_t height, uint32_t layer_count, mifx_oit** out)
{
    const char* who = "mifx_oit_create";
    MIFX_REQUIRE(ctx != nullptr && out != nullptr, "%s: null argument", who);
    MIFX_CHECK(create_check(width, height, layer_count, who));
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    mifx_oit* o = new mifx_oit();
    o->ctx = ctx; o->w = width; o->h = height; o->K = layer_count;
    mifx_status st = o->tail.alloc(width, height, MIFX_FORMAT_F32X2);
    if (st >= 0 && hipMalloc(&o->layers, size_t(width) * height * layer_count * 4u) != hipSuccess)
    {
        set_error("%s: hipMalloc of %zu bytes for the layers failed", who, size_t(width) * height * layer_count * 4u);
        o->layers = nullptr;
        st        = MIFX_ERR_HIP;
    }
    if (st < 0)
    {
        delete o;
        return st;
    }
    *out = o;
    return MIFX_OK;
}

void mifx_oit_destroy(mifx_oit* oit) { delete oit; }

mifx_status mifx_oit_get_layers(mifx_oit* oit, void** out_data, uint64_t* out_words)
{
    MIFX_REQUIRE(oit != nullptr && out_data != nullptr && out_words != nullptr, "mifx_oit_get_layers: null argument");
    *out_data  = oit->layers;
    *out_words = uint64_t(oit->w) * oit->h * oit->K;
    return MIFX_OK;
}

mifx_status mifx_oit_get_tail(mifx_oit* oit, mifx_image2d* out)
{
    MIFX_REQUIRE(oit != nullptr && out != nullptr, "mifx_oit_get_tail: null argument");
    *out = oit->tail.desc();
    return MIFX_OK;
}

#define MIFX_OIT_RUN(...)                          \
    MIFX_HIP_CHECK(hipSetDevice(oit->ctx->device)); \
    __VA_ARGS__                                    \
    return MIFX_OK

// ClearOITLayers.csh, and the tail's clear value of HnBeginOITPassTask.cpp:139-144
mifx_status mifx_oit_clear_layers(mifx_oit* oit)
{
    const char* who = "mifx_oit_clear_layers";
    MIFX_REQUIRE(oit != nullptr, "%s: null object", who);
    OitFrameK f{};
    MIFX_OIT_RUN(MIFX_CHECK(run_clear(oit, f)););
}

// UpdateOITLayers.psh:54-109 with BS_UpdateOITTail (PBR_Renderer.cpp:1849-1865)
mifx_status mifx_oit_update_layers(mifx_oit* oit, const mifx_oit_slice* slice, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera)
{
    const char* who = "mifx_oit_update_layers";
    MIFX_REQUIRE(oit != nullptr && slice != nullptr && camera != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slice, 1u, opaque_depth, camera, nullptr, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_update(oit, f, 0)););
}

// ApplyOITAttenuation.psh with BS_OITAttenuation (PBR_Renderer.cpp:2309-2324)
mifx_status mifx_oit_apply_attenuation(mifx_oit* oit, const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_apply_attenuation";
    MIFX_REQUIRE(oit != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, nullptr, 0u, nullptr, nullptr, targets, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_attenuate(oit, f)););
}

// one transparent draw: RenderPBR.psh:388-418, :544-559, :632, USD_Renderer.cpp:122-167, the blend state of PBR_Renderer.cpp:2096-2127
mifx_status mifx_oit_blend(mifx_oit* oit, const mifx_oit_slice* slice, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera, const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_blend";
    MIFX_REQUIRE(oit != nullptr && slice != nullptr && camera != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slice, 1u, opaque_depth, camera, targets, who, f));
    MIFX_OIT_RUN(MIFX_CHECK(run_blend(oit, f, 0)););
}

// clear_layers, then update_layers of every slice: one launch where a fused kernel exists for the layer count and the fusion is on
mifx_status mifx_oit_build_layers(mifx_oit* oit, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera)
{
    const char* who = "mifx_oit_build_layers";
    MIFX_REQUIRE(oit != nullptr, "%s: null object", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slices, count, opaque_depth, camera, nullptr, who, f));
    MIFX_OIT_RUN(
        if (g_oit_fusion && oit_has_fused_kernel(oit->K)) MIFX_CHECK(run_build(oit, f));
        else
        {
            MIFX_CHECK(run_clear(oit, f));
            for (uint32_t i = 0; i < count; ++i) MIFX_CHECK(run_update(oit, f, int(i)));
        });
}

// apply_attenuation, then blend of every slice
mifx_status mifx_oit_resolve(mifx_oit* oit, const mifx_oit_slice* slices, uint32_t count, const mifx_image2d* opaque_depth, const mifx_camera_attribs* camera,
                             const mifx_oit_targets* targets)
{
    const char* who = "mifx_oit_resolve";
    MIFX_REQUIRE(oit != nullptr && targets != nullptr, "%s: null argument", who);
    OitFrameK f;
    MIFX_CHECK(frame_check(oit->w, oit->h, slices, count, opaque_depth, camera, targets, who, f));
    MIFX_OIT_RUN(
        if (g_oit_fusion && oit_has_fused_kernel(oit->K)) MIFX_CHECK(run_resolve(oit, f));
        else
        {
            MIFX_CHECK(run_attenuate(oit, f));
            for (uint32_t i = 0; i < count; ++i) MIFX_CHECK(run_blend(oit, f, int(i)));
        });
}

} // extern "C"
