// TEST INFRASTRUCTURE ONLY.  The per-pixel body of material_fetch_kernel (diligentfx_amd/csrc/mifx_material.h: the head of the reference's pixel shader over interpolant planes,
// with the sampler and the quad derivatives of include/mifx.h "material fetch"), compiled for the HOST by the test suite as shade_targets_host.cpp compiles the shade's footer:
// `hipcc --cuda-host-only`, __device__ redefined to "host and device".  The kernel's source, not a second implementation, and not a product path.
#include <hip/hip_runtime.h>
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "mifx_material.h"
#include <cstring>
#include <vector>

using namespace mifx;

extern "C" {
struct host_plane { float* data; int w, h, c; int pitch_bytes; }; // pitch_bytes 0: tightly packed
struct host_texture { const void* data; int w, h, slices, mips, rgba8; unsigned long long slice_pitch_bytes; };
// One launch of material.hip on the launcher's own arguments (launch_material_fetch), in place on the memory they name: every pixel's stores are those of the kernel
// (material_fetch_store: only a pixel with a fragment stores).  tests/cpu_product/device.py: the handler of the host-only build.
int mifx_host_material_fetch_launch(const MaterialFetchK* k, const CamK* cam)
{
    const bool atlas = (k->flags & MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS) != 0u;
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < k->depth.h; ++y)
        for (int x = 0; x < k->depth.w; ++x)
        {
            if (atlas) material_fetch_store<true>(x, y, *k, *cam);
            else material_fetch_store<false>(x, y, *k, *cam);
        }
    return 0;
}
// interpolants: depth (c = 1), uv0, uv1 (c = 2), mesh normal, colour (c = 4), face, material index (c = 1); a null plane is the permutation without it
// outputs: base colour, normal, material, emissive (c = 4), occlusion (c = 1), clear coat, its normal, sheen, anisotropy, iridescence (c = 4), transmission (c = 1); null = not written
// materials: material_count records of mifx_pbr_material; textures: as the entry takes them once its checks have passed.  The launch above on these arguments.
int mifx_host_material_fetch(const host_plane* interpolants, const host_plane* outputs, const mifx_pbr_material* materials, int material_count, const host_texture* textures,
                             int texture_count, unsigned layer_flags, unsigned flags, float mip_bias, const mifx_camera_attribs* camera, int reversed_depth)
{
    auto img = [](const host_plane& p) { return p.data ? Img{reinterpret_cast<unsigned char*>(p.data), p.w, p.h, p.pitch_bytes ? p.pitch_bytes : p.w * p.c * 4, 0, 0} : Img{}; };
    std::vector<MaterialTexK> tex(static_cast<size_t>(texture_count > 0 ? texture_count : 1));
    for (int i = 0; i < texture_count; ++i)
    {
        const host_texture& t = textures[i];
        tex[size_t(i)] = make_material_texk(mifx_texture_array{t.data, uint32_t(t.w), uint32_t(t.h), uint32_t(t.slices), uint32_t(t.mips),
                                                               uint32_t(t.rgba8 ? MIFX_NATIVE_FORMAT_RGBA8_UNORM : MIFX_NATIVE_FORMAT_RGBA32_FLOAT), 0u, t.slice_pitch_bytes});
    }
    MaterialFetchK k;
    std::memset(&k, 0, sizeof(k));
    k.depth = img(interpolants[0]); k.uv0 = img(interpolants[1]); k.uv1 = img(interpolants[2]); k.meshNormal = img(interpolants[3]); k.color = img(interpolants[4]);
    k.face = img(interpolants[5]); k.index = img(interpolants[6]);
    k.outBaseColor = img(outputs[0]); k.outNormal = img(outputs[1]); k.outMaterial = img(outputs[2]); k.outEmissive = img(outputs[3]); k.outOcclusion = img(outputs[4]);
    k.outClearcoat = img(outputs[5]); k.outClearcoatNormal = img(outputs[6]); k.outSheen = img(outputs[7]); k.outAnisotropy = img(outputs[8]); k.outIridescence = img(outputs[9]);
    k.outTransmission = img(outputs[10]);
    k.materials = materials; k.textures = tex.data(); k.materialCount = material_count; k.textureCount = texture_count;
    k.layers = layer_flags; k.flags = flags; k.mipBias = mip_bias; k.handness = camera->fHandness; k.workflow = materials[0].basic.Workflow;
    const CamK cam = make_camk(*camera, reversed_depth != 0);
    return mifx_host_material_fetch_launch(&k, &cam);
}
}
