// api_material.cpp -- C ABI of the material fetch (include/mifx.h "material fetch": mifx_pbr_material_fetch, mifx_pbr_material_fetch_check): the argument checks of both
// entries, the material and texture tables as the kernel reads them (kept on the context, uploaded when they differ from the last call's) and the launch, whose launcher
// is in material.hip (mifx_material_host.h).
#include "mifx_objects.h"
#include "mifx_material_host.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mifx;

namespace
{
const char* const kSlotNames[MIFX_PBR_TEXTURE_COUNT] = {"BASE_COLOR", "PHYS_DESC", "NORMAL", "OCCLUSION", "EMISSIVE", "METALLIC", "ROUGHNESS", "CLEAR_COAT", "CLEAR_COAT_ROUGHNESS",
                                                        "CLEAR_COAT_NORMAL", "SHEEN_COLOR", "SHEEN_ROUGHNESS", "ANISOTROPY", "IRIDESCENCE", "IRIDESCENCE_THICKNESS", "TRANSMISSION"};
constexpr uint32_t kKnownLayers = MIFX_PBR_LAYER_CLEAR_COAT | MIFX_PBR_LAYER_SHEEN | MIFX_PBR_LAYER_ANISOTROPY | MIFX_PBR_LAYER_IRIDESCENCE | MIFX_PBR_LAYER_TRANSMISSION;
constexpr uint32_t kKnownFlags  = MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS | MIFX_MATERIAL_FETCH_FLAG_TEXCOORD_TRANSFORM | MIFX_MATERIAL_FETCH_FLAG_SRGB_TO_LINEAR;

// the layer a slot belongs to (0: the base layer): a slot of a layer that is off is not read
uint32_t slot_layer(int slot)
{
    switch (slot)
    {
        case MIFX_PBR_TEXTURE_CLEAR_COAT: case MIFX_PBR_TEXTURE_CLEAR_COAT_ROUGHNESS: case MIFX_PBR_TEXTURE_CLEAR_COAT_NORMAL: return MIFX_PBR_LAYER_CLEAR_COAT;
        case MIFX_PBR_TEXTURE_SHEEN_COLOR: case MIFX_PBR_TEXTURE_SHEEN_ROUGHNESS: return MIFX_PBR_LAYER_SHEEN;
        case MIFX_PBR_TEXTURE_ANISOTROPY: return MIFX_PBR_LAYER_ANISOTROPY;
        case MIFX_PBR_TEXTURE_IRIDESCENCE: case MIFX_PBR_TEXTURE_IRIDESCENCE_THICKNESS: return MIFX_PBR_LAYER_IRIDESCENCE;
        case MIFX_PBR_TEXTURE_TRANSMISSION: return MIFX_PBR_LAYER_TRANSMISSION;
        default: return 0u;
    }
}

// Every check of both entries (no device call); fills what the launch needs: the kernel's constants and the texture descriptors as the kernel reads them.
mifx_status check_material_fetch(const char* who, const mifx_material_interpolants* in, const mifx_material_fetch_desc* d, const mifx_camera_attribs* camera, const mifx_gbuffer* g,
                                 const mifx_pbr_layers* layers, MaterialFetchK& k, std::vector<MaterialTexK>& textures)
{
    static_assert(sizeof(mifx_pbr_texture_attribs) == 48 && sizeof(mifx_pbr_material) == 1008 && sizeof(mifx_texture_array) == 40 && sizeof(mifx_material_fetch_desc) == 48 &&
                      sizeof(mifx_material_interpolants) == 56 && sizeof(MaterialTexK) == 104,
                  "PBR_Structures.fxh:245-254; include/mifx.h");
    MIFX_REQUIRE(in != nullptr && d != nullptr && camera != nullptr && g != nullptr, "%s: null argument (interpolants, desc, camera and gbuffer are required)", who);
    std::memset(&k, 0, sizeof(k));
    MIFX_REQUIRE(in->depth != nullptr, "%s: interpolants->depth is required", who);
    MIFX_CHECK(to_img(in->depth, MIFX_FORMAT_F32, "interpolants->depth", k.depth));
    const uint32_t w = in->depth->width, h = in->depth->height;
    if (in->uv0) MIFX_CHECK(to_img_wh(in->uv0, MIFX_FORMAT_F32X2, w, h, "interpolants->uv0", k.uv0));
    if (in->uv1) MIFX_CHECK(to_img_wh(in->uv1, MIFX_FORMAT_F32X2, w, h, "interpolants->uv1", k.uv1));
    if (in->mesh_normal) MIFX_CHECK(to_img_wh(in->mesh_normal, MIFX_FORMAT_F32X4, w, h, "interpolants->mesh_normal", k.meshNormal));
    if (in->color) MIFX_CHECK(to_img_wh(in->color, MIFX_FORMAT_F32X4, w, h, "interpolants->color", k.color));
    if (in->face) MIFX_CHECK(to_img_wh(in->face, MIFX_FORMAT_F32, w, h, "interpolants->face", k.face));
    if (in->material_index) MIFX_CHECK(to_img_wh(in->material_index, MIFX_FORMAT_F32, w, h, "interpolants->material_index", k.index));

    MIFX_REQUIRE((d->layer_flags & ~kKnownLayers) == 0u, "%s: desc->layer_flags has unknown bits 0x%x", who, d->layer_flags & ~kKnownLayers);
    MIFX_REQUIRE((d->flags & ~kKnownFlags) == 0u, "%s: desc->flags has unknown bits 0x%x", who, d->flags & ~kKnownFlags);
    MIFX_REQUIRE(std::isfinite(d->mip_bias), "%s: desc->mip_bias is not finite", who);
    MIFX_REQUIRE(d->materials != nullptr && d->material_count > 0 && d->material_count <= 65536u, "%s: desc->materials is null or desc->material_count (%u) outside [1, 65536]", who,
                 d->material_count);
    MIFX_REQUIRE(d->texture_count <= 65536u && (d->textures != nullptr || d->texture_count == 0), "%s: desc->textures is null with desc->texture_count %u (at most 65536)", who,
                 d->texture_count);
    MIFX_REQUIRE(layers != nullptr || d->layer_flags == 0u, "%s: layers is null with desc->layer_flags 0x%x", who, d->layer_flags);

    // ---- the texture table
    textures.assign(d->texture_count, MaterialTexK{});
    for (uint32_t i = 0; i < d->texture_count; ++i)
    {
        const mifx_texture_array& t = d->textures[i];
        MIFX_REQUIRE(t.data != nullptr && t.width > 0 && t.height > 0 && t.slices > 0 && t.width <= 16384u && t.height <= 16384u && t.slices <= 2048u,
                     "%s: desc->textures[%u] is null or %ux%ux%u (each side at most 16384, at most 2048 slices)", who, i, t.width, t.height, t.slices);
        MIFX_REQUIRE(t.format == MIFX_NATIVE_FORMAT_RGBA32_FLOAT || t.format == MIFX_NATIVE_FORMAT_RGBA8_UNORM,
                     "%s: desc->textures[%u].format %u: MIFX_NATIVE_FORMAT_RGBA32_FLOAT or MIFX_NATIVE_FORMAT_RGBA8_UNORM", who, i, t.format);
        uint32_t full = 1;
        while ((std::max(t.width, t.height) >> full) != 0u) ++full;
        MIFX_REQUIRE(t.mips >= 1 && t.mips <= full, "%s: desc->textures[%u].mips %u outside [1, %u] for %ux%u", who, i, t.mips, full, t.width, t.height);
        const uint32_t ts = t.format == MIFX_NATIVE_FORMAT_RGBA8_UNORM ? 4u : 16u;
        uint64_t       texels = 0;
        for (uint32_t l = 0; l < t.mips; ++l) texels += uint64_t(std::max(t.width >> l, 1u)) * std::max(t.height >> l, 1u);
        MIFX_REQUIRE(texels * ts <= 0xFFFFFFFFull, "%s: desc->textures[%u]: a slice of %llu bytes exceeds the 4 GiB addressing limit of one slice", who, i,
                     static_cast<unsigned long long>(texels * ts));
        MIFX_REQUIRE(t.slice_pitch_bytes >= texels * ts && t.slice_pitch_bytes % ts == 0 && reinterpret_cast<uintptr_t>(t.data) % ts == 0,
                     "%s: desc->textures[%u].slice_pitch_bytes %llu / data alignment: the chain of a slice is %llu bytes of %u-byte texels", who, i,
                     static_cast<unsigned long long>(t.slice_pitch_bytes), static_cast<unsigned long long>(texels * ts), ts);
        textures[i] = make_material_texk(t);
    }

    // ---- the material table: one workflow, one iridescence IOR and one anisotropy rotation per call (the lighting takes one of each)
    const mifx_pbr_material& m0 = d->materials[0];
    bool anyClearcoatNormalMap = false;
    for (uint32_t i = 0; i < d->material_count; ++i)
    {
        const mifx_pbr_material& m = d->materials[i];
        MIFX_REQUIRE(m.basic.Workflow != 2, "%s: desc->materials[%u].basic.Workflow is PBR_WORKFLOW_UNLIT: an unlit material has a base colour only (describe it as metallic-roughness "
                     "and shade it with mifx_pbr_shade_output's unlit)", who, i);
        MIFX_REQUIRE(m.basic.Workflow == MIFX_PBR_WORKFLOW_METALLIC_ROUGHNESS || m.basic.Workflow == MIFX_PBR_WORKFLOW_SPECULAR_GLOSSINESS,
                     "%s: desc->materials[%u].basic.Workflow %d is unknown", who, i, m.basic.Workflow);
        MIFX_REQUIRE(m.basic.Workflow == m0.basic.Workflow, "%s: desc->materials[%u].basic.Workflow %d differs from materials[0]'s %d: the lighting takes one workflow per call", who, i,
                     m.basic.Workflow, m0.basic.Workflow);
        MIFX_REQUIRE(!(d->layer_flags & MIFX_PBR_LAYER_IRIDESCENCE) || m.iridescence.IOR == m0.iridescence.IOR,
                     "%s: desc->materials[%u].iridescence.IOR %g differs from materials[0]'s %g: the lighting takes one iridescence IOR per call", who, i, double(m.iridescence.IOR),
                     double(m0.iridescence.IOR));
        MIFX_REQUIRE(!(d->layer_flags & MIFX_PBR_LAYER_ANISOTROPY) || m.anisotropy.Rotation == m0.anisotropy.Rotation,
                     "%s: desc->materials[%u].anisotropy.Rotation %g differs from materials[0]'s %g: the lighting takes one anisotropy rotation per call", who, i,
                     double(m.anisotropy.Rotation), double(m0.anisotropy.Rotation));
        MIFX_REQUIRE(m.basic.Workflow != MIFX_PBR_WORKFLOW_SPECULAR_GLOSSINESS ||
                         (m.basic.SpecularFactorR == 1.0f && m.basic.SpecularFactorG == 1.0f && m.basic.SpecularFactorB == 1.0f),
                     "%s: desc->materials[%u].basic.SpecularFactor (%g, %g, %g) is not 1: the shade converts the specular-glossiness plane from sRGB itself and applies no factor", who, i,
                     double(m.basic.SpecularFactorR), double(m.basic.SpecularFactorG), double(m.basic.SpecularFactorB));
        for (int s = 0; s < MIFX_PBR_TEXTURE_COUNT; ++s)
        {
            const int32_t t = m.texture[s];
            MIFX_REQUIRE(t >= -1 && (t < 0 || uint32_t(t) < d->texture_count), "%s: desc->materials[%u].texture[%s] = %d is outside the texture table of %u entries", who, i,
                         kSlotNames[s], t, d->texture_count);
            if (t < 0) continue;
            MIFX_REQUIRE(in->uv0 != nullptr || in->uv1 != nullptr, "%s: desc->materials[%u].texture[%s] is present while interpolants->uv0 and interpolants->uv1 are both null", who, i,
                         kSlotNames[s]);
            if (slot_layer(s) != 0u && !(d->layer_flags & slot_layer(s))) continue; // (not read)
            if (s == MIFX_PBR_TEXTURE_CLEAR_COAT_NORMAL) anyClearcoatNormalMap = true;
            const mifx_pbr_texture_attribs& a = m.textures[s];
            MIFX_REQUIRE(std::isfinite(a.TextureSlice) && std::isfinite(a.UBias) && std::isfinite(a.VBias), "%s: desc->materials[%u].textures[%s]: non-finite slice or bias", who, i,
                         kSlotNames[s]);
            if (d->flags & MIFX_MATERIAL_FETCH_FLAG_TEXTURE_ATLAS)
            {
                const float *r = a.AtlasUVScaleAndBias, x0 = std::fmin(r[2], r[2] + r[0]), x1 = std::fmax(r[2], r[2] + r[0]), y0 = std::fmin(r[3], r[3] + r[1]),
                            y1 = std::fmax(r[3], r[3] + r[1]);
                MIFX_REQUIRE(x0 >= 0.0f && y0 >= 0.0f && x1 <= 1.0f && y1 <= 1.0f, // (NaN fails)
                             "%s: desc->materials[%u].textures[%s].AtlasUVScaleAndBias (%g, %g, %g, %g): the atlas region lies outside [0, 1]", who, i, kSlotNames[s], double(r[0]),
                             double(r[1]), double(r[2]), double(r[3]));
            }
        }
    }

    // ---- the output planes
    MIFX_REQUIRE(g->base_color != nullptr && g->normal != nullptr && g->material != nullptr, "%s: gbuffer->base_color, gbuffer->normal and gbuffer->material are required", who);
    MIFX_CHECK(to_img_wh(g->base_color, MIFX_FORMAT_F32X4, w, h, "gbuffer->base_color", k.outBaseColor));
    MIFX_CHECK(to_img_wh(g->normal, MIFX_FORMAT_F32X4, w, h, "gbuffer->normal", k.outNormal));
    MIFX_CHECK(to_img_wh(g->material, MIFX_FORMAT_F32X4, w, h, "gbuffer->material", k.outMaterial));
    if (g->emissive) MIFX_CHECK(to_img_wh(g->emissive, MIFX_FORMAT_F32X4, w, h, "gbuffer->emissive", k.outEmissive));
    if (g->occlusion) MIFX_CHECK(to_img_wh(g->occlusion, MIFX_FORMAT_F32, w, h, "gbuffer->occlusion", k.outOcclusion));
    if (d->layer_flags & MIFX_PBR_LAYER_CLEAR_COAT)
    {
        MIFX_CHECK(to_img_wh(layers->clearcoat, MIFX_FORMAT_F32X4, w, h, "layers->clearcoat", k.outClearcoat));
        if (anyClearcoatNormalMap) MIFX_CHECK(to_img_wh(layers->clearcoat_normal, MIFX_FORMAT_F32X4, w, h, "layers->clearcoat_normal", k.outClearcoatNormal));
        else
            MIFX_REQUIRE(layers->clearcoat_normal == nullptr,
                         "%s: layers->clearcoat_normal must be null: no material has a CLEAR_COAT_NORMAL map, and the shade reads null as the G-buffer normal", who);
    }
    if (d->layer_flags & MIFX_PBR_LAYER_SHEEN) MIFX_CHECK(to_img_wh(layers->sheen, MIFX_FORMAT_F32X4, w, h, "layers->sheen", k.outSheen));
    if (d->layer_flags & MIFX_PBR_LAYER_ANISOTROPY) MIFX_CHECK(to_img_wh(layers->anisotropy, MIFX_FORMAT_F32X4, w, h, "layers->anisotropy", k.outAnisotropy));
    if (d->layer_flags & MIFX_PBR_LAYER_IRIDESCENCE) MIFX_CHECK(to_img_wh(layers->iridescence, MIFX_FORMAT_F32X4, w, h, "layers->iridescence", k.outIridescence));
    if (d->layer_flags & MIFX_PBR_LAYER_TRANSMISSION) MIFX_CHECK(to_img_wh(layers->transmission, MIFX_FORMAT_F32, w, h, "layers->transmission", k.outTransmission));
    // no output may alias another output or an input: a pixel reads its quad partners' interpolants while they store
    const Img* const outs[11] = {&k.outBaseColor, &k.outNormal, &k.outMaterial, &k.outEmissive, &k.outOcclusion, &k.outClearcoat, &k.outClearcoatNormal, &k.outSheen, &k.outAnisotropy,
                                 &k.outIridescence, &k.outTransmission};
    static const char* const outNames[11] = {"gbuffer->base_color", "gbuffer->normal", "gbuffer->material", "gbuffer->emissive", "gbuffer->occlusion", "layers->clearcoat",
                                             "layers->clearcoat_normal", "layers->sheen", "layers->anisotropy", "layers->iridescence", "layers->transmission"};
    const Img* const ins[7] = {&k.depth, &k.uv0, &k.uv1, &k.meshNormal, &k.color, &k.face, &k.index};
    static const char* const inNames[7] = {"depth", "uv0", "uv1", "mesh_normal", "color", "face", "material_index"};
    for (int i = 0; i < 11; ++i)
    {
        if (outs[i]->p == nullptr) continue;
        for (int j = 0; j < i; ++j) MIFX_REQUIRE(outs[j]->p != outs[i]->p, "%s: %s aliases %s", who, outNames[i], outNames[j]);
        for (int j = 0; j < 7; ++j) MIFX_REQUIRE(ins[j]->p != outs[i]->p, "%s: %s aliases interpolants->%s", who, outNames[i], inNames[j]);
    }
    k.materialCount = int(d->material_count);
    k.textureCount  = int(d->texture_count);
    k.layers   = d->layer_flags;
    k.flags    = d->flags;
    k.mipBias  = d->mip_bias;
    k.handness = camera->fHandness;
    k.workflow = m0.basic.Workflow;
    return MIFX_OK;
}
} // namespace

extern "C" {

mifx_status mifx_pbr_material_fetch_check(const mifx_material_interpolants* interpolants, const mifx_material_fetch_desc* desc, const mifx_camera_attribs* camera,
                                          const mifx_gbuffer* gbuffer, const mifx_pbr_layers* layers)
{
    MaterialFetchK            k;
    std::vector<MaterialTexK> textures;
    return check_material_fetch("mifx_pbr_material_fetch_check", interpolants, desc, camera, gbuffer, layers, k, textures);
}

mifx_status mifx_pbr_material_fetch(mifx_postfx* ctx, const mifx_material_interpolants* interpolants, const mifx_material_fetch_desc* desc, const mifx_camera_attribs* camera,
                                    const mifx_gbuffer* gbuffer, const mifx_pbr_layers* layers)
{
    // (every argument check precedes the first device call)
    MIFX_REQUIRE(ctx != nullptr, "mifx_pbr_material_fetch: null context");
    MaterialFetchK            k;
    std::vector<MaterialTexK> textures;
    MIFX_CHECK(check_material_fetch("mifx_pbr_material_fetch", interpolants, desc, camera, gbuffer, layers, k, textures));
#ifdef MIFX_STORAGE_H4
    ::mifx::set_error("mifx_pbr_material_fetch: the material fetch is not part of the native-storage build yet");
    return MIFX_ERR_NOT_IMPLEMENTED;
#else
    MIFX_REQUIRE(ctx->need.empty() && ctx->band.empty(), "mifx_pbr_material_fetch: not available inside a row band");
    MIFX_HIP_CHECK(hipSetDevice(ctx->device));
    // The tables as the kernel reads them: the material records, then the texture descriptors.  Uploaded when they differ from the last call's (a frame's calls share them);
    // the upload waits for the stream first, because a fetch queued earlier may still be reading the old tables.
    const size_t materialBytes = size_t(desc->material_count) * sizeof(mifx_pbr_material), textureBytes = textures.size() * sizeof(MaterialTexK);
    std::vector<unsigned char> blob(materialBytes + textureBytes);
    std::memcpy(blob.data(), desc->materials, materialBytes);
    if (textureBytes) std::memcpy(blob.data() + materialBytes, textures.data(), textureBytes);
    if (blob != ctx->material_tables_host || ctx->material_tables.data == nullptr)
    {
        MIFX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->material_tables_host.clear();
        MIFX_CHECK(ctx->material_tables.reserve(blob.size()));
        MIFX_HIP_CHECK(hipMemcpy(ctx->material_tables.data, blob.data(), blob.size(), hipMemcpyHostToDevice));
        ctx->material_tables_host.swap(blob);
    }
    k.materials = static_cast<const mifx_pbr_material*>(ctx->material_tables.data);
    k.textures  = reinterpret_cast<const MaterialTexK*>(static_cast<const unsigned char*>(ctx->material_tables.data) + materialBytes);
    MifxKernelTimer timer(ctx, "material_fetch_kernel");
    return launch_material_fetch(ctx->stream, k, make_camk(*camera, (ctx->flags & MIFX_POSTFX_FEATURE_FLAG_REVERSED_DEPTH) != 0));
#endif
}

} // extern "C"
