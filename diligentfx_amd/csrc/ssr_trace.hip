// MIFX_BUILD_FLAGS: -mllvm -amdgpu-sched-strategy=max-memory-clause
// (build.py reads the line above.  The backend's memory-clause scheduling strategy for this file only: R4 342 -> 330 us in two A/B runs, bit-identical output; the other
//  strategies and the other files lose or do not move -- max-ilp: TAA +19 %, Bloom's final pass +32 %; max-memory-clause on ssr_temporal.hip: R6 +12 % --
//  profiles/r04_ab_sched_strategy.txt.)
// ssr_trace.hip -- ScreenSpaceReflection pass R4 (ray generation + hierarchical march; the other passes are in ssr.hip) (AMD-SSSR-derived stochastic screen-space reflections).
// Math follows Shaders/PostProcess/ScreenSpaceReflection/private/SSR_*.fx; host sequence in api_ssr.cpp.
//
// Masking: the reference marks reflection samples in a D16 depth target and depth-tests R4-R7 against it
// (ScreenSpaceReflection.cpp:47-51,550,626,...).  Here the mask is a float plane (1 = reflection sample); R4 writes 0 to masked-out texels of its two targets, which the
// reference clears every frame (R5 / R6 leave theirs alone, as the reference's depth test does: ssr.hip).
#include "mifx_host.h"
#include "mifx_effects.h"
#include "mifx_pbr.h"

namespace mifx
{


// ------------------------------------------------------------------------------------------------ R4: intersection (SSR_ComputeIntersection.fx:31-335)
// Texture.Load on the depth hierarchy: out of bounds -> 0.  All levels live in one allocation (HizSlab), so a tap is one 32-bit offset from a
// uniform base: the level record {offset, pitch, w, h} comes from LDS (one ds_read_b128), the address is a 32-bit multiply-add.  The slab is read
// through a buffer resource (buffer_load_dword ... offen): an offset computed from coordinates outside the level can be anything, the range check of
// the descriptor turns it into a harmless read (0 beyond the slab), and the value is discarded by the bounds test anyway -- no address select per tap.
// One LDS record per level: the address record and {MipResolution, rcp(MipResolution)} side by side, so that a march step fetches both with one address as soon
// as the next level is known (two ds_read_b128 in flight together instead of one at the end of a step and a dependent one at the start of the next).
struct HizLevel
{
    uint4 addr; // {offset, pitch, w, h}
    v4    res;  // {w_f, h_f, 1 / w_f, 1 / h_f} of the level as the reference carries them
};
// The table has one entry in front of level 0 (a copy of it): the march keeps its level as the byte offset of the entry, (level + 1) * sizeof(HizLevel), and a
// ray that leaves the most detailed level (level -1 when that is level 0) still reads an entry.
struct HizLds
{
    __amdgpu_buffer_rsrc_t rsrc;
    const HizLevel*        lv;
    __amdgpu_buffer_rsrc_t rsrc0; // DIRECT0: level 0 = the caller's depth plane, read where it lies (HizSlab::base0)
};
// DIRECT0 (round 6): level 0 is not in the slab.  A tap picks its descriptor by the lane's level -- two loads under complementary lane masks, one v_cmp and a few scalar
// instructions more per tap; the offset arithmetic is the same (the level-0 record holds offset 0 and the plane's own pitch).  `level0`: this lane's tap is a level-0 tap.
template <bool DIRECT0> MIFX_D float load_hiz(const HizLds& hz, uint4 L, int x, int y, bool level0)
{
    const bool     in  = unsigned(x) < L.z && unsigned(y) < L.w;
    // offset + y * pitch + x * 4 in two instructions (the compiler's own choice is a multiply, a shift and a three-operand add); the 24-bit multiply is exact for
    // every row inside the level (pitch, rows < 2^24)
    unsigned row, off;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(y), "v"(L.y), "v"(L.x));
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(off) : "v"(x), "v"(row));
    float v;
    if (DIRECT0)
    {
        // two loads under complementary lane masks.  (Written plainly, the compiler merges the two calls into one load whose descriptor is a per-lane select and wraps it in
        // a readfirstlane loop -- twice the scalar work and a serialised pair of loads; the differing empty asm statements keep the branches apart.)
        if (level0)
        {
            v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hz.rsrc0, int(off), 0, 0));
            asm volatile("; level 0: the depth plane" : : "v"(off)); // (an operand that is ready: nothing waits for the load here)
        }
        else
        {
            v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hz.rsrc, int(off), 0, 0));
            asm volatile("; levels 1 ..: the slab" : : "v"(off));
        }
    }
    else v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hz.rsrc, int(off), 0, 0));
    return in ? v : 0.0f;
}
template <bool DIRECT0> MIFX_D float load_hiz(const HizLds& hz, int x, int y, int mip) { return load_hiz<DIRECT0>(hz, hz.lv[mip + 1].addr, x, y, mip == 0); }

// HizLevel::res of level m = {MipResolution, rcp(MipResolution)}.  The reference carries both through the loop with exact *2 / *0.5 updates
// (:176-178), so they only ever take the values screen * 2^-m and 1 / (screen * 2^-m): the per-level table in LDS returns the identical
// floats and takes six vector instructions and a branch out of every march step.
// The multiply-adds of a march step stay separate multiplies and adds, as the reference's shader compiler emits them for an fp32 target without contraction.
// (Measured and not taken: fusing 8 of the step's 45 vector instructions is -3 % (round 2), but 1.4e-3 of the specular values of a 224 x 96 frame then differ by
// more than 1e-3 -- rays that cross a tile edge at another step -- where the separate form has none: profiles/r04_parity_outliers_strict_vs_fast.txt.  Parity first, see build.py.)
// Round 3, measured and rejected on the MI355X (tools/ab_gpu.sh; profiles/r03_ab_mlp.txt, r03_ab_r4_alignment.txt, r03_ab_r4_epilogue.txt; every variant passed the
// parity suite).  The counters say the kernel is latency-bound (74 % of the wave cycles parked on s_waitcnt, 13 % issuing VALU, eight waves per SIMD), yet:
//   * the records of both candidate next levels requested from LDS beside the depth tap and selected afterwards (the LDS round trip out of the step's dependent
//     chain): 341 -> 363 us (re-measured over 60 frames at the steady-state clock: 310 -> 330 us) -- eight selects and two more LDS reads per step cost more than the
//     latency they hide;
//   * the pdf, the hit confidence and the edge vignette on 1-ulp reciprocals / square roots with the per-frame quotients (2 / screen, 0.005 2^mip / screen, 1 / fov,
//     1 / thickness) computed on the host: 74 vector instructions less per ray, 328 -> 343 us with an instruction-for-instruction identical march loop;
//   * the march loop aligned to 64 bytes (.p2align, with and without a 32-byte offset): 343 / 342 / 341 us, nothing;
//   * the three loads of the hit validation (depth hierarchy, normal, colour at the hit) issued as one group right after the march instead of behind its early
//     exits: 330 -> 333 us.
//   * the hierarchy stored as 8 x 4-texel tiles of one 128-byte line each (a twin written by the pyramid kernels; six address instructions per tap instead of two),
//     because the L1 counters show 55 of the 64 lanes of a depth tap on a line of their own (profiles/r03_pmc_tcp1_v8.txt): 328.9 -> 330.4 us
//     (profiles/r03_ab_hiz_tiled.txt; re-measured over 60 frames at the steady-state clock: 313.1 vs 313.2 us) -- the tag lookups are not the limit either;
//   * the tiles handed to the XCDs in 128 x 32-pixel chunks so that an L2 serves neighbouring tiles (mifx_device.h, tiled_xy): +3.5 %.
//   * the two coarsest levels of the hierarchy (120x67 + 60x33 texels at 4K, 40 KB) resident in LDS, because HALF of all march steps run there (49 % at levels >= 5,
//     62 % at >= 4: tools/r4_stats.py), as 512-thread workgroups that fill their copy per 512 pixels: 311 -> 418 us (the fill is 80 bytes per pixel); as persistent
//     waves (the grid fills the device once, every workgroup fills its cache once, every wave walks its own sequence of tiles): 400 us, against 418 us for the same
//     persistent kernel WITHOUT the cache -- the cache is worth 4 %, the static tile sequence costs 34 % (profiles/r03_ab_r4_lds_cache.txt).  The taps at the coarse
//     levels were L1 hits already; the step time is set by the taps at the fine levels, which the cache does not touch.  All variants bit-identical.
// What is left is the march itself: 47 steps per wave on average (38.6 per ray; the lanes of a wave are 80 % busy, profiles/r03_r4_march_steps.txt), each a chain
// of a dependent L1/L2 round trip, an LDS read and ~32 vector instructions, at 5.3 resident waves per SIMD on average: ~480 ns per step, 46 % of it covered by the
// other waves' arithmetic.
// REV = SSR_OPTION_INVERTED_DEPTH (:108-113, 118-124): larger depth is closer to the camera
template <bool REV, bool DIRECT0>
MIFX_D v3 hierarchical_raymarch(const HizLds& hiz, v3 origin, v3 dir, v2 screen, int mostDetailedMip, unsigned maxIter, bool& validHit, unsigned& steps) // :139-189
{
    const v3 invDir{dir.x != 0.0f ? fdiv(1.0f, dir.x) : SSR_FLT_MAX, dir.y != 0.0f ? fdiv(1.0f, dir.y) : SSR_FLT_MAX, dir.z != 0.0f ? fdiv(1.0f, dir.z) : SSR_FLT_MAX};
    constexpr int kEntry = int(sizeof(HizLevel));
    const int     loMin  = (mostDetailedMip + 1) * kEntry;
    int           lo     = loMin; // (CurrentMip + 1) * sizeof(HizLevel)
    // (two 16-byte vector loads: a struct copy is split into scalar LDS reads that end up at the top of the step, in front of the address arithmetic)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    auto entry = [&](int o) {
        const char* p = reinterpret_cast<const char*>(hiz.lv) + o;
        const u32x4   a = *reinterpret_cast<const u32x4*>(p);
        const mifx_f4 r = *reinterpret_cast<const mifx_f4*>(p + 16);
        return HizLevel{uint4{a.x, a.y, a.z, a.w}, v4{r.x, r.y, r.z, r.w}};
    };
    HizLevel L = entry(lo);
    v2  mipRes{L.res.x, L.res.y};
    v2  invMipRes{L.res.z, L.res.w};
    // t.z of a step is (surfaceDepth - origin.z) / dir.z for a ray that moves away from the camera and FLT_MAX otherwise (:118-124): a choice per ray
    const bool away = REV ? dir.z < 0.0f : dir.z > 0.0f;
    v2  uvOffset = (0.005f * float(1 << mostDetailedMip)) / screen;
    uvOffset.x = dir.x < 0.0f ? -uvOffset.x : uvOffset.x;
    uvOffset.y = dir.y < 0.0f ? -uvOffset.y : uvOffset.y;
    const v2 floorOffset{dir.x < 0.0f ? 0.0f : 1.0f, dir.y < 0.0f ? 0.0f : 1.0f};

    // InitialAdvanceRay :66-86
    float curT;
    v3    pos;
    {
        const v2 mp = mipRes * mk2(origin.x, origin.y);
        v2 plane{floorf(mp.x) + floorOffset.x, floorf(mp.y) + floorOffset.y};
        plane = plane * invMipRes + uvOffset;
        const v2 t{plane.x * invDir.x - origin.x * invDir.x, plane.y * invDir.y - origin.y * invDir.y};
        curT = fminf(t.x, t.y);
        pos  = origin + curT * dir;
    }
    unsigned idx = 0u;
#ifdef MIFX_R4_STATS
    unsigned coarse5 = 0u, coarse4 = 0u; // steps taken at hierarchy levels >= 5 / >= 4 (tools/r4_stats.py)
#endif
    // Round 6: the march runs at raised wave priority.  A SIMD's eight waves are in different phases -- some in the ~960 vector instructions of the ray set-up or in the
    // hit validation, some in the march, where every step is a dependent chain (tap -> compare -> next level -> LDS record -> next tap) of ~30 instructions.  At equal
    // priority a marching wave whose tap has arrived queues behind the set-up arithmetic of its neighbours; in front of them it asks for its next tap sooner, and the
    // set-up waves lose nothing they were not going to wait for anyway.  s_setprio 3 around the loop: 307.8 / 306.6 / 308.6 / 309.4 -> 301.7 / 301.6 / 303.1 / 304.6 us in
    // four A/B runs on three boxes (-1.7 %; priority 2 the same, 1 half of it; kept through the hit validation as well: 305.9); same instructions, same values
    // (profiles/r06_ab_r4_setprio.txt).  Raised priority from a wave's start until its first loads are out as well: 304.5 / 304.6 us, nothing.  The same idea for the load groups of the straight-line kernels (R6, TAA: raised priority until a wave's loads are out) loses 1 - 3 %.
    __builtin_amdgcn_s_setprio(3);
    while (idx < maxIter && lo >= loMin)
    {
#ifdef MIFX_R4_STATS
        coarse5 += lo >= 6 * kEntry ? 1u : 0u;
        coarse4 += lo >= 5 * kEntry ? 1u : 0u;
#endif
        const v2    mp = mipRes * mk2(pos.x, pos.y);
        const float surfaceDepth = load_hiz<DIRECT0>(hiz, L.addr, int(mp.x), int(mp.y), lo <= kEntry);
        // AdvanceRay :88-137
        v2 plane{floorf(mp.x) + floorOffset.x, floorf(mp.y) + floorOffset.y};
        plane = plane * invMipRes + uvOffset;
        v3 t{plane.x * invDir.x - origin.x * invDir.x, plane.y * invDir.y - origin.y * invDir.y, surfaceDepth * invDir.z - origin.z * invDir.z};
        t.z = away ? t.z : SSR_FLT_MAX;
        const float tmin = fminf(fminf(t.x, t.y), t.z);
        const bool  above = REV ? surfaceDepth < pos.z : surfaceDepth > pos.z;
        const bool  skipped = __float_as_uint(tmin) != __float_as_uint(t.z) && above;
        curT = above ? tmin : curT;
        pos  = origin + curT * dir;

        // CurrentMip += SkippedTile ? 1 : -1 unless that would leave the generated levels (:171-179); CurrentMip never exceeds SSR_MAX_MIP (MostDetailedMip is
        // validated against it), so "stay" is the upper clamp
        lo = min(lo + (skipped ? kEntry : -kEntry), (SSR_MAX_MIP + 1) * kEntry);
        L  = entry(lo);
        mipRes    = v2{L.res.x, L.res.y};
        invMipRes = v2{L.res.z, L.res.w};
        ++idx;
    }
    __builtin_amdgcn_s_setprio(0);
    validHit = true; // ValidHit = (i <= MaxTraversalIntersections) :187 -- the loop cannot leave i above the bound
    steps = idx;
#ifdef MIFX_R4_STATS
    steps = idx + 256u * coarse5 + 65536u * coarse4;
#endif
    return pos;
}
MIFX_D float smoothstepf(float a, float b, float x)
{
    const float t = saturate(fdiv(x - a, b - a));
    return t * t * (3.0f - 2.0f * t);
}
MIFX_D float edge_vignette(v2 hit, v2 screen) // CalculateEdgeVignette :191-196
{
    const v2 fov{0.05f * fdiv(screen.y, screen.x), 0.05f * 1.0f};
    const v2 border{smoothstepf(0.0f, fov.x, hit.x) * (1.0f - smoothstepf(1.0f - fov.x, 1.0f, hit.x)),
                    smoothstepf(0.0f, fov.y, hit.y) * (1.0f - smoothstepf(1.0f - fov.y, 1.0f, hit.y))};
    return border.x * border.y;
}
// hitPrev (PREV only): the hit moved back along its motion vector, SSR_OPTION_PREVIOUS_FRAME :230-231
template <bool PREV, bool REV, bool DIRECT0>
MIFX_D float validate_hit(const HizLds& hiz, const Img& normalTex, v3 hit, v2 hitPrev, v2 uv, v3 rayDirWS, v2 screen, float thickness, const m44& proj) // ValidateHit :199-252
{
    if (hit.x < 0.0f || hit.y < 0.0f || hit.x > 1.0f || hit.y > 1.0f) return 0.0f;
    const v2 manhattan{fabsf(hit.x - uv.x), fabsf(hit.y - uv.y)};
    if (manhattan.x < fdiv(2.0f, screen.x) && manhattan.y < fdiv(2.0f, screen.y)) return 0.0f;
    const int   tx = int(screen.x * hit.x), ty = int(screen.y * hit.y);
    const float surfaceDepth = load_hiz<DIRECT0>(hiz, tx, ty, 0);
    if (is_background(surfaceDepth, REV)) return 0.0f;
    const v3 hitNormal = (tx < 0 || ty < 0 || tx >= normalTex.w || ty >= normalTex.h) ? mk3(0.0f) : xyz(ld<v4>(normalTex, tx, ty));
    if (dot(hitNormal, rayDirWS) > 0.0f) return 0.0f;
    const v3    surfaceVS = screen_xy_depth_to_view_space(v3{hit.x, hit.y, surfaceDepth}, proj);
    const v3    hitVS     = screen_xy_depth_to_view_space(hit, proj);
    const float dist      = length(surfaceVS - hitVS);
    const float vignette  = PREV ? fminf(edge_vignette(hitPrev, screen), edge_vignette(mk2(hit.x, hit.y), screen)) : edge_vignette(mk2(hit.x, hit.y), screen);
    float confidence = 1.0f - smoothstepf(0.0f, thickness, dist * fdiv(1.0f, surfaceVS.z + SSR_FLT_EPS));
    confidence *= confidence;
    return vignette * confidence;
}

// PREV = FEATURE_FLAG_PREVIOUS_FRAME: `radiance` is last frame's colour; the hit is reprojected with the motion vector at the hit (:310-314)
// Scalar registers (the cap of 72): a CU admits min(8, 800 / (16 ceil(sgprs / 16) + 16)) workgroups of 256 threads (MI355X_MICROARCH.md, "Residency"): with the 84 - 88 the
// allocator takes when left alone that is 7, with <= 80 it is 8 -- and the march's time follows the resident waves (6 workgroups per CU: +10 %, 4: +37 %,
// profiles/r05_ab_occupancy_r4_a3.txt).  No waves-per-SIMD hint: the kernel needs ~50 vector registers, eight waves fit as it is.
template <bool PREV, bool REV, bool DIRECT0 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(72))) void ssr_intersection_kernel(Img radiance, Img normalTex, Img roughnessTex, Img noiseXY, HizSlab hizSlab, Img mask, Img motionTex, Img outSpec,
                                                               Img outDirPdf, CamK cam, SsrK k, Img hitCoords, int localBegin, int localEnd)
{
    __shared__ HizLevel hizLv[SSR_MAX_MIP + 2];
    // (round 5: the texel's reflection mask is requested before the level table is staged -- the table's rows come out of the kernel arguments by a vector load and are
    //  followed by a barrier, a round trip the mask's now shares; clamped coordinates for the threads outside the image, which drop the value)
    int x, y;
    const bool  inImage   = tiled_xy(outSpec, x, y);
    const float maskValue = ld<mask_t>(mask, min(x, outSpec.w - 1), min(y, row_end(outSpec) - 1));
    // Clean tiles.  A wave is one 8 x 8 tile of the ray planes and owns one word of hizSlab.tileFlags: 0 = every texel of the tile (inside the plane)
    // holds the cleared values in both targets -- one way only, a set word over a clean tile is allowed.  A texel outside the mask is cleared to 0 every frame by the
    // reference, and a tile that lies outside the mask now nearly always did so the frame before: under kR4ClearTrust a wave with no texel inside the mask whose word
    // is 0 stores nothing (32 B per texel of zeros over zeros).  The word is requested with the mask (one round trip for both), read and written by this wave alone,
    // launches on these planes are ordered on one stream: plain loads and stores.  Whole-plane launches only (api_ssr.cpp: the tile grid starts at the window's first row).
    const unsigned clearMode   = hizSlab.clearMode;
    const bool     tileInImage = (x & ~7) < outSpec.w; // wave-uniform; the grid's rows always reach into the window
    const unsigned tile        = blockIdx.y * unsigned((outSpec.w + 7) >> 3) + unsigned(x >> 3);
    unsigned       tileFlag    = 1u;
    if (clearMode == kR4ClearTrust && tileInImage) tileFlag = *(const MIFX_GLOBAL unsigned*)(hizSlab.tileFlags + tile);
    if (threadIdx.x < unsigned(SSR_MAX_MIP + 2))
    {
        const unsigned m = threadIdx.x == 0u ? 0u : threadIdx.x - 1u; // entry 0 = a second copy of level 0
        const float s = fdiv(1.0f, float(1 << int(m)));
        const v2    r{cam.vw * s, cam.vh * s};
        hizLv[threadIdx.x] = HizLevel{uint4{hizSlab.offset[m], hizSlab.pitch[m], hizSlab.w[m], hizSlab.h[m]}, v4{r.x, r.y, fdiv(1.0f, r.x), fdiv(1.0f, r.y)}};
    }
    __syncthreads();
    const HizLds hiz{__builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(hizSlab.base), 0, int(hizSlab.bytes), 0x00020000), hizLv,
                     __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(DIRECT0 ? hizSlab.base0 : hizSlab.base), 0, int(DIRECT0 ? hizSlab.bytes0 : hizSlab.bytes), 0x00020000)};
    bool skipClear = false;
    if (clearMode != kR4ClearAlways)
    {
        const bool any   = __ballot(inImage && maskValue != 0.0f) != 0ull; // (the threads outside the image take no part: an edge tile is the tile within the image)
        const bool dirty = __builtin_amdgcn_readfirstlane(int(tileFlag)) != 0;
        skipClear        = clearMode == kR4ClearTrust && !any && !dirty;
        // rebuild: the exact word, whatever was there; trust: the word only where it changes (0 -> 1 before this wave's rays are stored, 1 -> 0 with the zeros below)
        if (tileInImage && (clearMode == kR4ClearRebuild || any != dirty) && (threadIdx.x & 63u) == 0u) *(MIFX_GLOBAL unsigned*)(hizSlab.tileFlags + tile) = any ? 1u : 0u;
    }
    if (!inImage) return;
    if (maskValue == 0.0f)
    {
        if (!skipClear)
        {
            st<v4>(outSpec, x, y, mk4(0.0f)); // both targets are cleared to 0 (ScreenSpaceReflection.cpp:993-994)
            st<v4>(outDirPdf, x, y, mk4(0.0f));
        }
        if (hitCoords.p != nullptr) st<float>(hitCoords, x, y, __uint_as_float(0xffffffffu));
        return;
    }
    const v2 screen{cam.vw, cam.vh};
    // the full-resolution pixel whose ray this texel traces: itself, or (half resolution, :283-288) one pixel of its 2x2 block chosen by
    // ComputeHalfResolutionOffset (PostFX_Common.fxh:45-55); targets, mask and noise stay indexed by the texel (x, y)
    int px = x, py = y;
    if (k.HalfResolution)
    {
        const unsigned sampleIdx = (1320229860u >> (((unsigned(x) & 3u) << 3u) + ((unsigned(y) & 3u) << 1u))) & 3u;
        px = 2 * x + int(sampleIdx & 1u);
        py = 2 * y + int(sampleIdx >> 1u);
    }
    const v2 uv{(float(px) + 0.5f) * cam.ivw, (float(py) + 0.5f) * cam.ivh};
    const v3 normalVS  = mul_dir(xyz(ld<v4>(normalTex, px, py)), cam.view);
    const float rough  = ld<rough_t>(roughnessTex, px, py);
    const bool mirror  = rough < 0.01f; // IsMirrorReflection
    const int  mdm     = mirror ? 0 : int(k.MostDetailedMip);
    const v2   mipRes  = screen * fdiv(1.0f, float(1 << mdm));
    const v3   originSS{uv.x, uv.y, load_hiz<DIRECT0>(hiz, int(uv.x * mipRes.x), int(uv.y * mipRes.y), mdm)};
    const v3   originVS = screen_xy_depth_to_view_space(originSS, cam.proj);

    // SampleReflectionVector :254-278 (GGX VNDF, spherical caps)
    const v3 view = -normalize(originVS);
    v3 dirVS;
    float pdf;
    {
        const float alpha = rough * rough;
        const v3 N = normalVS;
        const v3 T = normalize(cross(N, fabsf(N.y) > 0.5f ? v3{1.0f, 0.0f, 0.0f} : v3{0.0f, 1.0f, 0.0f}));
        const v3 B = cross(T, N);
        v2 xi = ld<v2>(noiseXY, x & 127, y & 127);
        xi.y  = lerpf(xi.y, 0.0f, k.GGXImportanceSampleBias);
        const v3 viewTS{dot(T, view), dot(B, view), dot(N, view)};
        const v3 micro  = smith_ggx_sample_visible_normal_sc(viewTS, alpha, alpha, xi.x, xi.y);
        const v3 sampTS = reflect(-viewTS, micro);
        const float NdotV = viewTS.z, NdotH = micro.z;
        const float D  = normal_distribution_ggx(NdotH, alpha);
        const float G1 = smith_ggx_masking(NdotV, alpha);
        pdf   = fdiv(G1 * D, 4.0f * NdotV + SSR_FLT_EPS);
        dirVS = sampTS.x * T + sampTS.y * B + sampTS.z * N;
    }
    const v3 dirSS = project_position(originVS + dirVS, cam.proj) - originSS; // ProjectDirection
    const v3 dirWS = mul_dir(dirVS, cam.viewInv);

    bool validHit = false;
    unsigned steps = 0u;
    const v3 hitSS = hierarchical_raymarch<REV, DIRECT0>(hiz, originSS, dirSS, screen, mdm, k.MaxTraversalIntersections, validHit, steps);
#ifdef MIFX_R4_STATS // tools/r4_stats.py: the number of march steps of every ray in place of the pdf
    pdf = float(steps);
#endif
    const v3 hitVS = screen_xy_depth_to_view_space(hitSS, cam.proj);
    v2 hitPrev{hitSS.x, hitSS.y};
    if (PREV && validHit)
    {
        const v2 m = ld_zero_v2(motionTex, int(screen.x * hitSS.x), int(screen.y * hitSS.y)); // LoadMotion :56-59
        hitPrev = v2{hitSS.x - m.x * 0.5f, hitSS.y - m.y * -0.5f};
    }
    const float confidence = validHit ? validate_hit<PREV, REV, DIRECT0>(hiz, normalTex, hitSS, hitPrev, uv, dirWS, screen, k.DepthBufferThickness, cam.proj) : 0.0f;
    v3 refl = mk3(0.0f);
    // Row-band sharding (hitCoords.p != null, uniform): the colour at the hit may lie in a row this rank did not shade.  For such a hit the march only records WHERE it
    // is (0xffffffff: nothing to fetch) and pbr_hit_fetch_kernel (pbr.hip) shades that pixel on the spot; a hit in the rows [localBegin, localEnd) this rank shaded itself
    // is loaded here as in the unsharded frame (round 5: until then the fetch pass loaded those too -- 52 B per ray texel through a second kernel, 71 us per band at 8K).
    unsigned where = 0xffffffffu;
    if (confidence > 0.0f)
    {
        const int  rx = int(screen.x * hitPrev.x), ry = int(screen.y * hitPrev.y);
        const bool in = rx >= 0 && ry >= 0 && rx < radiance.w && ry < radiance.h;
        if (hitCoords.p != nullptr && (ry < localBegin || ry >= localEnd)) where = in ? unsigned(rx) | (unsigned(ry) << 16) : 0xffffffffu;
        else if (in) refl = xyz(ld<v4>(radiance, rx, ry));
    }
    if (hitCoords.p != nullptr) st<float>(hitCoords, x, y, __uint_as_float(where));
    st<v4>(outSpec, x, y, mk4(refl, confidence));
    st<v4>(outDirPdf, x, y, mk4(dirWS * length(hitVS - originVS), pdf));
}


// (Round 5, measured and not taken: two rays per lane -- a wave on 16 x 8 pixels, both taps of a step issued before either is used, the tails parked in LDS -- 320.5 us
//  against 310.1 us, bit-identical output.  A step is as long as its slowest lane's tap, and 128 rays per wave have a slower slowest lane than 64: the march is bound by the
//  rate at which the L1 hands out the taps of rays that share no cache line, not by how many are waiting.  profiles/r05_ab_r4_two_rays.txt.)

static const dim3 kBlock(64, 4, 1);
#define MIFX_LAUNCH_END()              \
    MIFX_HIP_CHECK(hipGetLastError()); \
    return MIFX_OK

mifx_status launch_ssr_intersection(hipStream_t s, Img radiance, Img normal, Img roughness, Img noiseXY, const HizSlab& hiz, Img mask, Img motion, Img outSpec, Img outDirPdf,
                                    const CamK& cam, const mifx_ssr_attribs& a, bool previousFrame, bool halfResolution, Img hitCoords, int localBegin, int localEnd)
{
    const bool rev = cam.reversedDepth != 0;
    const SsrK k   = make_k(a, rev, halfResolution);
    constexpr int kR4Block = 256; // (measured late in round 2: one or two 8x8 tiles per workgroup, 64 / 128 threads, are 2-4 % slower)
    const dim3 r4grid((outSpec.w + kR4Block / 8 - 1) / (kR4Block / 8), (window_rows(outSpec) + 7) / 8, 1);
#define MIFX_R4_LAUNCH(P, R)                                                                                                                                                       \
    do {                                                                                                                                                                           \
        if (hiz.base0 != nullptr) hipLaunchKernelGGL((ssr_intersection_kernel<P, R, true>), r4grid, dim3(kR4Block, 1, 1), 0, s, radiance, normal, roughness, noiseXY, hiz, mask, motion, outSpec, outDirPdf, cam, k, hitCoords, localBegin, localEnd); \
        else hipLaunchKernelGGL((ssr_intersection_kernel<P, R>), r4grid, dim3(kR4Block, 1, 1), 0, s, radiance, normal, roughness, noiseXY, hiz, mask, motion, outSpec, outDirPdf, cam, k, hitCoords, localBegin, localEnd); \
    } while (0)
    if (previousFrame) { if (rev) MIFX_R4_LAUNCH(true, true); else MIFX_R4_LAUNCH(true, false); }
    else { if (rev) MIFX_R4_LAUNCH(false, true); else MIFX_R4_LAUNCH(false, false); }
#undef MIFX_R4_LAUNCH
    MIFX_LAUNCH_END();
}
} // namespace mifx
