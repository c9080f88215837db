// mifx_coordinate_grid.h -- the world-space coordinate grid and the X / Y / Z axes, per pixel: the body of coordinate_grid_kernel and copy_frame_grid_kernel (grid.hip), in a
// header so that the test suite can also compile it for the host (tests/host_kernels/grid_host.cpp).  Follows Shaders/Common/public/CoordinateGrid.fxh:
// CreateCameraRay :13, ComputeRayPlaneIntersection :31, ComputeGrid :48, ComputeAxis :73, ComputePlaneIntersectionAttribs :134, ComputeCoordinateGrid :158.
//
// Arithmetic.  ComputeGrid takes fwidth() of the plane coordinate: neighbouring coordinates are subtracted, so their fp32 rounding is amplified by the pixel footprint
// (at 4K footprints two evaluations that differ only in rounding are up to 5e-2 apart in alpha).  Everything here is therefore strict fp32 in the reference's operation
// order: no contraction (`#pragma clang fp contract(off)` in every body, which is lexical -- the bodies call no helper with a multiply-add), IEEE division and square
// root (plain `/` and sqrtf: the compiler's correctly rounded expansions, not fdiv / fsqrt, whose rare 1-ulp cases would show in a device-against-host comparison),
// libm log10f (it feeds floor), libm fmodf (exact), libm expf.  The host compilation of this header and the device kernels agree bit for bit on the coordinate, its
// fwidth, the plane alpha and the axis distances; log10f / expf are each platform's libm.
//
// fwidth(Coord) = |ddx| + |ddy| with the project's quad convention (mifx_ssr_cleanup.h, the checker's hl_deriv): fine derivatives inside the 2x2 quad whose origin is
// (x & ~1, y & ~1); ddx = right - left of this pixel's row, ddy = bottom - top of this pixel's column.  Coord is analytic (a function of the pixel's NDC only), so every
// thread evaluates the plane hit of its two quad partners (x ^ 1, y) and (x, y ^ 1) itself -- same arithmetic, same bits as the partner's own evaluation -- and a partner
// is evaluated at its OWN PIXEL CENTRE EVEN WHEN THAT LIES OUTSIDE THE FRAME (what a rasteriser's helper lane does; only the last column / row of an odd-sized frame is
// affected).
//
// pow(Subdivision, floor(LodLevel)) has a non-negative integer exponent and is evaluated as a multiply loop over it (grid_ipow), not m_pow: a relative error e of Lod
// becomes a phase error of about Coord * e in fmod(|Coord - Lod / 2|, Lod), which is divided by a line width of one pixel footprint.  Every product of the loop that is
// exactly representable is exact, hence equal to a correctly rounded powf: for Subdivision 10 (the default) that is every k <= 10 (the LOD of a grid of 1e-4 cells seen
// through pixel footprints of 1e-4 .. 1e+5 units).  Measured against pow rounded once from float64 over Subdivision 2 .. 10 and k = 0 .. 12: 0 ulp for 2, 3, 4, 5, 6, 8
// and 10, 1 ulp for 7 and 9 (tests/test_grid_cpu.py holds these figures).  The exponent is clamped to 128 (any Subdivision >= 2 has overflowed to infinity by then, as
// pow has).
//
// normalize(ViewRay.Origin) in ComputeAxis (:124) is 0 * (1 / 0) = NaN for a ray that starts at the world origin.  IEEE is followed, no guard is added: with a
// perspective camera at the origin Delta = 0, so DistFromCamera = 0 fails `> 0` before that line is reached and the axes are not drawn; an orthographic ray that starts
// exactly at the origin reaches it with NaN, saturate(NaN) = 0 (fmin(fmax(NaN, 0), 1)) and the axis alpha of that pixel is 0.
#pragma once
#include <cmath>
#include "mifx.h"
#include "mifx_device.h"

namespace mifx
{
// the members of CameraAttribs that ComputeCoordinateGrid reads, passed by value
struct GridCamK
{
    float vpi[16];  // mViewProjInv
    float viewZ[4]; // column 2 of mView: mul(float4(p, 1), mView).z
    float p00, p11, p22, p23, p32, p33; // mProj[0][0], [1][1], [2][2], [2][3], [3][2], [3][3]
    float pos[3];   // f4Position.xyz
    float nearDepth, farDepth, farZ; // fNearPlaneDepth, fFarPlaneDepth, fFarPlaneZ
    float ivw, ivh; // f4ViewportSize.zw
    float jx, jy;   // f2Jitter
};
inline GridCamK make_gridcamk(const mifx_camera_attribs& c)
{
    GridCamK k;
    for (int i = 0; i < 16; ++i) k.vpi[i] = c.mViewProjInv[i];
    for (int i = 0; i < 4; ++i) k.viewZ[i] = c.mView[4 * i + 2];
    k.p00 = c.mProj[0]; k.p11 = c.mProj[5]; k.p22 = c.mProj[10]; k.p23 = c.mProj[11]; k.p32 = c.mProj[14]; k.p33 = c.mProj[15];
    k.pos[0] = c.f4Position[0]; k.pos[1] = c.f4Position[1]; k.pos[2] = c.f4Position[2];
    k.nearDepth = c.fNearPlaneDepth; k.farDepth = c.fFarPlaneDepth; k.farZ = c.fFarPlaneZ;
    k.ivw = c.f4ViewportSize[2]; k.ivh = c.f4ViewportSize[3];
    k.jx = c.f2Jitter[0]; k.jy = c.f2Jitter[1];
    return k;
}

constexpr uint32_t kGridPlaneFlags = MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_YZ | MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XZ | MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XY;
constexpr uint32_t kGridAxisFlags  = MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_X | MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Y | MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Z;

struct GridRay
{
    v3 o, d;
};

// f2NormalizedXY of the full-screen triangle at the centre of pixel (x, y) of a W x H frame, plus f2Jitter (CoordinateGridPS.psh:28, HnCopyFrame.psh:53); x / y may lie
// outside the frame (a quad partner of the last column / row)
MIFX_D v2 grid_ndc(int x, int y, int W, int H, const GridCamK& c)
{
#pragma clang fp contract(off)
    const float u = (float(x) + 0.5f) / float(W), v = (float(y) + 0.5f) / float(H);
    return v2{(2.0f * u - 1.0f) + c.jx, (1.0f - 2.0f * v) + c.jy};
}

// mul(float4(ndc, z, 1), mViewProjInv), xyz / w
MIFX_D v3 grid_unproject(v2 ndc, float z, const float* M)
{
#pragma clang fp contract(off)
    const float x = ndc.x * M[0] + ndc.y * M[4] + z * M[8] + M[12];
    const float y = ndc.x * M[1] + ndc.y * M[5] + z * M[9] + M[13];
    const float s = ndc.x * M[2] + ndc.y * M[6] + z * M[10] + M[14];
    const float w = ndc.x * M[3] + ndc.y * M[7] + z * M[11] + M[15];
    return v3{x / w, y / w, s / w};
}

// CreateCameraRay (:13-29); DepthToNormalizedDeviceZ is the identity (NDC_MIN_Z = 0)
MIFX_D GridRay grid_camera_ray(v2 ndc, const GridCamK& c)
{
#pragma clang fp contract(off)
    const v3 s = grid_unproject(ndc, c.nearDepth, c.vpi), e = grid_unproject(ndc, c.farDepth, c.vpi);
    const v3 d{e.x - s.x, e.y - s.y, e.z - s.z};
    const float inv = 1.0f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z); // normalize(v) = v * (1 / sqrt(dot(v, v)))
    GridRay r;
    r.d = v3{d.x * inv, d.y * inv, d.z * inv};
    r.o = c.p33 == 0.0f ? v3{c.pos[0], c.pos[1], c.pos[2]} : s;
    return r;
}

template <int AXIS> MIFX_D float grid_comp(v3 a) { return AXIS == 0 ? a.x : AXIS == 1 ? a.y : a.z; }
// the two coordinates of a point in the plane whose normal is the axis AXIS: Positions[0].yz, Positions[1].xz, Positions[2].xy (:206-218)
template <int AXIS> MIFX_D v2 grid_plane_coords(v3 p) { return AXIS == 0 ? v2{p.y, p.z} : AXIS == 1 ? v2{p.x, p.z} : v2{p.x, p.y}; }

// ComputeRayPlaneIntersection (:31-36) for the plane through the origin whose normal is the unit axis AXIS.  The two dot products with (1, 0, 0) and its like are one
// component plus two signed zeros: exactly that component for finite rays (and a zero of either sign takes the same branches below).
template <int AXIS> MIFX_D float grid_plane_distance(const GridRay& r)
{
#pragma clang fp contract(off)
    float nd = grid_comp<AXIS>(r.d);
    nd = fmaxf(fabsf(nd), 1e-6f) * (nd > 0.0f ? 1.0f : -1.0f);
    return (0.0f - grid_comp<AXIS>(r.o)) / nd;
}
template <int AXIS> MIFX_D v3 grid_plane_hit(const GridRay& r, float dist)
{
#pragma clang fp contract(off)
    return v3{r.o.x + r.d.x * dist, r.o.y + r.d.y * dist, r.o.z + r.d.z * dist};
}

// pow(s, e) for e = floor(x) >= 0: the product of e factors, from the left (see the head of the file)
MIFX_D float grid_ipow(float s, float e)
{
#pragma clang fp contract(off)
    const int n = int(fminf(e, 128.0f));
    float p = 1.0f;
    for (int k = 0; k < n; ++k) p = p * s;
    return p;
}

// one LodAlpha of ComputeGrid (:67)
MIFX_D float grid_lod_alpha(v2 c, float lod, v2 lineWidth)
{
#pragma clang fp contract(off)
    const float h = 0.5f * lod;
    const float ax = 1.0f - saturate(fabsf((fmodf(fabsf(c.x - h), lod) - h) / lineWidth.x));
    const float ay = 1.0f - saturate(fabsf((fmodf(fabsf(c.y - h), lod) - h) / lineWidth.y));
    return fmaxf(ax, ay);
}

// fwidth(Coord) from the pixel's coordinate and those of its horizontal and vertical quad partners (right / bottom: the pixel is the right / bottom one of its pair)
MIFX_D v2 grid_fwidth(v2 c, v2 cH, v2 cV, bool right, bool bottom)
{
#pragma clang fp contract(off)
    const v2 ddx = right ? v2{c.x - cH.x, c.y - cH.y} : v2{cH.x - c.x, cH.y - c.y};
    const v2 ddy = bottom ? v2{c.x - cV.x, c.y - cV.y} : v2{cV.x - c.x, cV.y - c.y};
    return v2{fabsf(ddx.x) + fabsf(ddy.x), fabsf(ddx.y) + fabsf(ddy.y)};
}

// ComputeGrid (:48-71) with Coord and fwidth(Coord) given
MIFX_D v4 grid_lines(v2 c, v2 mag, float subdivision, const mifx_coordinate_grid_attribs& a)
{
#pragma clang fp contract(off)
    const v2    lineWidth{0.5f * mag.x * a.GridLineWidth, 0.5f * mag.y * a.GridLineWidth};
    const float lodLevel = fmaxf(0.0f, log10f(sqrtf(mag.x * mag.x + mag.y * mag.y) * a.GridMinCellWidth / a.GridMinCellSize) + 1.0f);
    const float lodFloor = floorf(lodLevel);
    const float lodFade  = lodLevel - lodFloor;
    const float lod0 = a.GridMinCellSize * grid_ipow(subdivision, lodFloor);
    const float lod1 = lod0 * subdivision;
    const float lod2 = lod1 * subdivision;
    const float a0 = grid_lod_alpha(c, lod0, lineWidth), a1 = grid_lod_alpha(c, lod1, lineWidth), a2 = grid_lod_alpha(c, lod2, lineWidth);
    const float* thick = a.GridMajorColor;
    const float* thin  = a.GridMinorColor;
    if (a2 > 0.0f) return v4{thick[0], thick[1], thick[2], a2};
    if (a1 > 0.0f) return v4{thick[0] + lodFade * (thin[0] - thick[0]), thick[1] + lodFade * (thin[1] - thick[1]), thick[2] + lodFade * (thin[2] - thick[2]), a1};
    return v4{thin[0], thin[1], thin[2], a0 * (1.0f - lodFade)};
}

// What the frame-constant part of ComputeCoordinateGrid (:169-174) gives a pixel
struct GridDepthRange
{
    float pixelSize, maxCameraZ, cameraZRange;
};
MIFX_D GridDepthRange grid_depth_range(const GridCamK& c, float minDepth, float maxDepth)
{
#pragma clang fp contract(off)
    GridDepthRange r;
    const float sx = c.ivw / c.p00, sy = c.ivh / c.p11;
    r.pixelSize = sqrtf(sx * sx + sy * sy);
    const float z0 = (c.p32 - minDepth * c.p33) / (minDepth * c.p23 - c.p22); // DepthToCameraZ (ShaderUtilities.fxh:24-39)
    const float z1 = (c.p32 - maxDepth * c.p33) / (maxDepth * c.p23 - c.p22);
    const float minZ = fminf(z0, z1);
    r.maxCameraZ   = fmaxf(z0, z1);
    r.cameraZRange = fmaxf(r.maxCameraZ - minZ, 1e-6f);
    return r;
}

// ComputePlaneIntersectionAttribs (:134-156): PlaneAlpha of the hit at distance `dist`, position `pos`
MIFX_D float grid_plane_alpha(float dist, v3 pos, const GridCamK& cam, const GridDepthRange& z)
{
#pragma clang fp contract(off)
    float alpha = dist > 0.0f ? 1.0f : 0.0f;
    const float cameraZ = pos.x * cam.viewZ[0] + pos.y * cam.viewZ[1] + pos.z * cam.viewZ[2] + cam.viewZ[3];
    alpha = alpha * saturate((z.maxCameraZ - cameraZ) / z.cameraZRange + 0.1f);
    alpha = alpha * saturate(1.0f - cameraZ / cam.farZ);
    return alpha;
}

// ComputePlaneIntersectionAttribs + ComputeGrid * PlaneAlpha (:206-218) of one plane.  debug: (Coord.xy, fwidth(Coord).xy) instead.
template <int AXIS>
MIFX_D v4 grid_plane(const GridRay& r, const GridRay& rH, const GridRay& rV, bool right, bool bottom, const GridCamK& cam, const GridDepthRange& z, float scale, float subdivision,
                     const mifx_coordinate_grid_attribs& a, bool debug)
{
#pragma clang fp contract(off)
    const float dist = grid_plane_distance<AXIS>(r);
    const v3    pos  = grid_plane_hit<AXIS>(r, dist);
    const float alpha = grid_plane_alpha(dist, pos, cam, z);
    const v2 p = grid_plane_coords<AXIS>(pos);
    const v2 pH = grid_plane_coords<AXIS>(grid_plane_hit<AXIS>(rH, grid_plane_distance<AXIS>(rH)));
    const v2 pV = grid_plane_coords<AXIS>(grid_plane_hit<AXIS>(rV, grid_plane_distance<AXIS>(rV)));
    const v2 c{p.x * scale, p.y * scale}, cH{pH.x * scale, pH.y * scale}, cV{pV.x * scale, pV.y * scale};
    const v2 mag = grid_fwidth(c, cH, cV, right, bottom);
    if (debug) return v4{c.x, c.y, mag.x, mag.y};
    const v4 g = grid_lines(c, mag, subdivision, a);
    return v4{g.x * alpha, g.y * alpha, g.z * alpha, g.w * alpha};
}

// The distances of ComputeAxis (:86-103) for the unit axis AXIS through the origin.  All four are evaluated before the two tests of :91 / :95 (a quotient by a Denom that
// fails the first test is an unused infinity or NaN).
struct GridAxisTerms
{
    float denom, distFromCamera, distFromOrigin, distToAxis;
};
template <int AXIS> MIFX_D GridAxisTerms grid_axis_terms(const GridRay& r)
{
#pragma clang fp contract(off)
    const v3 A{AXIS == 0 ? 1.0f : 0.0f, AXIS == 1 ? 1.0f : 0.0f, AXIS == 2 ? 1.0f : 0.0f};
    const v3 D = r.d;
    const v3 cr{A.y * D.z - A.z * D.y, A.z * D.x - A.x * D.z, A.x * D.y - A.y * D.x}; // cross(AxisDirection, ViewRay.Direction)
    const v3 delta = r.o;                                                              // ViewRay.Origin - AxisOrigin
    GridAxisTerms t;
    t.denom = cr.x * cr.x + cr.y * cr.y + cr.z * cr.z;
    const v3 dxa{delta.y * A.z - delta.z * A.y, delta.z * A.x - delta.x * A.z, delta.x * A.y - delta.y * A.x}; // cross(Delta, AxisDirection)
    t.distFromCamera = (dxa.x * cr.x + dxa.y * cr.y + dxa.z * cr.z) / t.denom;
    const v3 dxd{delta.y * D.z - delta.z * D.y, delta.z * D.x - delta.x * D.z, delta.x * D.y - delta.y * D.x}; // cross(Delta, ViewRay.Direction)
    t.distFromOrigin = (dxd.x * cr.x + dxd.y * cr.y + dxd.z * cr.z) / t.denom;
    t.distToAxis     = fabsf(delta.x * cr.x + delta.y * cr.y + delta.z * cr.z) / fmaxf(sqrtf(t.denom), 0.001f);
    return t;
}

// ComputeAxis (:73-132)
template <int AXIS>
MIFX_D v4 grid_axis(const GridRay& r, float axisLen, float pixelSize, const GridDepthRange& z, const GridCamK& cam, const float* positive, const float* negative)
{
#pragma clang fp contract(off)
    const v3 A{AXIS == 0 ? 1.0f : 0.0f, AXIS == 1 ? 1.0f : 0.0f, AXIS == 2 ? 1.0f : 0.0f};
    const GridAxisTerms t = grid_axis_terms<AXIS>(r);
    if (!(fabsf(t.denom) > 1e-7f)) return v4{0.0f, 0.0f, 0.0f, 0.0f};
    if (!(t.distFromCamera > 0.0f)) return v4{0.0f, 0.0f, 0.0f, 0.0f};
    const v3 axisPos{0.0f + A.x * t.distFromOrigin, 0.0f + A.y * t.distFromOrigin, 0.0f + A.z * t.distFromOrigin};
    float axisWidth = pixelSize;
    if (cam.p33 == 0.0f) axisWidth = axisWidth * t.distFromCamera;
    const float line = fabsf(t.distToAxis) / axisWidth;
    float alpha = (1.0f - fminf(line * line, 1.0f)) * saturate(1.0f - t.distFromCamera / axisLen);
    float axisPosZ = axisPos.x * cam.viewZ[0] + axisPos.y * cam.viewZ[1] + axisPos.z * cam.viewZ[2] + cam.viewZ[3];
    axisPosZ = axisPosZ + axisWidth;
    alpha = alpha * saturate((z.maxCameraZ - axisPosZ) / z.cameraZRange);
    // fade out when looking straight along the axis: normalize(ViewRay.Origin) -- 0 * inf = NaN for an origin of zero, see the head of the file
    const float invLen = 1.0f / sqrtf(r.o.x * r.o.x + r.o.y * r.o.y + r.o.z * r.o.z);
    const v3    n{r.o.x * invLen, r.o.y * invLen, r.o.z * invLen};
    alpha = alpha * saturate((1.0f - fabsf(n.x * A.x + n.y * A.y + n.z * A.z)) * 1e+6f);
    // (the components are selected by value: a per-lane choice between two pointers into the kernel arguments would become vector loads from the kernarg segment)
    const bool pos = t.distFromOrigin > 0.0f;
    const v3   col{pos ? positive[0] : negative[0], pos ? positive[1] : negative[1], pos ? positive[2] : negative[2]};
    return v4{col.x * alpha, col.y * alpha, col.z * alpha, alpha};
}

// ComputeCoordinateGrid (:158-227) for the pixel whose NDC (jitter included) is `ndc`; ndcH / ndcV: the NDC of its quad partners (x ^ 1, y) and (x, y ^ 1), right / bottom:
// x & 1, y & 1.  `flags`: MIFX_COORDINATE_GRID_FEATURE_FLAG_* -- the reference's COORDINATE_GRID_* macros as wave-uniform branches.  With
// MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD the result is (Coord.xy, fwidth(Coord).xy) of the first plane whose flag is set.
MIFX_D v4 coordinate_grid(v2 ndc, v2 ndcH, v2 ndcV, bool right, bool bottom, const GridCamK& cam, float minDepth, float maxDepth, const mifx_coordinate_grid_attribs& a, uint32_t flags)
{
#pragma clang fp contract(off)
    const GridRay        r = grid_camera_ray(ndc, cam);
    const GridDepthRange z = grid_depth_range(cam, minDepth, maxDepth);
    v4 grid{0.0f, 0.0f, 0.0f, 0.0f}, axis{0.0f, 0.0f, 0.0f, 0.0f};
    if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_X)
        axis = axis + grid_axis<0>(r, cam.farZ, z.pixelSize * a.XAxisWidth, z, cam, a.PositiveXAxisColor, a.NegativeXAxisColor);
    if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Y)
        axis = axis + grid_axis<1>(r, cam.farZ, z.pixelSize * a.YAxisWidth, z, cam, a.PositiveYAxisColor, a.NegativeYAxisColor);
    if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_AXIS_Z)
        axis = axis + grid_axis<2>(r, cam.farZ, z.pixelSize * a.ZAxisWidth, z, cam, a.PositiveZAxisColor, a.NegativeZAxisColor);
    if (flags & kGridPlaneFlags)
    {
        const bool    debug = (flags & MIFX_COORDINATE_GRID_DEBUG_FLAG_COORD) != 0;
        const GridRay rH = grid_camera_ray(ndcH, cam), rV = grid_camera_ray(ndcV, cam);
        if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_YZ)
        {
            const v4 g = grid_plane<0>(r, rH, rV, right, bottom, cam, z, a.GridScale[0], a.GridSubdivision[0], a, debug);
            if (debug) return g;
            grid = grid + g;
        }
        if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XZ)
        {
            const v4 g = grid_plane<1>(r, rH, rV, right, bottom, cam, z, a.GridScale[1], a.GridSubdivision[1], a, debug);
            if (debug) return g;
            grid = grid + g;
        }
        if (flags & MIFX_COORDINATE_GRID_FEATURE_FLAG_RENDER_PLANE_XY)
        {
            const v4 g = grid_plane<2>(r, rH, rV, right, bottom, cam, z, a.GridScale[2], a.GridSubdivision[2], a, debug);
            if (debug) return g;
            grid = grid + g;
        }
    }
    // (exp(-0) = 1 exactly when no axis is drawn)
    const float fade = (flags & kGridAxisFlags) ? expf(-10.0f * axis.w * axis.w) : 1.0f;
    return v4{grid.x * fade + axis.x, grid.y * fade + axis.y, grid.z * fade + axis.z, grid.w * (1.0f - axis.w) + axis.w};
}

// the same for the pixel (x, y) of a W x H frame
MIFX_D v4 coordinate_grid_at(int x, int y, int W, int H, const GridCamK& cam, float minDepth, float maxDepth, const mifx_coordinate_grid_attribs& a, uint32_t flags)
{
    return coordinate_grid(grid_ndc(x, y, W, H, cam), grid_ndc(x ^ 1, y, W, H, cam), grid_ndc(x, y ^ 1, W, H, cam), (x & 1) != 0, (y & 1) != 0, cam, minDepth, maxDepth, a, flags);
}

// the fixed-function blend of the stand-alone renderer (BS_AlphaBlend on rgb; the target's alpha is left as it is -- DESIGN.md section 2) and the in-shader lerp of
// HnCopyFrame.psh:57
MIFX_D v3 grid_blend(v3 dst, v4 g)
{
#pragma clang fp contract(off)
    const float k = 1.0f - g.w;
    return v3{g.x * g.w + dst.x * k, g.y * g.w + dst.y * k, g.z * g.w + dst.z * k};
}
MIFX_D v3 grid_lerp(v3 c, v4 g)
{
#pragma clang fp contract(off)
    return v3{c.x + g.w * (g.x - c.x), c.y + g.w * (g.y - c.y), c.z + g.w * (g.z - c.z)};
}
} // namespace mifx
