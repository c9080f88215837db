"""TEST INFRASTRUCTURE ONLY.  A float32 numpy restatement of the coordinate grid and axes (Shaders/Common/public/CoordinateGrid.fxh: CreateCameraRay :13,
ComputeRayPlaneIntersection :31, ComputeGrid :48, ComputeAxis :73, ComputePlaneIntersectionAttribs :134, ComputeCoordinateGrid :158), of the stand-alone renderer's pixel
shader (CoordinateGridPS.psh:24-38) and of the grid part of the copy-frame pass (HnCopyFrame.psh:38-58), written from the shader text one operation per numpy operation.

Every operation is a float32 numpy operation in the shader's order (numpy rounds each one: no contraction), so the values that involve no transcendental -- Coord,
fwidth(Coord), PlaneAlpha, the axis distances -- can be held bit for bit against the product's header compiled for the host.  fwidth follows the project's quad
convention: fine derivatives in the 2x2 quad at (x & ~1, y & ~1), a partner outside the frame evaluated at its own pixel centre.

Cameras and attribs are flat float32 arrays in the byte layout of CameraAttribs (144 floats) and CoordinateGridAttribs (48 floats)."""
import numpy as np

F = np.float32

FLAG_SRGB, FLAG_YZ, FLAG_XZ, FLAG_XY, FLAG_AXIS_X, FLAG_AXIS_Y, FLAG_AXIS_Z = 1, 2, 4, 8, 16, 32, 64
FLAG_DEBUG_COORD = 256
PLANES = FLAG_YZ | FLAG_XZ | FLAG_XY
AXES = FLAG_AXIS_X | FLAG_AXIS_Y | FLAG_AXIS_Z
ALL = PLANES | AXES

# float offsets into CameraAttribs (BasicStructures.fxh:84-149)
CAM_POS, CAM_VIEWPORT, CAM_NEAR_Z, CAM_FAR_Z, CAM_NEAR_DEPTH, CAM_FAR_DEPTH, CAM_JITTER = 0, 4, 8, 9, 10, 11, 26
CAM_VIEW, CAM_PROJ, CAM_VIEWPROJ, CAM_VIEW_INV, CAM_PROJ_INV, CAM_VIEWPROJ_INV = 28, 44, 60, 76, 92, 108
# float offsets into CoordinateGridAttribs (CoordinateGridStructures.fxh:6-29)
A_POS_X, A_POS_Y, A_POS_Z, A_NEG_X, A_NEG_Y, A_NEG_Z, A_WIDTHS, A_MAJOR, A_MINOR, A_SCALE, A_SUBDIV, A_LINE_WIDTH, A_MIN_CELL_WIDTH, A_MIN_CELL_SIZE = \
    0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 45, 46


def default_attribs():
    a = np.zeros(48, F)
    a[0:24] = [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0.40, 0.15, 0.15, 1, 0.15, 0.40, 0.15, 1, 0.15, 0.15, 0.40, 1]
    a[24:28] = [3, 3, 3, 0]
    a[28:44] = [0.4, 0.4, 0.4, 1, 0.1, 0.1, 0.1, 1, 1, 1, 1, 0, 10, 10, 10, 0]
    a[44:48] = [2, 4, 0.0001, 0]
    return a


def make_camera(W, H, eye, at, fov_deg=60.0, near=0.1, far=100.0, ortho_height=None, reversed_depth=False, jitter=(0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """A CameraAttribs block (row-vector matrices, D3D depth range) computed in float64 and rounded once."""
    eye, at, up = (np.array(v, np.float64) for v in (eye, at, up))
    z = at - eye
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    V = np.eye(4)
    V[:3, 0], V[:3, 1], V[:3, 2] = x, y, z
    V[3, :3] = [-x @ eye, -y @ eye, -z @ eye]
    P = np.zeros((4, 4))
    n, f = (far, near) if reversed_depth else (near, far)  # (reversed depth: the near plane maps to depth 1)
    if ortho_height is None:
        s = 1.0 / np.tan(np.radians(fov_deg) / 2)
        P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = s * H / W, s, f / (f - n), 1.0, -n * f / (f - n)
    else:
        P[0, 0], P[1, 1], P[2, 2], P[3, 2], P[3, 3] = 2.0 / (ortho_height * W / H), 2.0 / ortho_height, 1.0 / (f - n), -n / (f - n), 1.0
    VP = V @ P
    c = np.zeros(144, np.float64)
    c[CAM_POS:CAM_POS + 4] = [*eye, 1.0]
    c[CAM_VIEWPORT:CAM_VIEWPORT + 4] = [W, H, 1.0 / W, 1.0 / H]
    c[CAM_NEAR_Z], c[CAM_FAR_Z] = near, far
    c[CAM_NEAR_DEPTH], c[CAM_FAR_DEPTH] = (1.0, 0.0) if reversed_depth else (0.0, 1.0)
    c[12:16] = [near, far, c[CAM_NEAR_DEPTH], c[CAM_FAR_DEPTH]]
    c[16] = 1.0
    c[CAM_JITTER:CAM_JITTER + 2] = jitter
    for off, m in ((CAM_VIEW, V), (CAM_PROJ, P), (CAM_VIEWPROJ, VP), (CAM_VIEW_INV, np.linalg.inv(V)), (CAM_PROJ_INV, np.linalg.inv(P)), (CAM_VIEWPROJ_INV, np.linalg.inv(VP))):
        c[off:off + 16] = m.reshape(16)
    return c.astype(F)


def camera_z_to_depth(z, cam):
    """CameraZToDepth in float64 (for building depth planes)."""
    P = cam[CAM_PROJ:CAM_PROJ + 16].astype(np.float64).reshape(4, 4)
    return ((P[2, 2] * z + P[3, 2]) / (P[2, 3] * z + P[3, 3])).astype(F)


def saturate(x):
    return np.fmin(np.fmax(x, F(0)), F(1))  # saturate(NaN) = 0


def ndc_of(x, y, W, H, cam):
    u = (x.astype(F) + F(0.5)) / F(W)
    v = (y.astype(F) + F(0.5)) / F(H)
    return (F(2) * u - F(1)) + cam[CAM_JITTER], (F(1) - F(2) * v) + cam[CAM_JITTER + 1]


def unproject(nx, ny, z, M):
    r = [nx * M[0 + i] + ny * M[4 + i] + F(z) * M[8 + i] + M[12 + i] for i in range(4)]
    return [r[0] / r[3], r[1] / r[3], r[2] / r[3]]


def camera_ray(nx, ny, cam):
    """CreateCameraRay: (origin[3], direction[3])"""
    M = cam[CAM_VIEWPROJ_INV:CAM_VIEWPROJ_INV + 16]
    s = unproject(nx, ny, cam[CAM_NEAR_DEPTH], M)
    e = unproject(nx, ny, cam[CAM_FAR_DEPTH], M)
    d = [e[i] - s[i] for i in range(3)]
    inv = F(1) / np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    d = [c * inv for c in d]
    if cam[CAM_PROJ + 15] == 0:
        o = [np.full_like(nx, cam[CAM_POS + i]) for i in range(3)]
    else:
        o = s
    return o, d


def plane_hit(o, d, axis):
    nd = d[axis]
    nd = np.fmax(np.abs(nd), F(1e-6)) * np.where(nd > 0, F(1), F(-1))
    dist = (F(0) - o[axis]) / nd
    return dist, [o[i] + d[i] * dist for i in range(3)]


def depth_range(cam, min_depth, max_depth):
    P = cam[CAM_PROJ:CAM_PROJ + 16]
    sx, sy = cam[CAM_VIEWPORT + 2] / P[0], cam[CAM_VIEWPORT + 3] / P[5]
    pixel = np.sqrt(sx * sx + sy * sy)
    z0 = (P[14] - min_depth * P[15]) / (min_depth * P[11] - P[10])
    z1 = (P[14] - max_depth * P[15]) / (max_depth * P[11] - P[10])
    max_z = np.fmax(z0, z1)
    return pixel, max_z, np.fmax(max_z - np.fmin(z0, z1), F(1e-6))


def view_z(p, cam):
    V = cam[CAM_VIEW:CAM_VIEW + 16]
    return p[0] * V[2] + p[1] * V[6] + p[2] * V[10] + V[14]


def ipow(s, e):
    """pow(s, e) for e = floor(x) >= 0 as the product of e factors from the left (the product's grid_ipow)."""
    n = np.fmin(e, F(128)).astype(np.int32)
    p = np.ones_like(e, dtype=F)
    for k in range(int(n.max()) if n.size else 0):
        p = np.where(k < n, p * F(s), p)
    return p


def log10_f32(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log10(x.astype(np.float64)).astype(F)


PLANE_COORDS = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def coord_and_fwidth(x, y, W, H, cam, axis, scale):
    """Coord = PlanePos * Scale of the plane whose normal is `axis` at the pixels (x, y), and fwidth(Coord) by the quad convention."""
    def coord(px, py):
        o, d = camera_ray(*ndc_of(px, py, W, H, cam), cam)
        _, p = plane_hit(o, d, axis)
        i, j = PLANE_COORDS[axis]
        return p[i] * F(scale), p[j] * F(scale)

    c, ch, cv = coord(x, y), coord(x ^ 1, y), coord(x, y ^ 1)
    right, bottom = (x & 1) != 0, (y & 1) != 0
    mag = []
    for k in range(2):
        ddx = np.where(right, c[k] - ch[k], ch[k] - c[k])
        ddy = np.where(bottom, c[k] - cv[k], cv[k] - c[k])
        mag.append(np.abs(ddx) + np.abs(ddy))
    return c, mag


def lod_alpha(c, lod, lw):
    h = F(0.5) * lod
    with np.errstate(divide="ignore", invalid="ignore"):
        a = [F(1) - saturate(np.abs((np.fmod(np.abs(c[k] - h), lod) - h) / lw[k])) for k in range(2)]
    return np.fmax(a[0], a[1])


def grid_lines(c, mag, subdivision, a):
    """ComputeGrid: (rgb[3], alpha)"""
    lw = [F(0.5) * m * a[A_LINE_WIDTH] for m in mag]
    lod_level = np.fmax(F(0), log10_f32(np.sqrt(mag[0] * mag[0] + mag[1] * mag[1]) * a[A_MIN_CELL_WIDTH] / a[A_MIN_CELL_SIZE]) + F(1))
    lod_floor = np.floor(lod_level)
    fade = lod_level - lod_floor
    lod0 = a[A_MIN_CELL_SIZE] * ipow(subdivision, lod_floor)
    lod1 = lod0 * F(subdivision)
    lod2 = lod1 * F(subdivision)
    a0, a1, a2 = lod_alpha(c, lod0, lw), lod_alpha(c, lod1, lw), lod_alpha(c, lod2, lw)
    thick, thin = a[A_MAJOR:A_MAJOR + 3], a[A_MINOR:A_MINOR + 3]
    rgb = [np.where(a2 > 0, thick[k], np.where(a1 > 0, thick[k] + fade * (thin[k] - thick[k]), thin[k])) for k in range(3)]
    alpha = np.where(a2 > 0, a2, np.where(a1 > 0, a1, a0 * (F(1) - fade)))
    return rgb, alpha, lod_floor


def plane_alpha(dist, pos, cam, max_z, z_range):
    alpha = np.where(dist > 0, F(1), F(0))
    cz = view_z(pos, cam)
    alpha = alpha * saturate((max_z - cz) / z_range + F(0.1))
    return alpha * saturate(F(1) - cz / cam[CAM_FAR_Z])


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def axis_terms(o, d, axis):
    """(Denom, DistFromCamera, DistFromOrigin, DistToAxis) of ComputeAxis"""
    A = [np.full_like(d[0], F(1) if i == axis else F(0)) for i in range(3)]
    cr = cross(A, d)
    denom = dot3(cr, cr)
    with np.errstate(divide="ignore", invalid="ignore"):
        from_camera = dot3(cross(o, A), cr) / denom
        from_origin = dot3(cross(o, d), cr) / denom
        to_axis = np.abs(dot3(o, cr)) / np.fmax(np.sqrt(denom), F(0.001))
    return denom, from_camera, from_origin, to_axis


def axis_rgba(o, d, axis, pixel_size, max_z, z_range, cam, positive, negative):
    denom, from_camera, from_origin, to_axis = axis_terms(o, d, axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        width = np.full_like(d[0], pixel_size)
        if cam[CAM_PROJ + 15] == 0:
            width = width * from_camera
        line = np.abs(to_axis) / width
        alpha = (F(1) - np.fmin(line * line, F(1))) * saturate(F(1) - from_camera / cam[CAM_FAR_Z])
        A = [F(1) if i == axis else F(0) for i in range(3)]
        pos = [F(0) + A[i] * from_origin for i in range(3)]
        pz = view_z(pos, cam) + width
        alpha = alpha * saturate((max_z - pz) / z_range)
        inv = F(1) / np.sqrt(dot3(o, o))
        n = [c * inv for c in o]
        alpha = alpha * saturate((F(1) - np.abs(n[0] * A[0] + n[1] * A[1] + n[2] * A[2])) * F(1e6))
    live = (np.abs(denom) > F(1e-7)) & (from_camera > 0)
    alpha = np.where(live, alpha, F(0))
    col = [np.where(from_origin > 0, positive[k], negative[k]) for k in range(3)]
    return [np.where(live, col[k] * alpha, F(0)) for k in range(3)], alpha


def coordinate_grid(x, y, W, H, cam, min_depth, max_depth, attribs, flags):
    """ComputeCoordinateGrid at the pixels (x, y) (integer arrays) of a W x H frame: float32 array (..., 4)"""
    a = attribs
    nx, ny = ndc_of(x, y, W, H, cam)
    o, d = camera_ray(nx, ny, cam)
    pixel, max_z, z_range = depth_range(cam, np.asarray(min_depth, F), np.asarray(max_depth, F))
    grid = [np.zeros(nx.shape, F) for _ in range(4)]
    axes = [np.zeros(nx.shape, F) for _ in range(4)]
    for axis, flag, pos_c, neg_c in ((0, FLAG_AXIS_X, A_POS_X, A_NEG_X), (1, FLAG_AXIS_Y, A_POS_Y, A_NEG_Y), (2, FLAG_AXIS_Z, A_POS_Z, A_NEG_Z)):
        if flags & flag:
            rgb, alpha = axis_rgba(o, d, axis, pixel * a[A_WIDTHS + axis], max_z, z_range, cam, a[pos_c:pos_c + 3], a[neg_c:neg_c + 3])
            axes = [axes[k] + rgb[k] for k in range(3)] + [axes[3] + alpha]
    for axis, flag in ((0, FLAG_YZ), (1, FLAG_XZ), (2, FLAG_XY)):
        if flags & flag:
            dist, pos = plane_hit(o, d, axis)
            pa = plane_alpha(dist, pos, cam, max_z, z_range)
            c, mag = coord_and_fwidth(x, y, W, H, cam, axis, a[A_SCALE + axis])
            rgb, alpha, _ = grid_lines(c, mag, a[A_SUBDIV + axis], a)
            grid = [grid[k] + rgb[k] * pa for k in range(3)] + [grid[3] + alpha * pa]
    fade = np.exp((F(-10) * axes[3] * axes[3]).astype(np.float64)).astype(F) if flags & AXES else F(1)
    out = [grid[k] * fade + axes[k] for k in range(3)] + [grid[3] * (F(1) - axes[3]) + axes[3]]
    return np.stack(out, -1).astype(F)


def linear_to_srgb(c):
    with np.errstate(invalid="ignore"):
        hi = (np.power(c.astype(np.float64), 1.0 / 2.4).astype(F)) * F(1.055) - F(0.055)
    lo = c * F(12.92)
    return lo + np.where(c >= F(0.0031308), F(1), F(0)) * (hi - lo)


def pixel_grid(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return x.astype(np.int32), y.astype(np.int32)


def render(depth, cam, attribs, flags):
    """ComputeGridAxesPS (CoordinateGridPS.psh:24-38) over a whole depth plane"""
    H, W = depth.shape
    x, y = pixel_grid(W, H)
    out = coordinate_grid(x, y, W, H, cam, depth, depth, attribs, flags)
    if flags & FLAG_SRGB:
        out[..., :3] = linear_to_srgb(out[..., :3])
    return out


def depth_min_max_3x3(depth):
    """HnCopyFrame.psh:41-51: start values 1 / 0, a texel outside the frame reads 0"""
    H, W = depth.shape
    p = np.zeros((H + 2, W + 2), F)
    p[1:-1, 1:-1] = depth
    lo, hi = np.full((H, W), F(1)), np.full((H, W), F(0))
    for i in range(3):
        for j in range(3):
            t = p[j:j + H, i:i + W]
            lo, hi = np.fmin(lo, t), np.fmax(hi, t)
    return lo, hi


def copy_frame_tail(tone_mapped, depth, cam, attribs, flags, srgb=False):
    """HnCopyFrame.psh:38-62 on a colour that is already tone mapped: the 3x3 depth range, the grid, lerp, optional LinearToSRGB; alpha passes through"""
    H, W = depth.shape
    x, y = pixel_grid(W, H)
    lo, hi = depth_min_max_3x3(depth)
    g = coordinate_grid(x, y, W, H, cam, lo, hi, attribs, flags)
    out = tone_mapped.astype(F).copy()
    for k in range(3):
        out[..., k] = out[..., k] + g[..., 3] * (g[..., k] - out[..., k])
    if srgb:
        out[..., :3] = linear_to_srgb(out[..., :3])
    return out


def blend(dst, g):
    """BS_AlphaBlend on rgb: grid.rgb * grid.a + dst.rgb * (1 - grid.a); dst.a is left as it is"""
    out = dst.astype(F).copy()
    k = F(1) - g[..., 3]
    for c in range(3):
        out[..., c] = g[..., c] * g[..., 3] + dst[..., c] * k
    return out
