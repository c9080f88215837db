"""Shared helpers of the cascaded-shadow tests (test infrastructure): the synthetic inputs that tests/golden/make_golden_shadows.py stores and that the larger
device-against-host comparison rebuilds -- a ground plane seen by a perspective camera, a directional light with nested orthographic cascades, and shadow-map slices
that are NOT rendered: every texel holds the ground's own light-space depth plus or minus a relief of at least 0.03, so both outcomes of every depth comparison occur
and no receiver lies on its occluder's depth."""
import ctypes

import numpy as np

import grid_util as G

F = np.float32
MODE_PCF, MODE_VSM, MODE_EVSM2, MODE_EVSM4 = 1, 2, 3, 4
FLT_MAX = float(np.finfo(np.float32).max)


def attribs_struct():
    from diligentfx_amd import binding as B

    return B.ShadowMapAttribs


def light_view():
    """mWorldToLightView (row-vector): a directional light from above, slanted"""
    d = np.array([0.35, -1.0, 0.25])
    d /= np.linalg.norm(d)
    eye = np.array([0.0, 0.0, 8.0]) - 30.0 * d
    z = d
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    V = np.eye(4)
    V[:3, 0], V[:3, 1], V[:3, 2] = x, y, z
    V[3, :3] = [-x @ eye, -y @ eye, -z @ eye]
    return V


Z_NEAR, Z_RANGE = 5.0, 50.0  # light-space z range of every cascade


def cascade(i, V):
    """Cascade i: a box of half extent e_i around the light-space position of the ground point (0, 0, end_i / 2); camera-space z range [start_i, end_i]"""
    end = 5.0 * 1.5 ** (i + 1)
    start = 0.5 if i == 0 else 5.0 * 1.5 ** i
    e = 1.1 * end
    c = np.array([0.0, 0.0, end / 2.0, 1.0]) @ V
    scale = np.array([1.0 / e, 1.0 / e, 1.0 / Z_RANGE, 0.0])
    bias = np.array([-c[0] / e, -c[1] / e, -Z_NEAR / Z_RANGE, 0.0])
    return dict(scale=scale, bias=bias, start_end=np.array([start, end, 0.0, 0.0]), margin=np.array([0.06, 0.06, 0.02, 0.02]))


def make_attribs(n, map_w, map_h, **over):
    """ShadowMapAttribs bytes (1200) as a float32 / int32 view pair: returns the ctypes struct"""
    A = attribs_struct().default()
    V = light_view()
    A.mWorldToLightView[:] = [float(v) for v in V.reshape(16).astype(F)]
    for i in range(8):
        c = cascade(i, V)
        A.Cascades[i].f4LightSpaceScale[:] = [float(v) for v in c["scale"].astype(F)]
        A.Cascades[i].f4LightSpaceScaledBias[:] = [float(v) for v in c["bias"].astype(F)]
        A.Cascades[i].f4StartEndZ[:] = [float(v) for v in c["start_end"].astype(F)]
        A.Cascades[i].f4MarginProjSpace[:] = [float(v) for v in c["margin"].astype(F)]
        A.fCascadeCamSpaceZEnd[i] = float(c["start_end"][1]) if i < n else FLT_MAX  # (ShadowMapManager.cpp:180: +FLT_MAX beyond the last cascade)
    A.f4ShadowMapDim[:] = [float(map_w), float(map_h), float(F(1.0 / map_w)), float(F(1.0 / map_h))]
    A.iNumCascades, A.fNumCascades = n, float(n)
    A.fVSMBias = 1e-3
    for k, v in over.items():
        setattr(A, k, v)
    return A


def attribs_from_bytes(b):
    return attribs_struct().from_buffer_copy(bytes(b))


def shadow_slices(n, w, h, seed=0):
    """(n, h, w) float32: per texel the ground's light-space depth in that cascade, moved towards the light (an occluder) or away from it (none) by 0.03 .. 0.06 in blocks"""
    V = light_view()
    Vi = np.linalg.inv(V)
    out = np.zeros((n, h, w), F)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        c = cascade(i, V)
        u, v = (xx + 0.5) / w, (yy + 0.5) / h
        nx, ny = 2.0 * u - 1.0, 1.0 - 2.0 * v
        lx, ly = (nx - c["bias"][0]) / c["scale"][0], (ny - c["bias"][1]) / c["scale"][1]
        lz = -(lx * Vi[0, 1] + ly * Vi[1, 1] + Vi[3, 1]) / Vi[2, 1]  # world y = 0
        ground = lz * c["scale"][2] + c["bias"][2]
        block = ((xx // (5 + i)) + (yy // (4 + i)) + seed) % 3
        relief = np.where(block == 0, -1.0, 1.0) * (0.03 + 0.03 * (0.5 + 0.5 * np.sin(0.7 * xx + 0.4 * yy + i)))
        out[i] = np.clip(ground + relief, 0.0, 1.0).astype(F)
    return out


def frame_camera(W, H):
    return G.make_camera(W, H, eye=(0.0, 6.0, -10.0), at=(0.0, 0.0, 4.0), fov_deg=60.0, near=0.5, far=60.0)


def frame_depth(cam, W, H):
    """The ground plane y = 0 (and two raised slabs) through the camera; rays that miss it, or hit it beyond the far plane, are background (fFarPlaneDepth)"""
    x, y = G.pixel_grid(W, H)
    nx, ny = 2.0 * ((x + 0.5) / W) - 1.0, 1.0 - 2.0 * ((y + 0.5) / H)
    M = cam[G.CAM_VIEWPROJ_INV:G.CAM_VIEWPROJ_INV + 16].astype(np.float64).reshape(4, 4)
    View = cam[G.CAM_VIEW:G.CAM_VIEW + 16].astype(np.float64).reshape(4, 4)

    def unproject(z):
        p = np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], -1) @ M
        return p[..., :3] / p[..., 3:4]

    o, e = unproject(0.0), unproject(1.0)
    d = e - o
    depth = np.full((H, W), cam[G.CAM_FAR_DEPTH], F)
    for height, x0, x1 in ((0.0, -1e9, 1e9), (1.5, -6.0, -2.0), (0.8, 3.0, 9.0)):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (height - o[..., 1]) / d[..., 1]
        hit = o + t[..., None] * d
        camz = hit @ View[:3, 2] + View[3, 2]
        ok = (t > 0) & (t < 1) & (hit[..., 0] > x0) & (hit[..., 0] < x1) & ((height == 0.0) | ((hit[..., 2] > 2.0) & (hit[..., 2] < 12.0)))
        dz = G.camera_z_to_depth(np.where(ok, camz, 1.0), cam)
        depth = np.where(ok & (dz < depth), dz, depth).astype(F)
    return depth


def periodic_slices(n, w, h):
    """(n, h, w) float32 depths in [0, 1] with a period of 13 x 7 texels (coprime with every tile size), a different phase per slice: the conversion's expected output is
    then periodic away from the borders and compresses well"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(((xx % 13) * 5 + (yy % 7) * 11 + s * 3) % 17 / 16.0 * 0.9 + 0.05).astype(F) for s in range(n)])


def camera_struct(cam):
    from diligentfx_amd import binding as B

    return B.camera_from_bytes(np.asarray(cam, F).tobytes())


def fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
