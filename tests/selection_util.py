"""A float32 numpy restatement of the selection outline of Hydrogent, step by step as the reference's shaders define it (test infrastructure):
  * the closest-selected-location plane: HnProcessSelectionTask.cpp:302-369 -- HnInitClosestSelectedLocation.psh, then HnUpdateClosestSelectedLocation.psh once per step
    with SampleRange = 1 << (n - 1 - i), n = ceil(log2(max(MaximumDistance, 1))) + 1 (HnProcessSelectionTask.cpp:71), encoded as HnClosestSelectedLocation.fxh;
  * the composite's selection tail: HnPostProcess.psh:211-241.
Every operation is one float32 numpy operation (no fused multiply-add), so the plane is the reference's bit for bit."""
import numpy as np

F = np.float32


def iterations(max_distance):
    """m_NumJFIterations (HnProcessSelectionTask.cpp:71)."""
    return int(np.ceil(np.log2(max(F(max_distance), F(1.0))))) + 1


def encode(lx, ly, valid):
    """EncodeClosestSelectedLocation (HnClosestSelectedLocation.fxh): (x, y * 0.5 + 0.5) for a location, (0, 0) for none."""
    out = np.zeros(lx.shape + (2,), F)
    out[..., 0] = np.where(valid, lx, F(0))
    out[..., 1] = np.where(valid, ly * F(0.5) + F(0.5), F(0))
    return out


def decode(enc):
    """DecodeClosestSelectedLocation: (valid, x, y); y <= 0.25 is invalid."""
    return enc[..., 1] > F(0.25), enc[..., 0], enc[..., 1] * F(2.0) - F(1.0)


def init(selection_depth, clear_depth):
    """HnInitClosestSelectedLocation.psh: IsSelected = depth != ClearDepth, Location = f4PixelPos.xy / (Width, Height)."""
    h, w = selection_depth.shape
    x = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    y = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    lx, ly = np.broadcast_to(x[None, :], (h, w)), np.broadcast_to(y[:, None], (h, w))
    return encode(lx, ly, selection_depth != F(clear_depth))


def tap(p, offset, sample_range, n):
    """Load(int(Pos + Offset * SampleRange)) along one axis, Pos = p + 0.5: the conversion truncates toward zero, so p + o * r = -1 reads texel 0 and anything below
    -1 or at n and beyond is outside the frame (a Load there returns 0).  Returns (clamped index, inside)."""
    t = p + offset * sample_range
    t = np.where(t == -1, 0, t)
    inside = (t >= 0) & (t < n)
    return np.clip(t, 0, n - 1), inside


def step(src, sample_range):
    """HnUpdateClosestSelectedLocation.psh: nine taps in the shader's order, the first strictly closer candidate wins (ClosestDistance starts at 1e10)."""
    h, w = src.shape[:2]
    xs, ys = np.arange(w), np.arange(h)
    px, py = (xs.astype(F) + F(0.5))[None, :], (ys.astype(F) + F(0.5))[:, None]
    best = np.full((h, w), F(1e10), F)
    cx, cy = np.zeros((h, w), F), np.zeros((h, w), F)
    valid = np.zeros((h, w), bool)
    for oy in (-1, 0, 1):
        ty, iny = tap(ys, oy, sample_range, h)
        for ox in (-1, 0, 1):
            tx, inx = tap(xs, ox, sample_range, w)
            e = src[ty][:, tx]
            ok, lx, ly = decode(e)
            ok = ok & iny[:, None] & inx[None, :]
            dx = lx * F(w) - px
            dy = ly * F(h) - py
            d2 = dx * dx + dy * dy
            take = ok & (d2 < best)
            best = np.where(take, d2, best)
            cx, cy = np.where(take, lx, cx), np.where(take, ly, cy)
            valid |= take
    return encode(cx, cy, valid)


def jump_flood(selection_depth, clear_depth=1.0, max_distance=4.0, selection_id=1):
    """The final closest-selected-location plane (HnProcessSelectionTask::Execute); nothing selected: the target cleared to 0 (:329-335)."""
    selection_depth = np.asarray(selection_depth, F)
    if selection_id == 0:
        return np.zeros(selection_depth.shape + (2,), F)
    n = iterations(max_distance)
    p = init(selection_depth, clear_depth)
    for i in range(n):
        p = step(p, 1 << (n - 1 - i))
    return p


def composite_tail(rgba, depth, selection_depth, closest, outline_color, occluded_color, desaturation=0.0, clear_depth=1.0, outline_width=4.0):
    """HnPostProcess.psh:211-241 on the composite's colour (after its optional tone map).  lerp(a, b, t) = a + t * (b - a).  Alpha untouched."""
    rgba = np.array(rgba, F)
    depth, selection_depth = np.asarray(depth, F), np.asarray(selection_depth, F)
    h, w = depth.shape
    clear = F(clear_depth)
    r, g, b = rgba[..., 0], rgba[..., 1], rgba[..., 2]
    selected = (depth != clear) & (selection_depth == depth)
    desat = np.where(selected, F(0), F(desaturation))
    lum = r * F(0.2126) + g * F(0.7152) + b * F(0.0722)
    rgb = [c + desat * (lum - c) for c in (r, g, b)]
    valid, lx, ly = decode(np.asarray(closest, F))
    lx, ly = lx * F(w), ly * F(h)
    dx = lx - (np.arange(w, dtype=F) + F(0.5))[None, :]
    dy = ly - (np.arange(h, dtype=F) + F(0.5))[:, None]
    dist = np.sqrt(dx * dx + dy * dy)
    outline = np.clip(F(1) - dist / F(outline_width), F(0), F(1))
    outline = outline * np.where(selection_depth != clear, F(0), F(1))
    draw = valid & (outline > F(0))
    ix, iy = np.trunc(lx).astype(np.int64), np.trunc(ly).astype(np.int64)
    inside = draw & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    ixc, iyc = np.clip(ix, 0, w - 1), np.clip(iy, 0, h - 1)
    d = np.where(inside, depth[iyc, ixc], F(0))
    sd = np.where(inside, selection_depth[iyc, ixc], F(0))
    visible = d == sd
    for c in range(3):
        col = np.where(visible, F(outline_color[c]), F(occluded_color[c]))
        rgb[c] = np.where(draw, rgb[c] + outline * (col - rgb[c]), rgb[c])
    out = rgba.copy()
    for c in range(3):
        out[..., c] = rgb[c]
    return out


def make_selection_depth(depth, rng, clear_depth=1.0, occluded_frac=0.3, seeds=6, max_radius=None):
    """A selection depth plane for tests: a few random discs of `depth` (the selected prim rendered where it is visible), part of them offset so that the scene
    occludes them (selection depth != depth there), clear_depth elsewhere."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    sel = np.full((h, w), F(clear_depth), F)
    yy, xx = np.mgrid[0:h, 0:w]
    max_radius = max_radius or max(2, min(w, h) // 8)
    for _ in range(seeds):
        cx, cy, rad = rng.integers(0, w), rng.integers(0, h), rng.integers(1, max_radius + 1)
        m = (xx - cx) ** 2 + (yy - cy) ** 2 <= rad * rad
        sel[m] = depth[m]
        if rng.random() < occluded_frac:
            sel[m] = depth[m] * F(0.5) + F(0.25)  # (differs from the scene depth: occluded)
    return sel
