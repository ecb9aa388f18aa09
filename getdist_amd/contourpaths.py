"""
Contour geometry of 2D densities, traced on the device: what ``ax.contour`` / ``ax.contourf`` otherwise get from a host
contouring library one grid at a time.  ``contour_paths`` sends a batch of grids through one native call
(``gd_contour_paths``, csrc/contourpaths.hip) and returns one ``ContourPaths`` per density; ``Density2D.getContourPaths`` and
``MCSamples.get2DContourPaths`` are the single-density and the samples-to-paths forms.

The raw result per (density, level) is the boundary of ``{P > level}`` as closed loops with the set on their left --
peaks counter-clockwise, holes clockwise -- that run along the domain edge where the set touches it (those vertices carry
flag 1): ``xy[n, 2]``, ``flag[n]`` and ``loop_off[nloops + 1]``, the loops ordered by their smallest lattice edge
(include/gdhip.h has the full statement).  ``ContourPaths`` turns that into polygons, contour lines and matplotlib paths.
"""

import numpy as np

from .densities import DensitiesError

MAX_LEVELS, MAX_SIDE = 8, 4096


def _ring_area(r):
    if len(r) < 3:
        return 0.0
    x, y = r[:, 0], r[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


class ContourPaths:
    """The contours of one density at ``levels``.  ``raw[k]`` = (xy, flag, loop_off) of level k; needs no device."""

    def __init__(self, x, y, levels, raw, density=None):
        self.x, self.y = np.asarray(x), np.asarray(y)
        self.levels = np.asarray(levels, dtype=np.float64).reshape(-1)
        self.raw = [(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(flag, dtype=np.uint8).reshape(-1),
                     np.asarray(off, dtype=np.int64).reshape(-1)) for xy, flag, off in raw]
        if len(self.raw) != len(self.levels):
            raise ValueError("one raw result per level")
        self.density = density

    def __len__(self):
        return len(self.levels)

    def loops(self, k):
        """[(xy, flag)] of the closed loops of level k, as traced."""
        xy, flag, off = self.raw[k]
        return [(xy[a:b], flag[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]

    def polygons(self, k):
        """The (m, 2) rings of {P > levels[k]}: outer rings counter-clockwise, holes clockwise, not repeating the first point;
        consecutive identical points are dropped, and with them rings that keep fewer than three."""
        out = []
        for p, _ in self.loops(k):
            keep = np.any(p != np.roll(p, 1, axis=0), axis=1)
            if int(keep.sum()) >= 3:
                out.append(p[keep])
        return out

    def lines(self, k):
        """The contour lines proper: every loop without its flagged vertices, i.e. split where it runs along the domain
        edge.  A loop without flagged vertices comes back closed, its first point repeated at the end."""
        out = []
        for p, f in self.loops(k):
            marks = np.flatnonzero(f)
            if marks.size == 0:
                out.append(np.concatenate([p, p[:1]]))
                continue
            shift = int(marks[-1]) + 1  # start behind a flagged vertex, so that no line wraps around the end
            p, f = np.roll(p, -shift, axis=0), np.roll(f, -shift)
            cuts = np.flatnonzero(f)
            start = 0
            for c in cuts.tolist():
                if c > start:
                    out.append(p[start:c].copy())
                start = c + 1
        return out

    def area(self, k):
        """Sum of the signed areas of the loops of level k: the area of {P > levels[k]} (holes count negative)."""
        return float(sum(_ring_area(p) for p, _ in self.loops(k)))

    def to_path(self, k, filled=True):
        """One compound matplotlib.path.Path of level k: the polygons (``filled``), or the lines."""
        from matplotlib.path import Path

        verts, codes = [], []
        for ring in (self.polygons(k) if filled else self.lines(k)):
            closed = filled or (len(ring) > 2 and bool(np.all(ring[0] == ring[-1])))
            pts = np.concatenate([ring, ring[:1]]) if filled else ring
            c = np.full(len(pts), Path.LINETO, dtype=Path.code_type)
            c[0] = Path.MOVETO
            if closed:
                c[-1] = Path.CLOSEPOLY
            verts.append(pts)
            codes.append(c)
        if not verts:
            return Path(np.zeros((0, 2)))
        return Path(np.concatenate(verts), np.concatenate(codes))


def _levels_of(densities, levels):
    B = len(densities)
    if levels is None:
        rows = []
        for d in densities:
            c = getattr(d, "contours", None)
            if c is None:
                raise DensitiesError("contour_paths: the density has no contour levels (pass levels=, or make it with "
                                     "get_density=False)")
            rows.append(np.asarray(c, dtype=np.float64).reshape(-1))
        if len({r.size for r in rows}) > 1:
            raise ValueError("contour_paths: the densities carry different numbers of contour levels")
        lv = np.array(rows, dtype=np.float64).reshape(B, -1)
    else:
        lv = np.asarray(levels, dtype=np.float64)
        if lv.ndim == 1:
            lv = np.tile(lv, (B, 1))
        if lv.ndim != 2 or lv.shape[0] != B:
            raise ValueError("contour_paths: levels must have shape (nc,) or (B, nc)")
    if not 1 <= lv.shape[1] <= MAX_LEVELS:
        raise ValueError("contour_paths: 1..%d levels per density" % MAX_LEVELS)
    if not np.all(np.isfinite(lv)):
        raise ValueError("contour_paths: non-finite contour level")
    return np.ascontiguousarray(lv)


def _shared_block(grids):
    """(block, element offset of every grid in it) when all grids are contiguous views of one float64 block that they
    mostly fill -- the page-locked block of a batched 2D call --, else None."""
    root = None
    for P in grids:
        a = P
        while isinstance(a.base, np.ndarray):
            a = a.base
        if root is None:
            root = a
        if a is not root or not P.flags.c_contiguous:
            return None
    if root.dtype != np.float64 or not root.flags.c_contiguous:
        return None
    flat = root.reshape(-1)
    offs = np.array([P.ctypes.data - flat.ctypes.data for P in grids], dtype=np.int64)
    if np.any(offs % 8) or np.any(offs < 0):
        return None
    offs //= 8
    ends = offs + np.array([P.size for P in grids], dtype=np.int64)
    lo, hi = int(offs.min()), int(ends.max())
    if hi > flat.size or hi - lo > 2 * sum(P.size for P in grids) + (1 << 17):
        return None
    return flat[lo:hi], offs - lo


def _pack_axes(axes):
    """The distinct arrays among ``axes`` (by identity: the pairs of a triangle share their parameters' axes) back to back,
    and every entry's offset into that."""
    at, parts, offs, total = {}, [], [], 0
    for a in axes:
        if id(a) not in at:
            at[id(a)] = total
            parts.append(np.asarray(a, dtype=np.float64).reshape(-1))
            total += parts[-1].size
        offs.append(at[id(a)])
    return np.concatenate(parts), np.array(offs, dtype=np.int64)


def contour_paths(densities, levels=None, ctx=None):
    """
    The contour paths of a batch of Density2D in one native call: a list of ContourPaths, one per density, each keeping
    its ``density``.  ``levels``: None for every density's own ``contours`` (DensitiesError when a density has none), an
    (nc,) array for all, or a (B, nc) array; 1 <= nc <= 8.  Grids may differ in size and need not be square (sides 2..4096).
    The grids go up in one copy: the block they already share when they are the grids of one batched 2D call, else a
    page-locked staging block they are packed into.  ``ctx``: the device context; None opens Context(0) for the call.
    A grid with a non-finite value raises DensitiesError; there is no host route.
    """
    densities = list(densities)
    if not densities:
        return []
    lv = _levels_of(densities, levels)
    grids = []
    for d in densities:
        P = np.asarray(d.P)  # (waits for a grid that is still in flight)
        if P.ndim != 2 or P.shape != (np.size(d.y), np.size(d.x)):
            raise DensitiesError("contour_paths: P must be a 2D grid matching the axes (P[iy, ix])")
        if min(P.shape) < 2 or max(P.shape) > MAX_SIDE:
            raise ValueError("contour_paths: grid sides must be 2..%d" % MAX_SIDE)
        grids.append(P)
    from ._lib import Context

    own = ctx is None
    if own:
        ctx = Context(0)
    dev = None
    try:
        shared = _shared_block(grids)
        if shared is None:
            sizes = np.array([P.size for P in grids], dtype=np.int64)
            offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
            block = ctx.pinned_array((int(sizes.sum()),), np.float64)
            for P, o in zip(grids, offs.tolist()):
                block[o:o + P.size] = P.reshape(-1)
        else:
            block, offs = shared
        dev = ctx.alloc(block.nbytes)
        dev.from_host(block)
        ny = [P.shape[0] for P in grids]
        nx = [P.shape[1] for P in grids]
        xs, x_off = _pack_axes([d.x for d in densities])
        ys, y_off = _pack_axes([d.y for d in densities])
        xy, flag, loops, voff, loff, status = ctx.contour_paths(dev, offs, ny, nx, xs, x_off, ys, y_off, lv)
    finally:
        if dev is not None:
            dev.free()
        if own:
            ctx.close()
    bad = np.flatnonzero(status)
    if bad.size:
        raise DensitiesError("contour_paths: non-finite value in the grid of density %d" % int(bad[0]))
    nc = lv.shape[1]
    voff, loff = voff.tolist(), loff.tolist()
    out = []
    for b, d in enumerate(densities):
        raw = []
        for t in range(b * nc, (b + 1) * nc):
            v0, v1 = voff[t], voff[t + 1]
            off = np.empty(loff[t + 1] - loff[t] + 1, dtype=np.int64)
            off[:-1] = loops[loff[t]:loff[t + 1]]
            off[-1] = v1 - v0
            raw.append((xy[v0:v1], flag[v0:v1], off))
        out.append(ContourPaths(d.x, d.y, lv[b], raw, density=d))
    return out
