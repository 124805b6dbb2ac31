"""
Friction maps: location dependent grip for ``calc_vel_profile``'s ``local_gg`` (OnlineTrajectoryHandler.py:633-666: a dict with one
``[ax, ay]`` row per path coordinate of every offered key). ``FrictionGrid`` is the HOST MIRROR and the definition of the maps a fleet keeps
in device memory (``Fleet.friction``, ltpl_fleet_friction, csrc/fleet_core.hpp ``friction_at``): the device reproduces ``rows`` bit for bit.
"""
import numpy as np


class FrictionGrid:
    """Regular grid of friction limits, bilinear inside a cell, clamped at the border. Node (iy, ix) lies at (x0 + ix dx, y0 + iy dy);
    ``ax`` / ``ay``: [ny, nx] with nx, ny >= 2, dx, dy > 0, every value finite and positive."""

    def __init__(self, x0, y0, dx, dy, ax, ay):
        self.x0, self.y0, self.dx, self.dy = float(x0), float(y0), float(dx), float(dy)
        self.ax = np.ascontiguousarray(np.asarray(ax, np.float64))
        self.ay = np.ascontiguousarray(np.asarray(ay, np.float64))
        if self.ax.ndim != 2 or self.ax.shape != self.ay.shape or min(self.ax.shape) < 2:
            raise ValueError("FrictionGrid: ax and ay need the same shape [ny, nx] with nx, ny >= 2")
        if not (np.isfinite([self.x0, self.y0, self.dx, self.dy]).all() and self.dx > 0.0 and self.dy > 0.0):
            raise ValueError("FrictionGrid: x0, y0 must be finite, dx and dy finite and positive")
        for a in (self.ax, self.ay):
            if not (np.isfinite(a).all() and (a > 0.0).all()):
                raise ValueError("FrictionGrid: node values must be finite and positive")
        self.ny, self.nx = self.ax.shape

    @staticmethod
    def _cell(t0, d, q, n):
        t = (q - t0) / d
        f = np.floor(t)
        f = np.where(f >= 0.0, f, 0.0)                    # (not (f >= 0) -> 0: a NaN coordinate reads cell 0)
        f = np.where(f > float(n - 2), float(n - 2), f)
        u = t - f
        u = np.where(u < 0.0, 0.0, u)
        u = np.where(u > 1.0, 1.0, u)
        return f.astype(np.int64), u

    def rows(self, xy, scale=1.0):
        """[n, 2] = [ax, ay] at the points ``xy`` [n, 2], times ``scale``. THE ORDER OF OPERATIONS (fp64, no fused multiply-add), for x
        (y likewise with y0, dy, ny, giving fy and v)::

            tx = (x - x0) / dx
            fx = floor(tx);  not (fx >= 0): fx = 0;  fx > nx - 2: fx = nx - 2        (cell index)
            u  = tx - fx;    u < 0: u = 0;           u > 1: u = 1                    (fraction)
            lo = (1 - u) * a[fy, fx]     + u * a[fy, fx + 1]
            hi = (1 - u) * a[fy + 1, fx] + u * a[fy + 1, fx + 1]
            value = ((1 - v) * lo + v * hi) * scale

        for ``ax`` and ``ay`` each. A node reproduces its value exactly (u, v in {0, 1}: one weight is 1, the other 0); outside the grid
        the nearest border value holds."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        ix, u = self._cell(self.x0, self.dx, xy[:, 0], self.nx)
        iy, v = self._cell(self.y0, self.dy, xy[:, 1], self.ny)
        cu, cv = 1.0 - u, 1.0 - v
        s = np.float64(scale)
        out = np.empty((xy.shape[0], 2), np.float64)
        for c, a in enumerate((self.ax, self.ay)):
            lo = cu * a[iy, ix] + u * a[iy, ix + 1]
            hi = cu * a[iy + 1, ix] + u * a[iy + 1, ix + 1]
            out[:, c] = (cv * lo + v * hi) * s
        return out

    def local_gg(self, paths, scale=1.0):
        """The dict ``calc_vel_profile`` takes as ``local_gg``: ``paths`` = {key: path_param rows [x, y, ...]} (or {key: [rows]}, the
        reference's action set) -> {key: [rows(path_param[:, 0:2])]}."""
        out = {}
        for k, pp in paths.items():
            if isinstance(pp, (list, tuple)):
                pp = pp[0]
            pp = np.asarray(pp, np.float64)
            out[k] = [self.rows(pp[:, 0:2], scale)]
        return out

    def inside(self, xy):
        """[n] bool: the point lies inside the grid (no clamping)."""
        xy = np.asarray(xy, np.float64).reshape(-1, 2)
        return ((xy[:, 0] >= self.x0) & (xy[:, 0] <= self.x0 + self.dx * (self.nx - 1)) &
                (xy[:, 1] >= self.y0) & (xy[:, 1] <= self.y0 + self.dy * (self.ny - 1)))

    def nodes(self):
        """[ny * nx, 2]: [ax, ay] of node (iy, ix) at row iy * nx + ix (the layout of ltpl_fleet_friction_in.nodes)."""
        return np.ascontiguousarray(np.column_stack((self.ax.reshape(-1), self.ay.reshape(-1))))

    @classmethod
    def from_function(cls, f, bbox, cell):
        """Samples ``f(xy [n, 2]) -> [n, 2]`` on nodes ``cell`` apart (scalar or (dx, dy)) covering ``bbox`` = (xmin, ymin, xmax, ymax)."""
        xmin, ymin, xmax, ymax = (float(b) for b in bbox)
        dx, dy = (float(cell), float(cell)) if np.ndim(cell) == 0 else (float(cell[0]), float(cell[1]))
        nx = max(2, int(np.ceil((xmax - xmin) / dx)) + 1)
        ny = max(2, int(np.ceil((ymax - ymin) / dy)) + 1)
        gx, gy = np.meshgrid(xmin + dx * np.arange(nx), ymin + dy * np.arange(ny))
        val = np.asarray(f(np.column_stack((gx.reshape(-1), gy.reshape(-1)))), np.float64).reshape(-1, 2)
        return cls(xmin, ymin, dx, dy, val[:, 0].reshape(ny, nx), val[:, 1].reshape(ny, nx))

    def save(self, path):
        np.savez_compressed(path, geom=np.array([self.x0, self.y0, self.dx, self.dy], np.float64), ax=self.ax, ay=self.ay)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            g = z["geom"]
            return cls(g[0], g[1], g[2], g[3], z["ax"], z["ay"])
