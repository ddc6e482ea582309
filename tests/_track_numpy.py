"""An independent restatement of the track-sample contract (include/picles_hip.h "track samples") and of the TrackWriter's record
arithmetic (picles_amd/track_output.py, module docstring), fed from full State arrays — the host route: step, get_state, step ...
The station definition is tests/_station_numpy.py's, event by event and corner by corner with NumPy fp64 scalars."""
import numpy as np

import _station_numpy as SN

G_ANY, RG_ANY = 9.81, 0.9          # record() wants them; only its first three values (E, MX, MY) are used here


def is_wet(v):
    e, mx, my = (np.float64(x) for x in v)
    return bool(np.isfinite(e) and np.isfinite(mx) and np.isfinite(my) and e > 0 and mx * mx + my * my > 0)


def event_means(S, corners, weights):
    """(E, MX, MY) of one event from State S [Nx, Ny, 3]: NaN in all three when not valid; and its number of wet corners"""
    cv = [(tuple(S[i, j, :]), w) for (i, j), w in zip(corners, weights)]
    return SN.record(cv, G_ANY, RG_ANY)[:3], sum(is_wet(v) for v, _ in cv)


class Table:
    """the 8 x m table and the rule of a sample"""

    def __init__(self, times, corners, weights, H):
        self.t, self.corners, self.weights, self.H = np.asarray(times, dtype=np.float64), corners, weights, np.float64(H)
        assert (np.diff(self.t) >= 0).all()
        self.tab = np.full((8, len(self.t)), np.nan)
        self.n_wet = np.full(len(self.t), -1)          # wet corners at the event's latest before-sample
        self.visits = []                               # per sample: the indices visited

    def sample(self, T, S):
        T = np.float64(T)
        lo, hi = T - self.H, T + self.H
        seen = [k for k in range(len(self.t)) if lo < self.t[k] < hi]
        self.visits.append(seen)
        for k in seen:
            v, nw = event_means(S, self.corners[k], self.weights[k])
            if self.t[k] >= T:
                self.tab[0:3, k], self.tab[3, k], self.n_wet[k] = v, T, nw
            if self.t[k] <= T and np.isnan(self.tab[7, k]):
                self.tab[4:7, k], self.tab[7, k] = v, T
        return self

    def copy(self):
        c = Table(self.t, self.corners, self.weights, self.H)
        c.tab, c.n_wet, c.visits = self.tab.copy(), self.n_wet.copy(), list(self.visits)
        return c


def records(tab, times, g, r_g):
    """[m, 8] in the order of station_output.VAR_NAMES: the writer's interpolation and record arithmetic, event by event"""
    out = np.full((len(times), 8), np.nan)
    two, four = np.float64(2.0), np.float64(4.0)
    for k, tk in enumerate(np.asarray(times, dtype=np.float64)):
        col = tab[:, k]
        if np.isnan(col).any():
            continue
        tb, ta = col[3], col[7]
        if ta == tb:
            E, MX, MY = col[0], col[1], col[2]
        else:
            s = (tk - tb) / (ta - tb)
            E, MX, MY = (col[q] + s * (col[4 + q] - col[q]) for q in range(3))
        M2 = MX * MX + MY * MY
        if not M2 > 0:
            continue
        cbar = E / (two * np.sqrt(M2))
        tp = (SN.FOUR_PI * max(cbar / np.float64(r_g), np.float64(0.1))) / np.float64(g)
        out[k] = [E, MX, MY, four * np.sqrt(E), tp, (MX * E) / (two * M2), (MY * E) / (two * M2), np.arctan2(MY, MX)]
    return out


def make_events(grid, periodic_model, clocks, dt, seed=20250611, wet=None, never=None):
    """(times, points) in a shuffled caller's order, about 300 events over [T_0 - 2 dt, T_n + 2 dt] for sample clocks T_0 .. T_n
    (n >= 6): events exactly on T_0, on an interior clock and on T_n; equal times; more than 64 events in (T_2, T_3) and none in
    (T_4, T_5); points on a node, on cell edges, on the last node of an open axis, across a periodic wrap, and in cells with four
    and with one to three dry corners where the mask has any (land, coast, and the rim of a model without periodic_boundary).
    wet: bool [Nx, Ny], the nodes that carry sea at every sample of the host route: six in seven of the random points fall into cells
    whose four corners do (a sphere under one wind blob is calm, and so not valid, over most of its area).  never: bool [Nx, Ny],
    the nodes that carry none at the samples T_1 and T_2 — the special points' times lie between them —: they, not the mask, say
    which cells are dry (the seeded State is wet on coast and rim, and a coast node keeps what the scatter leaves on it)"""
    from picles_amd.station_output import _kind
    xs, ys = np.asarray(grid.data.x)[:, 0].astype(np.float64), np.asarray(grid.data.y)[0, :].astype(np.float64)
    Nx, Ny = len(xs), len(ys)
    dx, dy = (xs[-1] - xs[0]) / (Nx - 1), (ys[-1] - ys[0]) / (Ny - 1)
    px, py = _kind(grid.stats.Nx) == "periodic", _kind(grid.stats.Ny) == "periodic"
    top = Ny - 3 if _kind(grid.stats.Ny) == "tripolar" else Ny - 1
    rng = np.random.default_rng(seed)
    T0, Tn = clocks[0], clocks[-1]

    def rand_points(n):
        x = xs[0] + rng.uniform(0.0, 1.0, n) * ((Nx if px else Nx - 1) * dx) * 0.999
        y = ys[0] + rng.uniform(0.0, 1.0, n) * ((Ny if py else top) * dy) * 0.999
        if wet is not None:
            cells = np.argwhere(wet[:-1, :-1] & wet[1:, :-1] & wet[:-1, 1:] & wet[1:, 1:])
            cells = cells[cells[:, 1] < top]
            if len(cells):
                c = cells[rng.integers(len(cells), size=n)]
                fx, fy, use = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n) < 6.0 / 7.0
                x = np.where(use, xs[c[:, 0]] + fx * dx, x)
                y = np.where(use, ys[c[:, 1]] + fy * dy, y)
        return list(zip(x, y))

    t = list(rng.uniform(T0 - 2 * dt, Tn + 2 * dt, 180))
    t = [v for v in t if not (clocks[4] < v < clocks[5])]                      # an interval with no event
    t += list(rng.uniform(clocks[2] + 0.01 * dt, clocks[3] - 0.01 * dt, 80))   # ... and one with more than a workgroup of them
    t += [T0] * 4 + [clocks[3]] * 4 + [Tn] * 4                                 # exactly on clocks
    t += [t[5]] * 3 + [t[11]] * 3                                              # equal times
    p = rand_points(len(t))
    sp = [(xs[5], ys[3]), (xs[7], ys[2] + 0.4 * dy), (xs[3] + 0.25 * dx, ys[4])]          # a node, two cell edges
    if not px:
        sp += [(xs[-1], ys[2] + 0.5 * dy), (xs[-1], ys[3])]
    if not py and top == Ny - 1:
        sp += [(xs[4] + 0.5 * dx, ys[-1])]
        if not px:
            sp += [(xs[-1], ys[-1])]
    if px:
        sp += [(xs[-1] + 0.3 * dx, ys[3] + 0.2 * dy), (xs[-1] + 0.999 * dx, ys[1])]
    if py:
        sp += [(xs[2] + 0.1 * dx, ys[-1] + 0.6 * dy)]
    mask = np.asarray(grid.data.mask)
    dry = (mask == 0) | (mask == 2) | ((mask == 3) & (not periodic_model)) if never is None else never
    sure = np.ones_like(dry) if wet is None else (wet | dry)          # every corner is always wet or never
    nd = dry[:-1, :-1].astype(int) + dry[1:, :-1] + dry[:-1, 1:] + dry[1:, 1:]
    nd[~(sure[:-1, :-1] & sure[1:, :-1] & sure[:-1, 1:] & sure[1:, 1:])] = -1
    nd[:, top:] = -1
    cells = [c for c in np.argwhere(nd == 4)][:6]
    part = np.argwhere((nd > 0) & (nd < 4))
    cells += [part[k] for k in np.linspace(0, len(part) - 1, min(len(part), 10)).astype(int)] if len(part) else []
    sp += [(xs[i] + 0.3 * dx, ys[j] + 0.6 * dy) for i, j in cells]
    t += list(rng.uniform(clocks[1] + 0.01 * dt, clocks[2] - 0.01 * dt, len(sp)))
    p += sp
    order = rng.permutation(len(t))
    return np.asarray(t, dtype=np.float64)[order], np.asarray(p, dtype=np.float64)[order]
