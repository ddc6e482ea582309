"""The run-statistics contract of include/picles_hip.h ("run statistics") restated in vectorised NumPy fp64 over a list of
(State, clock) samples — State as picles_get_state returns it, shaped [Nx, ny, 3].  Test infrastructure: the device planes are held
against this bit for bit (tests/test_gpu_run_stats*.py), and this against a scalar pure-Python restatement that shares no code with
it (tests/test_run_stats_host.py).

Every operation below is one IEEE operation on float64 arrays (NumPy does not contract), in the order of the contract."""
import numpy as np

PEAK, MEAN, EXCEED = 1, 2, 4
PEAK_PLANES = ("e_peak", "mx_peak", "my_peak", "t_peak")
MEAN_PLANES = ("sum_e", "sum_mx", "sum_my", "sum_hs")


def zeros(shape, mask, thresholds=()):
    """all accumulators of the groups in `mask` at zero, for planes of `shape` = (Nx, ny)"""
    acc = {"n_wet": np.zeros(shape, dtype=np.uint32), "n_samples": 0, "t_first": 0.0, "t_last": 0.0}
    if mask & PEAK:
        acc.update({k: np.zeros(shape) for k in PEAK_PLANES})
    if mask & MEAN:
        acc.update({k: np.zeros(shape) for k in MEAN_PLANES})
    if mask & EXCEED:
        acc["n_exc"] = np.zeros(tuple(shape) + (len(thresholds),), dtype=np.uint32)
    return acc


def wet(S):
    e, mx, my = S[..., 0], S[..., 1], S[..., 2]
    with np.errstate(all="ignore"):
        m2 = mx * mx + my * my
        return np.isfinite(e) & np.isfinite(mx) & np.isfinite(my) & (e > 0.0) & (m2 > 0.0)


def update(acc, S, clock, mask, thresholds=()):
    """one update with the sample (S, clock), in place"""
    S = np.asarray(S, dtype=np.float64)
    e, mx, my = S[..., 0], S[..., 1], S[..., 2]
    w = wet(S)
    first = w & (acc["n_wet"] == 0)
    acc["n_wet"][w] += np.uint32(1)
    if mask & PEAK:
        with np.errstate(all="ignore"):
            new = first | (w & (e > acc["e_peak"]))
        acc["e_peak"][new] = e[new]
        acc["mx_peak"][new] = mx[new]
        acc["my_peak"][new] = my[new]
        acc["t_peak"][new] = clock
    if mask & (MEAN | EXCEED):
        with np.errstate(all="ignore"):
            hs = 4.0 * np.sqrt(e)
        if mask & MEAN:
            with np.errstate(all="ignore"):
                for name, x in (("sum_e", e), ("sum_mx", mx), ("sum_my", my), ("sum_hs", hs)):
                    acc[name][w] = acc[name][w] + x[w]
        if mask & EXCEED:
            for k, thr in enumerate(thresholds):
                hit = w.copy()
                hit[w] = hs[w] >= thr
                acc["n_exc"][..., k][hit] += np.uint32(1)
    if acc["n_samples"] == 0:
        acc["t_first"] = float(clock)
    acc["t_last"] = float(clock)
    acc["n_samples"] += 1
    return acc


def accumulate(samples, mask, thresholds=(), acc=None):
    """the accumulators after the (State, clock) samples in order, from zero or from `acc` (not modified)"""
    samples = list(samples)
    if acc is None:
        acc = zeros(np.asarray(samples[0][0]).shape[:-1], mask, thresholds)
    else:
        acc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in acc.items()}
    for S, clock in samples:
        update(acc, S, clock, mask, thresholds)
    return acc


def plane_names(mask):
    return (PEAK_PLANES if mask & PEAK else ()) + (MEAN_PLANES if mask & MEAN else ()) + ("n_wet",) + (("n_exc",) if mask & EXCEED else ())


def assert_equal(got, want, mask, what):
    """every plane bitwise (tobytes) and the three scalars"""
    for name in plane_names(mask):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint64 if a.dtype == np.float64 else np.uint32) != b.view(np.uint64 if a.dtype == np.float64 else np.uint32))
            k = tuple(bad[0])
            raise AssertionError(f"{what}: plane {name} differs at {len(bad)} of {a.size} entries; first at {k}: {a[k]!r} != {b[k]!r}")
    for name in ("n_samples", "t_first", "t_last"):
        assert got[name] == want[name], (what, name, got[name], want[name])
