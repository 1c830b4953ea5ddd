"""Inputs and references for the scans of ``biapy_amd.prepost`` at their edges (test infrastructure, pure NumPy; the restated reference
functions are ``oracle/prepost_oracle.py``).

The golden volumes of ``test_prepost_scans`` are positive, continuous and free of ties.  The classes here are what images are made of:

* ``signed``  ``randn * 50``: both branches of the order-preserving float key;
* ``u8``      integers 0..255 as float32: nothing but ties;
* ``two``     values from {0.25, 0.75}: two tie runs, and NOT a binary channel;
* ``zeros``   drawn from {-0.0, +0.0, +-1e-40, +-1}: signed zeros and denormals around the sign change of the key;
* ``extreme`` drawn from {+-FLT_MAX, +-inf, +-FLT_MIN, 0.5}: the ends of the key (order statistics only);
* ``sigmoid`` ``sigmoid(randn * 6)`` in float32, written ``0.5 * (1 + tanh(x / 2))`` so that it saturates to exactly 0 and exactly 1 on both
  sides (``1 / (1 + exp(-x))`` reaches 1 but never 0 in float32) with runs of ties next to both.

Everything is seeded by class and size, computed once per process, cached and handed out read-only."""
import numpy as np

SIZES = (1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025, 4099)
LARGE = 2 ** 24 + 4099          # past the 4096-block cap of the float4 loops (2^24 elements), past float32 integer exactness, an odd tail
CLASSES = ("signed", "u8", "two", "zeros", "extreme", "sigmoid")
QS = (0.1, 1, 5, 33.3, 50, 99, 99.9)
NBINS = (1, 2, 255, 256, 257, 1024, 1025, 4096)
HIST_CLASSES = ("signed", "u8", "sigmoid", "two")
HIST_N = 4099
CONSTANTS = (0.0, 1.0, 0.37, -3.0)
CONSTANT_SHAPE = (5, 7, 9)
ARGMAX_VOXELS = (1, 1025, 70001)
ARGMAX_CK = ((2, 2), (3, 1), (3, 2), (9, 8), (8, 8))
ARGMAX_VALUES = np.array([0, 0.25, 0.5, 1], np.float32)
ARGMAX_P = (0.1, 0.1, 0.2, 0.6)  # P(tied maximum) for two class channels = sum p^2 = 0.42: above the third the CPU test asks for
_F = np.finfo(np.float32)
_POOLS = {
    "two": np.array([0.25, 0.75], np.float32),
    "zeros": np.array([-0.0, 0.0, 1e-40, -1e-40, 1.0, -1.0], np.float32),
    "extreme": np.array([_F.max, -_F.max, np.inf, -np.inf, _F.tiny, -_F.tiny, 0.5], np.float32),
}
_cache = {}


def _ro(a, dtype=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _draw(cls, n):
    rng = np.random.default_rng([CLASSES.index(cls), n])
    if cls == "signed":
        return rng.standard_normal(n, dtype=np.float32) * np.float32(50)
    if cls == "u8":
        return rng.integers(0, 256, size=n).astype(np.float32)
    if cls == "sigmoid":
        z = rng.standard_normal(n, dtype=np.float32) * np.float32(6)
        return np.float32(0.5) * (np.float32(1) + np.tanh(z * np.float32(0.5)))
    return rng.choice(_POOLS[cls], size=n)


def sample(cls, n):
    """The float32 input of class ``cls`` with ``n`` elements (flat)."""
    x = _memo(("x", cls, n), lambda: _ro(_draw(cls, n), np.float32))
    assert x.dtype == np.float32 and x.shape == (n,)
    return x


def sorted_sample(cls, n):
    return _memo(("sorted", cls, n), lambda: _ro(np.sort(sample(cls, n))))


def tie_run(s, k):
    """First and last index of the run of values equal to ``s[k]`` in the sorted array ``s``."""
    return int(np.searchsorted(s, s[k], "left")), int(np.searchsorted(s, s[k], "right")) - 1


def ranks(cls, n):
    """{0, 1, n//3, n//2, n-2, n-1} clipped to the range; for the tied classes the two ends of the tie run that holds n//2 as well."""
    ks = {min(max(k, 0), n - 1) for k in (0, 1, n // 3, n // 2, n - 2, n - 1)}
    if cls in ("u8", "two"):
        ks |= set(tie_run(sorted_sample(cls, n), n // 2))
    return sorted(ks)


def large():
    return sample("signed", LARGE)


def large_order_stats():
    """(ranks, values) of the large input by one ``np.partition``: the plain ranks and the pairs every q of ``QS`` interpolates between."""
    def make():
        n = LARGE
        ks = {0, 1, n // 3, n // 2, n - 2, n - 1}
        for q in QS:
            lo = int(np.floor(np.float32(n - 1) * (np.float32(q) / np.float32(100))))
            ks |= {lo, min(lo + 1, n - 1)}
        ks = sorted(ks)
        part = np.partition(large(), ks)
        return {k: float(part[k]) for k in ks}
    return _memo("large_os", make)


def percentile_ref(cls, n, q):
    return _memo(("pct", cls, n, q), lambda: float(np.percentile(sample(cls, n) if n != LARGE else large(), q)))


def mean_std_ref(x):
    x = np.asarray(x).reshape(-1)
    return float(np.mean(x, dtype=np.float64)), float(np.std(x, dtype=np.float64))


def mean_std_bounds(x):
    """(|mean - ref| allowed, relative std error allowed) - derived in tests/test_prepost_edges_gpu.py::test_mean_std."""
    x = np.asarray(x).reshape(-1)
    n = x.size
    return 2 * n * 2.0 ** -53 * float(np.mean(np.abs(x), dtype=np.float64)), 4 * n * 2.0 ** -53


def znorm_ref(x, mean, std, eps=1e-6):
    """The float32 statement of ``(x - mean) / max(std, eps)``: both scalars rounded to float32 once, then float32 operations."""
    return (x - np.float32(mean)) / np.float32(max(std, eps))


def hist_input(cls, nbins):
    """(x, mn, mx, edges): a class sample plus the float32 edge table ``np.histogram`` builds for its range, plus the neighbours of every edge
    one ulp below and above, clipped to the range (so min and max stay what they were), at a length that is no multiple of 4.  Values ON an
    edge are the only place where the two edge corrections of the bin index matter."""
    def make():
        s = sample(cls, HIST_N)
        mn, mx = s.min(), s.max()
        edges = np.linspace(mn, mx, nbins + 1, endpoint=True, dtype=np.float32)
        x = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)), s])
        x = np.clip(x, mn, mx).astype(np.float32)
        if x.size % 4 == 0:
            x = x[:-1]
        return _ro(x), mn, mx, _ro(edges)
    return _memo(("hist", cls, nbins), make)


def hist_ref(cls, nbins):
    def make():
        x, mn, mx, _ = hist_input(cls, nbins)
        counts, edges = np.histogram(x, bins=nbins, range=(mn, mx))
        return _ro(counts), _ro(edges)
    return _memo(("hist_ref", cls, nbins), make)


def refused_inputs():
    """(name, x, nbins): what ``np.histogram`` refuses - a range that is not finite (a NaN, a +inf in the data) and float32 edges that cannot
    be strictly increasing (max = nextafter(min) at 1025 bins)."""
    base = sample("signed", 1025)
    nan, inf = base.copy(), base.copy()
    nan[512], inf[1024] = np.nan, np.inf
    lo = np.float32(0.37)
    narrow = np.where(sample("two", 1025) == 0.25, lo, np.nextafter(lo, np.float32(1)))
    return [("nan", _ro(nan), 256), ("inf", _ro(inf), 256), ("narrow", _ro(narrow, np.float32), 1025)]


def binary_like():
    """(name, array (1, n), is a binary channel): inputs on either side of the reference's test for a channel of 0 / 1 only."""
    rng = np.random.default_rng(7)
    b = rng.integers(0, 2, size=1025).astype(np.float32)
    def put(v):
        a = b.copy()
        a[511] = v
        return a
    cases = [("binary", b, True), ("all0", np.zeros(7, np.float32), True), ("all1", np.ones(257, np.float32), True),
             ("minus_zero", put(-0.0), True), ("half", put(0.5), False), ("denormal", put(1e-40), False), ("below", put(-1e-40), False),
             ("above", put(np.nextafter(np.float32(1), np.float32(2))), False), ("two", sample("two", 1025), False)]
    return [(name, _ro(a[None], np.float32), flag) for name, a, flag in cases]


def argmax_input(vox, C):
    return _memo(("am", vox, C), lambda: _ro(np.random.default_rng([vox, C]).choice(ARGMAX_VALUES, size=(vox, C), p=ARGMAX_P), np.float32))


def argmax_ref(a, k):
    """The last k channels of (voxels, C) replaced by ONE channel holding np.argmax over them (the first maximum)."""
    C = a.shape[1]
    return np.concatenate([a[:, :C - k], np.argmax(a[:, C - k:], axis=1).astype(np.float32)[:, None]], axis=1)


def tied_share(a, k):
    cls = a[:, a.shape[1] - k:]
    return float(((cls == cls.max(axis=1, keepdims=True)).sum(axis=1) >= 2).mean())
