"""Cases of the domain distances (tests/golden/domain_distances.npz, made by scripts/make_domain_golden.py from the
reference's own domain_tools/distance.py) and a NumPy statement of the arithmetic, written for this project: the tests
compare it with the fixture bit for bit without a GPU, and the device with the fixture on one.

Windows: populations of N = 4 copies x R = 40 loci (a Gaussian walk; the walk with an isolated NaN locus and a run of 12;
an integer-lattice walk with a duplicated locus: ties, zero distances, v_inter + v_intra == 0), one asymmetric 40 x 40 map
with 5 % NaN, R = 7 (every locus on the edge at wd = 9) and R = 1; window sizes WDS, all five metrics.
Domain distances: N = 3 x R = 150 with NaN loci 10, 71, 100..102 (copy 2 also 70: a domain that is entirely NaN), starts
STARTS (domains of 1 and 2 loci, an inter block of 67 x 64), a lattice walk, an asymmetric NaN-bearing map.
Contacts: the same populations, thresholds 400, an exact lattice distance, a negative one; starts without 0 and with R."""
import numpy as np

WDS = [1, 2, 3, 5, 8, 9, 16]
WINDOW_METRICS = ['median', 'mean', 'ks', 'normed_insulation', 'insulation']
DIST_METRICS = ['median', 'absolute_median', 'insulation']
STARTS = [0, 1, 3, 70, 71, 135]
CONTACT_STARTS = [3, 70, 71, 135, 150]          # without 0, with R
R_WIN, N_WIN, R_DOM, N_DOM = 40, 4, 150, 3
NEIGHBOR_OPTIONS = [(True, 5), (True, 1), (False, 5)]   # (use_local, min_dom_sz)
SINGLE_CALLS = [((5, 5), (10, 20)), ((0, 1), (1, 3)), ((3, 70), (71, 135)), ((20, 60), (40, 90)), ((70, 71), (135, 150))]


def same(a, b):
    """Equal in every bit where neither is NaN (so -0 differs from +0, inf equals inf), NaN where the other has a NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint64)[~na] == b.view(np.uint64)[~nb]).all())


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def _walk(seed, N, R, scale=120.):
    return np.cumsum(np.random.RandomState(seed).randn(N, R, 3) * scale, axis=1)


def _lattice(seed, N, R):
    z = np.cumsum(np.random.RandomState(seed).randint(-1, 2, size=(N, R, 3)) * 100., axis=1)
    z[:, 11] = z[:, 10]          # a duplicated locus: a zero distance
    return z


def _map(seed, R):
    rng = np.random.RandomState(seed)
    m = rng.rand(R, R) * 1000.
    m[rng.rand(R, R) < 0.05] = np.nan
    m[rng.rand(R, R) < 0.02] = 0.
    m[rng.rand(R, R) < 0.01] *= -1.
    np.fill_diagonal(m, 0.)
    return m


def window_populations():
    """name -> (N, R, 3) coordinates."""
    walk = _walk(1, N_WIN, R_WIN)
    holes = walk.copy()
    for n in range(N_WIN):
        holes[n, 5 + n] = np.nan
        holes[n, 20:32] = np.nan
    return {"walk": walk, "holes": holes, "lattice": _lattice(2, N_WIN, R_WIN), "short": _walk(3, 2, 7), "one": _walk(4, 2, 1)}


def window_map():
    return _map(5, R_WIN)


def domain_populations():
    walk = _walk(6, N_DOM, R_DOM)
    for at in (10, 71, 100, 101, 102):
        walk[:, at] = np.nan
    walk[2, 70] = np.nan
    return {"walk": walk, "lattice": _lattice(7, N_DOM, R_DOM)}


def domain_map():
    return _map(8, R_DOM)


def normalization():
    """Symmetric, zero diagonal, positive elsewhere."""
    i = np.arange(R_DOM)
    g = np.abs(i[:, None] - i[None, :]).astype(np.float64)
    noise = np.random.RandomState(9).rand(R_DOM, R_DOM)
    m = 40. * g ** 0.5 + 5. * (noise + noise.T)
    np.fill_diagonal(m, 0.)
    return m


def lattice_thresholds():
    return [400, 100.0, float(np.sqrt(20000.)), -1.0]


# ---- the arithmetic in NumPy ----------------------------------------------------------------------------------------------------

def pair_dist(a, b):
    """scipy's cdist(a, b) for three columns: sqrt((dz*dz + dx*dx) + dy*dy), every operation rounded on its own."""
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def distance_map(zxy):
    """squareform(pdist(zxy)): symmetric, the diagonal the literal 0 (for a NaN locus too)."""
    m = pair_dist(zxy, zxy)
    np.fill_diagonal(m, 0.)
    return m


def _ks(a, b):
    """The two-sided statistic of SciPy 1.15's ks_2samp(a, b) from counts of `<=`; its exact method (samples of up to 10000
    values) rounds the largest difference to a multiple of 1 / lcm(n1, n2)."""
    import math
    both = np.concatenate([a, b])
    ca = (a[None, :] <= both[:, None]).sum(axis=1) / len(a)
    cb = (b[None, :] <= both[:, None]).sum(axis=1) / len(b)
    diff = ca - cb
    d = max(np.clip(-diff.min(), 0, 1), diff.max())
    lcm = (len(a) // math.gcd(len(a), len(b))) * len(b)
    return int(np.round(d * lcm)) * 1.0 / lcm


def np_window(mat, wd, metric):
    """One row of sliding-window distances of a distance map."""
    R = len(mat)
    out = np.zeros(R)
    for i in range(R):
        if i - wd // 2 < 0 or i + wd // 2 >= R:
            continue
        l0, r1 = max(0, i - wd), min(i + wd, R)
        parts = []
        for lo, hi in ((l0, i), (i, r1)):
            blk = mat[lo:hi, lo:hi]
            v = blk[np.triu_indices(hi - lo, 1)]
            parts.append(v[v > 0])                       # NaN > 0 is False
        intra = np.concatenate(parts)
        inter = mat[l0:i, i:r1].ravel()
        inter = inter[~np.isnan(inter)]
        if len(intra) == 0 or len(inter) == 0:
            continue
        with np.errstate(all="ignore"):
            if metric == 'ks':
                out[i] = np.sign(np.median(inter) - np.median(intra)) * _ks(intra, inter)
            elif metric == 'median':
                mi, ma = np.median(inter), np.median(intra)
                di, da = inter - mi, intra - ma
                out[i] = (mi - ma) / np.sqrt(np.median(di * di) + np.median(da * da))
            elif metric == 'mean':
                out[i] = (np.mean(inter) - np.mean(intra)) / np.sqrt(np.var(inter) + np.var(intra))
            elif metric == 'normed_insulation':
                out[i] = (np.mean(intra) - np.mean(inter)) / (np.mean(intra) + np.mean(inter))
            elif metric == 'insulation':
                out[i] = np.mean(inter) / np.mean(intra)
            else:
                raise ValueError(metric)
    return out


def _block(data, rows, cols):
    """Distances [rows, cols] of (R, 3) coordinates (cdist) or of a map."""
    if data.shape[0] != data.shape[1]:
        return pair_dist(data[rows], data[cols])
    return data[rows, cols]


def np_domain_sets(data, b1, b2, norm=None):
    """(inter, intra) distances of the domains [b1[0], b1[1]) and [b2[0], b2[1]), NaN included."""
    s1, s2 = slice(int(b1[0]), int(b1[1])), slice(int(b2[0]), int(b2[1]))
    with np.errstate(all="ignore"):
        intra = []
        for s in (s1, s2):
            blk = _block(data, s, s)
            if norm is not None:
                blk = blk / norm[s, s]
            intra.append(blk[np.triu_indices(len(blk), 1)])
        inter = _block(data, s1, s2)
        if norm is not None:
            inter = inter / norm[s1, s2]
    return inter.ravel(), np.concatenate(intra)


def np_domain_distance(data, b1, b2, metric='median', norm=None, allow_minus=True):
    """The distance of the domains [b1[0], b1[1]) and [b2[0], b2[1]): np.float64, or the integer 0."""
    inter, intra = np_domain_sets(data, b1, b2, norm)
    with np.errstate(all="ignore"):
        if np.isnan(inter).all() or np.isnan(intra).all():
            return 0
        mi, ma = np.nanmedian(inter), np.nanmedian(intra)
        if metric == 'median':
            di, da = inter - mi, intra - ma
            f = (mi - ma) / np.sqrt(np.nanmedian(di * di) + np.nanmedian(da * da))
        elif metric == 'insulation':
            f = mi / ma
        elif metric == 'absolute_median':
            f = mi - ma
        else:
            raise ValueError(metric)
    return f if allow_minus or not 0 > f else 0


def _ends(starts, R):
    return list(starts[1:]) + [R]


def np_domain_pdists(data, starts, metric='median', norm=None, allow_minus=False):
    ends = _ends(starts, len(data))
    return np.array([np_domain_distance(data, (starts[i], ends[i]), (starts[j], ends[j]), metric, norm, allow_minus)
                     for i in range(len(starts)) for j in range(i + 1, len(starts))])


def np_domain_neighboring_dists(data, starts, metric='median', use_local=True, min_dom_sz=5, norm=None, allow_minus=True):
    ends = _ends(starts, len(data))
    out = []
    for i in range(len(starts) - 1):
        s1, e1, s2, e2 = starts[i], ends[i], starts[i + 1], ends[i + 1]
        if use_local:
            s1, e2 = max(s1, e1 - 2 * max(e2 - s2, min_dom_sz)), min(e2, s2 + 2 * max(e1 - s1, min_dom_sz))
        out.append(np_domain_distance(data, (s1, e1), (s2, e2), metric, norm, allow_minus))
    return np.array(out)


def np_contact_freq(data, starts, th=400):
    mat = data if data.shape[0] == data.shape[1] else distance_map(data)
    R = len(mat)
    starts = sorted(set([0] + [int(s) for s in starts]) - {R})
    ends = _ends(starts, R)
    with np.errstate(invalid="ignore"):
        hit = mat <= th
    # entry [i, j] and entry [j, i] are both the share of the block [domain i, domain j] with j <= i
    out = np.zeros([len(starts), len(starts)])
    for i, (si, ei) in enumerate(zip(starts, ends)):
        for j, (sj, ej) in enumerate(zip(starts[:i + 1], ends)):
            out[i, j] = out[j, i] = hit[si:ei, sj:ej].sum() / float((ei - si) * (ej - sj))
    return out


def as_float(results):
    """A list of np.float64 / integer-0 results as (float64 values, int_zero flags)."""
    return (np.array([float(r) for r in results], dtype=np.float64),
            np.array([isinstance(r, (int, np.integer)) for r in results], dtype=bool))


# ---- the calls whose results the fixture holds: key -> thunk(functions) -----------------------------------------------------------

def fixture_calls():
    """(key, f) pairs; f(ns) computes the value of the key from a namespace of functions named like the reference's
    (``_sliding_window_dist``, ``domain_distance``, ``domain_pdists``, ``domain_neighboring_dists``,
    ``_domain_contact_freq``): the reference's module, this harness's NumPy statement (``numpy_namespace``) or the
    package under test."""
    calls = []
    wp, wm = window_populations(), window_map()
    for name, pop in wp.items():
        maps = [distance_map(z) for z in pop]
        for metric in WINDOW_METRICS:
            calls.append(("win_%s_%s" % (name, metric),
                          lambda ns, maps=maps, metric=metric: np.array([[ns._sliding_window_dist(m, wd, metric) for wd in WDS] for m in maps])))
    for metric in WINDOW_METRICS:
        calls.append(("win_map_%s" % metric, lambda ns, metric=metric: np.array([[ns._sliding_window_dist(wm, wd, metric) for wd in WDS]])))
    dp, dm, norm = domain_populations(), domain_map(), normalization()
    sources = [(name, list(pop)) for name, pop in dp.items()] + [("map", [dm])]
    for name, copies in sources:
        for metric in DIST_METRICS:
            for allow in (False, True):
                for nm, nmat in (("raw", None), ("norm", norm)):
                    if name == "lattice" and nm == "norm":
                        continue
                    calls.append(("pd_%s_%s_%d_%s" % (name, metric, allow, nm),
                                  lambda ns, copies=copies, metric=metric, allow=allow, nmat=nmat: np.array(
                                      [ns.domain_pdists(c, STARTS, metric=metric, normalization_mat=nmat, allow_minus_dist=allow)
                                       for c in copies], dtype=np.float64)))
        for use_local, mds in NEIGHBOR_OPTIONS:
            for nm, nmat in (("raw", None), ("norm", norm)):
                calls.append(("nb_%s_%d_%d_%s" % (name, use_local, mds, nm),
                              lambda ns, copies=copies, use_local=use_local, mds=mds, nmat=nmat: np.array(
                                  [ns.domain_neighboring_dists(c, STARTS, use_local=use_local, min_dom_sz=mds, normalization_mat=nmat)
                                   for c in copies], dtype=np.float64)))
        def singles(ns, copies=copies):
            res = [ns.domain_distance(copies[-1], b1, b2, _metric=metric, _allow_minus_distance=allow)
                   for b1, b2 in SINGLE_CALLS for metric in DIST_METRICS for allow in (True, False)]
            return as_float(res)
        calls.append(("dd_%s_values" % name, lambda ns, f=singles: f(ns)[0]))
        calls.append(("dd_%s_intzero" % name, lambda ns, f=singles: f(ns)[1]))
        ths = lattice_thresholds() if name == "lattice" else [400, -1.0]
        for k, th in enumerate(ths):
            for sn, starts in (("a", STARTS), ("b", CONTACT_STARTS)):
                calls.append(("cf_%s_%d_%s" % (name, k, sn),
                              lambda ns, copies=copies, th=th, starts=starts: np.array([ns._domain_contact_freq(c, starts, th) for c in copies])))
    return calls


class numpy_namespace(object):
    """The NumPy statement under the reference's names."""
    @staticmethod
    def _sliding_window_dist(_mat, _wd, _dist_metric='median'):
        return np_window(_mat, _wd, _dist_metric)

    @staticmethod
    def domain_distance(coordinates, _dom1_bds, _dom2_bds, _metric='median', _normalization_mat=None, _allow_minus_distance=True):
        return np_domain_distance(coordinates, _dom1_bds, _dom2_bds, _metric, _normalization_mat, _allow_minus_distance)

    @staticmethod
    def domain_pdists(coordinates, domain_starts, metric='median', normalization_mat=None, allow_minus_dist=False):
        return np_domain_pdists(coordinates, domain_starts, metric, normalization_mat, allow_minus_dist)

    @staticmethod
    def domain_neighboring_dists(coordinates, domain_starts, metric='median', use_local=True, min_dom_sz=5,
                                 normalization_mat=None, allow_minus_dist=True):
        return np_domain_neighboring_dists(coordinates, domain_starts, metric, use_local, min_dom_sz, normalization_mat, allow_minus_dist)

    @staticmethod
    def _domain_contact_freq(_coordinates, _domain_starts, _contact_th=400):
        return np_contact_freq(_coordinates, _domain_starts, _contact_th)


SIGNATURE_NAMES = ["_sliding_window_dist", "domain_distance", "domain_pdists", "domain_neighboring_dists", "_domain_contact_freq"]
