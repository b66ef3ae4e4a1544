"""Designed clouds and neighbour tables of the neighbourhood-feature tests (csrc/dc_features.hip: features_fwd_kernel,
features_fwd_tile_kernel, features_grec_kernel, features_bwd_kernel).  Host only: numpy and scipy's cKDTree.

Clouds: rng.uniform(-1, 1, (n, 3)) * [1.0, 0.6, 0.25] + [3.0, -2.0, 1.0], rounded through float32 so that a float32 and a float64
kernel see the same points.  The offset makes the cancellation in x_j - cmean visible in float32.

Tables [n, k] int32, a cKDTree k-NN table (self first in every row; n < k padded with -1) and then edited:

  full       untouched
  ragged     ~20 % of the slots other than slot 0 set to -1, ~30 % of the rows rotated by one slot (self last; some of them with -1
             in slot 0), ~10 % of the rows with a duplicated neighbour
  designed   ragged plus, inside wavefront 0 (centres 0..63): a row that is all -1 (W = 0), a row with self only (W = 1), a row with
             two valid members (W = 2), a row with three (W = 3); one point, the hub, listed in every row that can take it; one
             point listed in no row at all, its own included
  per_wave   wavefront 0 full and self-first in every lane, wavefront 1 with a missing slot in every lane (self first), wavefront 2
             alternating full self-first lanes with rotated lanes that miss slots, the rest ragged
  hub_all    ragged with the hub in EVERY row, in-degree n, whatever it does to the spectra: exempt from the condition below and
             fed g_mean and g_cov only, whose derivatives need no eigenvector (backward tests only)

The gradient tests need every neighbourhood's eigenvectors defined: a row with three or more DISTINCT valid points must have
min(lam1 - lam0, lam2 - lam1) / lam2 >= GAP.  The generator keeps a margin of two (float64 numpy): a ragged row that misses it goes
back to its k-NN row, the hub stays out of a row it would flatten (one far point stretches lam2 and shrinks the relative gap of the
other two), and the centres of the rows that still miss it are drawn again until none does.  test_features_reference_host.py asserts the
condition itself, on the exact spectrum."""
import functools

import numpy as np

EXTENT = np.array([1.0, 0.6, 0.25])
OFFSET = np.array([3.0, -2.0, 1.0])
GAP = 1e-3
KINDS = ('full', 'ragged', 'designed', 'per_wave', 'hub_all')
WAVE = 64
# the lanes of wavefront 0 that hold the designed rows
LANE_W0, LANE_W1, LANE_W2, LANE_W3 = 5, 17, 23, 41


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 3)) * EXTENT + OFFSET).astype(np.float32).astype(np.float64)


def dirs_of(n, seed):
    """Unit viewing directions, rounded through float32."""
    rng = np.random.default_rng(1000 + seed)
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def knn_table(x, k):
    from scipy.spatial import cKDTree
    n = len(x)
    tab = np.full((n, k), -1, dtype=np.int32)
    kk = min(k, n)
    idx = np.asarray(cKDTree(x).query(x, k=kk)[1]).reshape(n, kk)
    tab[:, :kk] = idx
    assert np.array_equal(tab[:, 0], np.arange(n))                       # distinct points: every point is its own nearest
    return tab


def row_stats(x, tab):
    """(W [n], distinct valid points per row [n], gap [n]) with gap = min(lam1 - lam0, lam2 - lam1) / lam2 of the row's Bessel
    covariance in float64 (inf where fewer than three distinct points)."""
    valid = tab >= 0
    W = valid.sum(1)
    distinct = np.array([len(set(r[r >= 0].tolist())) for r in tab])
    p = x[np.where(valid, tab, 0)]
    w = valid[..., None].astype(np.float64)
    mean = (w * p).sum(1) / np.maximum(W, 1)[:, None]
    d = (p - mean[:, None]) * w
    cov = np.einsum('nki,nkj->nij', d, d) / np.maximum(W - 1, 1e-6)[:, None, None]
    lam = np.linalg.eigvalsh(cov)
    with np.errstate(divide='ignore', invalid='ignore'):
        gap = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / lam[:, 2]
    return W, distinct, np.where(distinct >= 3, gap, np.inf)


def _ragged(x, base, rng):
    n, k = base.shape
    tab = base.copy()
    miss = rng.random((n, k)) < 0.2
    miss[:, 0] = False
    tab[miss] = -1
    for i in np.flatnonzero(rng.random(n) < 0.1):                        # a duplicated neighbour
        have = np.flatnonzero(tab[i] >= 0)
        if len(have) >= 2 and k >= 3:
            q = int(rng.integers(1, k))
            src = int(rng.choice(have[have != q])) if np.any(have != q) else 0
            tab[i, q] = tab[i, src]
    rot = rng.random(n) < 0.3
    tab[rot] = np.roll(tab[rot], -1, axis=1)
    bad = row_stats(x, tab)[2] < 2 * GAP
    tab[bad] = base[bad]
    return tab


def _put_hub(x, tab, hub, rows, everywhere=False):
    """The hub into the last slot that does not hold the row's own centre, where the row's spectrum stays separated with it (or
    wherever it is missing, with `everywhere`)."""
    n, k = tab.shape
    cand = tab.copy()
    todo = [i for i in rows if hub not in tab[i] and k >= 2]
    for i in todo:
        q = k - 1 if tab[i, k - 1] != i else k - 2
        cand[i, q] = hub
    ok = row_stats(x, cand)[2] >= 2 * GAP
    for i in todo:
        if ok[i] or everywhere:
            tab[i] = cand[i]


def _hub_all(x, base, rng):
    n, k = base.shape
    assert n >= WAVE and k >= 3
    tab = _ragged(x, base, rng)
    hub = int(np.argmin(np.linalg.norm(x - x.mean(0), axis=1)))
    _put_hub(x, tab, hub, range(n), everywhere=True)
    return tab, dict(hub=hub)


def _designed(x, base, rng):
    n, k = base.shape
    assert n >= WAVE and k >= 3
    tab = _ragged(x, base, rng)
    r0, r1, r2, r3 = LANE_W0, LANE_W1, LANE_W2, LANE_W3
    special = (r0, r1, r2, r3)
    centre = np.linalg.norm(x - x.mean(0), axis=1)
    centre[list(special)] = np.inf
    hub = int(np.argmin(centre))
    centre[hub] = np.inf
    orphan = int(np.argmin(centre))
    tab[tab == orphan] = -1                                             # listed nowhere: its own row loses its centre too
    tab[r0] = -1
    tab[r1] = -1
    tab[r1, 0] = r1
    tab[r2] = -1
    tab[r2, :2] = (r2, hub)
    best, pick = -1.0, None
    for c in base[r3, 1:]:                                              # the third member that keeps the triangle widest
        if c < 0 or c in (hub, orphan, r3):
            continue
        row = np.full((1, k), -1, dtype=np.int32)
        row[0, :3] = (r3, hub, c)
        g = row_stats(x, row)[2][0]
        if g > best:
            best, pick = g, int(c)
    assert pick is not None
    tab[r3] = -1
    tab[r3, :3] = (r3, hub, pick)
    _put_hub(x, tab, hub, [i for i in range(n) if i not in special and i != hub])
    return tab, dict(hub=hub, orphan=orphan, rows=special)


def _per_wave(x, base, rng):
    n, k = base.shape
    assert n >= 3 * WAVE and k >= 3
    tab = _ragged(x, base, rng)
    tab[:WAVE] = base[:WAVE]
    w1 = base[WAVE:2 * WAVE].copy()
    w1[np.arange(WAVE), rng.integers(1, k, WAVE)] = -1
    tab[WAVE:2 * WAVE] = w1
    w2 = base[2 * WAVE:3 * WAVE].copy()
    odd = np.arange(1, WAVE, 2)
    w2[odd, rng.integers(1, k, len(odd))] = -1
    w2[odd] = np.roll(w2[odd], -1, axis=1)
    tab[2 * WAVE:3 * WAVE] = w2
    return tab


@functools.lru_cache(maxsize=None)
def make_case(n, k, kind):
    """(points f64 [n, 3], dirs f64 [n, 3], table i32 [n, k], info) of a case; deterministic.  info: the seed and, for 'designed', the
    hub, the orphan and the four designed rows."""
    assert kind in KINDS
    seed = 7919 * n + 101 * k + KINDS.index(kind)
    x = cloud(n, seed)
    redraw = np.random.default_rng(seed + 7)
    table_seed = seed + 1
    for attempt in range(256):
        base = knn_table(x, k)
        rng = np.random.default_rng(table_seed)
        info = dict(seed=seed)
        if n < WAVE or kind == 'full':
            tab = base if kind == 'full' or n < 4 else _ragged(x, base, rng)
        elif kind == 'ragged':
            tab = _ragged(x, base, rng)
        elif kind == 'designed':
            tab, extra = _designed(x, base, rng)
            info.update(extra)
        elif kind == 'hub_all':
            tab, extra = _hub_all(x, base, rng)
            info.update(extra)
        else:
            tab = _per_wave(x, base, rng)
        try:                                    # a draw without, say, a duplicated neighbour is not a case of its kind
            assert_claims(kind, tab, info)
        except AssertionError:
            table_seed += 100003
            continue
        bad = np.zeros(n, dtype=bool) if kind == 'hub_all' else row_stats(x, tab)[2] < 2 * GAP
        if not bad.any():
            for a in (x, tab):
                a.setflags(write=False)
            d = dirs_of(n, seed)
            d.setflags(write=False)
            return x, d, tab, info
        # the centres of the rows that miss the condition are drawn again, from the cloud's own distribution
        x[bad] = (redraw.uniform(-1, 1, (int(bad.sum()), 3)) * EXTENT + OFFSET).astype(np.float32).astype(np.float64)
    raise AssertionError('no seed gives separated spectra for %r' % ((n, k, kind),))


# ---- which wavefront takes which branch of features_fwd_tile_kernel, from the table alone -------------------------------------------
def branches(tab):
    """Per wavefront (64 consecutive centres; the idle lanes of a partial last one repeat its first lane) the outcome of the two
    wave-wide ballots: self_first in 'all' / 'none' / 'mixed' lanes, a missing slot in 'none' / 'all' / 'mixed' lanes.  Returns two
    dicts of counts."""
    sf, am = dict(all=0, none=0, mixed=0), dict(none=0, all=0, mixed=0)
    for s, a in wave_outcomes(tab):
        sf[s] += 1
        am[a] += 1
    return sf, am


def wave_outcomes(tab):
    """[(self_first outcome, any_missing outcome)] per wavefront."""
    out = []
    for i0 in range(0, len(tab), WAVE):
        rows = tab[i0:i0 + WAVE]
        first = rows[:, 0] == np.arange(i0, i0 + len(rows))
        miss = (rows < 0).any(1)
        out.append(('all' if first.all() else ('none' if not first.any() else 'mixed'),
                    'all' if miss.all() else ('none' if not miss.any() else 'mixed')))
    return out


CLAIMS = {'full': (('all',), ('none',)), 'ragged': (('mixed',), ('mixed',)), 'designed': (('mixed',), ('mixed',)),
          'per_wave': (('all', 'mixed'), ('none', 'all', 'mixed')), 'hub_all': (('mixed',), ('mixed',))}


def assert_claims(kind, tab, info=None):
    """Every branch the table's kind claims is populated (clouds of at least one whole wavefront), and the designed rows are what
    they are said to be."""
    n, k = tab.shape
    if n < WAVE - 1:
        return
    sf, am = branches(tab)
    for b in CLAIMS[kind][0]:
        assert sf[b] >= 1, (kind, 'self_first', b, sf)
    for b in CLAIMS[kind][1]:
        assert am[b] >= 1, (kind, 'any_missing', b, am)
    if kind == 'full':
        assert sf['mixed'] == sf['none'] == 0 and am['mixed'] == am['all'] == 0
    if kind == 'per_wave':
        assert wave_outcomes(tab)[:3] == [('all', 'none'), ('all', 'all'), ('mixed', 'mixed')], wave_outcomes(tab)[:3]
    if kind in ('ragged', 'designed', 'per_wave'):
        valid = tab >= 0
        assert (~valid[:, 0]).any() or k < 3                              # a rotated row with -1 in slot 0
        assert any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in tab)      # a duplicated neighbour
    if kind == 'designed':
        W = (tab >= 0).sum(1)
        r0, r1, r2, r3 = info['rows']
        assert max(info['rows']) < WAVE and (W[r0], W[r1], W[r2], W[r3]) == (0, 1, 2, 3)
        assert tab[r1, 0] == r1
        indeg = np.bincount(tab[tab >= 0], minlength=n)
        # the hub: every row but the W = 0 and W = 1 rows, less the rows it would flatten (see the module's docstring; with three
        # slots a row with the far hub is a thin triangle: about a third of them stay without; 'hub_all' is the hub of in-degree n)
        assert indeg[info['hub']] >= 0.5 * n, (indeg[info['hub']], n)
        assert indeg[info['orphan']] == 0
    if kind == 'hub_all':
        assert all(info['hub'] in r for r in tab)                          # in-degree n


# ---- the cases of the GPU tests (test_gpu_features_edge.py); test_features_reference_host.py checks every one of them ----------------
def tables_for(n):
    """The tables a cloud of n points can take: a single centre has one row, [0, -1, ...]; the designed rows need one whole wavefront,
    per_wave three."""
    return ('full',) if n < 4 else ('full', 'ragged') if n < WAVE else ('full', 'ragged', 'designed') if n < 3 * WAVE else KINDS[:4]


def _product(sizes, ks, kinds=KINDS[:4]):
    return [(n, k, kind) for n in sizes for k in ks for kind in tables_for(n) if kind in kinds]


TILED_K, GENERAL_K = (4, 8, 10, 16), (3, 5, 12)
# forward, k compiled into features_fwd_tile_kernel: a single centre, one lane short of a wavefront, a whole one, one lane over, two
# and a lane, and ten wavefronts (577: an uneven last round of the XCD block mapping)
FWD_TILED = _product((1, 63, 64, 65, 129, 577), TILED_K)
# forward, any other k: features_fwd_kernel, blocks of 256
FWD_GENERAL = _product((255, 256, 257, 2305), GENERAL_K)
# backward
BWD = _product((1, 65, 257, 2305), (4, 10, 16, 5), ('full', 'designed'))
ALL_CASES = list(dict.fromkeys(FWD_TILED + FWD_GENERAL + BWD))
# backward through g_mean and g_cov only: a hub of in-degree n (exempt from the gap condition, see the module's docstring)
BWD_HUB = [(65, 4, 'hub_all'), (257, 10, 'hub_all')]
