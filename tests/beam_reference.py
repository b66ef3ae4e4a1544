"""Finite-beam rendering restated in numpy (no call into the package): the footprint pattern, the sub-rays of a beam and the
reduction of a bundle of sub-ray returns to one return.  Definitions: include/dc_hip.h, DESIGN "Finite-beam rendering"."""
import math

import numpy as np

MEAN, QUANTILE = 0, 1
EPS = 2.0 ** -52


def pattern(n_samples, rho_max=1.5):
    """[S,3] rows (px, py, weight): equal-power samples of a Gaussian truncated at rho_max, on a Vogel spiral."""
    out = np.empty((n_samples, 3))
    for j in range(n_samples):
        u = j / n_samples
        rho = math.sqrt(-0.5 * math.log1p(-u * (1.0 - math.exp(-2.0 * rho_max * rho_max))))
        phi = j * (math.pi * (3.0 - math.sqrt(5.0)))
        out[j] = rho * math.cos(phi), rho * math.sin(phi), 1.0
    return out


def frame(s):
    """(d, e1, e2) of the direction s, or None for a direction that is zero or not finite."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(all='ignore'):
        d = s / np.sqrt(s @ s)
    if not np.isfinite(d).all():
        return None
    k = int(np.argmin(np.abs(d)))                   # the first of equal minima
    a = np.zeros(3)
    a[k] = 1.0
    c = np.cross(a, d)
    e1 = c / np.sqrt(c @ c)
    return d, e1, np.cross(d, e1)


def subrays(vps, dirs, pat, r0, spread):
    """origins [n,S,3], directions [n,S,3] (not normalised) of the beams (vps, dirs) [n,3]; NaN for a beam without a frame."""
    vps, dirs = np.asarray(vps, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    n, S = len(dirs), len(pat)
    o, D = np.full((n, S, 3), np.nan), np.full((n, S, 3), np.nan)
    for i in range(n):
        fr = frame(dirs[i])
        if fr is None:
            continue
        d, e1, e2 = fr
        q = pat[:, :1] * e1[None] + pat[:, 1:2] * e2[None]
        o[i] = vps[i][None] + r0 * q
        D[i] = d[None] + spread * q
    return o, D


def reduce(sub_face, sub_t, sub_w, detection, tau, min_hits):
    """(face [n], depth [n], n_hits [n]) of the bundles sub_* [n,S]."""
    sub_face, sub_t, sub_w = np.asarray(sub_face), np.asarray(sub_t, dtype=np.float64), np.asarray(sub_w, dtype=np.float64)
    n, S = sub_face.shape
    face, depth, n_hits = np.full(n, -1, dtype=np.int32), np.full(n, np.inf), np.zeros(n, dtype=np.int32)
    for i in range(n):
        H = np.flatnonzero((sub_face[i] >= 0) & np.isfinite(sub_w[i]))
        n_hits[i] = len(H)
        if len(H) < min_hits or len(H) == 0:
            continue
        t, w = sub_t[i, H], sub_w[i, H]
        if detection == MEAN:
            sw = swt = 0.0
            for a in range(len(H)):
                sw += w[a]
                swt += w[a] * t[a]
            if not sw > 0.0:
                continue
            d = swt / sw
        else:
            order = np.lexsort((H, t))
            c = np.cumsum(w[order])
            if not c[-1] > 0.0:
                continue
            d = t[order][np.flatnonzero(c >= tau * c[-1])[0]]
        dist = np.abs(t - d)
        face[i] = sub_face[i, H[int(np.argmin(dist))]]          # the first of equal minima: the lower j
        depth[i] = d
    return face, depth, n_hits


def soup(seed, n_faces, extent, scale):
    """A triangle soup (the construction of test_gpu_bias._soup): verts f64 [3F,3], faces i32 [F,3], and the generator, to go on with."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-extent, extent, size=(n_faces, 1, 3))
    verts = (centres + rng.normal(scale=scale, size=(n_faces, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3), rng
