"""The exact reference of the ICP-loss tests: what csrc/dc_icp.hip computes -- the point-to-plane and point-to-point pair sums, the
sequence sums, the pose-correction chain and its adjoint, the Adam update, one whole finishing step of a pose-training iteration and
the joining of several sequences' sums -- restated correspondence by correspondence in mpmath (200 bits).  Host only, no torch.

Every quantity is a pair (value, magnitude).  The value is the exact result.  The magnitude is the same expression with every
addend replaced by its absolute value at every addition (sums of |products|), carried through products, quotients and square roots
to first order: the standard running bound of a forward error analysis, under which a float64 evaluation with at most c roundings
on any path from an exactly represented input to the output is within c 2^-52 magnitude of the value (gamma_c with 2^-53 per
rounding, a factor two to spare).  The bounds of the GPU tests are ``c * U * magnitude`` with the c's derived below; where an output
is a sum over correspondences its magnitude is the sum of the addends' magnitudes.

The float32 cast of the world points (loss.py:436-437) is part of the function: x = R x_l + t is rounded to float32 (nearest even,
from the exact value) and widened; its magnitude starts again at |x| because the kernel's x is then exactly the same number --
unless the exact coordinate lies next to a rounding tie, where a float64 evaluation may land on the other side.  ``scan_world``
reports every such coordinate (within 2^-40 of a tie, relative to the magnitude of the coordinate's sum); the case builders redraw
those points.

Conventions at the singular points, as the kernels': sign(0) = 0, the norm's subgradient at zero is zero, the exponent gradient is
zero where inc <= 0, the cast passes the gradient through unchanged; in the pose chain only the taken branch of the small-angle
switch gets a gradient and d|a|/da = 0 at the origin.

``flaws`` plants one named mistake into a copy of the reference (test_icploss_reference_host: the designed cases must notice it)."""
import math
from collections import Counter

import mpmath
import numpy as np

M = mpmath.MPContext()
M.prec = 200
mpf = M.mpf
U = 2.0 ** -52
MAX_TERMS = 8
KINDS = {None: 0, 'BaseModel': 0, 'Polynomial': 1, 'ScaledPolynomial': 2, 'Linear': 3, 'InvCos': 4, 'ScaledInvCos': 5}
BLOCK = 256                  # correspondences per block row
SEQ_PAIRS = 16               # pairs per launch of the sequence kernels
TIE_REL = 2.0 ** -40

# ---- rounding counts (c of the bounds); one unit = one float64 rounding, a library function (pow, log, cos, sincos) counts two ----
# Longest path of one correspondence, from exactly represented inputs to its addend (scan_point_bwd's exponent gradient of the
# polynomial kinds): n = R n_l 3, |n| 4 (two adds, a product, the root), s na n - s nb n 3, R^T g 3, dir . (R^T g) 3, -d gd 1,
# base w pk log(inc) 3 + 2 (log) with pk = pow() in parallel (2, or 4 products of the fast path), the two += of sides A and B 2:
# 24.  The world point never adds to it: its own path (model 15, x_l 2, R x_l + t 4 = 21) ends at the cast, after which the value is
# exact again; x_l itself enters dT through one product and two additions (17 + 3 = 20 < 24).
C_TERM = 24
C_BLOCK = 8                  # icp_block_sums: six butterfly steps, two joins of the four wavefronts


def c_sums(rows, n_pairs=1):
    """c of a pair's or a sequence's sums: the addend, the block, the rows of a pair (a thread of the reduction adds at most
    ceil(rows / 6) rows one after the other in the fused kernel, ceil(rows / 256) in the others, then 6 phases or 6 + 2 butterfly
    and wavefront joins: at most ceil(rows / 6) + 8), the pair's weight and the two directed sums 2, one addition per pair."""
    return C_TERM + C_BLOCK + (-(-int(rows) // 6) + 8) + 2 + int(n_pairs)


# pose chain forward: |a| 4, sincos 2, k 2, q = a k 1, s = 2 / |q|^2 5, an entry of R 4, T = T0 X 3: 21
C_CHAIN_FWD = 24
# its adjoint: q 10, T0^T G 4, the nine-fold accumulation into ds 3 + 9, dn 2, dq += 2, a . dq 3, dtheta 4, g 3 = 40, the block sum of
# a shared correction 8 + ceil(S / 256)
C_CHAIN_BWD = 56
# the finishing step: the adjoint with the gradient scale 41 + shared sum 11, Adam 12 (lerp 3, v 4, root and bias 3, quotient and
# step 3 -- pow() of the bias terms enters through the magnitudes), then the forward chain on the updated correction 21: 96
C_FINISH = 96


class V(object):
    """value and running magnitude"""
    __slots__ = ('v', 'm')

    def __init__(self, v, m=None):
        self.v = v if isinstance(v, M.mpf) else mpf(v)
        self.m = abs(self.v) if m is None else m

    def __add__(a, b):
        b = _v(b)
        return V(a.v + b.v, a.m + b.m)
    __radd__ = __add__

    def __sub__(a, b):
        b = _v(b)
        return V(a.v - b.v, a.m + b.m)

    def __rsub__(a, b):
        return _v(b) - a

    def __neg__(a):
        return V(-a.v, a.m)

    def __mul__(a, b):
        b = _v(b)
        return V(a.v * b.v, a.m * b.m)
    __rmul__ = __mul__

    def __truediv__(a, b):
        b = _v(b)
        return V(a.v / b.v, a.m / abs(b.v) + abs(a.v) * (b.m - abs(b.v)) / (b.v * b.v))

    def __rtruediv__(a, b):
        return _v(b) / a


def _v(x):
    return x if isinstance(x, V) else V(mpf(float(x)) if not isinstance(x, M.mpf) else x)


ZERO = V(mpf(0))


def vabs(a):
    return V(abs(a.v), a.m)


def vsqrt(a):
    if a.v == 0:
        return V(mpf(0), M.sqrt(a.m))
    s = M.sqrt(a.v)
    return V(s, s + (a.m - a.v) / (2 * s))


def vsin(a):
    s, c = M.sin(a.v), M.cos(a.v)
    return V(s, 2 * abs(s) + abs(c) * (a.m - abs(a.v)))


def vcos(a):
    s, c = M.sin(a.v), M.cos(a.v)
    return V(c, 2 * abs(c) + abs(s) * (a.m - abs(a.v)))


def sign(x, flaws=()):
    if x > 0:
        return 1
    if x < 0:
        return -1
    return 1 if 'sign0_is_1' in flaws else 0


def exact(x):
    return V(mpf(float(x)))


def round_f32(x):
    """x (mpf) rounded to the nearest float32, ties to even, as an mpf"""
    return M.make_mpf(mpmath.libmp.mpf_pos(x._mpf_, 24, 'n'))


def near_tie(x, scale):
    """|x| within TIE_REL * scale of the midpoint of two neighbouring float32 numbers"""
    if x == 0:
        return False
    _, ex = M.frexp(abs(x))                         # |x| = mant 2^ex, mant in [0.5, 1)
    ulp = M.ldexp(mpf(1), ex - 24)
    frac = abs(x) / ulp
    frac = frac - M.floor(frac)
    return abs(frac - mpf(0.5)) * ulp < TIE_REL * scale


# ---- the depth model (dc_pointmath.h) ---------------------------------------------------------------------------------------------
def pow_term(inc, e):
    ev = float(e.v)
    if ev == int(ev) and 0 <= int(ev) <= 8:
        r = V(mpf(1))
        for _ in range(int(ev)):
            r = r * inc
        return r
    p = M.power(inc.v, e.v)
    return V(p, 2 * abs(p))


def model_depth(kind, w, e, d, inc, lm):
    if kind == 0 or not lm:
        return d
    if kind == 3:
        return w[0] * d + w[1] * inc + w[2]
    if kind == 4:
        return d - w[0] / vcos(inc)
    if kind == 5:
        return d * (1 - w[0] / vabs(vcos(inc)))
    b = ZERO
    for k in range(len(w)):
        b = b + pow_term(inc, e[k]) * w[k]
    return d * (1 - b) if kind == 2 else d - b


def model_dw_other(kind, k, d, inc):
    if kind == 3:
        return d if k == 0 else (inc if k == 1 else V(mpf(1)))
    if kind == 4:
        return -(1 / vcos(inc))
    return -(d / vabs(vcos(inc)))


def as_model(model):
    """(kind name or code, w, e) -> (code, [V] w, [V] e); None or kind 0: no model"""
    if model is None:
        return 0, [], []
    kind, w, e = model
    kind = KINDS[kind] if not isinstance(kind, int) else kind
    if kind == 0:
        return 0, [], []
    return kind, [exact(x) for x in w], [exact(x) for x in e]


# ---- scan points ------------------------------------------------------------------------------------------------------------------
class Point(object):
    __slots__ = ('xl', 'dr', 'nl', 'x', 'n', 'd', 'inc', 'lm', 'ties')


def scan_point(scan, i, model, pose, flaws=()):
    """Point i of scan = dict(vps [n,3] | None, dirs [n,3], depth [n], inc [n] | None, lmask bool [n] | None, normals [n,3] | None)
    under model = as_model(...) and pose = 12 floats (row-major [R|t])."""
    kind, w, e = model
    row = lambda a: [exact(a[i][q]) for q in range(3)]
    p = Point()
    vp = row(scan['vps']) if scan.get('vps') is not None else [ZERO, ZERO, ZERO]
    p.dr = row(scan['dirs'])
    p.nl = row(scan['normals']) if scan.get('normals') is not None else [ZERO, ZERO, ZERO]
    p.d = exact(scan['depth'][i])
    p.lm = True if scan.get('lmask') is None or 'ignore_lmask' in flaws else bool(scan['lmask'][i])
    p.inc = exact(scan['inc'][i]) if (kind != 0 and p.lm) else ZERO
    dc = model_depth(kind, w, e, p.d, p.inc, p.lm)
    p.xl = [vp[a] + dc * p.dr[a] for a in range(3)]
    T = [exact(q) for q in pose]
    p.x, p.n, p.ties = [], [], []
    for r in range(3):
        xe = T[4 * r] * p.xl[0] + T[4 * r + 1] * p.xl[1] + T[4 * r + 2] * p.xl[2] + T[4 * r + 3]
        if 'no_cast' in flaws:
            p.x.append(xe)
        else:
            if near_tie(xe.v, xe.m):
                p.ties.append(r)
            p.x.append(V(round_f32(xe.v)))
        p.n.append(T[4 * r] * p.nl[0] + T[4 * r + 1] * p.nl[1] + T[4 * r + 2] * p.nl[2])
    return p


def scan_world(scan, model, pose):
    """-> (x float64 [n,3]: the float32 world points, ties: sorted indices of the points with a coordinate next to a rounding tie)"""
    mdl = as_model(model)
    n = len(scan['depth'])
    x, ties = np.zeros((n, 3)), []
    for i in range(n):
        p = scan_point(scan, i, mdl, pose)
        x[i] = [float(c.v) for c in p.x]
        if p.ties:
            ties.append(i)
    return x, ties


def scan_point_bwd(model, pose, p, gx, gn, flaws=()):
    """-> (gw [P], ge [P], gT [12]) of one scan point from dL/dx and dL/dn (world frame)"""
    kind, w, e = model
    T = [exact(q) for q in pose]
    rg = [T[c] * gx[0] + T[4 + c] * gx[1] + T[8 + c] * gx[2] for c in range(3)]
    gd = p.dr[0] * rg[0] + p.dr[1] * rg[1] + p.dr[2] * rg[2]
    P = len(w)
    gw, ge = [ZERO] * P, [ZERO] * P
    if kind > 2 and p.lm:
        for k in range(min(P, 3)):
            gw[k] = gd * model_dw_other(kind, k, p.d, p.inc)
    elif kind != 0 and p.lm:
        base = -(p.d * gd) if kind == 2 else -gd
        for k in range(P):
            pk = pow_term(p.inc, e[k])
            gw[k] = base * pk
            if p.inc.v > 0:
                lg = M.log(p.inc.v)
                ge[k] = base * w[k] * pk * V(lg, 2 * abs(lg))
            elif 'egrad_at_inc0' in flaws:
                ge[k] = -(base * w[k])
    gT = [ZERO] * 12
    for r in range(3):
        for c in range(3):
            gT[4 * r + c] = gx[r] * p.xl[c] + gn[r] * p.nl[c]
        gT[4 * r + 3] = gx[r]
    return gw, ge, gT


def pair_addend(a, b, model, pose_a, pose_b, plane, flaws=()):
    """One correspondence -> [t12, t21, gw [P], ge [P], gTa [12], gTb [12]] as V's"""
    dx = [b.x[q] - a.x[q] for q in range(3)]
    if 'no_cast' not in flaws:
        dx = [V(d.v) for d in dx]                   # a difference of two float32 numbers is exact in float64
    if plane:
        k12 = a.n[0] * dx[0] + a.n[1] * dx[1] + a.n[2] * dx[2]
        na = vsqrt(a.n[0] * a.n[0] + a.n[1] * a.n[1] + a.n[2] * a.n[2])
        k21 = -(b.n[0] * dx[0] + b.n[1] * dx[1] + b.n[2] * dx[2])
        nb = vsqrt(b.n[0] * b.n[0] + b.n[1] * b.n[1] + b.n[2] * b.n[2])
        if 'drop_norm' in flaws:
            t12, t21 = vabs(k12), vabs(k21)
        else:
            t12, t21 = vabs(k12) * na, vabs(k21) * nb
        s12, s21 = sign(k12.v, flaws), sign(k21.v, flaws)
        gxa, gxb, gna, gnb = [], [], [], []
        for q in range(3):
            t = s12 * (na * a.n[q]) - s21 * (nb * b.n[q])
            gxb.append(t)
            gxa.append(-t)
            gna.append(s12 * (na * dx[q]) + (vabs(k12) * a.n[q] / na if na.v > 0 else ZERO))
            gnb.append(-(s21 * (nb * dx[q])) + (vabs(k21) * b.n[q] / nb if nb.v > 0 else ZERO))
    else:
        ln = vsqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])
        t12, t21 = ln, ZERO
        gxb = [dx[q] / ln if ln.v > 0 else ZERO for q in range(3)]
        gxa = [-g for g in gxb]
        gna = gnb = [ZERO, ZERO, ZERO]
    gwa, gea, gTa = scan_point_bwd(model, pose_a, a, gxa, gna, flaws)
    gwb, geb, gTb = scan_point_bwd(model, pose_b, b, gxb, gnb, flaws)
    return [t12, t21] + [x + y for x, y in zip(gwa, gwb)] + [x + y for x, y in zip(gea, geb)] + gTa + gTb


def pair_sums(scan_a, scan_b, pose_a, pose_b, model, idx_a, idx_b, plane=True, flaws=()):
    """The pair layout {sum12, sum21, dw [P], de [P], dTa [12], dTb [12]} -> (value, magnitude) as mpf lists, and the set of
    (side, point) with a coordinate next to a float32 tie.  Equal correspondences are evaluated once and counted."""
    mdl = as_model(model)
    n_out = 26 + 2 * len(mdl[1])
    idx_a, idx_b = np.asarray(idx_a).tolist(), np.asarray(idx_b).tolist()
    if 'omit_row' in flaws and len(idx_a) > 256 * BLOCK:      # row 256 of a 257-row sum
        idx_a, idx_b = idx_a[:256 * BLOCK], idx_b[:256 * BLOCK]
    val, mag, ties = [mpf(0)] * n_out, [mpf(0)] * n_out, set()
    pa, pb = {}, {}
    for (ia, ib), cnt in sorted(Counter(zip(idx_a, idx_b)).items()):
        if ia not in pa:
            pa[ia] = scan_point(scan_a, ia, mdl, pose_a, flaws)
            if pa[ia].ties:
                ties.add((0, ia))
        if ib not in pb:
            pb[ib] = scan_point(scan_b, ib, mdl, pose_b, flaws)
            if pb[ib].ties:
                ties.add((1, ib))
        add = pair_addend(pa[ia], pb[ib], mdl, pose_a, pose_b, plane, flaws)
        for q in range(n_out):
            val[q] = val[q] + cnt * add[q].v
            mag[q] = mag[q] + cnt * add[q].m
    return val, mag, ties


def _f(xs):
    return np.array([float(x) for x in xs], dtype=np.float64)


def pair(scan_a, scan_b, pose_a, pose_b, model, idx_a, idx_b, plane=True, flaws=()):
    """pair_sums as float64 arrays (value rounded once, magnitude) and the tie set"""
    val, mag, ties = pair_sums(scan_a, scan_b, pose_a, pose_b, model, idx_a, idx_b, plane, flaws)
    return _f(val), _f(mag), ties


def sequence(scans, pairs, poses, model, plane=True, flaws=()):
    """The sequence layout {loss, dw [P], de [P], d[R|t] [S,12]}: pairs = [(scan_a, scan_b, idx_a, idx_b, weight)], poses [S][12].
    -> (value, magnitude) float64 [1 + 2P + 12 S], ties = set of (scan, point)."""
    mdl = as_model(model)
    P, S = len(mdl[1]), len(scans)
    n_out = 1 + 2 * P + 12 * S
    val, mag, ties = [mpf(0)] * n_out, [mpf(0)] * n_out, set()
    cache = {}
    for ip, (sa, sb, ia, ib, wt) in enumerate(pairs):
        if len(ia) == 0:
            continue
        key = (sa, sb, np.asarray(ia).tobytes(), np.asarray(ib).tobytes())
        if key not in cache:
            cache[key] = pair_sums(scans[sa], scans[sb], poses[sa], poses[sb], model, ia, ib, plane, flaws)
        v, m, tz = cache[key]
        ties |= set((sa if side == 0 else sb, i) for side, i in tz)
        wt = mpf(float(wt))
        dst_a = sa if not ('wrong_slot' in flaws and ip == 16) else (sa + 1) % S
        val[0] += wt * (v[0] + v[1])
        mag[0] += abs(wt) * (m[0] + m[1])
        for k in range(2 * P):
            val[1 + k] += wt * v[2 + k]
            mag[1 + k] += abs(wt) * m[2 + k]
        for j in range(12):
            val[1 + 2 * P + 12 * dst_a + j] += wt * v[2 + 2 * P + j]
            mag[1 + 2 * P + 12 * dst_a + j] += abs(wt) * m[2 + 2 * P + j]
            val[1 + 2 * P + 12 * sb + j] += wt * v[14 + 2 * P + j]
            mag[1 + 2 * P + 12 * sb + j] += abs(wt) * m[14 + 2 * P + j]
    return _f(val), _f(mag), ties


def sequence_rows(pairs):
    """(largest number of block rows of a pair, number of non-empty pairs): the arguments of c_sums for a sequence"""
    rows = [-(-len(p[2]) // BLOCK) for p in pairs if len(p[2])]
    return (max(rows) if rows else 0), len(rows)


# ---- the pose chain (pose_chain_fwd / pose_chain_bwd) -----------------------------------------------------------------------------
SWITCH = mpf(1e-6)


class Chain(object):
    __slots__ = ('q', 's', 'k', 'theta', 'sh', 'ch', 'small')


def chain_fwd(d6, flaws=()):
    """d6: six V's (xyz, axis-angle) -> (R [9] V's, Chain)"""
    a = d6[3:6]
    c = Chain()
    c.theta = vsqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    c.small = (c.theta.v <= SWITCH) if 'small_at_switch' in flaws else (c.theta.v < SWITCH)
    half = 0.5 * c.theta
    c.sh, c.ch = vsin(half), vcos(half)
    c.k = (0.5 - c.theta * c.theta / 48.0) if c.small else c.sh / c.theta
    c.q = [c.ch, a[0] * c.k, a[1] * c.k, a[2] * c.k]
    r, i, j, k = c.q
    c.s = 2.0 / (r * r + i * i + j * j + k * k)
    s = c.s
    R = [1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
         s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
         s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]
    return R, c


def chain_bwd(d6, c, gR):
    """dL/dR (row major) -> dL/d(axis-angle) [3], the adjoint of chain_fwd operation by operation"""
    r, i, j, k = c.q
    s = c.s
    g = gR
    ds = (-(j * j + k * k) * g[0] + (i * j - k * r) * g[1] + (i * k + j * r) * g[2] + (i * j + k * r) * g[3] - (i * i + k * k) * g[4]
          + (j * k - i * r) * g[5] + (i * k - j * r) * g[6] + (j * k + i * r) * g[7] - (i * i + j * j) * g[8])
    dr = s * (-(k * g[1]) + j * g[2] + k * g[3] - i * g[5] - j * g[6] + i * g[7])
    di = s * (j * g[1] + k * g[2] + j * g[3] - 2.0 * (i * g[4]) - r * g[5] + k * g[6] + r * g[7] - 2.0 * (i * g[8]))
    dj = s * (-2.0 * (j * g[0]) + i * g[1] + r * g[2] + i * g[3] + k * g[5] - r * g[6] + k * g[7] - 2.0 * (j * g[8]))
    dk = s * (-2.0 * (k * g[0]) - r * g[1] + i * g[2] + r * g[3] - 2.0 * (k * g[4]) + j * g[5] + i * g[6] + j * g[7])
    dn = -0.5 * (s * s * ds)
    dr, di, dj, dk = dr + 2.0 * (r * dn), di + 2.0 * (i * dn), dj + 2.0 * (j * dn), dk + 2.0 * (k * dn)
    a = d6[3:6]
    dkk = a[0] * di + a[1] * dj + a[2] * dk
    dtheta = -0.5 * (c.sh * dr)
    if c.small:
        dtheta = dtheta - (c.theta / 24.0) * dkk
    else:
        dtheta = dtheta + (0.5 * c.ch / c.theta - c.sh / (c.theta * c.theta)) * dkk
    out = []
    for q, dq in enumerate((di, dj, dk)):
        out.append(c.k * dq + (a[q] / c.theta * dtheta if c.theta.v > 0 else ZERO))
    return out


def compose(A, R, d6):
    """T = T0 X in full (all four rows of T0): A [16] V's -> [16] V's"""
    o = [ZERO] * 16
    for a in range(4):
        for b in range(3):
            o[4 * a + b] = A[4 * a] * R[b] + A[4 * a + 1] * R[3 + b] + A[4 * a + 2] * R[6 + b]
        o[4 * a + 3] = A[4 * a] * d6[0] + A[4 * a + 1] * d6[1] + A[4 * a + 2] * d6[2] + A[4 * a + 3]
    return o


def _vm(rows):
    return (np.array([[float(x.v) for x in r] for r in rows], dtype=np.float64),
            np.array([[float(x.m) for x in r] for r in rows], dtype=np.float64))


def corrected_poses(T0, deltas, flaws=()):
    """poses [S,16] floats, deltas [S,6] or [1,6] -> (value, magnitude) float64 [S,16]"""
    out = []
    for p in range(len(T0)):
        d6 = [exact(x) for x in deltas[p if len(deltas) != 1 else 0]]
        R, _ = chain_fwd(d6, flaws)
        out.append(compose([exact(x) for x in T0[p]], R, d6))
    return _vm(out)


def pose_grad(A, d6, G, rows, scale=None, flaws=()):
    """dL/d(delta) [6] V's of one pose: A [16], G = dL/dT with `rows` rows (4: corrected_poses; 3: the finishing step), times scale"""
    R, c = chain_fwd(d6, flaws)
    gR, g6 = [ZERO] * 9, [ZERO] * 6
    for a in range(3):
        for b in range(3):
            t = A[a] * G[b]
            for r in range(1, rows):
                t = t + A[4 * r + a] * G[4 * r + b]
            gR[3 * a + b] = t if scale is None else t * scale
        t = A[a] * G[3]
        for r in range(1, rows):
            t = t + A[4 * r + a] * G[4 * r + 3]
        g6[a] = t if scale is None else t * scale
    g6[3:6] = chain_bwd(d6, c, gR)
    return g6


def corrected_poses_bwd(T0, deltas, grad, flaws=()):
    """-> (value, magnitude) float64 [n_deltas, 6]; a shared correction gets the sum over the poses"""
    shared = len(deltas) == 1
    out = [[ZERO] * 6] if shared else []
    for p in range(len(T0)):
        d6 = [exact(x) for x in deltas[0 if shared else p]]
        g6 = pose_grad([exact(x) for x in T0[p]], d6, [exact(x) for x in grad[p]], 4, None, flaws)
        if shared:
            out[0] = [x + y for x, y in zip(out[0], g6)]
        else:
            out.append(g6)
    return _vm(out)


# ---- Adam and the finishing step --------------------------------------------------------------------------------------------------
def adam_one(p0, m, v, g, lr, b1, b2, eps, bias1, bias2_sqrt):
    """torch.optim.Adam's single-tensor update as adam_one of dc_icp.hip states it -> (p, m, v)"""
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = vsqrt(v) / bias2_sqrt + eps
    return p0 + (-(lr / bias1)) * (m / denom), m, v


def _bias(b1, b2, t):
    p1, p2 = M.power(b1.v, t), M.power(b2.v, t)
    return 1 - V(p1, 2 * abs(p1)), vsqrt(1 - V(p2, 2 * abs(p2)))


def finish_step(sums, layout, P, S, w, w_m, w_v, T0, delta, d_m, d_v, zero_first, step, lr_w, lr_d, b1, b2, eps, T_used,
                totals=None, rec_extra=(), sums_mag=None, flaws=()):
    """One dc_pose_train_finish.  sums: floats in layout 0 {sum, count, dw, de, dT [S,12]} or 1 {loss, dw, de, dT}; sums_mag: error
    scale of each entry where the sums are themselves a reference's (then the magnitudes carry it), else they are exact inputs.
    w None: no model; T0, T_used [S][16]; delta, d_m, d_v [n_deltas][6].
    -> dict of (value, magnitude) pairs: w, w_m, w_v [P], delta, d_m, d_v [n_deltas, 6], T_next [S,16], P12_next [S,12]; step; record
    (exact floats: sums, the weights used, the corrections used, T_used [S,12], rec_extra)."""
    head = 2 if layout == 0 else 1
    n_sums = head + 2 * P + 12 * S
    assert len(sums) == n_sums
    sv = [exact(x) for x in sums]
    if sums_mag is not None:
        sv = [V(x.v, max(x.m, mpf(float(mg)))) for x, mg in zip(sv, sums_mag)]
    nd = len(delta)
    record = [float(x) for x in sums] + ([float(x) for x in w] if w is not None else [0.0] * P) + \
        [float(x) for row in delta for x in row] + [float(x) for row in T_used for x in row[:12]] + [float(x) for x in rec_extra]
    if totals is not None:
        scale = 1 / exact(totals[1])
    elif layout == 0:
        scale = 1 / sv[1]
    else:
        scale = None
    t = step + 1
    lr_w_, lr_d_, b1_, b2_, eps_ = exact(lr_w), exact(lr_d), exact(b1), exact(b2), exact(eps)
    bias1, bias2_sqrt = _bias(b1_, b2_, step if 'bias_t' in flaws else t)
    gT = sv[head + 2 * P:]
    grads = []
    for p in range(S):
        d6 = [exact(x) for x in delta[p if nd != 1 else 0]]
        g6 = pose_grad([exact(x) for x in T0[p]], d6, gT[12 * p:12 * p + 12], 3, scale, flaws)
        if zero_first and p == 0 and 'ignore_zero_first' not in flaws:
            g6 = [ZERO] * 6
        grads.append(g6)
    if nd == 1:
        tot = [ZERO] * 6
        for g6 in grads:
            tot = [x + y for x, y in zip(tot, g6)]
        grads = [tot]
    new_d, new_m, new_v = [], [], []
    for p in range(nd):
        rows = [adam_one(exact(delta[p][q]), exact(d_m[p][q]), exact(d_v[p][q]), grads[p][q], lr_d_, b1_, b2_, eps_, bias1, bias2_sqrt)
                for q in range(6)]
        new_d.append([r[0] for r in rows]); new_m.append([r[1] for r in rows]); new_v.append([r[2] for r in rows])
    out = {}
    if w is not None:
        if float(lr_w) != 0.0:
            rows = []
            for k in range(P):
                g = exact(totals[2 + k]) if totals is not None else sv[head + k]
                if scale is not None:
                    g = g * scale
                rows.append(adam_one(exact(w[k]), exact(w_m[k]), exact(w_v[k]), g, lr_w_, b1_, b2_, eps_, bias1, bias2_sqrt))
        else:
            rows = [(exact(w[k]), exact(w_m[k]), exact(w_v[k])) for k in range(P)]
        for q, name in enumerate(('w', 'w_m', 'w_v')):
            val, mag = _vm([[r[q] for r in rows]])
            out[name] = (val[0], mag[0])
    out['delta'], out['d_m'], out['d_v'] = _vm(new_d), _vm(new_m), _vm(new_v)
    nxt = []
    for p in range(S):
        d6 = new_d[p if nd != 1 else 0]
        R, _ = chain_fwd(d6, flaws)
        nxt.append(compose([exact(x) for x in T0[p]], R, d6))
    out['T_next'] = _vm(nxt)
    out['P12_next'] = tuple(a[:, :12].copy() for a in out['T_next'])
    out['step'] = t
    if 'record_after' in flaws:
        record = record[:n_sums] + ([float(x) for x in out['w'][0]] if w is not None else [0.0] * P) + \
            [float(x) for x in out['delta'][0].reshape(-1)] + record[n_sums + P + 6 * nd:]
    out['record'] = np.array(record, dtype=np.float64)
    return out


def combine(outs, layout, P):
    """dc_pose_train_combine: {loss, divisor, dL/dw [P]} over the sequences' sums -> (value, magnitude) float64 [2 + P]"""
    head = 2 if layout == 0 else 1
    val, mag = np.zeros(2 + P), np.zeros(2 + P)
    cols = [[o[0] for o in outs], [o[1] if layout == 0 else 1.0 for o in outs]] + [[o[head + k] for o in outs] for k in range(P)]
    for q, col in enumerate(cols):
        val[q] = math.fsum(float(x) for x in col)
        mag[q] = math.fsum(abs(float(x)) for x in col)
    return val, mag
