"""numpy restatement of the range-image rules (DESIGN "Range-image neighbourhoods"), written from their statement:

  pixel rule      depth = |p|, yaw = -atan2(y, x), pitch = asin(z / (depth + 1e-8)), col = floor(0.5 (yaw / pi + 1) W),
                  row = floor((1 - (pitch + |fov_down|) / fov) H), both clamped into the image; clamp = False rejects a row outside
                  the image; a NaN / infinite row and a depth that is not > min_depth are rejected (-1)
  winner rule     the nearest point of a pixel wins, an exact depth tie goes to the lower index
  window slots    dr = -ah..ah outer, dc = -aw..aw inner, rows clip, columns wrap or clip
  membership      occupied and |x_j - x_i|^2 <= r^2 in fp64 (r <= 0 or infinite: no gate); the centre always
  features        fp64 closed form: mean, Bessel covariance with the denominator clamped at 1e-6, eigh, n <- -sign(dir . n) n,
                  inc = arccos |dir . n|
  shadow set      direction neighbours by brute force over all pairs (chord^2 <= r^2, products and sums rounded one by one)
Everything fp64 and slow on purpose.
"""
import numpy as np

MAX_WINDOW = 121


def pixel_coords(points, rows, cols, fov_up, fov_down):
    """(col coordinate, row coordinate) before the floor and the depth, fp64 [n] each."""
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        depth = np.sqrt((x * x + y * y) + z * z)
        up = fov_up / 180.0 * np.pi
        down = fov_down / 180.0 * np.pi
        fov = abs(down) + abs(up)
        yaw = -np.arctan2(y, x)
        pitch = np.arcsin(z / (depth + 1e-8))
        px = 0.5 * (yaw / np.pi + 1.0)
        py = 1.0 - (pitch + abs(down)) / fov
        px = px * cols
        py = py * rows
    return px, py, depth


def pixel_rule(points, rows, cols, fov_up, fov_down, clamp=True, min_depth=0.0):
    """(pixel int32 [n]: r W + c or -1, depth fp64 [n])."""
    p = np.asarray(points, dtype=np.float64)
    px, py, depth = pixel_coords(p, rows, cols, fov_up, fov_down)
    ok = np.isfinite(p).all(axis=1) & (depth > min_depth) & np.isfinite(depth)
    with np.errstate(invalid='ignore'):
        fx, fy = np.floor(px), np.floor(py)
        if not clamp:
            ok &= (fy >= 0) & (fy <= rows - 1)
        fx = np.maximum(0, np.minimum(cols - 1, fx))
        fy = np.maximum(0, np.minimum(rows - 1, fy))
    fx, fy = np.where(ok, fx, 0), np.where(ok, fy, 0)
    pix = fy.astype(np.int64) * cols + fx.astype(np.int64)
    return np.where(ok, pix, -1).astype(np.int32), depth


def near_pixel_edge(points, rows, cols, fov_up, fov_down, band=1e-9):
    """bool [n]: a pixel coordinate of the (finite) point lies within ``band`` of an integer -- where another atan2 / asin may
    floor to the other side."""
    px, py, _ = pixel_coords(points, rows, cols, fov_up, fov_down)
    with np.errstate(invalid='ignore'):
        near = (np.abs(px - np.rint(px)) <= band) | (np.abs(py - np.rint(py)) <= band)
    return near & np.isfinite(px) & np.isfinite(py)


def winners(pixel, depth, n_pixels):
    """(index_image int32 [n_pixels], range_image fp64 [n_pixels]): per pixel the lowest depth, then the lowest index; -1 / -1.0."""
    index_image = np.full(n_pixels, -1, dtype=np.int32)
    range_image = np.full(n_pixels, -1.0)
    for i in range(len(pixel)):
        p = pixel[i]
        if p < 0:
            continue
        if index_image[p] < 0 or depth[i] < range_image[p]:          # (strict: an equal depth leaves the lower index in place)
            index_image[p], range_image[p] = i, depth[i]
    return index_image, range_image


def organize(index_image):
    """(source rows of the survivors in ascending pixel order, their pixels, the index image over the compact rows)."""
    pix = np.nonzero(index_image >= 0)[0]
    compact = np.full_like(index_image, -1)
    compact[pix] = np.arange(len(pix), dtype=np.int32)
    return index_image[pix].astype(np.int64), pix.astype(np.int32), compact


def window_ok(rows, cols, ah, aw):
    return ah >= 0 and aw >= 0 and 2 * ah + 1 <= rows and 2 * aw + 1 <= cols and (2 * ah + 1) * (2 * aw + 1) <= MAX_WINDOW


def window_slots(rows, cols, wrap, r, c, ah, aw):
    """Pixels of the window of (r, c) in window order, -1 outside the image."""
    out = []
    for dr in range(-ah, ah + 1):
        for dc in range(-aw, aw + 1):
            rr, cc = r + dr, c + dc
            if rr < 0 or rr >= rows:
                out.append(-1)
            elif 0 <= cc < cols:
                out.append(rr * cols + cc)
            elif wrap:
                out.append(rr * cols + cc % cols)
            else:
                out.append(-1)
    return np.array(out, dtype=np.int32)


def member(occupied, centre, xi, xj, r):
    if not occupied:
        return False
    if centre or not (r is not None and r > 0.0 and np.isfinite(r)):
        return True
    d = np.asarray(xj, dtype=np.float64) - np.asarray(xi, dtype=np.float64)
    return bool((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= r * r)


def neighbor_table(points, pixel, index_image, rows, cols, wrap, ah, aw, r):
    """Membership table int32 [m, (2 ah + 1)(2 aw + 1)] of an organised cloud, -1 padded in place."""
    x = np.asarray(points, dtype=np.float64)
    k = (2 * ah + 1) * (2 * aw + 1)
    centre = ah * (2 * aw + 1) + aw
    table = np.full((len(x), k), -1, dtype=np.int32)
    for i in range(len(x)):
        slots = window_slots(rows, cols, wrap, int(pixel[i]) // cols, int(pixel[i]) % cols, ah, aw)
        for s, p in enumerate(slots):
            j = index_image[p] if p >= 0 else -1
            if member(j >= 0, s == centre, x[i], x[j] if j >= 0 else x[i], r):
                table[i, s] = j
    return table


def features(points, dirs, table):
    """fp64 closed form on a membership table: dict(nvalid, mean, cov, eigvals, eigvecs, normals, inc_angles)."""
    x = np.asarray(points, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    m = len(x)
    out = dict(nvalid=np.zeros(m, dtype=np.int32), mean=np.zeros((m, 3)), cov=np.zeros((m, 3, 3)), eigvals=np.zeros((m, 3)),
               eigvecs=np.zeros((m, 3, 3)), normals=np.zeros((m, 3)), inc_angles=np.zeros((m, 1)))
    for i in range(m):
        js = table[i][table[i] >= 0]
        w = len(js)
        out['nvalid'][i] = w
        mu = x[js].mean(axis=0)
        c = x[js] - mu
        cov = c.T @ c / max(w - 1.0, 1e-6)
        lam, vec = np.linalg.eigh(cov)
        cosine = float(d[i] @ vec[:, 0])
        out['mean'][i], out['cov'][i], out['eigvals'][i], out['eigvecs'][i] = mu, cov, lam, vec
        out['normals'][i] = -np.sign(cosine) * vec[:, 0]
        out['inc_angles'][i, 0] = np.arccos(min(abs(cosine), 1.0))
    return out


def direction_neighbors(dirs, r):
    """bool [n, n]: chord^2 between the fp64 directions <= r^2 (every pair, the point itself included)."""
    d = np.asarray(dirs, dtype=np.float64)
    diff = d[:, None, :] - d[None, :, :]
    sq = diff * diff
    with np.errstate(invalid='ignore'):
        return (sq[..., 0] + sq[..., 1]) + sq[..., 2] <= r * r


def window_holds(neighbors, pixel, cols, rows, wrap, ah, aw):
    """(every direction neighbour of every point lies in the point's window, the largest |dr| met, the largest |dc| met)."""
    r, c = pixel // cols, pixel % cols
    ii, jj = np.nonzero(neighbors)
    dr = np.abs(r[jj] - r[ii])
    dc = np.abs(c[jj] - c[ii])
    if wrap:
        dc = np.minimum(dc, cols - dc)
    return bool((dr <= ah).all() and (dc <= aw).all()), int(dr.max(initial=0)), int(dc.max(initial=0))


def room_scan(rows, cols, fov_up, fov_down, half=(3.0, 2.0, 1.25), sensor=(0.3, -0.2, 0.1), seed=0, jitter=0.6):
    """One ray per pixel of a spherical grid, jittered inside its bin, intersected with the inside of the box [-half, half]
    (a 6 x 4 x 2.5 m room) seen from ``sensor``.  Returns (points in the SENSOR frame fp64 [H W, 3] in pixel order, wall id
    [H W] = 2 axis + (1 if the + wall), wall normals [6,3])."""
    rng = np.random.default_rng(seed)
    up, down = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = abs(up) + abs(down)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    u = (c + 0.5 + jitter * (rng.random((rows, cols)) - 0.5)) / cols
    v = (r + 0.5 + jitter * (rng.random((rows, cols)) - 0.5)) / rows
    yaw = (2.0 * u - 1.0) * np.pi
    pitch = (1.0 - v) * fov - abs(down)
    d = np.stack([np.cos(pitch) * np.cos(yaw), -np.cos(pitch) * np.sin(yaw), np.sin(pitch)], axis=-1).reshape(-1, 3)
    o = np.asarray(sensor, dtype=np.float64)
    h = np.asarray(half, dtype=np.float64)
    with np.errstate(divide='ignore'):
        t = np.where(d > 0, (h - o) / d, np.where(d < 0, (-h - o) / d, np.inf))
    axis = t.argmin(axis=1)
    tt = t[np.arange(len(d)), axis]
    wall = 2 * axis + (d[np.arange(len(d)), axis] > 0)
    normals = np.zeros((6, 3))
    for a in range(3):
        normals[2 * a, a], normals[2 * a + 1, a] = 1.0, -1.0          # towards the inside
    return d * tt[:, None], wall.astype(np.int32), normals
