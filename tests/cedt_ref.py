"""Reference and cases for the CELossDT weight map (pemp_amd/csrc/cedt.hip), all on the CPU in integers / float64.

The reference works on the squared distance k = D^2, an integer: the boundary map in integers, k_ref from scipy's exact
Euclidean distance transform (what oracle/ref_cpu.py and the reference class use), a brute-force transform to check scipy's
answer, and the weight table  tab[k] = float32(exp(-sqrt(k) / sigma^2) + 1).  ``check`` holds a weight map to one float32
ulp of tab[k_ref]: up to ``k_res(sigma)`` neighbouring table entries lie at least 3 ulp apart, so there one ulp pins D^2
itself; beyond it the weight no longer tells neighbouring distances apart, and beyond the cut-off it is exactly 1.0f.

The cases are seeded and built for the launch branches of pemp_cedt_weight_f32 (see ``col_plan``)."""
import functools

import numpy as np

ULP = 2.0 ** -23                 # one float32 ulp in [1, 2): every weight but tab[0] = 2.0 lies there
GEOMETRY_SIGMA = 7.5             # exactly a float32; k_res = 66189 (257 px), the widest zone short of the largest sigma
BRUTE_BUDGET = 2 * 10 ** 7       # brute_k runs where H * W^2 stays below this: every case but the wide rows
_INF = 1 << 20                   # "no boundary pixel in this column" of the brute-force transform


# ------------------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------------------
def boundary(target):
    """core/losses.py:23-41 in integers: mask = (target == 1), s = zero-padded 3x3 box sum,
    boundary = ((min(s, 1) - mask) + (mask - clamp(s - 8, 0, 1))) != 0.   int64 [B,H,W] -> bool [B,H,W]."""
    t = np.asarray(target)
    m = (t == 1).astype(np.int64)
    B, H, W = m.shape
    p = np.zeros((B, H + 2, W + 2), dtype=np.int64)
    p[:, 1:-1, 1:-1] = m
    s = sum(p[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return ((np.minimum(s, 1) - m) + (m - np.clip(s - 8, 0, 1))) != 0


def k_ref(bd):
    """Exact squared distance to the nearest boundary pixel, int64 [B,H,W], from scipy.  An image without any boundary
    pixel comes out as (y + 1)^2 + x^2: scipy's feature transform stays at its initial value; nothing here special-cases it."""
    from scipy.ndimage import distance_transform_edt
    return np.stack([np.rint(distance_transform_edt(~b) ** 2).astype(np.int64) for b in bd])


def col_dist(b):
    """Vertical distance to the nearest boundary pixel of the same column, one image: int64 [H,W], _INF where the column has none."""
    H, W = b.shape
    g = np.full((H, W), _INF, dtype=np.int64)
    d = np.full(W, _INF, dtype=np.int64)
    for y in range(H):
        d = np.where(b[y], 0, np.minimum(d + 1, _INF))
        g[y] = d
    d = np.full(W, _INF, dtype=np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(b[y], 0, np.minimum(d + 1, _INF))
        g[y] = np.minimum(g[y], d)
    return g


def row_min(g):
    """min_j (g(y, j)^2 + (x - j)^2) over every j, one image, int64; an image whose columns are all empty gets (y+1)^2 + x^2."""
    H, W = g.shape
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2
    k = np.empty((H, W), dtype=np.int64)
    step = max(1, (1 << 22) // (W * W))
    for y0 in range(0, H, step):
        k[y0:y0 + step] = (g[y0:y0 + step, None, :] ** 2 + dx2[None]).min(axis=-1)
    if (g >= _INF).all():
        k = (np.arange(1, H + 1, dtype=np.int64) ** 2)[:, None] + (x ** 2)[None, :]
    return k


def brute_k(bd):
    """The same squared distance as k_ref, by brute force on integers: only to check scipy on the small cases."""
    assert bd.shape[1] * bd.shape[2] ** 2 <= BRUTE_BUDGET, bd.shape
    return np.stack([row_min(col_dist(b)) for b in bd])


def weight_of(k, sigma):
    """float32(exp(-sqrt(k) / sigma^2) + 1), evaluated in float64 like the reference class."""
    return (np.exp(-np.sqrt(np.asarray(k, dtype=np.float64)) / sigma ** 2) + 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tab(sigma):
    """The weight of every k up to well past the cut-off (exp(-d / sigma^2) < 2^-24 beyond d = 16.64 sigma^2)."""
    t = weight_of(np.arange(int((17.0 * sigma * sigma + 3.0) ** 2)), sigma)
    assert t[-1] == 1.0
    t.setflags(write=False)
    return t


def k_res(sigma):
    """The first k whose table entry lies less than 3 ulp above the next one: below it a weight within 1 ulp names its k."""
    t = tab(sigma).astype(np.float64)
    return int(np.argmax((t[:-1] - t[1:]) < 3 * ULP))


def k_cut(sigma):
    """The first k from which every weight is exactly 1.0f."""
    return int(np.nonzero(tab(sigma) != 1.0)[0][-1]) + 1


def check(got, target, sigma, k=None):
    """Hold a weight map to the reference.  Every pixel: |got - tab[k_ref]| <= 1 ulp (kernel and reference both evaluate
    the formula in double, one multiplying by 1 / sigma^2, one dividing: results a few double ulps apart round to float32
    values at most one ulp apart).  The cut-off is exact in both directions: got == 1.0f where the reference is 1.0f and
    nowhere else (the entries either side of k_cut lie 1e-6 of 2^-24 away from the rounding tie or more, at every sigma the
    tests use: test_cedt_cpu.py::test_the_cut_off_is_far_from_a_rounding_tie).
    Returns (worst difference in ulps, share of pixels with k_ref < k_res, i.e. held to an exact D^2)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == np.shape(target), (got.dtype, got.shape)
    if k is None:
        k = k_ref(boundary(target))
    ref = weight_of(k, sigma)
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ULP
    worst = float(ulps.max())
    at = np.unravel_index(int(ulps.argmax()), ulps.shape)
    assert worst <= 1.0, f"{worst} ulp at {at}: got {got[at]!r}, reference {ref[at]!r} (k = {k[at]})"
    one = ref == 1.0
    bad = np.argwhere((got == 1.0) != one)
    assert len(bad) == 0, f"cut-off: {len(bad)} pixels, first {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, k = {k[tuple(bad[0])]}"
    return worst, float((k < k_res(sigma)).mean())


# ------------------------------------------------------------------------------------------------------------------
# the strip rule of the column pass
# ------------------------------------------------------------------------------------------------------------------
def col_plan(H):
    """(cols, nseg, hs, lds_bytes) of edt_col_kernel for label images of height H.  This restates the strip rule of
    pemp_cedt_weight_f32 (cedt.hip) and is the ONE place in the tests that does: if the rule changes there, change it here.
    64 columns per block, halved while H x cols bytes + H x cols uint16 exceed 156 KB (never below 2); the strip is cut
    into nseg = 256 / cols row segments of hs = ceil(H / nseg) rows; above 64 KB the launch needs the LDS opt-in."""
    def nbytes(c):
        return ((H * c + 15) & ~15) + 2 * H * c
    cols = 64
    while cols > 2 and nbytes(cols) > 156 * 1024:
        cols >>= 1
    nseg = 256 // cols
    return cols, nseg, -(-H // nseg), nbytes(cols)


def empty_segments(b):
    """The (segment, column) pairs of a boundary image at which a whole segment of hs rows holds no boundary pixel while
    its two neighbour segments both hold one: there the distances come from the carry into the segment alone, from above
    and from below."""
    H = b.shape[0]
    _, nseg, hs, _ = col_plan(H)
    occ = np.stack([b[s * hs:(s + 1) * hs].any(axis=0) for s in range(nseg) if s * hs < H])
    full = np.array([min((s + 1) * hs, H) - s * hs == hs for s in range(occ.shape[0])])
    mid = occ[:-2] & ~occ[1:-1] & occ[2:] & full[1:-1, None]
    return [(int(s) + 1, int(c)) for s, c in np.argwhere(mid)]


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
def _blob(t, rng, y, x):
    """An isolated foreground pixel (a 3x3 boundary block) or a filled rectangle with its top-left corner at (y, x)."""
    H, W = t.shape
    if rng.rand() < 0.5:
        t[y, x] = 1
    else:
        t[y:min(y + rng.randint(2, 9), H), x:min(x + rng.randint(2, 13), W)] = 1


def _sprinkle(t, rng, p=0.03):
    """Label 255 (ignored) on some background pixels: background for the boundary."""
    t[(t == 0) & (rng.rand(*t.shape) < p)] = 255


def tall_case(H, W, seed, B=2):
    """Blobs down the image with row gaps of 60..200, a rectangle in an image corner, and one segment of the column pass
    left empty between two isolated pixels that sit in the last rows of the segment above and the first rows of the one below."""
    rng = np.random.RandomState(seed)
    _, nseg, hs, _ = col_plan(H)
    t = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        free = [s for s in range(1, nseg - 1) if (s + 1) * hs + 2 < H]
        s = free[rng.randint(len(free))]
        lo, hi = s * hs, (s + 1) * hs
        xp = rng.randint(W)
        t[b, lo - 2, xp] = t[b, hi + 1, xp] = 1
        y = rng.randint(0, 60)
        while y < H:
            if y + 8 < lo - 3 or y > hi + 3:
                _blob(t[b], rng, y, rng.randint(W))
            y += rng.randint(60, 201)
        if b % 2 == 0:
            t[b, :5, :3] = 1
        else:
            t[b, :4, W - 2:] = 1
        _sprinkle(t[b], rng)
    return t


def _mixed(H, W, rng):
    t = np.zeros((H, W), dtype=np.int64)
    if max(H, W) < 20:
        t[rng.rand(H, W) < 0.35] = 1
        return t
    tt = t if W >= H else t.T                      # blobs along the long axis, gaps of 40..150
    p = rng.randint(0, 40)
    while p < tt.shape[1]:
        tt[rng.randint(tt.shape[0]), p:p + rng.randint(1, 7)] = 1
        p += rng.randint(40, 151)
    return t


def tiny_case(H, W, seed):
    """All foreground, a mixed image, and a second one: for the smallest images the complement of the first."""
    rng = np.random.RandomState(seed)
    a = _mixed(H, W, rng)
    b = 1 - a if max(H, W) < 20 else _mixed(H, W, rng)
    t = np.stack([np.ones((H, W), dtype=np.int64), a, b])
    _sprinkle(t[1], rng, 0.2)
    return t


def seam_case(W, seed, H=5):
    """Foreground at columns 252..256 and 506..510, either side of the 254-pixel pieces of boundary_kernel: a run on one
    row, isolated pixels on the outer rows, and a filled block with an eroded interior."""
    rng = np.random.RandomState(seed)
    t = np.zeros((3, H, W), dtype=np.int64)
    for x0 in (252, 506):
        xs = [x for x in range(x0, x0 + 5) if x < W]
        for x in xs:
            t[0, 2, x] = 1
            t[1, (0, H - 1)[(x - x0) % 2], x] = (x - x0) % 3 != 1
            t[2, :, x] = 1
    for b in range(3):
        _sprinkle(t[b], rng)
    return t


def wide_case(H, W, seed):
    """One image, a blob every 150..400 columns and one in the last column."""
    rng = np.random.RandomState(seed)
    t = np.zeros((1, H, W), dtype=np.int64)
    x = rng.randint(0, 100)
    while x < W:
        _blob(t[0], rng, rng.randint(H), x)
        x += rng.randint(150, 401)
    t[0, rng.randint(H), W - 1] = 1
    _sprinkle(t[0], rng)
    return t


def left_blob(H, W):
    """A single isolated foreground pixel at the left end: distances run up to W - 2."""
    t = np.zeros((1, H, W), dtype=np.int64)
    t[0, H // 2, 0] = 1
    return t


def mixed_batch(seed=5, H=40, W=57):
    """An image without any boundary, one with only the image-border ring, and a blob image."""
    rng = np.random.RandomState(seed)
    t = np.zeros((3, H, W), dtype=np.int64)
    t[1] = 1
    for _ in range(4):
        _blob(t[2], rng, rng.randint(H), rng.randint(W))
    _sprinkle(t[2], rng)
    return t


def existing_97():
    """The 2 x 97 x 97 target of the tests that were here before (two synthetic query masks, one with an ignored corner)."""
    from tests.golden.cases import cedt_cases
    return cedt_cases()[0][0].numpy()


TALL_H = (341, 342, 401, 832, 833, 1664, 1665, 3329, 6657, 13313, 16384)
TINY_HW = ((1, 1), (1, 9), (2, 3), (3, 300), (300, 1))
SEAM_W = (253, 254, 255, 256, 508, 509)
WIDE_HW = ((3, 4096), (3, 4097), (2, 16384))
SIGMAS = (0.5, 1.0, 5.0, 7.8)


def _tall_cases():
    out = {}
    for H in TALL_H:
        for W in ((5, 70) if H <= 1665 else (5,)):
            for seed in ((1, 2) if H in (833, 16384) else (1,)):
                out[f"tall-{H}x{W}-s{seed}"] = functools.partial(tall_case, H, W, 1000 * seed + H + W)
    return out


#: name -> builder of the geometry cases: run at GEOMETRY_SIGMA, every pixel of every one has k_ref < k_res
TALL = _tall_cases()
TINY = {f"tiny-{H}x{W}": functools.partial(tiny_case, H, W, 7 + H + W) for H, W in TINY_HW}
SEAM = {f"seam-5x{W}": functools.partial(seam_case, W, W) for W in SEAM_W}
WIDE = {f"wide-{H}x{W}": functools.partial(wide_case, H, W, H + W) for H, W in WIDE_HW}
GEOMETRY = {**TALL, **TINY, **SEAM, **WIDE, "mixed-batch-40x57": mixed_batch}


@functools.lru_cache(maxsize=None)
def case(name):
    """(target int64 [B,H,W], k_ref int64 [B,H,W]) of a geometry case, built once and left unchanged."""
    t = GEOMETRY[name]()
    k = k_ref(boundary(t))
    t.setflags(write=False)
    k.setflags(write=False)
    return t, k
