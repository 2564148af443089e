"""Seeded inputs at the edges of the visual front end's domain (numpy only): images that drive the integer accumulators of tracking
and detection to their bounds, point sets on the bounds of the window test, descriptor sets at the ends of the Hamming range -- and the
case lists tests/test_gpu_frontend_extremes.py runs, so that tests/test_frontend_extremes_cpu.py can state facts about every one of
them from the restatements alone."""
from __future__ import annotations

import numpy as np

f32 = np.float32

# ---- images (uint8, any size) -------------------------------------------------------------------------------------------------------


def noise01(w: int, h: int, seed: int = 0) -> np.ndarray:
    """i.i.d. 0 / 255"""
    return (np.random.default_rng(seed).integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255)).astype(np.uint8)


def checker(w: int, h: int, period: int = 1) -> np.ndarray:
    """0 / 255 squares of `period` pixels.  Period 1 is the fastest texture and the central differences (Scharr, Sobel) of it are zero
    on every pixel: to the tracker and the detector it is a flat image with full-range values.  Period 2 reaches the largest
    magnitudes, 4080 (Scharr) and 1020 (Sobel)"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // period) + (y // period)) & 1) * 255).astype(np.uint8)


def uniform_noise(w: int, h: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def step_edges(w: int, h: int) -> np.ndarray:
    """0 | 255 half planes: two vertical edges (left third), a horizontal edge (middle third), a diagonal (right third); along an
    edge the gradient has one direction only (the aperture problem)"""
    y, x = np.mgrid[0:h, 0:w]
    a, b = w // 3, (2 * w) // 3
    img = np.zeros((h, w), np.uint8)
    img[(x >= a // 2) & (x < a)] = 255
    img[(x >= a) & (x < b) & (y >= h // 2)] = 255
    img[(x >= b) & ((x - b) + y >= (h + (w - b)) // 2)] = 255
    return img


def stripes(w: int, h: int, period: int = 2) -> np.ndarray:
    """vertical 0 / 255 stripes of `period` pixels; period 2 puts |Sobel dx| = 1020 on EVERY pixel: the 3 x 3 box sum of dx^2 reaches
    its analytic maximum 9 * 1020^2"""
    return np.tile((((np.arange(w) // period) & 1) * 255).astype(np.uint8), (h, 1))


def saturated(w: int, h: int, value: int) -> np.ndarray:
    return np.full((h, w), value, np.uint8)


def shifted(img: np.ndarray, dx: int, dy: int) -> np.ndarray:
    """the image moved by (dx, dy) whole pixels (a roll): a point at p is at p + (dx, dy) afterwards"""
    return np.roll(img, (dy, dx), axis=(0, 1))


FAMILIES = {
    "noise01": lambda w, h: noise01(w, h, 1),
    "checker1": lambda w, h: checker(w, h, 1),
    "checker2": lambda w, h: checker(w, h, 2),
    "uniform_noise": lambda w, h: uniform_noise(w, h, 2),
    "step_edges": step_edges,
    "saturated0": lambda w, h: saturated(w, h, 0),
    "saturated255": lambda w, h: saturated(w, h, 255),
}

# ---- point sets ---------------------------------------------------------------------------------------------------------------------


def uniform_points(n: int, w: int, h: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32)


def bound_coords(n: int, win: int):
    """coordinates p on both sides of the window test's bounds -win <= p - hw < n (hw = (win - 1) / 2, f32 arithmetic as in the
    kernel): p - hw equal to -win, the largest p below it (outside), p - hw equal to n - 1, equal to n (outside), the largest p below
    that (inside).  Where nextafter(bound) + hw is not a float, the neighbour of the bound IN p is what decides"""
    hw = f32((win - 1) * 0.5)

    def at(b):
        p = f32(f32(b) + hw)
        assert f32(p - hw) == f32(b)
        return p

    def below(b):
        p = at(b)
        while f32(p - hw) >= f32(b):
            p = np.nextafter(p, f32(-np.inf))
        return p
    return [at(-win), below(-win), at(n - 1), at(n), below(n)]


def boundary_points(w: int, h: int, win: int) -> np.ndarray:
    """56 points: the window corner p - hw on every bound of the window test in x, in y and in both; integer coordinates; fractions 0,
    0.5 and 1 - 2^-10; +/-1e9 and +/-3e38 (finite, far outside)"""
    bx, by = bound_coords(w, win), bound_coords(h, win)
    mx, my = f32(w // 2) + f32(0.25), f32(h // 2) + f32(0.75)
    pts = [(x, my) for x in bx] + [(mx, y) for y in by] + [(x, y) for x in bx for y in by]
    fr = [f32(0), f32(0.5), f32(1 - 2.0 ** -10)]
    pts += [(f32(w // 3) + a, f32(h // 3) + b) for a in fr for b in fr]
    pts += [(0, 0), (w - 1, h - 1), (w // 2, h // 2), (w // 4, (3 * h) // 4)]
    for big in (1e9, 3e38):
        pts += [(big, my), (-big, my), (mx, big), (mx, -big)]
    return np.asarray(pts, dtype=np.float32).reshape(-1, 2)


NON_FINITE_POINTS = np.array([[np.nan, 20], [30, np.inf], [-np.inf, np.nan], [np.inf, np.inf]], np.float32)

# ---- descriptor sets (uint8 [n, 64]) --------------------------------------------------------------------------------------------------


def desc_zeros(n: int = 1) -> np.ndarray:
    return np.zeros((n, 64), np.uint8)


def desc_ones(n: int = 1) -> np.ndarray:
    return np.full((n, 64), 255, np.uint8)


def desc_repeated_bytes() -> np.ndarray:
    """256 rows: row b is the byte b 64 times"""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 64, axis=1)


def desc_one_hot() -> np.ndarray:
    """512 rows: row i has bit i set only"""
    return np.packbits(np.eye(512, dtype=np.uint8), axis=1, bitorder="little")


def desc_one_cold() -> np.ndarray:
    return (~desc_one_hot()).astype(np.uint8)


def desc_at_distance(seed: int, n_train: int, d: int):
    """(query [n_train, 64], train [n_train, 64]): every query row's nearest train row is at distance exactly d.  Far end (d >= 500):
    all train rows are one random row and query i is its complement with 512 - d random bits put back, so every distance is d and
    the tie rule picks index 0.  Near end: query i is the random train row i with d bits flipped (random rows are ~256 apart)."""
    rng = np.random.default_rng(seed)
    if d >= 500:
        base = rng.integers(0, 256, (1, 64), dtype=np.uint8)
        train = np.repeat(base, n_train, axis=0)
        bits = np.unpackbits(~train, axis=1, bitorder="little")
        for i in range(n_train):
            bits[i, rng.choice(512, size=512 - d, replace=False)] ^= 1
        return np.packbits(bits, axis=1, bitorder="little"), train
    train = rng.integers(0, 256, (n_train, 64), dtype=np.uint8)
    bits = np.unpackbits(train, axis=1, bitorder="little")
    for i in range(n_train):
        bits[i, rng.choice(512, size=d, replace=False)] ^= 1
    return np.packbits(bits, axis=1, bitorder="little"), train


def descriptor_jobs():
    """name -> (query, train): the structured sets; expected nearest distances are asserted by the tests"""
    rb, hot, cold = desc_repeated_bytes(), desc_one_hot(), desc_one_cold()
    q512, t512 = desc_at_distance(11, 33, 512)
    q511, t511 = desc_at_distance(12, 33, 511)
    q1, t1 = desc_at_distance(13, 300, 1)
    return {
        "zeros_vs_ones": (desc_zeros(17), desc_ones(65)),            # every distance 512
        "ones_vs_zeros": (desc_ones(3), desc_zeros(1)),
        "zeros_vs_zeros": (desc_zeros(5), desc_zeros(70)),           # every distance 0, index 0
        "bytes_vs_bytes": (rb, rb[::-1].copy()),
        "bytes_vs_zeros_ones": (rb, np.concatenate([desc_ones(1), desc_zeros(1)])),
        "hot_vs_cold": (hot, cold),                                    # 510 or 512
        "cold_vs_hot": (cold, hot),
        "hot_vs_bytes": (hot, rb),
        "bytes_vs_hot": (rb, hot),
        "cold_vs_zeros": (cold, desc_zeros(2)),                        # 511
        "exactly_512": (q512, t512),
        "exactly_511": (q511, t511),
        "exactly_1": (q1, t1),
    }


# ---- the GPU module's tracking cases ----------------------------------------------------------------------------------------------

TRACK_SIZES = ((1226, 370), (641, 203))
TRACK_SHIFTS = ((3, -2), (45, 0))
TRACK_WINDOWS = ((5, 4), (21, 4), (31, 4), (5, 0), (21, 0), (31, 0))          # (window, max_level)
N_UNIFORM = 1000

SWEEP = ([dict(max_count=v) for v in (0, 1, 2, 100)] + [dict(epsilon=v) for v in (0.0, 1e-3, 10.0)] +
         [dict(min_eig_threshold=v) for v in (-1.0, 0.0, 1e-2, 1e3)] +
         [dict(flow_outlier=v) for v in (0.0, 1.0, float("inf"), float("-inf"))])


def track_points(w: int, h: int, win: int, seed: int = 7) -> np.ndarray:
    """1,000 uniform points and the boundary set of this window"""
    return np.concatenate([uniform_points(N_UNIFORM, w, h, seed), boundary_points(w, h, win)])


def family_pair(name: str, w: int, h: int, shift):
    img = FAMILIES[name](w, h)
    return img, shifted(img, shift[0], shift[1])


def step_edge_points(w: int, h: int, win: int) -> np.ndarray:
    """points along the three edges of step_edges (within 2 px of the edge: the window sees one gradient direction), the boundary
    set and four non-finite points"""
    rng = np.random.default_rng(3)
    a, b = w // 3, (2 * w) // 3
    n = 100
    e1 = np.stack([a // 2 + rng.uniform(-2, 2, n), rng.uniform(40, h - 40, n)], 1)
    e2 = np.stack([rng.uniform(a + 40, b - 40, n), h // 2 + rng.uniform(-2, 2, n)], 1)
    t = rng.uniform(0.3, 0.7, n)
    c = (h + (w - b)) // 2
    e3 = np.stack([b + t * c + rng.uniform(-1, 1, n), (1 - t) * c + rng.uniform(-1, 1, n)], 1)
    return np.concatenate([e1, e2, e3, boundary_points(w, h, win), NON_FINITE_POINTS]).astype(np.float32)


def non_finite_share(next_xy) -> float:
    """share of points with a non-finite coordinate in the restatement's result: what the GPU comparison may relax to class equality"""
    xy = np.asarray(next_xy, np.float32).reshape(-1, 2)
    return float((~np.isfinite(xy).all(1)).mean()) if len(xy) else 0.0


LEAVE_OUT_CAP = 0.05


def reference_map(fn, items, workers: int = 8):
    """[fn(item) for item in items] on a few threads (numpy releases the GIL in the restatements' large array operations)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as ex:
        return list(ex.map(fn, items))

# ---- small image sizes (w, h) -------------------------------------------------------------------------------------------------------

BUILD_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (15, 17), (16, 16), (17, 15), (33, 31), (65, 2))
BUILD_SIZES_GPU = BUILD_SIZES + ((16384, 1), (1, 16384))
DETECT_SMALL_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (17, 3), (5, 40))
