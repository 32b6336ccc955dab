"""The grids the inflation tests share (tests/test_inflation_host.py checks the rule's restatement and each case's property
on the CPU, tests/test_gpu_inflation.py holds the GPU to the restatement on the same grids).  Every grid is seeded; a
case is (name, grid int8 [H, W], the InflationConfig's fields).  The kernel works on tiles of 64 columns x 32 rows and
looks for a row's obstacles in three 64-bit words, so the shapes straddle those sizes."""
import numpy as np

TILE_W, TILE_H = 64, 32          # csrc/inflate.hip: INFL_TW, INFL_TH


def random_grid(seed, H, W, p_obstacle=0.02, p_unknown=0.3, top=99):
    """Unknown cells, known costs 0 .. top and a few cells of 100."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, top + 1, (H, W))
    u = rng.random((H, W))
    g = np.where(u < p_unknown, -1, g)
    g = np.where(rng.random((H, W)) < p_obstacle, 100, g)
    return g.astype(np.int8)


def cfg(R, inscribed=1.0, factor=0.3, **more):
    """Cells of 1 m, so the radius in cells is the radius in metres."""
    return dict(resolution=1.0, inscribed_radius=float(min(inscribed, R)), inflation_radius=float(R),
                cost_scaling_factor=float(factor), **more)


def _one_cell():
    return np.array([[100]], np.int8)


def _corners():
    g = random_grid(3, 29, 37, p_obstacle=0.01)
    g[0, 0] = g[0, -1] = g[-1, 0] = g[-1, -1] = 100
    return g


def _two_words():
    """Random obstacles right of column 100 only; left of it one obstacle at (31, 63), the last row of the first tile row
    and the last column of the first word: its neighbours to the right and below lie in another word and another tile."""
    g = random_grid(5, 65, 130, p_obstacle=0.0)
    right = random_grid(6, 65, 130, p_obstacle=0.03)
    g[:, 100:] = right[:, 100:]
    g[31, 63] = 100
    return g


def _max_radius():
    """Two obstacles in opposite corners of 70 x 70 under R = 64: (0, 64) is exactly R cells from the first, (0, 65) in
    reach of neither."""
    g = random_grid(7, 70, 70, p_obstacle=0.0)
    g[0, 0] = g[69, 69] = 100
    return g


def _threshold():
    """Costs up to 60, a few cells of 65 .. 100 (obstacles from 65 on), and a 64 with nothing lethal within the radius."""
    g = random_grid(8, 29, 37, p_obstacle=0.0, top=60)
    rng = np.random.default_rng(18)
    g = np.where(rng.random(g.shape) < 0.03, rng.integers(65, 101, g.shape), g).astype(np.int8)
    g[5:16, 5:16] = np.minimum(g[5:16, 5:16], 60)
    g[10, 10], g[10, 20], g[20, 10] = 64, 65, 100
    return g


CASES = [
    ("one_cell", _one_cell(), cfg(3)),
    ("one_row", random_grid(2, 1, 37, p_obstacle=0.08), cfg(5)),
    ("corners", _corners(), cfg(4)),
    ("radius_beyond_both_sides", random_grid(4, 29, 37, p_obstacle=0.004), cfg(40, factor=0.05)),
    ("two_words", _two_words(), cfg(17, factor=0.1)),
    ("max_radius", _max_radius(), cfg(64, factor=0.03)),
    ("all_obstacle", np.full((33, 70), 100, np.int8), cfg(6)),
    ("no_obstacle", random_grid(9, 33, 70, p_obstacle=0.0), cfg(6)),
    ("all_unknown", np.full((33, 70), -1, np.int8), cfg(6)),
    ("threshold", _threshold(), cfg(4, lethal_threshold=65, unknown_min_cost=99)),
]
NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[NAMES.index(name)]


# three different grids of one shape and one configuration: a batch whose every index must equal its own batch-1 result
BATCH_CFG = cfg(4)
BATCH = np.stack([_corners(), random_grid(11, 29, 37), random_grid(12, 29, 37, p_obstacle=0.1)])


def brute_distance2(grid, lethal, R):
    """The rule's DISTANCE read literally: a loop over the cells and, for each, over the obstacles."""
    H, W = grid.shape
    ys, xs = np.nonzero(grid >= lethal)
    out = np.full((H, W), R * R + 1, np.int64)
    for y in range(H):
        for x in range(W):
            for oy, ox in zip(ys.tolist(), xs.tolist()):
                dx, dy = ox - x, oy - y
                if abs(dx) <= R and abs(dy) <= R and dx * dx + dy * dy <= R * R:
                    out[y, x] = min(out[y, x], dx * dx + dy * dy)
    return out.astype(np.uint16)
