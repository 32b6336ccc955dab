"""frontier.py's restatement on the CPU: `frontier_np` against a second, independent statement (scipy.ndimage.label for
the partition, plain loops for the rest) on every shared case, the hand-pinned grid cell by cell, the configuration's
ranges, what each seeded case is there for, and the key widths at the extreme shapes."""
import numpy as np
import pytest
from scipy import ndimage

import frontier_cases as K

F = K.F


def _second(grid, cfg, ref, pot):
    """The rule again, by other means: the frontier test cell by cell, scipy's labelling, loops over the components."""
    c = F.FrontierConfig.from_any(cfg)
    H, W = grid.shape
    front = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if not 0 <= grid[y, x] <= c.free_max:
                continue
            for qx, qy in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                if 0 <= qx < W and 0 <= qy < H and grid[qy, qx] == -1:
                    front[y, x] = True
    structure = np.ones((3, 3), int) if c.connectivity == 8 else [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    comp, n_comp = ndimage.label(front, structure=structure)
    labels = np.full((H, W), F.NONE, np.uint32)
    rows, small, unreached = [], 0, 0
    for k in range(1, n_comp + 1):
        ys, xs = np.nonzero(comp == k)
        label = int((ys * W + xs).min())
        labels[ys, xs] = label
        n = len(xs)
        if n < c.min_size:
            small += 1
            continue
        sx, sy = int(xs.sum()), int(ys.sum())
        cx, cy = (2 * sx + n) // (2 * n), (2 * sy + n) // (2 * n)
        best = None
        for x, y in sorted(zip(xs.tolist(), ys.tolist()), key=lambda q: q[1] * W + q[0]):       # by index: the first least distance wins
            d = (x - cx) ** 2 + (y - cy) ** 2
            if best is None or d < best[0]:
                best = (d, x, y)
        _, x, y = best
        if c.use_field:
            D = int(pot[y, x])
            if D == F.UNREACHED:
                unreached += 1
                continue
        else:
            D = (x - ref[0]) ** 2 + (y - ref[1]) ** 2
        rows.append(((D, label) if c.rank == 0 else (-n, label), [x, y, cx, cy, n, label, D & 0xFFFFFFFF, D >> 32]))
    rows.sort(key=lambda r: r[0])
    words = np.array([r[1] for r in rows[:c.max_frontiers]], np.int64).reshape(-1, 8).astype(np.uint32).view(np.int32)
    info = np.array([front.sum(), n_comp, small, unreached, len(rows), len(words)], np.int32)
    return labels, words, info


@pytest.mark.parametrize("name", K.NAMES)
def test_restatement_equals_the_second_statement(name):
    _, g, cfg, ref, pot = K.case(name)
    labels, words, info = K.reference(name)
    wl, ww, wi = _second(g, cfg, ref, pot)
    assert labels.dtype == np.uint32 and words.dtype == np.int32 and info.dtype == np.int32
    assert np.array_equal(labels, wl), name
    assert np.array_equal(info, wi), (name, info, wi)
    assert np.array_equal(words, ww), name
    # every label is its component's least index, every representative a frontier cell of its cluster
    for lab in np.unique(labels[labels != F.NONE]):
        ys, xs = np.nonzero(labels == lab)
        assert lab == (ys * g.shape[1] + xs).min()
    for w in words:
        assert labels[w[1], w[0]] == np.uint32(w[5]) and 0 <= g[w[1], w[0]] <= F.FrontierConfig.from_any(cfg).free_max


def test_pinned_cell_by_cell():
    labels, words, info = K.reference("pinned")
    want = np.array([[F.NONE if v is None else v for v in row] for row in K.PINNED_LABELS], np.uint32)
    for y in range(5):
        for x in range(7):
            assert labels[y, x] == want[y, x], (x, y)
    assert words.tolist() == K.PINNED_WORDS and info.tolist() == K.PINNED_INFO
    assert F.cost_of(words) == [2, 4]


def test_cases_hold_what_they_are_there_for():
    info = {n: K.reference(n)[2] for n in K.NAMES}
    words = {n: K.reference(n)[1] for n in K.NAMES}
    for n in ("one_unknown", "one_free", "all_unknown", "all_free", "known_edges"):
        assert info[n].tolist() == [0] * 6, n
    assert info["free_max"][0] == 1 and words["free_max"][0, :2].tolist() == [1, 1]
    assert info["diagonal_c8"][1] == 1 and info["diagonal_c4"][1] == 2
    assert info["tile_corner_c8"][1] == 2 and info["tile_corner_c4"][1] == 4 and (words["tile_corner_c8"][:, 4] == 2).all()
    for W in (31, 33, 63, 65):                          # clusters on both sides of a tile edge in x and in y
        lab = K.reference(f"width_{W}_c8")[0]
        assert W % 4 != 0 and (lab[:, :K.TILE] != F.NONE).any() and (lab[K.TILE:, :] != F.NONE).any()
        assert W < K.TILE or (lab[:, K.TILE:] != F.NONE).any()
    ring = words["ring"][0]
    lab = K.reference("ring")[0]
    assert info["ring"][1] == 1 and lab[ring[3], ring[2]] == F.NONE                   # the centroid is no member
    assert ring[:2].tolist() == [70, 36] and (36 - 70) ** 2 == (70 - 36) ** 2          # (36, 70) is as near: the lesser index wins
    g = K.case("serpentine")[1]
    lab = K.reference("serpentine")[0]
    tiles = {(x // K.TILE, y // K.TILE) for y, x in zip(*np.nonzero(lab != F.NONE))}
    assert info["serpentine"][1] == 1 and len(tiles) >= 12 and g.shape == (70, 129) and words["serpentine"][0, 5] == 130
    u = words["u_shape"][0]
    assert K.case("u_shape")[1][u[3], u[2]] == 100 and K.case("u_shape")[1][u[1], u[0]] == 0      # a centroid in a wall
    for n in ("noise_min1", "noise_min3", "noise_largest", "noise_passes_min1", "noise_passes_min3"):
        assert info[n][4] > F.PP_FRONTIER_MAX == info[n][5], (n, info[n])            # more kept than are returned
    assert info["noise_min1"][2] == 0 < info["noise_min3"][2] and info["noise_passes_min3"][2] > 0
    assert info["noise_min1"][1] < K.SELECT_LANES < info["noise_passes_min1"][1]       # a lane per root, and the passes
    assert info["checkerboard"][1] > 2 * K.SELECT_CACHE and info["checkerboard"][5] == 64
    assert info["roots_256"][1] == K.SELECT_LANES == info["roots_257"][1] - 1                   # the last size of a lane per root, the first of the passes
    assert K.SELECT_LANES < info["roots_1200"][1] < K.SELECT_CACHE and info["roots_1200"][5] == 16
    assert len(set(F.cost_of(words["mirror_tie"]))) == 1 and words["mirror_tie"][:, 5].tolist() == [87, 99]
    e = words["equal_sizes_largest"]
    assert e[0, 4] == e[1, 4] and F.cost_of(e)[0] > F.cost_of(e)[1] and e[:, 5].tolist() == [87, 99]
    assert info["field_enclosed"][3] == 1 and info["field_enclosed"][4] == 1
    assert info["field_all_unreached"][3] == info["field_all_unreached"][1] == 2 and info["field_all_unreached"][5] == 0
    assert (K.case("field_all_unreached")[4] == F.UNREACHED).all()
    assert info["field_room_largest"][5] == 3 < info["field_room_largest"][4]
    for n in K.ROOMS:
        p = K.properties(n)
        for what in K.ROOM_PROPERTIES:
            assert p[what] > 0, (n, what, p)
    counts = [int(F.frontier_np(K.BATCH[b], K.BATCH_CFG, K.BATCH_REFS[b])[2][5]) for b in range(3)]
    assert counts[0] == 0 and len(set(counts)) == 3


def test_config_ranges():
    C = F.FrontierConfig
    assert C().to_dict() == dict(free_max=49, connectivity=8, min_size=3, max_frontiers=16, rank=0, use_field=0)
    for f, lo, hi in (("free_max", 0, 99), ("min_size", 1, K.F.PP_OCC_MAX_CELLS), ("max_frontiers", 1, 64), ("rank", 0, 1), ("use_field", 0, 1)):
        C(**{f: lo}), C(**{f: hi})
        for bad in (lo - 1, hi + 1):
            with pytest.raises(ValueError, match=f"FrontierConfig: {f} = {bad} outside"):
                C(**{f: bad})
    for conn in (3, 5, 6, 9):
        with pytest.raises(ValueError, match="connectivity"):
            C(connectivity=conn)
    with pytest.raises(ValueError, match="must be an integer"):
        C(free_max=1.5)
    with pytest.raises(ValueError, match="unknown keys"):
        C.from_any(dict(free=1))
    assert C.from_any(True) == C() and C.from_any(dict(rank=1)).rank == 1
    g = np.zeros((3, 3), np.int8)
    for ref in ((F.MAX_REF + 1, 0), (0, -F.MAX_REF - 1)):
        with pytest.raises(ValueError, match="reference cell"):
            F.frontier_np(g, {}, ref)
    with pytest.raises(ValueError, match="use_field = 1 needs pot"):
        F.frontier_np(g, dict(use_field=1), (0, 0))
    with pytest.raises(ValueError, match="int8"):
        F.frontier_np(g.astype(np.int32), {}, (0, 0))


@pytest.mark.parametrize("shape", [(1 << 20, 1), (1, 1 << 20)])
def test_key_widths_at_the_extreme_shapes(shape):
    """Python integers against uint64 arithmetic: nothing wraps where a coordinate is 2^20 - 1 and the reference lies at
    the far corner of its range."""
    H, W = shape
    g = np.zeros(shape, np.int8)
    flat = g.reshape(-1)
    flat[-2] = -1
    flat[3] = -1
    ref = (-F.MAX_REF, F.MAX_REF) if W > 1 else (F.MAX_REF, -F.MAX_REF)
    labels, words, info = F.frontier_np(g, dict(min_size=1), ref)
    assert info.tolist() == [4, 4, 0, 0, 4, 4]
    last = words[-1]
    x, y = int(last[0]), int(last[1])
    assert y * W + x == (1 << 20) - 1 == int(np.uint32(last[5]))
    D = F.cost_of(words)[-1]
    assert D == (x - ref[0]) ** 2 + (y - ref[1]) ** 2 and 1 << 42 < D < 1 << 43
    key = (D << 20) | int(np.uint32(last[5]))
    assert key < 1 << 64
    with np.errstate(over="raise"):
        dx, dy = np.uint64(abs(x - ref[0])), np.uint64(abs(y - ref[1]))
        k64 = ((dx * dx + dy * dy) << np.uint64(20)) | np.uint64(np.uint32(last[5]))
    assert int(k64) == key
    # the bounds the device's widths rest on: a sum of coordinates, a representative key, a sort key by size
    cells = 1 << 20
    assert cells * (cells - 1) < 1 << 64 and 2 * cells * (cells - 1) + cells < 1 << 64
    assert ((2 * (cells - 1) ** 2) << 20) | (cells - 1) < 1 << 64
    assert (((1 << 20) - 1) << 20) | (cells - 1) < 1 << 64
