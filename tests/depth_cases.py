"""Synthetic depth images (sensor_msgs/Image, 16UC1 / mono16 / 32FC1) shared by test_depth_ingest_host.py and
test_gpu_depth_ingest.py: sizes at which the three depth kernels can go wrong (chunk of 512 pixels, wave step of 64,
the scan's carry across 64 chunks), every encoding and byte order, padded rows, the clip, and the (first, decimate)
pairs the ingest is checked at.

A case is (image tuple, intrinsics, keyword arguments of the depth functions).  "64x8 with exactly 513 valid pixels"
cannot exist (64 x 8 is 512 pixels): 511 and 512 valid pixels are built at 64 x 8, and 511, 512 and 513 at 64 x 9, where
the 513th valid pixel sits in the second chunk."""
import numpy as np

SELECTIONS = [(1, 4), (0, 1), (3, 5)]


def intr(width, height, k=0):
    """Intrinsics that differ from case to case (float64, cast by intrinsics_of)."""
    return (0.6 * max(width, 1) + 1.3 * k, 0.61 * max(width, 1) - 0.7 * k, 0.5 * width - 0.13 + 0.01 * k,
            0.5 * height + 0.29 - 0.02 * k)


def _units(rng, height, width, invalid=0.3):
    """uint16 depths of 0.3 .. 6.5 m in millimetres, `invalid` of them 0."""
    d = rng.integers(300, 6500, (height, width)).astype(np.float64)
    d[rng.random((height, width)) < invalid] = 0
    return d


def _exact(rng, height, width, n_valid):
    """An image with exactly n_valid non-zero pixels, spread over it."""
    d = np.zeros(height * width)
    d[np.sort(rng.choice(height * width, n_valid, replace=False))] = rng.integers(300, 6500, n_valid)
    return d.reshape(height, width)


def cases(pp):
    """name -> (image, intrinsics, kwargs)."""
    s = pp.synth
    rng = np.random.default_rng(11)
    out = {}

    def u16(name, d, k=0, intrinsics=None, **kw):
        h, w = d.shape
        img_kw = {a: kw.pop(a) for a in ("step_pad", "bigendian", "encoding") if a in kw}
        scale = kw.get("depth_scale", 0.001)
        out[name] = (s.depth_from_z(d * scale, depth_scale=scale, seed=300 + len(out), **img_kw),
                     intrinsics if intrinsics is not None else intr(w, h, k), kw)

    u16("empty_0x0", np.zeros((0, 0)))
    u16("w1_h1", np.full((1, 1), 1234.0), 1)
    u16("w1_h513", _units(rng, 513, 1), 2)
    u16("w513_h1", _units(rng, 1, 513), 3)
    u16("w7_h73", _units(rng, 73, 7), 4)
    u16("w73_h7", _units(rng, 7, 73), 5)
    for n in (511, 512):
        u16(f"w64_h8_valid_{n}", _exact(rng, 8, 64, n), 6)
    for n in (511, 512, 513):
        u16(f"w64_h9_valid_{n}", _exact(rng, 9, 64, n), 7)
    u16("w256_h130_65_chunks", _units(rng, 130, 256), 8)
    u16("all_zero", np.zeros((24, 40)), 9)
    u16("all_valid", _units(rng, 31, 50, invalid=0.0), 10)
    for n in sorted({f for f, _ in SELECTIONS} - {0}):        # (first = 0: all_zero)
        u16(f"valid_{n}_keeps_nothing_at_first_{n}", _exact(rng, 20, 33, n), 11)
    u16("padded_rows_even", _units(rng, 37, 45), 12, step_pad=6)
    u16("padded_rows_odd_step", _units(rng, 33, 61), 13, step_pad=5)
    u16("bigendian_u16", _units(rng, 48, 64), 14, bigendian=True)
    u16("bigendian_u16_odd_step", _units(rng, 21, 30), 15, bigendian=True, step_pad=3)
    u16("mono16", _units(rng, 16, 24), 16, encoding="mono16")
    u16("depth_scale_quarter_mm", _units(rng, 40, 52), 17, depth_scale=0.00025)
    # the principal point on a pixel centre and a (K, D) camera info with zero distortion
    K = [38.5, 0.0, 20.0, 0.0, 38.25, 12.0, 0.0, 0.0, 1.0]
    u16("principal_point_on_a_pixel", _units(rng, 24, 40), intrinsics=(K, [0.0] * 5))

    # the clip on 16UC1: z is float32(0.001) * float32(d); one pixel equals z_max (kept), one equals z_min (dropped)
    d = _units(rng, 30, 44)
    d[3, 5], d[17, 9] = 1500, 4000
    f32 = np.float32
    u16("clip_u16", d, 18, z_min=float(f32(0.001) * f32(1500)), z_max=float(f32(0.001) * f32(4000)))

    def f32case(name, z, k=0, **kw):
        h, w = z.shape
        img_kw = {a: kw.pop(a) for a in ("step_pad", "bigendian") if a in kw}
        out[name] = (s.depth_from_z(z, "32FC1", seed=400 + len(out), **img_kw), intr(w, h, k), kw)

    def floats(h, w):
        z = rng.uniform(0.3, 6.5, (h, w)).astype(np.float32)      # normal numbers only
        sel = rng.random((h, w))
        for lo, v in ((0.00, np.nan), (0.05, np.inf), (0.10, -np.inf), (0.15, -1.25), (0.20, -0.0), (0.25, 0.0)):
            z[(sel >= lo) & (sel < lo + 0.05)] = v
        return z

    f32case("f32_little_endian", floats(36, 52), 19)
    f32case("f32_bigendian", floats(29, 47), 20, bigendian=True)
    f32case("f32_odd_step", floats(25, 35), 21, step_pad=3)
    f32case("f32_bigendian_padded", floats(19, 66), 22, bigendian=True, step_pad=2)
    z = floats(33, 40)
    z[2, 7], z[20, 11] = 1.5, 4.0
    f32case("clip_f32", z, 23, z_min=1.5, z_max=4.0)
    # depth_scale is not applied to 32FC1 (REP 118)
    f32case("f32_ignores_depth_scale", floats(12, 70), 24, depth_scale=0.00025)
    return out


def scene(pp, frame, width, height, **kw):
    """(image, intrinsics) of a seeded scene that fills pillars: synth.depth_image."""
    return pp.synth.depth_image(frame, width, height, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
