"""Inputs that tests/test_depth_sensor.py (CPU) and tests/test_gpu_depth_sensor.py (MI355X) share: the native configs of each
stage with the others off, the images, and the combined case (all stages on, a depth ramp with step edges)."""
import numpy as np

SEED, OFFSET, COUNTER = (5 << 32) | 77, 4000, (1 << 32) | 9
DENORMAL = float(np.float32(1e-40))
RANGE = (0.75, 5.5)                                    # both exactly representable


def native(range_min=0.0, range_max=np.inf, sigma=(0.0, 0.0, 0.0), p_drop=0.0, p_edge=0.0, edge_rel=0.1, edge_at_invalid=1,
           disparity_step=0.0, fb=0.0, inv_step=0.0, invalid_value=0.0):
    """A rover_depth_sensor_cfg set field by field (no cfg.DepthSensorCfg in between: fb and inv_step are the test's own)."""
    from isaac_rover_orbit_amd import _lib
    return _lib.DepthSensorCfg(range_min, range_max, sigma[0], sigma[1], sigma[2], p_drop, p_edge, edge_rel, edge_at_invalid,
                               disparity_step, fb, inv_step, invalid_value)


def blocks(n, H, W, seed=0):
    """(n, H * W) float32: plateaus of 7 x 5 pixels 0.6 m apart around 2 m with 1 cm of roughness (so every plateau border is an
    edge at edge_rel = 0.1 and nothing inside a plateau is), and one of each special value per image where the image has room:
    NaN, +inf, -inf, -1, 0, a denormal and both bounds of RANGE, exactly."""
    rng = np.random.default_rng(seed * 1000003 + n * 10007 + H * 131 + W)
    i, j = np.mgrid[0:H, 0:W]
    z = 2.0 + 0.6 * (((i // 7) + (j // 5)) % 3) + 0.01 * rng.standard_normal((n, H, W))
    z = z.astype(np.float32).reshape(n, H * W)
    specials = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, DENORMAL, RANGE[0], RANGE[1]], np.float32)
    for r in range(n):
        for s, v in enumerate(specials):
            if 13 * s + r < H * W:
                z[r, (13 * s + 11 * r) % (H * W)] = v
    return z


def stage_cfgs():
    """{name: native cfg}: one stage on, the others off (sigma = 0 adds an exact zero to every in-range finite depth)."""
    out = {"range": native(range_min=RANGE[0], range_max=RANGE[1]),
           "edge": native(range_min=RANGE[0], range_max=RANGE[1], p_edge=1.0),
           "edge_not_at_invalid": native(range_min=RANGE[0], range_max=RANGE[1], p_edge=1.0, edge_at_invalid=0, edge_rel=0.05),
           "drop0": native(range_min=RANGE[0], range_max=RANGE[1], p_drop=0.0, p_edge=0.0),
           "drop0.3": native(range_min=RANGE[0], range_max=RANGE[1], p_drop=0.3, p_edge=0.3),
           "drop1": native(range_min=RANGE[0], range_max=RANGE[1], p_drop=1.0, p_edge=1.0),
           "fill_inf": native(range_min=RANGE[0], range_max=RANGE[1], p_drop=0.3, p_edge=0.6, invalid_value=np.inf),
           "fill_minus1": native(range_min=RANGE[0], range_max=RANGE[1], p_drop=0.3, p_edge=0.6, invalid_value=-1.0)}
    return out


def quant_cfgs():
    """Quantisation alone, sigma = 0, on the full range [0, inf]: fb = 5 and 7 with a step of 1/8 px make d * inv_step = 40 / z and
    56 / z, so z = 16 is a tie (2.5 -> 2, 3.5 -> 4), z = 80 (fb = 5) the tie 0.5 -> 0: invalid."""
    return {"quant5": native(disparity_step=0.125, fb=5.0, inv_step=8.0, invalid_value=-1.0),
            "quant7": native(disparity_step=0.125, fb=7.0, inv_step=8.0, invalid_value=-1.0)}


def quant_images(n, H, W):
    """(n, H * W) float32 in [0.3, 20) with ties, k < 1 and very large depths sprinkled in."""
    rng = np.random.default_rng(n * 7919 + H * 131 + W)
    z = (0.3 + 19.7 * rng.random((n, H * W))).astype(np.float32)
    specials = np.array([16.0, 80.0, 32.0, 112.0, 1e6, 1e30, 3e38, 0.0, DENORMAL, 64.0], np.float32)
    for r in range(n):
        for s, v in enumerate(specials):
            if 7 * s + r < H * W:
                z[r, (7 * s + 3 * r) % (H * W)] = v
    return z


# ----------------------------------------------------------------------------------------------------------- the combined case
COMBINED_N, COMBINED_H, COMBINED_W = 3, 90, 160
COMBINED_FOCAL_PX, COMBINED_BASELINE, COMBINED_STEP = 160 * 2.12 / 6.055, 0.05, 0.125
LEFT_OUT_WITHIN, LEFT_OUT_CAP = 1e-3, 0.01


def combined_cfg():
    fb = float(np.float32(COMBINED_FOCAL_PX * COMBINED_BASELINE))
    return native(range_min=RANGE[0], range_max=RANGE[1], sigma=(0.001, 0.0005, 0.002), p_drop=0.05, p_edge=0.6, edge_rel=0.1,
                  disparity_step=COMBINED_STEP, fb=fb, inv_step=float(np.float32(1.0 / COMBINED_STEP)), invalid_value=0.0)


def combined_images():
    """(3, 90 * 160) float32: a ramp of 2 cm per column and 1.3 cm per row from 1 m, a step of 1.5 m at column 100, one of 0.8 m at
    row 50 and 10 cm per image.  The far corner leaves RANGE, so the ramp also has an edge at invalid neighbours."""
    i, j = np.mgrid[0:COMBINED_H, 0:COMBINED_W]
    z = 1.0 + 0.02 * j + 0.013 * i + 1.5 * (j >= 100) + 0.8 * (i >= 50)
    z = np.stack([z + 0.1 * r for r in range(COMBINED_N)])
    return z.astype(np.float32).reshape(COMBINED_N, -1)


def left_out(stages):
    """The pixels whose float64 d * inv_step lies within LEFT_OUT_WITHIN of a half-integer, among the spec's valid ones."""
    dk = stages["dk"]
    return stages["valid"] & (np.abs((dk - np.floor(dk)) - 0.5) < LEFT_OUT_WITHIN)
