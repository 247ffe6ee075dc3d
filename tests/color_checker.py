"""The contract of include/threecrate_hip_color.h in numpy float32, operation by operation (test infrastructure): what tc_colorize must
return bit for bit.  Every product, sum and quotient below is ONE float32 operation on float32 operands; the three lerps are three
separate operations each (no fused multiply-add); roundf is half away from zero and returns |x| >= 2^23 unchanged.

RULES names the rules a mutant changes (tests/test_color_cpu.py holds every mutant to a named case of tests/color_cases.py that tells
it apart, and tests/test_gpu_color.py runs the same cases on the device): colorize(..., rules={"round_half_even"}) is the contract with
that one rule replaced."""
import numpy as np

F = np.float32

RULES = {
    "min_depth_strict": "step 3 skips c_z == min_depth too (c_z > min_depth)",
    "round_half_even": "roundf rounds halves to even",
    "floor_trunc": "floorf truncates towards zero (a negative u)",
    "no_border_fallback": "bilinear mode: a clipped neighbourhood colours nothing instead of falling back to nearest",
    "fused_lerp": "every lerp is one fused multiply-add, fma(b - a, t, a)",
    "val_trunc": "the bilinear value is truncated, not rounded",
    "default_is_hit": "step 9 is missing: a pixel of the default colour counts as a hit",
    "last_wins": "the LAST source that colours a point wins",
    "depth_tol_strict": "step 7 needs |c_z - d| < tolerance",
    "depth_at_floor": "step 7 reads the depth at (xf, yf)",
    "project_div_first": "step 4 computes fx (c_x / c_z)",
    "nonfinite_point_samples": "a point that is not finite samples pixel (0, 0) of the first source (the reference's `as i32`)",
}


def roundf(x, half_even=False):
    """C roundf on float32: half away from zero; |x| >= 2^23 (and inf, NaN) comes back unchanged"""
    x = np.asarray(x, F)
    if half_even:
        return np.rint(x)
    with np.errstate(invalid="ignore"):
        a = np.abs(x)
        fl = np.floor(a)
        r = np.copysign(fl + ((a - fl) >= F(0.5)).astype(F), x)        # a - fl is exact
        return np.where(a >= F(2 ** 23), x, r).astype(F)


def lerp(a, b, t, fused=False):
    if fused:                                   # fma(b - a, t, a): the product and the sum are exact in float64, then ONE rounding
        return (a.astype(np.float64) + (b - a).astype(np.float64) * t.astype(np.float64)).astype(F)
    d = b - a
    p = d * t
    return a + p


def project(xyz, intrinsics, matrix, div_first=False):
    """steps 2 and 4: (c_z, u, v) of every point"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    m = np.asarray(matrix, F).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    with np.errstate(all="ignore"):
        c = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)]
        if div_first:
            u, v = fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy
        else:
            u, v = (fx * c[0]) / c[2] + cx, (fy * c[1]) / c[2] + cy
    return c[2], u, v


def colorize(xyz, sources, default_color=(128, 128, 128), interpolation=1, min_depth=1e-4, depth_tolerance=0.05, rules=()):
    """-> (rgb (n, 3) uint8, source_index (n,) int32, colored_count).  sources: (image H x W x 3 uint8, (fx, fy, cx, cy), matrix of 12
    or 16 floats[, depth H x W float32 or None]) in order."""
    rules = set(rules)
    assert rules <= set(RULES), rules - set(RULES)
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    dc = np.asarray(default_color, np.uint8)
    md, tol = F(min_depth), F(depth_tolerance)
    rgb, index = np.tile(dc, (n, 1)), np.full(n, -1, np.int32)
    finite_pt = np.isfinite(xyz).all(axis=1)                                            # (1)
    looking = finite_pt.copy()
    for s, src in enumerate(sources):
        img, k, m = src[:3]
        depth = src[3] if len(src) > 3 else None
        img = np.asarray(img, np.uint8)
        h, w = img.shape[:2]
        fw, fh = F(w), F(h)
        idx = np.nonzero(finite_pt if "last_wins" in rules else looking)[0]
        if not idx.size:
            continue
        with np.errstate(all="ignore"):
            cz, u, v = project(xyz[idx], k, m, "project_div_first" in rules)            # (2), (4)
            ok = (cz > md) if "min_depth_strict" in rules else (cz >= md)               # (3)
            ok &= np.isfinite(u) & np.isfinite(v)                                       # (5)
            xn, yn = roundf(u, "round_half_even" in rules), roundf(v, "round_half_even" in rules)     # (6)
            inside = (xn >= 0) & (xn < fw) & (yn >= 0) & (yn < fh)
            xf, yf = (np.trunc(u), np.trunc(v)) if "floor_trunc" in rules else (np.floor(u), np.floor(v))
            if depth is not None:                                                       # (7)
                dx, dy = (xf, yf) if "depth_at_floor" in rules else (xn, yn)
                ok &= (dx >= 0) & (dx < fw) & (dy >= 0) & (dy < fh)
                d = np.asarray(depth, F)[np.where(ok, dy, 0).astype(np.int64), np.where(ok, dx, 0).astype(np.int64)]
                gap = np.abs(cz - d)
                ok &= np.isfinite(d) & (d > 0) & ((gap < tol) if "depth_tol_strict" in rules else (gap <= tol))
            bil = ok & (interpolation == 1) & (xf >= 0) & (yf >= 0) & (xf + F(1) < fw) & (yf + F(1) < fh)    # (8)
            near = ok & ~bil & inside
            if "no_border_fallback" in rules and interpolation == 1:
                near[:] = False
            out = np.zeros((idx.size, 3), np.uint8)
            if bil.any():
                ub, vb = u[bil], v[bil]
                x0, y0 = xf[bil].astype(np.int64), yf[bil].astype(np.int64)
                tx, ty = (ub - xf[bil])[:, None], (vb - yf[bil])[:, None]
                c00, c10, c01, c11 = (img[y0 + j, x0 + i].astype(F) for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
                fused = "fused_lerp" in rules
                top = lerp(c00, c10, tx, fused)
                bot = lerp(c01, c11, tx, fused)
                val = lerp(top, bot, ty, fused)
                val = np.trunc(val) if "val_trunc" in rules else roundf(val, "round_half_even" in rules)
                out[bil] = np.clip(val, 0, 255).astype(np.uint8)
            if near.any():
                out[near] = img[yn[near].astype(np.int64), xn[near].astype(np.int64)]
        got = bil | near
        hit = got if "default_is_hit" in rules else got & ~(out == dc).all(axis=1)      # (9)
        sel = idx[hit]
        rgb[sel], index[sel] = out[hit], s                                              # (10)
        looking[sel] = False
    if "nonfinite_point_samples" in rules and len(sources):
        img = np.asarray(sources[0][0], np.uint8)
        px = np.zeros(3, np.uint8) if interpolation == 1 and img.shape[0] > 1 and img.shape[1] > 1 else img[0, 0]
        if not (px == dc).all():
            rgb[~finite_pt], index[~finite_pt] = px, 0
    return rgb, index, int((index >= 0).sum())
