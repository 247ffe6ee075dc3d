// grid_scan.h -- the walks over the cell-sorted record array: a ring block (scan_block), the cells of a ball (scan_pruned).
// Users: normals_point and knn_tagged (normals.hip), knn_kernel and radius_all_kernel (search.hip), coop_nearest (knn_coop.h: the
// axis gaps), the radius walks of fpfh.hip and cluster.hip.
#pragma once
#include "tc_internal.h"

namespace tc {

// square root for pruning radii: the raw v_sqrt_f32 (1 ulp; the callers add the cell-assignment fuzz, thousands of ulps, as slack;
// sqrtf's correctly rounded sequence costs ~10 instructions per row: 434 -> 421 us at 1 M points)
#define TC_FAST_SQRT(x) __builtin_amdgcn_sqrtf(x)

// distance from q to the box of cell index c along one axis, shaved by the cell-assignment fuzz
// `ext`: the grid's box is clamped (GridGeom::clamped): the first / last cell of the axis (c == 0 / c == last) also
// holds the points beyond the box, so it has no face on that side
template <bool EXT>
__device__ __forceinline__ float axis_gap_n(float q, float mn, float h, int c, int last) {
    const float lo = mn + (float)c * h, hi = lo + h;
    float a = lo - q, b = q - hi;
    if (EXT) {
        a = (c == 0) ? -INFINITY : a;
        b = (c == last) ? -INFINITY : b;
    }
    return fmaxf(fmaxf(a, b) - 2e-3f * h, 0.0f);
}

// visit every record of the Chebyshev ring block [c-R, c+R]^3 (clamped to the grid)
template <typename F>
__device__ __forceinline__ void scan_block(const GridView &gv, int cx, int cy, int cz, int R, F &&f) {
    const GridGeom &g = gv.g;
    const int x0 = max(cx - R, 0), x1 = min(cx + R, g.gx - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, g.gy - 1);
    const int z0 = max(cz - R, 0), z1 = min(cz + R, g.gz - 1);
    for (int z = z0; z <= z1; ++z) {
        for (int y = y0; y <= y1; ++y) {
            const uint32_t row = ((uint32_t)z * g.gy + y) * g.gx;
            const uint32_t s = gv.cell_start[row + x0], e = gv.cell_start[row + x1 + 1];
            // the record of step i + 1 is requested before step i is evaluated (the padding behind the array makes pts[e] readable):
            // 1-3 % (k = 10 / 16 / 32: 410 -> 398, 535 -> 532, 1048 -> 1029 us)
            // four records requested together (reads past the span stay inside the padded array and are not visited): 143 -> 133 us
            // on a 24 k-point frame (most SIMDs hold one wave there: its dependent round trips are the kernel's time), 520 -> 512 us
            // at 1 M points (one record ahead: 532)
            for (uint32_t j = s; j < e; j += 4) {
                const float4 c0 = gv.pts[j], c1 = gv.pts[j + 1], c2 = gv.pts[j + 2], c3 = gv.pts[j + 3];
                f(j, c0);
                if (j + 1 < e) f(j + 1, c1);
                if (j + 2 < e) f(j + 2, c2);
                if (j + 3 < e) f(j + 3, c3);
            }
        }
    }
}

// visit the records of the cells of block [c-R, c+R]^3 that (a) lie outside block [c-Rin, c+Rin]^3
// (Rin < 0: none excluded) and (b) whose box is within sqrt(lim) of q (ball pruning).  Returns
// whether any cell qualified.
// LIVE: after every row the limit is re-read from *live, which the visitor keeps up to date (a growing block scanned
// with an infinite limit starts pruning as soon as the list is full).
template <bool EXT, bool LIVE = false, typename F>
__device__ __forceinline__ bool scan_pruned(const GridView &gv, const float4 &q, int cx, int cy, int cz, int Rin, int R,
                                            float lim, F &&f, const float *live = nullptr, uint32_t *rowtag = nullptr) {
    const GridGeom &g = gv.g;
    const int x0 = max(cx - R, 0), x1 = min(cx + R, g.gx - 1);
    const int y0 = max(cy - R, 0), y1 = min(cy + R, g.gy - 1);
    const int z0 = max(cz - R, 0), z1 = min(cz + R, g.gz - 1);
    bool touched = false;
    for (int z = z0; z <= z1; ++z) {
        const float gz = axis_gap_n<EXT>(q.z, g.minz, g.h, z, g.gz - 1);
        for (int y = y0; y <= y1; ++y) {
            const float gy = axis_gap_n<EXT>(q.y, g.miny, g.h, y, g.gy - 1);
            const float rg = gy * gy + gz * gz;
            if (rg > lim) continue;
            const bool inner_row = (abs(z - cz) <= Rin) && (abs(y - cy) <= Rin);
            int xa = x0, xb = x1;
            {
                // x window the ball reaches, in closed form: cells whose box is within sqrt(lim - rg) of q.x (slack = the
                // cell-assignment fuzz twice, so never a cell too few; a clamped grid's boundary cells are open on the outer side,
                // which the same bounds cover).  The exact cell-by-cell trim this replaces cost more than the one or two extra
                // cells it saved: 515 -> 461 us at 1 M points, 133 -> 106 us on a 24 k-point frame.
                const float r = TC_FAST_SQRT(fmaxf(lim - rg, 0.0f)) + 4e-3f * g.h;
                const float fa = fminf(fmaxf((q.x - r - g.minx) * g.inv_h, 0.0f), (float)(g.gx - 1));
                const float fb = fmaxf(fminf((q.x + r - g.minx) * g.inv_h, (float)(g.gx - 1)), 0.0f);
                xa = max(xa, (int)fa);
                xb = min(xb, (int)fb);
            }
            if (xa > xb) continue;
            const uint32_t row = ((uint32_t)z * g.gy + y) * g.gx;
            if (rowtag) *rowtag = (uint32_t)((((z - cz + 3) & 7) << 3) | ((y - cy + 3) & 7)) << 6;     // knn_tagged: the row's code (|dz|, |dy| <= 3 there)
            auto span = [&](int a, int b) {
                if (a > b) return;
                touched = true;
                const uint32_t s = gv.cell_start[row + a], e = gv.cell_start[row + b + 1];
                for (uint32_t j = s; j < e; j += 4) {
                    const float4 c0 = gv.pts[j], c1 = gv.pts[j + 1], c2 = gv.pts[j + 2], c3 = gv.pts[j + 3];
                    f(j, c0);
                    if (j + 1 < e) f(j + 1, c1);
                    if (j + 2 < e) f(j + 2, c2);
                    if (j + 3 < e) f(j + 3, c3);
                }
            };
            if (!inner_row) span(xa, xb);
            else { span(xa, min(xb, cx - Rin - 1)); span(max(xa, cx + Rin + 1), xb); }   // only the cells outside the inner block
            if (LIVE) lim = *live;
        }
    }
    return touched;
}

}  // namespace tc
