// knn_list.h -- what the lane-per-query searches share besides the cell walks of grid_scan.h (device only): the sorted register
// list (normals.hip, search.hip) and the placement of a query in the grid (search.hip, fpfh.hip, cluster.hip).
#pragma once
#include "grid_scan.h"

namespace tc {

// ---- sorted register list -------------------------------------------------------------------
template <int L>
__device__ __forceinline__ void list_insert(float (&d)[L], float v) {
#pragma unroll
    for (int t = L - 1; t >= 1; --t) d[t] = __builtin_amdgcn_fmed3f(d[t - 1], v, d[t]);
    d[0] = fminf(d[0], v);
}

// ---- query placement --------------------------------------------------------------------------
// a NaN / infinite query has no finite distance to anything
__device__ __forceinline__ bool finite_query(float x, float y, float z) {
    return fabsf(x) <= 3.0e38f && fabsf(y) <= 3.0e38f && fabsf(z) <= 3.0e38f;
}
struct QueryPlace {
    int   cx, cy, cz;       // the cell of the query clamped into the box
    float mf;               // distance to the nearest face of that cell, in cells
    float out2;             // squared distance from the query to the box, shaved: |p - q|^2 >= |p - clamp(q)|^2 + |q - clamp(q)|^2 needs
                            // every record inside the box: not so when the box is clamped (EXT), 0 there
};
template <bool EXT>
__device__ __forceinline__ QueryPlace place_query(const GridGeom &g, const float4 &q) {
    const float qx = fminf(fmaxf(q.x, g.minx), g.maxx), qy = fminf(fmaxf(q.y, g.miny), g.maxy), qz = fminf(fmaxf(q.z, g.minz), g.maxz);
    QueryPlace pl;
    pl.cx = cell_coord(qx, g.minx, g.inv_h, g.gx); pl.cy = cell_coord(qy, g.miny, g.inv_h, g.gy); pl.cz = cell_coord(qz, g.minz, g.inv_h, g.gz);
    const float fx = (qx - g.minx) * g.inv_h - (float)pl.cx, fy = (qy - g.miny) * g.inv_h - (float)pl.cy, fz = (qz - g.minz) * g.inv_h - (float)pl.cz;
    pl.mf = fmaxf(fminf(fminf(fminf(fx, 1.0f - fx), fminf(fy, 1.0f - fy)), fminf(fz, 1.0f - fz)), 0.0f);
    const float ex = q.x - qx, ey = q.y - qy, ez = q.z - qz;
    pl.out2 = EXT ? 0.0f : (ex * ex + ey * ey + ez * ez) * 0.9999f;
    return pl;
}

}  // namespace tc
