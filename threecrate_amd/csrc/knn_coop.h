// knn_coop.h -- the k nearest records of one query by a whole block (device only): what the wave-per-point kernels share,
// normals_coop_kernel (normals.hip) and knn_coop_kernel (search.hip).
#pragma once
#include "grid_scan.h"

namespace tc {

constexpr int kCoopThreads = 256;

// shared scratch of one block of the wave-per-point kernels
template <int CAPB>
struct CoopShared {
    unsigned long long buf[CAPB];
    uint32_t hist[256];         // squared distances of the current ball over (hlo, lim], 256 bins: where an overflowing ball is cut
    uint32_t cnt;
    int bin;
};

// The K1 nearest records of q (any point, inside or outside the grid), as keys (distance bits << 32 | position) sorted ascending in
// sh.buf[0 .. return value): adaptive ball + LDS buffer + bitonic sort (see normals_coop_kernel).  Called by all threads of the block.
template <int CAPB>
__device__ __forceinline__ uint32_t coop_nearest(const GridView &gv, float qx, float qy, float qz, uint32_t K1, uint32_t nfin, CoopShared<CAPB> &sh) {
    const GridGeom &g = gv.g;
    const int tid = threadIdx.x;
    // the radius that certainly holds the whole cloud: the distance to the farthest corner of its (grid) box -- a clamped box
    // has records beyond it: there only the counts end the growth
    const float fxm = fmaxf(fabsf(qx - g.minx), fabsf(qx - g.maxx)), fym = fmaxf(fabsf(qy - g.miny), fabsf(qy - g.maxy)),
                fzm = fmaxf(fabsf(qz - g.minz), fabsf(qz - g.maxz));
    const float r_all = g.clamped ? 3.0e38f : sqrtf(fxm * fxm + fym * fym + fzm * fzm) * 1.001f;
    // the first radius at which the box proper comes into reach of a point outside it; no record INSIDE an exact box is
    // closer than the box (a clamped box has records beyond it, possibly nearer: they fall into the first histogram bin)
    const float bxo = fmaxf(fmaxf(g.minx - qx, qx - g.maxx), 0.0f), byo = fmaxf(fmaxf(g.miny - qy, qy - g.maxy), 0.0f),
                bzo = fmaxf(fmaxf(g.minz - qz, qz - g.maxz), 0.0f);
    const float d_box2 = (bxo * bxo + byo * byo + bzo * bzo) * 0.9999f;
    const float r_box = sqrtf(d_box2) + 2.0f * g.h;
    float r = 2.0f * g.h * cbrtf((float)K1 / 17.0f);
    // The ball is cut by KEY = (distance bits << 32 | position), compared exactly: khi = the largest key admitted to the buffer, klo =
    // a key known to have fewer than K1 records at or below it.  (The cut used to be a squared radius with relative safety factors
    // of 1e-5: a plateau of 1 500 exact duplicates 9e-6 beyond the (k+1)-th neighbour could not be cut off, the buffer overflowed and
    // the neighbours were whichever 512 records arrived first -- fuzz seed 611 case 3568.)
    unsigned long long klo = (!g.clamped && d_box2 > 0.0f) ? ((unsigned long long)__float_as_uint(d_box2) << 32) : 0ull;
    unsigned long long khi = ((unsigned long long)__float_as_uint(r * r) << 32) | 0xFFFFFFFFull;
    uint32_t total = 0;
    for (int guard = 0; guard < 200; ++guard) {
        if (tid == 0) sh.cnt = 0;
        sh.hist[tid] = 0;
        __syncthreads();
        const float lim = __uint_as_float((uint32_t)(khi >> 32));          // every admitted record lies within this squared radius
        r = sqrtf(lim) * 1.000001f;
        // 256 bins over the keys in (klo, khi]: bin = (key - klo - 1) >> sh
        const unsigned long long range = khi - klo;
        const int sh_bits = max(0, 64 - (int)__clzll((long long)(range - 1ull) | 1ll) - 8);
        const float ry = r * 1.0001f + 4e-3f * g.h;
        const int y0 = cell_coord(fminf(fmaxf(qy - ry, g.miny), g.maxy), g.miny, g.inv_h, g.gy), y1 = cell_coord(fminf(fmaxf(qy + ry, g.miny), g.maxy), g.miny, g.inv_h, g.gy);
        const int z0 = cell_coord(fminf(fmaxf(qz - ry, g.minz), g.maxz), g.minz, g.inv_h, g.gz), z1 = cell_coord(fminf(fmaxf(qz + ry, g.minz), g.maxz), g.minz, g.inv_h, g.gz);
        const int ny = y1 - y0 + 1;
        const uint32_t nrows = (uint32_t)ny * (uint32_t)(z1 - z0 + 1);
        auto take = [&](uint32_t j, const float4 &c) {
            const float v = d2_nc(c.x, c.y, c.z, qx, qy, qz);
            const unsigned long long key = ((unsigned long long)__float_as_uint(v) << 32) | j;
            if (key <= khi) {
                const uint32_t slot = atomicAdd(&sh.cnt, 1u);
                if (slot < (uint32_t)CAPB) sh.buf[slot] = key;
                if (key > klo) atomicAdd(&sh.hist[(uint32_t)min((key - klo - 1ull) >> sh_bits, 255ull)], 1u);
            }
        };
        for (uint32_t ri = (uint32_t)tid; ri < nrows; ri += kCoopThreads) {
            const int zz = z0 + (int)(ri / (uint32_t)ny), yy = y0 + (int)(ri % (uint32_t)ny);
            const float gy = g.clamped ? axis_gap_n<true>(qy, g.miny, g.h, yy, g.gy - 1) : axis_gap_n<false>(qy, g.miny, g.h, yy, g.gy - 1);
            const float gz = g.clamped ? axis_gap_n<true>(qz, g.minz, g.h, zz, g.gz - 1) : axis_gap_n<false>(qz, g.minz, g.h, zz, g.gz - 1);
            const float rg = gy * gy + gz * gz;
            if (rg > lim) continue;
            const float rx = sqrtf(fmaxf(lim - rg, 0.0f)) * 1.0001f + 4e-3f * g.h;
            const int xa = (int)fminf(fmaxf((qx - rx - g.minx) * g.inv_h, 0.0f), (float)(g.gx - 1));
            const int xb = (int)fmaxf(fminf((qx + rx - g.minx) * g.inv_h, (float)(g.gx - 1)), 0.0f);
            if (xa > xb) continue;
            const uint32_t row = ((uint32_t)zz * g.gy + yy) * g.gx;
            const uint32_t s = gv.cell_start[row + xa], e = gv.cell_start[row + xb + 1];
            for (uint32_t j = s; j < e; j += 4) {          // (reads past the span stay inside the padded array)
                const float4 c0 = gv.pts[j], c1 = gv.pts[j + 1], c2 = gv.pts[j + 2], c3 = gv.pts[j + 3];
                take(j, c0);
                if (j + 1 < e) take(j + 1, c1);
                if (j + 2 < e) take(j + 2, c2);
                if (j + 3 < e) take(j + 3, c3);
            }
        }
        __syncthreads();
        total = sh.cnt;
        if (total > (uint32_t)CAPB) {
            // too many for the buffer: cut at the bin in which the count reaches K1 -- the new range holds the K1-th key and 1/256
            // of the old one; a range of <= 256 keys has one key per bin, the cut is then the K1-th key itself (keys are unique:
            // the position is part of them), so a plateau of exact ties is cut by position, lowest first, like every other path
            if (tid == 0) {
                uint32_t in_bins = 0;
                for (int b = 0; b < 256; ++b) in_bins += sh.hist[b];
                uint32_t cum = total - in_bins;            // records at or below klo
                int b = 0;
                for (; b < 255; ++b) { cum += sh.hist[b]; if (cum >= K1) break; }
                sh.bin = b;
            }
            __syncthreads();
            const unsigned long long mybin = (unsigned long long)sh.bin;
            const unsigned long long width = 1ull << sh_bits;
            const unsigned long long cut = klo + (mybin + 1ull) * width;          // (bin 255 also holds everything beyond it)
            if (mybin < 255ull && cut < khi) khi = cut;
            klo = klo + mybin * width;
            __syncthreads();
            continue;
        }
        __syncthreads();
        if (total >= K1 || total >= nfin || r >= r_all) break;
        klo = khi;                                // too few: grow towards the expected count (at most 2x per step), and at least to the box
        float rn = r * fminf(2.0f, fmaxf(1.26f, cbrtf(1.5f * (float)K1 / (float)max(total, 1u))));
        if (r < r_box) rn = fmaxf(rn, r_box);
        r = fminf(rn, r_all);
        khi = ((unsigned long long)__float_as_uint(r * r) << 32) | 0xFFFFFFFFull;
    }
    total = min(total, (uint32_t)CAPB);            // (cannot bind: the loop ends with K1 <= total <= CAPB, or with the whole cloud)
    // bitonic sort of the first n2 = 2^m >= total entries (padding: all ones)
    uint32_t n2 = 2 * kCoopThreads;
    while (n2 < total) n2 <<= 1;
    for (uint32_t i = total + tid; i < n2; i += kCoopThreads) sh.buf[i] = ~0ull;
    __syncthreads();
    for (uint32_t kk = 2; kk <= n2; kk <<= 1) {
        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
            for (uint32_t t = (uint32_t)tid; t < (n2 >> 1); t += kCoopThreads) {
                const uint32_t i = 2 * t - (t & (jj - 1));          // the lower index of pair t at distance jj
                const uint32_t l = i + jj;
                const unsigned long long a = sh.buf[i], b = sh.buf[l];
                const bool up = (i & kk) == 0;
                if ((a > b) == up) { sh.buf[i] = b; sh.buf[l] = a; }
            }
            __syncthreads();
        }
    }
    return total;
}

}  // namespace tc
