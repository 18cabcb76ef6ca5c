// tde_vector_obs_dev.h — the device helpers of the vector observation, shared by the units whose kernels take it: tde_vector_obs.hip
// (vector_obs_kernel: slot 0 observes) and tde_agents.hip (agent_obs_kernel: any slot observes).  The per-wavefront LDS block, the
// ray / box slab test and the road channel's march over the class maps; include/tde_hip.h (tde_vector_obs) is the specification.
#pragma once
#include "tde_kernels.h"

namespace tde {

constexpr int kVoWaves = 4;         // envs per workgroup
#ifndef TDE_VO_BATCH
#define TDE_VO_BATCH 8
#endif
constexpr int kVoBatch = TDE_VO_BATCH;  // road samples whose look-ups are in flight together
constexpr float kVoSkipMargin = 0.05f;  // metres taken off a coarse tile's clearance: the fp32 error of the sample positions

struct VoWave {
    float4 box[TDE_MAX_AGENTS];                 // the other present agents: x, y, c, s
    float2 ext[TDE_MAX_AGENTS];                 // half length, half width
    unsigned long long key[TDE_MAX_AGENTS];     // (d2 bits << 32) | slot of the neighbour candidates, ~0 otherwise (by slot)
    float4 lbox[kWave];                         // a chunk of red stop lines: x, y, c, s
    float2 lext[kWave];                         //                            hl, hw
};

// per axis of a box: the ray's parameter interval inside the slab |o + t d| <= h
TDE_DEV void vo_slab(float o, float d, float h, float &lo, float &hi)
{
    if (d == 0.0f) {
        const bool in = -h <= o && o <= h;
        lo = in ? -INFINITY : INFINITY;
        hi = in ? INFINITY : -INFINITY;
    } else {
        const float ta = (-h - o) / d, tb = (h - o) / d;
        lo = fminf(ta, tb);
        hi = fmaxf(ta, tb);
    }
}

// entry distance of the ray (x0, y0) + t (ux, uy) into the box (b.x, b.y, c = b.z, s = b.w, half extents h); +inf on a miss
TDE_DEV float vo_ray_box(float x0, float y0, float ux, float uy, float4 b, float2 h)
{
    const float rx = x0 - b.x, ry = y0 - b.y;
    const float o0 = rx * b.z + ry * b.w, o1 = ry * b.z - rx * b.w;
    const float d0 = ux * b.z + uy * b.w, d1 = uy * b.z - ux * b.w;
    float lo0, hi0, lo1, hi1;
    vo_slab(o0, d0, h.x, lo0, hi0);
    vo_slab(o1, d1, h.y, lo1, hi1);
    const float tn = fmaxf(lo0, lo1), tf = fminf(hi0, hi1);
    return (tn <= tf && tf >= 0.0f) ? fmaxf(tn, 0.0f) : INFINITY;
}

// class | clearance << 2 of the coarse tile that holds the cell of (px, py) (the clamp of cell_class_lookup; tde_abi.h: cell_coarse)
TDE_DEV uint32_t vo_coarse(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    static_assert(TDE_COARSE_CELLS == 4, "coarse tiles of 4 x 4 cells");
    const uint32_t cx = (uint32_t)(int)fx >> 2, cy = (uint32_t)(int)fy >> 2;
    const uint32_t line = (uint32_t)m.coarse_base + ((cy >> 3) << (m.row_shift - 6)) + (cx >> 4);
    return w.cell_coarse[(line << 7) | (((cy & 7u) << 4) | (cx & 15u))];
}

// class of the sub-cell of (px, py) in its cell (meaningful for a MIXED cell; tde_abi.h: cell_sub, the rasteriser's subcell_class)
TDE_DEV uint32_t vo_subcell(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    const uint32_t ix = (uint32_t)(int)fx, iy = (uint32_t)(int)fy;
    const uint32_t tile = ((iy >> 2) << (m.row_shift - 3)) + (ix >> 3);
    const uint32_t bm = w.cell_sub[(uint32_t)m.cell_base + ((tile << 5) | (((iy & 3u) << 3) | (ix & 7u)))];
    const int sx = min((int)(__builtin_amdgcn_fractf(fx) * (float)TDE_CELL_SUB), TDE_CELL_SUB - 1);
    const int sy = min((int)(__builtin_amdgcn_fractf(fy) * (float)TDE_CELL_SUB), TDE_CELL_SUB - 1);
    return (bm >> (2 * (sy * TDE_CELL_SUB + sx))) & 3u;
}

// a point of a MIXED sub-cell: on the road when one of the cell's candidate triangles is within the threshold
TDE_DEV bool vo_mixed_off(const tde_world &w, const tde_map &m, float px, float py, float thr2)
{
    const uint32_t wd = cell_lookup(w, m, px, py);
    const float4 *recs = reinterpret_cast<const float4 *>(w.cell_tri);
    uint32_t cur = (wd >> 10) + (uint32_t)m.rec_base;
    const uint32_t end = cur + ((wd >> 2) & 255u);
    for (; cur < end; cur += 2) {                             // two records per trip (offroad_resolve's PAIR form)
        const float4 *r0 = recs + 3 * (size_t)cur, *r1 = recs + 3 * (size_t)(cur + 1 < end ? cur + 1 : cur);
        const float4 a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2];
        if (point_tri_d2_words(px, py, a0, a1, a2) <= thr2) return false;
        if (cur + 1 < end && point_tri_d2_words(px, py, b0, b1, b2) <= thr2) return false;
    }
    return true;
}

// the road channel of one ray over its samples j0..j1: the first j off the road, INT_MAX without one
TDE_DEV int vo_road(const tde_world &w, const tde_map &m, float x0, float y0, float ux, float uy, float step, int j0, int j1, float thr2)
{
    const int M = j1;
    for (int j = j0; j <= M;) {
        uint32_t cls[kVoBatch];
#pragma unroll
        for (int i = 0; i < kVoBatch; ++i) {                  // (independent look-ups, all in flight before the first is used)
            const float t = (float)min(j + i, M) * step;
            cls[i] = cell_class_lookup(w, m, x0 + t * ux, y0 + t * uy) & 3u;
        }
        const float t0 = (float)j * step;
        const uint32_t co = vo_coarse(w, m, x0 + t0 * ux, y0 + t0 * uy);
        // a FULL tile under sample j with clearance R: every sample closer than R to it lies in a FULL cell
        // (sample j itself lies in the tile: covered >= 0 exempts it; -1 = nothing proved)
        int covered = -1;
        if ((co & 3u) == TDE_CELL_FULL) covered = max(0, (int)(((float)(co >> 2) * TDE_COARSE_UNIT - kVoSkipMargin) / step));
        uint32_t empty = 0u, mixed = 0u;
#pragma unroll
        for (int i = 0; i < kVoBatch; ++i) {
            const bool in = j + i <= M && i > covered;
            empty |= (in && cls[i] == TDE_CELL_EMPTY) ? 1u << i : 0u;
            mixed |= (in && cls[i] == TDE_CELL_MIXED) ? 1u << i : 0u;
        }
        // the samples in MIXED cells: their sub-cell classes, fetched together; only a MIXED sub-cell walks the candidate triangles
        uint32_t sub_e = 0u, sub_m = 0u;
        if (mixed) {
            uint32_t sc[kVoBatch];
#pragma unroll
            for (int i = 0; i < kVoBatch; ++i) {
                const float t = (float)min(j + i, M) * step;
                sc[i] = vo_subcell(w, m, x0 + t * ux, y0 + t * uy);
            }
#pragma unroll
            for (int i = 0; i < kVoBatch; ++i) {
                const bool mi = ((mixed >> i) & 1u) != 0u;
                sub_e |= (mi && sc[i] == TDE_CELL_EMPTY) ? 1u << i : 0u;
                sub_m |= (mi && sc[i] == TDE_CELL_MIXED) ? 1u << i : 0u;
            }
        }
        const uint32_t off_now = empty | sub_e;
        for (uint32_t pend = off_now | sub_m; pend; pend &= pend - 1u) {    // in sample order
            const int i = __ffs((int)pend) - 1;
            const float t = (float)(j + i) * step;
            if ((off_now >> i) & 1u) return j + i;
            if (vo_mixed_off(w, m, x0 + t * ux, y0 + t * uy, thr2)) return j + i;
        }
        j += max(kVoBatch, covered + 1);
    }
    return INT_MAX;
}

}  // namespace tde
