// tde_render_scene.hip — the large-view rasteriser of tde_render_scene (BirdviewRecordingWrapper frames, render_mode="video", ref
// gym_env.py:295-297) and its launcher.  render_views_kernel stages a whole view in the 4 KB layer plane of one wavefront, so its
// views stop at 4096 pixels; here a view of up to 4096 x 4096 pixels is cut into kSceneTileH x kSceneTileW tiles (one 128-byte
// line per plane row), one wavefront per tile, each running raster_view's stages on its tile (tde_raster.h: RasterTile) -
// the pixels are those of the full-view specification, bit for bit.
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

struct SceneArgs {
    const tde_map *maps;
    const uint32_t *cell_word;
    const float *cell_tri;
    const tde_scenario *scn_tab;
    const double *wp_xy;
    const tde_stopline *stoplines;
    const tde_light_phase *phases;
    const float *x, *y, *psi, *len, *wid;
    const uint8_t *present;
    const int32_t *scn, *steps, *target_idx;
    const uint32_t *cell_cls2, *cell_sub;
    const uint8_t *cell_coarse;
    const tde_scene_view *views;
    uint8_t *out;
    float thr2, res, inv_res;
    uint32_t flags;                     // tde_config.flags
    int32_t rflags;                     // TDE_RENDER_*
    int32_t NW, A, B, H, W;
    int32_t ntc;                        // tiles per view row
    int32_t tpv;                        // tiles per view
    int32_t K8, K4;                     // raster_block_clearance(8 / 4, res)
    bool vec;                           // rows of every view 16-byte aligned (W % 16 == 0 and out 16-byte aligned)
};

// the occupancy of render_views_kernel (eight wavefronts per SIMD, 5 KB of LDS each), four tiles per workgroup, tiles [t0, n_tiles)
// of the request (a loop over tiles inside the kernel keeps the arguments live across the raster stages: 60 VGPRs spilled)
__global__ __launch_bounds__(kWave * kViewsPerGroup) __attribute__((amdgpu_waves_per_eu(TDE_RENDER_WAVES, TDE_RENDER_WAVES), amdgpu_num_sgpr(TDE_RENDER_SGPRS)))
void render_scene_kernel(SceneArgs sa, int64_t t0, int64_t n_tiles)
{
    __shared__ RasterScratch Sall[kViewsPerGroup];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63u);
    RasterScratch &S = Sall[wv];
    const int64_t plane = (int64_t)sa.H * sa.W;
    const int64_t t = t0 + (int64_t)blockIdx.x * kViewsPerGroup + wv;
    if (t >= n_tiles) return;
    {
        const int64_t view = t / sa.tpv;
        const int rem = (int)(t - view * sa.tpv), tr = rem / sa.ntc, tc = rem - tr * sa.ntc;
        const int r0 = tr * kSceneTileH, c0 = tc * kSceneTileW;
        RasterTile T;
        T.hu = (0.5f * (float)sa.H - 0.5f) - (float)r0;       // exact: half-integers below 2048
        T.hv = (0.5f * (float)sa.W - 0.5f) - (float)c0;
        T.vh = min(kSceneTileH, sa.H - r0); T.vw = min(kSceneTileW, sa.W - c0);
        T.ld = sa.W; T.plane = plane; T.vec = sa.vec;
        uint8_t *out = sa.out + view * 3 * plane + (int64_t)r0 * sa.W + c0;
        const tde_scene_view cam = sa.views[view];
        const int e = cam.env;
        if (e < 0 || e >= sa.B) {                             // a view of no env: zeros
            raster_tile_out(T, out, nullptr, lane);
            return;
        }
        const int64_t g0 = (int64_t)e * sa.A;
        const int scn = sa.scn[e];
        const int4 sc = reinterpret_cast<const int4 *>(sa.scn_tab)[scn];           // map, wp_n, start_heading, pad
        RasterJob J;
        J.cell_word = sa.cell_word; J.cell_tri = sa.cell_tri; J.cell_cls2 = sa.cell_cls2; J.cell_sub = sa.cell_sub;
        J.cell_coarse = sa.cell_coarse;
        J.m = sa.maps[sc.x];
        J.stoplines = sa.stoplines + J.m.stop_base;
        J.wp = sa.wp_xy + (int64_t)scn * sa.NW * 2;
        J.lights = (sa.flags & TDE_F_TRAFFIC_LIGHTS) != 0 && J.m.n_stop > 0;
        J.red = 0u;
        if (J.lights) {
            tde_world w{};
            w.phases = sa.phases;
            J.red = red_mask(w, J.m, sa.steps[e]);
        }
        J.n_wp = sc.y; J.ti = sa.target_idx[e]; J.A = sa.A;
        J.ex = cam.x; J.ey = cam.y;
        sincos_f32(cam.psi, J.se, J.ce);                     // (the sincos of the ego's pose in render_views_kernel)
        J.H = kSceneTileH; J.W = kSceneTileW; J.ns = 1; J.phase = 0; J.flags = sa.rflags;
        J.res = sa.res; J.inv_res = sa.inv_res; J.thr2 = sa.thr2;
        J.K8 = sa.K8; J.K4 = sa.K4;
        J.out = out;
        J.ring = nullptr;
        J.fresh = false;
        raster_view<0, StateAgents, true>(S, J, StateAgents{sa.x, sa.y, sa.psi, sa.len, sa.wid, sa.present, g0}, nullptr, T);
    }
}

}  // namespace tde

namespace tde_host {

int launch_render_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_scene_view *views,
                        int32_t n_views, int32_t H, int32_t W, float fov, int32_t flags, uint8_t *out, void *stream)
{
    tde::SceneArgs sa;
    sa.maps = world->maps; sa.cell_word = world->cell_word; sa.cell_tri = world->cell_tri; sa.scn_tab = world->scn;
    sa.wp_xy = world->wp_xy; sa.stoplines = world->stoplines; sa.phases = world->phases;
    sa.x = st->x; sa.y = st->y; sa.psi = st->psi; sa.len = st->len; sa.wid = st->wid; sa.present = st->present;
    sa.scn = st->scn; sa.steps = st->steps; sa.target_idx = st->target_idx;
    sa.cell_cls2 = world->cell_cls2; sa.cell_sub = world->cell_sub; sa.cell_coarse = world->cell_coarse;
    sa.views = views; sa.out = out;
    sa.thr2 = cfg->offroad_threshold_squared ? cfg->offroad_threshold : cfg->offroad_threshold * cfg->offroad_threshold;
    sa.res = fov / (float)W; sa.inv_res = 1.0f / sa.res;
    sa.flags = cfg->flags; sa.rflags = flags;
    sa.NW = world->NW; sa.A = st->A; sa.B = st->B; sa.H = H; sa.W = W;
    const int ntr = (H + tde::kSceneTileH - 1) / tde::kSceneTileH;
    sa.ntc = (W + tde::kSceneTileW - 1) / tde::kSceneTileW;
    sa.tpv = ntr * sa.ntc;
    sa.K8 = tde::raster_block_clearance(8, sa.res); sa.K4 = tde::raster_block_clearance(4, sa.res);
    sa.vec = (W % 16) == 0 && ((uintptr_t)out & 15u) == 0;
    const int64_t n_tiles = (int64_t)n_views * sa.tpv;
    // one wavefront per tile, at most 2^20 workgroups (4 Mi tiles: 1024 views of 4096 x 4096) per launch
    constexpr int64_t kMaxTiles = ((int64_t)1 << 20) * tde::kViewsPerGroup;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += kMaxTiles) {
        const int64_t n = n_tiles - t0 < kMaxTiles ? n_tiles - t0 : kMaxTiles;
        const unsigned ng = (unsigned)((n + tde::kViewsPerGroup - 1) / tde::kViewsPerGroup);
        tde::render_scene_kernel<<<ng, tde::kWave * tde::kViewsPerGroup, 0, (hipStream_t)stream>>>(sa, t0, n_tiles);
        const int rc = launch_status("tde_render_scene");
        if (rc) return rc;
    }
    return 0;
}

}  // namespace tde_host
