/*
 * tde_hip.h — C-ABI of libtde_hip.so: the MI355X (gfx950) implementation of the per-timestep env step path of
 * inverted-ai/torchdriveenv.  Plain pointers (DEVICE memory unless stated), sizes, and a HIP stream passed as
 * void* (hipStream_t; NULL = the default stream).  No torch types.  All entry points are asynchronous on the given
 * stream, allocate nothing, and return 0 on success or a hipError_t value (message: tde_last_error()).
 *
 * Each entry point names the reference interface it replaces (file:line into /root/reference/torchdriveenv/).
 * The reference has no FFI of its own (it is pure Python over torchdrivesim); INTEGRATION.md shows the ctypes stub a
 * maintainer would add and how GymEnv/WaypointSuiteEnv would call it.
 *
 * Struct arguments (tde_config, tde_world, tde_state, tde_rollout, tde_eval: include/tde_abi.h) are HOST structs whose pointer
 * members are device pointers; they are copied by value into the kernel arguments at launch.
 */
#ifndef TDE_HIP_H
#define TDE_HIP_H

#include "tde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_API __attribute__((visibility("default")))

/* TDE_ABI_VERSION the library was built with. */
TDE_API int tde_abi_version(void);

/* Message of the last failing call on this thread ("" if none). */
TDE_API const char *tde_last_error(void);

/* Test / tuning hook (no reference counterpart): tde_env_rollout and tde_env_step each have several kernel forms (one, two
 * or three wavefronts per 64 agent slots) and pick one by group shape and batch size; this forces a form for the calling
 * process - 0 = automatic (default), rollout_team 1 | 2 | 3, step_team 1 | 3 (2 at 128 slots) - so that every form can be held against the
 * oracle and A/B-timed.  A forced three-wavefront form still needs 8, 16 or 32 agents per env; at 128 agent slots per env
 * rollout_team / step_team 1 = the one-role kernel, 2 = the two-role kernel in its four-wavefront form at any batch size (the
 * library itself takes the eight-wavefront form up to half a residency round), 3 leaves the choice as it is.  The two values are atomics: a call from one thread while another launches is a race on the choice, not on memory. */
TDE_API int tde_kernel_override(int rollout_team, int step_team);

/* ---- operator level: the SimulatorInterface methods GymEnv calls ------------------------------------ */

/* simulator.step(action) restricted to the kinematic model — KinematicBicycle.step for n agents.
 * Replaces: gym_env.py:117 (simulator.step), model built at gym_env.py:245-247 (lr = rear_axis_offset).
 * x,y,psi,v: in/out [n]; lr [n]; present [n] or NULL; action [n][2] = (acceleration, steering). */
TDE_API int tde_kinematics_step(int64_t n, float *x, float *y, float *psi, float *v, const float *lr,
                                const uint8_t *present, const float *action, float dt, void *stream);

/* simulator.compute_collision() > 0 per agent: strict OBB overlap with any other present agent of the same env.
 * Replaces: gym_env.py:143, 415, 428 (CollisionMetric.nograd, gym_env.py:48).  All arrays [B*A]; out u8 [B*A]. */
TDE_API int tde_compute_collision(int32_t B, int32_t A, const float *x, const float *y, const float *psi,
                                  const float *len, const float *wid, const uint8_t *present, uint8_t *out,
                                  void *stream);

/* simulator.compute_offroad() > 0 per agent: a box corner farther than `threshold` from the drivable mesh of the
 * env's map.  Replaces: gym_env.py:142, 415, 427 (mesh: gym_env.py:184,260).  map_of_env [B]; out u8 [B*A]. */
TDE_API int tde_compute_offroad(int32_t B, int32_t A, const float *x, const float *y, const float *psi,
                                const float *len, const float *wid, const uint8_t *present, const tde_world *world,
                                const int32_t *map_of_env, float threshold, uint8_t *out, void *stream);

/* Fused kinematics + all-pairs collision for every agent (BASELINE.json configs[1]: "bicycle kinematics + OBB
 * collision only").  action [B*A][2].  Replaces: gym_env.py:117 followed by :143. */
TDE_API int tde_kin_collide_step(int32_t B, int32_t A, float *x, float *y, float *psi, float *v, const float *lr,
                                 const float *len, const float *wid, const uint8_t *present, const float *action,
                                 float dt, uint8_t *collided, void *stream);

/* The part of the step the reference owns, batched over n envs: environment_steps += 1 (gym_env.py:116),
 * WaypointSuiteEnv.get_reward (:396-411), check_reach_target (:391-394), is_terminated (:413-417), is_truncated
 * (:134-135), get_info terms (:419-437), waypoint advance (:378-383).
 * pre_* = ego state before simulator.step (last_x.. :371-375), x.. = after; flags u8 [n]; tl_violation may be NULL.
 * wp_xy f64 [S][NW][2], wp_n [S], scn [n]; steps/target_idx/reached in/out [n];
 * info f64 [n][4] = psi_smoothness, speed_smoothness, psi_reward, dist_reward (or NULL); info_reached [n] or NULL. */
TDE_API int tde_waypoint_reward(const tde_config *cfg, int32_t n, const float *pre_x, const float *pre_y,
                                const float *pre_psi, const float *pre_v, const float *x, const float *y,
                                const float *psi, const float *v, const uint8_t *offroad, const uint8_t *collided,
                                const uint8_t *tl_violation, const double *wp_xy, const int32_t *wp_n, int32_t NW,
                                const int32_t *scn, int32_t *steps, int32_t *target_idx, int32_t *reached,
                                float *reward, uint8_t *terminated, uint8_t *truncated, double *info,
                                int32_t *info_reached, void *stream);

/* ---- env level: the fused hot path ---------------------------------------------------------------------------- */

/* WaypointSuiteEnv.reset for the envs selected by mask (u8 [B], NULL = all): scenario draw, start pose/speed/heading
 * noise, spawn of NPC slots, counters.  Replaces: gym_env.py:319-367 + the initial tensors of build_simulator
 * (:192-198, :241-247).  Network parts (IAI initialize, :236-238) are out of scope. */
TDE_API int tde_env_reset(const tde_config *cfg, const tde_world *world, const tde_state *state, const uint8_t *mask,
                          void *stream);

/* One timestep of every env in ONE kernel: SingleAgentWrapper.step -> WaypointSuiteEnv.step -> GymEnv.step
 * (gym_env.py:453-461, 369-389, 115-120): bicycle kinematics, heuristic NPC controller (in place of the IAI call,
 * :285-294), replay override (:275-283), all-pairs OBB collision, drivable-mesh offroad, WaypointSuite reward,
 * termination/truncation, info, waypoint advance, and (TDE_F_AUTORESET) in-place re-spawn of finished envs.
 * Reads state->action [B][2]; writes state in place.
 * Per-slot routes (tde_state.slot_route != NULL; A >= 4, fewer is rejected): slot a > 0 of env e with word w = slot_route[e * A + a]
 * != 0 steps as if its spawn record said route = (w & 0xFFFFF) - 1 and route_n = w >> 20 - its target is route_xy[route][route_wp]
 * while state.route_wp < route_n, under TDE_F_NPC - everything else (replay row, attributes, the re-spawn under TDE_F_AUTORESET) stays
 * the record's; w == 0: the record's route, as without the array.  The step then always runs its routed one-role kernel
 * (env_step_routed_kernel; tde_kernel_override and the lookup caches do not apply) and does not write the array: after an in-place
 * re-spawn call tde_near_field_spawn before the next step, as after tde_env_reset.
 * (At 128 agent slots the kernel reads (cfg, world, state) from an immutable argument block the library keeps in device memory, one
 *  per distinct argument set, uploaded on `stream` at first use; every other form takes them by value.  INTEGRATION.md, section 1.) */
TDE_API int tde_env_step(const tde_config *cfg, const tde_world *world, const tde_state *state, void *stream);

/* K consecutive timesteps with the ego actions taken from a resident [K][B][2] buffer (open-loop / action-repeat
 * rollouts; how bench.py drives the path without a host round trip per step).  Per-step reward [K][B] and done bits
 * [K][B] are written to `rollout`. */
/* (tde_env_rollout, tde_env_step_render, tde_forecast_agents, tde_forecast_scene and tde_score_plans_scene read every slot's route from
 * its spawn record: each rejects a state with slot_route != NULL - "<entry point>: state.slot_route is set: ..." - rather than drive the
 * spawned agents to a standstill.  tde_plan_action, tde_score_plans(_forecast), tde_vector_obs, the rasterisers, tde_env_post_step,
 * tde_env_reset(_to) and tde_eval_advance do not read routes and take such a state as any other.) */
TDE_API int tde_env_rollout(const tde_config *cfg, const tde_world *world, const tde_state *state,
                            const tde_rollout *rollout, void *stream);

/* GymEnv.get_obs / render: simulator.render_egocentric() for the ego of every env -> uint8 [B][3*n_stack][H][W]
 * (channels first, obs space gym_env.py:95; frame stack as VecFrameStack(n_stack=3, channels_order="first"),
 * examples/rl_training.py:160).  Replaces: gym_env.py:122-124, 152-155.  Layer/palette definition: tde_abi.h. */
TDE_API int tde_render_ego(const tde_config *cfg, const tde_world *world, const tde_state *state,
                           const tde_render *render, void *stream);

/* Camera pose of one tde_render_scene view, world coordinates: the view of env `env` is centred on (x, y), image rows up along
 * heading psi. */
typedef struct tde_scene_view {
    int32_t env;
    float x, y, psi;
} tde_scene_view;

/* BirdviewRecordingWrapper(res=(H, W), fov) frames (render_mode="video", gym_env.py:295-297; GymEnv.close writes them,
 * :172-176): views[i] (DEVICE [n_views]) -> out[i] = uint8 [3][H][W] (DEVICE [n_views][3][H][W]), any H, W in [1, 4096], any
 * camera pose.  Pixels are tde_render_ego's specification (tde_abi.h, oracle tde_render_env) with the camera pose in place of the
 * ego's: u = (H/2 - 0.5) - r, v = (W/2 - 0.5) - c, world = cam + u (ax, ay) + v (bx, by), res = fov / W; layers, palette,
 * waypoint discs (the env's target_idx), stop-line colours (the env's steps), agent draw order and flags (TDE_RENDER_*) as there;
 * slot 0 is painted as the ego whatever the camera.  A view whose env is outside [0, B) is written as zeros.  n_views == 0 is a
 * no-op.  Rejected: H or W outside [1, 4096], fov not finite or <= 0, n_views < 0, views or out NULL with n_views > 0.
 * One wavefront per 32 x 128 tile of a view. */
TDE_API int tde_render_scene(const tde_config *cfg, const tde_world *world, const tde_state *state,
                             const tde_scene_view *views, int32_t n_views, int32_t H, int32_t W, float fov, int32_t flags,
                             uint8_t *out, void *stream);

/* The re-spawn of the envs an SB3-style auto-reset has just seen finish, and their first observation, in ONE call: tde_env_reset
 * for the envs with mask[e] != 0 (uint8 [B], required) followed by tde_render_ego of exactly those views - their newest frame
 * rendered again in place, their older stack frames blanked (render->fresh and render->only are set to `mask` by the call, so its entries must be 0 or 1: the rasteriser reads bits 0-1 of a fresh byte; phase
 * = the phase of the LAST full render).  Replaces: the reset() + get_obs() a VecEnv issues for finished envs
 * (gym_env.py:319-349, 122-124; examples/rl_training.py:159-160). */
TDE_API int tde_env_reset_render(const tde_config *cfg, const tde_world *world, const tde_state *state, const uint8_t *mask,
                                 const tde_render *render, void *stream);

/* One timestep + (render != NULL) the birdview of every env, as n_streams contiguous sub-batches of the batch, sub-batch i
 * launched on streams[i] (hipStream_t; the step, then the rasteriser): GymEnv.step followed by get_obs (gym_env.py:115-124)
 * for every env, the step of one sub-batch overlapping the rasteriser of another - both kernels are latency-bound alone
 * (DESIGN.md section 5, round 3).  Results are those of tde_env_step + tde_render_ego on the whole batch (envs are independent
 * and the reset RNG is keyed by the global env index: each sub-batch runs with env_base advanced to its first env).
 * Sub-batches are cut at multiples of 64 envs.  The caller orders the streams against the producer of state->action and the
 * consumer of the outputs (events); consecutive calls on the same streams are ordered per sub-batch, which is all the
 * path needs.  n_streams in [1, 16]. */
TDE_API int tde_env_step_render(const tde_config *cfg, const tde_world *world, const tde_state *state,
                                const tde_render *render, void *const *streams, int32_t n_streams);

/* Compact kinematic observation of every env's ego, float32 [B][8] (no reference counterpart; the reference only has
 * the birdview of gym_env.py:122-124): x, y, psi, v, offset of the current target waypoint in the ego frame (forward,
 * left; 0 when the route is finished, gym_env.py:378-383), 1 while a target exists, environment_steps.  One launch
 * instead of a dozen framework ops per step in closed-loop use. */
TDE_API int tde_state_obs(const tde_world *world, const tde_state *state, float *out, void *stream);

/* Infraction MAGNITUDES of every env's ego, float32 [B][4] = (offroad, collision, number of overlapping agents, 0): what the
 * reference's info dict holds under "offroad" / "collision" - simulator.compute_offroad() and compute_collision() for the exposed
 * agent, gym_env.py:427-428 (Monitor logs them, examples/rl_training.py:128) - where the step path only needs `> 0`.  offroad = sum
 * over the four box corners of clamp(dist - offroad_threshold, min = 0), dist = distance of the corner to the drivable mesh (the
 * SQUARED distance under tde_config.offroad_threshold_squared); collision = sum over the other present agents whose box overlaps
 * the ego's of the IoU of the two boxes (CollisionMetric.nograd's published form, gym_env.py:48).  Evaluated on the state as it
 * is: call it after a step WITHOUT TDE_F_AUTORESET and before tde_env_reset re-spawns the finished envs.  Cost: a corner within a
 * few metres of the mesh is a handful of table look-ups; the nearest triangle of a corner r metres away is found by scanning the
 * grid cells of a square of side ~ 2r around it - microseconds up to ~ 10 m - and, once that square would hold more cells than
 * (eight times) the map has triangles, by the definition itself: the minimum over all the map's triangles (tde_world.tri), 64 per
 * trip - tens of microseconds for an ego that keeps driving hundreds of metres off a junction map under
 * terminated_at_infraction = 0 (a millisecond by the scan alone).  The same holds for tde_state.magnitudes of tde_env_step. */
TDE_API int tde_ego_infractions(const tde_config *cfg, const tde_world *world, const tde_state *state, float *out, void *stream);

/* What follows a step that was launched WITHOUT TDE_F_AUTORESET, in one launch (one wavefront per env):
 *  (a) magnitudes != NULL: magnitudes[e] = tde_ego_infractions' four values for the state that step left - computed only for the
 *      envs whose ego the step flagged (state.collided / state.offroad of slot 0; a magnitude is zero without its flag), so the
 *      flags in `state` must be those of that step;
 *  (b) with TDE_F_AUTORESET in config->flags: tde_env_reset for the envs the step finished (terminated | truncated; the two
 *      arrays keep the step's values) and, when state.obs is set, the compact observation of their new episode.
 * step (no auto-reset) + this = the one-launch step's results, plus the reference's info["offroad" | "collision"] values
 * (gym_env.py:427-428).  Replaces: simulator.compute_offroad() / compute_collision() for the exposed agent followed by the
 * reset() a VecEnv issues for finished envs (gym_env.py:319-349; examples/rl_training.py:159-160). */
TDE_API int tde_env_post_step(const tde_config *config, const tde_world *world, const tde_state *state, float *magnitudes, void *stream);

/* (ABI 11) Fills the world's first-step gap cache (tde_world.first_gap, see tde_first_gap in tde_abi.h) for `config`: per (scenario, NPC
 * slot) what the NPC controller finds on the FIRST step of an episode apart from the ego - min(leader gap over the scenario's other
 * NPCs at their spawn poses, gap to a stop line that is red at step one) - keyed by the controller hash of (config, world).  With it
 * the role-split kernels give a re-spawned env its first NPC actions (TDE_F_NPC_FIRST_STEP; the reference's NPCs are driven from the
 * first simulator.step: IAIWrapper, gym_env.py:285-294) from one exact test against the ego's row instead of the controller's sweep;
 * without it (or with entries of another configuration) they run the whole controller: same results either way.
 * tde_env_step / tde_env_rollout call this themselves, on their stream, the first time they meet a (world, configuration) pair (a
 * small per-process memo of the pairs already served): a caller only needs it to choose WHEN the launch happens (e.g. outside a
 * stream capture).  One launch of n_scn * A lanes; up to 128 agent slots per env (at 128 slots the two-role one-step kernel reads
 * the cache; the 128-slot rollout kernel does not).  This launch alone writes the cache: no step or rollout kernel does. */
TDE_API int tde_first_gaps(const tde_config *config, const tde_world *world, void *stream);

/* Near-field traffic at reset (the stand-in for iai_conditional_initialize, gym_env.py:232-238, iai.py:6-60): fills the free slots of
 * every env with mask[e] != 0 (uint8 [B]; NULL: all envs) from the candidate table `nf` (tde_abi.h: tde_near_field), on the state
 * as the preceding tde_env_reset / in-place re-spawn left it.  For env e (scenario s = state.scn[e], counter c = state.episode[e],
 * g = config.env_base + e): free slots = slots 1..A-1 whose spawn record has present == 0, ascending; n_present = present slots,
 * n_in = those with d2 < radius^2 from the ego; T = max(0, min(free, max(count - n_present, density) - n_in)).  Candidate i has
 * priority word (i & 3) of philox(seed, g, c, i >> 2, TDE_NF_TAG) and is visited by ascending (priority, i); it is accepted when
 * it is not fixed, clear_ego^2 <= d2 <= radius^2, no neighbour of it is accepted and fewer than T are.  d2 = dx*dx + dy*dy in
 * float64 of the float32 positions.  The k-th accepted candidate goes to the k-th free slot: pose, attributes, vdes, v = (float)
 * (u01(word (i & 3) of philox(seed, g, c, 512 + (i >> 2), TDE_NF_TAG)) * vdes), route_wp = 0, present = 1, collided = offroad = 0;
 * the env's act_cache key (if any) and the written slots' slot_cache entries are invalidated.  One wavefront per env.
 * Per-slot routes (state.slot_route != NULL): for every env with mask[e] != 0 - whatever T is, and also when state.scn[e] is outside
 * [0, nf.S) - the entries of ALL slots 1..A-1 are written: the slot that received candidate i with cand.route != 0 gets
 * cand.route | cand.route_n << 20 and state.route_wp = cand.route_wp (instead of 0); every other slot gets 0, so no word of an earlier
 * episode survives a re-spawn.  Entry 0 of an env (the ego's) and the entries of the other envs are not written.  With
 * state.slot_route == NULL the candidates' route words are not read.  Acceptance order, Philox words and speeds do not depend on it.
 * Rejected: NULL cfg / world / state / nf or nf tables, nf.S != world.n_scn, nf.A != state.A (a power of two <= 128), NC or K out
 * of range.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_near_field_spawn(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_near_field *nf,
                                 const uint8_t *mask, void *stream);

/* Vector observation of every env with only[e] != 0 (uint8 [B]; NULL: all envs) -> out[e] = float32 [D], D = TDE_VO_EGO + TDE_VO_NBR *
 * vo.k_nbr + TDE_VO_RAY * vo.n_rays (tde_abi.h: struct tde_vector_obs); the other rows are not written.  No reference counterpart.
 * Every expression below is float32 with one rounding per written operation (no contraction), so a restatement matches it bit
 * for bit.  Env e: s = state.scn[e], m = world.maps[world.scn[s].map], ego = slot 0 (x0, y0, psi0, v0, len0, wid0) with
 * (s0, c0) = sincos_f32(psi0); every agent's (c, s) is sincos_f32 of its psi (tde_device.h); "frame(dx, dy)" = (dx*c0 + dy*s0,
 * dy*c0 - dx*s0), (forward, left).
 * Ego block [0, 10): v0, len0, wid0; for j = target_idx and target_idx + 1: frame((float)wp.x - x0, (float)wp.y - y0) of waypoint
 * j of scenario s when j < wp_n, else (0, 0) (2 + 2 values; the first pair is tde_state_obs's); (float)min(max(wp_n - target_idx,
 * 0), 2); (float)steps / (float)config.max_steps; 1 when m.n_stop > 0 and m.cycle_steps > 0, else 0.
 * Neighbour block, k_nbr entries of 9 from 10: the present slots a in 1..A-1 with d2 < nbr_radius*nbr_radius, where dx = x_a - x0,
 * dy = y_a - y0, d2 = dx*dx + dy*dy, ordered by (d2, a), the first k_nbr of them: 1, frame(dx, dy), cr = c_a*c0 + s_a*s0, sr =
 * s_a*c0 - c_a*s0, v_a*cr - v0, v_a*sr, len_a, wid_a.  Entries past the last neighbour are zeros.
 * Ray block, n_rays rays of 3 from 10 + 9 * k_nbr: ray k has the world direction ux = rx*c0 - ry*s0, uy = rx*s0 + ry*c0, (rx, ry) =
 * vo.ray_dir[k], and M = ray_range / ray_step.
 *   road  (float)j * ray_step for the first j in 1..M whose sample (x0 + ((float)j * ray_step)*ux, y0 + ((float)j * ray_step)*uy)
 *         is farther than the offroad threshold from the map's mesh (the predicate of one box corner of the step: d^2 > thr2 with
 *         thr2 as config.offroad_threshold_squared selects; the grid index equals the brute force over m's triangles), else
 *         ray_range
 *   car   min(ray_range, least entry distance over the present slots a in 1..A-1), the box of a = (x_a, y_a, c_a, s_a, 0.5f*len_a,
 *         0.5f*wid_a)
 *   red   the same over the stop lines q of m (box x, y, c, s, hl, hw) whose light is red at state.steps[e]: with
 *         TDE_F_TRAFFIC_LIGHTS in config.flags, (red_mask >> (light & 31)) & 1 of the phase of steps % cycle_steps (the lines
 *         tde_render_ego paints red); none without the flag
 *   entry distance of a box (bx, by, bc, bs, h0, h1): rx = x0 - bx, ry = y0 - by; o0 = rx*bc + ry*bs, o1 = ry*bc - rx*bs; d0 =
 *         ux*bc + uy*bs, d1 = uy*bc - ux*bs; per axis i: d_i == 0 -> [-inf, +inf] when -h_i <= o_i <= h_i, else a miss; otherwise
 *         ta = (-h_i - o_i) / d_i, tb = (h_i - o_i) / d_i, [min(ta, tb), max(ta, tb)]; tn = max of the lows, tf = min of the
 *         highs; a hit when tn <= tf and tf >= 0, at max(tn, 0)
 * One wavefront per env, four envs per workgroup, one lane per ray.  Rejected: NULL cfg / world / state / vo / out, ray_dir NULL
 * with n_rays > 0, k_nbr or n_rays out of range, nbr_radius / ray_range / ray_step not finite or <= 0, ray_range / ray_step not an
 * integer in [1, TDE_VO_MAX_SAMPLES], config.max_steps < 1.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_vector_obs(const tde_config *cfg, const tde_world *world, const tde_state *state, const struct tde_vector_obs *vo,
                           const uint8_t *only, float *out, void *stream);

/* (ABI 13) Sampling planner: for every env with only[e] != 0 (uint8 [B]; NULL: all envs) action[e] = (acceleration, steering) for
 * the ego (slot 0) on the state as it is; the other rows of action (and of diag) are not written.  No reference counterpart (its
 * policies come from outside: examples/rl_training.py).  plan = tde_planner (tde_abi.h, a HOST struct with its lattice inline).
 * Every expression below is float32 with one rounding per written operation (no contraction); (s, c) of a heading = sincos_f32
 * (tde_device.h); bicycle and obb_overlap are the step's own (tde_device.h); tests/planner_ref.py restates this in numpy.
 * Env e: s = state.scn[e], m = world.maps[world.scn[s].map], wp_n = world.scn[s].wp_n, ego = slot 0: (x0, y0, psi0, v0), inv_lr =
 * 1.0f / lr0, hl0 = 0.5f * len0, hw0 = 0.5f * wid0, dt = config.dt, H = plan.horizon, rr = (float)config.reach_radius.
 * Candidate i in [0, n_a * n_s): a = accel[i / n_s], d = steer[i % n_s].
 *   Trajectory  (x, y, psi, v) = the ego's state; for h = 1..H: a_h = 0.0f when v + a * dt < 0.0f (a candidate does not plan to
 *               reverse), else a; bicycle(x, y, psi, v, inv_lr, a_h, d, dt) gives s_h; (sn, cs) = sincos_f32(psi) of s_h.
 *   Others      every present slot j in 1..A-1, (c_j, s_j) = sincos_f32(psi_j): at step h the box (x_j + (float)h * ((v_j * c_j) *
 *               dt), y_j + (float)h * ((v_j * s_j) * dt), c_j, s_j, 0.5f * len_j + margin, 0.5f * wid_j + margin).
 *   Failure     f = the first h in 1..H at which one of these holds for s_h, else H + 1:
 *               (i)   a corner of the box (x, y, cs, sn, hl0, hw0) is off the road: the step's predicate (tde_compute_offroad: corners
 *                     FL, FR, RR, RL = (x +- hl0*cs) -+ hw0*sn, (y +- hl0*sn) +- hw0*cs; d^2 > thr2 with thr2 as
 *                     config.offroad_threshold_squared selects; the grid index equals the brute force over m's triangles);
 *               (ii)  obb_overlap(ego box; box of j at step h) for some j (the ego's box first, not inflated);
 *               (iii) with TDE_F_TRAFFIC_LIGHTS, m.n_stop > 0 and m.cycle_steps > 0: obb_overlap(ego box; x, y, c, s, hl, hw of stop
 *                     line q of m) for a q with (red >> (light_q & 31)) & 1, red = the red mask of the phase of (state.steps[e] + h) %
 *                     cycle_steps - the value of environment_steps the real step would judge s_h under.
 *   Cost        ti = state.target_idx[e], gain = 0, sv = 0; when ti < wp_n: (wx, wy) = ((float)wp.x, (float)wp.y) of waypoint ti, dx =
 *               wx - x0, dy = wy - y0, dp = sqrtf(dx*dx + dy*dy).  At every step h < f, in this order, on s_h:
 *                 when ti < wp_n: dx = wx - x, dy = wy - y, dn = sqrtf(dx*dx + dy*dy); gain = gain + (dp - dn); dp = dn; when dn < rr
 *                   (check_reach_target, gym_env.py:391-394, in float32): ti = ti + 1 and, when still ti < wp_n, (wx, wy) = waypoint
 *                   ti and dp = its distance from s_h by the same expression;
 *                 ev = v - (ti < wp_n ? v_target : 0.0f) (a finished route plans a stop); sv = sv + ev * ev.
 *               run = (w_speed * sv + w_steer * (d * d)) - w_progress * gain;
 *               cost = (float)(H + 1 - f) * TDE_PLAN_FAIL_UNIT + fminf(fmaxf(run + TDE_PLAN_RUN_BIAS, 0.0f), TDE_PLAN_RUN_MAX):
 *               a candidate that fails earlier costs more than any that fails later or never, whatever the weights.
 *   Winner      the least (k, i), k = the cost's bits b as an ordered integer (b ^ 0x80000000 for b >= 0 as int32, else ~b): exact ties
 *               go to the lower index; when every candidate fails this picks the one that fails last.
 *   action[e] = (a_1 of the winner - its a after the no-reverse rule at the state as it is -, its d);
 *   diag[e]   = (winner, its f, its cost, the number of candidates with f == H + 1) when diag != NULL.
 * One wavefront per env, one lane per candidate, four envs per workgroup; reads state only.  Rejected: NULL cfg / world / state /
 * plan / action, n_a or n_s < 1 or n_a * n_s > TDE_PLAN_MAX_CAND, horizon outside [1, TDE_PLAN_MAX_H], an accel outside [-1, 1] or a
 * steer outside [-0.3, 0.3] (gym_env.py:83-84) or not finite, v_target / margin / a weight negative or not finite, config.dt not
 * finite or <= 0.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_plan_action(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_planner *plan,
                            const uint8_t *only, float *action, tde_plan_diag *diag, void *stream);

/* (ABI 14) Judge caller-given action sequences: for every env with only[e] != 0 (uint8 [B]; NULL: all envs) and every sequence n
 * in [0, set.N): cost[e][n] and fail_step[e][n]; with action / diag != NULL also the winner's first action and a diag row.  Rows of
 * every output with only[e] == 0 are not written.  No reference counterpart.  set = tde_plan_set (tde_abi.h; set.seq on the device,
 * [B][N][K][2] float32); plan supplies H = plan.horizon, margin, v_target and the three weights - its lattice (accel, steer, n_a,
 * n_s) is not read.  T = set.tail, L = set.knot_len, K = set.K.  Everything not restated here is tde_plan_action's, expression for
 * expression (env quantities, Others, the three Failure predicates, the Cost walk, the ordered key); tests/plan_set_ref.py restates
 * this in numpy.
 *   Knots       step h in 1..H uses knot k_h = min((h - 1) / L, K - 1) of sequence n: a = fminf(fmaxf(seq[e][n][k_h][0], -1.0f), 1.0f),
 *               d = fminf(fmaxf(seq[e][n][k_h][1], -0.3f), 0.3f) (TDE_PLAN_BOX_ACCEL / _STEER; a NaN becomes the lower bound; the
 *               kernel cannot reject device values).
 *   Horizon     for h = 1..H: tde_plan_action's Trajectory step with this step's (a, d) - a_h = 0.0f when v + a * dt < 0.0f, else a -
 *               and its Failure predicates on s_h (red mask of state.steps[e] + h, the others' boxes at step h); at every step
 *               h < f its Cost walk (gain, sv, the waypoint advance).
 *   Brake tail  a sequence with no failure in 1..H goes on for t = 1..T with a = -1.0f and the d of step H.  At the first t with
 *               v + a * dt < 0.0f it ends, safe (it stands as far as this action box can stop it).  Otherwise bicycle(x, y, psi, v,
 *               inv_lr, a, d, dt) and the three Failure predicates at step H + t (red mask of state.steps[e] + H + t, the others'
 *               boxes (float)(H + t) steps ahead); a failure gives f = H + t.  The tail adds nothing to gain or sv.
 *               f = H + T + 1 when nothing failed.
 *   Cost        dm = the largest d * d (fmaxf, from 0.0f) over the steps h in 1..min(f, H): d * d for a constant sequence;
 *               run = (w_speed * sv + w_steer * dm) - w_progress * gain;
 *               cost = (float)(H + T + 1 - f) * TDE_PLAN_FAIL_UNIT + fminf(fmaxf(run + TDE_PLAN_RUN_BIAS, 0.0f), TDE_PLAN_RUN_MAX): a
 *               sequence that cannot be brought to rest safely costs more than any that can and less than any that fails inside
 *               the horizon.  With T = 0 and K = 1 this is tde_plan_action's cost of the candidate (a, d).
 *   Winner      the least (ordered cost bits, n) over the N sequences; action[e] = (a_1 of the winner - knot 0's clamped a after the
 *               no-reverse rule at the state as it is -, knot 0's clamped d); diag[e] = (n of the winner, its f, its cost, the
 *               number of sequences with f == H + T + 1).
 * One lane per sequence: N <= 64 one wavefront per env, four envs per workgroup; N > 64 one workgroup of ceil(N / 64) wavefronts per
 * env.  Reads state only.  Rejected: NULL cfg / world / state / plan / set / set.seq / cost / fail_step, N outside [1,
 * TDE_PLAN_MAX_SET], K outside [1, TDE_PLAN_MAX_H], knot_len < 1, tail outside [0, TDE_PLAN_MAX_TAIL], horizon outside [1,
 * TDE_PLAN_MAX_H], v_target / margin / a weight negative or not finite, config.dt not finite or <= 0.  No allocation, no
 * synchronisation (graph-capturable). */
TDE_API int tde_score_plans(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_planner *plan,
                            const tde_plan_set *set, const uint8_t *only, float *cost, int32_t *fail_step, float *action,
                            tde_plan_diag *diag, void *stream);

/* Free-flow forecast of the other agents: for every env with only[e] != 0 (uint8 [B]; NULL: all envs), every slot j and h = 1..T,
 * out[e][h - 1][j] = (x, y, psi, v) of slot j at environment_steps = state.steps[e] + h when nobody is in its cone (out: DEVICE float32
 * [B][T][A][4]; envs with only[e] == 0 are not touched).  Slot 0 (the ego) and absent slots get four zeros at every h.  No reference
 * counterpart (its NPCs are a service's: gym_env.py:285-294).  The rule is tde_env_step's treatment of a present slot j >= 1, in its
 * order, with the controller's leader sweep replaced by "no leader": for an agent whose cone stays empty - and for a replayed one
 * while its record lasts - row h is, bit for bit, what the h-th tde_env_step from here leaves in the state.  Every expression is
 * float32 with one rounding per written operation (no contraction); bicycle, sincos_f32, the controller and the stop-line gap are the
 * step's own (tde_device.h, tde_kernels.h: npc_act_of_gap, red_line_gap; the oracle's tde_npc_action with an empty scene);
 * tests/forecast_ref.py restates this in numpy.
 * Env e: F = config.flags, s = state.scn[e], m = world.maps[world.scn[s].map], dt = config.dt; slot j: (x, y, psi, v) and len, lr, vdes
 * from the state, inv_lr = 1.0f / lr, wp = state.route_wp[e][j] (a running copy: the state is not written), rec = world.spawn[s * A + j]:
 * route = rec.route and route_n = rec.route_n with TDE_F_NPC (else no route), replay = rec.replay and replay_len = rec.replay_len
 * with TDE_F_REPLAY (else none); (tx, ty) = world.route_xy[route * RW + wp] while route >= 0 and wp < route_n.
 * For h = 1..T, k = state.steps[e] + h, (sp, cp) = sincos_f32(psi):
 *   Action       has_target = TDE_F_NPC and route >= 0 and wp < route_n.  (acc, beta) = (0, 0) without TDE_F_NPC, and at k == 1 without
 *                TDE_F_NPC_FIRST_STEP.  Otherwise, with amax = npc_max_accel, smax = npc_max_steer, clamp(u, lo, hi) = fminf(fmaxf(u, lo), hi):
 *                  without has_target: acc = clamp(npc_k_speed * (0.0f - v), -amax, amax), beta = 0 (a finished route brakes to rest);
 *                  else dx = tx - x, dy = ty - y, fwd = dx*cp + dy*sp, lat = dy*cp - dx*sp, dist = sqrtf(dx*dx + dy*dy), sin_err = lat /
 *                  fmaxf(dist, 1e-3f); beta = copysignf(smax, lat) when fwd < 0.0f, else clamp(npc_k_steer * sin_err, -smax, smax);
 *                  gap = fminf(1e30f, red_gap) - 1e30f is what the leader sweep returns when it takes no slot -; vd = fminf(vdes,
 *                  sqrtf(amax * fmaxf(gap - npc_gap_s0, 0.0f))); acc = clamp(npc_k_speed * (vd - v), -amax, amax).
 *                red_gap = 1e30f unless TDE_F_TRAFFIC_LIGHTS is set, m.n_stop > 0, has_target holds and red != 0, red = the red mask of
 *                the phase of k % m.cycle_steps (0 when cycle_steps <= 0); then the least g + npc_gap_s0 - 1.0f (fminf from 1e30f) over
 *                the stop lines q of m with (red >> light_q) & 1, where ex = x_q - x, ey = y_q - y, fj = ex*cp + ey*sp, lj = ey*cp - ex*sp,
 *                hd = cp*c_q + sp*s_q, g = fj - 0.5f * len, that have g > 0.0f, fabsf(lj) < hw_q and hd > 0.5f.
 *   Bicycle      bicycle(x, y, psi, v, inv_lr, acc, beta, dt).
 *   Replay       with TDE_F_REPLAY, replay >= 0 and k < replay_len: (x, y, psi, v) = world.replay_states[replay * RT + k].
 *   Route        when has_target and dx*dx + dy*dy < npc_reach * npc_reach for dx = tx - x, dy = ty - y at the new position: wp = wp + 1
 *                and (tx, ty) = the next route waypoint while wp < route_n.
 *   Row          out[e][h - 1][j] = (x, y, psi, v).
 * One lane per (env, slot), the T steps a loop in registers; at every step the lanes of an env store A consecutive 16-byte rows.  Reads
 * state only.  Rejected: NULL cfg / world / state / out, T outside [1, TDE_PLAN_MAX_H + TDE_PLAN_MAX_TAIL], config.dt not finite or
 * <= 0, a NULL array among the state's x, y, psi, v, len, wid, lr, vdes, route_wp, present, scn, steps (a slot is read by the step's own
 * load_agent, which takes wid with the rest) or world.spawn / world.scn.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_forecast_agents(const tde_config *cfg, const tde_world *world, const tde_state *state, int32_t T, const uint8_t *only,
                                float *out /* DEVICE [B][T][A][4] */, void *stream);

/* tde_score_plans with the other agents where a caller-given forecast puts them: forecast = DEVICE float32 [B][forecast_T][A][4], rows of
 * (x, y, psi, v) per step and slot in tde_forecast_agents' layout (tde_forecast_agents' output, a learned predictor's, ...; v is not
 * read).  Every line of the tde_score_plans specification holds except
 *   Others      every present slot j in 1..A-1 (presence, len_j and wid_j from the state): at horizon or tail step h in 1..H + T the box
 *               (x, y, c, s, 0.5f * len_j + margin, 0.5f * wid_j + margin) with (x, y, psi) = forecast[e][h - 1][j] and (s, c) =
 *               sincos_f32(psi).
 * A forecast that holds x_j + (float)h * ((v_j * c_j) * dt), y_j + (float)h * ((v_j * s_j) * dt), psi_j gives tde_score_plans' bits.
 * The rows of envs with only[e] == 0 are not read.  Same two forms as tde_score_plans; each wavefront stages the rows of a step for
 * itself, (s, c) once per row.  Rejected in addition: forecast NULL, forecast_T < horizon + tail, forecast_T > TDE_PLAN_MAX_H +
 * TDE_PLAN_MAX_TAIL.  No allocation, no synchronisation (graph-capturable).  tests/forecast_ref.py restates it in numpy. */
TDE_API int tde_score_plans_forecast(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_planner *plan,
                                     const tde_plan_set *set, const uint8_t *only, float *cost, int32_t *fail_step, float *action,
                                     tde_plan_diag *diag, const float *forecast, int32_t forecast_T, void *stream);

/* Forecast of the whole scene under caller-given ego actions, with the controller's leader sweep kept: for every env with only[e] != 0
 * (uint8 [B]; NULL: all envs), every slot j - the ego included - and h = 1..T, out[e][h - 1][j] = (x, y, psi, v) of slot j at
 * environment_steps = state.steps[e] + h when the ego (slot 0) takes ego_action[e][h - 1] at step h (out: DEVICE float32 [B][T][A][4],
 * tde_forecast_agents' layout except that ROW 0 HOLDS THE EGO'S POSE; absent slots get four zeros; envs with only[e] == 0 are not
 * touched).  No reference counterpart.  This is the motion half of tde_env_step - every present slot acts on the scene of step h - 1,
 * then moves - without its judging half: no collision, offroad or stop-line verdict, no reward, no termination, no re-spawn.  None of
 * those feeds back into motion while an episode lasts, so row h equals, bit for bit and for every slot, what the h-th tde_env_step
 * with these ego actions leaves in the state as long as the env has not re-spawned.  Rows past an episode's end describe the scene as
 * if the episode had gone on.  The state is not written; the first-step gap cache is not consulted (it holds the same bits).  Every
 * expression is float32 with one rounding per written operation (no contraction); bicycle, sincos_f32, the controller, its leader
 * sweep and the stop-line gap are the step's own (tde_device.h, tde_kernels.h: npc_action, npc_act_of_gap, red_line_gap; the oracle's
 * tde_npc_action); tests/forecast_scene_ref.py restates this in numpy.
 * Env e, slot j: everything tde_forecast_agents reads (F, s, m, dt; x, y, psi, v, len, lr, vdes, inv_lr, wp, rec, route, route_n,
 * replay, replay_len, (tx, ty)) and wid_j; hl_j = 0.5f * len_j, hw_j = 0.5f * wid_j; slot 0 has no route and no replay record.
 * For h = 1..T, k = state.steps[e] + h, (sp_j, cp_j) = sincos_f32(psi_j) of every slot, all read from the scene of step h - 1 (the
 * state itself at h = 1) before any slot moves:
 *   Action       slot 0: (acc, beta) = ego_action[e][h - 1] as given - no clamp, no scaling -, (0, 0) when ego_action is NULL (the ego
 *                coasts).  Slot i >= 1: tde_forecast_agents' Action line for line - has_target, the (0, 0) exceptions without TDE_F_NPC
 *                and at k == 1 without TDE_F_NPC_FIRST_STEP, the no-target brake, beta, red_gap, vd, acc - except
 *                  gap = fminf(lead, red_gap), lead = the least g (fminf from 1e30f) over the present slots j != i of the env, slot 0
 *                  included, that are taken: ex = x_j - x_i, ey = y_j - y_i, fj = ex*cp_i + ey*sp_i, lj = ey*cp_i - ex*sp_i, al =
 *                  fabsf(lj), halfw = npc_lane_half + hw_j, hd = cp_i*cp_j + sp_i*sp_j, g = fj - (hl_i + hl_j);
 *                  inlane = al < halfw; cone = j < i and fj < npc_cone_range and al < halfw + npc_cone_k * fj and hd > -0.5f;
 *                  taken = fj > 0.0f and (inlane or cone).
 *   Bicycle, Replay, Route   tde_forecast_agents' (slot 0: the bicycle only).
 *   Row          out[e][h - 1][j] = (x, y, psi, v), slot 0 included.
 * One lane per (env, slot), env-major, 256-thread workgroups, the T steps a loop in registers; the env's rows live in the step's LDS
 * tile with two tile syncs per step (up to 64 slots an env sits inside one wavefront; at 128 it spans two); at every step the lanes of
 * an env store A consecutive 16-byte rows.  tde_score_plans_forecast reads the result unchanged (it ignores row 0).  Reads state
 * only.  Rejected: NULL cfg / world / state / out, T outside [1, TDE_FORECAST_MAX_T], config.dt not finite or <= 0, the NULL state /
 * world arrays tde_forecast_agents rejects, world.maps NULL with TDE_F_OFFROAD or TDE_F_TRAFFIC_LIGHTS.  An empty batch returns 0
 * before any launch.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_forecast_scene(const tde_config *cfg, const tde_world *world, const tde_state *state, int32_t T,
                               const float *ego_action /* DEVICE [B][T][2] (acc, steer), or NULL */, const uint8_t *only,
                               float *out /* DEVICE [B][T][A][4] */, void *stream);

/* tde_score_plans with every sequence judged in a scene that reacts to it: for every env with only[e] != 0 (uint8 [B]; NULL: all envs)
 * and every sequence n, a scene of its own in which the ego takes that sequence's actions and every other slot runs the controller with
 * its leader sweep over THAT scene - tde_forecast_scene's rule - while the ego's box is judged against it step by step.  Arguments and
 * outputs are tde_score_plans'.  No reference counterpart.  Every line of the tde_score_plans specification holds (Knots, Horizon,
 * Brake tail, Cost, Winner, `only`, action, diag) except
 *   Others      for sequence n of env e the other agents are where tde_forecast_scene (above; every float32 expression is stated there)
 *               puts them with T = H + tail and the ego actions ego_action[h - 1] = (a_h, d_h) for h in 1..H - a_h the clamped knot
 *               acceleration after the no-reverse rule (0.0f when v + a * dt < 0.0f), d_h the clamped knot steering - and (-1.0f, d_H)
 *               at the tail steps for as long as the sequence is still judged.  At horizon or tail step h the box of present slot
 *               j >= 1 (presence, len_j and wid_j from the state) is (x, y, c, s, 0.5f * len_j + margin, 0.5f * wid_j + margin) with
 *               (x, y, psi) = that scene's row h and (s, c) = sincos_f32(psi): tde_score_plans_forecast's Others.
 *   Ego         the judged trajectory is tde_score_plans' Trajectory - bicycle(x, y, psi, v, inv_lr, a_h, d_h, dt) with inv_lr = 1.0f /
 *               lr_0 from the state as it is - and the ego's row of the scene is that pose: the same bicycle on the same inputs as
 *               tde_forecast_scene's slot 0.  Should the two ever differ in a bit, the judge's expression is the specification.  An
 *               absent slot 0 is judged all the same (tde_score_plans reads no presence of the ego); the others do not see it.
 * Contract: cost[e][n] and fail_step[e][n] equal, bit for bit, what tde_score_plans_forecast returns for sequence n alone when given
 * tde_forecast_scene(T = H + tail, ego_action = n's effective actions) as its forecast.  Rows after a sequence has failed or stands
 * are never read, so what its scene does after that is unspecified.  With margin = 0 fail_step is the step at which tde_env_step
 * would end the episode by an infraction (collision, offroad, red line) if those actions were taken; the three predicates are the
 * step's own (obb_overlap, the offroad test of the four corners, tde_tl_violation's expression).  The first-step gap cache is not
 * consulted.  tests/plan_scene_ref.py restates this by composition in numpy.
 * One lane per (env, sequence, slot), sequence-major inside an env, 256-thread workgroups, the scene's rows in the step's LDS tile
 * with two tile syncs per step; no forecast is written.  With action or diag != NULL a second kernel on the same stream (one
 * wavefront per env) reduces cost and fail_step to the Winner.  Reads state only.  Rejected: everything tde_score_plans and
 * tde_forecast_scene reject (NULL cfg / world / state / plan / set / set.seq / cost / fail_step, N, K, knot_len, tail and horizon out
 * of range, v_target / margin / a weight negative or not finite, config.dt not finite or <= 0, a NULL array among the state's x, y,
 * psi, v, len, wid, lr, vdes, route_wp, present, scn, steps, target_idx or the world's tables), and a launch grid that is too large:
 * B * N * A must not exceed TDE_PLAN_SCENE_MAX_LANES = 2^31 - 256 lanes.  An empty batch returns 0 before any launch.  No allocation,
 * no synchronisation (graph-capturable). */
#define TDE_PLAN_SCENE_MAX_LANES 2147483392LL
TDE_API int tde_score_plans_scene(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_planner *plan,
                                  const tde_plan_set *set, const uint8_t *only, float *cost, int32_t *fail_step, float *action,
                                  tde_plan_diag *diag, void *stream);

/* ---- evaluation over chosen scenarios --------------------------------------------------------------------------------- */

/* tde_env_reset with the scenario given: env e with scn[e] >= 0 (DEVICE int32 [B]) starts scenario scn[e]; an env with scn[e] < 0,
 * and every env when scn is NULL, draws it as tde_env_reset does (scn = (philox(seed, env, episode, 0).x * n_scn) >> 32).  The draw
 * is the only use of that random word, so everything else is tde_env_reset's, line for line: the Philox counters and words (blocks
 * 0 and 1 of (seed, env_base + e, episode, tag 0x7DE)), the ego's start (ego_spawn: point on the first waypoint segment, speed,
 * heading noise, TDE_F_EGO_ONLY_ATTRS attributes), the slots' spawn records, steps = 0, target_idx = 1, reached = 0, episode + 1,
 * ep_return zeroed, collided and offroad cleared; like tde_env_reset it writes none of the lookup caches (their entries carry the
 * key they were formed for and are rebuilt by the step that meets another).  `mask` (u8 [B], NULL = all) selects the envs as there.
 * What the reference does with WaypointSuiteEnv.reset when the suite index is chosen instead of sampled (gym_env.py:319-323; how
 * examples/rl_training.py:136-160 runs validation_cases.yml).  An id >= world.n_scn cannot be rejected on the host - the array
 * lives on the device - : such an env is left UNWRITTEN, counters included.  Rejected: what tde_env_reset rejects (NULL cfg / world
 * / state, A not a power of two in [1, 128], world.A != state.A, the npc_max_steer / npc_max_accel ranges under TDE_F_NPC).  An
 * empty batch returns 0 before any launch.  No allocation, no synchronisation (graph-capturable). */
TDE_API int tde_env_reset_to(const tde_config *cfg, const tde_world *world, const tde_state *state, const uint8_t *mask,
                             const int32_t *scn /* DEVICE [B], or NULL */, void *stream);

/* One step of an evaluation over chosen scenarios, after a tde_env_step launched WITHOUT TDE_F_AUTORESET: ONE launch, one wavefront
 * per env (tde_env_post_step is the model).  eval = tde_eval (tde_abi.h), R = eval.R.  For every env e with active[e] != 0:
 *   1. fold the step into acc[e]: ret = ret + (double)state.reward[e], psi_sum = psi_sum + state.info[e][0], speed_sum = speed_sum
 *      + state.info[e][1] (float64 additions, in step order);
 *   2. when !(state.terminated[e] | state.truncated[e]): done with e;
 *   3. else results[round[e]][e] = acc[e] with length = state.steps[e], reached = state.info_reached[e], scn = state.scn[e], bits =
 *      state.done_bits[e] (tde_episode_record); acc[e] = zeros; round[e] = round[e] + 1;
 *   4. when round[e] < R and plan[round[e]][e] lies in [0, world.n_scn): the env is re-spawned to that scenario by
 *      tde_env_reset_to's rule and, when state.obs is set, the compact observation of the new episode is written (as
 *      tde_env_post_step does); state.terminated / truncated / reward / done_bits keep the step's values;
 *   5. else active[e] = 0 and the state stays as the step left it.
 * Envs with active[e] == 0 are not touched.  A round[e] outside [0, R) when an episode ends - a caller's error the host cannot see -
 * records nothing and sets active[e] = 0.  An episode ends here with terminated | truncated; the reference's callback ends one with
 * `infraction or is_success` (examples/rl_training.py:51-53): the two coincide under terminated_at_infraction = 1, the default.
 * No atomics: every env owns its column of plan and results.  Rejected: NULL cfg / world / state / eval or a NULL array in eval, R
 * < 1, a state without reward, terminated, truncated, done_bits, info, info_reached, steps or scn, TDE_F_AUTORESET in cfg->flags
 * (the step would already have re-spawned the env), and what tde_env_reset rejects.  An empty batch returns 0 before any launch.
 * No allocation, no synchronisation (graph-capturable); every store is an ordinary vector store. */
TDE_API int tde_eval_advance(const tde_config *cfg, const tde_world *world, const tde_state *state, const tde_eval *eval, void *stream);

/* ---- host side: static tables ------------------------------------------------------------------------------------ */

/* Offroad grid index of ONE drivable mesh - what the simulator prepares once per map from the road mesh it is constructed
 * with (Simulator(road_mesh=map_cfg.road_mesh), gym_env.py:184, 260) so that compute_offroad (:142) is a cell look-up plus a
 * few candidate triangles instead of a pass over the mesh.  HOST pointers, no GPU involved, synchronous, n_threads host
 * threads (0 = all).  tri = [n_tri][6] fp32 vertices ax,ay,bx,by,cx,cy (the fp32 values the kernels and the oracle see);
 * threshold = the effective offroad distance in metres (sqrt of the threshold under offroad_threshold_squared); cell = cell
 * edge; margin = classification margin (0.05: absorbs fp32 evaluation at coordinates of kilometres); near_range (ABI 10) = how far
 * beyond the threshold, in metres, the coarse tiles carry a NEAR LIST (tde_world.tile_near: the triangles among which the nearest
 * one of any point of the tile is found - what the MAGNITUDE of the offroad infraction needs, gym_env.py:427; 0 = none, the
 * kernels then scan the grid around a corner; a few metres cover an ego that left the road within the last step or two).  Classes and lists are
 * conservative (csrc/tde_gridbuild.h), so the kernels' masks equal a brute-force pass over every triangle.  The result is
 * owned by the library until tde_grid_free. */
TDE_API int tde_grid_build(const float *tri, int32_t n_tri, float threshold, float cell, float margin, float near_range,
                           int32_t n_threads, tde_grid **out);
TDE_API void tde_grid_free(tde_grid *grid);

#ifdef __cplusplus
}
#endif
#endif /* TDE_HIP_H */
