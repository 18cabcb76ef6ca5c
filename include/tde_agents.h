/* tde_agents.h — observe and score any slot: the vector observation of tde_vector_obs taken from chosen (env, slot) pairs, and each
 * pair's reward and flags after the step(s) that followed - what a policy that drives a slot through tde_env_step_driven
 * (include/tde_driven.h) needs besides the actions: observe the pairs, step, read their outcomes.  An ADDITIVE header over tde_hip.h
 * with a version of its own: TDE_ABI_VERSION and every struct and entry point of the older headers are untouched; a library that
 * exports these symbols implements TDE_AGENTS_VERSION.
 *
 * The caller owns all memory; the entry points allocate nothing, synchronise nothing, work on the stream they are given (they can be
 * captured in a graph), return 0 or a hipError_t value and leave their message in tde_last_error().  Every argument rule is checked
 * on the host before anything is launched.
 */
#ifndef TDE_AGENTS_H
#define TDE_AGENTS_H

#include "tde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_AGENTS_VERSION 1

/* What tde_agent_obs saw of a pair, for tde_agent_outcomes to score what happened since. */
typedef struct tde_agent_track {   /* 32 bytes, written by tde_agent_obs, read by tde_agent_outcomes */
    float x, y, psi, v;            /* the slot's pose when it was observed */
    int32_t route_wp, episode;     /* state.route_wp of the slot, state.episode of the env, at that time */
    int32_t steps; uint32_t present;
} tde_agent_track;

/* flag bits of tde_agent_outcomes */
#define TDE_AG_VALID    1   /* the row is an outcome (the pair was observed, is in range and is not the ego) */
#define TDE_AG_COLLIDED 2   /* state.collided of the slot */
#define TDE_AG_OFFROAD  4   /* state.offroad of the slot */
#define TDE_AG_REACHED  8   /* state.route_wp of the slot is greater than at the observation */
#define TDE_AG_ENDED    16  /* the agent that was observed is gone: its env was re-spawned, or the slot is no longer present */

/* Row i of out (float32 [n][D], D = TDE_VO_EGO + TDE_VO_NBR * vo.k_nbr + TDE_VO_RAY * vo.n_rays) = the vector observation of pair
 * (e, a) = (pairs[2 i], pairs[2 i + 1]):
 *   - e outside [0, B), a outside [0, A) or state.present[e * A + a] == 0: the row is zeros and track[i] is all zero (present = 0);
 *   - otherwise tde_vector_obs's specification (include/tde_hip.h) word for word - the float32 expression trees, one rounding per
 *     written operation - with slot a as the observer: (x0, y0, psi0, v0, len0, wid0) are slot a's; "the other present agents" of
 *     the neighbour block and of the car ray channel are the present slots b != a in 0..A-1, the ego included, neighbours ordered
 *     by (d2 bits, b); the road and red channels, entries 8 and 9 are env e's as there.
 *   Waypoint entries [3, 8): for a == 0 the scenario's waypoints at target_idx, as tde_vector_obs.  For a >= 1 the slot's route:
 *     with w = state.slot_route[e * A + a] when the array is set and the word is not 0, route = (w & 0xFFFFF) - 1 and route_n =
 *     w >> 20, else route / route_n of the spawn record of (state.scn[e], a); for j = route_wp and route_wp + 1 (state.route_wp of
 *     the slot): frame(route_xy[route][j] - (x0, y0)) while 0 <= j < route_n, else (0, 0); entry 7 = (float)min(max(route_n -
 *     route_wp, 0), 2).  Without a route (route outside [0, world.n_routes)) all five entries are 0.  TDE_F_NPC is not consulted.
 *   A pair with slot 0 equals tde_vector_obs's row of that env bit for bit.
 * track (may be NULL): track[i] = the slot's x, y, psi, v and route_wp, the env's episode and steps, present = 1.
 * Duplicate pairs are allowed (each row is written from the same state); n == 0 is a no-op.  One wavefront per pair, four pairs per
 * workgroup, one lane per ray.
 * Refused on the host: everything tde_vector_obs refuses (in its words, under this entry point's name), world.spawn NULL,
 * state.route_wp or state.episode NULL, world.route_xy NULL with world.n_routes > 0, n < 0, pairs or out NULL with n > 0. */
TDE_API int tde_agent_obs(const tde_config *cfg, const tde_world *world, const tde_state *state, const struct tde_vector_obs *vo,
                          const int32_t *pairs /* DEVICE [n][2] = (env, slot) */, int32_t n, float *out /* DEVICE [n][D] */,
                          tde_agent_track *track /* DEVICE [n], may be NULL */, void *stream);

/* What became of the pairs since tde_agent_obs wrote `track`, on the state that the step(s) after the observation left behind.
 * Row i, pair (e, a):
 *   - track[i].present == 0, e outside [0, B), a outside [1, A):            flags = 0, reward = 0.  (The ego's outcome is the step's
 *     own outputs - state.reward, terminated, truncated, done_bits - which is why a == 0 is reported as invalid.)
 *   - state.episode[e] != track[i].episode (the env was re-spawned in between and the slot holds a new agent), or the slot is no
 *     longer present:                                                       flags = VALID | ENDED, reward = 0.
 *   - otherwise: flags = VALID | COLLIDED when state.collided of the slot | OFFROAD when state.offroad of the slot | REACHED when
 *     state.route_wp of the slot > track[i].route_wp, and reward = the reference's get_reward (gym_env.py:396-411) applied to the
 *     slot, in float64 on the fp32 state as the ego's is (reward_core's pieces):
 *       reach = REACHED ? config.waypoint_bonus : 0
 *       dist  = (dist((x, y), (track.x, track.y)) > config.distance_cutoff) ? config.distance_bonus : 0
 *       psi   = (1 - cos((double)(psi - track.psi))) * -config.heading_penalty       (the difference in fp32)
 *       reward = (float)((reach + dist) + psi)
 * One lane per pair.
 * Refused on the host: NULL cfg / world / state, n < 0, pairs / track / reward / flags NULL with n > 0, a NULL state array among
 * x, y, psi, route_wp, present, collided, offroad, episode with n > 0. */
TDE_API int tde_agent_outcomes(const tde_config *cfg, const tde_world *world, const tde_state *state,
                               const int32_t *pairs /* DEVICE [n][2] */, int32_t n, const tde_agent_track *track /* DEVICE [n] */,
                               float *reward /* DEVICE [n] */, uint8_t *flags /* DEVICE [n] */, void *stream);

TDE_API int tde_agents_version(void);

#ifdef __cplusplus
}
#endif
#endif
