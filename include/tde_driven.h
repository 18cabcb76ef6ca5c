/* tde_driven.h — a step in which chosen NPC slots take their (acceleration, steering) from the caller, exactly as slot 0 does: what an
 * adversary, a learned traffic model, self-play and a perturbed log are made of.  An ADDITIVE header over tde_hip.h with a version of
 * its own: TDE_ABI_VERSION and every struct and entry point of the older headers are untouched; a library that exports these symbols
 * implements TDE_DRIVEN_VERSION.
 *
 * The caller owns all memory; the entry point allocates nothing, synchronises nothing, works on the stream it is given (it can be
 * captured in a graph), returns 0 or a hipError_t value and leaves its message in tde_last_error().  Every argument rule is checked on
 * the host before anything is launched.
 */
#ifndef TDE_DRIVEN_H
#define TDE_DRIVEN_H

#include "tde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_DRIVEN_VERSION 1

/* One timestep of every env: tde_env_step's definition, word for word, with one difference.  A lane (e, a) with a >= 1, a present slot
 * and driven[e * A + a] != 0 is DRIVEN:
 *
 *   - acc = agent_action[(e * A + a) * 2], beta = agent_action[(e * A + a) * 2 + 1] go to the bicycle model as slot 0's do: raw units,
 *     no clamp the ego does not get;
 *   - the controller's result for the lane is discarded (the lane still takes part in the controller's sweep);
 *   - this holds at every step count k: a driven slot also acts at k == 1 without TDE_F_NPC_FIRST_STEP, and acts without TDE_F_NPC;
 *   - the replay record is not applied to the lane (an undriven replayed slot is pulled to its record as before);
 *   - route bookkeeping is untouched: with TDE_F_NPC the slot's route_wp advances by the npc_reach rule as an NPC's does, so control
 *     can be handed back to the controller at any step;
 *   - everything after the motion is the step's own: collision sweep, offroad test, traffic lights, the ego's reward and termination,
 *     the auto-reset re-spawn and every output tde_env_step writes (done_bits, obs, ep_*, info, magnitudes).  Other NPCs see a driven
 *     slot as any other agent.
 *
 * agent_action: DEVICE float [B][A][2]; driven: DEVICE uint8 [B][A].  Row 0 of both is never read (the ego's action is state.action),
 * nor are the entries of absent slots or the agent_action entries of undriven slots: a NaN there reaches no result.  driven == NULL
 * means that no slot is driven; agent_action may then be NULL too, and the results equal those of tde_env_step's one-role kernel bit
 * for bit.  The mask is by SLOT INDEX: an env that is re-spawned inside the step keeps the caller's mask for its new agents - the next
 * call drives whoever then sits in the slot.
 *
 * Caches: if state.act_cache is set, the key entry of every env is made invalid (episode -1), as tde_near_field_spawn does - the stored
 * actions were the controller's.  slot_cache and env_cache are neither read nor written: their keys see the new state themselves.
 * Always the one-role kernel, its arguments by value at every slot count: tde_kernel_override does not apply.
 *
 * Refused on the host: everything tde_env_step refuses; driven != NULL with agent_action == NULL; state.slot_route != NULL (routes of
 * near-field agents plus outside actions are out of scope of this version). */
TDE_API int tde_env_step_driven(const tde_config *cfg, const tde_world *world, const tde_state *state,
                                const float *agent_action /* DEVICE [B][A][2], may be NULL with driven */,
                                const uint8_t *driven /* DEVICE [B][A], may be NULL */, void *stream);

TDE_API int tde_driven_version(void);

#ifdef __cplusplus
}
#endif
#endif
