// tde_step_body.inc - the body of the one-role step kernels, included by tde_kernels.h inside env_step_kernel (TDE_STEP_ROUTED 0,
// TDE_STEP_DRIVEN 0), env_step_routed_kernel (TDE_STEP_ROUTED 1) and env_step_driven_kernel (TDE_STEP_DRIVEN 1): ONE text, so that the
// routed family is the one-role step plus one load, the driven family the one-role step plus a mask byte and an action per driven slot,
// and the existing family compiles from exactly the tokens it always had.
    __shared__ Tiles<kBlock> t;
    __shared__ Cold cold;
    if (threadIdx.x == 0) fill_cold(cold, cfg, w);
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(g / A), a = (int)(g % A);
    const bool valid = e < st.B;
    const int64_t gs = valid ? g : 0;
    const int es = valid ? e : 0;
    Agent ag;
    load_agent(st, gs, ag);
#if TDE_STEP_ROUTED
    const uint32_t slot_word = st.slot_route[gs];        // (with the state's own arrays: ahead of the chain scenario -> spawn record that load_ctx walks)
#endif
    if (!valid) ag.present = false;
#if TDE_STEP_DRIVEN
    // the slot's mask byte and, behind it, its action: beside the state's own arrays, ahead of the table chain.  Row 0 (the ego's action
    // is state.action) and the entries of absent or undriven slots are never read.
    bool drv = false;
    float2 dact = make_float2(0.0f, 0.0f);
    if (driven && a > 0 && ag.present) drv = driven[gs] != 0;
    if (drv) dact = reinterpret_cast<const float2 *>(agent_action)[gs];
#endif
    EnvRegs er{st.scn[es], st.steps[es], st.target_idx[es], st.reached[es], st.episode[es]};
    Ctx cx;
    // (the one-role kernel does not use the lookup caches even when they are there: read in its prologue and kept like the
    //  three-role kernel keeps them they made it SLOWER - 8192 x 16: 10.4 -> 11.0 us, configs[4] on three streams 42.4 -> 44.3 -
    //  for 6 MB more traffic per step: its wavefronts have the whole serial step ahead of them, the table chain is not what
    //  they wait for.  profiles/r03_f_solo_with_caches.txt)
#if TDE_STEP_ROUTED
    load_ctx<A, true>(cfg, cold, a, ag, er, cx, slot_word);
#else
    load_ctx<A>(cfg, cold, a, ag, er, cx);
#endif
    const float2 act = reinterpret_cast<const float2 *>(action)[es];
    float c0, s0;
    sincos_f32(ag.psi, s0, c0);
    write_tile_slot(t.a[threadIdx.x], t.b[threadIdx.x], valid && ag.present, ag, c0, s0, cfg.npc_lane_half);
    tile_sync<A>();
    const int map0 = cx.map_id;                     // (MAG: the map of the episode that is being stepped; a re-spawn replaces cx)
#if TDE_STEP_DRIVEN
    StepOut o = step_lane<A, kBlock, LIGHTS, BIG, MAG, true>(cfg, w, cold, st, t, es, a, valid, ag, er, cx, c0, s0, act.x, act.y, st.magnitudes, drv, dact.x, dact.y);
#else
    StepOut o = step_lane<A, kBlock, LIGHTS, BIG, MAG>(cfg, w, cold, st, t, es, a, valid, ag, er, cx, c0, s0, act.x, act.y, st.magnitudes);
#endif
    const unsigned long long hit_m = MAG ? __ballot(o.collided != 0) : 0ull, off_m = MAG ? __ballot(o.offroad != 0) : 0ull;
    if (valid) {
        store_agent_dynamic(st, g, ag);
        if (o.respawned) store_agent_static(st, g, ag);
        // flags of a re-spawned agent are cleared, as tde_reset_env does
        st.collided[g] = o.respawned ? 0 : o.collided;
        st.offroad[g] = o.respawned ? 0 : o.offroad;
        if (a == 0) {
            st.steps[e] = er.steps;
            st.target_idx[e] = er.target_idx;
            st.reached[e] = er.reached;
            st.reward[e] = o.reward;
            st.terminated[e] = o.terminated;
            st.truncated[e] = o.truncated;
            if (st.tl_violation) st.tl_violation[e] = o.tl;
            if (o.respawned) { st.scn[e] = er.scn; st.episode[e] = er.episode; }
#if TDE_STEP_DRIVEN
            // the stored NPC actions were computed for a step the controller takes: the env's key goes invalid, as tde_near_field_spawn
            // leaves it (slot_cache / env_cache are keyed by what they cache - scenario, episode, waypoint indices - and see the new state)
            if (st.act_cache) *reinterpret_cast<int2 *>(st.act_cache + (int64_t)e * (A + 1) + A) = make_int2(-1, 0);
#endif
            if (reward_k) reward_k[e] = o.reward;
            if (done_k)
                done_k[e] = (uint8_t)(o.terminated | (o.truncated << 1) | (o.offroad << 2) | (o.collided << 3) | (o.tl << 4));
            if (st.ep_return) {
                // Monitor-style episode statistics (examples/rl_training.py:123-128): float64 sum of the episode's rewards
                double ret = st.ep_return[e] + (double)o.reward;
                if (o.terminated | o.truncated) {
                    if (st.ep_final) st.ep_final[e] = ret;
                    if (st.ep_final_len) st.ep_final_len[e] = o.k;
                    if (o.respawned) ret = 0.0;
                }
                st.ep_return[e] = ret;
            }
            if (OBS && st.obs) {
                // compact observation of the state after the step (and re-spawn), as state_obs_kernel forms it.  The cached
                // ego target is current unless the reward path is off or the episode just ended without a re-spawn.
                const bool ended = (o.terminated | o.truncated) && !o.respawned;
                // (the target from cx as VALUES behind an empty asm: left to itself the compiler turns "cx.wtx or the table entry" into
                //  ONE load through a select of ADDRESSES, which pins cx in scratch memory - 24 B of private segment, and a one-step
                //  launch with a private segment costs 1.3 us more to dispatch, profiles/r03_g_step_outputs_cost.txt)
                bool has = er.target_idx < cx.n_wp;
                double tx = cx.wtx, ty = cx.wty;
                asm volatile("" : "+v"(tx), "+v"(ty));            // (values, not loads from cx: nothing to merge with the load below)
                if (!(cfg.flags & TDE_F_REWARD) || ended) {
                    has = er.target_idx < reinterpret_cast<const int4 *>(w.scn)[er.scn].y;
                    const double2 t2 = reinterpret_cast<const double2 *>(w.wp_xy)[(int64_t)er.scn * w.NW + (has ? er.target_idx : 0)];
                    tx = t2.x; ty = t2.y;
                }
                float fwd = 0.0f, lat = 0.0f;
                if (has) {
                    const float dx = (float)tx - ag.x, dy = (float)ty - ag.y;
                    fwd = dx * c0 + dy * s0;
                    lat = dy * c0 - dx * s0;
                }
                float4 *ob = reinterpret_cast<float4 *>(st.obs) + 2 * (int64_t)e;
                ob[0] = make_float4(ag.x, ag.y, ag.psi, ag.v);
                ob[1] = make_float4(fwd, lat, has ? 1.0f : 0.0f, (float)er.steps);
            }
        }
    }
    if constexpr (MAG) {
        // tde_state.magnitudes (get_info's "collision" / "offroad", ref gym_env.py:427-428) for the egos this step flagged: the whole
        // wavefront works on one ego at a time, from the rows of THIS step (a re-spawn does not rewrite them in this kernel) and
        // the map descriptor fetched again through the scalar path.  Placed BEHIND the stores, where nothing of the step is live
        // any more: inside step_lane the section raised the kernel from 84 to 114 VGPRs (4 instead of 6 wavefronts per SIMD:
        // +15 % per step at 65 536 envs x 16, where this kernel runs)
        const unsigned long long ego = __ballot(a == 0 && valid);
        const int w0 = (int)(threadIdx.x & ~63u);
        // (LEAN = true: the low-register scan of the role-split kernels here too)
        ego_magnitudes_of_wave<A, true>(cfg, w, [&](int src) { return cold.maps[__builtin_amdgcn_readlane(map0, src)]; }, ego,
                                        hit_m, off_m, &t.a[w0], &t.b[w0], (int)(threadIdx.x & 63u), t.poly[threadIdx.x >> 6],
                                        (a == 0 && valid) ? reinterpret_cast<float4 *>(st.magnitudes) + e : nullptr);
    }
