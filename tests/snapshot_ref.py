"""numpy restatement of tde_state_copy (include/tde_snapshot.h) over the dicts of EnvState.host(): written from the header - the three
groups of tde_state's arrays, the NULL rule, the invalidation of the destination rows' caches, the turn of the layer planes, the skip of a
pair with an index out of range - and used by tests/test_snapshot_cpu.py (against a brute force) and tests/test_gpu_snapshot.py."""
import numpy as np

# the header's list, group by group
COPIED_AGENT = ["x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "collided", "offroad", "slot_route"]
COPIED_ENV = ["scn", "steps", "target_idx", "reached", "episode", "action", "obs", "ep_return"]
OUTPUTS = ["reward", "terminated", "truncated", "tl_violation", "done_bits", "info", "info_reached", "ep_final", "ep_final_len", "magnitudes"]
INVALIDATED = ["slot_cache", "env_cache", "act_cache"]
SNAPSHOT_OUTPUTS, SNAPSHOT_CHECK = 1, 2


def group(name):
    """"copied" | "outputs" | "invalidated" of a tde_state array; KeyError for a name the restatement does not know"""
    hits = [g for g, names in (("copied", COPIED_AGENT + COPIED_ENV), ("outputs", OUTPUTS), ("invalidated", INVALIDATED)) if name in names]
    if len(hits) != 1:
        raise KeyError(f"{name!r} is in {len(hits)} groups of tde_state_copy")
    return hits[0]


def rows(a, B):
    """the array as [B, bytes of a row] uint8 (a view)"""
    return a.reshape(B, -1).view(np.uint8)


def valid_pairs(src_env, dst_env, sB, dB):
    return [(int(s), int(d)) for s, d in zip(src_env, dst_env) if 0 <= s < sB and 0 <= d < dB]


def state_copy(src, dst, sB, dB, A, src_env, dst_env, outputs=False):
    """`dst` (a dict of numpy arrays; absent or None = a NULL pointer) after tde_state_copy from `src`: modified in place and returned"""
    pairs = valid_pairs(src_env, dst_env, sB, dB)
    names = COPIED_AGENT + COPIED_ENV + (OUTPUTS if outputs else [])
    for n in names:
        a, b = src.get(n), dst.get(n)
        if a is None or b is None:
            continue
        ra, rb = rows(a, sB), rows(b, dB)
        for s, d in pairs:
            rb[d] = ra[s]
    for s, d in pairs:
        for n in ("slot_cache", "env_cache"):
            if dst.get(n) is not None:
                rows(dst[n], dB)[d] = 0
        if dst.get("act_cache") is not None:
            r = dst["act_cache"].reshape(dB, A + 1, 2)
            r[d] = 0
            r[d, A, 0] = -1
    return dst


def frames_copy(src_layers, dst_layers, src_obs, dst_obs, n_stack, src_phase, dst_phase, src_env, dst_env):
    """the frames part: layers [B, n_stack, plane], obs [B, 3 * n_stack, plane] (either pair may be None); dst modified in place"""
    sB = (src_layers if src_layers is not None else src_obs).shape[0]
    dB = (dst_layers if dst_layers is not None else dst_obs).shape[0]
    for s, d in valid_pairs(src_env, dst_env, sB, dB):
        if src_layers is not None:
            for j in range(n_stack):
                dst_layers[d, (j - src_phase + dst_phase) % n_stack] = src_layers[s, j]
        if src_obs is not None:
            dst_obs[d] = src_obs[s]
    return dst_layers, dst_obs


def check_indices(src_env, dst_env, sB, dB, same):
    """the message fragment TDE_SNAPSHOT_CHECK refuses the indices with, or None"""
    seen = set()
    for s, d in zip(src_env, dst_env):
        if not 0 <= s < sB:
            return "src_env index is outside"
        if not 0 <= d < dB:
            return "dst_env index is outside"
        if d in seen:
            return "names a row twice"
        seen.add(d)
    if same and seen & set(int(s) for s in src_env):
        return "overlaps src_env"
    return None
