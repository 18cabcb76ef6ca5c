// tde_torch_ext.cpp — the PyTorch-ROCm C++ extension of the env step path (BASELINE.json north_star: "hand-written CDNA4
// HIP kernels behind a PyTorch-ROCm C++ extension").  It is a thin binding of the SAME C-ABI entry points that
// include/tde_hip.h declares (libtde_hip.so): torch tensors in, TORCH_CHECK on dtype / shape / device / contiguity, the
// launch stream taken from torch's current HIP stream in C++, HIP errors raised as RuntimeError.  No kernel lives here.
// What it removes is the per-call ctypes marshalling of the Python binding (struct copies, byref, argument conversion:
// about 7 us per call on the host), which is what bounds closed-loop stepping (one tde_env_step per policy action,
// reference loop: gym_env.py:453-461).  The ctypes binding stays as the reference-side stub.
#include <torch/extension.h>

// PyTorch-ROCm keeps the device type "cuda" for HIP devices: the guard / stream accessors are the "masquerading" ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "tde_hip.h"
#include "tde_snapshot.h"

namespace {

void check_rc(int rc, const char *what)
{
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + tde_last_error());
}

const void *dev_ptr(const at::Tensor &t, at::ScalarType dt, int64_t numel, const char *name, const at::Device &dev)
{
    TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (there is no CPU path)");
    TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), ", expected ", dev);
    TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
    TORCH_CHECK(numel < 0 || t.numel() == numel, name, " must have ", numel, " elements, got ", t.numel());
    return t.data_ptr();
}

// the checked pointer as the C-ABI types it, and the launch stream: torch's current HIP stream of the device
template <typename T> T *ptr(const at::Tensor &t, at::ScalarType dt, int64_t numel, const char *name, const at::Device &dev)
{
    return static_cast<T *>(const_cast<void *>(dev_ptr(t, dt, numel, name, dev)));
}
void *cur_stream(const at::Device &dev) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream(); }

// ---- typed carriers of the C-ABI's argument structs -----------------------------------------------------------------
// Round 4: the extension no longer takes raw addresses.  A Config is built from the BYTES of a tde_config (length checked),
// a World and an EnvHandle from NAMED device tensors (dtype / device / contiguity / size checked against the struct's
// field), and both keep those tensors alive for as long as they exist: nothing here dereferences an integer that Python
// passed, and a state buffer that Python re-allocates cannot leave the handle pointing at freed memory (the handle
// still holds the old tensor; make a new handle for the new buffers).
class Config {
  public:
    explicit Config(const py::bytes &raw)
    {
        const std::string b = raw;
        TORCH_CHECK(b.size() == sizeof(tde_config), "tde_config is ", sizeof(tde_config), " bytes, got ", b.size());
        std::memcpy(&c, b.data(), sizeof(c));
    }
    tde_config c;
};

struct Field {
    const char *name;
    size_t off;                 // offset of the pointer member in the struct
    at::ScalarType dt;
    int kind;                   // how many elements: see count_of
    bool required;
};
enum { K_ANY = 0, K_AGENT, K_ENV, K_ENV2, K_ENV4, K_ENV8, K_SLOT8, K_ACT };

#define WF(n, dt) {#n, offsetof(tde_world, n), dt, K_ANY, true}
const Field kWorldFields[] = {WF(maps, at::kByte), WF(tri, at::kFloat), WF(cell_word, at::kUInt32), WF(cell_tri, at::kFloat),
                              WF(cell_cls2, at::kUInt32), WF(cell_sub, at::kUInt32), WF(cell_coarse, at::kByte), WF(tile_near, at::kUInt32), WF(scn, at::kByte),
                              WF(wp_xy, at::kDouble), WF(spawn, at::kByte), WF(route_xy, at::kFloat), WF(replay_states, at::kFloat),
                              WF(stoplines, at::kByte), WF(phases, at::kByte), WF(start_psi, at::kFloat),
                              {"first_gap", offsetof(tde_world, first_gap), at::kUInt32, K_ANY, false}};
#undef WF
#define SF(n, dt, k, req) {#n, offsetof(tde_state, n), dt, k, req}
const Field kStateFields[] = {
    SF(x, at::kFloat, K_AGENT, true), SF(y, at::kFloat, K_AGENT, true), SF(psi, at::kFloat, K_AGENT, true), SF(v, at::kFloat, K_AGENT, true),
    SF(len, at::kFloat, K_AGENT, true), SF(wid, at::kFloat, K_AGENT, true), SF(lr, at::kFloat, K_AGENT, true), SF(vdes, at::kFloat, K_AGENT, true),
    SF(route_wp, at::kInt, K_AGENT, true), SF(present, at::kByte, K_AGENT, true), SF(collided, at::kByte, K_AGENT, true),
    SF(offroad, at::kByte, K_AGENT, true), SF(scn, at::kInt, K_ENV, true), SF(steps, at::kInt, K_ENV, true),
    SF(target_idx, at::kInt, K_ENV, true), SF(reached, at::kInt, K_ENV, true), SF(episode, at::kInt, K_ENV, true),
    SF(action, at::kFloat, K_ENV2, true), SF(reward, at::kFloat, K_ENV, true), SF(terminated, at::kByte, K_ENV, true),
    SF(truncated, at::kByte, K_ENV, true), SF(tl_violation, at::kByte, K_ENV, true), SF(info, at::kDouble, K_ENV4, false),
    SF(info_reached, at::kInt, K_ENV, false), SF(done_bits, at::kByte, K_ENV, false), SF(obs, at::kFloat, K_ENV8, false),
    SF(ep_return, at::kDouble, K_ENV, false), SF(ep_final, at::kDouble, K_ENV, false), SF(ep_final_len, at::kInt, K_ENV, false),
    SF(slot_cache, at::kInt, K_SLOT8, false), SF(env_cache, at::kInt, K_ENV8, false), SF(act_cache, at::kInt, K_ACT, false),
    SF(magnitudes, at::kFloat, K_ENV4, false), SF(slot_route, at::kInt, K_AGENT, false)};
#undef SF

int64_t count_of(int kind, int64_t B, int64_t A)
{
    switch (kind) {
        case K_AGENT: return B * A;
        case K_ENV: return B;
        case K_ENV2: return 2 * B;
        case K_ENV4: return 4 * B;
        case K_ENV8: return 8 * B;
        case K_SLOT8: return 8 * B * A;
        case K_ACT: return 2 * B * (A + 1);
        default: return -1;
    }
}

// fills the pointer members of a struct from a dict of named tensors; every tensor used is appended to `keep`
template <size_t N>
void fill_struct(void *st, const Field (&fields)[N], const py::dict &tensors, int64_t B, int64_t A, const at::Device &dev,
                 std::vector<at::Tensor> &keep, const char *what)
{
    for (const Field &f : fields) {
        const void *p = nullptr;
        if (tensors.contains(f.name) && !tensors[f.name].is_none()) {
            const at::Tensor t = py::cast<at::Tensor>(tensors[f.name]);
            p = dev_ptr(t, f.dt, count_of(f.kind, B, A), f.name, dev);
            TORCH_CHECK(t.numel() > 0, what, ".", f.name, " is empty");
            keep.push_back(t);
        } else {
            TORCH_CHECK(!f.required, what, " lacks the tensor '", f.name, "'");
        }
        std::memcpy(static_cast<char *>(st) + f.off, &p, sizeof(p));
    }
    for (const auto &kv : tensors) {
        const std::string k = py::cast<std::string>(kv.first);
        bool known = false;
        for (const Field &f : fields) known = known || k == f.name;
        TORCH_CHECK(known, what, " has no field '", k, "'");
    }
}

class World {
  public:
    World(const py::dict &tensors, const py::dict &ints, int64_t device_index) : dev(at::kCUDA, static_cast<c10::DeviceIndex>(device_index))
    {
        std::memset(&w, 0, sizeof(w));
        fill_struct(&w, kWorldFields, tensors, 0, 0, dev, keep_, "world");
        auto geti = [&](const char *k) {
            TORCH_CHECK(ints.contains(k), "world lacks the size '", k, "'");
            return static_cast<int32_t>(py::cast<int64_t>(ints[k]));
        };
        w.n_maps = geti("n_maps"); w.n_scn = geti("n_scn"); w.NW = geti("NW"); w.A = geti("A");
        w.n_routes = geti("n_routes"); w.RW = geti("RW"); w.n_replay = geti("n_replay"); w.RT = geti("RT");
        w.hints = geti("hints"); w.NH = geti("NH");
        // the tables whose sizes the struct's integers imply
        auto bytes_of = [&](const char *k) { const at::Tensor t = py::cast<at::Tensor>(tensors[k]); return (int64_t)t.numel() * (int64_t)t.element_size(); };
        TORCH_CHECK(w.n_maps >= 1 && w.n_scn >= 1 && w.NW >= 2 && w.A >= 1, "world sizes out of range");
        TORCH_CHECK(bytes_of("maps") == (int64_t)w.n_maps * (int64_t)sizeof(tde_map), "world.maps: expected n_maps * sizeof(tde_map) bytes");
        TORCH_CHECK(bytes_of("scn") == (int64_t)w.n_scn * (int64_t)sizeof(tde_scenario), "world.scn: expected n_scn * sizeof(tde_scenario) bytes");
        TORCH_CHECK(bytes_of("spawn") == (int64_t)w.n_scn * w.A * (int64_t)sizeof(tde_spawn), "world.spawn: expected n_scn * A * sizeof(tde_spawn) bytes");
        TORCH_CHECK(bytes_of("wp_xy") == (int64_t)w.n_scn * w.NW * 16, "world.wp_xy: expected [n_scn][NW][2] float64");
        TORCH_CHECK(bytes_of("route_xy") >= (int64_t)w.n_routes * w.RW * 8, "world.route_xy: smaller than [n_routes][RW][2] float32");
        TORCH_CHECK(bytes_of("replay_states") >= (int64_t)w.n_replay * w.RT * 16, "world.replay_states: smaller than [n_replay][RT][4] float32");
        TORCH_CHECK(w.NH >= 0 && bytes_of("start_psi") >= (int64_t)w.n_scn * w.NH * 4, "world.start_psi: smaller than [n_scn][NH] float32");
        // (first_gap may be absent: a world without the first-step gap cache, as near-field envs use it)
        TORCH_CHECK(!w.first_gap || bytes_of("first_gap") == (int64_t)w.n_scn * w.A * (int64_t)sizeof(tde_first_gap), "world.first_gap: expected n_scn * A * sizeof(tde_first_gap) bytes");
    }
    tde_world w;
    at::Device dev;

  private:
    std::vector<at::Tensor> keep_;
};

// tde_near_field over named device tensors (kept alive) and its scalar parameters
#define NF(n, dt) {#n, offsetof(tde_near_field, n), dt, K_ANY, true}
const Field kNearFieldFields[] = {NF(cand, at::kFloat), NF(nbr, at::kShort), NF(nbr_n, at::kByte), NF(fixed, at::kByte), NF(n_cand, at::kInt)};
#undef NF
class NearField {
  public:
    NearField(const py::dict &tensors, int64_t S, int64_t A, int64_t NC, int64_t K, double radius, double clear_ego, int64_t count,
              int64_t density, int64_t device_index)
        : dev(at::kCUDA, static_cast<c10::DeviceIndex>(device_index))
    {
        std::memset(&nf, 0, sizeof(nf));
        fill_struct(&nf, kNearFieldFields, tensors, 0, 0, dev, keep_, "near_field");
        TORCH_CHECK(S >= 1 && NC >= 1 && NC <= TDE_NF_MAX_CAND && K >= 1 && K <= TDE_NF_MAX_NBR, "near_field sizes out of range");
        auto numel = [&](const char *k) { return (int64_t)py::cast<at::Tensor>(tensors[k]).numel(); };
        TORCH_CHECK(numel("cand") == S * NC * (int64_t)(sizeof(tde_nf_cand) / 4), "near_field.cand: expected [S][NC] tde_nf_cand");
        TORCH_CHECK(numel("nbr") == S * NC * K, "near_field.nbr: expected [S][NC][K]");
        TORCH_CHECK(numel("nbr_n") == S * NC && numel("fixed") == S * NC && numel("n_cand") == S, "near_field: nbr_n / fixed [S][NC], n_cand [S]");
        nf.S = (int32_t)S; nf.A = (int32_t)A; nf.NC = (int32_t)NC; nf.K = (int32_t)K;
        nf.radius = (float)radius; nf.clear_ego = (float)clear_ego; nf.count = (int32_t)count; nf.density = (int32_t)density;
    }
    tde_near_field nf;
    at::Device dev;

  private:
    std::vector<at::Tensor> keep_;
};

class EnvHandle {
  public:
    EnvHandle(const Config &cfg, std::shared_ptr<World> world, const py::dict &state, int64_t B, int64_t A)
        : cfg_(cfg.c), world_(world->w), wkeep_(std::move(world)), dev_(wkeep_->dev)
    {
        TORCH_CHECK(tde_abi_version() == TDE_ABI_VERSION, "libtde_hip.so ABI ", tde_abi_version(), " != header ", TDE_ABI_VERSION);
        TORCH_CHECK(B >= 0 && A >= 1 && A <= TDE_MAX_AGENTS && (A & (A - 1)) == 0, "A must be a power of two <= ", TDE_MAX_AGENTS);
        std::memset(&state_, 0, sizeof(state_));
        fill_struct(&state_, kStateFields, state, B, A, dev_, keep_, "state");
        state_.B = static_cast<int32_t>(B);
        state_.A = static_cast<int32_t>(A);
    }

    // tde_env_step: one timestep of every env; `action` float32 [B, 2] on the device, read in place
    void step(const at::Tensor &action, int64_t flags)
    {
        tde_state st = state_;
        st.action = ptr<const float>(action, at::kFloat, 2 * (int64_t)state_.B, "action", dev_);
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_step(&cfg_, &world_, &st, cur_stream(dev_)), "tde_env_step");
    }

    void reset(const std::optional<at::Tensor> &mask, int64_t flags)
    {
        cfg_.flags = static_cast<uint32_t>(flags);
        const uint8_t *m = mask_ptr(mask, "mask");
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_reset(&cfg_, &world_, &state_, m, cur_stream(dev_)), "tde_env_reset");
    }

    void rollout(const at::Tensor &actions, const at::Tensor &reward, const at::Tensor &done, int64_t flags)
    {
        cfg_.flags = static_cast<uint32_t>(flags);
        TORCH_CHECK(actions.dim() == 3 && actions.size(1) == state_.B && actions.size(2) == 2, "actions must be [K, B, 2]");
        const int64_t K = actions.size(0);
        tde_rollout ro;
        ro.actions = ptr<const float>(actions, at::kFloat, K * state_.B * 2, "actions", dev_);
        ro.reward = ptr<float>(reward, at::kFloat, K * state_.B, "reward", dev_);
        ro.done = ptr<uint8_t>(done, at::kByte, K * state_.B, "done", dev_);
        ro.K = static_cast<int32_t>(K);
        ro.ldb = 0;
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_rollout(&cfg_, &world_, &state_, &ro, cur_stream(dev_)), "tde_env_rollout");
    }

    // tde_env_step_render: the timestep + the birdview as streams.size() sub-batches, each on its own stream (raw hipStream_t
    // values, e.g. torch.cuda.Stream.cuda_stream); `out` = None: the step only
    void step_render(const at::Tensor &action, int64_t flags, const std::optional<at::Tensor> &out, int64_t H, int64_t W, double fov,
                     int64_t n_stack, const std::optional<at::Tensor> &layers, int64_t phase, int64_t rflags,
                     const std::optional<at::Tensor> &fresh, const std::vector<int64_t> &streams)
    {
        tde_state st = state_;
        st.action = ptr<const float>(action, at::kFloat, 2 * (int64_t)state_.B, "action", dev_);
        cfg_.flags = static_cast<uint32_t>(flags);
        const int64_t ns = n_stack > 1 ? n_stack : 1;
        tde_render rd{};
        if (out) {
            rd.out = ptr<uint8_t>(*out, at::kByte, state_.B * 3 * ns * H * W, "out", dev_);
            rd.H = static_cast<int32_t>(H);
            rd.W = static_cast<int32_t>(W);
            rd.fov = static_cast<float>(fov);
            rd.n_stack = static_cast<int32_t>(n_stack);
            rd.layers = opt<uint8_t>(layers, at::kByte, state_.B * ns * H * W, "layers");
            rd.phase = static_cast<int32_t>(phase);
            rd.flags = static_cast<int32_t>(rflags);
            rd.fresh = mask_ptr(fresh, "fresh");
            rd.only = nullptr;
        }
        TORCH_CHECK(!streams.empty() && streams.size() <= 16, "streams: 1 to 16 raw stream handles");
        void *sv[16];
        for (size_t i = 0; i < streams.size(); ++i) sv[i] = reinterpret_cast<void *>(static_cast<uintptr_t>(streams[i]));
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_step_render(&cfg_, &world_, &st, out ? &rd : nullptr, sv, static_cast<int32_t>(streams.size())), "tde_env_step_render");
    }

    void render(const at::Tensor &out, int64_t H, int64_t W, double fov, int64_t n_stack, const std::optional<at::Tensor> &layers,
                int64_t phase, int64_t flags, const std::optional<at::Tensor> &fresh, const std::optional<at::Tensor> &only)
    {
        const int64_t ns = n_stack > 1 ? n_stack : 1;
        tde_render rd;
        rd.out = ptr<uint8_t>(out, at::kByte, state_.B * 3 * ns * H * W, "out", dev_);
        rd.H = static_cast<int32_t>(H);
        rd.W = static_cast<int32_t>(W);
        rd.fov = static_cast<float>(fov);
        rd.n_stack = static_cast<int32_t>(n_stack);
        rd.layers = opt<uint8_t>(layers, at::kByte, state_.B * ns * H * W, "layers");
        rd.phase = static_cast<int32_t>(phase);
        rd.flags = static_cast<int32_t>(flags);
        rd.fresh = mask_ptr(fresh, "fresh");
        rd.only = mask_ptr(only, "only");
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_render_ego(&cfg_, &world_, &state_, &rd, cur_stream(dev_)), "tde_render_ego");
    }

    // tde_env_reset_render: masked reset + the re-spawned views' first observation (their newest frame in place, older stack frames
    // blank) in one call; `phase` = the phase of the last full render
    void reset_render(const at::Tensor &mask, int64_t flags, const at::Tensor &out, int64_t H, int64_t W, double fov, int64_t n_stack,
                      const std::optional<at::Tensor> &layers, int64_t phase, int64_t rflags)
    {
        cfg_.flags = static_cast<uint32_t>(flags);
        const int64_t ns = n_stack > 1 ? n_stack : 1;
        tde_render rd{};
        rd.out = ptr<uint8_t>(out, at::kByte, state_.B * 3 * ns * H * W, "out", dev_);
        rd.H = static_cast<int32_t>(H); rd.W = static_cast<int32_t>(W); rd.fov = static_cast<float>(fov);
        rd.n_stack = static_cast<int32_t>(n_stack);
        rd.layers = opt<uint8_t>(layers, at::kByte, state_.B * ns * H * W, "layers");
        rd.phase = static_cast<int32_t>(phase);
        rd.flags = static_cast<int32_t>(rflags);
        const uint8_t *m = ptr<const uint8_t>(mask, at::kByte, state_.B, "mask", dev_);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_reset_render(&cfg_, &world_, &state_, m, &rd, cur_stream(dev_)), "tde_env_reset_render");
    }

    void state_obs(const at::Tensor &out)
    {
        float *p = ptr<float>(out, at::kFloat, (int64_t)state_.B * 8, "out", dev_);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_state_obs(&world_, &state_, p, cur_stream(dev_)), "tde_state_obs");
    }

    // tde_vector_obs: float32 [B, D] (D = 10 + 9 k_nbr + 3 n_rays) of the envs in `only` (all without it); ray_dir float32 [n_rays, 2]
    void vector_obs(const at::Tensor &out, const at::Tensor &ray_dir, int64_t k_nbr, int64_t n_rays, double nbr_radius, double ray_range,
                    double ray_step, const std::optional<at::Tensor> &only, int64_t flags)
    {
        TORCH_CHECK(k_nbr >= 0 && k_nbr <= TDE_VO_MAX_NBR && n_rays >= 0 && n_rays <= TDE_VO_MAX_RAYS, "vector_obs: k_nbr / n_rays out of range");
        const int64_t D = TDE_VO_EGO + TDE_VO_NBR * k_nbr + TDE_VO_RAY * n_rays;
        struct tde_vector_obs vo;
        std::memset(&vo, 0, sizeof(vo));
        vo.ray_dir = ptr<const float>(ray_dir, at::kFloat, 2 * n_rays, "ray_dir", dev_);
        vo.k_nbr = (int32_t)k_nbr;
        vo.n_rays = (int32_t)n_rays;
        vo.nbr_radius = (float)nbr_radius;
        vo.ray_range = (float)ray_range;
        vo.ray_step = (float)ray_step;
        float *p = ptr<float>(out, at::kFloat, (int64_t)state_.B * D, "out", dev_);
        const uint8_t *m = mask_ptr(only, "only");
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_vector_obs(&cfg_, &world_, &state_, &vo, m, p, cur_stream(dev_)), "tde_vector_obs");
    }

    // tde_plan_action: float32 [B, 2] ego actions of the envs in `only` (all without it); diag: optional int32 [B, 4] = tde_plan_diag rows
    void plan_action(const at::Tensor &out, const std::vector<double> &accel, const std::vector<double> &steer, int64_t horizon,
                     double v_target, double margin, double w_progress, double w_speed, double w_steer,
                     const std::optional<at::Tensor> &only, const std::optional<at::Tensor> &diag, int64_t flags)
    {
        TORCH_CHECK(!accel.empty() && !steer.empty() && accel.size() * steer.size() <= (size_t)TDE_PLAN_MAX_CAND,
                    "plan_action: accel x steer must hold 1 .. TDE_PLAN_MAX_CAND candidates");
        tde_planner pl = planner_of(horizon, v_target, margin, w_progress, w_speed, w_steer);
        for (size_t i = 0; i < accel.size(); ++i) pl.accel[i] = (float)accel[i];
        for (size_t i = 0; i < steer.size(); ++i) pl.steer[i] = (float)steer[i];
        pl.n_a = (int32_t)accel.size();
        pl.n_s = (int32_t)steer.size();
        float *p = ptr<float>(out, at::kFloat, (int64_t)state_.B * 2, "out", dev_);
        const uint8_t *m = mask_ptr(only, "only");
        tde_plan_diag *d = diag_ptr(diag);
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_plan_action(&cfg_, &world_, &state_, &pl, m, p, d, cur_stream(dev_)), "tde_plan_action");
    }

    // tde_score_plans: cost float32 [B, N] and fail_step int32 [B, N] of the N sequences of seq (float32 [B, N, K, 2], contiguous); action
    // float32 [B, 2] / diag int32 [B, 4]: optional, the winner's first action and its tde_plan_diag row
    void score_plans(const at::Tensor &seq, int64_t knot_len, int64_t tail, const at::Tensor &cost, const at::Tensor &fail_step,
                     int64_t horizon, double v_target, double margin, double w_progress, double w_speed, double w_steer,
                     const std::optional<at::Tensor> &only, const std::optional<at::Tensor> &action,
                     const std::optional<at::Tensor> &diag, int64_t flags, const std::optional<at::Tensor> &forecast)
    {
        score_plans_any(seq, knot_len, tail, cost, fail_step, horizon, v_target, margin, w_progress, w_speed, w_steer, only, action, diag, flags,
                        forecast, false);
    }

    // tde_score_plans_scene: score_plans' arguments, tensor checks and outputs; every sequence is judged in a scene that reacts to it
    void score_plans_scene(const at::Tensor &seq, int64_t knot_len, int64_t tail, const at::Tensor &cost, const at::Tensor &fail_step,
                           int64_t horizon, double v_target, double margin, double w_progress, double w_speed, double w_steer,
                           const std::optional<at::Tensor> &only, const std::optional<at::Tensor> &action,
                           const std::optional<at::Tensor> &diag, int64_t flags)
    {
        score_plans_any(seq, knot_len, tail, cost, fail_step, horizon, v_target, margin, w_progress, w_speed, w_steer, only, action, diag, flags,
                        std::nullopt, true);
    }

    void score_plans_any(const at::Tensor &seq, int64_t knot_len, int64_t tail, const at::Tensor &cost, const at::Tensor &fail_step,
                         int64_t horizon, double v_target, double margin, double w_progress, double w_speed, double w_steer,
                         const std::optional<at::Tensor> &only, const std::optional<at::Tensor> &action,
                         const std::optional<at::Tensor> &diag, int64_t flags, const std::optional<at::Tensor> &forecast, bool scene)
    {
        TORCH_CHECK(seq.dim() == 4 && seq.size(0) == state_.B && seq.size(3) == 2, "score_plans: seq must be [B, N, K, 2]");
        TORCH_CHECK(seq.is_contiguous(), "score_plans: seq must be contiguous (no copy of it is made)");
        const int64_t N = seq.size(1), K = seq.size(2);
        const tde_planner pl = planner_of(horizon, v_target, margin, w_progress, w_speed, w_steer);
        tde_plan_set ps;
        ps.seq = ptr<const float>(seq, at::kFloat, (int64_t)state_.B * N * K * 2, "seq", dev_);
        ps.N = (int32_t)N;
        ps.K = (int32_t)K;
        ps.knot_len = (int32_t)knot_len;
        ps.tail = (int32_t)tail;
        float *pc = ptr<float>(cost, at::kFloat, (int64_t)state_.B * N, "cost", dev_);
        int32_t *pf = ptr<int32_t>(fail_step, at::kInt, (int64_t)state_.B * N, "fail_step", dev_);
        const uint8_t *m = mask_ptr(only, "only");
        float *pa = opt<float>(action, at::kFloat, (int64_t)state_.B * 2, "action");
        tde_plan_diag *d = diag_ptr(diag);
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        if (forecast) {
            // float32 [B, T, A, 4], contiguous: the others' (x, y, psi, v) per step (tde_score_plans_forecast)
            const at::Tensor &fc = *forecast;
            TORCH_CHECK(fc.dim() == 4 && fc.size(0) == state_.B && fc.size(2) == state_.A && fc.size(3) == 4,
                        "score_plans: forecast must be [B, T, A, 4]");
            TORCH_CHECK(fc.is_contiguous(), "score_plans: forecast must be contiguous (no copy of it is made)");
            const float *pfc = ptr<const float>(fc, at::kFloat, fc.numel(), "forecast", dev_);
            check_rc(tde_score_plans_forecast(&cfg_, &world_, &state_, &pl, &ps, m, pc, pf, pa, d, pfc, (int32_t)fc.size(1), cur_stream(dev_)),
                     "tde_score_plans_forecast");
            return;
        }
        if (scene) {
            check_rc(tde_score_plans_scene(&cfg_, &world_, &state_, &pl, &ps, m, pc, pf, pa, d, cur_stream(dev_)), "tde_score_plans_scene");
            return;
        }
        check_rc(tde_score_plans(&cfg_, &world_, &state_, &pl, &ps, m, pc, pf, pa, d, cur_stream(dev_)), "tde_score_plans");
    }

    // tde_forecast_agents: out float32 [B, T, A, 4] = (x, y, psi, v) of every slot at each of the next T steps (rows of envs outside `only` untouched)
    void forecast_agents(const at::Tensor &out, const std::optional<at::Tensor> &only, int64_t flags)
    {
        TORCH_CHECK(out.dim() == 4 && out.size(0) == state_.B && out.size(2) == state_.A && out.size(3) == 4,
                    "forecast_agents: out must be [B, T, A, 4]");
        float *p = ptr<float>(out, at::kFloat, out.numel(), "out", dev_);
        const uint8_t *m = mask_ptr(only, "only");
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_forecast_agents(&cfg_, &world_, &state_, (int32_t)out.size(1), m, p, cur_stream(dev_)), "tde_forecast_agents");
    }

    // tde_forecast_scene: out float32 [B, T, A, 4] = (x, y, psi, v) of every slot, the ego included, at each of the next T steps under
    // ego_actions (float32 [B, T, 2], contiguous; none: the ego coasts), the leader sweep kept (rows of envs outside `only` untouched)
    void forecast_scene(const at::Tensor &out, const std::optional<at::Tensor> &ego_actions, const std::optional<at::Tensor> &only, int64_t flags)
    {
        TORCH_CHECK(out.dim() == 4 && out.size(0) == state_.B && out.size(2) == state_.A && out.size(3) == 4,
                    "forecast_scene: out must be [B, T, A, 4]");
        const int64_t T = out.size(1);
        float *p = ptr<float>(out, at::kFloat, out.numel(), "out", dev_);
        const float *pa = nullptr;
        if (ego_actions) {
            const at::Tensor &ea = *ego_actions;
            TORCH_CHECK(ea.dim() == 3 && ea.size(0) == state_.B && ea.size(1) == T && ea.size(2) == 2, "forecast_scene: ego_actions must be [B, T, 2]");
            TORCH_CHECK(ea.is_contiguous(), "forecast_scene: ego_actions must be contiguous (no copy of it is made)");
            pa = ptr<const float>(ea, at::kFloat, (int64_t)state_.B * T * 2, "ego_actions", dev_);
        }
        const uint8_t *m = mask_ptr(only, "only");
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_forecast_scene(&cfg_, &world_, &state_, (int32_t)T, pa, m, p, cur_stream(dev_)), "tde_forecast_scene");
    }

    // tde_ego_infractions: float32 [B, 4] = the ego's (offroad, collision, overlap count, 0) magnitudes of the state as it is (gym_env.py:427-428)
    void ego_infractions(const at::Tensor &out, int64_t flags)
    {
        float *p = ptr<float>(out, at::kFloat, (int64_t)state_.B * 4, "out", dev_);
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_ego_infractions(&cfg_, &world_, &state_, p, cur_stream(dev_)), "tde_ego_infractions");
    }

    // tde_env_post_step: magnitudes (optional) of the state a step without TDE_F_AUTORESET left + the re-spawn of the envs it finished
    void post_step(const std::optional<at::Tensor> &mag, int64_t flags)
    {
        float *p = opt<float>(mag, at::kFloat, (int64_t)state_.B * 4, "magnitudes");
        cfg_.flags = static_cast<uint32_t>(flags);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_post_step(&cfg_, &world_, &state_, p, cur_stream(dev_)), "tde_env_post_step");
    }

    // tde_env_reset_to: tde_env_reset with the scenario of env e given by scn[e] >= 0 (int32 [B]; without it every env draws)
    void reset_to(const std::optional<at::Tensor> &scn, const std::optional<at::Tensor> &mask, int64_t flags)
    {
        cfg_.flags = static_cast<uint32_t>(flags);
        const uint8_t *m = mask_ptr(mask, "mask");
        const int32_t *s = opt<const int32_t>(scn, at::kInt, state_.B, "scn");
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_env_reset_to(&cfg_, &world_, &state_, m, s, cur_stream(dev_)), "tde_env_reset_to");
    }

    // tde_eval_advance: plan int32 [R, B], round int32 [B], active uint8 [B], acc uint8 [B, 48], results uint8 [R, B, 48]
    // (tde_episode_record rows as raw bytes)
    void eval_advance(const at::Tensor &plan, const at::Tensor &round, const at::Tensor &active, const at::Tensor &acc,
                      const at::Tensor &results, int64_t flags)
    {
        static_assert(sizeof(tde_episode_record) == 48, "tde_episode_record rows are 48 bytes");
        TORCH_CHECK(plan.dim() == 2 && plan.size(0) >= 1 && plan.size(1) == state_.B, "plan must be [R >= 1, B]");
        const int64_t R = plan.size(0), B = state_.B;
        cfg_.flags = static_cast<uint32_t>(flags);
        tde_eval ev;
        std::memset(&ev, 0, sizeof(ev));
        ev.plan = ptr<const int32_t>(plan, at::kInt, R * B, "plan", dev_);
        ev.round = ptr<int32_t>(round, at::kInt, B, "round", dev_);
        ev.active = ptr<uint8_t>(active, at::kByte, B, "active", dev_);
        ev.acc = ptr<tde_episode_record>(acc, at::kByte, B * 48, "acc", dev_);
        ev.results = ptr<tde_episode_record>(results, at::kByte, R * B * 48, "results", dev_);
        ev.R = static_cast<int32_t>(R);
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_eval_advance(&cfg_, &world_, &state_, &ev, cur_stream(dev_)), "tde_eval_advance");
    }

    // tde_near_field_spawn: near-field traffic in the free slots of the masked envs (all without a mask)
    void near_field_spawn(const NearField &nf, const std::optional<at::Tensor> &mask, int64_t flags)
    {
        cfg_.flags = static_cast<uint32_t>(flags);
        TORCH_CHECK(nf.dev == dev_, "near_field is on ", nf.dev, ", expected ", dev_);
        const uint8_t *m = mask_ptr(mask, "mask");
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev_);
        check_rc(tde_near_field_spawn(&cfg_, &world_, &state_, &nf.nf, m, cur_stream(dev_)), "tde_near_field_spawn");
    }

    int64_t flags() const { return cfg_.flags; }
    int64_t num_envs() const { return state_.B; }
    int64_t agents_per_env() const { return state_.A; }
    // (for state_copy below, which launches on two handles' states)
    const tde_state &state() const { return state_; }
    const at::Device &device() const { return dev_; }

  private:
    // an optional tensor's checked pointer, NULL without it
    template <typename T> T *opt(const std::optional<at::Tensor> &t, at::ScalarType dt, int64_t numel, const char *name) const
    {
        return t ? ptr<T>(*t, dt, numel, name, dev_) : nullptr;
    }
    // ... of a uint8 [B] mask over the envs (`only`, `mask`, `fresh`)
    const uint8_t *mask_ptr(const std::optional<at::Tensor> &m, const char *name) const { return opt<const uint8_t>(m, at::kByte, state_.B, name); }
    // ... of the planner family's int32 [B, 4] diag output, as tde_plan_diag rows
    tde_plan_diag *diag_ptr(const std::optional<at::Tensor> &diag) const
    {
        static_assert(sizeof(tde_plan_diag) == 4 * sizeof(int32_t), "tde_plan_diag rows are four 32-bit words");
        return opt<tde_plan_diag>(diag, at::kInt, (int64_t)state_.B * 4, "diag");
    }
    // a tde_planner of the six scalars, its lattice empty (tde_plan_action's caller fills it; the plan-set judges do not read it)
    static tde_planner planner_of(int64_t horizon, double v_target, double margin, double w_progress, double w_speed, double w_steer)
    {
        tde_planner pl;
        std::memset(&pl, 0, sizeof(pl));
        pl.horizon = (int32_t)horizon;
        pl.v_target = (float)v_target;
        pl.margin = (float)margin;
        pl.w_progress = (float)w_progress;
        pl.w_speed = (float)w_speed;
        pl.w_steer = (float)w_steer;
        return pl;
    }

    tde_config cfg_;
    tde_world world_;
    std::shared_ptr<World> wkeep_;         // (owns the world's tensors)
    tde_state state_;
    at::Device dev_;
    std::vector<at::Tensor> keep_;         // the state's tensors
};

// tde_state_copy (include/tde_snapshot.h): env rows src_env[k] of `src`'s state into rows dst_env[k] of `dst`'s (the same handle: a fork).
// A launch on TWO states, so a function of two handles and not a method of one.  frames: (src_layers, dst_layers, src_obs, dst_obs) uint8
// tensors, each pair optional, with the ring's n_stack, plane and the two phases.
void state_copy(const EnvHandle &src, const EnvHandle &dst, const at::Tensor &src_env, const at::Tensor &dst_env,
                const std::optional<at::Tensor> &src_layers, const std::optional<at::Tensor> &dst_layers,
                const std::optional<at::Tensor> &src_obs, const std::optional<at::Tensor> &dst_obs, int64_t n_stack, int64_t plane,
                int64_t src_phase, int64_t dst_phase, int64_t flags)
{
    TORCH_CHECK(tde_snapshot_version() == TDE_SNAPSHOT_VERSION, "libtde_hip.so snapshot version ", tde_snapshot_version(), " != header ", TDE_SNAPSHOT_VERSION);
    const at::Device dev = dst.device();
    TORCH_CHECK(src.device() == dev, "src is on ", src.device(), ", dst on ", dev);
    const int64_t n = src_env.numel();
    const int32_t *ps = ptr<const int32_t>(src_env, at::kInt, n, "src_env", dev), *pd = ptr<const int32_t>(dst_env, at::kInt, n, "dst_env", dev);
    tde_snapshot_frames fr;
    std::memset(&fr, 0, sizeof(fr));
    const bool with_frames = src_layers || dst_layers || src_obs || dst_obs;
    if (with_frames) {
        TORCH_CHECK(n_stack >= 1 && n_stack <= TDE_SNAPSHOT_MAX_STACK && plane >= 1 && plane <= (1 << 24), "frames: n_stack / plane out of range");
        const int64_t sB = src.state().B, dB = dst.state().B, row = n_stack * plane;
        fr.src_layers = src_layers ? ptr<const uint8_t>(*src_layers, at::kByte, sB * row, "src_layers", dev) : nullptr;
        fr.dst_layers = dst_layers ? ptr<uint8_t>(*dst_layers, at::kByte, dB * row, "dst_layers", dev) : nullptr;
        fr.src_obs = src_obs ? ptr<const uint8_t>(*src_obs, at::kByte, sB * 3 * row, "src_obs", dev) : nullptr;
        fr.dst_obs = dst_obs ? ptr<uint8_t>(*dst_obs, at::kByte, dB * 3 * row, "dst_obs", dev) : nullptr;
        fr.n_stack = (int32_t)n_stack; fr.plane = (int32_t)plane; fr.src_phase = (int32_t)src_phase; fr.dst_phase = (int32_t)dst_phase;
    }
    tde_state to = dst.state();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    check_rc(tde_state_copy(&src.state(), &to, (int32_t)n, ps, pd, with_frames ? &fr : nullptr, (uint32_t)flags, cur_stream(dev)), "tde_state_copy");
}

// ---- operator level: the SimulatorInterface methods GymEnv calls (include/tde_hip.h, first block), torch tensors in / out ----

// tde_kinematics_step: KinematicBicycle.step for n agents, in place (ref gym_env.py:117)
void kinematics_step(const at::Tensor &x, const at::Tensor &y, const at::Tensor &psi, const at::Tensor &v, const at::Tensor &lr,
                     const at::Tensor &action, const std::optional<at::Tensor> &present, double dt)
{
    const int64_t n = x.numel();
    const at::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    check_rc(tde_kinematics_step(n, ptr<float>(x, at::kFloat, n, "x", dev), ptr<float>(y, at::kFloat, n, "y", dev),
                                 ptr<float>(psi, at::kFloat, n, "psi", dev), ptr<float>(v, at::kFloat, n, "v", dev),
                                 ptr<float>(lr, at::kFloat, n, "lr", dev),
                                 present ? ptr<uint8_t>(*present, at::kByte, n, "present", dev) : nullptr,
                                 ptr<float>(action, at::kFloat, 2 * n, "action", dev), (float)dt, cur_stream(dev)),
             "tde_kinematics_step");
}

// tde_compute_collision: compute_collision() > 0 per agent -> uint8 [B * A] (ref gym_env.py:143)
at::Tensor compute_collision(int64_t B, int64_t A, const at::Tensor &x, const at::Tensor &y, const at::Tensor &psi,
                             const at::Tensor &length, const at::Tensor &width, const at::Tensor &present)
{
    const int64_t n = B * A;
    const at::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    at::Tensor out = at::empty({n}, at::TensorOptions().dtype(at::kByte).device(dev));
    check_rc(tde_compute_collision((int32_t)B, (int32_t)A, ptr<float>(x, at::kFloat, n, "x", dev), ptr<float>(y, at::kFloat, n, "y", dev),
                                   ptr<float>(psi, at::kFloat, n, "psi", dev), ptr<float>(length, at::kFloat, n, "length", dev),
                                   ptr<float>(width, at::kFloat, n, "width", dev), ptr<uint8_t>(present, at::kByte, n, "present", dev),
                                   out.data_ptr<uint8_t>(), cur_stream(dev)),
             "tde_compute_collision");
    return out;
}

// tde_compute_offroad: compute_offroad() > 0 per agent -> uint8 [B * A] (ref gym_env.py:142)
at::Tensor compute_offroad(int64_t B, int64_t A, const at::Tensor &x, const at::Tensor &y, const at::Tensor &psi,
                           const at::Tensor &length, const at::Tensor &width, const at::Tensor &present, const World &world,
                           const at::Tensor &map_of_env, double threshold)
{
    const int64_t n = B * A;
    const at::Device dev = x.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    at::Tensor out = at::empty({n}, at::TensorOptions().dtype(at::kByte).device(dev));
    check_rc(tde_compute_offroad((int32_t)B, (int32_t)A, ptr<float>(x, at::kFloat, n, "x", dev), ptr<float>(y, at::kFloat, n, "y", dev),
                                 ptr<float>(psi, at::kFloat, n, "psi", dev), ptr<float>(length, at::kFloat, n, "length", dev),
                                 ptr<float>(width, at::kFloat, n, "width", dev), ptr<uint8_t>(present, at::kByte, n, "present", dev),
                                 &world.w, ptr<int32_t>(map_of_env, at::kInt, B, "map_of_env", dev),
                                 (float)threshold, out.data_ptr<uint8_t>(), cur_stream(dev)),
             "tde_compute_offroad");
    return out;
}

// tde_waypoint_reward (ref gym_env.py:391-437): pre / post = (x, y, psi, v) stacked [4][n]; steps / target_idx / reached
// int32 [n], updated in place; -> (reward f32 [n], terminated u8 [n], truncated u8 [n], info f64 [n][4], info_reached i32 [n])
std::vector<at::Tensor> waypoint_reward(const Config &cfg, const at::Tensor &pre, const at::Tensor &post, const at::Tensor &offroad,
                                        const at::Tensor &collided, const std::optional<at::Tensor> &tl, const at::Tensor &wp_xy,
                                        const at::Tensor &wp_n, const at::Tensor &scn, const at::Tensor &steps,
                                        const at::Tensor &target_idx, const at::Tensor &reached)
{
    TORCH_CHECK(pre.dim() == 2 && pre.size(0) == 4 && post.dim() == 2 && post.size(0) == 4, "pre / post must be [4][n]");
    TORCH_CHECK(wp_xy.dim() == 3 && wp_xy.size(2) == 2, "wp_xy must be [S][NW][2]");
    const int64_t n = pre.size(1), S = wp_xy.size(0), NW = wp_xy.size(1);
    const at::Device dev = pre.device();
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);
    const float *p0 = ptr<float>(pre, at::kFloat, 4 * n, "pre", dev), *p1 = ptr<float>(post, at::kFloat, 4 * n, "post", dev);
    const auto opt = at::TensorOptions().device(dev);
    at::Tensor reward = at::empty({n}, opt.dtype(at::kFloat)), term = at::empty({n}, opt.dtype(at::kByte)),
               trunc = at::empty({n}, opt.dtype(at::kByte)), info = at::empty({n, 4}, opt.dtype(at::kDouble)),
               info_reached = at::empty({n}, opt.dtype(at::kInt));
    check_rc(tde_waypoint_reward(&cfg.c, (int32_t)n, p0, p0 + n, p0 + 2 * n, p0 + 3 * n, p1,
                                 p1 + n, p1 + 2 * n, p1 + 3 * n, ptr<uint8_t>(offroad, at::kByte, n, "offroad", dev),
                                 ptr<uint8_t>(collided, at::kByte, n, "collided", dev),
                                 tl ? ptr<uint8_t>(*tl, at::kByte, n, "tl", dev) : nullptr,
                                 ptr<double>(wp_xy, at::kDouble, S * NW * 2, "wp_xy", dev), ptr<int32_t>(wp_n, at::kInt, S, "wp_n", dev),
                                 (int32_t)NW, ptr<int32_t>(scn, at::kInt, n, "scn", dev), ptr<int32_t>(steps, at::kInt, n, "steps", dev),
                                 ptr<int32_t>(target_idx, at::kInt, n, "target_idx", dev), ptr<int32_t>(reached, at::kInt, n, "reached", dev),
                                 reward.data_ptr<float>(), term.data_ptr<uint8_t>(), trunc.data_ptr<uint8_t>(), info.data_ptr<double>(),
                                 info_reached.data_ptr<int32_t>(), cur_stream(dev)),
             "tde_waypoint_reward");
    return {reward, term, trunc, info, info_reached};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "PyTorch-ROCm C++ extension over the C-ABI of libtde_hip.so (include/tde_hip.h)";
    m.def("abi_version", []() { return tde_abi_version(); });
    m.def("kinematics_step", &kinematics_step, py::arg("x"), py::arg("y"), py::arg("psi"), py::arg("v"), py::arg("lr"),
          py::arg("action"), py::arg("present") = py::none(), py::arg("dt") = 0.1);
    m.def("compute_collision", &compute_collision, py::arg("B"), py::arg("A"), py::arg("x"), py::arg("y"), py::arg("psi"),
          py::arg("length"), py::arg("width"), py::arg("present"));
    m.def("compute_offroad", &compute_offroad, py::arg("B"), py::arg("A"), py::arg("x"), py::arg("y"), py::arg("psi"),
          py::arg("length"), py::arg("width"), py::arg("present"), py::arg("world"), py::arg("map_of_env"),
          py::arg("threshold") = 0.5);
    m.def("waypoint_reward", &waypoint_reward, py::arg("cfg"), py::arg("pre"), py::arg("post"), py::arg("offroad"),
          py::arg("collided"), py::arg("tl"), py::arg("wp_xy"), py::arg("wp_n"), py::arg("scn"), py::arg("steps"),
          py::arg("target_idx"), py::arg("reached"));
    m.def("state_copy", &state_copy, py::arg("src"), py::arg("dst"), py::arg("src_env"), py::arg("dst_env"), py::arg("src_layers"),
          py::arg("dst_layers"), py::arg("src_obs"), py::arg("dst_obs"), py::arg("n_stack"), py::arg("plane"), py::arg("src_phase"),
          py::arg("dst_phase"), py::arg("flags"));
    py::class_<Config>(m, "Config", "tde_config by value, from its bytes").def(py::init<const py::bytes &>(), py::arg("raw"));
    py::class_<World, std::shared_ptr<World>>(m, "World", "tde_world over named device tensors (kept alive)")
        .def(py::init<const py::dict &, const py::dict &, int64_t>(), py::arg("tensors"), py::arg("ints"), py::arg("device_index"));
    py::class_<NearField>(m, "NearField", "tde_near_field over named device tensors (kept alive)")
        .def(py::init<const py::dict &, int64_t, int64_t, int64_t, int64_t, double, double, int64_t, int64_t, int64_t>(), py::arg("tensors"),
             py::arg("S"), py::arg("A"), py::arg("NC"), py::arg("K"), py::arg("radius"), py::arg("clear_ego"), py::arg("count"),
             py::arg("density"), py::arg("device_index"));
    py::class_<EnvHandle>(m, "EnvHandle")
        .def(py::init<const Config &, std::shared_ptr<World>, const py::dict &, int64_t, int64_t>(), py::arg("cfg"), py::arg("world"),
             py::arg("state"), py::arg("B"), py::arg("A"))
        .def("step", &EnvHandle::step, py::arg("action"), py::arg("flags"))
        .def("reset", &EnvHandle::reset, py::arg("mask"), py::arg("flags"))
        .def("rollout", &EnvHandle::rollout, py::arg("actions"), py::arg("reward"), py::arg("done"), py::arg("flags"))
        .def("render", &EnvHandle::render, py::arg("out"), py::arg("H"), py::arg("W"), py::arg("fov"), py::arg("n_stack"),
             py::arg("layers"), py::arg("phase"), py::arg("flags"), py::arg("fresh"), py::arg("only"))
        .def("step_render", &EnvHandle::step_render, py::arg("action"), py::arg("flags"), py::arg("out"), py::arg("H"), py::arg("W"),
             py::arg("fov"), py::arg("n_stack"), py::arg("layers"), py::arg("phase"), py::arg("rflags"), py::arg("fresh"), py::arg("streams"))
        .def("reset_render", &EnvHandle::reset_render, py::arg("mask"), py::arg("flags"), py::arg("out"), py::arg("H"), py::arg("W"), py::arg("fov"),
             py::arg("n_stack"), py::arg("layers"), py::arg("phase"), py::arg("rflags"))
        .def("state_obs", &EnvHandle::state_obs)
        .def("ego_infractions", &EnvHandle::ego_infractions, py::arg("out"), py::arg("flags"))
        .def("post_step", &EnvHandle::post_step, py::arg("magnitudes"), py::arg("flags"))
        .def("near_field_spawn", &EnvHandle::near_field_spawn, py::arg("nf"), py::arg("mask"), py::arg("flags"))
        .def("reset_to", &EnvHandle::reset_to, py::arg("scn"), py::arg("mask"), py::arg("flags"))
        .def("eval_advance", &EnvHandle::eval_advance, py::arg("plan"), py::arg("round"), py::arg("active"), py::arg("acc"),
             py::arg("results"), py::arg("flags"))
        .def("vector_obs", &EnvHandle::vector_obs, py::arg("out"), py::arg("ray_dir"), py::arg("k_nbr"), py::arg("n_rays"),
             py::arg("nbr_radius"), py::arg("ray_range"), py::arg("ray_step"), py::arg("only"), py::arg("flags"))
        .def("plan_action", &EnvHandle::plan_action, py::arg("out"), py::arg("accel"), py::arg("steer"), py::arg("horizon"),
             py::arg("v_target"), py::arg("margin"), py::arg("w_progress"), py::arg("w_speed"), py::arg("w_steer"), py::arg("only"),
             py::arg("diag"), py::arg("flags"))
        .def("score_plans", &EnvHandle::score_plans, py::arg("seq"), py::arg("knot_len"), py::arg("tail"), py::arg("cost"),
             py::arg("fail_step"), py::arg("horizon"), py::arg("v_target"), py::arg("margin"), py::arg("w_progress"), py::arg("w_speed"),
             py::arg("w_steer"), py::arg("only"), py::arg("action"), py::arg("diag"), py::arg("flags"), py::arg("forecast") = py::none())
        .def("score_plans_scene", &EnvHandle::score_plans_scene, py::arg("seq"), py::arg("knot_len"), py::arg("tail"), py::arg("cost"),
             py::arg("fail_step"), py::arg("horizon"), py::arg("v_target"), py::arg("margin"), py::arg("w_progress"), py::arg("w_speed"),
             py::arg("w_steer"), py::arg("only"), py::arg("action"), py::arg("diag"), py::arg("flags"))
        .def("forecast_agents", &EnvHandle::forecast_agents, py::arg("out"), py::arg("only"), py::arg("flags"))
        .def("forecast_scene", &EnvHandle::forecast_scene, py::arg("out"), py::arg("ego_actions"), py::arg("only"), py::arg("flags"))
        .def_property_readonly("flags", &EnvHandle::flags)
        .def_property_readonly("num_envs", &EnvHandle::num_envs)
        .def_property_readonly("agents_per_env", &EnvHandle::agents_per_env);
}
