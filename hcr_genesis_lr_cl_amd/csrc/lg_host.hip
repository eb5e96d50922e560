// lg_host.hip -- host side of the library: the C ABI of include/lgsim.h (engine handle, launch selection, profiling timers).
// The kernels themselves are instantiated in lg_inst.hip (lg_kernel.h: one leg per lane; lg_quad.h: one vector component per lane) and
// reached through the launchers declared in lg_shared.h.
#include "lg_shared.h"
#include "lg_dpp_kat.h"
#include <algorithm>
#include <unistd.h>

// ---------------------------------------------------------------------------------------------
// sliding observation history ran out of slack: move the newest stack-1 frames of every row back to frames [1, stack)
__global__ __launch_bounds__(256) void obs_compact_kernel(float *buf, int n_rows, int row, int frame, int stack, int from) {
    const int per = (stack - 1) * frame;
    const long long total = (long long)n_rows * per;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int e = (int)(t / per), i = (int)(t % per);
        buf[(size_t)e * row + frame + i] = buf[(size_t)e * row + (size_t)(from + 1) * frame + i];
    }
}

// =============================== host side: the C ABI ==========================================
static thread_local std::string g_err;
static int fail(const std::string &m) { g_err = m; return 1; }
int lg_fail_msg(const std::string &m) { return fail(m); }   // for the other translation units of the library (lg_rollout.hip)
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(std::string(#x) + ": " + hipGetErrorString(_e)); } while (0)

struct LgEngine {
    LgModelDesc model; LgSimOptions opts; LgTaskCfg task;
    LgModelDesc *d_model = nullptr; LgSimOptions *d_opts = nullptr; LgTaskCfg *d_task = nullptr; LgHot *d_hot = nullptr;
    float *d_lane = nullptr;
    const int16_t *hf = nullptr;
    LgBuffers bufs; bool bound = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    LgHot hot;           // host copy of the hot block (upload_hot)
    int obs_win = 0;     // window of the latest stacked observation (obs_slack > 0)
    int obs_set = 0;     // copy of the observation buffers the latest observation launch wrote (obs_sets == 2)
    std::string last_kernel;   // launcher instantiation(s) of the latest lg_step (lg_last_kernel)
    // fixed by the model (model_frames): KParams.k.joint_axis / .jrot_identity, and whether the component-per-lane kernels apply
    int joint_axis[4], jrot_identity; bool quad_ok;
    // bounded run-ahead: the host never gets more than ~128 lg_step calls ahead of the device (see lg_step)
    hipEvent_t ra_ev[4] = {nullptr, nullptr, nullptr, nullptr}; long long ra_calls = 0;
    // sampling timer of the physics kernel (lg_profile)
    int prof_stride = 0, prof_count = 0; long long prof_seen = 0;
    std::vector<hipEvent_t> prof_ev;
};

extern "C" const char *lg_last_error(void) { return g_err.c_str(); }
extern "C" int lg_abi_version(void) { return LG_ABI_VERSION; }

static int upload_hot(LgEngine *h) {
    LgHot hot;
    fill_hot(hot, h->task, h->opts, h->model);
    h->hot = hot;
    if (!h->d_hot) { hipError_t e = hipMalloc(&h->d_hot, 1024); if (e != hipSuccess) return fail(std::string("hipMalloc(hot): ") + hipGetErrorString(e)); }
    HIPCHK(hipMemset(h->d_hot, 0, 1024));
    HIPCHK(hipMemcpy(h->d_hot, &hot, sizeof(LgHot), hipMemcpyHostToDevice));
    // the lane table of the component-per-lane kernels follows the model and the options (lg_shared.h)
    std::vector<float> lt(LG_LT_STG * 256);
    lg_fill_lane_table(lt.data(), h->model, h->opts);
    if (!h->d_lane) { hipError_t e = hipMalloc(&h->d_lane, lt.size() * sizeof(float)); if (e != hipSuccess) return fail(std::string("hipMalloc(lane table): ") + hipGetErrorString(e)); }
    HIPCHK(hipMemcpy(h->d_lane, lt.data(), lt.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

static int validate_model(const LgModelDesc *m) {
    if (m->n_legs != 2 && m->n_legs != 4) return fail("lg_create: engine supports 2 or 4 legs");
    const int J = m->n_bodies == 1 + 3 * m->n_legs ? 3 : 4;     // joints per leg
    if (m->n_bodies != 1 + J * m->n_legs || (J == 4 && m->n_legs != 2))
        return fail("lg_create: n_bodies must be 1 + 3*n_legs (2 or 4 legs of 3 revolute joints) or 1 + 4*2 (two legs of 4)");
    if (m->n_links < m->n_bodies || m->n_links > LG_MAX_LINKS) return fail("lg_create: bad n_links");
    if (m->n_spheres < m->n_legs || m->n_spheres > LG_MAX_SPHERES) return fail("lg_create: bad n_spheres");
    for (int l = 0; l < m->n_legs; l++) {
        int fl = m->foot_link[l], fsph = m->foot_sphere[l];
        if (fl < 4 || fl >= m->n_links) return fail("lg_create: foot link index out of range");
        if (fsph < 0 || fsph >= m->n_spheres || m->sph_body[fsph] != J + J * l) return fail("lg_create: foot sphere must sit on the last body of its leg");
        // kernel assumes the four link rows of a leg are contiguous: [hip, thigh, calf, foot] (the foot a kept link of the calf body) or,
        // with four joints, the four bodies themselves (the foot is the last one)
        for (int k = 0; k < 3; k++)
            if (m->link_body[fl - 3 + k] != 1 + J * l + k) return fail("lg_create: leg links must be contiguous and end with the foot");
        if (m->link_body[fl] != J + J * l) return fail("lg_create: foot link must move with the last body of its leg");
    }
    if (m->link_body[0] != 0) return fail("lg_create: link 0 must be the base");
    for (int l = 0; l < m->n_legs; l++) {   // register-resident sphere tables of the kernel: 2 / 2 / [3 /] 5 (+foot) per chain body
        const int *st = m->body_sph_start + 1 + J * l;
        if (st[1] - st[0] > 2 || st[2] - st[1] > 2 || (J == 4 && st[3] - st[2] > 3) || st[J] - st[J - 1] > 6)
            return fail("lg_create: too many collision spheres on a leg body (max 2/2/5+foot, or 2/2/3/5+foot with four joints)");
    }
    if ((m->body_sph_start[1] - m->body_sph_start[0] + m->n_legs - 1) / m->n_legs > 4) return fail("lg_create: too many base collision spheres (max 4 per leg lane)");
    for (int b = 0; b <= m->n_bodies; b++)
        if (m->body_sph_start[b] < 0 || m->body_sph_start[b] > m->n_spheres || (b && m->body_sph_start[b] < m->body_sph_start[b - 1]))
            return fail("lg_create: body_sph_start not monotone");
    for (int b = 0; b < m->n_bodies; b++)
        if (!(m->mass[b] > 0.f)) return fail("lg_create: non-positive body mass");
    return 0;
}

// identity joint frames and hip-x / thigh-y / knee-y (/ y) axes: what the component-per-lane kernels are specialised for (lg_quad.h)
static void model_frames(LgEngine *h) {
    const LgModelDesc &m = h->model;
    const int J = m.n_bodies == 1 + 3 * m.n_legs ? 3 : 4;     // joints per leg (validate_model)
    h->joint_axis[3] = -1;
    for (int j = 0; j < J; j++) {
        int code = -2;
        for (int l = 0; l < m.n_legs; l++) {
            const float *ax = m.axis[1 + J * l + j];
            int c = -1;
            for (int k = 0; k < 3; k++)
                if (fabsf(fabsf(ax[k]) - 1.f) < 1e-6f && fabsf(ax[(k + 1) % 3]) < 1e-6f && fabsf(ax[(k + 2) % 3]) < 1e-6f) c = k;
            code = (code == -2 || code == c) ? c : -1;
        }
        h->joint_axis[j] = code;
    }
    h->jrot_identity = 1;
    for (int b = 1; b < m.n_bodies; b++)
        for (int k = 0; k < 9; k++)
            if (m.jrot[b][k] != ((k % 4 == 0) ? 1.f : 0.f)) h->jrot_identity = 0;
    h->quad_ok = h->jrot_identity && h->joint_axis[0] == 0 && h->joint_axis[1] == 1 && h->joint_axis[2] == 1 && (J == 3 || h->joint_axis[3] == 1);
}

extern "C" int lg_create(const LgModelDesc *model, const LgSimOptions *opts, const LgTaskCfg *task, LgHandle *out) {
    if (!model || !opts || !task || !out) return fail("lg_create: null argument");
    if (validate_model(model)) return 1;
    if (!(opts->dt > 0.f) || opts->decimation < 1 || opts->decimation > 64) return fail("lg_create: bad dt/decimation");
    if (opts->contact_iters < 1 || opts->contact_iters > 16) return fail("lg_create: contact_iters must be in [1,16]");
    if (task->obs_slack < 0 || (task->obs_slack > 0 && (task->obs_slack < task->obs_stack || task->obs_slack < task->priv_stack)))
        return fail("lg_create: obs_slack must be 0 or at least as large as the history stacks");
    if (task->obs_sets > 1 && task->obs_slack > 0 && (task->obs_slack <= task->obs_stack || task->obs_slack <= task->priv_stack))
        return fail("lg_create: with two observation sets obs_slack must exceed the history stacks");
    if (task->obs_sets > 2 && (task->obs_stack > 1 || task->priv_stack > 1))
        return fail("lg_create: more than two observation sets (rollout-resident observations) need unstacked observations");
    if (task->obs_sets > 4096) return fail("lg_create: obs_sets out of range");
    LgEngine *h = new LgEngine();
    h->model = *model; h->opts = *opts; h->task = *task;
    model_frames(h);
    memset(&h->bufs, 0, sizeof(h->bufs));
    hipError_t e;
    if ((e = hipMalloc(&h->d_model, MODEL_STG * BLOCK * 16)) != hipSuccess || (e = hipMalloc(&h->d_opts, sizeof(LgSimOptions))) != hipSuccess ||
        (e = hipMalloc(&h->d_task, sizeof(LgTaskCfg))) != hipSuccess) { delete h; return fail(std::string("lg_create: hipMalloc: ") + hipGetErrorString(e)); }
    HIPCHK(hipMemset(h->d_model, 0, MODEL_STG * BLOCK * 16));
    HIPCHK(hipMemcpy(h->d_model, model, sizeof(LgModelDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_opts, opts, sizeof(LgSimOptions), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_task, task, sizeof(LgTaskCfg), hipMemcpyHostToDevice));
    if (upload_hot(h)) return 1;
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    *out = h;
    return 0;
}

extern "C" int lg_destroy(LgHandle h) {
    if (!h) return 0;
    (void)hipFree(h->d_model); (void)hipFree(h->d_opts); (void)hipFree(h->d_task); (void)hipFree(h->d_hot); (void)hipFree(h->d_lane);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    for (hipEvent_t ev : h->prof_ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : h->ra_ev) if (ev) (void)hipEventDestroy(ev);
    delete h;
    return 0;
}

extern "C" int lg_set_task(LgHandle h, const LgTaskCfg *task) {
    if (!h || !task) return fail("lg_set_task: null argument");
    h->task = *task;
    HIPCHK(hipMemcpy(h->d_task, task, sizeof(LgTaskCfg), hipMemcpyHostToDevice));
    return upload_hot(h);
}

extern "C" int lg_set_terrain(LgHandle h, const int16_t *hf, int32_t rows, int32_t cols) {
    if (!h) return fail("lg_set_terrain: null handle");
    if (hf && (rows < 2 || cols < 2)) return fail("lg_set_terrain: heightfield needs at least 2x2 samples");
    h->hf = hf;
    h->opts.terrain_rows = hf ? rows : 0;
    h->opts.terrain_cols = hf ? cols : 0;
    HIPCHK(hipMemcpy(h->d_opts, &h->opts, sizeof(LgSimOptions), hipMemcpyHostToDevice));
    return upload_hot(h);
}

extern "C" int lg_bind(LgHandle h, const LgBuffers *b) {
    if (!h || !b) return fail("lg_bind: null argument");
    if (b->n_envs < 1) return fail("lg_bind: n_envs must be positive");
#define REQ(f) if (!b->f) return fail("lg_bind: required buffer " #f " is NULL")
    REQ(base_pos); REQ(base_quat); REQ(base_lin_vel_w); REQ(base_ang_vel_w); REQ(dof_pos); REQ(dof_vel);
    REQ(base_lin_vel); REQ(base_ang_vel); REQ(projected_gravity); REQ(base_euler);
    REQ(last_base_lin_vel); REQ(last_base_ang_vel); REQ(last_dof_vel); REQ(last_feet_vel);
    REQ(torques); REQ(link_contact_forces); REQ(feet_pos); REQ(feet_vel); REQ(env_origins);
#undef REQ
    h->bufs = *b;
    h->bound = true;
    return 0;
}

static int prof_begin(LgEngine *h, hipStream_t st) {
    if (h->prof_stride <= 0 || (h->prof_seen++ % h->prof_stride) != 0 || h->prof_count >= 1024) return -1;
    if ((int)h->prof_ev.size() < 2 * (h->prof_count + 1)) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
        h->prof_ev.push_back(a); h->prof_ev.push_back(b);
    }
    (void)st;
    return h->prof_count++;
}
static bool flat_noise_ok(const LgEngine *h) {   // commands and actions carry no observation noise (go2.py:92-117)
    const int A = h->model.n_bodies - 1;
    for (int i = 0; i < 3; i++) if (h->task.noise_vec[i] != 0.f) return false;
    for (int i = 0; i < A; i++) if (h->task.noise_vec[9 + 2 * A + i] != 0.f) return false;
    return true;
}

// ---- task profiles (lg_shared.h LG_PROF_*): each predicate checks that the task really has every switch its profile's instantiations
//      hard-wire.  inj: the injected-uniform test instantiations (rand_in REQUIRED instead of forbidden).  No side effects.
static bool hf_bound(const LgEngine *h) { return h->hf != nullptr && h->opts.terrain_rows > 0; }
static bool uniforms_ok(const LgEngine *h, bool inj) { return inj ? h->bufs.rand_in != nullptr : !h->bufs.rand_in; }
static bool rewards_ok(const LgEngine *h, int prof) { return ((unsigned)h->hot.reward_mask & lg_tail_reward_excluded(prof)) == 0; }
static bool window_stacks(const LgEngine *h) {   // sliding-window stacks of both outputs, one set or two behind obs_dirty
    const LgTaskCfg &t = h->task; return t.obs_slack > 0 && t.obs_stack > 1 && t.priv_stack > 1 && t.obs_sets <= 2 && (t.obs_sets < 2 || h->bufs.obs_dirty);
}
static bool offset_fits(const LgEngine *h, int stack, int frame) {   // 32-bit byte offsets into an observation allocation (lg_quad.h)
    return (double)h->bufs.n_envs * (stack + h->task.obs_slack) * frame * 4.0 < 4.0e9; }

// biped_profile: tron1_pf_ee (TRON1_PF_EE = the component-layout tail of lg_quad.h for the three-joint biped)
static bool biped_profile(const LgEngine *h, bool inj) {
    const LgTaskCfg &t = h->task; const LgBuffers &b = h->bufs;
    if (h->model.n_bodies != 7 || !hf_bound(h)) return false;
    const int K = __builtin_popcount(h->model.state_link_mask), P = h->opts.n_height_points, A = 6, F = 2;
    return t.obs_layout == LG_OBS_TRON1_EE && t.gait_mode == 2 && t.double_shift == 1 && t.cat_enable == 0 && t.behavior_resample_steps == 0 &&
           window_stacks(h) && uniforms_ok(h, inj) &&
           t.obs_frame == 9 + 3 * A + 2 * F && t.priv_frame == t.obs_frame + 7 + 2 * A + 3 + F + K + P + 3 * F + 9 * F && t.num_labels == 3 + K + F + 3 * F &&
           P > 0 && P <= 7 * 8 && h->opts.feet_terrain_info && b.priv_obs_buf && b.labels_buf && b.task_state && b.rand_push_vels &&
           t.task_state_width == LG_TASK_STATE_BIPED && b.link_contact_states &&
           (!t.terrain_curriculum || (b.terrain_levels && b.terrain_types && b.terrain_origins && b.env_origins)) &&
           (!t.dr_joint_on || (b.joint_armature && b.joint_friction && b.joint_damping)) &&
           (t.slots.reset_root_xy & 3) != 3 &&       // the two root xy draws share a Philox block
           offset_fits(h, t.priv_stack, t.priv_frame) && offset_fits(h, t.obs_stack, t.obs_frame) &&
           t.noise_vec[0] == 0.f && t.noise_vec[1] == 0.f && t.noise_vec[2] == 0.f &&    // commands carry no observation noise (tron1_pf_ee.py:322-342)
           rewards_ok(h, LG_PROF_TRON1_PF_EE);
}
// flat_profile: the plain go2-on-a-plane task (GO2_FLAT), every switch the FLAT instantiations hard-wire (env_step_body) really has that value
static bool flat_profile(const LgEngine *h, bool inj) {
    const LgTaskCfg &t = h->task; const LgSimOptions &o = h->opts; const LgBuffers &b = h->bufs;
    return t.obs_layout == LG_OBS_GO2 && t.gait_mode == 0 && t.double_shift == 0 && t.obs_stack == 1 && t.obs_slack == 0 && t.priv_frame == 0 &&
           t.priv_stack <= 1 && t.num_priv_obs == 0 && t.terrain_curriculum == 0 && t.custom_origins == 0 && t.sit_percent == 0.f &&
           t.behavior_resample_steps == 0 && t.num_labels == 0 && t.cat_enable == 0 && t.noise_vec[9 + 6 * h->model.n_legs] == 0.f && t.air_time_cmd_dims != 3 &&
           h->model.n_bodies == 1 + 3 * h->model.n_legs &&
           o.n_height_points == 0 && o.terrain_rows == 0 && o.feet_terrain_info == 0 && !b.link_contact_states && !b.task_state && !h->hf &&
           uniforms_ok(h, inj) && !b.joint_armature && !t.dr_joint_on && !t.dr_pd_on && t.reset_lin_vel_span == 0.f && t.reset_ang_vel_span == 0.f && flat_noise_ok(h) &&
           (double)b.n_envs * (9 + 9 * h->model.n_legs) * 4.0 < 4.0e9 &&      // 32-bit byte offsets into one set of the observation rows (lg_quad.h)
           rewards_ok(h, LG_PROF_GO2_FLAT);
}
// wtw_profile: go2_wtw on the plane (GO2_WTW): sliding-window stacks of 61 | 99-wide frames, Philox draws, no per-env joint parameters,
// no noise on commands / actions
static bool wtw_profile(const LgEngine *h, bool inj) {
    const LgTaskCfg &t = h->task; const LgSimOptions &o = h->opts; const LgBuffers &b = h->bufs;
    return t.obs_layout == LG_OBS_GO2_WTW && t.gait_mode == 1 && t.double_shift == 1 && t.terrain_curriculum == 0 && t.custom_origins == 0 &&
           t.sit_percent == 0.f && t.num_labels == 0 && t.cat_enable == 0 && t.noise_vec[9 + 6 * h->model.n_legs] == 0.f &&
           o.n_height_points == 0 && o.terrain_rows == 0 && o.feet_terrain_info == 0 && !b.link_contact_states && !h->hf && b.task_state &&
           t.obs_frame == 61 && t.priv_frame == 61 + 10 + 6 * h->model.n_legs + h->model.n_legs &&
           window_stacks(h) && uniforms_ok(h, inj) && !b.joint_armature && !t.dr_joint_on && flat_noise_ok(h) &&
           h->model.n_legs == 4 && h->model.n_bodies == 13 && b.priv_obs_buf && b.rand_push_vels && rewards_ok(h, LG_PROF_GO2_WTW);
}
// rough_profile: the Go2-rough family on a heightfield (lg_quad.h HFC) -- GO2_EE (go2_ee packaging), GO2_PROGRAM (observation programs: go2_ts / go2_cts /
// go2_dreamwaq / go2_cat) or NONE.  No gait clock, no sit pose, no noise on actions; terrain, curriculum, stacks and (GO2_PROGRAM) CaT stay runtime
static int rough_profile(const LgEngine *h, bool inj) {
    const LgTaskCfg &t = h->task; const LgBuffers &b = h->bufs;
    if (t.gait_mode != 0 || t.sit_percent != 0.f || t.behavior_resample_steps != 0 || t.noise_vec[9 + 6 * h->model.n_legs] != 0.f || b.task_state || !hf_bound(h))
        return LG_PROF_NONE;
    const int K = __builtin_popcount(h->model.state_link_mask), P = h->opts.n_height_points, A = h->model.n_bodies - 1;
    const bool common = t.double_shift == 0 && t.cat_enable == 0 && t.obs_frame == 9 + 3 * A && window_stacks(h) && uniforms_ok(h, inj) &&
                        !b.joint_armature && !t.dr_joint_on && flat_noise_ok(h) &&
                        h->model.n_legs == 4 && h->model.n_bodies == 13 && P > 0 && P <= 7 * 16 && h->opts.feet_terrain_info && b.priv_obs_buf &&
                        b.rand_push_vels && t.air_time_cmd_dims != 3 && t.num_priv_obs > 0 &&
                        (!t.terrain_curriculum || (b.terrain_levels && b.terrain_types && b.terrain_origins && b.env_origins)) &&
                        rewards_ok(h, LG_PROF_GO2_EE);   // the same exclusions as GO2_PROGRAM
    if (!common) return LG_PROF_NONE;
    if (t.obs_layout == LG_OBS_GO2_EE)
        return (t.priv_frame == 9 + 3 * A + 7 + 2 * A + K + P && t.num_labels == 3 + K + h->model.n_legs && b.labels_buf) ? LG_PROF_GO2_EE : LG_PROF_NONE;
    if (t.obs_layout == LG_OBS_PROGRAM) {
        if (t.num_labels > 0 && !b.labels_buf) return LG_PROF_NONE;
        for (const LgObsProgram *pr : {&t.priv_prog, &t.labels_prog})
            for (int i = 0; i < pr->n_segs; i++)
                if (pr->kind[i] == LG_SEG_DR_JOINT || pr->kind[i] <= LG_SEG_END || pr->kind[i] > LG_SEG_KD) return LG_PROF_NONE;
        return LG_PROF_GO2_PROGRAM;
    }
    return LG_PROF_NONE;
}
// The profile whose hard-wired switches the task really has, LG_PROF_NONE for none.
static int task_profile(const LgEngine *h, bool inj) {
    if (h->model.n_legs == 2) return biped_profile(h, inj) ? LG_PROF_TRON1_PF_EE : LG_PROF_NONE;
    if (flat_profile(h, inj)) return LG_PROF_GO2_FLAT;
    if (wtw_profile(h, inj)) return LG_PROF_GO2_WTW;
    return rough_profile(h, inj);
}

// Developer switches: 1 / 0 when the environment variable is set to a non-zero number / 0, -1 when unset.  Read on every lg_step (the
// tests flip them between steps), in one pass over the environment: as cheap as one getenv.
enum { SW_MDP_REPLICAS, SW_REWARD_SET_CONST, SW_BIPED_FUSE, SW_BIPED_TAIL, SW_COUNT };
static void read_switches(int sw[SW_COUNT]) {
    static const char *const name[SW_COUNT] = {"LG_MDP_REPLICAS=", "LG_REWARD_SET_CONST=", "LG_BIPED_FUSE=", "LG_BIPED_TAIL="};
    for (int i = 0; i < SW_COUNT; i++) sw[i] = -1;
    for (char **e = environ; *e; e++) {
        if (strncmp(*e, "LG_", 3)) continue;
        for (int i = 0; i < SW_COUNT; i++)
            if (sw[i] < 0 && !strncmp(*e, name[i], strlen(name[i]))) sw[i] = atoi(*e + strlen(name[i])) != 0;   // the first, as getenv
    }
}

// ---- launch selection: lg_step validates, plan() picks at most two launches without side effects, execute() runs them ----------------
using LgLauncher = void (*)(dim3, hipStream_t, hipEvent_t, hipEvent_t, const KParams &);
struct LgKernel { LgLauncher fn; const char *name; };   // a launcher of lg_shared.h and the name lg_last_kernel reports for it
#define LG_KERNEL(kern) LgKernel{kern, #kern}
template <int LEGS, int PROF> static void launch_inj(dim3 grid, hipStream_t st, hipEvent_t, hipEvent_t, const KParams &p) { lg_launch_quad_inj<LEGS, PROF>(grid, st, p); }

// Every kernel lg_step launches, named once, as the launcher expression lg_step has always reported (LEGS / JPL / PR tokens included:
// bench.py's roofline.kernel and the GPU tests match on these strings, so profiles are literals: pinned to their names here).  A row is
// instantiated only where plan() uses it.
static_assert(LG_PROF_NONE == 0); static_assert(LG_PROF_GO2_FLAT == 1); static_assert(LG_PROF_GO2_WTW == 2); static_assert(LG_PROF_GO2_EE == 3);
static_assert(LG_PROF_GO2_PROGRAM == 4); static_assert(LG_PROF_NONE_HF == 5); static_assert(LG_PROF_TRON1_PF_EE == 6);
template <int LEGS, int JPL> struct Kernels {
    static constexpr unsigned PR = LG_PHASE_POST | LG_PHASE_RESET;
    // leg per lane (lg_kernel.h), one launch per phase set; POST | RESET also replicated (env_step_kernel<..., REPL>).  NONE; all_flat GO2_FLAT
    static constexpr LgKernel all = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_ALL, 0, JPL, false>)), all_flat = LG_KERNEL((lg_launch_env<4, LG_PHASE_ALL, 1, 3, false>)),
        sim = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_SIM, 0, JPL, false>)), pre_sim = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_PRE | LG_PHASE_SIM, 0, JPL, false>)),
        pre_sim_post = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_PRE | LG_PHASE_SIM | LG_PHASE_POST, 0, JPL, false>)),
        pre_post_reset = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_PRE | PR, 0, JPL, false>)), pre_post = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_PRE | LG_PHASE_POST, 0, JPL, false>)),
        post_reset = LG_KERNEL((lg_launch_env<LEGS, PR, 0, JPL, false>)), post_reset_repl = LG_KERNEL((lg_launch_env<LEGS, PR, 0, JPL, true>)),
        post = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_POST, 0, JPL, false>)), reset = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_RESET, 0, JPL, false>));
    // component per lane (lg_quad.h), three joints per leg.  Physics only by [PRE][heightfield bound]: NONE / NONE_HF (lg_quad.h HFC: no
    // branch in front of the terrain loads)
    static constexpr LgKernel phys[2][2] = {{LG_KERNEL((lg_launch_quad<LEGS, false, 0u, 0, 3>)), LG_KERNEL((lg_launch_quad<LEGS, false, 0u, 5, 3>))},
                                            {LG_KERNEL((lg_launch_quad<LEGS, true, 0u, 0, 3>)), LG_KERNEL((lg_launch_quad<LEGS, true, 0u, 5, 3>))}};
    // quadruped whole step: the leg-per-lane MDP body in the tail (NONE), the tails of GO2_FLAT .. GO2_PROGRAM [profile - 1] and the same with
    // the default reward set as a constant (lg_quad.h RS); biped whole step: the leg-per-lane MDP body in the tail (NONE, NONE_HF), TRON1_PF_EE's
    static constexpr LgKernel quad_pre_sim_post = LG_KERNEL((lg_launch_quad<4, true, LG_PHASE_POST, 0, 3>)), quad_all = LG_KERNEL((lg_launch_quad<4, true, PR, 0, 3>)),
        biped_all = LG_KERNEL((lg_launch_quad<2, true, PR, 0, 3>)), biped_all_hf = LG_KERNEL((lg_launch_quad<2, true, PR, 5, 3>)),
        biped_all_ee = LG_KERNEL((lg_launch_quad<2, true, PR, 6, 3>));
    static constexpr LgKernel quad_prof[4] = {LG_KERNEL((lg_launch_quad<4, true, PR, 1, 3>)), LG_KERNEL((lg_launch_quad<4, true, PR, 2, 3>)),
                                              LG_KERNEL((lg_launch_quad<4, true, PR, 3, 3>)), LG_KERNEL((lg_launch_quad<4, true, PR, 4, 3>))};
    static constexpr LgKernel quad_prof_rs[4] = {LG_KERNEL((lg_launch_quad_rs<4, 1, false>)), LG_KERNEL((lg_launch_quad_rs<4, 2, false>)),
                                                 LG_KERNEL((lg_launch_quad_rs<4, 3, false>)), LG_KERNEL((lg_launch_quad_rs<4, 4, false>))};
    // golden replays: PRE | POST | RESET through the tails of GO2_FLAT .. GO2_PROGRAM [profile - 1] / TRON1_PF_EE on injected inputs (lg_quad.h INJ)
    static constexpr LgKernel inj[4] = {{launch_inj<4, 1>, "(lg_launch_quad_inj<4, 1>)"}, {launch_inj<4, 2>, "(lg_launch_quad_inj<4, 2>)"},
                                        {launch_inj<4, 3>, "(lg_launch_quad_inj<4, 3>)"}, {launch_inj<4, 4>, "(lg_launch_quad_inj<4, 4>)"}};
    static constexpr LgKernel inj_rs[4] = {{lg_launch_quad_rs<4, 1, true>, "(lg_launch_quad_inj<4, 1>, reward set constant)"}, {lg_launch_quad_rs<4, 2, true>, "(lg_launch_quad_inj<4, 2>, reward set constant)"},
                                           {lg_launch_quad_rs<4, 3, true>, "(lg_launch_quad_inj<4, 3>, reward set constant)"}, {lg_launch_quad_rs<4, 4, true>, "(lg_launch_quad_inj<4, 4>, reward set constant)"}};
    static constexpr LgKernel inj_biped = {launch_inj<2, 6>, "(lg_launch_quad_inj<2, 6>)"};
    // four joints per leg (TRON1 sole foot; these exist for the biped alone, hence plan()'s `if constexpr`): physics by [PRE], then MDP; NONE
    static constexpr LgKernel sole_phys[2] = {LG_KERNEL((lg_launch_quad<LEGS, false, 0u, 0, 4>)), LG_KERNEL((lg_launch_quad<LEGS, true, 0u, 0, 4>))};
    static constexpr LgKernel sole_post_reset = LG_KERNEL((lg_launch_env<LEGS, PR, 0, 4, false>)), sole_post_reset_repl = LG_KERNEL((lg_launch_env<LEGS, PR, 0, 4, true>)),
        sole_post = LG_KERNEL((lg_launch_env<LEGS, LG_PHASE_POST, 0, 4, false>));
};

struct LgPlan { struct { LgKernel k; dim3 grid; } l[2]; int n = 0; bool sim = false; };   // launches in order; sim: a sampled (SIM) step

// The launches of one lg_step for a robot shape, on phases lg_step has validated.  No side effects.
template <int LEGS, int JPL> static LgPlan plan(const LgEngine *h, uint32_t ph, const int sw[SW_COUNT]) {
    using K = Kernels<LEGS, JPL>;
    constexpr unsigned PR = K::PR;
    LgPlan pl; pl.sim = (ph & LG_PHASE_SIM) != 0;
    const auto add = [&pl](const LgKernel &k, dim3 grid) { pl.l[pl.n].k = k; pl.l[pl.n].grid = grid; pl.n++; };
    const int threads = h->bufs.n_envs * LEGS;
    const dim3 grid((threads + BLOCK - 1) / BLOCK), qgrid((threads * 4 + BLOCK - 1) / BLOCK), rgrid((threads + 15) / 16);
    const bool pre = (ph & LG_PHASE_PRE) != 0, hfb = hf_bound(h);
    const uint32_t rest = ph & PR;
    // MDP-only launches of small biped batches run replicated (env_step_kernel<..., REPL>) while four times the waves still fit one per
    // SIMD.  Measured at 4096 envs, us per step, plain / replicated: tron1_pf_ee 55.8 / 53.7, tron1_sf 52.3 / 50.7, tron1_pf 43.4 / 43.4;
    // go2_cat (16 k leg-lanes already) 59.4 / 59.6: quadrupeds stay plain.  LG_MDP_REPLICAS=0/1 forces either.
    const bool repl = sw[SW_MDP_REPLICAS] >= 0 ? sw[SW_MDP_REPLICAS] != 0 : (LEGS == 2 && (long long)threads * 4 <= 1024LL * BLOCK);
    const auto mdp = [&](uint32_t m) {   // POST | RESET or POST leg per lane, behind a physics launch or on its own
        if (m == PR) add(repl ? K::post_reset_repl : K::post_reset, repl ? rgrid : grid); else add(K::post, grid); };
    // rs(P): the task's reward set is profile P's default one and the solver options are the configs' defaults -> the instantiation with
    // them as constants (lg_quad.h RS; LG_REWARD_SET_CONST=0: off).  The same instantiation takes the configs' branch switches, the bound /
    // unbound optional buffers as given (lg_shared.h lg_rs_constants_hold): anything else runs the general form
    const auto rs = [&](int prof) {
        return (unsigned)h->hot.reward_mask == lg_default_reward_mask(prof) && h->hot.o_contact_iters == LG_DEFAULT_CONTACT_ITERS &&
               h->hot.o_contact_w_every == LG_DEFAULT_CONTACT_W_EVERY && lg_rs_constants_hold(prof, h->task, h->bufs) &&
               sw[SW_REWARD_SET_CONST] != 0; };
    // physics layout (lg_quad.h): one vector component per lane while the batch cannot fill the SIMDs with one leg per
    // lane; the MDP phases then follow in a second launch on the same stream
    // auto: component-per-lane while that needs at most two waves per SIMD (1024 SIMDs).  Measured go2, us per step,
    // component vs leg layout: 4096 envs 34.7 / 56.6, 8192: 50.9 / 55.2, 12288: 69.2 / 55.5, 16384: 92 / 60
    // the component-per-lane kernel is specialised for identity joint frames and hip-x / thigh-y / knee-y axes (lg_quad.h)
    const int layout = h->opts.sim_layout ? h->opts.sim_layout : ((h->quad_ok && (long long)threads * 4 <= 2048LL * BLOCK) ? 2 : 1);
    if (layout == 2 && pl.sim) {   // ALL, SIM, PRE | SIM, PRE | SIM | POST
        if constexpr (JPL == 4) {   // four-joint legs: physics in component layout, then the MDP phases
            add(K::sole_phys[pre], qgrid);
            if (rest == PR) add(repl ? K::sole_post_reset_repl : K::sole_post_reset, repl ? rgrid : grid);
            else if (rest == LG_PHASE_POST) add(K::sole_post, grid);
        } else if (LEGS == 4 && pre && rest == LG_PHASE_POST) {
            // the quadruped runs the MDP phases in the tail of the same launch (measured 39.5 vs 40.6 us for go2, 69.6 vs 72.5 for go2_ee)
            add(K::quad_pre_sim_post, qgrid);
        } else if (LEGS == 4 && pre && rest == PR) {
            const int prof = task_profile(h, false);
            add(prof == LG_PROF_NONE ? K::quad_all : rs(prof) ? K::quad_prof_rs[prof - 1] : K::quad_prof[prof - 1], qgrid);
        } else if (LEGS == 2 && pre && rest == PR && sw[SW_BIPED_FUSE] != 0) {
            // biped (TRON1 point foot): the whole step in one launch too -- the leg-per-lane MDP body in the tail, four replicas of the
            // wave's 16 leg-lanes (8 envs) -- unless the job-wide CaT flag has to pass between the phases (lg_step refuses that fused).
            // LG_BIPED_FUSE=0: two launches.  TRON1_PF_EE: workgroups of two waves per group of 8 envs (lg_quad.h DUO: both run the physics,
            // then split the tail); LG_BIPED_TAIL=0: the leg-per-lane MDP body in the tail even where the component-layout tail applies
            if (hfb && task_profile(h, false) == LG_PROF_TRON1_PF_EE && sw[SW_BIPED_TAIL] != 0) add(K::biped_all_ee, qgrid);
            else add(hfb ? K::biped_all_hf : K::biped_all, qgrid);
        } else {   // physics, then the MDP phases as a second launch (84.7 vs 90.6 us for tron1_pf_ee: 8 envs per wave there)
            add(K::phys[pre][hfb], qgrid);
            if (rest) mdp(rest);
        }
        return pl;
    }
    if (JPL == 3 && ph == (LG_PHASE_PRE | PR) && h->opts.sim_layout == 2 && h->bufs.rand_in) {
        // golden replays through the benchmarked tails (tests/test_gpu_mdp.py, tail = "fused-profile"): the component-layout tail of the task's
        // profile on injected read-backs and uniforms (lg_quad.h INJ); a task outside every profile takes the leg-per-lane launch below
        const int prof = task_profile(h, true);
        if (LEGS == 4 && prof != LG_PROF_NONE) { add(rs(prof) ? K::inj_rs[prof - 1] : K::inj[prof - 1], qgrid); return pl; }
        if (LEGS == 2 && prof == LG_PROF_TRON1_PF_EE) { add(K::inj_biped, qgrid); return pl; }
    }
    switch (ph) {
    case LG_PHASE_ALL:
        if (LEGS == 4 && JPL == 3 && task_profile(h, false) == LG_PROF_GO2_FLAT) add(K::all_flat, grid);   // large go2 batches: same FLAT constants
        else add(K::all, grid);
        break;
    case LG_PHASE_SIM: add(K::sim, grid); break;
    case LG_PHASE_PRE | LG_PHASE_SIM: add(K::pre_sim, grid); break;
    case LG_PHASE_PRE | LG_PHASE_SIM | LG_PHASE_POST: add(K::pre_sim_post, grid); break;
    case LG_PHASE_PRE | PR: add(K::pre_post_reset, grid); break;
    case LG_PHASE_PRE | LG_PHASE_POST: add(K::pre_post, grid); break;
    case LG_PHASE_RESET: add(K::reset, grid); break;
    case PR: case LG_PHASE_POST: mdp(ph); break;
    }
    return pl;
}

// Runs a plan: the observation bookkeeping of a RESET step, then the launches.  A sampled step (lg_profile) has the begin timestamp on its
// first launch and the end timestamp on its last (a two-launch sample includes the gap); hipExtLaunchKernelGGL attaches the events to the
// dispatch packet itself, so the reading is the kernel's duration, comparable with rocprofv3's.
static int execute(LgEngine *h, const LgPlan &pl, uint32_t ph, const float *actions, int64_t counter, hipStream_t st) {
    KParams p;
    p.M = h->d_model; p.O = h->d_opts; p.T = h->d_task; p.H = h->d_hot; p.LT = h->d_lane; p.hf = h->hf; p.B = h->bufs; p.actions = actions; p.counter = counter;
    p.jrot_identity = h->jrot_identity;
    const LgHot &hot = h->hot;   // refreshed by upload_hot
    p.k.m_n_links = hot.m_n_links;
    for (int i = 0; i < 4; i++) { p.k.m_foot_link[i] = hot.m_foot_link[i]; p.k.joint_axis[i] = h->joint_axis[i]; }
    p.k.foot_pack = lg_foot_pack(hot.m_foot_link, h->model.n_legs);
    p.k.obs_layout = hot.obs_layout; p.k.o_n_height_points = hot.o_n_height_points; p.k.cat_enable = h->task.cat_enable;
    p.k.reward_mask = (unsigned)hot.reward_mask; p.k.clip_actions = hot.clip_actions;
    p.obs_win = 0; p.obs_set = h->obs_set;
    if (ph & LG_PHASE_RESET) {
        const LgTaskCfg &t = h->task;
        const int sets = t.obs_sets > 1 ? t.obs_sets : 1;
        if (sets > 1) p.obs_set = h->obs_set = (h->obs_set + 1) % sets;      // this launch writes a copy the caller is NOT holding
        if (t.obs_slack > 0) {
            // the observation written by this launch lives one frame further; out of slack -> compact first (source and
            // destination ranges are disjoint because lg_create enforces slack >= stack, and with two sets the window the
            // caller still holds, [slack, slack + stack), is clear of everything written here because slack >= stack + 1).
            // Both sets are compacted together: they are one allocation of sets * n rows
            if (h->obs_win >= t.obs_slack) {
                const int n = h->bufs.n_envs * sets;
                if (t.obs_stack > 1)
                    hipLaunchKernelGGL(obs_compact_kernel, dim3(1024), dim3(256), 0, st, h->bufs.obs_buf, n, (t.obs_stack + t.obs_slack) * t.obs_frame, t.obs_frame, t.obs_stack, h->obs_win);
                if (t.num_priv_obs > 0 && t.priv_stack > 1)
                    hipLaunchKernelGGL(obs_compact_kernel, dim3(1024), dim3(256), 0, st, h->bufs.priv_obs_buf, n, (t.priv_stack + t.obs_slack) * t.priv_frame, t.priv_frame, t.priv_stack, h->obs_win);
                h->obs_win = 0;
            }
            p.obs_win = ++h->obs_win;
        }
    }
    const int pi = pl.sim ? prof_begin(h, st) : -1;
    h->last_kernel.clear();
    for (int i = 0; i < pl.n; i++) {
        if (i) h->last_kernel += " + ";
        h->last_kernel += pl.l[i].k.name;
        pl.l[i].k.fn(pl.l[i].grid, st, pi >= 0 && i == 0 ? h->prof_ev[2 * pi] : nullptr, pi >= 0 && i == pl.n - 1 ? h->prof_ev[2 * pi + 1] : nullptr, p);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int check_mdp_bufs(const LgEngine *h, uint32_t ph) {
    const LgBuffers &b = h->bufs;
    if (ph & (LG_PHASE_PRE | LG_PHASE_POST | LG_PHASE_RESET)) {
#define REQ(f) if (!b.f) return fail("lg_step: MDP phases need buffer " #f)
        REQ(actions); REQ(last_actions); REQ(llast_actions); REQ(commands); REQ(feet_air_time); REQ(last_contacts);
        REQ(episode_length_buf); REQ(fail_buf); REQ(reset_buf); REQ(time_out_buf); REQ(rew_buf); REQ(obs_buf);
        REQ(episode_sums); REQ(episode_done_sums); REQ(episode_done_step); REQ(command_ranges); REQ(rand_push_vels);
        REQ(friction_values); REQ(added_base_mass); REQ(base_com_bias); REQ(kp_scale); REQ(kd_scale);
#undef REQ
        if (h->task.cat_enable && (!b.cstr_prob || !b.cstr_sums || !b.cstr_done_sums)) return fail("lg_step: cat_enable needs buffers cstr_prob, cstr_sums, cstr_done_sums");
        if (h->task.obs_sets > 1 && h->task.obs_slack > 0 && !b.obs_dirty) return fail("lg_step: two observation sets with history stacks need buffer obs_dirty");
    }
    return 0;
}

extern "C" int lg_step(LgHandle h, uint32_t phases, const float *actions, int64_t counter, void *stream) {
    // everything is checked before the first side effect: a refused call leaves the engine as it was
    if (!h) return fail("lg_step: null handle");
    if (!h->bound) return fail("lg_step: lg_bind has not been called");
    if ((phases & (LG_PHASE_PRE | LG_PHASE_SIM)) && !actions) return fail("lg_step: actions pointer is NULL");
    if (h->opts.terrain_rows > 0 && !h->hf) return fail("lg_step: heightfield options set but lg_set_terrain was not called");
    if (check_mdp_bufs(h, phases)) return 1;
    if (h->task.cat_enable && (phases & LG_PHASE_SIM) && (phases & LG_PHASE_POST))
        return fail("lg_step: with cat_enable the physics and the MDP phases must be separate launches (job-wide constraint flag, LG_CR_ANY_FAST)");
    if (h->opts.sim_layout == 2 && !h->quad_ok) return fail("lg_step: sim_layout 2 needs identity joint frames and x / y / y (/ y) joint axes");
    constexpr uint32_t PRE = LG_PHASE_PRE, SIM = LG_PHASE_SIM, POST = LG_PHASE_POST, RESET = LG_PHASE_RESET;
    switch (phases) {
    case LG_PHASE_ALL: case SIM: case PRE | SIM: case PRE | SIM | POST: case PRE | POST | RESET: case PRE | POST: case POST | RESET: case POST: case RESET: break;
    default: return fail("lg_step: unsupported phase combination (ALL, SIM, PRE|SIM, PRE|POST|RESET, PRE|SIM|POST, PRE|POST, POST|RESET, POST, RESET)");
    }
    int sw[SW_COUNT]; read_switches(sw);
    const LgPlan pl = h->model.n_bodies == 1 + 4 * h->model.n_legs ? plan<2, 4>(h, phases, sw)    // validate_model: two legs
                      : h->model.n_legs == 4                        ? plan<4, 3>(h, phases, sw) : plan<2, 3>(h, phases, sw);
    hipStream_t st = (hipStream_t)stream;
    // Bounded run-ahead.  A host that enqueues thousands of launches ahead of the device (a bench loop without a
    // policy in between) drives the runtime into a slow submission path: measured 90 us per step instead of 42 with
    // ~4000 launches in flight.  Every 32nd call records an event; before a slot is reused (128 calls later) the host
    // waits for it, which is free unless it really is that far ahead.
    if ((h->ra_calls++ & 31) == 0) {
        const int slot = (int)((h->ra_calls >> 5) & 3);
        if (h->ra_ev[slot]) HIPCHK(hipEventSynchronize(h->ra_ev[slot]));
        else HIPCHK(hipEventCreateWithFlags(&h->ra_ev[slot], hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ra_ev[slot], st));
    }
    return execute(h, pl, phases, actions, counter, st);
}

__global__ __launch_bounds__(256) void stream_copy_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, long long n4) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    // one 16-byte load and store per lane and iteration: measured 5.0-5.1 TB/s (read + write) on an MI355X; four loads in flight per lane
    // before the stores measured 4.5, torch's elementwise copy_ 4.8
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
}

extern "C" int lg_stream_copy(const void *src, void *dst, int64_t bytes, int32_t iters, void *stream, float *gbs) {
    if (!src || !dst || !gbs || bytes < 16 || (bytes & 15) || iters < 1) return fail("lg_stream_copy: bad argument");
    if (((uintptr_t)src | (uintptr_t)dst) & 15) return fail("lg_stream_copy: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long n4 = bytes / 16;
    // 256 CUs x 8 workgroups of 256 threads: every SIMD holds two waves, each streaming 16 B per lane per iteration
    const dim3 grid((unsigned)std::min<long long>((n4 + 255) / 256, 256 * 8)), block(256);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    hipLaunchKernelGGL(stream_copy_kernel, grid, block, 0, st, (const float4 *)src, (float4 *)dst, n4);
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; i++) hipLaunchKernelGGL(stream_copy_kernel, grid, block, 0, st, (const float4 *)src, (float4 *)dst, n4);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    *gbs = ms > 0.f ? (float)(2.0 * (double)bytes * iters / (ms * 1e-3) / 1e9) : 0.f;
    return 0;
}

// ---- heightfield generation (include/lgsim.h lg_terrain_generate) ---------------------------------------------------------------------
// One thread per pixel of a tile.  Everything float is float64 with the reference's (numpy / FITPACK) operation order and NO contraction
// into fused multiply-adds (__dmul_rn / __dadd_rn / __ddiv_rn): the grid has to come out sample for sample.
__global__ __launch_bounds__(256) void terrain_tile_kernel(const LgTerrainTile *__restrict__ tiles, const double *__restrict__ aux,
                                                           const int32_t *__restrict__ iaux, int16_t *__restrict__ hf, int cols, int W, int border) {
    const LgTerrainTile T = tiles[blockIdx.y];
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * W) return;
    const int x = pix / W, y = pix % W;
    int v = 0;
    if (T.kind == LG_TILE_SLOPE) {
        // (peak * ramp_x * ramp_y).astype(int16) inside the edge, then clip to [min(ref, 0), max(ref, 0)] (terrain_utils.py:160-181)
        const int peak = T.ip[0], edge = T.ip[1], half = T.ip[2], c = W / 2;
        auto val = [&](int px, int py) {
            if (px < edge || px >= W - edge || py < edge || py >= W - edge) return 0;
            const double rx = __ddiv_rn((double)(c - abs(c - px)), (double)c), ry = __ddiv_rn((double)(c - abs(c - py)), (double)c);
            return (int)(int16_t)__dmul_rn(__dmul_rn((double)peak, rx), ry);
        };
        const int ref = val(W / 2 - half, W / 2 - half);
        v = min(max(val(x, y), min(ref, 0)), max(ref, 0));
    } else if (T.kind == LG_TILE_STAIRS) {
        // nested squares [r w, W - r w)^2 at height r h while the square is wider than the platform (terrain_utils.py:361-371)
        const int w = T.ip[0], h = T.ip[1], plat = T.ip[2];
        int rings = 0;
        for (int lo = 0, hi = W; hi - lo > plat; lo += w, hi -= w) rings++;
        const int d = min(min(x, W - 1 - x), min(y, W - 1 - y));
        v = rings > 0 ? min(d / w, rings - 1) * h : 0;
    } else if (T.kind == LG_TILE_OBSTACLES || T.kind == LG_TILE_STONES) {
        // background, rectangles in draw order (the last one covering the pixel wins), then the zero platform
        const bool stones = T.kind == LG_TILE_STONES;
        const int n = T.ip[0];
        const int a = stones ? T.ip[1] : (W - T.ip[1]) / 2, b = stones ? T.ip[2] : (W + T.ip[1]) / 2;
        const int32_t *r = iaux + T.aux_off;
        v = stones ? T.ip[3] : 0;
        for (int k = n - 1; k >= 0; k--)
            if (x >= r[5 * k] && x < r[5 * k] + r[5 * k + 2] && y >= r[5 * k + 1] && y < r[5 * k + 1] + r[5 * k + 3]) { v = r[5 * k + 4]; break; }
        if (x >= a && x < b && y >= a && y < b) v = 0;
    } else if (T.kind == LG_TILE_GAP) {
        // the -1000 square, then the zero platform inside it (terrain_utils.py:489-490)
        if (x >= T.ip[0] && x < T.ip[1] && y >= T.ip[0] && y < T.ip[1]) v = -1000;
        if (x >= T.ip[2] && x < T.ip[3] && y >= T.ip[2] && y < T.ip[3]) v = 0;
    } else if (T.kind == LG_TILE_PIT) {
        if (x >= T.ip[0] && x < T.ip[1] && y >= T.ip[0] && y < T.ip[1]) v = T.ip[2];
    } else if (T.kind == LG_TILE_WAVE) {
        // (amplitude cos(yy / div) + amplitude sin(xx / div)).astype(int16) inside the edge (terrain_utils.py:300-301); both factors
        // come from the host (numpy's cos / sin), so the only arithmetic here is numpy's one float64 add and the truncation
        const int edge = T.ip[0], n = T.ip[1], i = x - edge, j = y - edge;
        if (i >= 0 && i < n && j >= 0 && j < n) {
            const double *cy = aux + T.aux_off, *sx = cy + n;
            v = (int)(int16_t)__dadd_rn(cy[j], sx[i]);
        }
    } else if (T.kind == LG_TILE_UNIFORM) {
        // np.rint(RectBivariateSpline(kx = ky = 1)(xs, ys)) inside the edge: FITPACK fpbisp / fpbspl for degree 1
        const int edge = T.ip[0], nx = T.ip[1], ny = T.ip[2], mx = T.ip[3], my = T.ip[4];
        const int i = x - edge, j = y - edge;
        if (i >= 0 && i < mx && j >= 0 && j < my) {
            const double *tx = aux + T.aux_off, *ty = tx + nx, *cf = ty + ny, *xs = cf + (nx - 2) * (ny - 2), *ys = xs + mx;
            auto basis = [](const double *t, int n, double arg, int &l, double &h1, double &h2) {
                const int k1 = 2, nk1 = n - k1;                       // fpbisp: clamp, then the knot interval (1-based l: t(l) <= arg < t(l+1))
                const double tb = t[k1 - 1], te = t[nk1];
                if (arg < tb) arg = tb;
                if (arg > te) arg = te;
                l = k1;
                while (!(arg < t[l]) && l != nk1) l++;                // t(l1) with l1 = l + 1 is t[l] in 0-based terms
                const double f = __ddiv_rn(1.0, __dadd_rn(t[l], -t[l - 1]));      // fpbspl, k = 1
                h1 = __dmul_rn(f, __dadd_rn(t[l], -arg));
                h2 = __dmul_rn(f, __dadd_rn(arg, -t[l - 1]));
            };
            int lx, ly;
            double wx1, wx2, wy1, wy2;
            basis(tx, nx, xs[i], lx, wx1, wx2);
            basis(ty, ny, ys[j], ly, wy1, wy2);
            const int nky1 = ny - 2;
            int l1 = (lx - 2) * nky1 + (ly - 2);
            double sp = 0.0;
            sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(cf[l1], wx1), wy1));
            sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(cf[l1 + 1], wx1), wy2));
            l1 += nky1;
            sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(cf[l1], wx2), wy1));
            sp = __dadd_rn(sp, __dmul_rn(__dmul_rn(cf[l1 + 1], wx2), wy2));
            v = (int)(int16_t)rint(sp);                               // np.rint: half to even
        }
    }
    hf[(size_t)(border + T.row * W + x) * cols + border + T.col * W + y] = (int16_t)v;
}

__global__ __launch_bounds__(256) void terrain_origin_kernel(const LgTerrainTile *__restrict__ tiles, const int16_t *__restrict__ hf, int cols, int W,
                                                             int border, int o1, int o2, double vscale, double *__restrict__ origin_z) {
    __shared__ int smax[256];
    const LgTerrainTile T = tiles[blockIdx.x];
    const int n = o2 - o1;
    int m = -32768;
    for (int k = threadIdx.x; k < n * n; k += blockDim.x)
        m = max(m, (int)hf[(size_t)(border + T.row * W + o1 + k / n) * cols + border + T.col * W + o1 + k % n]);
    smax[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + s]); __syncthreads(); }
    if (threadIdx.x == 0) origin_z[blockIdx.x] = __dmul_rn((double)smax[0], vscale);
}

extern "C" int lg_terrain_max_kind(void) { return LG_TILE_MAX_KIND; }

extern "C" int lg_terrain_generate(const LgTerrainTile *tiles, int32_t n_tiles, const double *aux, const int32_t *iaux, int16_t *hf, int32_t rows,
                                   int32_t cols, int32_t tile_px, int32_t border_px, int32_t o1, int32_t o2, double vertical_scale, double *origin_z,
                                   void *stream) {
    if (!tiles || !hf || !origin_z || n_tiles < 1 || tile_px < 1 || rows < 2 || cols < 2 || o1 < 0 || o2 <= o1 || o2 > tile_px)
        return fail("lg_terrain_generate: bad argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(hf, 0, (size_t)rows * cols * sizeof(int16_t), st));
    hipLaunchKernelGGL(terrain_tile_kernel, dim3((tile_px * tile_px + 255) / 256, n_tiles), dim3(256), 0, st, tiles, aux, iaux, hf, cols, tile_px, border_px);
    hipLaunchKernelGGL(terrain_origin_kernel, dim3(n_tiles), dim3(256), 0, st, tiles, hf, cols, tile_px, border_px, o1, o2, vertical_scale, origin_z);
    HIPCHK(hipGetLastError());
    return 0;
}

__global__ void philox_kat_kernel(U4 c, unsigned k0, unsigned k1, unsigned *out) {
    const U4 r = philox4x32_10(c, k0, k1);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

extern "C" int lg_philox(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    if (!counter || !key || !out) return fail("lg_philox: null argument");
    unsigned *d = nullptr;
    HIPCHK(hipMalloc(&d, 16));
    const U4 c = {counter[0], counter[1], counter[2], counter[3]};
    hipLaunchKernelGGL(philox_kat_kernel, dim3(1), dim3(1), 0, 0, c, key[0], key[1], d);
    hipError_t e = hipMemcpy(out, d, 16, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(std::string("lg_philox: ") + hipGetErrorString(e));
    return 0;
}

// DPP operand known-answer test (tests/test_gpu_dpp_operands.py): the behaviour of THIS chip that hcr_genesis_lr_cl_amd/dpp_hazard_pass.py builds on.
// The rule "VALU writes a VGPR -> DPP read: two wait states" concerns the DPP-routed source (src0) only; a plain operand (src1) or the
// accumulator of a DPP multiply-add written in the slot before is forwarded like for any VALU instruction -- cases 0 and 1, no wait state, must
// be exact.  Case 2: a fresh DPP source behind `s_nop 1` -- exact.  Case 3: the same without the nop -- the negative control, reported, not
// required either way (it reads whatever the register held before: here a NaN).  This file is compiled with plain hipcc: the pass never sees it.
__global__ void dpp_kat_kernel(const float *in, float *out) {
    const int t = threadIdx.x;
    const float x = in[t], y = in[64 + t];
    float a, r0, r1, r2, r3;
    asm volatile(
        "s_nop 4\n\t"
        "v_mul_f32_e32 %0, %5, %6\n\t"
        "v_add_f32_dpp %1, %5, %0 quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t"
        "v_mul_f32_e32 %2, %5, %6\n\t"
        "v_fmac_f32_dpp %2, %5, %6 quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t"
        "v_mul_f32_e32 %3, %5, %6\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %3, %3, %5 quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_e32 %4, 0x7fc00000\n\t"
        "s_nop 4\n\t"
        "v_mul_f32_e32 %4, %5, %6\n\t"
        "v_add_f32_dpp %4, %4, %5 quad_perm:[1,2,0,3] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 4"
        : "=&v"(a), "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(x), "v"(y));
    out[t] = r0; out[64 + t] = r1; out[128 + t] = r2; out[192 + t] = r3; out[256 + t] = a;
}

extern "C" int lg_dpp_kat(const float *in_host, float *out_host) {
    if (!in_host || !out_host) return fail("lg_dpp_kat: null argument");
    float *d = nullptr;
    HIPCHK(hipMalloc(&d, (128 + 320) * sizeof(float)));
    HIPCHK(hipMemcpy(d, in_host, 128 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dpp_kat_kernel, dim3(1), dim3(64), 0, 0, d, d + 128);
    hipError_t e = hipMemcpy(out_host, d + 128, 320 * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(std::string("lg_dpp_kat: ") + hipGetErrorString(e));
    return 0;
}

// The table-driven DPP operand known-answer test (csrc/lg_dpp_kat.h; tests/test_gpu_dpp_operands.py): every (mnemonic, role, writer, distance,
// control) the built kernels forward, a grid of them under one control, and the fresh-DPP-source negative controls.  Each case is one asm block
// between `s_nop 4`s (tests/test_dpp_hazard_pass.py checks in the disassembly that it reaches the chip exactly as written: this file is compiled
// with plain hipcc, the pass never sees it).  Launched with one wave or many per SIMD: outputs go to addresses derived from the case and
// threadIdx / blockIdx only -- the first wave's two registers per case in full, every wave's lanes that differ from `expect` as counts.
#define LG_KAT_ONE(role, writer, dist, text) +1
constexpr int LG_DPP_KAT_N = 0 LG_DPP_KAT_CASES(LG_KAT_ONE);
#undef LG_KAT_ONE

__device__ __forceinline__ void kat_store(int k, float d, float r, int lane, bool first_wave, float *first, const unsigned *expect, unsigned *mismatch) {
    const int i = 2 * k * 64 + lane;
    if (first_wave) { first[i] = d; first[i + 64] = r; }
    if (expect) {
        if (__float_as_uint(d) != expect[i]) atomicAdd(mismatch + i, 1u);
        if (__float_as_uint(r) != expect[i + 64]) atomicAdd(mismatch + i + 64, 1u);
    }
}

__global__ void __launch_bounds__(1024) dpp_kat_table_kernel(const float *in, const unsigned *expect, float *first, unsigned *mismatch) {
    const int lane = threadIdx.x & 63;
    const bool first_wave = blockIdx.x == 0 && threadIdx.x < 64;
    const float x = in[lane], y = in[64 + lane], z = in[128 + lane], s = in[192 + lane], o = in[256 + lane];
    int k = 0;
#define LG_KAT_RUN(role, writer, dist, text) { \
        float d_, r_, t_; \
        asm volatile("s_nop 4\n\tv_mov_b32_e32 %[r], %[s]\n\tv_mov_b32_e32 %[d], %[o]\n\ts_nop 4\n\t" text "s_nop 4" \
                     : [d] "=&v"(d_), [r] "=&v"(r_), [t] "=&v"(t_) : [x] "v"(x), [y] "v"(y), [z] "v"(z), [s] "v"(s), [o] "v"(o)); \
        (void)t_; \
        kat_store(k++, d_, r_, lane, first_wave, first, expect, mismatch); }
    LG_DPP_KAT_CASES(LG_KAT_RUN)
#undef LG_KAT_RUN
}

extern "C" int lg_dpp_kat_cases(void) { return LG_DPP_KAT_N; }

extern "C" int lg_dpp_kat_run(const float *in_host, const uint32_t *expect_host, int32_t blocks, int32_t threads, float *first_host,
                              uint32_t *mismatch_host) {
    if (!in_host || !first_host || (expect_host && !mismatch_host) || blocks < 1 || blocks > 65536 || threads < 64 || threads > 1024 || threads % 64)
        return fail("lg_dpp_kat_run: bad argument");
    const size_t n_out = (size_t)2 * LG_DPP_KAT_N * 64;
    char *d = nullptr;
    HIPCHK(hipMalloc(&d, 5 * 64 * sizeof(float) + 3 * n_out * sizeof(float)));
    float *d_in = (float *)d, *d_first = d_in + 5 * 64;
    unsigned *d_expect = (unsigned *)(d_first + n_out), *d_mis = d_expect + n_out;
    hipError_t e = hipMemcpy(d_in, in_host, 5 * 64 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_first, 0, n_out * sizeof(float));
    if (e == hipSuccess && expect_host) e = hipMemcpy(d_expect, expect_host, n_out * sizeof(unsigned), hipMemcpyHostToDevice);
    if (e == hipSuccess && expect_host) e = hipMemset(d_mis, 0, n_out * sizeof(unsigned));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dpp_kat_table_kernel, dim3(blocks), dim3(threads), 0, 0, d_in, expect_host ? d_expect : nullptr, d_first, d_mis);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(first_host, d_first, n_out * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && expect_host) e = hipMemcpy(mismatch_host, d_mis, n_out * sizeof(unsigned), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(std::string("lg_dpp_kat_run: ") + hipGetErrorString(e));
    return 0;
}

extern "C" const char *lg_last_kernel(LgHandle h) { return h ? h->last_kernel.c_str() : ""; }

extern "C" int lg_obs_window(LgHandle h, int32_t *first_frame) {
    if (!h || !first_frame) return fail("lg_obs_window: null argument");
    *first_frame = h->task.obs_slack > 0 ? h->obs_win : 0;
    return 0;
}

extern "C" int lg_obs_set(LgHandle h, int32_t *set) {
    if (!h || !set) return fail("lg_obs_set: null argument");
    *set = h->task.obs_sets > 1 ? h->obs_set : 0;
    return 0;
}

extern "C" int lg_obs_set_select(LgHandle h, int32_t set) {
    if (!h) return fail("lg_obs_set_select: null handle");
    const int sets = h->task.obs_sets > 1 ? h->task.obs_sets : 1;
    if (set < 0 || set >= sets) return fail("lg_obs_set_select: set out of range");
    h->obs_set = set;
    return 0;
}

extern "C" int lg_obs_window_select(LgHandle h, int32_t first_frame) {
    if (!h) return fail("lg_obs_window_select: null handle");
    if (first_frame < 0 || first_frame > h->task.obs_slack) return fail("lg_obs_window_select: window out of range");
    h->obs_win = h->task.obs_slack > 0 ? first_frame : 0;
    return 0;
}

extern "C" int lg_profile(LgHandle h, int32_t stride) {
    if (!h || stride < 0) return fail("lg_profile: bad argument");
    h->prof_stride = stride; h->prof_seen = 0;
    return 0;
}

extern "C" int lg_profile_read(LgHandle h, float *mean_us, int32_t *samples) {
    if (!h || !mean_us || !samples) return fail("lg_profile_read: null argument");
    double sum = 0.0;
    for (int i = 0; i < h->prof_count; i++) {
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(h->prof_ev[2 * i + 1]));
        HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
        sum += ms;
    }
    *samples = h->prof_count;
    *mean_us = h->prof_count ? (float)(sum / h->prof_count * 1e3) : 0.f;
    h->prof_count = 0;
    return 0;
}

extern "C" int lg_time_steps(LgHandle h, const float *actions, int64_t first_counter, int32_t count, void *stream, float *ms) {
    if (!h || !ms || count < 1) return fail("lg_time_steps: bad argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipEventRecord(h->ev0, st));
    for (int i = 0; i < count; i++)
        if (lg_step(h, LG_PHASE_ALL, actions, first_counter + i, stream)) return 1;
    HIPCHK(hipEventRecord(h->ev1, st));
    HIPCHK(hipEventSynchronize(h->ev1));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, h->ev0, h->ev1));
    *ms = t / count;
    return 0;
}

