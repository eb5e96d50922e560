// lg_train_cts.hip -- the fused RL pass of the concurrent teacher-student family behind include/lgtraincts.h: ActorCriticCTS over a
// mini-batch of three independent row sets (teacher rows: privilege encoder -> [obs | z] -> actor; student rows: history encoder ->
// [obs | z] -> the same actor; critic rows: the critic) with its backward over the actor, the critic and the privilege encoder.  The
// encoder step of PPO_CTS is lg_train_ts.hip's encoder pass with a mask of ones and needs nothing here.
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_cts.py:193-267 (_compute_rl_loss's network calls) and the share of loss.backward()
// in PPO_CTS.update() (ppo_cts.py:156-160) that runs through the MLPs of ActorCriticCTS and that an optimizer ever reads.
//
// The layer routines are lg_train_tiles.h's, the chain, seed, combine, plan-chain and bind-chain routines lg_train_pass.h's, unchanged.
// What is this family's own:
//   two descriptors of the actor   `c[ACT]` addresses the actor's workspace regions from row 0 of a row space of Bt + Bs rows (the teacher's
//                     rows, and the whole chain for the weight gradients); `c[STA]` has the same weights with h_off / g_off advanced by Bt rows
//                     of each layer's width and out / gin at the student's mu / grad_mu, so that the shared routines run on a student tile
//                     with a local row0.
//   one-dimensional grids   block -> (role, local tile): the critic's tiles first, then the teacher's, then the student's.
//   per-chain row counts    a weight-gradient job runs over the rows of its own chain (Bt, Bt + Bs, Bc); grad_std has two slabs of slice
//                     partials, the teacher's grad_sigma over Bt rows and the student's over Bs, back to back, combined in that order.
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtraincts.h"

#define PRI LG_TRAIN_CTS_PRIVILEGE
#define ACT LG_TRAIN_CTS_ACTOR
#define CRI LG_TRAIN_CTS_CRITIC
#define HIS LG_TRAIN_CTS_HISTORY
#define TEA LG_TRAIN_CTS_TEACHER
#define STU LG_TRAIN_CTS_STUDENT
#define STA LG_TRAIN_CTS_CHAINS                 // CArgs::c's index of the student's descriptor of the actor

struct CArgs : PArgs {
    TChain c[LG_TRAIN_CTS_CHAINS + 1];          // c[STA]: the actor as the student rows address it
    const float *obs[LG_TRAIN_CTS_GROUPS];      // (Bt, O), (Bs, O): the first columns of the actor's input
    float *sig[LG_TRAIN_CTS_GROUPS];
    const float *gsig[LG_TRAIN_CTS_GROUPS];
    int obs_stride[LG_TRAIN_CTS_GROUPS], sig_stride[LG_TRAIN_CTS_GROUPS], gsig_stride[LG_TRAIN_CTS_GROUPS];
    int rows[LG_TRAIN_CTS_CHAINS];              // Bt, Bt + Bs, Bc, Bs: the rows of each chain
    int tiles[LG_TRAIN_CTS_ROLES];              // row tiles of the teacher, the student, the critic
    int enc_start[LG_TRAIN_CTS_GROUPS];
    int grp_S[LG_TRAIN_CTS_GROUPS], grp_rps[LG_TRAIN_CTS_GROUPS];       // the two std slabs' slices and rows per slice
    long long cat_off;
};
static_assert(sizeof(CArgs) <= 4096, "CArgs is passed by value: the kernel-argument segment is 4 KB");

// the workgroup's role (LG_TRAIN_CTS_TEACHER, _STUDENT or _ROLE_CRITIC) and its tile within the role: critic, teacher, student
__device__ __forceinline__ int role_of(const CArgs &a, int &tile) {
    const int b = blockIdx.x, tc = a.tiles[LG_TRAIN_CTS_ROLE_CRITIC];
    if (b < tc) { tile = b; return LG_TRAIN_CTS_ROLE_CRITIC; }
    if (b < tc + a.tiles[TEA]) { tile = b - tc; return TEA; }
    tile = b - tc - a.tiles[TEA];
    return STU;
}

template <int RB> __global__ __launch_bounds__(256) void train_cts_forward_kernel(CArgs a) {
    extern __shared__ __align__(16) float lds[];
    int tile;
    const int role = role_of(a, tile);
    const int R = a.R, row0 = tile * R;
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    if (role == LG_TRAIN_CTS_ROLE_CRITIC) {
        const TChain &c = a.c[CRI];
        const int rows = min(R, a.rows[CRI] - row0);
        const lds_f *v = chain_from_rows<RB>(a.ws, c, b0, b1, true, false, a.clip, R, rows, row0);
        copy_out(v, c.l[c.n_layers - 1].so, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
        return;
    }
    const bool stu = role == STU;
    const TChain &e = a.c[stu ? HIS : PRI], &c = a.c[stu ? STA : ACT];
    const int n = a.rows[stu ? HIS : PRI], es = a.enc_start[role];
    const int rows = min(R, n - row0);
    const int Z = e.l[e.n_layers - 1].M, O = c.l[0].K - Z;
    const lds_f *z = chain_from_rows<RB>(a.ws, e, es ? b1 : b0, es ? b0 : b1, !stu, false, a.clip, R, rows, row0);        // ends in b1: es is chosen so
    const int sa = c.l[0].sa, sz = e.l[e.n_layers - 1].so;
    stage_rows(a.obs[role], O, a.obs_stride[role], b0, sa, R, rows, row0);             // [obs | z] in b0, at the actor's stride
    for (int i = threadIdx.x; i < R * Z; i += kThreads) {
        const int row = i / Z, col = i - row * Z;
        b0[row * sa + O + col] = row < rows ? z[row * sz + col] : 0.f;
    }
    __syncthreads();
    copy_out(b0, sa, (float *)c.in, O + Z, O + Z, rows, row0);                         // c.in: this group's rows of the stored concatenation
    const lds_f *m = chain_forward<RB>(a.ws, c, b0, b1, true, a.clip_on != 0, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, a.A, c.out_stride, rows, row0);
    store_sigma(m, sm, a.A, a.std, a.sig[role], a.sig_stride[role], rows, row0);
}

// the forward's grid.  Critic: the critic's chain.  Student: the actor down to layer 1 (its latent is a constant of this pass).  Teacher:
// the actor, on through actor layer 0 and, from its latent columns, the privilege encoder.
template <int RB> __global__ __launch_bounds__(256) void train_cts_input_grad_kernel(CArgs a) {
    extern __shared__ __align__(16) float lds[];
    int tile;
    const int role = role_of(a, tile);
    const TChain &c = a.c[role == LG_TRAIN_CTS_ROLE_CRITIC ? CRI : role == STU ? STA : ACT];
    const int n = a.rows[role == LG_TRAIN_CTS_ROLE_CRITIC ? CRI : role == STU ? HIS : PRI];
    const int R = a.R, row0 = tile * R;
    const int rows = min(R, n - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, nullptr, nullptr, role != LG_TRAIN_CTS_ROLE_CRITIC && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);
    if (role != TEA) return;
    // G_0 of the actor sits in b1.  Through actor layer 0: d loss / d [obs | z] into b0 at the stride the concatenation had there.  No
    // ELU factor: the concatenation is no activation.
    const TLayer &L0 = c.l[0];
    bwd_layer<RB>(L0, b1, b0, false, R);
    __syncthreads();                                                   // b0 is complete; b1 (G_0 and its copy to the workspace) has been read
    const TChain &e = a.c[PRI];
    const int ne = e.n_layers;
    const TLayer &EL = e.l[ne - 1];
    const int Z = EL.M, O = L0.K - Z;
    lds_f *s0 = a.enc_start[TEA] ? b1 : b0, *s1 = a.enc_start[TEA] ? b0 : b1;      // the encoder's forward pair: its G_L belongs in b1
    {
        lds_f *g = (ne & 1) ? s1 : s0;
        float *gws = a.ws + EL.g_off;
        for (int i = threadIdx.x; i < R * Z; i += kThreads) {
            const int row = i / Z, col = i - row * Z;
            const float v = b0[row * L0.sa + O + col];                 // rows behind `rows` carry zeros: their G_L was zero
            if (row < rows) gws[(size_t)(row0 + row) * Z + col] = v;
            g[row * EL.so + col] = v;
        }
    }
    __syncthreads();
    chain_backward<RB>(a.ws, e, s0, s1, R, rows, row0);
}

// one wave per job, as lg_train_pass.h's wgrad_job with the rows of the job's own chain and the two std slabs
__global__ __launch_bounds__(64) void train_cts_weight_grad_kernel(CArgs a) {
    const int job = blockIdx.x;
    if (job >= a.std_job0) {
        const int j = job - a.std_job0, g = j >= a.grp_S[TEA] ? STU : TEA, s = g ? j - a.grp_S[TEA] : j;
        colsum_wave(a.gsig[g], a.gsig_stride[g], a.A, a.ws + a.std_p_off + (g ? (size_t)a.grp_S[TEA] * a.A : 0), s, a.grp_rps[g], a.rows[g ? HIS : PRI]);
        return;
    }
    int ci = PRI, li = 0;
    for (int c = PRI; c <= CRI; c++)
        for (int l = 0; l < a.c[c].n_layers; l++)
            if (job >= a.c[c].l[l].job0) { ci = c; li = l; }          // job0 rises with (c, l)
    const TChain &c = a.c[ci];
    const TLayer &L = c.l[li];
    wgrad_wave(L, a.ws + L.g_off, li ? a.ws + c.l[li - 1].h_off : c.in, li ? L.K : c.in_stride, a.ws, job - L.job0, a.rows[ci]);
}

__global__ __launch_bounds__(256) void train_cts_combine_kernel(CArgs a) { combine_all(a, a.c, PRI, CRI + 1); }

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChainCTS[LG_TRAIN_CTS_CHAINS] = {"chain[0] (privilege encoder)", "chain[1] (actor)", "chain[2] (critic)", "chain[3] (history encoder)"};
static const char *kGroup[LG_TRAIN_CTS_GROUPS] = {"[0] (teacher)", "[1] (student)"};
static void (*const kForward[2])(CArgs) = {train_cts_forward_kernel<1>, train_cts_forward_kernel<2>};
static void (*const kInputGrad[2])(CArgs) = {train_cts_input_grad_kernel<1>, train_cts_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_input_grad[2][64];

static int make_plan_cts(const char *fn, const LgTrainCTSArgs *p, LgTrainCTSPlan &pl, CArgs &k) {
    const std::string f(fn);
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (p->n_teacher < 1) return lg_fail_msg(f + ": n_teacher = " + std::to_string(p->n_teacher) + " < 1");
    if (p->n_student < 1) return lg_fail_msg(f + ": n_student = " + std::to_string(p->n_student) + " < 1");
    if (p->n_critic < 1) return lg_fail_msg(f + ": n_critic = " + std::to_string(p->n_critic) + " < 1");
    if (p->n_obs < 1) return lg_fail_msg(f + ": n_obs = " + std::to_string(p->n_obs) + " < 1");
    if ((long long)p->n_teacher + p->n_student > INT32_MAX) return lg_fail_msg(f + ": n_teacher + n_student is above 2^31 - 1");
    pl = LgTrainCTSPlan{};
    k = CArgs{};
    int w[2] = {0, 0};
    const int Bt = p->n_teacher, Bs = p->n_student, Bc = p->n_critic;
    k.rows[PRI] = Bt; k.rows[ACT] = Bt + Bs; k.rows[CRI] = Bc; k.rows[HIS] = Bs;
    k.enc_start[TEA] = pl.enc_first_buffer[TEA] = (p->chain[PRI].n_layers & 1) ? 0 : 1;
    k.enc_start[STU] = pl.enc_first_buffer[STU] = (p->chain[HIS].n_layers & 1) ? 0 : 1;
    for (int ci = 0; ci < LG_TRAIN_CTS_CHAINS; ci++)
        if (plan_chain(f + ": " + kChainCTS[ci], p->chain[ci], k.c[ci], ci == PRI ? k.enc_start[TEA] : ci == HIS ? k.enc_start[STU] : 0, w)) return 1;
    const int O = p->n_obs, Z = k.c[PRI].l[k.c[PRI].n_layers - 1].M, Zh = k.c[HIS].l[k.c[HIS].n_layers - 1].M;
    if (Zh != Z)
        return lg_fail_msg(f + ": " + kChainCTS[HIS] + ".layer[" + std::to_string(k.c[HIS].n_layers - 1) + "].n_out = " + std::to_string(Zh) +
                           ", but the privilege encoder ends at " + std::to_string(Z) + " columns: the two encoders' output widths differ");
    if (k.c[ACT].l[0].K != O + Z)
        return lg_fail_msg(f + ": " + kChainCTS[ACT] + ".layer[0].n_in = " + std::to_string(k.c[ACT].l[0].K) + ", but [obs | encoder output] has " +
                           std::to_string(O) + " + " + std::to_string(Z) + " columns (n_obs + the encoders' last n_out)");
    // the workspace: the concatenation, h / g of the three stored chains over their own rows, the slice partials, the two std slabs
    long long off = 0;
    int jobs = 0;
    pl.cat_off = k.cat_off = off; off += (long long)(Bt + Bs) * (O + Z);
    for (int ci = 0; ci < LG_TRAIN_CTS_CHAINS; ci++)
        for (int li = 0; li < LG_POLICY_MAX_LAYERS; li++) pl.h_off[ci][li] = pl.g_off[ci][li] = pl.p_off[ci][li] = -1;
    for (int ci = PRI; ci <= CRI; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            if (li < k.c[ci].n_layers - 1) { L.h_off = pl.h_off[ci][li] = off; off += (long long)k.rows[ci] * L.M; }
            L.g_off = pl.g_off[ci][li] = off; off += (long long)k.rows[ci] * L.M;
        }
    for (int ci = PRI; ci <= CRI; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            const int tn = (L.M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            L.tiles_k = (L.K + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            slice_rule(k.rows[ci], (long long)tn * L.tiles_k, L.S, L.rps, LG_TRAIN_TS_TARGET_JOBS);
            pl.slices[ci][li] = L.S; pl.slice_rows[ci][li] = L.rps;
            L.p_off = pl.p_off[ci][li] = off; off += (long long)L.S * ((long long)L.M * L.K + L.M);
            L.job0 = jobs; jobs += L.S * tn * L.tiles_k;
        }
    k.A = k.c[ACT].l[k.c[ACT].n_layers - 1].M;
    slice_rule(Bt, 1, k.grp_S[TEA], k.grp_rps[TEA], LG_TRAIN_TS_TARGET_JOBS);
    slice_rule(Bs, 1, k.grp_S[STU], k.grp_rps[STU], LG_TRAIN_TS_TARGET_JOBS);
    for (int g = 0; g < LG_TRAIN_CTS_GROUPS; g++) { pl.std_slices[g] = k.grp_S[g]; pl.std_slice_rows[g] = k.grp_rps[g]; }
    k.std_S = k.grp_S[TEA] + k.grp_S[STU];                     // what the combine adds: the teacher's partials first
    k.std_p_off = pl.std_p_off = off; off += (long long)k.std_S * k.A;
    k.std_job0 = jobs; jobs += k.std_S;
    k.n_jobs = pl.weight_jobs = jobs;
    k.N = Bt + Bs; k.c0 = PRI; k.c1 = CRI + 1;
    pl.workspace_floats = off;
    for (int R = 32; R >= 8; R >>= 1) {
        const size_t bytes = (size_t)R * (w[0] + w[1]) * sizeof(float);
        if (bytes > kLdsBytes) continue;
        k.R = pl.row_tile = R; k.q_off = R * w[0]; k.red_off = R * (w[0] + w[1]); pl.lds_bytes = (int)bytes;
        k.tiles[TEA] = pl.tiles[TEA] = (Bt + R - 1) / R;
        k.tiles[STU] = pl.tiles[STU] = (Bs + R - 1) / R;
        k.tiles[LG_TRAIN_CTS_ROLE_CRITIC] = pl.tiles[LG_TRAIN_CTS_ROLE_CRITIC] = (Bc + R - 1) / R;
        k.n_tiles = k.tiles[0] + k.tiles[1] + k.tiles[2];
        return 0;
    }
    return lg_fail_msg(f + ": an 8-row tile of these widths (" + std::to_string(w[0] + w[1]) + " floats per row) does not fit the 160 KB of LDS");
}

static int bind_cts(const char *fn, const LgTrainCTSArgs *p, const LgTrainCTSPlan &pl, CArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_CTS_CHAINS; ci++)
        if (bind_chain(f + ": " + kChainCTS[ci], p->chain[ci], k.c[ci], ci == ACT ? p->n_obs : p->chain[ci].layer[0].n_in, backward && ci != HIS)) return 1;
    const int A = k.A, V = k.c[CRI].l[k.c[CRI].n_layers - 1].M, O = p->n_obs;
    if (!p->student_obs) return lg_fail_msg(f + ": student_obs is null");
    if (p->student_obs_stride < O) return lg_fail_msg(f + ": student_obs_stride = " + std::to_string(p->student_obs_stride) + " is below its width " + std::to_string(O));
    if (p->clip_on && !(p->clip_actions >= 0.f)) return lg_fail_msg(f + ": clip_actions must be >= 0 under clip_on");
    if (!p->std) return lg_fail_msg(f + ": std is null");
    for (int g = 0; g < LG_TRAIN_CTS_GROUPS; g++) {
        if (!p->mu[g]) return lg_fail_msg(f + ": mu" + kGroup[g] + " is null");
        if (!p->sigma[g]) return lg_fail_msg(f + ": sigma" + kGroup[g] + " is null");
        if (p->mu_stride[g] < A) return lg_fail_msg(f + ": mu_stride" + kGroup[g] + " = " + std::to_string(p->mu_stride[g]) + " is below its width " + std::to_string(A));
        if (p->sigma_stride[g] < A) return lg_fail_msg(f + ": sigma_stride" + kGroup[g] + " = " + std::to_string(p->sigma_stride[g]) + " is below its width " + std::to_string(A));
    }
    if (!p->values) return lg_fail_msg(f + ": values is null");
    if (p->values_stride < V) return lg_fail_msg(f + ": values_stride = " + std::to_string(p->values_stride) + " is below its width " + std::to_string(V));
    if (backward) {
        if (!p->grad_std) return lg_fail_msg(f + ": grad_std is null");
        for (int g = 0; g < LG_TRAIN_CTS_GROUPS; g++) {
            if (!p->grad_mu[g]) return lg_fail_msg(f + ": grad_mu" + kGroup[g] + " is null");
            if (!p->grad_sigma[g]) return lg_fail_msg(f + ": grad_sigma" + kGroup[g] + " is null");
            if (p->grad_mu_stride[g] < A)
                return lg_fail_msg(f + ": grad_mu_stride" + kGroup[g] + " = " + std::to_string(p->grad_mu_stride[g]) + " is below its width " + std::to_string(A));
            if (p->grad_sigma_stride[g] < A)
                return lg_fail_msg(f + ": grad_sigma_stride" + kGroup[g] + " = " + std::to_string(p->grad_sigma_stride[g]) + " is below its width " + std::to_string(A));
        }
        if (!p->grad_values) return lg_fail_msg(f + ": grad_values is null");
        if (p->grad_values_stride < V) return lg_fail_msg(f + ": grad_values_stride = " + std::to_string(p->grad_values_stride) + " is below its width " + std::to_string(V));
    }
    if (check_ws(f, p->workspace, p->workspace_capacity, pl.workspace_floats, false)) return 1;
    k.ws = p->workspace; k.std = p->std; k.grad_std = p->grad_std;
    k.clip_on = p->clip_on != 0; k.clip = p->clip_actions;
    k.obs[TEA] = p->chain[ACT].input; k.obs_stride[TEA] = p->chain[ACT].in_stride;
    k.obs[STU] = p->student_obs; k.obs_stride[STU] = p->student_obs_stride;
    for (int g = 0; g < LG_TRAIN_CTS_GROUPS; g++) {
        k.sig[g] = p->sigma[g]; k.sig_stride[g] = p->sigma_stride[g];
        k.gsig[g] = p->grad_sigma[g]; k.gsig_stride[g] = p->grad_sigma_stride[g];
    }
    TChain &act = k.c[ACT], &cri = k.c[CRI];
    const int K0 = act.l[0].K;
    act.in = p->workspace + pl.cat_off; act.in_stride = K0;            // the stored concatenation, Bt + Bs rows
    act.out = p->mu[TEA]; act.out_stride = p->mu_stride[TEA];
    act.gin = p->grad_mu[TEA]; act.gin_stride = p->grad_mu_stride[TEA];
    cri.out = p->values; cri.out_stride = p->values_stride;
    cri.gin = p->grad_values; cri.gin_stride = p->grad_values_stride;
    // the student's descriptor of the actor: the same weights, every region advanced by the teacher's rows.  Its gradient pointers are
    // never read: the weight gradients and the combine go through c[ACT].
    const long long Bt = p->n_teacher;
    TChain &st = k.c[STA];
    st = act;
    st.in = act.in + Bt * K0;
    st.out = p->mu[STU]; st.out_stride = p->mu_stride[STU];
    st.gin = p->grad_mu[STU]; st.gin_stride = p->grad_mu_stride[STU];
    for (int li = 0; li < act.n_layers; li++) {
        TLayer &L = st.l[li];
        if (li < act.n_layers - 1) L.h_off += Bt * L.M;
        L.g_off += Bt * L.M;
        L.gW = nullptr; L.gb = nullptr;
    }
    return 0;
}

static int launch_role_tiles(const char *fn, void (*const (&kern)[2])(CArgs), bool (&raised)[2][64], int lds_bytes, hipStream_t stream, const CArgs &k) {
    const int rb = k.R == 32;
    if (raise_lds(fn, (const void *)kern[rb], raised[rb])) return 1;
    hipLaunchKernelGGL(kern[rb], dim3((unsigned)k.n_tiles), dim3(kThreads), (size_t)lds_bytes, stream, k);
    return 0;
}

extern "C" int lg_train_cts_plan(const LgTrainCTSArgs *args, LgTrainCTSPlan *out) {
    if (!out) return lg_fail_msg("lg_train_cts_plan: null plan");
    CArgs k;
    return make_plan_cts("lg_train_cts_plan", args, *out, k);
}

extern "C" int lg_train_cts_forward(const LgTrainCTSArgs *args, void *stream) {
    static const char *fn = "lg_train_cts_forward";
    LgTrainCTSPlan pl; CArgs k;
    if (make_plan_cts(fn, args, pl, k) || bind_cts(fn, args, pl, k, false)) return 1;
    return launch_role_tiles(fn, kForward, raised_forward, pl.lds_bytes, (hipStream_t)stream, k) || done(fn);
}

extern "C" int lg_train_cts_backward(const LgTrainCTSArgs *args, void *stream) {
    static const char *fn = "lg_train_cts_backward";
    LgTrainCTSPlan pl; CArgs k;
    if (make_plan_cts(fn, args, pl, k) || bind_cts(fn, args, pl, k, true)) return 1;
    if (launch_role_tiles(fn, kInputGrad, raised_input_grad, pl.lds_bytes, (hipStream_t)stream, k)) return 1;
    hipLaunchKernelGGL(train_cts_weight_grad_kernel, dim3((unsigned)k.n_jobs), dim3(64), 0, (hipStream_t)stream, k);
    long long elems = k.A;
    for (int ci = PRI; ci <= CRI; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            const long long n = (long long)k.c[ci].l[li].M * k.c[ci].l[li].K + k.c[ci].l[li].M;
            if (n > elems) elems = n;
        }
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(train_cts_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    return done(fn);
}
