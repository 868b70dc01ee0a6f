// gx_safelayer.hip -- libguardx_safelayer.so (include/guardx_safelayer.h): `ac.step(o)` followed by the safety layer's
// action correction (safe_rl_libX/safelayer/safelayer.py:514-546, safelayer_core.py:147-190; Dalal et al. 2018) for one
// control step over all envs, with the prev_c update of the step just made in front of it.  The observation row feeds
// three two-hidden-layer tanh networks: the actor's mu_net, the critic v and g_net, whose A outputs are the cost's
// predicted sensitivity to the action.
//
// The networks' arithmetic is the fused rollout's (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward): every
// hidden unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias (that instruction accumulates
// exactly like a sequential fmaf chain, tools/probes/mfma_f32_probe.hip), then tanh_f; an output is 16 lane partials over
// the units 64 c + 4 l + j folded by the butterfly of head2_out; the noise, the action and log pi(a | o) are those of
// gx_policy_step.hip:policy_step_tail (gx_step.h:sample_row).  The actor and v therefore give the bits of rollout_policy.  The correction's
// order of operations is the header's, one IEEE operation per operator (the library is built with -ffp-contract=off).
//
// Organisation: a 768-thread workgroup (12 waves) serves 16 envs from ONE staged copy of their rows.  Waves 4 n .. 4 n + 3
// own network n (0 actor, 1 v, 2 g) and a quarter of its hidden units each: H / 64 output tiles of 16 adjacent units per
// wave, the tiling of the step-wise rollout_policy (gx_policy_step.hip:policy_step_mfma_kernel).  The B operands are the
// hidden layers transposed to [k][unit] (gxl_prepare, into the caller's workspace, once per call): read by every
// workgroup, resident in L2, fetched eight k-steps ahead of the MFMAs that consume them.  The A operands (the rows
// zero-padded to a multiple of four, then the first hidden layer) come from LDS.  At env_num = 2000 this is 125
// workgroups on 256 CUs: the launch is bound by latency, which is why the three networks run side by side, each on four
// waves.
//
// The one-episode form (guardx_safelayer_policy_step_episode, the `safelayer_one_episode` learner) is the same kernel under the
// uniform argument StepCommon::ep.on: the rows sanitised, the first-done bookkeeping after the prologue's copies
// (gx_step.h), prev_c = the step's cost whatever `done` says, and the tail's no-bootstrap rule.
//
// Here: the LDS layout, the correction, the kernel and the C entry points.  The hidden layers' MFMA chain, the sample /
// log-prob block, the transpose kernel and the host side's checks, dispatch and launches are gx_step.h's, shared with
// the other step libraries.
#include "../../include/guardx_safelayer.h"
#include "gx_step.h"

#ifndef GXL_BUILD_ID
#define GXL_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxl_status fail(gxl_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kThreads = 768;  // 12 waves: four per network

// per env in `outs`: mu[A] | v | g[A] | act[A]
GX_HD int outs_stride(int A) { return 3 * A + 1; }

// LDS, in floats: pi head | v head | g head (b1 b2 W3 b3 each) | X [16][pad4 D + 1] | H1 pi, v [16][H + 4], g [16][HG + 4] |
// H2 likewise | outs [16][3 A + 1]
struct Lds { int headP, headV, headG, X, H1, H2, outs, total; };
GX_HD Lds lds_layout(int D, int A, int H, int HG)
{
    Lds L;
    int o = 0;
    L.headP = o; o += pad4(mlp2_head_floats(A, H));
    L.headV = o; o += pad4(mlp2_head_floats(1, H));
    L.headG = o; o += pad4(mlp2_head_floats(A, HG));
    L.X = o; o += pad4(kEnv * (pad4(D) + 1));
    const int hid = kEnv * (2 * (H + 4) + (HG + 4));
    L.H1 = o; o += hid;
    L.H2 = o; o += hid;
    L.outs = o; o += pad4(kEnv * outs_stride(A));
    L.total = o;
    return L;
}
size_t lds_bytes(int D, int A, int H, int HG) { return sizeof(float) * (size_t)lds_layout(D, A, H, HG).total; }

// The correction of include/guardx_safelayer.h on one row; __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn: one IEEE
// operation each, whatever the contraction setting.
GX_D void safety_correct(const float* g, const float* a, int A, float prev_c, float delta, float* a_safe)
{
    float ga = __fmul_rn(g[0], a[0]), gg = __fmul_rn(g[0], g[0]);
    for (int k = 1; k < A; ++k) {
        ga = __fadd_rn(ga, __fmul_rn(g[k], a[k]));
        gg = __fadd_rn(gg, __fmul_rn(g[k], g[k]));
    }
    const float pred = __fadd_rn(ga, prev_c);
    if (pred <= delta) {
        for (int k = 0; k < A; ++k) a_safe[k] = a[k];
        return;
    }
    const float numer = __fsub_rn(pred, delta);
    const float denom = __fadd_rn(gg, 1e-8f);
    float mult = __fdiv_rn(numer, denom);
    mult = mult > 0.0f ? mult : 0.0f;
    for (int k = 0; k < A; ++k) {
        float x = __fsub_rn(a[k], __fmul_rn(mult, g[k]));
        x = x < -1.0f ? -1.0f : x;
        x = x > 1.0f ? 1.0f : x;
        a_safe[k] = x;
    }
}

__global__ void correction_probe_kernel(int n, int A, const float* __restrict__ g, const float* __restrict__ a,
                                        const float* __restrict__ prev_c, float delta, float* __restrict__ a_safe)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        safety_correct(g + (size_t)i * A, a + (size_t)i * A, A, prev_c[i], delta, a_safe + (size_t)i * A);
}

// the kernel's view of gxl_step_args: this step's row blocks resolved on the host
struct StepArgs {
    StepCommon c;
    int D, A, correct;
    float delta;
    const float* gp;
    float* prev_c;
    float *act_safe, *g, *prev_cost; // row block t
};

template <int H, int HG>
__global__ __launch_bounds__(kThreads) void safelayer_step_kernel(StepArgs sa)
{
    const StepCommon& a = sa.c;
    constexpr int HS = H + 4, HSG = HG + 4;
    extern __shared__ float4 sl_lds4[];
    float* lds = reinterpret_cast<float*>(sl_lds4);
    const int D = sa.D, A = sa.A, Dp = pad4(D), XS = Dp + 1, OS = outs_stride(A);
    const Lds L = lds_layout(D, A, H, HG);
    float* X = lds + L.X;
    float* H1 = lds + L.H1;
    float* H2 = lds + L.H2;
    float* outs = lds + L.outs;
    const int tid = threadIdx.x, wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int net = wave >> 2, quarter = wave & 3;
    const int env0 = blockIdx.x * kEnv;
    const int msz_pi = (int)net_floats(D, A, H), msz_v = (int)net_floats(D, 1, H);

    mlp2_head_stage(lds + L.headP, a.params, D, A, tid, kThreads, H);
    mlp2_head_stage(lds + L.headV, a.params + msz_pi, D, 1, tid, kThreads, H);
    mlp2_head_stage(lds + L.headG, sa.gp, D, A, tid, kThreads, HG);
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);
    const Mlp2Head hg = mlp2_head_view(lds + L.headG, A, HG);

    // prologue: the prev_c update of the step just made (safelayer.py:546, 576-581).  The thread that updates env's
    // prev_c here is the one that reads it below (tid < kEnv, env = env0 + tid): program order, no fence.  In the
    // one-episode form nothing is re-initialised at a done, so prev_c is the step's cost whatever `done` says
    // (safelayer_one_episode/safelayer.py:553), and the first-done bookkeeping follows the copies.
    float prev_c = 0.0f;
    if (tid < kEnv) {
        const int env = env0 + tid;
        if (env < a.N) {
            if (a.prologue) {
                const float rew = a.rew_in[env], cost = a.cost_in[env], done = a.done_in[env];
                a.rew_p[env] = rew;
                a.cost_p[env] = cost;
                a.done_p[env] = done;
                if (a.ep.on) episode_book(a.ep, env, rew, cost, done);
                prev_c = (done > 0.0f && !a.ep.on) ? 0.0f : cost;
                sa.prev_c[env] = prev_c;
            } else if (!a.tail)
                prev_c = sa.prev_c[env];
        }
    }
    stage_rows(a, D, XS, X, env0, tid, kThreads); // (sanitised in the one-episode form)
    wg_sync_lds(); // rows and heads

    const bool skip = a.tail && net != 1; // the bootstrap needs the critic only
    const float* wtn = a.wt + (size_t)net * wt_floats(D, H); // (net 2 starts after the two H-wide networks)
    float* h1 = H1 + net * kEnv * HS;
    float* h2 = H2 + net * kEnv * HS;
    if (!skip) {
        if (net < 2) hidden_layer<H / 64, true>((net ? hv : hp).b1, wtn, H, (H / 4) * quarter, X, XS, Dp, h1, c16, kq);
        else hidden_layer<HG / 64, true>(hg.b1, wtn, HG, (HG / 4) * quarter, X, XS, Dp, h1, c16, kq);
    }
    wg_sync_lds();
    if (!skip) {
        if (net < 2) hidden_layer<H / 64, true>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, (H / 4) * quarter, h1, HS, H, h2, c16, kq);
        else hidden_layer<HG / 64, true>(hg.b2, wtn + (size_t)Dp * HG, HG, (HG / 4) * quarter, h1, HSG, HG, h2, c16, kq);
    }
    wg_sync_lds();
    // output layers: task (env e, output o) on 16 lanes; o < A: mu_o, o == A: the value, o > A: g_(o - A - 1), which
    // goes out from here
    const int l = tid & 15;
    for (int task = tid >> 4; task < kEnv * (2 * A + 1); task += kThreads / 16) {
        const int e = task / (2 * A + 1), o = task - e * (2 * A + 1);
        if (a.tail && o != A) continue; // (16-lane groups take the branch together)
        float y;
        if (o < A) y = head2_out<H>(hp, o, l, H2 + e * HS);
        else if (o == A) y = head2_out<H>(hv, 0, l, H2 + (kEnv + e) * HS);
        else y = head2_out<HG>(hg, o - A - 1, l, H2 + 2 * kEnv * HS + e * HSG);
        if (l == 0) {
            outs[e * OS + o] = y;
            if (o > A && env0 + e < a.N) sa.g[(size_t)(env0 + e) * A + (o - A - 1)] = y;
        }
    }
    wg_sync_lds();
    // per env: the value, and (not in the tail) the noise, the action and log pi(a | o) of ac.step, then the correction
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            float* oe = outs + e * OS;
            a.val[env] = tail_row_unusable(a, D, env) ? 0.0f : oe[A];
            if (!a.tail) {
                sample_row(a, A, gls, env, oe, oe + 2 * A + 1);
                sa.prev_cost[env] = prev_c;
                float* as = sa.act_safe + (size_t)env * A;
                if (sa.correct) safety_correct(oe + A + 1, oe + 2 * A + 1, A, prev_c, sa.delta, as);
                else
                    for (int d = 0; d < A; ++d) as[d] = oe[2 * A + 1 + d];
            }
        }
    }
    if (!a.tail) logstd_write(a.logstd, gls, A, tid);
}

struct StepKernel { template <int H, int HG> static const void* get() { return reinterpret_cast<const void*>(safelayer_step_kernel<H, HG>); } };

} // namespace

extern "C" const char* gxl_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxl_build_id(void) { return GXL_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["safelayer"].source_hash()

extern "C" int64_t gxl_params_floats(int32_t D, int32_t A, int32_t hidden) { return params_floats(D, A, hidden); }

extern "C" int64_t gxl_g_floats(int32_t D, int32_t A, int32_t g_hidden)
{
    return (shape_ok(D, A) && width_ok(g_hidden)) ? net_floats(D, A, g_hidden) : -1;
}

extern "C" int64_t gxl_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden) { return work_floats(D, A, hidden, g_hidden); }

extern "C" gxl_status gxl_prepare(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden, const float* d_params,
                                  const float* d_g_params, float* d_work, void* stream)
{
    return prepare<StepKernel>(fail, "gxl_prepare", kRowD, lds_bytes, D, A, hidden, g_hidden, D, d_params, d_g_params, d_work, stream);
}

namespace {

// gxl_policy_step (book == null) and guardx_safelayer_policy_step_episode under their own names
gxl_status policy_step(const char* who, const gxl_step_args* g, const gx_first_done_state* book, bool episode, void* stream)
{
    gxl_status st = check_common(
        fail, who, g, kRowD, lds_bytes, &gxl_step_args::D, &gxl_step_args::g_hidden, &gxl_step_args::d_g_params,
        [](const gxl_step_args&) { return true; }, "",
        [](const gxl_step_args& g, bool tail) { return g.d_prev_c && (tail || (g.d_act_safe && g.d_g && g.d_prev_cost)); });
    if (st == GXL_OK && episode) st = check_book(fail, who, book);
    if (st != GXL_OK || g->N == 0) return st;
    StepArgs a;
    const size_t tn = fill_common(*g, g->D, a.c), A = (size_t)g->A;
    fill_book(book, g->t, a.c);
    a.D = g->D; a.A = g->A; a.correct = g->correct != 0;
    a.delta = g->delta;
    a.gp = g->d_g_params;
    a.prev_c = g->d_prev_c;
    a.act_safe = a.c.tail ? nullptr : g->d_act_safe + tn * A;
    a.g = a.c.tail ? nullptr : g->d_g + tn * A;
    a.prev_cost = a.c.tail ? nullptr : g->d_prev_cost + tn;
    return q_launch(fail, who, q_kernel_for<StepKernel>(g->hidden, g->g_hidden), g->N, kThreads, a,
                    lds_bytes(g->D, g->A, g->hidden, g->g_hidden), stream);
}

} // namespace

extern "C" gxl_status gxl_policy_step(const gxl_step_args* g, void* stream)
{
    return policy_step("gxl_policy_step", g, nullptr, false, stream);
}

extern "C" gxl_status guardx_safelayer_policy_step_episode(const gxl_step_args* g, const gx_first_done_state* book, void* stream)
{
    return policy_step("guardx_safelayer_policy_step_episode", g, book, true, stream);
}

extern "C" gxl_status guardx_safelayer_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t g_hidden, const float* d_params,
                                     const float* d_g_params, const float* d_work, const float* d_rows, float* d_obs_last,
                                     float* d_val_last, void* stream)
{
    const char* who = "guardx_safelayer_tail_probe";
    if (n < 0) return fail(GXL_ERR_ARG, std::string(who) + ": n must be >= 0");
    const gxl_status st = check_shape(fail, who, kRowD, lds_bytes, D, A, hidden, g_hidden);
    if (st != GXL_OK) return st;
    if (!d_params || !d_g_params || !d_work || !d_rows || !d_obs_last || !d_val_last)
        return fail(GXL_ERR_ARG, std::string(who) + ": null pointer");
    if (n == 0) return GXL_OK;
    StepArgs a = {};
    fill_tail_probe(a.c, n, d_params, d_work, d_rows, d_obs_last, d_val_last);
    a.D = D; a.A = A;
    a.gp = d_g_params;
    return q_launch(fail, who, q_kernel_for<StepKernel>(hidden, g_hidden), n, kThreads, a, lds_bytes(D, A, hidden, g_hidden), stream);
}

extern "C" gxl_status gxl_correction_probe(int32_t n, int32_t A, const float* d_g, const float* d_a, const float* d_prev_c,
                                           float delta, float* d_a_safe, void* stream)
{
    if (!d_g || !d_a || !d_prev_c || !d_a_safe) return fail(GXL_ERR_ARG, "gxl_correction_probe: null pointer");
    if (n < 0) return fail(GXL_ERR_ARG, "gxl_correction_probe: n must be >= 0");
    if (A < 1 || A > kMaxA) return fail(GXL_ERR_UNSUPPORTED, "gxl_correction_probe: A must be in 1 .. 16");
    if (n == 0) return GXL_OK;
    return launch_flat(fail, "gxl_correction_probe", correction_probe_kernel, n, 4096, stream, n, A, d_g, d_a, d_prev_c, delta,
                       d_a_safe);
}
