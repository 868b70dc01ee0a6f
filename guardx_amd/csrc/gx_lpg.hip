// gx_lpg.hip -- libguardx_lpg.so (include/guardx_lpg.h): `ac.step(o)` of the LPG learner (safe_rl_libX/lpg/lpg.py:486-564,
// lpg_core.py:148-198, 224-233) for one control step over all envs: the actor's mu_net and the critic v on the observation
// row, the cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) on the sampled action, and the learner's correction:
// one closed-form projection a + lam G along G, the scaled gradient of Q at the ZERO action.
//
// The actor, v, the noise, the action and log pi(a | o) are the USL library's (gx_qstep.h:q_step_front) and therefore
// rollout_policy's; c_net runs on the device code the USL library uses (gx_qcritic.h), in the operation order
// include/guardx_usl.h fixes for one pass.
//
// Organisation: a 768-thread workgroup (12 waves) serves 16 envs from ONE staged copy of their rows.  Waves 0 .. 3 own the
// actor, 4 .. 7 the critic, 8 .. 11 the observation part P of c_net's first layer, a quarter of the hidden units each.
// Then two passes over c_net, one after the other on the q_waves(h_c) waves that share its unit tiles: the act pass (the
// A action terms on top of P, tanh, the forward GEMM, the head: qc) and, when the call corrects, the zero pass
// (h1 = tanh(P), the forward GEMM, the head, the backward GEMM against (1 - h2^2) w3, the (1 - h1^2) scale, the A output
// sums: G).  One lane per row then projects.  At h_c = 64 both layouts of W2 live in LDS; wider ones are streamed from L2.
//
// Here: the two passes' sequence, the per-row projection, the two kernels and the C entry points.  The pass itself is
// gx_qcritic.h:q_pass, the one USL's iteration runs; the step kernel's front end, the probe kernel's and the LDS layouts
// are gx_qstep.h's, shared with gx_usl.hip; the sample / log-prob block, the MFMA chain and the host side's checks,
// dispatch and launches are gx_step.h's, shared with every step library.
#include "../../include/guardx_lpg.h"
#include "gx_qstep.h"

#ifndef GXP_BUILD_ID
#define GXP_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxp_status fail(gxp_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

// the kernel's view of gxp_step_args
struct StepArgs {
    QStepCommon c;       // (c.q.niter and c.q.eta are USL's and unused here)
    int store;           // this launch writes q_init
    float sign;
    float* q_init;       // [N]
    float* lam;          // row block t
};

struct ProbeArgs {
    int n;
    float sign;
    QArgs q;
    const float *obs, *act, *q_init;
    float *a_safe, *qv, *G, *lam;
    int* branch;
};

// z3 of the two passes, held by the threads tid < 16 for their row (z0 = 0 when the call does not correct: no zero pass)
struct RowZ { float zact, z0; };

// The two passes over c_net (gx_qcritic.h:q_pass): the act pass, forward alone, and when the call corrects the zero pass
// with its backward pass, which leaves g~ in lds[L.gt].  Entry and exit as q_pass's.  Whole-workgroup call.
template <int HC>
GX_D RowZ q_passes(float* lds, const QLds& L, float* H1, float* H2, const QArgs& q, int tid)
{
    RowZ z;
    z.zact = z.z0 = 0.0f;
    float wa[kMaxA / 4][q_tiles(HC)];
    q_load_wa<HC>(wa, q, tid);
    q_pass<HC, true>(lds, L, H1, H2, q, wa, false, tid);
    if (tid < kEnv) z.zact = lds[L.z3 + tid]; // (the zero pass writes z3 two barriers from here)
    if (q.correct) {                          // uniform
        q_pass<HC, false>(lds, L, H1, H2, q, wa, true, tid);
        if (tid < kEnv) z.z0 = lds[L.z3 + tid];
    }
    return z;
}

// per row, what the projection returns
struct RowOut { float lam; int branch; };

// The projection of include/guardx_lpg.h on row `tid` (< 16), by that lane alone: lds[L.gt] row g~ -> G, lds[L.act] row
// act -> a_safe.  qc = Q(obs, act), z0 = the zero pass's z3, qi = the row's q_init.
GX_D RowOut project_row(float* lds, const QLds& L, const QArgs& q, float sign, float qc, float z0, float qi, int tid)
{
    RowOut ro;
    ro.lam = 0.0f; ro.branch = 0;
    if (!q.correct) return ro;
    const int A = q.A;
    float* g = lds + L.gt + tid * kAS;
    float* a = lds + L.act + tid * kAS;
    const float c0 = __fmul_rn(q.gscale, softplus_grad_f(z0));
    for (int k = 0; k < A; ++k) g[k] = __fmul_rn(c0, g[k]);
    if (qc <= q.delta) return ro;
    const float eps = fabsf(__fsub_rn(q.delta, qi));
    float top = __fmul_rn(g[0], a[0]), bot = __fmul_rn(g[0], g[0]);
    for (int k = 1; k < A; ++k) {
        top = __fadd_rn(top, __fmul_rn(g[k], a[k]));
        bot = __fadd_rn(bot, __fmul_rn(g[k], g[k]));
    }
    top = __fsub_rn(top, eps);
    float lam = __fdiv_rn(top, bot);
    lam = lam < 0.0f ? 0.0f : lam; // (a NaN stays a NaN)
    for (int k = 0; k < A; ++k) a[k] = __fadd_rn(a[k], __fmul_rn(sign, __fmul_rn(lam, g[k])));
    ro.lam = lam;
    ro.branch = lam > 0.0f ? 1 : 2;
    return ro;
}

template <int H, int HC>
__global__ __launch_bounds__(kThreads) void lpg_step_kernel(StepArgs a)
{
    extern __shared__ float4 lpg_lds4[];
    float* lds = reinterpret_cast<float*>(lpg_lds4);
    const Lds L = lds_layout(a.c.q.D, a.c.q.A, H, HC);
    const int A = a.c.q.A, tid = threadIdx.x, env0 = blockIdx.x * kEnv;
    if (q_step_front<H, HC>(lds, L, a.c, tid)) return; // the tail
    const int rows = a.c.N - env0 < kEnv ? a.c.N - env0 : kEnv;
    float* Q1 = lds + L.U;
    const RowZ z = q_passes<HC>(lds, L.q, Q1, Q1 + kEnv * (HC + 4), a.c.q, tid);
    if (tid < rows) {
        const int env = env0 + tid;
        const float qc = softplus_f(z.zact);
        float qi = qc;
        if (a.store) a.q_init[env] = qc;
        else if (a.c.q.correct) qi = a.q_init[env];
        const RowOut ro = project_row(lds, L.q, a.c.q, a.sign, qc, z.z0, qi, tid);
        a.c.qc[env] = qc;
        a.lam[env] = ro.lam;
        for (int d = 0; d < A; ++d) a.c.act_safe[(size_t)env * A + d] = lds[L.q.act + tid * kAS + d];
    }
}

template <int HC>
__global__ __launch_bounds__(kThreads) void lpg_probe_kernel(ProbeArgs a)
{
    extern __shared__ float4 lpg_lds4[];
    float* lds = reinterpret_cast<float*>(lpg_lds4);
    const Lds L = probe_lds_layout(a.q.D, a.q.A, HC);
    const int A = a.q.A, tid = threadIdx.x;
    const int row0 = blockIdx.x * kEnv;
    const int rows = a.n - row0 < kEnv ? a.n - row0 : kEnv;
    q_probe_front<HC>(lds, L, a.q, a.obs, a.act, row0, rows, tid);
    float* Q1 = lds + L.U;
    const RowZ z = q_passes<HC>(lds, L.q, Q1, Q1 + kEnv * (HC + 4), a.q, tid);
    if (tid < rows) {
        const int r = row0 + tid;
        const float qc = softplus_f(z.zact);
        const RowOut ro = project_row(lds, L.q, a.q, a.sign, qc, z.z0, a.q_init[r], tid);
        a.qv[r] = qc;
        a.lam[r] = ro.lam;
        a.branch[r] = ro.branch;
        for (int d = 0; d < A; ++d) {
            a.a_safe[(size_t)r * A + d] = lds[L.q.act + tid * kAS + d];
            a.G[(size_t)r * A + d] = lds[L.q.gt + tid * kAS + d];
        }
    }
}

struct StepKernel { template <int H, int HC> static const void* get() { return reinterpret_cast<const void*>(lpg_step_kernel<H, HC>); } };
struct ProbeKernel { template <int, int HC> static const void* get() { return reinterpret_cast<const void*>(lpg_probe_kernel<HC>); } };

} // namespace

extern "C" const char* gxp_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxp_build_id(void) { return GXP_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["lpg"].source_hash()

extern "C" int64_t gxp_params_floats(int32_t D, int32_t A, int32_t hidden) { return params_floats(D, A, hidden); }

extern "C" int64_t gxp_q_floats(int32_t D, int32_t A, int32_t c_hidden) { return q_floats(D, A, c_hidden); }

extern "C" int64_t gxp_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden) { return work_floats(D, A, hidden, c_hidden); }

extern "C" int64_t gxp_probe_work_floats(int32_t D, int32_t A, int32_t c_hidden) { return probe_work_floats(D, A, c_hidden); }

extern "C" gxp_status gxp_prepare(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                                  const float* d_c_params, float* d_work, void* stream)
{
    return q_prepare<StepKernel>(fail, "gxp_prepare", D, A, hidden, c_hidden, d_params, d_c_params, d_work, stream);
}

namespace {

// gxp_policy_step (book == null) and guardx_lpg_policy_step_episode under their own names
gxp_status policy_step(const char* who, const gxp_step_args* g, const gx_first_done_state* book, bool episode, void* stream)
{
    gxp_status st = q_check_common(
        fail, who, g, [](const gxp_step_args&) { return true; }, "",
        [](const gxp_step_args& g, bool tail) { return g.d_q_init && (tail || g.d_lam); });
    if (st == GXP_OK && episode) st = check_book(fail, who, book);
    if (st != GXP_OK || g->N == 0) return st;
    StepArgs a;
    const size_t tn = q_fill_common(*g, a.c);
    fill_book(book, g->t, a.c);
    a.store = g->t == 0 && g->store_init != 0;
    a.sign = g->step_sign;
    a.q_init = g->d_q_init;
    a.lam = a.c.tail ? nullptr : g->d_lam + tn;
    return q_launch(fail, who, q_kernel_for<StepKernel>(g->hidden, g->c_hidden), g->N, kThreads, a,
                    step_lds_bytes(g->D, g->A, g->hidden, g->c_hidden), stream);
}

} // namespace

extern "C" gxp_status gxp_policy_step(const gxp_step_args* g, void* stream)
{
    return policy_step("gxp_policy_step", g, nullptr, false, stream);
}

extern "C" gxp_status guardx_lpg_policy_step_episode(const gxp_step_args* g, const gx_first_done_state* book, void* stream)
{
    return policy_step("guardx_lpg_policy_step_episode", g, book, true, stream);
}

extern "C" gxp_status guardx_lpg_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                                     const float* d_c_params, const float* d_work, const float* d_rows, float* d_obs_last,
                                     float* d_val_last, void* stream)
{
    return q_tail_probe<StepKernel, StepArgs>(fail, "guardx_lpg_tail_probe", n, D, A, hidden, c_hidden, d_params, d_c_params, d_work,
                                              d_rows, d_obs_last, d_val_last, stream);
}

extern "C" gxp_status gxp_projection_probe(int32_t n, int32_t D, int32_t A, int32_t c_hidden, const float* d_c_params,
                                           float* d_work, const float* d_obs, const float* d_act, const float* d_q_init,
                                           float delta, float grad_scale, float step_sign, float* d_a_safe, float* d_q,
                                           float* d_G, float* d_lam, int32_t* d_branch, void* stream)
{
    if (!d_c_params || !d_work || !d_obs || !d_act || !d_q_init || !d_a_safe || !d_q || !d_G || !d_lam || !d_branch)
        return fail(GXP_ERR_ARG, "gxp_projection_probe: null pointer");
    if (n < 0) return fail(GXP_ERR_ARG, "gxp_projection_probe: n must be >= 0");
    ProbeArgs a;
    a.n = n;
    a.sign = step_sign;
    a.q = q_args(D, A, true, delta, grad_scale, d_c_params, d_work);
    a.obs = d_obs; a.act = d_act; a.q_init = d_q_init;
    a.a_safe = d_a_safe; a.qv = d_q; a.G = d_G; a.lam = d_lam; a.branch = d_branch;
    return q_probe_run<ProbeKernel>(fail, "gxp_projection_probe", n, D, A, c_hidden, d_c_params, d_work, a, stream);
}
