// gx_usl.hip -- libguardx_usl.so (include/guardx_usl.h): `ac.step(o)` of the USL learner (safe_rl_libX/usl/usl.py:478-553,
// usl_core.py:146-196, 239-248) for one control step over all envs: the actor's mu_net and the critic v on the observation
// row, the cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) on the sampled action, and the learner's correction:
// up to niter passes of a = a - eta acc / (max |acc| + 1e-8), acc the running sum over the passes so far of s, the scaled
// gradient of Q with respect to the action (the reference never clears act.grad).
//
// The networks' arithmetic is the fused rollout's (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward): every
// hidden unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias (that instruction accumulates
// exactly like a sequential fmaf chain, tools/probes/mfma_f32_probe.hip), then tanh_f; an output is 16 lane partials over
// the units 64 c + 4 l + j folded by a butterfly; the noise, the action and log pi(a | o) are those of
// gx_policy_step.hip:policy_step_tail.  The actor and v therefore give the bits of rollout_policy.  The backward pass and
// the update follow the header's order, one IEEE operation per operator.
//
// Organisation: a 768-thread workgroup (12 waves) serves 16 envs from ONE staged copy of their rows.  Waves 0 .. 3 own the
// actor, 4 .. 7 the critic, 8 .. 11 the observation part of c_net's first layer (its pre-activation without the action
// columns, kept in LDS for the whole launch), a quarter of the hidden units each.  The iteration is a serial chain per
// pass -- A action terms, tanh, the h_c x h_c forward GEMM, tanh, the head, the h_c x h_c backward GEMM against
// (1 - h2^2) w3, the (1 - h1^2) scale, the A output sums, the update -- so c_net's h_c / 16 unit tiles are spread over as
// many waves as divide them (4, 8, 12, 8 waves at h_c = 64, 128, 192, 256).  The forward GEMM reads the [k][unit]
// transposed copy of W2 (gxu_prepare), the backward GEMM reads W2 as torch lays it out, [unit j][k]: that IS the B operand
// of the transposed product.  At h_c = 64 both copies live in LDS; wider ones are streamed from L2, eight k-steps ahead of
// the MFMAs that consume them.  A workgroup leaves the loop when none of its rows is live (the reference's early break).
//
// Here: the iteration's per-row logic (the two tests, the update, the `live` vote), the two kernels and the C entry
// points.  The pass over c_net is gx_qcritic.h:q_pass; the step kernel's front end (ac.step up to the sampled action),
// the probe kernel's and the LDS layouts are gx_qstep.h's, shared with gx_lpg.hip; the sample / log-prob block, the MFMA
// chain and the host side's checks, dispatch and launches are gx_step.h's, shared with every step library.
#include "../../include/guardx_usl.h"
#include "gx_qstep.h"

#ifndef GXU_BUILD_ID
#define GXU_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxu_status fail(gxu_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

// the kernel's view of gxu_step_args
struct StepArgs {
    QStepCommon c;
    float* iters; // row block t
};

struct ProbeArgs {
    int n;
    QArgs q;
    const float *obs, *act;
    float *a_safe, *q0, *grad0;
    int *iters, *stop;
};

// per row, what the iteration returns
struct RowOut { float q0; int iters, stop; };

// One row's update on AA action components.  act.grad is never cleared between the reference's passes
// (usl_core.py:180-194), so the step uses acc, the running sum of the passes' scaled gradients s = c g: the first pass
// sets it (the first backward() sets act.grad), the later ones add to it.  g0 (may be null): where s itself goes.
template <int AA>
GX_D void q_update(float (&acc)[kMaxA], float* a, const float* g, float c, float eta, bool first, float* g0)
{
    float Z = 0.0f;
#pragma unroll
    for (int k = 0; k < AA; ++k) {
        const float s = __fmul_rn(c, g[k]);
        if (g0) g0[k] = s;
        acc[k] = first ? s : __fadd_rn(acc[k], s);
        const float m = fabsf(acc[k]);
        Z = (k == 0 || m > Z) ? m : Z;
    }
    const float den = __fadd_rn(Z, 1e-8f);
#pragma unroll
    for (int k = 0; k < AA; ++k) a[k] = __fsub_rn(a[k], __fmul_rn(eta, __fdiv_rn(acc[k], den)));
}

// The iteration of include/guardx_usl.h on the 16 rows of the workgroup.  On entry (after a barrier): the rows' actions in
// lds[L.act], P = the first layer's pre-activation over the observation columns, c_net's parts staged.  On exit (after a
// barrier): the final actions in lds[L.act]; the threads tid < 16 hold their row's result.  rows = valid rows;
// grad0 (may be null): [rows][A] in global memory.  Whole-workgroup call, every branch on pass state is uniform.
template <int HC>
GX_D RowOut q_iterate(float* lds, const QLds& L, float* H1, float* H2, const QArgs& q, int rows, float* grad0, int tid)
{
    const int A = q.A;
    float* act = lds + L.act;
    const float* gt = lds + L.gt;
    const float* z3 = lds + L.z3;
    int* live = reinterpret_cast<int*>(lds + L.live);
    const int npass = q.correct ? q.niter : 0;
    float wa[kMaxA / 4][q_tiles(HC)]; // hoisted out of the loop
    q_load_wa<HC>(wa, q, tid);
    RowOut ro;
    ro.q0 = 0.0f; ro.iters = 0; ro.stop = tid < rows ? -1 : 3;
    float acc[kMaxA]; // the row's running sum of s over its passes
#pragma unroll
    for (int k = 0; k < kMaxA; ++k) acc[k] = 0.0f;

    for (int pass = 0;; ++pass) {
        q_pass<HC, true>(lds, L, H1, H2, q, wa, npass > 0, tid);
        // per row: the two tests, then the update
        if (tid < kEnv) {
            const float z = z3[tid];
            const float qv = softplus_f(z);
            if (pass == 0) ro.q0 = qv;
            float* a = act + tid * kAS;
            bool moved = false;
            if (ro.stop < 0) {
                float mx = a[0];
                for (int k = 1; k < A; ++k) mx = a[k] > mx ? a[k] : mx;
                if (pass >= npass) ro.stop = 0;
                else if (mx > 1.0f) ro.stop = 1;
                else if (qv <= q.delta) ro.stop = 2;
                else {
                    const float c = __fmul_rn(q.gscale, softplus_grad_f(z));
                    const float* g = gt + tid * kAS;
                    float* g0 = pass == 0 && grad0 ? grad0 + (size_t)tid * A : nullptr;
                    switch (A) { // even, 2 .. kMaxA (gx_step.h:shape_ok): every form indexes acc statically
                    case 2: q_update<2>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 4: q_update<4>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 6: q_update<6>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 8: q_update<8>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 10: q_update<10>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 12: q_update<12>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    case 14: q_update<14>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    default: q_update<16>(acc, a, g, c, q.eta, ro.iters == 0, g0); break;
                    }
                    moved = true;
                    ro.iters += 1;
                    if (pass + 1 >= npass) ro.stop = 0;
                }
            }
            if (pass == 0 && grad0 && !moved && tid < rows)
                for (int k = 0; k < A; ++k) grad0[(size_t)tid * A + k] = 0.0f;
            live[tid] = ro.stop < 0;
        }
        wg_sync_lds();
        int any = 0;
#pragma unroll
        for (int e = 0; e < kEnv; e += 4) {
            const int4 v = *reinterpret_cast<const int4*>(live + e);
            any |= v.x | v.y | v.z | v.w;
        }
        if (!any) break; // workgroup-uniform
    }
    return ro;
}

template <int H, int HC>
__global__ __launch_bounds__(kThreads) void usl_step_kernel(StepArgs a)
{
    extern __shared__ float4 usl_lds4[];
    float* lds = reinterpret_cast<float*>(usl_lds4);
    const Lds L = lds_layout(a.c.q.D, a.c.q.A, H, HC);
    const int A = a.c.q.A, tid = threadIdx.x, env0 = blockIdx.x * kEnv;
    if (q_step_front<H, HC>(lds, L, a.c, tid)) return; // the tail
    const int rows = a.c.N - env0 < kEnv ? a.c.N - env0 : kEnv;
    float* Q1 = lds + L.U;
    const RowOut ro = q_iterate<HC>(lds, L.q, Q1, Q1 + kEnv * (HC + 4), a.c.q, rows, nullptr, tid);
    if (tid < rows) {
        const int env = env0 + tid;
        a.c.qc[env] = ro.q0;
        a.iters[env] = (float)ro.iters;
        for (int d = 0; d < A; ++d) a.c.act_safe[(size_t)env * A + d] = lds[L.q.act + tid * kAS + d];
    }
}

template <int HC>
__global__ __launch_bounds__(kThreads) void usl_probe_kernel(ProbeArgs a)
{
    extern __shared__ float4 usl_lds4[];
    float* lds = reinterpret_cast<float*>(usl_lds4);
    const Lds L = probe_lds_layout(a.q.D, a.q.A, HC);
    const int A = a.q.A, tid = threadIdx.x;
    const int row0 = blockIdx.x * kEnv;
    const int rows = a.n - row0 < kEnv ? a.n - row0 : kEnv;
    q_probe_front<HC>(lds, L, a.q, a.obs, a.act, row0, rows, tid);
    float* Q1 = lds + L.U;
    const RowOut ro = q_iterate<HC>(lds, L.q, Q1, Q1 + kEnv * (HC + 4), a.q, rows, a.grad0 + (size_t)row0 * A, tid);
    if (tid < rows) {
        const int r = row0 + tid;
        a.q0[r] = ro.q0;
        a.iters[r] = ro.iters;
        a.stop[r] = ro.stop;
        for (int d = 0; d < A; ++d) a.a_safe[(size_t)r * A + d] = lds[L.q.act + tid * kAS + d];
    }
}

struct StepKernel { template <int H, int HC> static const void* get() { return reinterpret_cast<const void*>(usl_step_kernel<H, HC>); } };
struct ProbeKernel { template <int, int HC> static const void* get() { return reinterpret_cast<const void*>(usl_probe_kernel<HC>); } };

} // namespace

extern "C" const char* gxu_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxu_build_id(void) { return GXU_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["usl"].source_hash()

extern "C" int64_t gxu_params_floats(int32_t D, int32_t A, int32_t hidden) { return params_floats(D, A, hidden); }

extern "C" int64_t gxu_q_floats(int32_t D, int32_t A, int32_t c_hidden) { return q_floats(D, A, c_hidden); }

extern "C" int64_t gxu_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden) { return work_floats(D, A, hidden, c_hidden); }

extern "C" int64_t gxu_probe_work_floats(int32_t D, int32_t A, int32_t c_hidden) { return probe_work_floats(D, A, c_hidden); }

extern "C" gxu_status gxu_prepare(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                                  const float* d_c_params, float* d_work, void* stream)
{
    return q_prepare<StepKernel>(fail, "gxu_prepare", D, A, hidden, c_hidden, d_params, d_c_params, d_work, stream);
}

namespace {

// gxu_policy_step (book == null) and guardx_usl_policy_step_episode under their own names
gxu_status policy_step(const char* who, const gxu_step_args* g, const gx_first_done_state* book, bool episode, void* stream)
{
    gxu_status st = q_check_common(
        fail, who, g, [](const gxu_step_args& g) { return g.niter >= 0; }, ", niter >= 0",
        [](const gxu_step_args& g, bool tail) { return tail || g.d_iters; });
    if (st == GXU_OK && episode) st = check_book(fail, who, book);
    if (st != GXU_OK || g->N == 0) return st;
    StepArgs a;
    const size_t tn = q_fill_common(*g, a.c);
    fill_book(book, g->t, a.c);
    a.c.q.niter = g->niter; a.c.q.eta = g->eta;
    a.iters = a.c.tail ? nullptr : g->d_iters + tn;
    return q_launch(fail, who, q_kernel_for<StepKernel>(g->hidden, g->c_hidden), g->N, kThreads, a,
                    step_lds_bytes(g->D, g->A, g->hidden, g->c_hidden), stream);
}

} // namespace

extern "C" gxu_status gxu_policy_step(const gxu_step_args* g, void* stream)
{
    return policy_step("gxu_policy_step", g, nullptr, false, stream);
}

extern "C" gxu_status guardx_usl_policy_step_episode(const gxu_step_args* g, const gx_first_done_state* book, void* stream)
{
    return policy_step("guardx_usl_policy_step_episode", g, book, true, stream);
}

extern "C" gxu_status guardx_usl_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                                     const float* d_c_params, const float* d_work, const float* d_rows, float* d_obs_last,
                                     float* d_val_last, void* stream)
{
    return q_tail_probe<StepKernel, StepArgs>(fail, "guardx_usl_tail_probe", n, D, A, hidden, c_hidden, d_params, d_c_params, d_work,
                                              d_rows, d_obs_last, d_val_last, stream);
}

extern "C" gxu_status gxu_correction_probe(int32_t n, int32_t D, int32_t A, int32_t c_hidden, const float* d_c_params,
                                           float* d_work, const float* d_obs, const float* d_act, float delta, int32_t niter,
                                           float eta, float grad_scale, float* d_a_safe, float* d_q0, float* d_grad0,
                                           int32_t* d_iters, int32_t* d_stop, void* stream)
{
    if (!d_c_params || !d_work || !d_obs || !d_act || !d_a_safe || !d_q0 || !d_grad0 || !d_iters || !d_stop)
        return fail(GXU_ERR_ARG, "gxu_correction_probe: null pointer");
    if (n < 0 || niter < 0) return fail(GXU_ERR_ARG, "gxu_correction_probe: n and niter must be >= 0");
    ProbeArgs a;
    a.n = n;
    a.q = q_args(D, A, true, delta, grad_scale, d_c_params, d_work);
    a.q.niter = niter; a.q.eta = eta;
    a.obs = d_obs; a.act = d_act;
    a.a_safe = d_a_safe; a.q0 = d_q0; a.grad0 = d_grad0; a.iters = d_iters; a.stop = d_stop;
    return q_probe_run<ProbeKernel>(fail, "gxu_correction_probe", n, D, A, c_hidden, d_c_params, d_work, a, stream);
}
