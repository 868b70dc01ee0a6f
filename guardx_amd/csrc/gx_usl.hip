// gx_usl.hip -- libguardx_usl.so (include/guardx_usl.h): `ac.step(o)` of the USL learner (safe_rl_libX/usl/usl.py:478-553,
// usl_core.py:146-196, 239-248) for one control step over all envs: the actor's mu_net and the critic v on the observation
// row, the cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) on the sampled action, and the learner's correction:
// up to niter passes of a = a - eta s / (max |s| + 1e-8), s the scaled gradient of Q with respect to the action.
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
#include "../../include/guardx_usl.h"
#include "gx_policy.h"
#include "gx_qcritic.h"
#include <hip/hip_runtime.h>
#include <string>

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

constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
bool shape_ok(int D, int A) { return D >= 1 && A >= 2 && A <= kMaxA && !(A & 1); }
int64_t params_floats(int D, int A, int H) { return net_floats(D, A, H) + net_floats(D, 1, H) + A; }
int64_t work_floats(int D, int H, int HC) { return 2 * wt_floats(D, H) + wt_floats(D, HC); }

// LDS of the step kernel: pi head | v head | X [16][pad4 D + 1] | outs [16][A + 1] | Q part | U, where U holds first
// the actor's and the critic's activations (H1, H2: [2][16][H + 4] each) and then, once mu and v are out, c_net's
// (H1, H2: [16][HC + 4] each)
struct Lds { int headP, headV, X, outs, U, total; QLds q; };
GX_HD Lds lds_layout(int D, int A, int H, int HC)
{
    Lds L;
    int o = 0;
    L.headP = o; o += pad4(mlp2_head_floats(A, H));
    L.headV = o; o += pad4(mlp2_head_floats(1, H));
    L.X = o; o += pad4(kEnv * (pad4(D) + 1));
    L.outs = o; o += pad4(kEnv * (A + 1));
    L.q = q_lds_layout(A, HC, o);
    o = L.q.total;
    L.U = o;
    const int upv = 4 * kEnv * (H + 4), uq = 2 * kEnv * (HC + 4);
    o += upv > uq ? upv : uq;
    L.total = o;
    return L;
}
// the probe kernel: X | Q part | H1, H2
GX_HD Lds probe_lds_layout(int D, int A, int HC)
{
    Lds L;
    int o = 0;
    L.headP = L.headV = L.outs = 0;
    L.X = o; o += pad4(kEnv * (pad4(D) + 1));
    L.q = q_lds_layout(A, HC, o);
    o = L.q.total;
    L.U = o; o += 2 * kEnv * (HC + 4);
    L.total = o;
    return L;
}

// the kernel's view of gxu_step_args: this step's row blocks resolved on the host
struct StepArgs {
    int N, env_offset;
    int tail, prologue;
    uint32_t seed0, seed1, tnoise;
    QArgs q;
    const float *params, *wt;
    const float* obs_rd;              // [N][D]
    const float *rew_in, *cost_in, *done_in;
    float *rew_p, *cost_p, *done_p;                                      // row block t - 1
    float *obs, *act, *act_safe, *mu, *logp, *val, *qc, *iters, *logstd; // row block t (tail: obs_last, val_last)
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

// The iteration of include/guardx_usl.h on the 16 rows of the workgroup.  On entry (after a barrier): the rows' actions in
// lds[L.act], P = the first layer's pre-activation over the observation columns, c_net's parts staged.  On exit (after a
// barrier): the final actions in lds[L.act]; the threads tid < 16 hold their row's result.  rows = valid rows;
// grad0 (may be null): [rows][A] in global memory.  Whole-workgroup call, every branch on pass state is uniform.
template <int HC>
GX_D RowOut q_iterate(float* lds, const QLds& L, float* H1, float* H2, const QArgs& q, int rows, float* grad0, int tid)
{
    constexpr int HS = HC + 4, TT = HC == 256 ? 2 : 1, LB = TT == 2 ? 4 : kLB;
    const int NW = q_waves(HC);
    const int wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int A = q.A, in = q.D + A;
    const float* hd = lds + L.head;
    const float* b2 = hd + HC;
    const float* w3 = hd + 2 * HC;
    float* P = lds + L.P;
    float* act = lds + L.act;
    float* gt = lds + L.gt;
    float* z3 = lds + L.z3;
    int* live = reinterpret_cast<int*>(lds + L.live);
    const float* gW2 = q.cp + (size_t)HC * in + HC;
    const float* Bf = HC == 64 ? lds + L.Wt2 : q.cwt + (size_t)pad4(q.D) * HC; // forward: [k][unit]
    const float* Bb = HC == 64 ? lds + L.W2 : gW2;                             // backward: [unit j][k]
    const int col0 = 16 * TT * wave;
    const int npass = q.correct ? q.niter : 0;

    // this lane's B operands of the action k-steps: W1[unit][D + 4 s + kq]
    float wa[kMaxA / 4][TT];
    if (wave < NW) {
#pragma unroll
        for (int s = 0; s < kMaxA / 4; ++s)
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                const int k = 4 * s + kq;
                wa[s][tt] = k < A ? q.cp[(size_t)(col0 + 16 * tt + c16) * in + q.D + k] : 0.0f;
            }
    }
    RowOut ro;
    ro.q0 = 0.0f; ro.iters = 0; ro.stop = tid < rows ? -1 : 3;

    for (int pass = 0;; ++pass) {
        // first layer: the A action terms on top of P, tanh
        if (wave < NW) {
            mfma_f4 acc[TT];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[tt][r] = P[(4 * kq + r) * HS + col0 + 16 * tt + c16];
#pragma unroll
            for (int s = 0; s < kMaxA / 4; ++s)
                if (4 * s < A) {
                    const float av = act[c16 * kAS + 4 * s + kq];
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wa[s][tt], acc[tt], 0, 0, 0);
                }
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) H1[(4 * kq + r) * HS + col0 + 16 * tt + c16] = tanh_f(acc[tt][r]);
        }
        wg_sync_lds();
        // second layer
        if (wave < NW) {
            mfma_f4 acc[TT];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) { const float bb = b2[col0 + 16 * tt + c16]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
            q_chain<TT, false, LB>(acc, Bf, HC, col0, H1, HS, w3, HC, c16, kq);
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) H2[(4 * kq + r) * HS + col0 + 16 * tt + c16] = tanh_f(acc[tt][r]);
        }
        wg_sync_lds();
        // the head (row e on the 16 lanes of tid = 16 e ..), and the backward GEMM, which does not wait for it
        if (tid < 16 * kEnv) {
            const int e = tid >> 4, l = tid & 15;
            const float z = hd[3 * HC] + dot16<HC>(w3, H2 + e * HS, l);
            if (l == 0) z3[e] = z;
        }
        if (npass > 0 && wave < NW) {
            mfma_f4 acc[TT];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = mfma_f4{0.0f, 0.0f, 0.0f, 0.0f};
            q_chain<TT, true, LB>(acc, Bb, HC, col0, H2, HS, w3, HC, c16, kq);
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { // g1 in place of h1: every element is read and written by its own lane alone
                    float* p = H1 + (4 * kq + r) * HS + col0 + 16 * tt + c16;
                    const float h = *p;
                    *p = __fmul_rn(__fsub_rn(1.0f, __fmul_rn(h, h)), acc[tt][r]);
                }
        }
        wg_sync_lds();
        // the A output sums: task (row e, component i) on 16 lanes
        if (npass > 0) {
            const int l = tid & 15;
            for (int task = tid >> 4; task < kEnv * A; task += kThreads / 16) {
                const int e = task / A, i = task - e * A;
                const float g = dot16<HC>(lds + L.W1a + i * HC, H1 + e * HS, l);
                if (l == 0) gt[e * kAS + i] = g;
            }
            wg_sync_lds();
        }
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
                    float Z = fabsf(__fmul_rn(c, g[0]));
                    for (int k = 1; k < A; ++k) { const float s = fabsf(__fmul_rn(c, g[k])); Z = s > Z ? s : Z; }
                    const float den = __fadd_rn(Z, 1e-8f);
                    for (int k = 0; k < A; ++k) {
                        const float s = __fmul_rn(c, g[k]);
                        if (pass == 0 && grad0) grad0[(size_t)tid * A + k] = s;
                        a[k] = __fsub_rn(a[k], __fmul_rn(q.eta, __fdiv_rn(s, den)));
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
    constexpr int HS = H + 4;
    extern __shared__ float4 usl_lds4[];
    float* lds = reinterpret_cast<float*>(usl_lds4);
    const int D = a.q.D, A = a.q.A, Dp = pad4(D), XS = Dp + 1, OS = A + 1;
    const Lds L = lds_layout(D, A, H, HC);
    float* X = lds + L.X;
    float* H1 = lds + L.U;
    float* H2 = H1 + 2 * kEnv * HS;
    float* outs = lds + L.outs;
    const int tid = threadIdx.x, wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int net = wave >> 2, quarter = wave & 3;
    const int env0 = blockIdx.x * kEnv;
    const int msz_pi = (int)net_floats(D, A, H), msz_v = (int)net_floats(D, 1, H);

    mlp2_head_stage(lds + L.headP, a.params, D, A, tid, kThreads, H);
    mlp2_head_stage(lds + L.headV, a.params + msz_pi, D, 1, tid, kThreads, H);
    if (!a.tail) q_stage<HC>(lds, L.q, a.q, tid);
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);

    // prologue: the copies of the step just made
    if (a.prologue && tid < kEnv) {
        const int env = env0 + tid;
        if (env < a.N) {
            a.rew_p[env] = a.rew_in[env];
            a.cost_p[env] = a.cost_in[env];
            a.done_p[env] = a.done_in[env];
        }
    }
    for (int i = tid; i < kEnv * XS; i += kThreads) {
        const int e = i / XS, k = i - e * XS;
        const int env = env0 + e;
        float x = 0.0f;
        if (k < D && env < a.N) {
            x = a.obs_rd[(size_t)env * D + k];
            a.obs[(size_t)env * D + k] = x;
        }
        X[i] = x;
    }
    wg_sync_lds(); // rows and heads

    const float* wtn = a.wt + (size_t)net * wt_floats(D, H); // (net 2 starts after the two H-wide networks)
    float* h1 = H1 + net * kEnv * HS;
    float* h2 = H2 + net * kEnv * HS;
    if (net < 2) {
        if (!(a.tail && net == 0)) // the bootstrap needs the critic only
            hidden_layer<H / 64, true>((net ? hv : hp).b1, wtn, H, (H / 4) * quarter, X, XS, Dp, h1, c16, kq);
    } else if (!a.tail)
        q_first_layer<HC>(lds + L.q.head, wtn, quarter, X, XS, Dp, lds + L.q.P, c16, kq);
    wg_sync_lds();
    if (net < 2 && !(a.tail && net == 0))
        hidden_layer<H / 64, true>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, (H / 4) * quarter, h1, HS, H, h2, c16, kq);
    wg_sync_lds();
    // output layers: task (env e, output o) on 16 lanes; o < A: mu_o, o == A: the value
    const int l = tid & 15;
    for (int task = tid >> 4; task < kEnv * OS; task += kThreads / 16) {
        const int e = task / OS, o = task - e * OS;
        if (a.tail && o != A) continue; // (16-lane groups take the branch together)
        const float y = o < A ? head2_out<H>(hp, o, l, H2 + e * HS) : head2_out<H>(hv, 0, l, H2 + (kEnv + e) * HS);
        if (l == 0) outs[e * OS + o] = y;
    }
    wg_sync_lds();
    // per env: the value, and (not in the tail) the noise, the action and log pi(a | o) of ac.step
    // (gx_policy_step.hip:policy_step_tail)
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            const float* oe = outs + e * OS;
            a.val[env] = oe[A];
            if (!a.tail) {
                float lp = 0.0f;
                for (int pr = 0; 2 * pr < A; ++pr) { // one counter per pair of action dimensions
                    float z[2];
                    normal_pair(a.seed0, a.seed1, (uint32_t)(a.env_offset + env), a.tnoise * 16u + (uint32_t)pr, z[0], z[1]);
                    for (int q = 0; q < 2; ++q) {
                        const int d = 2 * pr + q;
                        const float sd = exp_f(gls[d]);
                        const float lsd = log_f(sd);
                        const float m = oe[d];
                        const float act = fmaf(sd, z[q], m);
                        const float df = act - m;
                        const float var = sd * sd;
                        lp = lp + ((-(df * df) / (2.0f * var) - lsd) - 0.9189385332046727f);
                        a.act[(size_t)env * A + d] = act;
                        a.mu[(size_t)env * A + d] = m;
                        lds[L.q.act + e * kAS + d] = act;
                    }
                }
                a.logp[env] = lp;
            }
        }
    }
    if (a.tail) return;
    if (blockIdx.x == 0 && tid >= 64 && tid < 64 + A) a.logstd[tid - 64] = log_f(exp_f(gls[tid - 64]));
    wg_sync_lds(); // the actions; from here U is c_net's
    const int rows = a.N - env0 < kEnv ? a.N - env0 : kEnv;
    float* Q1 = lds + L.U;
    const RowOut ro = q_iterate<HC>(lds, L.q, Q1, Q1 + kEnv * (HC + 4), a.q, rows, nullptr, tid);
    if (tid < rows) {
        const int env = env0 + tid;
        a.qc[env] = ro.q0;
        a.iters[env] = (float)ro.iters;
        for (int d = 0; d < A; ++d) a.act_safe[(size_t)env * A + d] = lds[L.q.act + tid * kAS + d];
    }
}

template <int HC>
__global__ __launch_bounds__(kThreads) void usl_probe_kernel(ProbeArgs a)
{
    extern __shared__ float4 usl_lds4[];
    float* lds = reinterpret_cast<float*>(usl_lds4);
    const int D = a.q.D, A = a.q.A, Dp = pad4(D), XS = Dp + 1;
    const Lds L = probe_lds_layout(D, A, HC);
    float* X = lds + L.X;
    const int tid = threadIdx.x, wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int row0 = blockIdx.x * kEnv;
    const int rows = a.n - row0 < kEnv ? a.n - row0 : kEnv;
    q_stage<HC>(lds, L.q, a.q, tid);
    for (int i = tid; i < kEnv * XS; i += kThreads) {
        const int e = i / XS, k = i - e * XS;
        X[i] = (k < D && e < rows) ? a.obs[(size_t)(row0 + e) * D + k] : 0.0f;
    }
    wg_sync_lds(); // (q_stage zeroes the action rows)
    for (int i = tid; i < rows * A; i += kThreads) {
        const int e = i / A, k = i - e * A;
        lds[L.q.act + e * kAS + k] = a.act[(size_t)(row0 + e) * A + k];
    }
    if (wave >= 8) q_first_layer<HC>(lds + L.q.head, a.q.cwt, wave & 3, X, XS, Dp, lds + L.q.P, c16, kq);
    wg_sync_lds();
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

template <int H, int HC>
const void* kernel_of() { return reinterpret_cast<const void*>(usl_step_kernel<H, HC>); }

template <int H>
const void* kernel_of_hc(int HC)
{
    switch (HC) {
    case 64: return kernel_of<H, 64>();
    case 128: return kernel_of<H, 128>();
    case 192: return kernel_of<H, 192>();
    default: return kernel_of<H, 256>();
    }
}

const void* kernel_for(int H, int HC)
{
    switch (H) {
    case 64: return kernel_of_hc<64>(HC);
    case 128: return kernel_of_hc<128>(HC);
    case 192: return kernel_of_hc<192>(HC);
    default: return kernel_of_hc<256>(HC);
    }
}

const void* probe_kernel_for(int HC)
{
    switch (HC) {
    case 64: return reinterpret_cast<const void*>(usl_probe_kernel<64>);
    case 128: return reinterpret_cast<const void*>(usl_probe_kernel<128>);
    case 192: return reinterpret_cast<const void*>(usl_probe_kernel<192>);
    default: return reinterpret_cast<const void*>(usl_probe_kernel<256>);
    }
}

gxu_status check_shape(const char* who, int D, int A, int H, int HC, bool probe)
{
    if (D < 1 || A < 1) return fail(GXU_ERR_ARG, std::string(who) + ": D and A must be >= 1");
    if (!width_ok(H) || !width_ok(HC))
        return fail(GXU_ERR_UNSUPPORTED, std::string(who) + ": hidden width not in {64, 128, 192, 256}");
    if (!shape_ok(D, A)) return fail(GXU_ERR_UNSUPPORTED, std::string(who) + ": needs an even action width <= 16");
    if (D > 65536 || sizeof(float) * (size_t)(probe ? probe_lds_layout(D, A, HC) : lds_layout(D, A, H, HC)).total > kLdsMax)
        return fail(GXU_ERR_UNSUPPORTED, std::string(who) + ": D too wide for the LDS tile");
    return GXU_OK;
}

gxu_status raise_lds(const char* who, const void* kernel, size_t lds)
{
    if (lds > 64 * 1024) { // more dynamic LDS than the default cap: raise it for this kernel (on the current device)
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(GXU_ERR_HIP, std::string(who) + ": hipFuncSetAttribute failed");
    }
    return GXU_OK;
}

} // namespace

extern "C" const char* gxu_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxu_build_id(void) { return GXU_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["usl"].source_hash()

extern "C" int64_t gxu_params_floats(int32_t D, int32_t A, int32_t hidden)
{
    return (shape_ok(D, A) && width_ok(hidden)) ? params_floats(D, A, hidden) : -1;
}

extern "C" int64_t gxu_q_floats(int32_t D, int32_t A, int32_t c_hidden)
{
    return (shape_ok(D, A) && width_ok(c_hidden)) ? net_floats(D + A, 1, c_hidden) : -1;
}

extern "C" int64_t gxu_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden)
{
    return (shape_ok(D, A) && width_ok(hidden) && width_ok(c_hidden)) ? work_floats(D, hidden, c_hidden) : -1;
}

extern "C" int64_t gxu_probe_work_floats(int32_t D, int32_t A, int32_t c_hidden)
{
    return (shape_ok(D, A) && width_ok(c_hidden)) ? wt_floats(D, c_hidden) : -1;
}

extern "C" gxu_status gxu_prepare(int32_t D, int32_t A, int32_t hidden, int32_t c_hidden, const float* d_params,
                                  const float* d_c_params, float* d_work, void* stream)
{
    if (!d_params || !d_c_params || !d_work) return fail(GXU_ERR_ARG, "gxu_prepare: null pointer");
    gxu_status st = check_shape("gxu_prepare", D, A, hidden, c_hidden, false);
    if (st != GXU_OK) return st;
    st = raise_lds("gxu_prepare", kernel_for(hidden, c_hidden), sizeof(float) * (size_t)lds_layout(D, A, hidden, c_hidden).total);
    if (st != GXU_OK) return st;
    const long long n = work_floats(D, hidden, c_hidden);
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(usl_transpose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_params, d_c_params, d_work,
                       D, A, hidden, c_hidden, 0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXU_OK : fail(GXU_ERR_HIP, std::string("gxu_prepare launch failed: ") + hipGetErrorString(e));
}

extern "C" gxu_status gxu_policy_step(const gxu_step_args* g, void* stream)
{
    if (!g) return fail(GXU_ERR_ARG, "gxu_policy_step: null argument struct");
    if (g->struct_size != sizeof(gxu_step_args)) return fail(GXU_ERR_ARG, "gxu_policy_step: struct_size mismatch");
    if (g->N < 0 || g->T < 1 || g->t < 0 || g->t > g->T || g->env_offset < 0 || g->niter < 0)
        return fail(GXU_ERR_ARG, "gxu_policy_step: N must be >= 0, T >= 1, t in [0, T], env_offset >= 0, niter >= 0");
    const gxu_status st = check_shape("gxu_policy_step", g->D, g->A, g->hidden, g->c_hidden, false);
    if (st != GXU_OK) return st;
    const bool tail = g->t == g->T, prologue = g->t > 0;
    if (!g->d_params || !g->d_c_params || !g->d_work) return fail(GXU_ERR_ARG, "gxu_policy_step: null pointer");
    if (prologue ? (!g->d_obs_rd || !g->d_rew_in || !g->d_cost_in || !g->d_done_in || !g->d_rew || !g->d_cost || !g->d_done)
                 : !g->d_obs0)
        return fail(GXU_ERR_ARG, "gxu_policy_step: null pointer");
    if (tail ? (!g->d_obs_last || !g->d_val_last)
             : (!g->d_obs || !g->d_act || !g->d_act_safe || !g->d_mu || !g->d_logp || !g->d_val || !g->d_qc || !g->d_iters ||
                !g->d_logstd))
        return fail(GXU_ERR_ARG, "gxu_policy_step: null pointer");
    if (g->N == 0) return GXU_OK;
    const size_t N = (size_t)g->N, D = (size_t)g->D, A = (size_t)g->A;
    StepArgs a;
    a.N = g->N; a.env_offset = g->env_offset;
    a.tail = tail; a.prologue = prologue;
    a.seed0 = g->seed[0]; a.seed1 = g->seed[1]; a.tnoise = g->step0 + (uint32_t)g->t;
    a.q.D = g->D; a.q.A = g->A; a.q.niter = g->niter; a.q.correct = g->correct != 0;
    a.q.delta = g->delta; a.q.eta = g->eta; a.q.gscale = g->grad_scale;
    a.q.cp = g->d_c_params; a.q.cwt = g->d_work + 2 * wt_floats(g->D, g->hidden);
    a.params = g->d_params; a.wt = g->d_work;
    a.obs_rd = prologue ? g->d_obs_rd : g->d_obs0;
    a.rew_in = g->d_rew_in; a.cost_in = g->d_cost_in; a.done_in = g->d_done_in;
    const size_t tp = prologue ? (size_t)(g->t - 1) * N : 0;
    a.rew_p = prologue ? g->d_rew + tp : nullptr; a.cost_p = prologue ? g->d_cost + tp : nullptr;
    a.done_p = prologue ? g->d_done + tp : nullptr;
    const size_t tn = (size_t)g->t * N;
    if (tail) {
        a.obs = g->d_obs_last; a.val = g->d_val_last;
        a.act = a.act_safe = a.mu = a.logp = a.qc = a.iters = a.logstd = nullptr;
    } else {
        a.obs = g->d_obs + tn * D; a.act = g->d_act + tn * A; a.act_safe = g->d_act_safe + tn * A;
        a.mu = g->d_mu + tn * A; a.logp = g->d_logp + tn; a.val = g->d_val + tn;
        a.qc = g->d_qc + tn; a.iters = g->d_iters + tn; a.logstd = g->d_logstd;
    }
    const size_t lds = sizeof(float) * (size_t)lds_layout(g->D, g->A, g->hidden, g->c_hidden).total;
    const dim3 grid((unsigned)((g->N + kEnv - 1) / kEnv));
    void* kargs[] = {&a};
    const hipError_t e = hipLaunchKernel(kernel_for(g->hidden, g->c_hidden), grid, dim3(kThreads), kargs, lds, (hipStream_t)stream);
    return e == hipSuccess ? GXU_OK : fail(GXU_ERR_HIP, std::string("gxu_policy_step launch failed: ") + hipGetErrorString(e));
}

extern "C" gxu_status gxu_correction_probe(int32_t n, int32_t D, int32_t A, int32_t c_hidden, const float* d_c_params,
                                           float* d_work, const float* d_obs, const float* d_act, float delta, int32_t niter,
                                           float eta, float grad_scale, float* d_a_safe, float* d_q0, float* d_grad0,
                                           int32_t* d_iters, int32_t* d_stop, void* stream)
{
    if (!d_c_params || !d_work || !d_obs || !d_act || !d_a_safe || !d_q0 || !d_grad0 || !d_iters || !d_stop)
        return fail(GXU_ERR_ARG, "gxu_correction_probe: null pointer");
    if (n < 0 || niter < 0) return fail(GXU_ERR_ARG, "gxu_correction_probe: n and niter must be >= 0");
    gxu_status st = check_shape("gxu_correction_probe", D, A, 64, c_hidden, true);
    if (st != GXU_OK) return st;
    if (n == 0) return GXU_OK;
    const size_t lds = sizeof(float) * (size_t)probe_lds_layout(D, A, c_hidden).total;
    st = raise_lds("gxu_correction_probe", probe_kernel_for(c_hidden), lds);
    if (st != GXU_OK) return st;
    const long long nw = wt_floats(D, c_hidden);
    const unsigned blocks = (unsigned)std::min<long long>((nw + 255) / 256, 1024);
    hipLaunchKernelGGL(usl_transpose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_c_params, d_c_params, d_work,
                       D, A, c_hidden, c_hidden, 2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GXU_ERR_HIP, std::string("gxu_correction_probe launch failed: ") + hipGetErrorString(e));
    ProbeArgs a;
    a.n = n;
    a.q.D = D; a.q.A = A; a.q.niter = niter; a.q.correct = 1;
    a.q.delta = delta; a.q.eta = eta; a.q.gscale = grad_scale;
    a.q.cp = d_c_params; a.q.cwt = d_work;
    a.obs = d_obs; a.act = d_act;
    a.a_safe = d_a_safe; a.q0 = d_q0; a.grad0 = d_grad0; a.iters = d_iters; a.stop = d_stop;
    void* kargs[] = {&a};
    e = hipLaunchKernel(probe_kernel_for(c_hidden), dim3((unsigned)((n + kEnv - 1) / kEnv)), dim3(kThreads), kargs, lds,
                        (hipStream_t)stream);
    return e == hipSuccess ? GXU_OK : fail(GXU_ERR_HIP, std::string("gxu_correction_probe launch failed: ") + hipGetErrorString(e));
}
