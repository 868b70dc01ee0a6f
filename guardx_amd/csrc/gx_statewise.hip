// gx_statewise.hip -- libguardx_statewise.so (include/guardx_statewise.h): `ac.step(o_aug)` of the state-wise learners
// (SCPO: safe_rl_libX/scpo/scpo.py:640-720, scpo_core.py:158-200) for one control step over all envs, with the update of
// the running maximum cost M of the step just made in front of it.  o_aug = [obs | M] is D + 1 wide and feeds three
// two-hidden-layer tanh networks: the actor's mu_net, the critic v and the cost critic vc with its Softplus output.
//
// The arithmetic is the fused rollout's (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward): every hidden
// unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias (that instruction accumulates exactly
// like a sequential fmaf chain, tools/probes/mfma_f32_probe.hip), then tanh_f; an output is 16 lane partials over the
// units 64 c + 4 l + j folded by the butterfly of head2_out; the noise, the action and log pi(a | o) are those of
// gx_policy_step.hip:policy_step_tail.  With a zero weight on the M column the actor and v therefore give the bits of
// rollout_policy on the D-wide observation.
//
// Organisation: a 384-thread workgroup (6 waves) serves 16 envs from ONE staged copy of their rows.  Waves 2 n and
// 2 n + 1 own network n (0 actor, 1 v, 2 vc) and one half of its hidden units each (H / 32 output tiles of 16 units per
// wave: the streaming form of gx_policy.h, polS_chain / polS_store).  The B operands are the hidden layers transposed
// to [k][unit] (gxs_prepare, into the caller's workspace, once per call): read by every workgroup, resident in L2,
// fetched eight k-steps ahead of the MFMAs that consume them.  The A operands (the augmented rows zero-padded to a
// multiple of four, then the first hidden layer) come from LDS.  At env_num = 2000 this is 125 workgroups on 256 CUs:
// the launch is bound by latency, not by throughput, which is why all three networks run side by side in one launch.
#include "../../include/guardx_statewise.h"
#include "gx_policy.h"
#include <hip/hip_runtime.h>
#include <string>

#ifndef GXS_BUILD_ID
#define GXS_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxs_status fail(gxs_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kEnv = 16;       // envs per workgroup
constexpr int kThreads = 384;  // 6 waves: two per network
constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
bool shape_ok(int Da, int A) { return Da >= 2 && A >= 2 && A <= 16 && !(A & 1); }
GX_HD int64_t net_floats(int D, int Out, int H) { return (int64_t)H * D + H + (int64_t)H * H + H + (int64_t)Out * H + Out; }
int64_t params_floats(int Da, int A, int H) { return net_floats(Da, A, H) + net_floats(Da, 1, H) + A; }
GX_HD int64_t wt_floats(int Da, int H) { return (int64_t)pad4(Da) * H + (int64_t)H * H; }
int64_t work_floats(int Da, int H, int HC) { return 2 * wt_floats(Da, H) + wt_floats(Da, HC); }

// LDS, in floats: pi head | v head | vc head (b1 b2 W3 b3 each) | X [16][pad4 Da + 1] | H1 pi, v [16][H + 4], vc [16][HC + 4] |
// H2 likewise | outs [16][A + 2]
struct Lds { int headP, headV, headC, X, H1, H2, outs, total; };
GX_HD Lds lds_layout(int Da, int A, int H, int HC)
{
    Lds L;
    int o = 0;
    L.headP = o; o += pad4(mlp2_head_floats(A, H));
    L.headV = o; o += pad4(mlp2_head_floats(1, H));
    L.headC = o; o += pad4(mlp2_head_floats(1, HC));
    L.X = o; o += pad4(kEnv * (pad4(Da) + 1));
    const int hid = kEnv * (2 * (H + 4) + (HC + 4));
    L.H1 = o; o += hid;
    L.H2 = o; o += hid;
    L.outs = o; o += pad4(kEnv * (A + 2));
    L.total = o;
    return L;
}

// Softplus as torch evaluates it (beta = 1, threshold = 20): x > 20 ? x : log1p(exp(x)), in the form that neither
// overflows nor loses the small tail: max(x, 0) + log1p(exp(-|x|)).  log1p(u) for u = exp(-|x|) in [0, 1] through the
// project's log: w = fl(1 + u); log(w) u / (w - 1) (w - 1 is exact; the quotient takes back the rounding of 1 + u), and u
// itself once 1 + u rounds to 1.  A NaN comes out as a NaN.
GX_D float softplus_f(float x)
{
    if (x > 20.0f) return x;
    const float u = exp_f(-fabsf(x));
    const float w = 1.0f + u;
    const float l1p = (w == 1.0f) ? u : log_f(w) * (u / (w - 1.0f));
    return (x > 0.0f ? x : 0.0f) + l1p;
}

__global__ void softplus_probe_kernel(int n, const float* __restrict__ x, float* __restrict__ y)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = softplus_f(x[i]);
}

// wt = [pi Wt1 | pi Wt2 | v Wt1 | v Wt2 | vc Wt1 | vc Wt2]; Wt1 [pad4 Da][h] (rows Da .. zero), Wt2 [h][h], from the torch
// layout W1 [h][Da] b1 W2 [h][h] ...
__global__ void statewise_transpose_kernel(const float* __restrict__ params, const float* __restrict__ vcp,
                                           float* __restrict__ wt, int Da, int A, int H, int HC)
{
    const int Dp = pad4(Da);
    const long long per = (long long)Dp * H + (long long)H * H, perc = (long long)Dp * HC + (long long)HC * HC;
    const long long n = 2 * per + perc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int net = i < per ? 0 : (i < 2 * per ? 1 : 2);
        const long long r = i - (long long)net * per;
        const int h = net == 2 ? HC : H;
        const float* g = net == 0 ? params : (net == 1 ? params + net_floats(Da, A, H) : vcp);
        const long long n1 = (long long)Dp * h;
        if (r < n1) {
            const int k = (int)(r / h), j = (int)(r - (long long)k * h);
            wt[i] = k < Da ? g[(size_t)j * Da + k] : 0.0f;
        } else {
            const long long r2 = r - n1;
            const int k = (int)(r2 / h), j = (int)(r2 - (long long)k * h);
            wt[i] = g[(size_t)h * Da + h + (size_t)j * h + k];
        }
    }
}

// the kernel's view of gxs_step_args: this step's row blocks resolved on the host
struct StepArgs {
    int N, D, Da, A, env_offset;      // D = Da - 1: the width of the env's own observation
    int tail, prologue;
    uint32_t seed0, seed1, tnoise;
    const float *params, *vcp, *wt;
    const float* obs_rd;              // [N][D]
    const float *rew_in, *cost_in, *done_in;
    float *M, *first;
    float *rew_p, *cost_p, *done_p, *cost_inc_p, *M_after_p;  // row block t - 1
    float *obs, *act, *mu, *logp, *val, *vc, *logstd;         // row block t (tail: obs_last, val_last, vc_last)
};

// one hidden layer of this wave's tiles: acc = bias, chain over k ascending, tanh into the activation rows
template <int TT>
GX_D void hidden_layer(const float* bias, const float* __restrict__ wt, int Hn, int col0, const float* Ain, int AS, int K,
                       float* out, int c16, int kq)
{
    mfma_f4 acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) { const float bb = bias[col0 + TT * c16 + tt]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
    polS_chain<TT>(acc, wt, Hn, col0, Ain, AS, K, c16, kq);
    polS_store<TT>(acc, out + col0, Hn + 4, c16, kq);
}

template <int H, int HC>
__global__ __launch_bounds__(kThreads) void statewise_step_kernel(StepArgs a)
{
    constexpr int HS = H + 4, HSC = HC + 4;
    extern __shared__ float4 sw_lds4[];
    float* lds = reinterpret_cast<float*>(sw_lds4);
    const int D = a.D, Da = a.Da, A = a.A, Dp = pad4(Da), XS = Dp + 1;
    const Lds L = lds_layout(Da, A, H, HC);
    float* X = lds + L.X;
    float* H1 = lds + L.H1;
    float* H2 = lds + L.H2;
    float* outs = lds + L.outs;
    const int tid = threadIdx.x, wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int net = wave >> 1, half = wave & 1;
    const int env0 = blockIdx.x * kEnv;
    const int msz_pi = (int)net_floats(Da, A, H), msz_v = (int)net_floats(Da, 1, H);

    mlp2_head_stage(lds + L.headP, a.params, Da, A, tid, kThreads, H);
    mlp2_head_stage(lds + L.headV, a.params + msz_pi, Da, 1, tid, kThreads, H);
    mlp2_head_stage(lds + L.headC, a.vcp, Da, 1, tid, kThreads, HC);
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);
    const Mlp2Head hc = mlp2_head_view(lds + L.headC, 1, HC);

    // prologue: the M update of the step just made (scpo.py:644-654, 713-715), then M as column D of the row
    if (tid < kEnv) {
        const int env = env0 + tid;
        float M = 0.0f;
        if (env < a.N) {
            M = a.M[env];
            if (a.prologue) {
                const bool first = a.first[env] != 0.0f;
                const float cost = a.cost_in[env], done = a.done_in[env];
                const float d = cost - M;
                const float inc = first ? cost : (d > 0.0f ? d : 0.0f);
                const float Mn = first ? cost : M + inc;
                a.cost_inc_p[env] = inc;
                a.M_after_p[env] = Mn;
                a.rew_p[env] = a.rew_in[env];
                a.cost_p[env] = cost;
                a.done_p[env] = done;
                const bool fin = done > 0.0f;
                M = fin ? 0.0f : Mn;
                a.M[env] = M;
                a.first[env] = fin ? 1.0f : 0.0f;
            }
            a.obs[(size_t)env * Da + D] = M;
        }
        X[tid * XS + D] = M;
    }
    for (int i = tid; i < kEnv * XS; i += kThreads) {
        const int e = i / XS, k = i - e * XS;
        if (k == D) continue; // the prologue's
        const int env = env0 + e;
        float x = 0.0f;
        if (k < D && env < a.N) {
            x = a.obs_rd[(size_t)env * D + k];
            a.obs[(size_t)env * Da + k] = x;
        }
        X[i] = x;
    }
    wg_sync_lds(); // rows and heads

    const bool skip = a.tail && net == 0; // the bootstrap needs the critics only
    const float* wtn = a.wt + (size_t)net * wt_floats(Da, H); // (net 2 starts after the two H-wide networks)
    float* h1 = H1 + (net < 2 ? net * kEnv * HS : 2 * kEnv * HS);
    float* h2 = H2 + (net < 2 ? net * kEnv * HS : 2 * kEnv * HS);
    if (!skip) {
        if (net < 2) hidden_layer<H / 32>((net ? hv : hp).b1, wtn, H, 16 * (H / 32) * half, X, XS, Dp, h1, c16, kq);
        else hidden_layer<HC / 32>(hc.b1, wtn, HC, 16 * (HC / 32) * half, X, XS, Dp, h1, c16, kq);
    }
    wg_sync_lds();
    if (!skip) {
        if (net < 2) hidden_layer<H / 32>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, 16 * (H / 32) * half, h1, HS, H, h2, c16, kq);
        else hidden_layer<HC / 32>(hc.b2, wtn + (size_t)Dp * HC, HC, 16 * (HC / 32) * half, h1, HSC, HC, h2, c16, kq);
    }
    wg_sync_lds();
    // output layers: task (env e, output o) on 16 lanes; o < A: mu_o, o == A: the value, o == A + 1: vc before its Softplus
    const int l = tid & 15;
    for (int task = tid >> 4; task < kEnv * (A + 2); task += kThreads / 16) {
        const int e = task / (A + 2), o = task - e * (A + 2);
        if (a.tail && o < A) continue; // (16-lane groups take the branch together)
        float y;
        if (o < A) y = head2_out<H>(hp, o, l, H2 + e * HS);
        else if (o == A) y = head2_out<H>(hv, 0, l, H2 + (kEnv + e) * HS);
        else y = head2_out<HC>(hc, 0, l, H2 + 2 * kEnv * HS + e * HSC);
        if (l == 0) outs[e * (A + 2) + o] = y;
    }
    wg_sync_lds();
    // per env: the values, and (not in the tail) the noise, the action and log pi(a | o) of ac.step
    // (gx_policy_step.hip:policy_step_tail, scpo_core.py:189-198)
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            a.val[env] = outs[e * (A + 2) + A];
            a.vc[env] = softplus_f(outs[e * (A + 2) + A + 1]);
            if (!a.tail) {
                float lp = 0.0f;
                for (int pr = 0; 2 * pr < A; ++pr) { // one counter per pair of action dimensions
                    float z[2];
                    normal_pair(a.seed0, a.seed1, (uint32_t)(a.env_offset + env), a.tnoise * 16u + (uint32_t)pr, z[0], z[1]);
                    for (int q = 0; q < 2; ++q) {
                        const int d = 2 * pr + q;
                        const float sd = exp_f(gls[d]);
                        const float lsd = log_f(sd);
                        const float m = outs[e * (A + 2) + d];
                        const float act = fmaf(sd, z[q], m);
                        const float df = act - m;
                        const float var = sd * sd;
                        lp = lp + ((-(df * df) / (2.0f * var) - lsd) - 0.9189385332046727f);
                        a.act[(size_t)env * A + d] = act;
                        a.mu[(size_t)env * A + d] = m;
                    }
                }
                a.logp[env] = lp;
            }
        }
    }
    if (!a.tail && blockIdx.x == 0 && tid >= 64 && tid < 64 + A) a.logstd[tid - 64] = log_f(exp_f(gls[tid - 64]));
}

template <int H, int HC>
const void* kernel_of() { return reinterpret_cast<const void*>(statewise_step_kernel<H, HC>); }

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

gxs_status check_shape(const char* who, int Da, int A, int H, int HC)
{
    if (Da < 2 || A < 1) return fail(GXS_ERR_ARG, std::string(who) + ": D_aug must be >= 2 and A >= 1");
    if (!width_ok(H) || !width_ok(HC))
        return fail(GXS_ERR_UNSUPPORTED, std::string(who) + ": hidden width not in {64, 128, 192, 256}");
    if (!shape_ok(Da, A)) return fail(GXS_ERR_UNSUPPORTED, std::string(who) + ": needs an even action width <= 16");
    if (sizeof(float) * (size_t)lds_layout(Da, A, H, HC).total > kLdsMax)
        return fail(GXS_ERR_UNSUPPORTED, std::string(who) + ": D_aug too wide for the LDS tile");
    return GXS_OK;
}

} // namespace

extern "C" const char* gxs_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxs_build_id(void) { return GXS_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["statewise"].source_hash()

extern "C" int64_t gxs_params_floats(int32_t D_aug, int32_t A, int32_t hidden)
{
    return (shape_ok(D_aug, A) && width_ok(hidden)) ? params_floats(D_aug, A, hidden) : -1;
}

extern "C" int64_t gxs_work_floats(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden)
{
    return (shape_ok(D_aug, A) && width_ok(hidden) && width_ok(vc_hidden)) ? work_floats(D_aug, hidden, vc_hidden) : -1;
}

extern "C" gxs_status gxs_prepare(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden, const float* d_params,
                                  const float* d_vc_params, float* d_work, void* stream)
{
    if (!d_params || !d_vc_params || !d_work) return fail(GXS_ERR_ARG, "gxs_prepare: null pointer");
    const gxs_status st = check_shape("gxs_prepare", D_aug, A, hidden, vc_hidden);
    if (st != GXS_OK) return st;
    const size_t lds = sizeof(float) * (size_t)lds_layout(D_aug, A, hidden, vc_hidden).total;
    if (lds > 64 * 1024) { // more dynamic LDS than the default cap: raise it for this kernel (on the current device)
        if (hipFuncSetAttribute(kernel_for(hidden, vc_hidden), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(GXS_ERR_HIP, "gxs_prepare: hipFuncSetAttribute failed");
    }
    const long long n = work_floats(D_aug, hidden, vc_hidden);
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(statewise_transpose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_params, d_vc_params,
                       d_work, D_aug, A, hidden, vc_hidden);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXS_OK : fail(GXS_ERR_HIP, std::string("gxs_prepare launch failed: ") + hipGetErrorString(e));
}

extern "C" gxs_status gxs_policy_step(const gxs_step_args* g, void* stream)
{
    if (!g) return fail(GXS_ERR_ARG, "gxs_policy_step: null argument struct");
    if (g->struct_size != sizeof(gxs_step_args)) return fail(GXS_ERR_ARG, "gxs_policy_step: struct_size mismatch");
    if (g->N < 0 || g->T < 1 || g->t < 0 || g->t > g->T || g->env_offset < 0)
        return fail(GXS_ERR_ARG, "gxs_policy_step: N must be >= 0, T >= 1, t in [0, T], env_offset >= 0");
    const gxs_status st = check_shape("gxs_policy_step", g->D_aug, g->A, g->hidden, g->vc_hidden);
    if (st != GXS_OK) return st;
    const bool tail = g->t == g->T, prologue = g->t > 0;
    if (!g->d_params || !g->d_vc_params || !g->d_work || !g->d_M || !g->d_first)
        return fail(GXS_ERR_ARG, "gxs_policy_step: null pointer");
    if (prologue ? (!g->d_obs_rd || !g->d_rew_in || !g->d_cost_in || !g->d_done_in || !g->d_rew || !g->d_cost ||
                    !g->d_done || !g->d_cost_inc || !g->d_M_after)
                 : !g->d_obs0)
        return fail(GXS_ERR_ARG, "gxs_policy_step: null pointer");
    if (tail ? (!g->d_obs_last || !g->d_val_last || !g->d_vc_last)
             : (!g->d_obs || !g->d_act || !g->d_mu || !g->d_logp || !g->d_val || !g->d_vc || !g->d_logstd))
        return fail(GXS_ERR_ARG, "gxs_policy_step: null pointer");
    if (g->N == 0) return GXS_OK;
    const size_t N = (size_t)g->N, Da = (size_t)g->D_aug, A = (size_t)g->A;
    StepArgs a;
    a.N = g->N; a.Da = g->D_aug; a.D = g->D_aug - 1; a.A = g->A; a.env_offset = g->env_offset;
    a.tail = tail; a.prologue = prologue;
    a.seed0 = g->seed[0]; a.seed1 = g->seed[1]; a.tnoise = g->step0 + (uint32_t)g->t;
    a.params = g->d_params; a.vcp = g->d_vc_params; a.wt = g->d_work;
    a.obs_rd = prologue ? g->d_obs_rd : g->d_obs0;
    a.rew_in = g->d_rew_in; a.cost_in = g->d_cost_in; a.done_in = g->d_done_in;
    a.M = g->d_M; a.first = g->d_first;
    const size_t tp = prologue ? (size_t)(g->t - 1) * N : 0;
    a.rew_p = prologue ? g->d_rew + tp : nullptr; a.cost_p = prologue ? g->d_cost + tp : nullptr;
    a.done_p = prologue ? g->d_done + tp : nullptr; a.cost_inc_p = prologue ? g->d_cost_inc + tp : nullptr;
    a.M_after_p = prologue ? g->d_M_after + tp : nullptr;
    const size_t tn = (size_t)g->t * N;
    if (tail) {
        a.obs = g->d_obs_last; a.val = g->d_val_last; a.vc = g->d_vc_last;
        a.act = a.mu = a.logp = a.logstd = nullptr;
    } else {
        a.obs = g->d_obs + tn * Da; a.act = g->d_act + tn * A; a.mu = g->d_mu + tn * A; a.logp = g->d_logp + tn;
        a.val = g->d_val + tn; a.vc = g->d_vc + tn; a.logstd = g->d_logstd;
    }
    const size_t lds = sizeof(float) * (size_t)lds_layout(g->D_aug, g->A, g->hidden, g->vc_hidden).total;
    const dim3 grid((unsigned)((g->N + kEnv - 1) / kEnv));
    void* kargs[] = {&a};
    const hipError_t e = hipLaunchKernel(kernel_for(g->hidden, g->vc_hidden), grid, dim3(kThreads), kargs, lds, (hipStream_t)stream);
    return e == hipSuccess ? GXS_OK : fail(GXS_ERR_HIP, std::string("gxs_policy_step launch failed: ") + hipGetErrorString(e));
}

extern "C" gxs_status gxs_softplus_probe(int32_t n, const float* d_x, float* d_y, void* stream)
{
    if (!d_x || !d_y) return fail(GXS_ERR_ARG, "gxs_softplus_probe: null pointer");
    if (n < 0) return fail(GXS_ERR_ARG, "gxs_softplus_probe: n must be >= 0");
    if (n == 0) return GXS_OK;
    const unsigned blocks = (unsigned)std::min<long long>(((long long)n + 255) / 256, 4096);
    hipLaunchKernelGGL(softplus_probe_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, d_x, d_y);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXS_OK : fail(GXS_ERR_HIP, std::string("gxs_softplus_probe launch failed: ") + hipGetErrorString(e));
}
