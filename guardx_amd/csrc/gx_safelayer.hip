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
// gx_policy_step.hip:policy_step_tail.  The actor and v therefore give the bits of rollout_policy.  The correction's
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
#include "../../include/guardx_safelayer.h"
#include "gx_policy.h"
#include <hip/hip_runtime.h>
#include <string>

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

constexpr int kEnv = 16;       // envs per workgroup
constexpr int kThreads = 768;  // 12 waves: four per network
constexpr int kMaxA = 16;
constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
bool shape_ok(int D, int A) { return D >= 1 && A >= 2 && A <= kMaxA && !(A & 1); }
GX_HD int64_t net_floats(int D, int Out, int H) { return (int64_t)H * D + H + (int64_t)H * H + H + (int64_t)Out * H + Out; }
int64_t params_floats(int D, int A, int H) { return net_floats(D, A, H) + net_floats(D, 1, H) + A; }
GX_HD int64_t wt_floats(int D, int H) { return (int64_t)pad4(D) * H + (int64_t)H * H; }
int64_t work_floats(int D, int H, int HG) { return 2 * wt_floats(D, H) + wt_floats(D, HG); }

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

// wt = [pi Wt1 | pi Wt2 | v Wt1 | v Wt2 | g Wt1 | g Wt2]; Wt1 [pad4 D][h] (rows D .. zero), Wt2 [h][h], from the torch
// layout W1 [h][D] b1 W2 [h][h] ...
__global__ void safelayer_transpose_kernel(const float* __restrict__ params, const float* __restrict__ gp,
                                           float* __restrict__ wt, int D, int A, int H, int HG)
{
    const int Dp = pad4(D);
    const long long per = (long long)Dp * H + (long long)H * H, perg = (long long)Dp * HG + (long long)HG * HG;
    const long long n = 2 * per + perg;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int net = i < per ? 0 : (i < 2 * per ? 1 : 2);
        const long long r = i - (long long)net * per;
        const int h = net == 2 ? HG : H;
        const float* g = net == 0 ? params : (net == 1 ? params + net_floats(D, A, H) : gp);
        const long long n1 = (long long)Dp * h;
        if (r < n1) {
            const int k = (int)(r / h), j = (int)(r - (long long)k * h);
            wt[i] = k < D ? g[(size_t)j * D + k] : 0.0f;
        } else {
            const long long r2 = r - n1;
            const int k = (int)(r2 / h), j = (int)(r2 - (long long)k * h);
            wt[i] = g[(size_t)h * D + h + (size_t)j * h + k];
        }
    }
}

// the kernel's view of gxl_step_args: this step's row blocks resolved on the host
struct StepArgs {
    int N, D, A, env_offset;
    int tail, prologue, correct;
    uint32_t seed0, seed1, tnoise;
    float delta;
    const float *params, *gp, *wt;
    const float* obs_rd;              // [N][D]
    const float *rew_in, *cost_in, *done_in;
    float* prev_c;
    float *rew_p, *cost_p, *done_p;                                       // row block t - 1
    float *obs, *act, *act_safe, *mu, *g, *logp, *val, *prev_cost, *logstd; // row block t (tail: obs_last, val_last)
};

// acc[tile] += A[16 envs][K] * Wt[K][16 units of the tile], k ascending (the order of the fmaf chain); tile tt holds the
// units col0 + 16 tt + c16.  The operands of kLB k-steps are fetched together and one block AHEAD of the MFMAs that
// consume them (two register sets, the loop advances by two blocks).
constexpr int kLB = 8;
template <int TT>
GX_D void sl_fetch(float (&av)[kLB], float (&bv)[kLB][TT], const float* ap, const float* bp, int Hn, int s0, int ns)
{
#pragma unroll
    for (int i = 0; i < kLB; ++i) {
        const int sidx = s0 + i;
        if (sidx < ns) { // wave-uniform
            av[i] = ap[4 * sidx];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) bv[i][tt] = bp[(size_t)(4 * sidx) * Hn + 16 * tt];
        }
    }
}
template <int TT>
GX_D void sl_issue(mfma_f4 (&acc)[TT], const float (&av)[kLB], const float (&bv)[kLB][TT], int s0, int ns)
{
#pragma unroll
    for (int i = 0; i < kLB; ++i)
        if (s0 + i < ns) {
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i][tt], acc[tt], 0, 0, 0);
        }
}

// one hidden layer of this wave's tiles: acc = bias, chain over k ascending, tanh into the activation rows
template <int TT>
GX_D void hidden_layer(const float* bias, const float* __restrict__ wt, int Hn, int col0, const float* Ain, int AS, int K,
                       float* out, int c16, int kq)
{
    mfma_f4 acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) { const float bb = bias[col0 + 16 * tt + c16]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
    const int ns = K >> 2;
    const float* ap = Ain + c16 * AS + kq;
    const float* bp = wt + (size_t)kq * Hn + col0 + c16;
    float a0[kLB], b0[kLB][TT], a1[kLB], b1[kLB][TT];
    sl_fetch<TT>(a0, b0, ap, bp, Hn, 0, ns);
#pragma unroll 1
    for (int s0 = 0; s0 < ns; s0 += 2 * kLB) {
        sl_fetch<TT>(a1, b1, ap, bp, Hn, s0 + kLB, ns);
        sl_issue<TT>(acc, a0, b0, s0, ns);
        sl_fetch<TT>(a0, b0, ap, bp, Hn, s0 + 2 * kLB, ns);
        sl_issue<TT>(acc, a1, b1, s0 + kLB, ns);
    }
    float* o = out + col0 + c16;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(4 * kq + r) * (Hn + 4) + 16 * tt] = tanh_f(acc[tt][r]);
}

template <int H, int HG>
__global__ __launch_bounds__(kThreads) void safelayer_step_kernel(StepArgs a)
{
    constexpr int HS = H + 4, HSG = HG + 4;
    extern __shared__ float4 sl_lds4[];
    float* lds = reinterpret_cast<float*>(sl_lds4);
    const int D = a.D, A = a.A, Dp = pad4(D), XS = Dp + 1, OS = outs_stride(A);
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
    mlp2_head_stage(lds + L.headG, a.gp, D, A, tid, kThreads, HG);
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);
    const Mlp2Head hg = mlp2_head_view(lds + L.headG, A, HG);

    // prologue: the prev_c update of the step just made (safelayer.py:546, 576-581).  The thread that updates env's
    // prev_c here is the one that reads it below (tid < kEnv, env = env0 + tid): program order, no fence.
    float prev_c = 0.0f;
    if (tid < kEnv) {
        const int env = env0 + tid;
        if (env < a.N) {
            prev_c = a.prev_c[env];
            if (a.prologue) {
                const float cost = a.cost_in[env], done = a.done_in[env];
                a.rew_p[env] = a.rew_in[env];
                a.cost_p[env] = cost;
                a.done_p[env] = done;
                prev_c = done > 0.0f ? 0.0f : cost;
                a.prev_c[env] = prev_c;
            }
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

    const bool skip = a.tail && net != 1; // the bootstrap needs the critic only
    const float* wtn = a.wt + (size_t)net * wt_floats(D, H); // (net 2 starts after the two H-wide networks)
    float* h1 = H1 + net * kEnv * HS;
    float* h2 = H2 + net * kEnv * HS;
    if (!skip) {
        if (net < 2) hidden_layer<H / 64>((net ? hv : hp).b1, wtn, H, (H / 4) * quarter, X, XS, Dp, h1, c16, kq);
        else hidden_layer<HG / 64>(hg.b1, wtn, HG, (HG / 4) * quarter, X, XS, Dp, h1, c16, kq);
    }
    wg_sync_lds();
    if (!skip) {
        if (net < 2) hidden_layer<H / 64>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, (H / 4) * quarter, h1, HS, H, h2, c16, kq);
        else hidden_layer<HG / 64>(hg.b2, wtn + (size_t)Dp * HG, HG, (HG / 4) * quarter, h1, HSG, HG, h2, c16, kq);
    }
    wg_sync_lds();
    // output layers: task (env e, output o) on 16 lanes; o < A: mu_o, o == A: the value, o > A: g_(o - A - 1)
    const int l = tid & 15;
    for (int task = tid >> 4; task < kEnv * (2 * A + 1); task += kThreads / 16) {
        const int e = task / (2 * A + 1), o = task - e * (2 * A + 1);
        if (a.tail && o != A) continue; // (16-lane groups take the branch together)
        float y;
        if (o < A) y = head2_out<H>(hp, o, l, H2 + e * HS);
        else if (o == A) y = head2_out<H>(hv, 0, l, H2 + (kEnv + e) * HS);
        else y = head2_out<HG>(hg, o - A - 1, l, H2 + 2 * kEnv * HS + e * HSG);
        if (l == 0) outs[e * OS + o] = y;
    }
    wg_sync_lds();
    // per env: the value, and (not in the tail) the noise, the action and log pi(a | o) of ac.step
    // (gx_policy_step.hip:policy_step_tail), then the correction
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            float* oe = outs + e * OS;
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
                        a.g[(size_t)env * A + d] = oe[A + 1 + d];
                        oe[2 * A + 1 + d] = act;
                    }
                }
                a.logp[env] = lp;
                a.prev_cost[env] = prev_c;
                float* as = a.act_safe + (size_t)env * A;
                if (a.correct) safety_correct(oe + A + 1, oe + 2 * A + 1, A, prev_c, a.delta, as);
                else
                    for (int d = 0; d < A; ++d) as[d] = oe[2 * A + 1 + d];
            }
        }
    }
    if (!a.tail && blockIdx.x == 0 && tid >= 64 && tid < 64 + A) a.logstd[tid - 64] = log_f(exp_f(gls[tid - 64]));
}

template <int H, int HG>
const void* kernel_of() { return reinterpret_cast<const void*>(safelayer_step_kernel<H, HG>); }

template <int H>
const void* kernel_of_hg(int HG)
{
    switch (HG) {
    case 64: return kernel_of<H, 64>();
    case 128: return kernel_of<H, 128>();
    case 192: return kernel_of<H, 192>();
    default: return kernel_of<H, 256>();
    }
}

const void* kernel_for(int H, int HG)
{
    switch (H) {
    case 64: return kernel_of_hg<64>(HG);
    case 128: return kernel_of_hg<128>(HG);
    case 192: return kernel_of_hg<192>(HG);
    default: return kernel_of_hg<256>(HG);
    }
}

gxl_status check_shape(const char* who, int D, int A, int H, int HG)
{
    if (D < 1 || A < 1) return fail(GXL_ERR_ARG, std::string(who) + ": D and A must be >= 1");
    if (!width_ok(H) || !width_ok(HG))
        return fail(GXL_ERR_UNSUPPORTED, std::string(who) + ": hidden width not in {64, 128, 192, 256}");
    if (!shape_ok(D, A)) return fail(GXL_ERR_UNSUPPORTED, std::string(who) + ": needs an even action width <= 16");
    if (D > 65536 || sizeof(float) * (size_t)lds_layout(D, A, H, HG).total > kLdsMax)
        return fail(GXL_ERR_UNSUPPORTED, std::string(who) + ": D too wide for the LDS tile");
    return GXL_OK;
}

} // namespace

extern "C" const char* gxl_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxl_build_id(void) { return GXL_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["safelayer"].source_hash()

extern "C" int64_t gxl_params_floats(int32_t D, int32_t A, int32_t hidden)
{
    return (shape_ok(D, A) && width_ok(hidden)) ? params_floats(D, A, hidden) : -1;
}

extern "C" int64_t gxl_g_floats(int32_t D, int32_t A, int32_t g_hidden)
{
    return (shape_ok(D, A) && width_ok(g_hidden)) ? net_floats(D, A, g_hidden) : -1;
}

extern "C" int64_t gxl_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden)
{
    return (shape_ok(D, A) && width_ok(hidden) && width_ok(g_hidden)) ? work_floats(D, hidden, g_hidden) : -1;
}

extern "C" gxl_status gxl_prepare(int32_t D, int32_t A, int32_t hidden, int32_t g_hidden, const float* d_params,
                                  const float* d_g_params, float* d_work, void* stream)
{
    if (!d_params || !d_g_params || !d_work) return fail(GXL_ERR_ARG, "gxl_prepare: null pointer");
    const gxl_status st = check_shape("gxl_prepare", D, A, hidden, g_hidden);
    if (st != GXL_OK) return st;
    const size_t lds = sizeof(float) * (size_t)lds_layout(D, A, hidden, g_hidden).total;
    if (lds > 64 * 1024) { // more dynamic LDS than the default cap: raise it for this kernel (on the current device)
        if (hipFuncSetAttribute(kernel_for(hidden, g_hidden), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(GXL_ERR_HIP, "gxl_prepare: hipFuncSetAttribute failed");
    }
    const long long n = work_floats(D, hidden, g_hidden);
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(safelayer_transpose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_params, d_g_params,
                       d_work, D, A, hidden, g_hidden);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXL_OK : fail(GXL_ERR_HIP, std::string("gxl_prepare launch failed: ") + hipGetErrorString(e));
}

extern "C" gxl_status gxl_policy_step(const gxl_step_args* g, void* stream)
{
    if (!g) return fail(GXL_ERR_ARG, "gxl_policy_step: null argument struct");
    if (g->struct_size != sizeof(gxl_step_args)) return fail(GXL_ERR_ARG, "gxl_policy_step: struct_size mismatch");
    if (g->N < 0 || g->T < 1 || g->t < 0 || g->t > g->T || g->env_offset < 0)
        return fail(GXL_ERR_ARG, "gxl_policy_step: N must be >= 0, T >= 1, t in [0, T], env_offset >= 0");
    const gxl_status st = check_shape("gxl_policy_step", g->D, g->A, g->hidden, g->g_hidden);
    if (st != GXL_OK) return st;
    const bool tail = g->t == g->T, prologue = g->t > 0;
    if (!g->d_params || !g->d_g_params || !g->d_work || !g->d_prev_c)
        return fail(GXL_ERR_ARG, "gxl_policy_step: null pointer");
    if (prologue ? (!g->d_obs_rd || !g->d_rew_in || !g->d_cost_in || !g->d_done_in || !g->d_rew || !g->d_cost || !g->d_done)
                 : !g->d_obs0)
        return fail(GXL_ERR_ARG, "gxl_policy_step: null pointer");
    if (tail ? (!g->d_obs_last || !g->d_val_last)
             : (!g->d_obs || !g->d_act || !g->d_act_safe || !g->d_mu || !g->d_g || !g->d_logp || !g->d_val ||
                !g->d_prev_cost || !g->d_logstd))
        return fail(GXL_ERR_ARG, "gxl_policy_step: null pointer");
    if (g->N == 0) return GXL_OK;
    const size_t N = (size_t)g->N, D = (size_t)g->D, A = (size_t)g->A;
    StepArgs a;
    a.N = g->N; a.D = g->D; a.A = g->A; a.env_offset = g->env_offset;
    a.tail = tail; a.prologue = prologue; a.correct = g->correct != 0;
    a.seed0 = g->seed[0]; a.seed1 = g->seed[1]; a.tnoise = g->step0 + (uint32_t)g->t;
    a.delta = g->delta;
    a.params = g->d_params; a.gp = g->d_g_params; a.wt = g->d_work;
    a.obs_rd = prologue ? g->d_obs_rd : g->d_obs0;
    a.rew_in = g->d_rew_in; a.cost_in = g->d_cost_in; a.done_in = g->d_done_in;
    a.prev_c = g->d_prev_c;
    const size_t tp = prologue ? (size_t)(g->t - 1) * N : 0;
    a.rew_p = prologue ? g->d_rew + tp : nullptr; a.cost_p = prologue ? g->d_cost + tp : nullptr;
    a.done_p = prologue ? g->d_done + tp : nullptr;
    const size_t tn = (size_t)g->t * N;
    if (tail) {
        a.obs = g->d_obs_last; a.val = g->d_val_last;
        a.act = a.act_safe = a.mu = a.g = a.logp = a.prev_cost = a.logstd = nullptr;
    } else {
        a.obs = g->d_obs + tn * D; a.act = g->d_act + tn * A; a.act_safe = g->d_act_safe + tn * A;
        a.mu = g->d_mu + tn * A; a.g = g->d_g + tn * A; a.logp = g->d_logp + tn; a.val = g->d_val + tn;
        a.prev_cost = g->d_prev_cost + tn; a.logstd = g->d_logstd;
    }
    const size_t lds = sizeof(float) * (size_t)lds_layout(g->D, g->A, g->hidden, g->g_hidden).total;
    const dim3 grid((unsigned)((g->N + kEnv - 1) / kEnv));
    void* kargs[] = {&a};
    const hipError_t e = hipLaunchKernel(kernel_for(g->hidden, g->g_hidden), grid, dim3(kThreads), kargs, lds, (hipStream_t)stream);
    return e == hipSuccess ? GXL_OK : fail(GXL_ERR_HIP, std::string("gxl_policy_step launch failed: ") + hipGetErrorString(e));
}

extern "C" gxl_status gxl_correction_probe(int32_t n, int32_t A, const float* d_g, const float* d_a, const float* d_prev_c,
                                           float delta, float* d_a_safe, void* stream)
{
    if (!d_g || !d_a || !d_prev_c || !d_a_safe) return fail(GXL_ERR_ARG, "gxl_correction_probe: null pointer");
    if (n < 0) return fail(GXL_ERR_ARG, "gxl_correction_probe: n must be >= 0");
    if (A < 1 || A > kMaxA) return fail(GXL_ERR_UNSUPPORTED, "gxl_correction_probe: A must be in 1 .. 16");
    if (n == 0) return GXL_OK;
    const unsigned blocks = (unsigned)std::min<long long>(((long long)n + 255) / 256, 4096);
    hipLaunchKernelGGL(correction_probe_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, A, d_g, d_a, d_prev_c,
                       delta, d_a_safe);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXL_OK : fail(GXL_ERR_HIP, std::string("gxl_correction_probe launch failed: ") + hipGetErrorString(e));
}
