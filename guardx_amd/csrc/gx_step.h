// gx_step.h -- what the five step libraries (gx_statewise.hip, gx_safelayer.hip, gx_episode.hip, and through gx_qstep.h
// gx_usl.hip and gx_lpg.hip) share that is not about a Q critic.  Each runs `ac.step` on the device between two env.step launches, 16
// envs per workgroup, on three two-hidden-layer tanh networks whose hidden layers gx?_prepare transposes into a workspace.
// Device: the sizes, Softplus, the transpose kernel, the pipelined MFMA chain of a hidden layer, the Gaussian sample /
// log-prob block of ac.step on a row, the logstd write and the one-episode form of a step (the sanitising load of the
// rows, the first-done bookkeeping, the tail's no-bootstrap rule).  Host: the shape check, the (H, H3) kernel dispatch, the LDS
// cap, gx?_prepare, the checks and the row-block arithmetic of gx?_policy_step, the launches.  The host functions are
// templates over the library's status enum (the enums have equal values) and its public gx?_step_args (equal names
// for every shared field); they report through the library's own `fail`, passed first.  What differs between the
// libraries comes in as values; nothing here asks which library is calling.
// One translation unit per library: everything sits in an unnamed namespace.
#ifndef GX_STEP_H
#define GX_STEP_H
#include "gx_policy.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>

namespace {

using namespace gx;

constexpr int kEnv = 16;       // envs per workgroup
constexpr int kMaxA = 16;
constexpr size_t kLdsMax = 160 * 1024;

GX_HD int64_t net_floats(int D, int Out, int H) { return (int64_t)H * D + H + (int64_t)H * H + H + (int64_t)Out * H + Out; }

GX_HD int64_t wt_floats(int D, int H) { return (int64_t)pad4(D) * H + (int64_t)H * H; }

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

// wt = [pi Wt1 | pi Wt2 | v Wt1 | v Wt2 | n3 Wt1 | n3 Wt2]; Wt1 [pad4 D][h] (rows D .. zero), Wt2 [h][h], from the torch
// layout W1 [h][in] b1 W2 [h][h] ...  The actor and the critic (in `params`) are H wide on D inputs; the third network
// `p3` is H3 wide on in3 >= D inputs, of which Wt1 takes the first D columns (c_net: in3 = D + A, its observation
// columns).  first = 2: the third network alone (the probes of the Q libraries).
__global__ void step_transpose_kernel(const float* __restrict__ params, const float* __restrict__ p3, float* __restrict__ wt,
                                      int D, int A, int H, int H3, int in3, int first)
{
    const int Dp = pad4(D);
    const long long per = (long long)Dp * H + (long long)H * H, per3 = (long long)Dp * H3 + (long long)H3 * H3;
    const long long skip = first == 2 ? 2 * per : 0, n = 2 * per + per3 - skip;
    for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += (long long)gridDim.x * blockDim.x) {
        const long long i = i0 + skip;
        const int net = i < per ? 0 : (i < 2 * per ? 1 : 2);
        const long long r = i - (long long)net * per;
        const int h = net == 2 ? H3 : H, in = net == 2 ? in3 : D;
        const float* g = net == 0 ? params : (net == 1 ? params + net_floats(D, A, H) : p3);
        const long long n1 = (long long)Dp * h;
        if (r < n1) {
            const int k = (int)(r / h), j = (int)(r - (long long)k * h);
            wt[i0] = k < D ? g[(size_t)j * in + k] : 0.0f;
        } else {
            const long long r2 = r - n1;
            const int k = (int)(r2 / h), j = (int)(r2 - (long long)k * h);
            wt[i0] = g[(size_t)h * in + h + (size_t)j * h + k];
        }
    }
}

// The one-episode form of a step (the `*_one_episode` learners, safe_rl_libX/trpo_one_episode/trpo.py:450-545: no
// reset_done, the rows sanitised, the first-done bookkeeping).  on: uniform over the launch; the rest is read only where
// it is set.  k = t_base + t, the 1-based index in the episode of the step just made.
struct EpisodeBook {
    int on, k;
    int *first_done, *ep_len;
    float *ep_ret, *ep_cost;
};

// what every step kernel's view of a gx?_step_args holds: this step's row blocks resolved on the host
struct StepCommon {
    int N, env_offset;
    int tail, prologue;
    EpisodeBook ep;
    uint32_t seed0, seed1, tnoise;
    const float *params, *wt;
    const float* obs_rd;              // [N][the env's own observation width]
    const float *rew_in, *cost_in, *done_in;
    float *rew_p, *cost_p, *done_p;                // row block t - 1
    float *obs, *act, *mu, *logp, *val, *logstd;   // row block t (tail: obs_last, val_last)
};

// The sampling part of `ac.step` on row `env`, by one lane: the noise z from the Threefry block at (env_offset + env,
// 16 tnoise + pair), one counter per pair of action dimensions; act = fmaf(sd, z, mu); log pi(act | o) summed over the
// dimensions ascending.  This is gx_policy_step.hip:policy_step_tail's block, which the main library keeps for itself:
// the two copies give the same bits.  mu_row: the A means (LDS); gls: log_std.  Stores act and mu of row block t and
// logp.  keep (an LDS row, or null): the action once more, for a caller that goes on with it.
GX_D void sample_row(const StepCommon& a, int A, const float* gls, int env, const float* mu_row, float* keep)
{
    float lp = 0.0f;
    for (int pr = 0; 2 * pr < A; ++pr) { // one counter per pair of action dimensions
        float z[2];
        normal_pair(a.seed0, a.seed1, (uint32_t)(a.env_offset + env), a.tnoise * 16u + (uint32_t)pr, z[0], z[1]);
        for (int q = 0; q < 2; ++q) {
            const int d = 2 * pr + q;
            const float sd = exp_f(gls[d]);
            const float lsd = log_f(sd);
            const float m = mu_row[d];
            const float act = fmaf(sd, z[q], m);
            const float df = act - m;
            const float var = sd * sd;
            lp = lp + ((-(df * df) / (2.0f * var) - lsd) - 0.9189385332046727f);
            a.act[(size_t)env * A + d] = act;
            a.mu[(size_t)env * A + d] = m;
            if (keep) keep[d] = act;
        }
    }
    a.logp[env] = lp;
}

// NaN, +Inf and -Inf: the exponent field is all ones
GX_D bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// The rows of the workgroup's 16 envs into the X tile [16][XS] (columns D .. and rows past N zero) and through to row
// block t of obs, by all `threads` threads.  In the one-episode form what the networks read has its non-finite entries
// replaced by +0.0f (trpo.py:453-454), and that is what obs[t] keeps; the tail's obs_last is the row as it is.
GX_D void stage_rows(const StepCommon& a, int D, int XS, float* X, int env0, int tid, int threads)
{
    for (int i = tid; i < kEnv * XS; i += threads) {
        const int e = i / XS, k = i - e * XS;
        const int env = env0 + e;
        float x = 0.0f;
        if (k < D && env < a.N) {
            const float raw = a.obs_rd[(size_t)env * D + k];
            x = (a.ep.on && non_finite(raw)) ? 0.0f : raw;
            a.obs[(size_t)env * D + k] = a.tail ? raw : x;
        }
        X[i] = x;
    }
}

// The first-done bookkeeping of the step just made, by the thread that owns env's state (trpo.py:473-501): reward and
// cost are summed up to and including the step that finishes the env, one fp32 add each.
GX_D void episode_book(const EpisodeBook& b, int env, float rew, float cost, float done)
{
    if (b.first_done[env] == 0) {
        b.ep_ret[env] = b.ep_ret[env] + rew;
        b.ep_cost[env] = b.ep_cost[env] + cost;
        b.ep_len[env] = b.k;
        if (done > 0.0f) b.first_done[env] = b.k;
    }
}

// The tail's rule in the one-episode form: a row with a non-finite entry is not bootstrapped (the intent of
// trpo.py:513-521).  True for such a row of env; false in every other launch.
GX_D bool tail_row_unusable(const StepCommon& a, int D, int env)
{
    bool bad = false;
    if (a.tail && a.ep.on)
        for (int k = 0; k < D; ++k) bad = bad || non_finite(a.obs_rd[(size_t)env * D + k]);
    return bad;
}

// logstd as the learner stores it, log(exp(log_std)): written once, by the second wave of workgroup 0
GX_D void logstd_write(float* logstd, const float* gls, int A, int tid)
{
    if (blockIdx.x == 0 && tid >= 64 && tid < 64 + A) logstd[tid - 64] = log_f(exp_f(gls[tid - 64]));
}

// acc[tile] += A[16 envs][K] * B[K][16 units of the tile], k ascending (the order of the fmaf chain); tile tt holds the
// units col0 + 16 tt + c16.  The operands of kLB k-steps are fetched together and one block AHEAD of the MFMAs that
// consume them (two register sets, the loop advances by two blocks).  BWD: the A operand is built on the way in,
// d2[j] = (1 - h2[j] h2[j]) w3[j] from the activation row and the head's weights.
constexpr int kLB = 8;
template <int TT, bool BWD, int LB>
GX_D void q_fetch(float (&av)[LB], float (&bv)[LB][TT], const float* ap, const float* w3p, const float* bp, int ldb, int s0, int ns)
{
#pragma unroll
    for (int i = 0; i < LB; ++i) {
        const int sidx = s0 + i;
        if (sidx < ns) { // wave-uniform
            float x = ap[4 * sidx];
            if (BWD) x = __fmul_rn(__fsub_rn(1.0f, __fmul_rn(x, x)), w3p[4 * sidx]);
            av[i] = x;
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) bv[i][tt] = bp[(size_t)(4 * sidx) * ldb + 16 * tt];
        }
    }
}
template <int TT, int LB>
GX_D void q_issue(mfma_f4 (&acc)[TT], const float (&av)[LB], const float (&bv)[LB][TT], int s0, int ns)
{
#pragma unroll
    for (int i = 0; i < LB; ++i)
        if (s0 + i < ns) {
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i][tt], acc[tt], 0, 0, 0);
        }
}
// Ain: activation rows [16][AS]; B: [K][ldb], this wave's tiles starting at column col0.  LB: k-steps per block (fewer
// where two tiles per wave and the iteration's own state leave fewer registers)
template <int TT, bool BWD, int LB = kLB>
GX_D void q_chain(mfma_f4 (&acc)[TT], const float* B, int ldb, int col0, const float* Ain, int AS, const float* w3, int K,
                  int c16, int kq)
{
    const int ns = K >> 2;
    const float* ap = Ain + c16 * AS + kq;
    const float* wp = w3 + kq;
    const float* bp = B + (size_t)kq * ldb + col0 + c16;
    float a0[LB], b0[LB][TT], a1[LB], b1[LB][TT];
    q_fetch<TT, BWD, LB>(a0, b0, ap, wp, bp, ldb, 0, ns);
#pragma unroll 1
    for (int s0 = 0; s0 < ns; s0 += 2 * LB) {
        q_fetch<TT, BWD, LB>(a1, b1, ap, wp, bp, ldb, s0 + LB, ns);
        q_issue<TT, LB>(acc, a0, b0, s0, ns);
        q_fetch<TT, BWD, LB>(a0, b0, ap, wp, bp, ldb, s0 + 2 * LB, ns);
        q_issue<TT, LB>(acc, a1, b1, s0 + LB, ns);
    }
}

// one hidden layer of this wave's tiles: acc = bias, chain over k ascending; TANH: tanh into the activation rows,
// otherwise the pre-activation itself (c_net's first layer before its action columns)
template <int TT, bool TANH>
GX_D void hidden_layer(const float* bias, const float* __restrict__ wt, int Hn, int col0, const float* Ain, int AS, int K,
                       float* out, int c16, int kq)
{
    mfma_f4 acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) { const float bb = bias[col0 + 16 * tt + c16]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
    q_chain<TT, false>(acc, wt, Hn, col0, Ain, AS, Ain, K, c16, kq);
    float* o = out + col0 + c16;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(4 * kq + r) * (Hn + 4) + 16 * tt] = TANH ? tanh_f(acc[tt][r]) : acc[tt][r];
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
// the values of gxs_status, gxl_status, gxu_status and gxp_status
constexpr int kOk = 0, kErrArg = 1, kErrUnsupported = 2, kErrHip = 4;
// the library's `fail`: records the message as the calling thread's last error and returns the status
template <class Status>
using FailFn = Status (*)(Status, const std::string&);

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
bool shape_ok(int D, int A) { return D >= 1 && A >= 2 && A <= kMaxA && !(A & 1); }

// the gx?_params_floats and gx?_work_floats entry points: -1 if unsupported
int64_t params_floats(int D, int A, int H) { return (shape_ok(D, A) && width_ok(H)) ? net_floats(D, A, H) + net_floats(D, 1, H) + A : -1; }
int64_t work_floats(int D, int A, int H, int H3)
{
    return (shape_ok(D, A) && width_ok(H) && width_ok(H3)) ? 2 * wt_floats(D, H) + wt_floats(D, H3) : -1;
}

// how a library speaks of the width of its networks' input row: the least one, and the two messages that name it
struct RowText { int min; const char *too_small, *too_wide; };
constexpr RowText kRowD = {1, ": D and A must be >= 1", ": D too wide for the LDS tile"};

// lds_bytes(D, A, H, H3): the dynamic LDS of the kernel that is going to run
template <class Status, class LdsFn>
Status check_shape(FailFn<Status> fail, const char* who, const RowText& row, LdsFn lds_bytes, int D, int A, int H, int H3)
{
    if (D < row.min || A < 1) return fail(Status(kErrArg), std::string(who) + row.too_small);
    if (!width_ok(H) || !width_ok(H3))
        return fail(Status(kErrUnsupported), std::string(who) + ": hidden width not in {64, 128, 192, 256}");
    if (!shape_ok(D, A)) return fail(Status(kErrUnsupported), std::string(who) + ": needs an even action width <= 16");
    if (D > 65536 || lds_bytes(D, A, H, H3) > kLdsMax) return fail(Status(kErrUnsupported), std::string(who) + row.too_wide);
    return Status(kOk);
}

template <class Status>
Status raise_lds(FailFn<Status> fail, const char* who, const void* kernel, size_t lds)
{
    if (lds > 64 * 1024) { // more dynamic LDS than the default cap: raise it for this kernel (on the current device)
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(Status(kErrHip), std::string(who) + ": hipFuncSetAttribute failed");
    }
    return Status(kOk);
}

// Kernel dispatch.  K names a library's kernels: K::get<H, H3>() is the address of the instance (a probe kernel has no H
// and ignores it).
template <class K, int H>
const void* q_kernel_hc(int H3)
{
    switch (H3) {
    case 64: return K::template get<H, 64>();
    case 128: return K::template get<H, 128>();
    case 192: return K::template get<H, 192>();
    default: return K::template get<H, 256>();
    }
}
template <class K>
const void* q_kernel_for(int H, int H3)
{
    switch (H) {
    case 64: return q_kernel_hc<K, 64>(H3);
    case 128: return q_kernel_hc<K, 128>(H3);
    case 192: return q_kernel_hc<K, 192>(H3);
    default: return q_kernel_hc<K, 256>(H3);
    }
}

// `last` = hipGetLastError() after a <<< >>> launch or the result of hipLaunchKernel
template <class Status>
Status q_launched(FailFn<Status> fail, const char* who, hipError_t last)
{
    return last == hipSuccess ? Status(kOk) : fail(Status(kErrHip), std::string(who) + " launch failed: " + hipGetErrorString(last));
}

// one workgroup of `threads` per 16 rows
template <class Status, class Args>
Status q_launch(FailFn<Status> fail, const char* who, const void* kernel, int n, int threads, Args& a, size_t lds, void* stream)
{
    void* kargs[] = {&a};
    return q_launched(fail, who, hipLaunchKernel(kernel, dim3((unsigned)((n + kEnv - 1) / kEnv)), dim3((unsigned)threads), kargs,
                                                  lds, (hipStream_t)stream));
}

// a kernel over n elements, one per thread of 256-thread blocks, at most max_blocks of them (grid-stride beyond)
template <class Status, class Kernel, class... Args>
Status launch_flat(FailFn<Status> fail, const char* who, Kernel kernel, long long n, long long max_blocks, void* stream, Args... args)
{
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, max_blocks);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, args...);
    return q_launched(fail, who, hipGetLastError());
}

// the transposed hidden layers of `first` = 0: the three networks, 2: the third alone, into d_work (n floats)
template <class Status>
Status transpose(FailFn<Status> fail, const char* who, long long n, const float* d_params, const float* d_p3, float* d_work, int D,
                 int A, int H, int H3, int in3, int first, void* stream)
{
    return launch_flat(fail, who, step_transpose_kernel, n, 1024, stream, d_params, d_p3, d_work, D, A, H, H3, in3, first);
}

// gx?_prepare; StepK names the library's step kernels, d_p3 is its third network on in3 inputs
template <class StepK, class Status, class LdsFn>
Status prepare(FailFn<Status> fail, const char* who, const RowText& row, LdsFn lds_bytes, int D, int A, int H, int H3, int in3,
               const float* d_params, const float* d_p3, float* d_work, void* stream)
{
    if (!d_params || !d_p3 || !d_work) return fail(Status(kErrArg), std::string(who) + ": null pointer");
    Status st = check_shape(fail, who, row, lds_bytes, D, A, H, H3);
    if (st != Status(kOk)) return st;
    st = raise_lds(fail, who, q_kernel_for<StepK>(H, H3), lds_bytes(D, A, H, H3));
    if (st != Status(kOk)) return st;
    return transpose(fail, who, work_floats(D, A, H, H3), d_params, d_p3, d_work, D, A, H, H3, in3, 0, stream);
}

// The checks gx?_policy_step makes before it launches.  D, H3, p3: where G keeps the width of the networks' input row,
// the third network's hidden width and its parameters.  own_range(g): the library's own range checks, named by the tail
// `own_text` of the message; own_ptrs(g, tail): its own pointers are there.
template <class Status, class G, class LdsFn, class OwnRange, class OwnPtrs>
Status check_common(FailFn<Status> fail, const char* who, const G* g, const RowText& row, LdsFn lds_bytes, int32_t G::*D,
                    int32_t G::*H3, const float* G::*p3, OwnRange own_range, const char* own_text, OwnPtrs own_ptrs)
{
    const std::string w(who);
    if (!g) return fail(Status(kErrArg), w + ": null argument struct");
    if (g->struct_size != sizeof(G)) return fail(Status(kErrArg), w + ": struct_size mismatch");
    if (g->N < 0 || g->T < 1 || g->t < 0 || g->t > g->T || g->env_offset < 0 || !own_range(*g))
        return fail(Status(kErrArg), w + ": N must be >= 0, T >= 1, t in [0, T], env_offset >= 0" + own_text);
    const Status st = check_shape(fail, who, row, lds_bytes, g->*D, g->A, g->hidden, g->*H3);
    if (st != Status(kOk)) return st;
    const bool tail = g->t == g->T, prologue = g->t > 0;
    if (!g->d_params || !(g->*p3) || !g->d_work || !own_ptrs(*g, tail)) return fail(Status(kErrArg), w + ": null pointer");
    if (prologue ? (!g->d_obs_rd || !g->d_rew_in || !g->d_cost_in || !g->d_done_in || !g->d_rew || !g->d_cost || !g->d_done)
                 : !g->d_obs0)
        return fail(Status(kErrArg), w + ": null pointer");
    if (tail ? (!g->d_obs_last || !g->d_val_last) : (!g->d_obs || !g->d_act || !g->d_mu || !g->d_logp || !g->d_val || !g->d_logstd))
        return fail(Status(kErrArg), w + ": null pointer");
    return Status(kOk);
}

// the shared fields of a checked gx?_step_args, D = the width of a row of d_obs; returns the offset of row block t in a
// [T][N] array (0 in the tail)
template <class G>
size_t fill_common(const G& g, int D, StepCommon& c)
{
    const size_t N = (size_t)g.N, A = (size_t)g.A;
    c.N = g.N; c.env_offset = g.env_offset;
    c.tail = g.t == g.T; c.prologue = g.t > 0;
    c.ep = EpisodeBook{}; // the reset_done form; fill_book sets the other
    c.seed0 = g.seed[0]; c.seed1 = g.seed[1]; c.tnoise = g.step0 + (uint32_t)g.t;
    c.params = g.d_params; c.wt = g.d_work;
    c.obs_rd = c.prologue ? g.d_obs_rd : g.d_obs0;
    c.rew_in = g.d_rew_in; c.cost_in = g.d_cost_in; c.done_in = g.d_done_in;
    const size_t tp = c.prologue ? (size_t)(g.t - 1) * N : 0;
    c.rew_p = c.prologue ? g.d_rew + tp : nullptr; c.cost_p = c.prologue ? g.d_cost + tp : nullptr;
    c.done_p = c.prologue ? g.d_done + tp : nullptr;
    if (c.tail) {
        c.obs = g.d_obs_last; c.val = g.d_val_last;
        c.act = c.mu = c.logp = c.logstd = nullptr;
        return 0;
    }
    const size_t tn = (size_t)g.t * N;
    c.obs = g.d_obs + tn * (size_t)D; c.act = g.d_act + tn * A; c.mu = g.d_mu + tn * A;
    c.logp = g.d_logp + tn; c.val = g.d_val + tn; c.logstd = g.d_logstd;
    return tn;
}

// The checks of a guardx_<library>_policy_step_episode entry on its bookkeeping argument (gx_first_done_state), after those
// of gx?_policy_step on the step arguments and before anything is launched.
template <class Status, class Book>
Status check_book(FailFn<Status> fail, const char* who, const Book* b)
{
    const std::string w(who);
    if (!b) return fail(Status(kErrArg), w + ": null bookkeeping struct");
    if (b->struct_size != sizeof(Book)) return fail(Status(kErrArg), w + ": bookkeeping struct_size mismatch");
    if (b->t_base < 0) return fail(Status(kErrArg), w + ": t_base must be >= 0");
    if (!b->d_first_done || !b->d_ep_len || !b->d_ep_ret || !b->d_ep_cost) return fail(Status(kErrArg), w + ": null bookkeeping pointer");
    return Status(kOk);
}

// the one-episode form of step t (null: the reset_done form, as fill_common leaves it)
template <class Book>
void fill_book(const Book* b, int t, StepCommon& c)
{
    if (!b) return;
    c.ep.on = 1; c.ep.k = b->t_base + t;
    c.ep.first_done = b->d_first_done; c.ep.ep_len = b->d_ep_len;
    c.ep.ep_ret = b->d_ep_ret; c.ep.ep_cost = b->d_ep_cost;
}

// the view of a tail launch alone on n caller-supplied rows (the guardx_<library>_tail_probe entry points): no prologue, no state
inline void fill_tail_probe(StepCommon& c, int n, const float* params, const float* work, const float* rows, float* obs_last,
                            float* val_last)
{
    c = StepCommon{};
    c.N = n; c.tail = 1; c.ep.on = 1;
    c.params = params; c.wt = work; c.obs_rd = rows;
    c.obs = obs_last; c.val = val_last;
}

} // namespace
#endif // GX_STEP_H
