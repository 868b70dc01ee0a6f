// gx_episode.hip -- libguardx_episode.so (include/guardx_episode.h): `ac.step(o)` of the `*_one_episode` learners
// (safe_rl_libX/trpo_one_episode/trpo.py:450-545, cpo_one_episode/cpo.py:619-708) for one control step over all envs,
// with the first-done bookkeeping of the step just made in front of it, and the one-episode buffer's finish_path + get
// (trpo.py:67-132, cpo.py:72-156).  These learners never call reset_done(): the env launch between two policy steps is
// a plain step, and what the policy reads is the env's plain observation with its non-finite entries zeroed.  The row
// feeds the actor's mu_net, the critic v and, for the CPO family, the cost critic vc (identity output).
//
// The networks' arithmetic is the fused rollout's (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward): every
// hidden unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias, then tanh_f; an output is 16
// lane partials over the units 64 c + 4 l + j folded by the butterfly of head2_out; the noise, the action and
// log pi(a | o) are gx_step.h:sample_row's.  On a finite row the actor and v therefore give the bits of rollout_policy,
// and v and vc those of the batched critic pass (gx_critic.hip).
//
// Organisation: that of gx_safelayer.hip.  A 768-thread workgroup (12 waves) serves 16 envs from ONE staged copy of
// their rows; waves 4 n .. 4 n + 3 own network n (0 actor, 1 v, 2 vc) and a quarter of its hidden units each.  Without a
// cost critic the third group of waves does nothing: the caller passes the value network's block in the cost critic's
// place, so that gxe_prepare and the (H, H3) dispatch stay those of the other step libraries.
//
// Here: the LDS layout, the step kernel, the two kernels of gxe_finish / guardx_episode_finish_cols and the C entry points.  The
// one-episode behaviour itself (the sanitising load, the first-done bookkeeping, the tail's rule), the hidden layers'
// MFMA chain, the sample / log-prob block, the transpose kernel and the host side's checks, dispatch and launches are
// gx_step.h's, shared with the other step libraries: the safelayer, USL and LPG step kernels run the same device code
// in their one-episode form.
#include "../../include/guardx_episode.h"
#include "gx_step.h"
#include <cstring>

#ifndef GXE_BUILD_ID
#define GXE_BUILD_ID "unknown"
#endif

namespace {

using namespace gx;

thread_local std::string g_err;

gxe_status fail(gxe_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kThreads = 768;  // 12 waves: four per network

// LDS, in floats: pi head | v head | vc head (b1 b2 W3 b3 each) | X [16][pad4 D + 1] | H1 pi, v [16][H + 4], vc [16][HC + 4] |
// H2 likewise | outs [16][A + 2]
struct Lds { int headP, headV, headC, X, H1, H2, outs, total; };
GX_HD Lds lds_layout(int D, int A, int H, int HC)
{
    Lds L;
    int o = 0;
    L.headP = o; o += pad4(mlp2_head_floats(A, H));
    L.headV = o; o += pad4(mlp2_head_floats(1, H));
    L.headC = o; o += pad4(mlp2_head_floats(1, HC));
    L.X = o; o += pad4(kEnv * (pad4(D) + 1));
    const int hid = kEnv * (2 * (H + 4) + (HC + 4));
    L.H1 = o; o += hid;
    L.H2 = o; o += hid;
    L.outs = o; o += pad4(kEnv * (A + 2));
    L.total = o;
    return L;
}
size_t lds_bytes(int D, int A, int H, int HC) { return sizeof(float) * (size_t)lds_layout(D, A, H, HC).total; }

// the kernel's view of gxe_step_args: this step's row blocks resolved on the host (c.ep: always the one-episode form)
struct StepArgs {
    StepCommon c;
    int D, A, has_vc;
    const float* vcp;
    float* vc;                        // row block t (tail: vc_last)
};

template <int H, int HC>
__global__ __launch_bounds__(kThreads) void episode_step_kernel(StepArgs sa)
{
    const StepCommon& a = sa.c;
    constexpr int HS = H + 4, HSC = HC + 4;
    extern __shared__ float4 ep_lds4[];
    float* lds = reinterpret_cast<float*>(ep_lds4);
    const int D = sa.D, A = sa.A, Dp = pad4(D), XS = Dp + 1;
    const Lds L = lds_layout(D, A, H, HC);
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
    if (sa.has_vc) mlp2_head_stage(lds + L.headC, sa.vcp, D, 1, tid, kThreads, HC); // (uniform: a kernel argument)
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);
    const Mlp2Head hc = mlp2_head_view(lds + L.headC, 1, HC);

    // prologue: the first-done bookkeeping of the step just made (gx_step.h:episode_book).  One thread owns an env's state.
    if (a.prologue && tid < kEnv) {
        const int env = env0 + tid;
        if (env < a.N) {
            const float rew = a.rew_in[env], cost = a.cost_in[env], done = a.done_in[env];
            a.rew_p[env] = rew;
            a.cost_p[env] = cost;
            a.done_p[env] = done;
            episode_book(a.ep, env, rew, cost, done);
        }
    }
    stage_rows(a, D, XS, X, env0, tid, kThreads); // sanitised; the tail's obs_last raw
    wg_sync_lds(); // rows and heads

    const bool skip = (a.tail && net == 0) || (net == 2 && !sa.has_vc); // the bootstrap needs the critics only
    const float* wtn = a.wt + (size_t)net * wt_floats(D, H); // (net 2 starts after the two H-wide networks)
    float* h1 = H1 + net * kEnv * HS;
    float* h2 = H2 + net * kEnv * HS;
    if (!skip) {
        if (net < 2) hidden_layer<H / 64, true>((net ? hv : hp).b1, wtn, H, (H / 4) * quarter, X, XS, Dp, h1, c16, kq);
        else hidden_layer<HC / 64, true>(hc.b1, wtn, HC, (HC / 4) * quarter, X, XS, Dp, h1, c16, kq);
    }
    wg_sync_lds();
    if (!skip) {
        if (net < 2) hidden_layer<H / 64, true>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, (H / 4) * quarter, h1, HS, H, h2, c16, kq);
        else hidden_layer<HC / 64, true>(hc.b2, wtn + (size_t)Dp * HC, HC, (HC / 4) * quarter, h1, HSC, HC, h2, c16, kq);
    }
    wg_sync_lds();
    // output layers: task (env e, output o) on 16 lanes; o < A: mu_o, o == A: the value, o == A + 1: vc
    const int l = tid & 15;
    for (int task = tid >> 4; task < kEnv * (A + 2); task += kThreads / 16) {
        const int e = task / (A + 2), o = task - e * (A + 2);
        if ((a.tail && o < A) || (o == A + 1 && !sa.has_vc)) continue; // (16-lane groups take the branch together)
        float y;
        if (o < A) y = head2_out<H>(hp, o, l, H2 + e * HS);
        else if (o == A) y = head2_out<H>(hv, 0, l, H2 + (kEnv + e) * HS);
        else y = head2_out<HC>(hc, 0, l, H2 + 2 * kEnv * HS + e * HSC);
        if (l == 0) outs[e * (A + 2) + o] = y;
    }
    wg_sync_lds();
    // per env: the values, and (not in the tail) the noise, the action and log pi(a | o) of ac.step
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            float v = outs[e * (A + 2) + A], vc = sa.has_vc ? outs[e * (A + 2) + A + 1] : 0.0f;
            if (tail_row_unusable(a, D, env)) v = vc = 0.0f;
            a.val[env] = v;
            if (sa.has_vc) sa.vc[env] = vc;
            if (!a.tail) sample_row(a, A, gls, env, outs + e * (A + 2), nullptr);
        }
    }
    if (!a.tail) logstd_write(a.logstd, gls, A, tid);
}

struct StepKernel { template <int H, int HC> static const void* get() { return reinterpret_cast<const void*>(episode_step_kernel<H, HC>); } };

// ---------------------------------------------------------------------------------------------------------------------
// gxe_finish
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kFinEnvs = 256; // envs per block of the first launch: the granule of the offsets' prefix sum

// workspace, in 4-byte words: adv [T][N] | ret [T][N] | adc [T][N] | cost_ret [T][N] | stats [N][4] (mean, sd, cost mean)
// | len [N] (int) | block sums of len [ceil(N / 256)] (int)
struct FinWork { size_t adv, ret, adc, cret, stats, len, bsum, total; };
GX_HD FinWork fin_work(size_t N, size_t T)
{
    FinWork w;
    size_t o = 0;
    w.adv = o; o += T * N;
    w.ret = o; o += T * N;
    w.adc = o; o += T * N;
    w.cret = o; o += T * N;
    w.stats = o; o += 4 * N;
    w.len = o; o += N;
    w.bsum = o; o += (N + kFinEnvs - 1) / kFinEnvs;
    w.total = o;
    return w;
}

// One GAE channel of env `env` over [0, L) closed with `boot`, the order of include/guardx_episode.h: raw advantages
// and returns into the time-major work arrays, then mean and (scale) the standard deviation over all T entries.
GX_D void fin_channel(int N, int T, int L, int env, const float* __restrict__ rew, const float* __restrict__ val, float boot,
                      float gamma, double dg, double dgl, float* __restrict__ adv, float* __restrict__ ret, bool scale,
                      float& mean_out, float& sd_out)
{
    double acc = 0.0, r = (double)boot;
    float vnext = boot, s = 0.0f;
    for (int t = L - 1; t >= 0; --t) {
        const size_t i = (size_t)t * N + env;
        const float rt = rew[i], vt = val[i];
        const float delta = (rt + gamma * vnext) - vt;
        acc = (double)delta + dgl * acc;
        r = (double)rt + dg * r;
        const float af = (float)acc;
        adv[i] = af;
        ret[i] = (float)r;
        s = s + af;
        vnext = vt;
    }
    const float mean = s / (float)T;
    float sd = 1.0f;
    if (scale) {
        float q = 0.0f;
        for (int t = 0; t < T; ++t) {
            const float d = (t < L ? adv[(size_t)t * N + env] : 0.0f) - mean;
            q = q + d * d;
        }
        sd = sqrtf(q / (float)T);
    }
    mean_out = mean;
    sd_out = sd;
}

// launch 1, one thread per env: the path length, both channels, the block's sum of lengths
__global__ __launch_bounds__(kFinEnvs) void finish_gae_kernel(int N, int T, const int* __restrict__ first_done,
                                                              const float* __restrict__ rew, const float* __restrict__ val,
                                                              const float* __restrict__ val_last, const float* __restrict__ cost,
                                                              const float* __restrict__ vc, const float* __restrict__ vc_last,
                                                              float gamma, double dg, double dgl, float* __restrict__ work)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const FinWork w = fin_work((size_t)N, (size_t)T);
    const int env = blockIdx.x * kFinEnvs + threadIdx.x;
    if (env < N) {
        const int fd = first_done[env];
        const int L = fd > 0 ? (fd < T ? fd : T) : T;
        reinterpret_cast<int*>(work + w.len)[env] = L;
        atomicAdd(&total, L);
        float* st = work + w.stats + 4 * (size_t)env;
        fin_channel(N, T, L, env, rew, val, fd > 0 ? 0.0f : val_last[env], gamma, dg, dgl, work + w.adv, work + w.ret, true,
                    st[0], st[1]);
        if (cost) {
            float unused;
            fin_channel(N, T, L, env, cost, vc, fd > 0 ? 0.0f : vc_last[env], gamma, dg, dgl, work + w.adc, work + w.cret,
                        false, st[2], unused);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) reinterpret_cast<int*>(work + w.bsum)[blockIdx.x] = total;
}

// what guardx_episode_finish_cols adds to the gather launch (n == 0, qc == null: gxe_finish): extra time-major columns
// src [T][N][w] -> dst [.][w], and USL's / LPG's target targetc[t] = cost[t] + gamma qc[t + 1], one fp32 multiply and one
// fp32 add, the product taken as +0 at t + 1 == L (usl_one_episode/usl.py:105-107)
constexpr int kMaxCols = GXE_FINISH_MAX_COLS;
struct FinCols {
    int n;
    int w[kMaxCols];
    const float* src[kMaxCols];
    float* dst[kMaxCols];
    const float *qc, *qcost;
    float* targetc;
    float gamma;
};

// launch 2, one block per env: its offset (the lengths before it: whole blocks of launch 1, then its own block's envs),
// then its L rows gathered from the time-major tensors into the compacted env-major ones, the advantages normalised on
// the way.  The block of the last env also writes the total.
__global__ __launch_bounds__(256) void finish_gather_kernel(int N, int T, int D, int A, const float* __restrict__ obs,
                                                            const float* __restrict__ act, const float* __restrict__ mu,
                                                            const float* __restrict__ logp, const float* __restrict__ work,
                                                            int has_cost, float* __restrict__ obs_c, float* __restrict__ act_c,
                                                            float* __restrict__ mu_c, float* __restrict__ logp_c,
                                                            float* __restrict__ ret_c, float* __restrict__ adv_c,
                                                            float* __restrict__ cret_c, float* __restrict__ adc_c,
                                                            int* __restrict__ n_valid, FinCols x)
{
    __shared__ int offset;
    if (threadIdx.x == 0) offset = 0;
    __syncthreads();
    const FinWork w = fin_work((size_t)N, (size_t)T);
    const int* len = reinterpret_cast<const int*>(work + w.len);
    const int* bsum = reinterpret_cast<const int*>(work + w.bsum);
    const int env = blockIdx.x, blk = env / kFinEnvs, tid = threadIdx.x;
    int part = 0;
    for (int b = tid; b < blk; b += 256) part += bsum[b];
    for (int e = blk * kFinEnvs + tid; e < env; e += 256) part += len[e];
    if (part) atomicAdd(&offset, part); // integers: any order gives the same sum
    __syncthreads();
    const size_t off = (size_t)offset;
    const int L = len[env];
    if (env == N - 1 && tid == 0) *n_valid = (int)off + L;
    const float* st = work + w.stats + 4 * (size_t)env;
    const float mean = st[0], sd = st[1], cmean = st[2];
    for (int t = tid; t < L; t += 256) {
        const size_t i = (size_t)t * N + env;
        logp_c[off + t] = logp[i];
        ret_c[off + t] = work[w.ret + i];
        adv_c[off + t] = (work[w.adv + i] - mean) / sd;
        if (has_cost) {
            cret_c[off + t] = work[w.cret + i];
            adc_c[off + t] = work[w.adc + i] - cmean;
        }
    }
    const int W = D + 2 * A;
    for (long long j = tid; j < (long long)L * W; j += 256) {
        const int t = (int)(j / W), k = (int)(j - (long long)t * W);
        const size_t i = (size_t)t * N + env, o = off + t;
        if (k < D) obs_c[o * D + k] = obs[i * D + k];
        else if (k < D + A) act_c[o * A + (k - D)] = act[i * A + (k - D)];
        else mu_c[o * A + (k - D - A)] = mu[i * A + (k - D - A)];
    }
    for (int c = 0; c < x.n; ++c) { // uniform
        const int w = x.w[c];
        const float* src = x.src[c];
        float* dst = x.dst[c];
        for (long long j = tid; j < (long long)L * w; j += 256) {
            const int t = (int)(j / w), k = (int)(j - (long long)t * w);
            dst[(off + t) * w + k] = src[((size_t)t * N + env) * w + k];
        }
    }
    if (x.qc)
        for (int t = tid; t < L; t += 256) {
            const float next = t + 1 < L ? __fmul_rn(x.gamma, x.qc[(size_t)(t + 1) * N + env]) : 0.0f;
            x.targetc[off + t] = __fadd_rn(x.qcost[(size_t)t * N + env], next);
        }
}

__global__ void zero_count_kernel(int* n_valid) { *n_valid = 0; }

} // namespace

extern "C" const char* gxe_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxe_build_id(void) { return GXE_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["episode"].source_hash()

extern "C" int64_t gxe_params_floats(int32_t D, int32_t A, int32_t hidden) { return params_floats(D, A, hidden); }

extern "C" int64_t gxe_vc_floats(int32_t D, int32_t vc_hidden) { return (D >= 1 && width_ok(vc_hidden)) ? net_floats(D, 1, vc_hidden) : -1; }

extern "C" int64_t gxe_work_floats(int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden) { return work_floats(D, A, hidden, vc_hidden); }

extern "C" gxe_status gxe_prepare(int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden, const float* d_params,
                                  const float* d_vc_params, float* d_work, void* stream)
{
    return prepare<StepKernel>(fail, "gxe_prepare", kRowD, lds_bytes, D, A, hidden, vc_hidden, D, d_params, d_vc_params, d_work, stream);
}

extern "C" gxe_status gxe_policy_step(const gxe_step_args* g, void* stream)
{
    const gxe_status st = check_common(
        fail, "gxe_policy_step", g, kRowD, lds_bytes, &gxe_step_args::D, &gxe_step_args::vc_hidden, &gxe_step_args::d_vc_params,
        [](const gxe_step_args& g) { return g.t_base >= 0; }, ", t_base >= 0", [](const gxe_step_args& g, bool tail) {
            return g.d_first_done && g.d_ep_ret && g.d_ep_cost && g.d_ep_len && (!g.has_vc || (tail ? g.d_vc_last : g.d_vc));
        });
    if (st != GXE_OK || g->N == 0) return st;
    StepArgs a;
    const size_t tn = fill_common(*g, g->D, a.c);
    a.D = g->D; a.A = g->A; a.has_vc = g->has_vc != 0;
    fill_book(g, g->t, a.c); // (gxe_step_args carries the bookkeeping's fields itself)
    a.vcp = g->d_vc_params;
    a.vc = !a.has_vc ? nullptr : (a.c.tail ? g->d_vc_last : g->d_vc + tn);
    return q_launch(fail, "gxe_policy_step", q_kernel_for<StepKernel>(g->hidden, g->vc_hidden), g->N, kThreads, a,
                    lds_bytes(g->D, g->A, g->hidden, g->vc_hidden), stream);
}

extern "C" gxe_status gxe_tail_probe(int32_t n, int32_t D, int32_t A, int32_t hidden, int32_t vc_hidden, int32_t has_vc,
                                     const float* d_params, const float* d_vc_params, const float* d_work, const float* d_rows,
                                     float* d_obs_last, float* d_val_last, float* d_vc_last, void* stream)
{
    const char* who = "gxe_tail_probe";
    if (n < 0) return fail(GXE_ERR_ARG, std::string(who) + ": n must be >= 0");
    const gxe_status st = check_shape(fail, who, kRowD, lds_bytes, D, A, hidden, vc_hidden);
    if (st != GXE_OK) return st;
    if (!d_params || !d_vc_params || !d_work || !d_rows || !d_obs_last || !d_val_last || (has_vc && !d_vc_last))
        return fail(GXE_ERR_ARG, std::string(who) + ": null pointer");
    if (n == 0) return GXE_OK;
    StepArgs a;
    memset(&a, 0, sizeof a);
    fill_tail_probe(a.c, n, d_params, d_work, d_rows, d_obs_last, d_val_last);
    a.D = D; a.A = A; a.has_vc = has_vc != 0;
    a.vcp = d_vc_params;
    a.vc = a.has_vc ? d_vc_last : nullptr;
    return q_launch(fail, who, q_kernel_for<StepKernel>(hidden, vc_hidden), n, kThreads, a, lds_bytes(D, A, hidden, vc_hidden), stream);
}

extern "C" int64_t gxe_finish_work_floats(int32_t N, int32_t T)
{
    return (N >= 0 && T >= 1) ? (int64_t)fin_work((size_t)N, (size_t)T).total : -1;
}

namespace {

// gxe_finish (x.n == 0, no target) and guardx_episode_finish_cols under their own names
gxe_status finish(const char* who, int32_t N, int32_t T, int32_t D, int32_t A, float gamma, float lam, int32_t* d_first_done,
                  const float* d_obs, const float* d_act, const float* d_mu, const float* d_logp, const float* d_rew,
                  const float* d_val, const float* d_val_last, const float* d_cost, const float* d_vc, const float* d_vc_last,
                  float* d_work, float* d_obs_c, float* d_act_c, float* d_mu_c, float* d_logp_c, float* d_ret, float* d_adv,
                  float* d_cost_ret, float* d_adc, int32_t* d_n_valid, const FinCols& x, void* stream)
{
    if (N < 0 || T < 1 || D < 1 || A < 1) return fail(GXE_ERR_ARG, std::string(who) + ": N must be >= 0, T, D and A >= 1");
    if ((int64_t)N * T > 0x7fffffffLL) return fail(GXE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 rows");
    if (!d_first_done || !d_obs || !d_act || !d_mu || !d_logp || !d_rew || !d_val || !d_val_last || !d_work || !d_obs_c ||
        !d_act_c || !d_mu_c || !d_logp_c || !d_ret || !d_adv || !d_n_valid)
        return fail(GXE_ERR_ARG, std::string(who) + ": null pointer");
    const int n_cost = !!d_cost + !!d_vc + !!d_vc_last + !!d_cost_ret + !!d_adc;
    if (n_cost != 0 && n_cost != 5) return fail(GXE_ERR_ARG, std::string(who) + ": the cost channel's pointers are all given or all null");
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(1), 0, s, d_n_valid);
        return q_launched(fail, who, hipGetLastError());
    }
    const double dg = (double)gamma, dgl = (double)gamma * (double)lam;
    hipLaunchKernelGGL(finish_gae_kernel, dim3((unsigned)((N + kFinEnvs - 1) / kFinEnvs)), dim3(kFinEnvs), 0, s, N, T,
                       (const int*)d_first_done, d_rew, d_val, d_val_last, d_cost, d_vc, d_vc_last, gamma, dg, dgl, d_work);
    const gxe_status st = q_launched(fail, who, hipGetLastError());
    if (st != GXE_OK) return st;
    hipLaunchKernelGGL(finish_gather_kernel, dim3((unsigned)N), dim3(256), 0, s, N, T, D, A, d_obs, d_act, d_mu, d_logp,
                       (const float*)d_work, n_cost ? 1 : 0, d_obs_c, d_act_c, d_mu_c, d_logp_c, d_ret, d_adv, d_cost_ret, d_adc,
                       (int*)d_n_valid, x);
    return q_launched(fail, who, hipGetLastError());
}

} // namespace

extern "C" gxe_status gxe_finish(int32_t N, int32_t T, int32_t D, int32_t A, float gamma, float lam, int32_t* d_first_done,
                                 const float* d_obs, const float* d_act, const float* d_mu, const float* d_logp,
                                 const float* d_rew, const float* d_val, const float* d_val_last, const float* d_cost,
                                 const float* d_vc, const float* d_vc_last, float* d_work, float* d_obs_c, float* d_act_c,
                                 float* d_mu_c, float* d_logp_c, float* d_ret, float* d_adv, float* d_cost_ret, float* d_adc,
                                 int32_t* d_n_valid, void* stream)
{
    return finish("gxe_finish", N, T, D, A, gamma, lam, d_first_done, d_obs, d_act, d_mu, d_logp, d_rew, d_val, d_val_last,
                  d_cost, d_vc, d_vc_last, d_work, d_obs_c, d_act_c, d_mu_c, d_logp_c, d_ret, d_adv, d_cost_ret, d_adc,
                  d_n_valid, FinCols{}, stream);
}

extern "C" gxe_status guardx_episode_finish_cols(int32_t N, int32_t T, int32_t D, int32_t A, float gamma, float lam, int32_t* d_first_done,
                                      const float* d_obs, const float* d_act, const float* d_mu, const float* d_logp,
                                      const float* d_rew, const float* d_val, const float* d_val_last, const float* d_cost,
                                      const float* d_vc, const float* d_vc_last, float* d_work, float* d_obs_c, float* d_act_c,
                                      float* d_mu_c, float* d_logp_c, float* d_ret, float* d_adv, float* d_cost_ret,
                                      float* d_adc, int32_t n_cols, const gxe_finish_col* cols, const float* d_qc,
                                      const float* d_qcost, float* d_targetc, int32_t* d_n_valid, void* stream)
{
    const char* who = "guardx_episode_finish_cols";
    if (n_cols < 0 || n_cols > kMaxCols) return fail(GXE_ERR_ARG, std::string(who) + ": n_cols must be in 0 .. GXE_FINISH_MAX_COLS");
    if (n_cols > 0 && !cols) return fail(GXE_ERR_ARG, std::string(who) + ": null column list");
    FinCols x = {};
    x.n = n_cols;
    for (int c = 0; c < n_cols; ++c) {
        if (!cols[c].d_src || !cols[c].d_dst || cols[c].width < 1)
            return fail(GXE_ERR_ARG, std::string(who) + ": a column needs a source, a destination and a width >= 1");
        x.src[c] = cols[c].d_src; x.dst[c] = cols[c].d_dst; x.w[c] = cols[c].width;
    }
    const int n_q = !!d_qc + !!d_qcost + !!d_targetc;
    if (n_q != 0 && n_q != 3) return fail(GXE_ERR_ARG, std::string(who) + ": the target's pointers are all given or all null");
    x.qc = d_qc; x.qcost = d_qcost; x.targetc = d_targetc; x.gamma = gamma;
    return finish(who, N, T, D, A, gamma, lam, d_first_done, d_obs, d_act, d_mu, d_logp, d_rew, d_val, d_val_last, d_cost, d_vc,
                  d_vc_last, d_work, d_obs_c, d_act_c, d_mu_c, d_logp_c, d_ret, d_adv, d_cost_ret, d_adc, d_n_valid, x, stream);
}
