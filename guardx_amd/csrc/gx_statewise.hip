// gx_statewise.hip -- libguardx_statewise.so (include/guardx_statewise.h): `ac.step(o_aug)` of the state-wise learners
// (SCPO: safe_rl_libX/scpo/scpo.py:640-720, scpo_core.py:158-200) for one control step over all envs, with the update of
// the running maximum cost M of the step just made in front of it.  o_aug = [obs | M] is D + 1 wide and feeds three
// two-hidden-layer tanh networks: the actor's mu_net, the critic v and the cost critic vc with its Softplus output.
//
// The arithmetic is the fused rollout's (gx_policy.h) and the checker's (oracle/gx_oracle.c:mlp_forward): every hidden
// unit is one v_mfma_f32_16x16x4_f32 chain over k ascending, started from its bias (that instruction accumulates exactly
// like a sequential fmaf chain, tools/probes/mfma_f32_probe.hip), then tanh_f; an output is 16 lane partials over the
// units 64 c + 4 l + j folded by the butterfly of head2_out; the noise, the action and log pi(a | o) are those of
// gx_policy_step.hip:policy_step_tail (gx_step.h:sample_row).  With a zero weight on the M column the actor and v therefore give the bits of
// rollout_policy on the D-wide observation.
//
// Organisation: a 384-thread workgroup (6 waves) serves 16 envs from ONE staged copy of their rows.  Waves 2 n and
// 2 n + 1 own network n (0 actor, 1 v, 2 vc) and one half of its hidden units each (H / 32 output tiles of 16 units per
// wave: the streaming form of gx_policy.h, polS_chain / polS_store).  The B operands are the hidden layers transposed
// to [k][unit] (gxs_prepare, into the caller's workspace, once per call): read by every workgroup, resident in L2,
// fetched eight k-steps ahead of the MFMAs that consume them.  The A operands (the augmented rows zero-padded to a
// multiple of four, then the first hidden layer) come from LDS.  At env_num = 2000 this is 125 workgroups on 256 CUs:
// the launch is bound by latency, not by throughput, which is why all three networks run side by side in one launch.
//
// Here: the LDS layout, the hidden layer in gx_policy.h's streaming tiling, the kernel and the C entry points.  Softplus,
// the sample / log-prob block, the transpose kernel and the host side's checks, dispatch and launches are gx_step.h's,
// shared with the other step libraries.
#include "../../include/guardx_statewise.h"
#include "gx_step.h"

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

constexpr int kThreads = 384;  // 6 waves: two per network
// the networks' input row is the augmented one, D_aug = D + 1 wide: at least one observation column and M
constexpr RowText kRowDaug = {2, ": D_aug must be >= 2 and A >= 1", ": D_aug too wide for the LDS tile"};

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
size_t lds_bytes(int Da, int A, int H, int HC) { return sizeof(float) * (size_t)lds_layout(Da, A, H, HC).total; }

__global__ void softplus_probe_kernel(int n, const float* __restrict__ x, float* __restrict__ y)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = softplus_f(x[i]);
}

// the kernel's view of gxs_step_args: this step's row blocks resolved on the host
struct StepArgs {
    StepCommon c;
    int D, Da, A;                     // D = Da - 1: the width of the env's own observation
    const float* vcp;
    float *M, *first;
    float *cost_inc_p, *M_after_p;    // row block t - 1
    float* vc;                        // row block t (tail: vc_last)
};

// one hidden layer of this wave's tiles in the streaming tiling of gx_policy.h (unit col0 + TT c16 + tt): acc = bias,
// chain over k ascending, tanh into the activation rows
template <int TT>
GX_D void hidden_layerS(const float* bias, const float* __restrict__ wt, int Hn, int col0, const float* Ain, int AS, int K,
                       float* out, int c16, int kq)
{
    mfma_f4 acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) { const float bb = bias[col0 + TT * c16 + tt]; acc[tt] = mfma_f4{bb, bb, bb, bb}; }
    polS_chain<TT>(acc, wt, Hn, col0, Ain, AS, K, c16, kq);
    polS_store<TT>(acc, out + col0, Hn + 4, c16, kq);
}

template <int H, int HC>
__global__ __launch_bounds__(kThreads) void statewise_step_kernel(StepArgs sa)
{
    const StepCommon& a = sa.c;
    constexpr int HS = H + 4, HSC = HC + 4;
    extern __shared__ float4 sw_lds4[];
    float* lds = reinterpret_cast<float*>(sw_lds4);
    const int D = sa.D, Da = sa.Da, A = sa.A, Dp = pad4(Da), XS = Dp + 1;
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
    mlp2_head_stage(lds + L.headC, sa.vcp, Da, 1, tid, kThreads, HC);
    const Mlp2Head hp = mlp2_head_view(lds + L.headP, A, H);
    const Mlp2Head hv = mlp2_head_view(lds + L.headV, 1, H);
    const Mlp2Head hc = mlp2_head_view(lds + L.headC, 1, HC);

    // prologue: the M update of the step just made (scpo.py:644-654, 713-715), then M as column D of the row
    if (tid < kEnv) {
        const int env = env0 + tid;
        float M = 0.0f;
        if (env < a.N) {
            M = sa.M[env];
            if (a.prologue) {
                const bool first = sa.first[env] != 0.0f;
                const float cost = a.cost_in[env], done = a.done_in[env];
                const float d = cost - M;
                const float inc = first ? cost : (d > 0.0f ? d : 0.0f);
                const float Mn = first ? cost : M + inc;
                sa.cost_inc_p[env] = inc;
                sa.M_after_p[env] = Mn;
                a.rew_p[env] = a.rew_in[env];
                a.cost_p[env] = cost;
                a.done_p[env] = done;
                const bool fin = done > 0.0f;
                M = fin ? 0.0f : Mn;
                sa.M[env] = M;
                sa.first[env] = fin ? 1.0f : 0.0f;
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
        if (net < 2) hidden_layerS<H / 32>((net ? hv : hp).b1, wtn, H, 16 * (H / 32) * half, X, XS, Dp, h1, c16, kq);
        else hidden_layerS<HC / 32>(hc.b1, wtn, HC, 16 * (HC / 32) * half, X, XS, Dp, h1, c16, kq);
    }
    wg_sync_lds();
    if (!skip) {
        if (net < 2) hidden_layerS<H / 32>((net ? hv : hp).b2, wtn + (size_t)Dp * H, H, 16 * (H / 32) * half, h1, HS, H, h2, c16, kq);
        else hidden_layerS<HC / 32>(hc.b2, wtn + (size_t)Dp * HC, HC, 16 * (HC / 32) * half, h1, HSC, HC, h2, c16, kq);
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
    // per env: the values, and (not in the tail) the noise, the action and log pi(a | o) of ac.step (scpo_core.py:189-198)
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            a.val[env] = outs[e * (A + 2) + A];
            sa.vc[env] = softplus_f(outs[e * (A + 2) + A + 1]);
            if (!a.tail) sample_row(a, A, gls, env, outs + e * (A + 2), nullptr);
        }
    }
    if (!a.tail) logstd_write(a.logstd, gls, A, tid);
}

struct StepKernel { template <int H, int HC> static const void* get() { return reinterpret_cast<const void*>(statewise_step_kernel<H, HC>); } };

} // namespace

extern "C" const char* gxs_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxs_build_id(void) { return GXS_BUILD_ID; } // guardx_amd/build.py:LIBRARIES["statewise"].source_hash()

extern "C" int64_t gxs_params_floats(int32_t D_aug, int32_t A, int32_t hidden)
{
    return D_aug >= kRowDaug.min ? params_floats(D_aug, A, hidden) : -1;
}

extern "C" int64_t gxs_work_floats(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden)
{
    return D_aug >= kRowDaug.min ? work_floats(D_aug, A, hidden, vc_hidden) : -1;
}

extern "C" gxs_status gxs_prepare(int32_t D_aug, int32_t A, int32_t hidden, int32_t vc_hidden, const float* d_params,
                                  const float* d_vc_params, float* d_work, void* stream)
{
    return prepare<StepKernel>(fail, "gxs_prepare", kRowDaug, lds_bytes, D_aug, A, hidden, vc_hidden, D_aug, d_params, d_vc_params,
                               d_work, stream);
}

extern "C" gxs_status gxs_policy_step(const gxs_step_args* g, void* stream)
{
    const gxs_status st = check_common(
        fail, "gxs_policy_step", g, kRowDaug, lds_bytes, &gxs_step_args::D_aug, &gxs_step_args::vc_hidden, &gxs_step_args::d_vc_params,
        [](const gxs_step_args&) { return true; }, "", [](const gxs_step_args& g, bool tail) {
            return g.d_M && g.d_first && (g.t == 0 || (g.d_cost_inc && g.d_M_after)) && (tail ? g.d_vc_last : g.d_vc);
        });
    if (st != GXS_OK || g->N == 0) return st;
    StepArgs a;
    const size_t tn = fill_common(*g, g->D_aug, a.c);
    a.Da = g->D_aug; a.D = g->D_aug - 1; a.A = g->A;
    a.vcp = g->d_vc_params;
    a.M = g->d_M; a.first = g->d_first;
    const size_t tp = a.c.prologue ? (size_t)(g->t - 1) * (size_t)g->N : 0;
    a.cost_inc_p = a.c.prologue ? g->d_cost_inc + tp : nullptr;
    a.M_after_p = a.c.prologue ? g->d_M_after + tp : nullptr;
    a.vc = a.c.tail ? g->d_vc_last : g->d_vc + tn;
    return q_launch(fail, "gxs_policy_step", q_kernel_for<StepKernel>(g->hidden, g->vc_hidden), g->N, kThreads, a,
                    lds_bytes(g->D_aug, g->A, g->hidden, g->vc_hidden), stream);
}

extern "C" gxs_status gxs_softplus_probe(int32_t n, const float* d_x, float* d_y, void* stream)
{
    if (!d_x || !d_y) return fail(GXS_ERR_ARG, "gxs_softplus_probe: null pointer");
    if (n < 0) return fail(GXS_ERR_ARG, "gxs_softplus_probe: n must be >= 0");
    if (n == 0) return GXS_OK;
    return launch_flat(fail, "gxs_softplus_probe", softplus_probe_kernel, n, 4096, stream, n, d_x, d_y);
}
