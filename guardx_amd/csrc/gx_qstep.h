// gx_qstep.h -- what the step libraries of the learners with a Q critic (gx_usl.hip, gx_lpg.hip) share besides c_net
// itself (gx_qcritic.h): the LDS layouts of the step and the probe kernel, the fields both StepArgs have, the front end
// of the step kernel (ac.step on the observation row, up to the sampled action) and of the probe kernel, and the host
// side -- sizes, shape checks, kernel dispatch, the checks and the row-block arithmetic of gx?_policy_step, the launches.
// The host functions are templates over the library's status enum (the two enums have equal values) and its public
// gx?_step_args (equal names for every shared field); they report through the library's own `fail`, passed first.
// One translation unit per library: everything sits in an unnamed namespace.
#ifndef GX_QSTEP_H
#define GX_QSTEP_H
#include "gx_qcritic.h"
#include <algorithm>
#include <string>

namespace {

using namespace gx;

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

// what both kernels' views of a gx?_step_args hold: this step's row blocks resolved on the host
struct QStepCommon {
    int N, env_offset;
    int tail, prologue;
    uint32_t seed0, seed1, tnoise;
    QArgs q;
    const float *params, *wt;
    const float* obs_rd;              // [N][D]
    const float *rew_in, *cost_in, *done_in;
    float *rew_p, *cost_p, *done_p;                               // row block t - 1
    float *obs, *act, *act_safe, *mu, *logp, *val, *qc, *logstd;  // row block t (tail: obs_last, val_last)
};

// The front end of a step kernel, `ac.step(o)` on the 16 rows of the workgroup: the heads and c_net's parts staged, the
// prologue's copies, the X tile written through to obs, the two hidden layers of the actor and the critic beside c_net's
// first layer over the observation columns (P), the output tasks, the value, the noise, the action, log pi(a | o) and
// logstd.  Returns true in the tail (the caller returns); otherwise after the barrier that hands U to c_net, with the
// sampled actions in lds[L.q.act].  Whole-workgroup call.  The Gaussian sample / log-prob block is
// gx_policy_step.hip:policy_step_tail's and is written out at four sites: there, in gx_statewise.hip, in
// gx_safelayer.hip and here (five while gx_usl.hip and gx_lpg.hip each held this front end).
template <int H, int HC>
GX_D bool q_step_front(float* lds, const Lds& L, const QStepCommon& a, int tid)
{
    constexpr int HS = H + 4;
    const int D = a.q.D, A = a.q.A, Dp = pad4(D), XS = Dp + 1, OS = A + 1;
    float* X = lds + L.X;
    float* H1 = lds + L.U;
    float* H2 = H1 + 2 * kEnv * HS;
    float* outs = lds + L.outs;
    const int wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
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
    if (a.tail) return true;
    if (blockIdx.x == 0 && tid >= 64 && tid < 64 + A) a.logstd[tid - 64] = log_f(exp_f(gls[tid - 64]));
    wg_sync_lds(); // the actions; from here U is c_net's
    return false;
}

// The front end of a probe kernel on the rows row0 .. row0 + rows - 1 of obs [n][D] and act [n][A]: c_net's parts staged,
// the X tile, the action rows, P on the waves 8 .. 11; returns after the barrier.  Whole-workgroup call.
template <int HC>
GX_D void q_probe_front(float* lds, const Lds& L, const QArgs& q, const float* obs, const float* act, int row0, int rows, int tid)
{
    const int D = q.D, A = q.A, Dp = pad4(D), XS = Dp + 1;
    float* X = lds + L.X;
    const int wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    q_stage<HC>(lds, L.q, q, tid);
    for (int i = tid; i < kEnv * XS; i += kThreads) {
        const int e = i / XS, k = i - e * XS;
        X[i] = (k < D && e < rows) ? obs[(size_t)(row0 + e) * D + k] : 0.0f;
    }
    wg_sync_lds(); // (q_stage zeroes the action rows)
    for (int i = tid; i < rows * A; i += kThreads) {
        const int e = i / A, k = i - e * A;
        lds[L.q.act + e * kAS + k] = act[(size_t)(row0 + e) * A + k];
    }
    if (wave >= 8) q_first_layer<HC>(lds + L.q.head, q.cwt, wave & 3, X, XS, Dp, lds + L.q.P, c16, kq);
    wg_sync_lds();
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
// the values of gxu_status and gxp_status
constexpr int kOk = 0, kErrArg = 1, kErrUnsupported = 2, kErrHip = 4;
// the library's `fail`: records the message as the calling thread's last error and returns the status
template <class Status>
using FailFn = Status (*)(Status, const std::string&);

constexpr size_t kLdsMax = 160 * 1024;

bool width_ok(int H) { return H == 64 || H == 128 || H == 192 || H == 256; }
bool shape_ok(int D, int A) { return D >= 1 && A >= 2 && A <= kMaxA && !(A & 1); }

// the four gx?_*_floats entry points: -1 if unsupported
int64_t params_floats(int D, int A, int H) { return (shape_ok(D, A) && width_ok(H)) ? net_floats(D, A, H) + net_floats(D, 1, H) + A : -1; }
int64_t q_floats(int D, int A, int HC) { return (shape_ok(D, A) && width_ok(HC)) ? net_floats(D + A, 1, HC) : -1; }
int64_t work_floats(int D, int A, int H, int HC)
{
    return (shape_ok(D, A) && width_ok(H) && width_ok(HC)) ? 2 * wt_floats(D, H) + wt_floats(D, HC) : -1;
}
int64_t probe_work_floats(int D, int A, int HC) { return (shape_ok(D, A) && width_ok(HC)) ? wt_floats(D, HC) : -1; }

size_t step_lds_bytes(int D, int A, int H, int HC) { return sizeof(float) * (size_t)lds_layout(D, A, H, HC).total; }
size_t probe_lds_bytes(int D, int A, int HC) { return sizeof(float) * (size_t)probe_lds_layout(D, A, HC).total; }

template <class Status>
Status check_shape(FailFn<Status> fail, const char* who, int D, int A, int H, int HC, bool probe)
{
    if (D < 1 || A < 1) return fail(Status(kErrArg), std::string(who) + ": D and A must be >= 1");
    if (!width_ok(H) || !width_ok(HC))
        return fail(Status(kErrUnsupported), std::string(who) + ": hidden width not in {64, 128, 192, 256}");
    if (!shape_ok(D, A)) return fail(Status(kErrUnsupported), std::string(who) + ": needs an even action width <= 16");
    if (D > 65536 || (probe ? probe_lds_bytes(D, A, HC) : step_lds_bytes(D, A, H, HC)) > kLdsMax)
        return fail(Status(kErrUnsupported), std::string(who) + ": D too wide for the LDS tile");
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

// Kernel dispatch.  K names a library's kernels: K::get<H, HC>() is the address of the instance (a probe kernel has no H
// and ignores it).
template <class K, int H>
const void* q_kernel_hc(int HC)
{
    switch (HC) {
    case 64: return K::template get<H, 64>();
    case 128: return K::template get<H, 128>();
    case 192: return K::template get<H, 192>();
    default: return K::template get<H, 256>();
    }
}
template <class K>
const void* q_kernel_for(int H, int HC)
{
    switch (H) {
    case 64: return q_kernel_hc<K, 64>(HC);
    case 128: return q_kernel_hc<K, 128>(HC);
    case 192: return q_kernel_hc<K, 192>(HC);
    default: return q_kernel_hc<K, 256>(HC);
    }
}

// `last` = hipGetLastError() after a <<< >>> launch or the result of hipLaunchKernel
template <class Status>
Status q_launched(FailFn<Status> fail, const char* who, hipError_t last)
{
    return last == hipSuccess ? Status(kOk) : fail(Status(kErrHip), std::string(who) + " launch failed: " + hipGetErrorString(last));
}

// one workgroup per 16 rows
template <class Status, class Args>
Status q_launch(FailFn<Status> fail, const char* who, const void* kernel, int n, Args& a, size_t lds, void* stream)
{
    void* kargs[] = {&a};
    return q_launched(fail, who, hipLaunchKernel(kernel, dim3((unsigned)((n + kEnv - 1) / kEnv)), dim3(kThreads), kargs, lds,
                                                  (hipStream_t)stream));
}

// the transposed hidden layers of `first` = 0: the three networks, 2: c_net alone, into d_work (n floats)
template <class Status>
Status q_transpose(FailFn<Status> fail, const char* who, long long n, const float* d_params, const float* d_c_params, float* d_work,
                   int D, int A, int H, int HC, int first, void* stream)
{
    const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(usl_transpose_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_params, d_c_params, d_work, D, A,
                       H, HC, first);
    return q_launched(fail, who, hipGetLastError());
}

// gx?_prepare; StepK names the library's step kernels
template <class StepK, class Status>
Status q_prepare(FailFn<Status> fail, const char* who, int D, int A, int hidden, int c_hidden, const float* d_params,
                 const float* d_c_params, float* d_work, void* stream)
{
    if (!d_params || !d_c_params || !d_work) return fail(Status(kErrArg), std::string(who) + ": null pointer");
    Status st = check_shape(fail, who, D, A, hidden, c_hidden, false);
    if (st != Status(kOk)) return st;
    st = raise_lds(fail, who, q_kernel_for<StepK>(hidden, c_hidden), step_lds_bytes(D, A, hidden, c_hidden));
    if (st != Status(kOk)) return st;
    return q_transpose(fail, who, work_floats(D, A, hidden, c_hidden), d_params, d_c_params, d_work, D, A, hidden, c_hidden, 0, stream);
}

// the probe's own transpose of c_net into its scratch
template <class Status>
Status q_probe_transpose(FailFn<Status> fail, const char* who, int D, int A, int c_hidden, const float* d_c_params, float* d_work,
                         void* stream)
{
    return q_transpose(fail, who, wt_floats(D, c_hidden), d_c_params, d_c_params, d_work, D, A, c_hidden, c_hidden, 2, stream);
}

// a probe entry point after its own checks: the shape, the kernel's LDS, c_net's transpose, the launch over n rows
template <class ProbeK, class Status, class Args>
Status q_probe_run(FailFn<Status> fail, const char* who, int n, int D, int A, int c_hidden, const float* d_c_params, float* d_work,
                   Args& a, void* stream)
{
    Status st = check_shape(fail, who, D, A, 64, c_hidden, true);
    if (st != Status(kOk) || n == 0) return st;
    const void* kernel = q_kernel_hc<ProbeK, 0>(c_hidden);
    const size_t lds = probe_lds_bytes(D, A, c_hidden);
    st = raise_lds(fail, who, kernel, lds);
    if (st == Status(kOk)) st = q_probe_transpose(fail, who, D, A, c_hidden, d_c_params, d_work, stream);
    return st == Status(kOk) ? q_launch(fail, who, kernel, n, a, lds, stream) : st;
}

// QArgs without the iteration's own niter and eta (USL sets them)
QArgs q_args(int D, int A, bool correct, float delta, float gscale, const float* cp, const float* cwt)
{
    QArgs q;
    q.D = D; q.A = A; q.niter = 0; q.correct = correct;
    q.delta = delta; q.eta = 0.0f; q.gscale = gscale;
    q.cp = cp; q.cwt = cwt;
    return q;
}

// The checks gx?_policy_step makes before it launches.  own_range(g): the library's own range checks, named by the tail
// `own_text` of the message; own_ptrs(g, tail): its own pointers are there.
template <class Status, class G, class OwnRange, class OwnPtrs>
Status q_check_common(FailFn<Status> fail, const char* who, const G* g, OwnRange own_range, const char* own_text, OwnPtrs own_ptrs)
{
    const std::string w(who);
    if (!g) return fail(Status(kErrArg), w + ": null argument struct");
    if (g->struct_size != sizeof(G)) return fail(Status(kErrArg), w + ": struct_size mismatch");
    if (g->N < 0 || g->T < 1 || g->t < 0 || g->t > g->T || g->env_offset < 0 || !own_range(*g))
        return fail(Status(kErrArg), w + ": N must be >= 0, T >= 1, t in [0, T], env_offset >= 0" + own_text);
    const Status st = check_shape(fail, who, g->D, g->A, g->hidden, g->c_hidden, false);
    if (st != Status(kOk)) return st;
    const bool tail = g->t == g->T, prologue = g->t > 0;
    if (!g->d_params || !g->d_c_params || !g->d_work || !own_ptrs(*g, tail)) return fail(Status(kErrArg), w + ": null pointer");
    if (prologue ? (!g->d_obs_rd || !g->d_rew_in || !g->d_cost_in || !g->d_done_in || !g->d_rew || !g->d_cost || !g->d_done)
                 : !g->d_obs0)
        return fail(Status(kErrArg), w + ": null pointer");
    if (tail ? (!g->d_obs_last || !g->d_val_last)
             : (!g->d_obs || !g->d_act || !g->d_act_safe || !g->d_mu || !g->d_logp || !g->d_val || !g->d_qc || !g->d_logstd))
        return fail(Status(kErrArg), w + ": null pointer");
    return Status(kOk);
}

// the shared fields of a checked gx?_step_args; returns the offset of row block t in a [T][N] array (0 in the tail)
template <class G>
size_t q_fill_common(const G& g, QStepCommon& c)
{
    const size_t N = (size_t)g.N, D = (size_t)g.D, A = (size_t)g.A;
    c.N = g.N; c.env_offset = g.env_offset;
    c.tail = g.t == g.T; c.prologue = g.t > 0;
    c.seed0 = g.seed[0]; c.seed1 = g.seed[1]; c.tnoise = g.step0 + (uint32_t)g.t;
    c.q = q_args(g.D, g.A, g.correct != 0, g.delta, g.grad_scale, g.d_c_params, g.d_work + 2 * wt_floats(g.D, g.hidden));
    c.params = g.d_params; c.wt = g.d_work;
    c.obs_rd = c.prologue ? g.d_obs_rd : g.d_obs0;
    c.rew_in = g.d_rew_in; c.cost_in = g.d_cost_in; c.done_in = g.d_done_in;
    const size_t tp = c.prologue ? (size_t)(g.t - 1) * N : 0;
    c.rew_p = c.prologue ? g.d_rew + tp : nullptr; c.cost_p = c.prologue ? g.d_cost + tp : nullptr;
    c.done_p = c.prologue ? g.d_done + tp : nullptr;
    if (c.tail) {
        c.obs = g.d_obs_last; c.val = g.d_val_last;
        c.act = c.act_safe = c.mu = c.logp = c.qc = c.logstd = nullptr;
        return 0;
    }
    const size_t tn = (size_t)g.t * N;
    c.obs = g.d_obs + tn * D; c.act = g.d_act + tn * A; c.act_safe = g.d_act_safe + tn * A;
    c.mu = g.d_mu + tn * A; c.logp = g.d_logp + tn; c.val = g.d_val + tn;
    c.qc = g.d_qc + tn; c.logstd = g.d_logstd;
    return tn;
}

} // namespace
#endif // GX_QSTEP_H
