// gx_qstep.h -- what the step libraries of the learners with a Q critic (gx_usl.hip, gx_lpg.hip) share besides c_net
// itself (gx_qcritic.h) and what every step library shares (gx_step.h): the LDS layouts of the step and the probe kernel,
// the fields both StepArgs have, the front end of the step kernel (ac.step on the observation row, up to the sampled
// action) and of the probe kernel, and on the host the sizes, the probe's run and gx_step.h's prepare, checks and
// row-block arithmetic with c_net's own arguments filled in.  The host functions are templates like gx_step.h's.
// One translation unit per library: everything sits in an unnamed namespace.
#ifndef GX_QSTEP_H
#define GX_QSTEP_H
#include "gx_qcritic.h"

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

// what both step kernels' views of a gx?_step_args hold
struct QStepCommon : StepCommon {
    QArgs q;
    float *act_safe, *qc; // row block t
};

// The front end of a step kernel, `ac.step(o)` on the 16 rows of the workgroup: the heads and c_net's parts staged, the
// prologue's copies, the X tile written through to obs, the two hidden layers of the actor and the critic beside c_net's
// first layer over the observation columns (P), the output tasks, the value, the noise, the action, log pi(a | o) and
// logstd.  Returns true in the tail (the caller returns); otherwise after the barrier that hands U to c_net, with the
// sampled actions in lds[L.q.act].  Whole-workgroup call.  The Gaussian sample / log-prob block is gx_step.h:sample_row,
// the side libraries' one copy of gx_policy_step.hip:policy_step_tail's (two sites in all, where there were four).
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

    // prologue: the copies of the step just made and, in the one-episode form, its first-done bookkeeping
    if (a.prologue && tid < kEnv) {
        const int env = env0 + tid;
        if (env < a.N) {
            const float rew = a.rew_in[env], cost = a.cost_in[env], done = a.done_in[env];
            a.rew_p[env] = rew;
            a.cost_p[env] = cost;
            a.done_p[env] = done;
            if (a.ep.on) episode_book(a.ep, env, rew, cost, done);
        }
    }
    stage_rows(a, D, XS, X, env0, tid, kThreads); // (sanitised in the one-episode form: what c_net reads as well)
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
    const float* gls = a.params + msz_pi + msz_v;
    if (tid < kEnv) {
        const int e = tid, env = env0 + e;
        if (env < a.N) {
            a.val[env] = tail_row_unusable(a, D, env) ? 0.0f : outs[e * OS + A];
            if (!a.tail) sample_row(a, A, gls, env, outs + e * OS, lds + L.q.act + e * kAS);
        }
    }
    if (a.tail) return true;
    logstd_write(a.logstd, gls, A, tid);
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
// the gx?_q_floats and gx?_probe_work_floats entry points: -1 if unsupported
int64_t q_floats(int D, int A, int HC) { return (shape_ok(D, A) && width_ok(HC)) ? net_floats(D + A, 1, HC) : -1; }
int64_t probe_work_floats(int D, int A, int HC) { return (shape_ok(D, A) && width_ok(HC)) ? wt_floats(D, HC) : -1; }

size_t step_lds_bytes(int D, int A, int H, int HC) { return sizeof(float) * (size_t)lds_layout(D, A, H, HC).total; }
size_t probe_lds_bytes(int D, int A, int HC) { return sizeof(float) * (size_t)probe_lds_layout(D, A, HC).total; }

// gx?_prepare; StepK names the library's step kernels
template <class StepK, class Status>
Status q_prepare(FailFn<Status> fail, const char* who, int D, int A, int hidden, int c_hidden, const float* d_params,
                 const float* d_c_params, float* d_work, void* stream)
{
    return prepare<StepK>(fail, who, kRowD, step_lds_bytes, D, A, hidden, c_hidden, D + A, d_params, d_c_params, d_work, stream);
}

// the probe's own transpose of c_net into its scratch
template <class Status>
Status q_probe_transpose(FailFn<Status> fail, const char* who, int D, int A, int c_hidden, const float* d_c_params, float* d_work,
                         void* stream)
{
    return transpose(fail, who, wt_floats(D, c_hidden), d_c_params, d_c_params, d_work, D, A, c_hidden, c_hidden, D + A, 2, stream);
}

// a probe entry point after its own checks: the shape, the kernel's LDS, c_net's transpose, the launch over n rows
template <class ProbeK, class Status, class Args>
Status q_probe_run(FailFn<Status> fail, const char* who, int n, int D, int A, int c_hidden, const float* d_c_params, float* d_work,
                   Args& a, void* stream)
{
    Status st = check_shape(fail, who, kRowD, [](int d, int a, int, int hc) { return probe_lds_bytes(d, a, hc); }, D, A, 64, c_hidden);
    if (st != Status(kOk) || n == 0) return st;
    const void* kernel = q_kernel_hc<ProbeK, 0>(c_hidden);
    const size_t lds = probe_lds_bytes(D, A, c_hidden);
    st = raise_lds(fail, who, kernel, lds);
    if (st == Status(kOk)) st = q_probe_transpose(fail, who, D, A, c_hidden, d_c_params, d_work, stream);
    return st == Status(kOk) ? q_launch(fail, who, kernel, n, kThreads, a, lds, stream) : st;
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

// The checks gx?_policy_step makes before it launches (gx_step.h:check_common with c_net's and the corrected action's
// pointers).  own_range(g): the library's own range checks, named by the tail `own_text` of the message;
// own_ptrs(g, tail): its own pointers are there.
template <class Status, class G, class OwnRange, class OwnPtrs>
Status q_check_common(FailFn<Status> fail, const char* who, const G* g, OwnRange own_range, const char* own_text, OwnPtrs own_ptrs)
{
    return check_common(fail, who, g, kRowD, step_lds_bytes, &G::D, &G::c_hidden, &G::d_c_params, own_range, own_text,
                        [&](const G& s, bool tail) { return (tail || (s.d_act_safe && s.d_qc)) && own_ptrs(s, tail); });
}

// guardx_<library>_tail_probe: the tail launch alone on n caller-supplied rows, on the library's step kernels (StepK); A: its
// StepArgs, whose member c is the QStepCommon
template <class StepK, class A, class Status>
Status q_tail_probe(FailFn<Status> fail, const char* who, int n, int D, int Aw, int hidden, int c_hidden, const float* d_params,
                    const float* d_c_params, const float* d_work, const float* d_rows, float* d_obs_last, float* d_val_last,
                    void* stream)
{
    if (n < 0) return fail(Status(kErrArg), std::string(who) + ": n must be >= 0");
    const Status st = check_shape(fail, who, kRowD, step_lds_bytes, D, Aw, hidden, c_hidden);
    if (st != Status(kOk)) return st;
    if (!d_params || !d_c_params || !d_work || !d_rows || !d_obs_last || !d_val_last)
        return fail(Status(kErrArg), std::string(who) + ": null pointer");
    if (n == 0) return Status(kOk);
    A a = {};
    fill_tail_probe(a.c, n, d_params, d_work, d_rows, d_obs_last, d_val_last);
    a.c.q = q_args(D, Aw, false, 0.0f, 0.0f, d_c_params, d_work + 2 * wt_floats(D, hidden));
    return q_launch(fail, who, q_kernel_for<StepK>(hidden, c_hidden), n, kThreads, a, step_lds_bytes(D, Aw, hidden, c_hidden), stream);
}

// the shared fields of a checked gx?_step_args; returns the offset of row block t in a [T][N] array (0 in the tail)
template <class G>
size_t q_fill_common(const G& g, QStepCommon& c)
{
    const size_t tn = fill_common(g, g.D, c);
    c.q = q_args(g.D, g.A, g.correct != 0, g.delta, g.grad_scale, g.d_c_params, g.d_work + 2 * wt_floats(g.D, g.hidden));
    c.act_safe = c.tail ? nullptr : g.d_act_safe + tn * (size_t)g.A;
    c.qc = c.tail ? nullptr : g.d_qc + tn;
    return tn;
}

} // namespace
#endif // GX_QSTEP_H
