// gx_qcritic.h -- the cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) of the USL and the LPG learners as device
// code, for gx_usl.hip and gx_lpg.hip (through gx_qstep.h, which holds what their step and probe kernels and their host
// sides share).  The 768-thread workgroup, c_net's part of the LDS and its staging, Softplus' derivative, the 16-lane
// output sums and q_pass -- one forward pass over c_net, with or without the action terms and the backward pass: every
// trip of USL's iteration and both of LPG's passes.  Softplus, the MFMA chains of the hidden layers (forward, and backward
// against (1 - h2^2) w3) and the kernel that transposes the hidden layers into a path's workspace are gx_step.h's.
// The operation order of every function here is the one include/guardx_usl.h fixes; include/guardx_lpg.h refers to it.
// One translation unit per library: everything sits in an unnamed namespace.
#ifndef GX_QCRITIC_H
#define GX_QCRITIC_H
#include "gx_step.h"

namespace {

using namespace gx;

constexpr int kThreads = 768;  // 12 waves
constexpr int kAS = kMaxA + 1; // LDS row stride of the per-row action arrays

// waves that share c_net's unit tiles in a pass, and tiles per wave
GX_HD int q_waves(int HC) { return HC == 256 ? 8 : HC / 16; }
constexpr int q_tiles(int HC) { return HC == 256 ? 2 : 1; }

// LDS of the Q part, in floats: b1 b2 w3 b3 | W1 action block [A][HC] | P [16][HC + 4] | a [16][17] | s~ [16][17] |
// z3 [16] | live [16] | (HC == 64: Wt2 [64][64] | W2 [64][64])
struct QLds { int head, W1a, P, act, gt, z3, live, Wt2, W2, total; };
GX_HD QLds q_lds_layout(int A, int HC, int base)
{
    QLds L;
    int o = base;
    L.head = o; o += pad4(3 * HC + 1);
    L.W1a = o; o += A * HC;
    L.P = o; o += kEnv * (HC + 4);
    L.act = o; o += kEnv * kAS;
    L.gt = o; o += kEnv * kAS;
    L.z3 = o; o += kEnv;
    L.live = o; o += kEnv;
    L.Wt2 = o; o += HC == 64 ? 64 * 64 : 0;
    L.W2 = o; o += HC == 64 ? 64 * 64 : 0;
    L.total = o;
    return L;
}

// the derivative of Softplus (gx_step.h:softplus_f) as torch's backward evaluates it
GX_D float softplus_grad_f(float x)
{
    if (x > 20.0f) return 1.0f;
    const float e = exp_f(x);
    return __fdiv_rn(e, __fadd_rn(e, 1.0f));
}

// what the iteration needs besides LDS
struct QArgs {
    int D, A, niter, correct;
    float delta, eta, gscale;
    const float* cp;   // c_net as packed
    const float* cwt;  // its [pad4 D][HC] first-layer observation block and [HC][HC] second layer, transposed
};

// c_net's first layer over the observation columns, this wave's quarter of the units, at most two tiles at a time (the
// iteration's own registers stay live around it)
template <int HC>
GX_D void q_first_layer(const float* b1, const float* __restrict__ wt1, int quarter, const float* X, int XS, int Dp, float* P,
                        int c16, int kq)
{
    if constexpr (HC == 256) {
        hidden_layer<2, false>(b1, wt1, HC, 64 * quarter, X, XS, Dp, P, c16, kq);
        hidden_layer<2, false>(b1, wt1, HC, 64 * quarter + 32, X, XS, Dp, P, c16, kq);
    } else
        hidden_layer<HC / 64, false>(b1, wt1, HC, (HC / 4) * quarter, X, XS, Dp, P, c16, kq);
}

// 16 lane partials over the units 64 c + 4 l + j (c, then j ascending), fmaf chains from 0, folded by a butterfly
template <int H>
GX_D float dot16(const float* w, const float* h, int l)
{
    float pp = 0.0f;
#pragma unroll
    for (int c = 0; c < H / 64; ++c) {
        const float4 hv = *reinterpret_cast<const float4*>(h + 64 * c + 4 * l);
        const float4 wv = *reinterpret_cast<const float4*>(w + 64 * c + 4 * l);
        pp = fmaf(hv.x, wv.x, pp); pp = fmaf(hv.y, wv.y, pp); pp = fmaf(hv.z, wv.z, pp); pp = fmaf(hv.w, wv.w, pp);
    }
    pp = pp + __shfl_xor(pp, 8, 16);
    pp = pp + __shfl_xor(pp, 4, 16);
    pp = pp + __shfl_xor(pp, 2, 16);
    pp = pp + __shfl_xor(pp, 1, 16);
    return pp;
}

// c_net's small parts into LDS: b1 b2 w3 b3, the action block of W1 as [A][HC] rows, and at HC == 64 both forms of W2.
// Whole-workgroup call; the caller synchronises.
template <int HC>
GX_D void q_stage(float* lds, const QLds& L, const QArgs& q, int tid)
{
    const int in = q.D + q.A;
    const float* gb1 = q.cp + (size_t)HC * in;
    const float* gW2 = gb1 + HC;
    const float* gb2 = gW2 + HC * HC;
    const float* gw3 = gb2 + HC;
    float* hd = lds + L.head;
    for (int i = tid; i < HC; i += kThreads) { hd[i] = gb1[i]; hd[HC + i] = gb2[i]; hd[2 * HC + i] = gw3[i]; }
    if (tid == 0) hd[3 * HC] = gw3[HC];
    for (int i = tid; i < q.A * HC; i += kThreads) {
        const int k = i / HC, j = i - k * HC;
        lds[L.W1a + i] = q.cp[(size_t)j * in + q.D + k];
    }
    if (HC == 64)
        for (int i = tid; i < 64 * 64; i += kThreads) {
            const float w = gW2[i]; // W2[j][k], i = 64 j + k
            lds[L.W2 + i] = w;
            lds[L.Wt2 + (i & 63) * 64 + (i >> 6)] = w;
        }
    for (int i = tid; i < kEnv * kAS; i += kThreads) lds[L.act + i] = 0.0f; // (columns A .. stay zero: the padded k-steps)
}

// this lane's B operands of the action k-steps of its wave's tiles, W1[unit][D + 4 s + kq]: loaded once, used by every
// pass that takes the action terms
template <int HC>
GX_D void q_load_wa(float (&wa)[kMaxA / 4][q_tiles(HC)], const QArgs& q, int tid)
{
    constexpr int TT = q_tiles(HC);
    const int wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int in = q.D + q.A, col0 = 16 * TT * wave;
    if (wave < q_waves(HC)) {
#pragma unroll
        for (int s = 0; s < kMaxA / 4; ++s)
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                const int k = 4 * s + kq;
                wa[s][tt] = k < q.A ? q.cp[(size_t)(col0 + 16 * tt + c16) * in + q.D + k] : 0.0f;
            }
    }
}

// One pass over c_net on the 16 rows of the workgroup, in the order include/guardx_usl.h fixes.  On entry (after a
// barrier): P = the first layer's pre-activation over the observation columns, c_net's parts staged, and with ACT the
// rows' actions in lds[L.act] and wa from q_load_wa.  ACT: the first layer adds the A action terms on top of P (without
// it: none, h1 = tanh(P)).  bwd (workgroup-uniform): the backward GEMM against (1 - h2^2) w3, the (1 - h1^2) scale and
// the A output sums, which leave g~ in lds[L.gt].  On exit (after a barrier): z3 in lds[L.z3].  Whole-workgroup call.
template <int HC, bool ACT>
GX_D void q_pass(float* lds, const QLds& L, float* H1, float* H2, const QArgs& q, const float (&wa)[kMaxA / 4][q_tiles(HC)],
                 bool bwd, int tid)
{
    constexpr int HS = HC + 4, TT = q_tiles(HC), LB = TT == 2 ? 4 : kLB;
    const int NW = q_waves(HC);
    const int wave = tid >> 6, lw = tid & 63, c16 = lw & 15, kq = lw >> 4;
    const int A = q.A, in = q.D + A;
    const float* hd = lds + L.head;
    const float* b2 = hd + HC;
    const float* w3 = hd + 2 * HC;
    const float* P = lds + L.P;
    const float* act = lds + L.act;
    float* gt = lds + L.gt;
    float* z3 = lds + L.z3;
    const float* gW2 = q.cp + (size_t)HC * in + HC;
    const float* Bf = HC == 64 ? lds + L.Wt2 : q.cwt + (size_t)pad4(q.D) * HC; // forward: [k][unit]
    const float* Bb = HC == 64 ? lds + L.W2 : gW2;                             // backward: [unit j][k]
    const int col0 = 16 * TT * wave;

    // first layer: P, then (ACT) the A action terms on top of it; tanh
    if (wave < NW) {
        mfma_f4 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[tt][r] = P[(4 * kq + r) * HS + col0 + 16 * tt + c16];
        if constexpr (ACT) {
#pragma unroll
            for (int s = 0; s < kMaxA / 4; ++s)
                if (4 * s < A) {
                    const float av = act[c16 * kAS + 4 * s + kq];
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wa[s][tt], acc[tt], 0, 0, 0);
                }
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
    if (bwd && wave < NW) {
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
    if (bwd) {
        const int l = tid & 15;
        for (int task = tid >> 4; task < kEnv * A; task += kThreads / 16) {
            const int e = task / A, i = task - e * A;
            const float g = dot16<HC>(lds + L.W1a + i * HC, H1 + e * HS, l);
            if (l == 0) gt[e * kAS + i] = g;
        }
        wg_sync_lds();
    }
}

} // namespace
#endif // GX_QCRITIC_H
