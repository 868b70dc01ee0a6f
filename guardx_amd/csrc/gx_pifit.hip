// gx_pifit.hip -- libguardx_pifit.so (include/guardx_pifit.h): the first-order learners' fit of the Gaussian MLP actor (hidden
// width 64) by Adam on the clipped surrogate, with their early stop on kl, on the caller's stream and without a host
// synchronisation.  The header fixes the arithmetic; this file is its order of work, two launches per iteration:
//
//   grad_kernel<KS1>  gx_pgrad.hip:grad_kernel for one gradient, restated: a persistent grid of 4-wave workgroups; workgroup g
//                  walks the 64-row tiles g, g + grid, ... of obs.  LDS holds W2, W3 and the biases, the tile of obs and its
//                  activations; each lane keeps its KS1 operands of W1 in registers.  Per tile, with a workgroup barrier (LDS
//                  only) after each stage:
//                    1  z1 = o W1' + b1 -> h1                       (K = pad4 D; four chains: sum_acc)
//                    2  z2 = h1 W2' + b2 -> h2                      (K = 64; four chains)
//                    3  mu = h2 W3' + b3                            (wave w: rows 16 w ..)
//                    R  lane 4 i + p of wave w: row 16 w + i, the actions p, p + 4, ...: logp and ratio in the line search's
//                       words, which side of [lo, hi] ratio left, the row weight c (0 by selection where the clipped branch
//                       is the smaller), this lane's entries of dmu (0 for rows past B) and its terms of dlog_std; the row's
//                       terms of the loss, of cf and of kl to the lane's float64 sums
//                    4  gz2 = (dmu W3)(1 - h2^2)  (K = 16, the padded action width);  gW3 += dmu' h2, gb3 += dmu' 1
//                    5  gW2 += gz2' h1, gb2 += gz2' 1;  gz1 = (gz2 W2)(1 - h1^2) -> where h2 was
//                    6  gW1 += gz1' o, gb1 += gz1' 1
//                  The sums over a tile's 64 rows start from zero and are added to the workgroup's running sums after the
//                  stage, so that no float32 chain is longer than a tile.  The next tile's rows are loaded into registers
//                  while this one is computed.  The workgroup writes one partial vector of P floats (its log_std entries
//                  zero) and kSums float64: the sums of the loss, cf and kl and 16 of dlog_std.  In a fit every launch but
//                  the call's first returns at once when the stop flag is set, and so leaves the partial sums of the
//                  stopping iteration where they are.
//   step_kernel    one lane per entry of theta, ceil(P / 256) workgroups.  Every workgroup adds the workgroups' sums of the
//                  loss, cf and kl itself, in workgroup order through LDS, and takes the stop decision from kl: the same
//                  data in the same order, data that no workgroup of this launch writes, so all decide alike and none reads
//                  the flag to decide.  Not stopped: the partial vectors' entries (the float64 ones for log_std) added in
//                  workgroup order in float64, rounded once: g; then Adam in place, with t = the count the call started from
//                  (a slot that grad_kernel's first launch fills and nobody writes after) + i + 1: a call that has not
//                  stopped by iteration i has taken i steps.  Lane 0 of workgroup 0 alone reads and writes the flag, the
//                  count, stop_iter, steps and the traces; after a stop it finds the flag set and writes nothing.  The same
//                  kernel serves gxa_gradient (no Adam: g and the three means are written).
// No atomics anywhere: the same arguments give the same bits.  tanh_act, sum_acc and the tile code are gx_pgrad.hip's, Adam is
// gx_vfit.hip's, restated (a shared header would move the build ids of the libraries that hold them).
#include "../../include/guardx_pifit.h"
#include "gx_policy.h"
#include <cmath>
#include <string>

#ifndef GXA_BUILD_ID
#define GXA_BUILD_ID "unknown"
#endif

namespace {

using gx::mfma_f4;
using gx::wg_sync_lds;

thread_local std::string g_err;

gxa_status fail(gxa_status st, const std::string& msg)
{
    g_err = msg;
    return st;
}

constexpr int kH = gx::kPolHd;   // hidden width
constexpr int kTile = 64;        // rows of obs per tile
constexpr int kThreads = 256;    // four waves; wave w owns the hidden units 16 w .. 16 w + 15 and the rows 16 w .. 16 w + 15
constexpr int kAp = 16;          // the action width padded to one MFMA tile
constexpr int kSW = 66;          // LDS row stride of everything 64 wide: 16 rows x 2 k of a ds_read_b32 group hit 32 banks
constexpr int kSU = 18;          // ... of mu and dmu (64 x 16)
constexpr int kDefaultWg = 256;  // one workgroup per CU of the MI355X: the LDS image is over half a CU's 160 KB
constexpr int kMaxWg = 4096;
constexpr int kMaxD = 128;
constexpr int kAcc = 4;          // interleaved chains of a forward product (stages 1 to 3): see sum_acc
constexpr int kSums = 4 + kAp;   // float64 per workgroup: the sums of the loss's terms, of cf's, of l - logp, (unused), dlog_std
constexpr int kDbl = 3 * kAp + 4 * kSums;   // float64 at the head of LDS: log_std, 1 / v1, 1 / (2 v1) per action; the waves' sums
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// row stride of the obs tile: at least the 16 NT1 columns stage 6 reads, = 2 mod 32
constexpr int nt1_of(int KS1) { return (KS1 + 3) / 4; }
constexpr int obs_stride(int KS1) { return (16 * nt1_of(KS1) - 2 + 31) / 32 * 32 + 2; }
// W2, W3, b1 b2 b3, O, H1, H2 (then gz1), GZ2, MU, DMU
constexpr int lds_floats(int KS1)
{
    return 2 * kDbl + kH * kSW + kAp * kSW + 2 * kH + kAp + kTile * obs_stride(KS1) + 3 * kTile * kSW + 2 * kTile * kSU;
}

int64_t param_count(int D, int A, int h) { return (int64_t)A + (int64_t)h * D + h + (int64_t)h * h + h + (int64_t)A * h + A; }
int tiles_of(int B) { return (int)(((int64_t)B + kTile - 1) / kTile); }
int default_workgroups(int B) { return tiles_of(B) < kDefaultWg ? tiles_of(B) : kDefaultWg; }

struct GradArgs {
    int B, D, A, tiles;
    const float *theta, *obs, *act, *adv, *logp_old;
    int logp_loss, clip;    // the loss is logp's, not the ratio's; the ratio's is clipped to [lo, hi]
    float lo, hi;
    int first;              // the call's first launch: the flag is not read
    const int32_t* flag;    // null outside a fit
    long long* count;       // a fit's first launch: count[1] = count[0]; else null
    double* ent;            // where ent goes, or null
    float* partial;         // [grid][P]
    double* sums;           // [grid][kSums]
    double inv_b;           // 1 / B
};

#define GXA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__device__ __forceinline__ mfma_f4 splat(float v) { return mfma_f4{v, v, v, v}; }

// gx_fisher.hip:sum_acc: the sums over a layer's inputs are kAcc chains, k-step s on chain s mod kAcc, the bias on chain 0,
// added pairwise.  One chain rounds 64 times at the size of its running sum; four round 16 times each at half that size,
// which halves the error of the sum (the Fisher product's record: 7 x its yardstick at B = 1 with one chain, 1.3 x with four).
__device__ __forceinline__ mfma_f4 sum_acc(const mfma_f4 (&a)[kAcc])
{
    static_assert(kAcc == 4, "pairwise over four");
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// gx_fisher.hip:tanh_act: gx::tanh_f has a small absolute error, which below |x| ~ 0.6 is a large relative one, and here every
// activation multiplies gradients; there the odd polynomial x + x^3 P(x^2) of the Cephes single-precision tanh (public
// domain, S. Moshier) takes over: 2.3 ulp at worst over the whole line
__device__ __forceinline__ float tanh_act(float x)
{
    const float z = x * x;
    float p = fmaf(z, -5.70498872745e-3f, 2.06390887954e-2f);
    p = fmaf(z, p, -5.37397155531e-2f);
    p = fmaf(z, p, 1.33314422036e-1f);
    p = fmaf(z, p, -3.33332819422e-1f);
    const float small = fmaf(z * x, p, x);                      // x = -0: (+0) + (-0) = +0, hence the copysignf
    return fabsf(x) < 0.625f ? copysignf(small, x) : gx::tanh_f(x);
}

// test infrastructure (gxa_tanh_act): tanh_act by itself, one lane per element
__global__ __launch_bounds__(kThreads) void tanh_act_kernel(int n, const float* __restrict__ x, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = tanh_act(x[i]);
}

template <int KS1>
__global__ __launch_bounds__(kThreads) void grad_kernel(GradArgs a)
{
    if (a.flag && !a.first && a.flag[0]) return;                // stopped: uniform over the grid, before any barrier
    constexpr int NT1 = nt1_of(KS1), SO = obs_stride(KS1);
    extern __shared__ double lds_d[];
    double* const LS = lds_d;              // log_std
    double* const IV = LS + kAp;           // 1 / v1
    double* const I2 = IV + kAp;           // 1 / (2 v1)
    double* const WS = I2 + kAp;           // [wave][kSums]
    float* const W2 = reinterpret_cast<float*>(lds_d + kDbl);
    float* const W3 = W2 + kH * kSW;       // [kAp][kSW], the rows past A zero
    float* const b1 = W3 + kAp * kSW;
    float* const b2 = b1 + kH;
    float* const b3 = b2 + kH;
    float* const O = b3 + kAp;
    float* const H1 = O + kTile * SO;
    float* const H2 = H1 + kTile * kSW;    // h2, then gz1
    float* const GZ2 = H2 + kTile * kSW;
    float* const MU = GZ2 + kTile * kSW;
    float* const DMU = MU + kTile * kSU;   // the columns past A zero

    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int D = a.D, A = a.A;
    const int P = A + kH * D + kH + kH * kH + kH + A * kH + A;
    const int oW1 = A, ob1 = oW1 + kH * D, oW2 = ob1 + kH, ob2 = oW2 + kH * kH, oW3 = ob2 + kH, ob3 = oW3 + A * kH;
    const float* __restrict__ th = a.theta;

    // ---- the LDS image of theta, and this lane's W1 operands
    static_assert(kH * kH % kThreads == 0 && kAp * kH % kThreads == 0, "whole passes");
#pragma unroll
    for (int p = 0; p < kH * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W2[(i >> 6) * kSW + (i & 63)] = th[oW2 + i];
    }
#pragma unroll
    for (int p = 0; p < kAp * kH / kThreads; ++p) {
        const int i = tid + kThreads * p;
        W3[(i >> 6) * kSW + (i & 63)] = (i >> 6) < A ? th[oW3 + i] : 0.0f;
    }
    if (tid < kH) {
        b1[tid] = th[ob1 + tid];
        b2[tid] = th[ob2 + tid];
    }
    if (tid < kAp) {
        const bool in = tid < A;
        b3[tid] = in ? th[ob3 + tid] : 0.0f;
        const double ls = in ? (double)th[tid] : 0.0;
        const double v1 = exp(2.0 * ls);
        LS[tid] = ls;
        IV[tid] = 1.0 / v1;
        I2[tid] = 1.0 / (2.0 * v1);
    }
    for (int i = tid; i < kTile * SO; i += kThreads) O[i] = 0.0f;      // the columns past D stay zero
    for (int i = tid; i < kTile * kSU; i += kThreads) DMU[i] = 0.0f;   // the columns past A stay zero
    float w1[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) {
        const int k = 4 * s + q;
        w1[s] = k < D ? th[oW1 + (16 * w + c) * D + k] : 0.0f;
    }
    // element tid + 256 j of a tile (its rows are contiguous in obs) sits in row (tid + 256 j) / D, column (tid + 256 j) % D of O:
    // walked from j = 0 by steps of 256 = dr D + dc at every tile (a table of KS1 offsets per lane costs KS1 registers)
    const int row0 = tid / D, col0 = tid % D, dr = kThreads / D, dc = kThreads % D;
    float pf[KS1];
    auto load_tile = [&](int t) {
        const float* __restrict__ src = a.obs + (size_t)t * kTile * D;
        const int rows = a.B - t * kTile < kTile ? a.B - t * kTile : kTile;
        const int n = rows * D;                                 // nothing past row B - 1 is read
#pragma unroll
        for (int j = 0; j < KS1; ++j) pf[j] = tid + kThreads * j < n ? src[tid + kThreads * j] : 0.0f;
    };

    // the workgroup's running sums: W1 (NT1 column tiles), W2 (4), W3 (this wave's units), the three biases
    mfma_f4 rW1[NT1], rW2[4], rW3 = splat(0.0f), rb1 = splat(0.0f), rb2 = splat(0.0f), rb3 = splat(0.0f);
#pragma unroll
    for (int n = 0; n < NT1; ++n) rW1[n] = splat(0.0f);
#pragma unroll
    for (int n = 0; n < 4; ++n) rW2[n] = splat(0.0f);
    const int row = tid >> 2, part = tid & 3;                   // stage R: row 16 w + (lane >> 2), the actions part, part + 4, ...
    double run[3] = {0.0, 0.0, 0.0};                            // this lane's sums of the loss's terms, cf's, l - logp (part 0 only)
    double dls[4] = {0.0, 0.0, 0.0, 0.0};                       // ... of its actions' terms of dlog_std

    int t = blockIdx.x;
    if (t < a.tiles) load_tile(t);
    wg_sync_lds();                                              // O and DMU are zero before the first rows land in them
    if (blockIdx.x == 0 && tid == 0) {
        if (a.ent) {
            double ent = 0.0;
            for (int k = 0; k < A; ++k) ent += LS[k] + 0.5 + kHalfLog2Pi;
            a.ent[0] = ent;
        }
        if (a.count) a.count[1] = a.count[0];                   // the count the call starts from: read by every step_kernel
    }
    while (t < a.tiles) {
        {
            int rr = row0, cc = col0;
#pragma unroll
            for (int j = 0; j < KS1; ++j) {
                if (rr < kTile) O[rr * SO + cc] = pf[j];
                cc += dc;
                rr += dr;
                if (cc >= D) {
                    cc -= D;
                    ++rr;
                }
            }
        }
        const int tn = t + gridDim.x;
        if (tn < a.tiles) load_tile(tn);                        // in flight during the stages
        // this lane's share of its row of the batch, in flight too; nothing past row B - 1 is read
        const int64_t grow = (int64_t)t * kTile + row;
        const bool valid = grow < a.B;
        float r_adv = 0.0f, r_lpo = 0.0f, r_act[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ac = part + 4 * k;
            r_act[k] = valid && ac < A ? a.act[grow * A + ac] : 0.0f;
        }
        if (valid) {
            r_adv = a.adv[grow];
            r_lpo = a.logp_old[grow];
        }
        wg_sync_lds();

        float d1[4][4], d2[4][4];                               // 1 - h1^2, 1 - h2^2 of this lane's outputs
        // ---- 1
        {
            const float bz = b1[16 * w + c];
            mfma_f4 acc[4][kAcc];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i == 0 ? bz : 0.0f);
#pragma unroll
            for (int s = 0; s < KS1; ++s) {
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb][s % kAcc] = GXA_MFMA(O[(16 * rb + c) * SO + 4 * s + q], w1[s], acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[r]);
                    d1[rb][r] = fmaf(-h, h, 1.0f);
                    H1[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                }
            }
        }
        wg_sync_lds();
        // ---- 2
        {
            const float bz = b2[16 * w + c];
            mfma_f4 acc[4][kAcc];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int i = 0; i < kAcc; ++i) acc[rb][i] = splat(i == 0 ? bz : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s) {
                const float bw = W2[(16 * w + c) * kSW + 4 * s + q];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    acc[rb][s % kAcc] = GXA_MFMA(H1[(16 * rb + c) * kSW + 4 * s + q], bw, acc[rb][s % kAcc]);
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const mfma_f4 z = sum_acc(acc[rb]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float h = tanh_act(z[r]);
                    d2[rb][r] = fmaf(-h, h, 1.0f);
                    H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = h;
                }
            }
        }
        wg_sync_lds();
        // ---- 3: this wave's 16 rows
        {
            mfma_f4 acc[kAcc];
#pragma unroll
            for (int i = 0; i < kAcc; ++i) acc[i] = splat(i == 0 ? b3[c] : 0.0f);
#pragma unroll
            for (int s = 0; s < kH / 4; ++s)
                acc[s % kAcc] = GXA_MFMA(H2[(16 * w + c) * kSW + 4 * s + q], W3[c * kSW + 4 * s + q], acc[s % kAcc]);
            const mfma_f4 m = sum_acc(acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) MU[(16 * w + 4 * q + r) * kSU + c] = m[r];
        }
        wg_sync_lds();
        // ---- R: the rows
        {
            double lps = 0.0, da[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ac = part + 4 * k;
                da[k] = 0.0;
                if (ac < A) {
                    da[k] = (double)r_act[k] - (double)MU[row * kSU + ac];
                    lps += -(da[k] * da[k]) * I2[ac] - LS[ac] - kHalfLog2Pi;
                }
            }
            lps += __shfl_xor(lps, 1);
            lps += __shfl_xor(lps, 2);
            const float lp = (float)lps;
            const float diff = lp - r_lpo;
            const float ratio = (float)exp((double)diff);
            const bool above = a.clip && ratio > a.hi, below = a.clip && ratio < a.lo;
            const bool active = !((r_adv > 0.0f && above) || (r_adv < 0.0f && below));
            const float ra = ratio * r_adv;
            const float ca = (below ? a.lo : above ? a.hi : ratio) * r_adv;   // torch.clamp: a NaN ratio stays one
            const float term = a.logp_loss ? lp * r_adv : ca < ra ? ca : ra;  // torch.min of the two branches
            const double cfull = a.logp_loss ? -(double)r_adv * a.inv_b : -((double)r_adv * (double)ratio) * a.inv_b;
            const double cd = (double)(active ? (float)cfull : 0.0f);         // selection, never a product with zero
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ac = part + 4 * k;
                if (ac < A) {
                    const double iv = IV[ac];
                    DMU[row * kSU + ac] = valid ? (float)((cd * da[k]) * iv) : 0.0f;
                    dls[k] += valid ? cd * ((da[k] * da[k]) * iv - 1.0) : 0.0;
                }
            }
            const bool on = valid && part == 0;
            run[0] += on ? (double)term : 0.0;
            run[1] += on && (above || below) ? 1.0 : 0.0;
            run[2] += on ? (double)(r_lpo - lp) : 0.0;
        }
        wg_sync_lds();
        // ---- 4
        {
            mfma_f4 z[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kAp / 4; ++s) {
                const float bv = W3[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXA_MFMA(DMU[(16 * rb + c) * kSU + 4 * s + q], bv, z[rb]);
            }
            mfma_f4 t3 = splat(0.0f), tb = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = DMU[(4 * s + q) * kSU + c];
                t3 = GXA_MFMA(av, H2[(4 * s + q) * kSW + 16 * w + c], t3);
                tb = GXA_MFMA(av, 1.0f, tb);
            }
            rW3 += t3;
            rb3 += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int r = 0; r < 4; ++r) GZ2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d2[rb][r];
        }
        wg_sync_lds();
        // ---- 5
        {
            mfma_f4 t2[4], tb = splat(0.0f), z[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) t2[n] = splat(0.0f);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) z[rb] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = GZ2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < 4; ++n) t2[n] = GXA_MFMA(av, H1[(4 * s + q) * kSW + 16 * n + c], t2[n]);
                tb = GXA_MFMA(av, 1.0f, tb);
                const float bv = W2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) z[rb] = GXA_MFMA(GZ2[(16 * rb + c) * kSW + 4 * s + q], bv, z[rb]);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) rW2[n] += t2[n];
            rb2 += tb;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)                      // h2 was last read in stage 4
#pragma unroll
                for (int r = 0; r < 4; ++r) H2[(16 * rb + 4 * q + r) * kSW + 16 * w + c] = z[rb][r] * d1[rb][r];
        }
        wg_sync_lds();
        // ---- 6
        {
            mfma_f4 t1[NT1], tb = splat(0.0f);
#pragma unroll
            for (int n = 0; n < NT1; ++n) t1[n] = splat(0.0f);
#pragma unroll
            for (int s = 0; s < kTile / 4; ++s) {
                const float av = H2[(4 * s + q) * kSW + 16 * w + c];
#pragma unroll
                for (int n = 0; n < NT1; ++n) t1[n] = GXA_MFMA(av, O[(4 * s + q) * SO + 16 * n + c], t1[n]);
                tb = GXA_MFMA(av, 1.0f, tb);
            }
#pragma unroll
            for (int n = 0; n < NT1; ++n) rW1[n] += t1[n];
            rb1 += tb;
        }
        wg_sync_lds();                                          // O and gz1 are free for the next tile
        t = tn;
    }

    // ---- the partial vector: an accumulator's entry r is row 4 q + r, column c of its 16 x 16 tile
    float* __restrict__ out = a.partial + (size_t)blockIdx.x * P;
    if (tid < A) out[tid] = 0.0f;                               // log_std: step_kernel takes it from the float64 sums
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int unit = 16 * w + 4 * q + r;
#pragma unroll
        for (int n = 0; n < NT1; ++n)
            if (16 * n + c < D) out[oW1 + unit * D + 16 * n + c] = rW1[n][r];
#pragma unroll
        for (int n = 0; n < 4; ++n) out[oW2 + unit * kH + 16 * n + c] = rW2[n][r];
        if (c == 0) {
            out[ob1 + unit] = rb1[r];
            out[ob2 + unit] = rb2[r];
        }
        const int act = 4 * q + r;
        if (act < A) {
            out[oW3 + act * kH + 16 * w + c] = rW3[r];
            if (w == 0 && c == 0) out[ob3 + act] = rb3[r];
        }
    }
    // ---- the float64 sums: a wave's lanes as a tree (the rows of a part: lanes part + 4 i), then the waves in wave order
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = run[i];
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
        if (lane == 0) WS[w * kSums + i] = s;
    }
    if (lane == 0) WS[w * kSums + 3] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = dls[k];
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) s += __shfl_xor(s, m);
        if (lane < 4) WS[w * kSums + 4 + lane + 4 * k] = s;     // lane = part: the action part + 4 k
    }
    wg_sync_lds();
    if (tid < kSums)
        a.sums[(size_t)blockIdx.x * kSums + tid] = ((WS[tid] + WS[kSums + tid]) + WS[2 * kSums + tid]) + WS[3 * kSums + tid];
}

struct StepArgs {
    int P, A, grid, B, fit, iter, iters, t_sat;
    const float* partial;   // [grid][P]
    const double* sums;     // [grid][kSums]
    float* g_out;           // fit == 0
    double* info;           // fit == 0: loss, kl, cf
    float *theta, *m, *v;   // fit != 0, as everything below
    long long* count;       // [0] the optimizer's count, written by workgroup 0; [1] the count the call started from, read
    const double* table;    // [t_sat][2]: b1^t, b2^t
    double lr, b1, b2, omb1, omb2, eps, target_kl;
    double* trace;          // [3][iters]
    int32_t* ctl;           // flag, stop_iter, steps
    double* last;           // loss, kl, cf
};

__global__ __launch_bounds__(kThreads) void step_kernel(StepArgs a)
{
    __shared__ double sh[kThreads];
    __shared__ double mean[3];
    const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid;
    // the workgroups' sums of the loss, cf and kl in workgroup order, 64 workgroups at a time through LDS: every workgroup
    // of this launch does the same
    double s = 0.0;
    for (int base = 0; base < a.grid; base += kThreads / 4) {
        const int n = a.grid - base < kThreads / 4 ? a.grid - base : kThreads / 4;
        if (tid < 4 * n) sh[tid] = a.sums[(size_t)(base + (tid >> 2)) * kSums + (tid & 3)];
        __syncthreads();
        if (tid < 3) {
#pragma unroll 16
            for (int wg = 0; wg < n; ++wg) s += sh[4 * wg + tid];
        }
        __syncthreads();
    }
    if (tid < 3) {
        s = s / (double)a.B;
        mean[tid] = tid == 0 ? -s : s;
    }
    __syncthreads();
    const double kl = mean[2];
    const bool stop = a.fit && kl > a.target_kl;                // a NaN on either side does not stop, as in Python
    long long t = 0;
    if (a.fit) t = a.count[1] + a.iter + 1;                     // not stopped by iteration i: i steps taken in this call
    if (i < a.P && !stop) {
        double gs = 0.0;
        if (i < a.A) {
#pragma unroll 8
            for (int wg = 0; wg < a.grid; ++wg) gs += a.sums[(size_t)wg * kSums + 4 + i];
        } else {
#pragma unroll 8
            for (int wg = 0; wg < a.grid; ++wg) gs += (double)a.partial[(size_t)wg * a.P + i];
        }
        const float gi = (float)gs;
        if (a.fit) {
            const long long tc = t < a.t_sat ? t : (long long)a.t_sat;
            const long long at = tc < 1 ? 0 : tc - 1;           // entry min(t, t_sat); never outside the table
            const double p1 = a.table[2 * at], p2 = a.table[2 * at + 1];
            const double step_size = a.lr / (1.0 - p1), bc2_sqrt = sqrt(1.0 - p2);
            const double g = (double)gi;
            const double M = a.b1 * (double)a.m[i] + a.omb1 * g;
            const double V = a.b2 * (double)a.v[i] + a.omb2 * (g * g);
            const double T = (double)a.theta[i] - step_size * (M / (sqrt(V) / bc2_sqrt + a.eps));
            a.m[i] = (float)M;
            a.v[i] = (float)V;
            a.theta[i] = (float)T;
        } else {
            a.g_out[i] = gi;
        }
    }
    if (blockIdx.x != 0 || tid != 0) return;
    if (!a.fit) {
        a.info[0] = mean[0];
        a.info[1] = mean[2];
        a.info[2] = mean[1];
        return;
    }
    if (a.iter > 0 && a.ctl[0]) return;                         // stopped at an earlier iteration: nothing is evaluated here
    a.trace[a.iter] = mean[0];
    a.trace[a.iters + a.iter] = mean[2];
    a.trace[2 * a.iters + a.iter] = mean[1];
    a.last[0] = mean[0];
    a.last[1] = mean[2];
    a.last[2] = mean[1];
    if (stop) {
        a.ctl[0] = 1;
        a.ctl[1] = a.iter;
    } else {
        a.ctl[0] = 0;                                           // the call's first launch clears what an earlier call left
        a.ctl[2] = a.iter + 1;
        a.count[0] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
gxa_status check_shape(const char* who, int B, int D, int A, int hidden, int workgroups)
{
    if (B < 1 || D < 1 || A < 1) return fail(GXA_ERR_ARG, std::string(who) + ": B, D and A must be at least 1");
    if (workgroups < 0 || workgroups > kMaxWg)
        return fail(GXA_ERR_ARG, std::string(who) + ": workgroups must be 0 (the default) .. " + std::to_string(kMaxWg));
    if (hidden != kH) return fail(GXA_ERR_UNSUPPORTED, std::string(who) + " supports hidden width 64, not " + std::to_string(hidden));
    if (D > kMaxD) return fail(GXA_ERR_UNSUPPORTED, std::string(who) + " supports an observation width <= 128, not " + std::to_string(D));
    if (A % 2 || A > kAp) return fail(GXA_ERR_UNSUPPORTED, std::string(who) + " supports an even action width <= 16, not " + std::to_string(A));
    return GXA_OK;
}

// the loss kind and its clip_ratio (NaN: none)
gxa_status check_loss(const char* who, int loss, double clip)
{
    if (loss != 0 && loss != 1) return fail(GXA_ERR_ARG, std::string(who) + ": loss must be 0 (ratio) or 1 (logp)");
    if (loss == 1 && !std::isnan(clip)) return fail(GXA_ERR_ARG, std::string(who) + ": the logp loss takes no clip_ratio");
    if (!std::isnan(clip) && !(clip >= 0.0)) return fail(GXA_ERR_ARG, std::string(who) + ": clip_ratio must not be negative");
    return GXA_OK;
}

int64_t partial_bytes(int64_t P, int grid) { return (4 * (int64_t)grid * P + 7) / 8 * 8; }
int64_t work_bytes(int64_t P, int grid) { return partial_bytes(P, grid) + 8 * (int64_t)kSums * grid; }

template <int KS1>
gxa_status launch_grad(const GradArgs& a, int grid, hipStream_t s)
{
    constexpr int lds = lds_floats(KS1) * (int)sizeof(float);
    static_assert(lds <= 160 * 1024, "the LDS image fits one CU");
    static_assert(obs_stride(KS1) >= 4 * KS1 && obs_stride(KS1) >= 16 * nt1_of(KS1), "a row of the obs tile holds what stages 1 and 6 read");
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&grad_kernel<KS1>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess) return fail(GXA_ERR_HIP, std::string("gxa: hipFuncSetAttribute failed: ") + hipGetErrorString(attr));
    hipLaunchKernelGGL(grad_kernel<KS1>, dim3(grid), dim3(kThreads), lds, s, a);
    return GXA_OK;
}

gxa_status gradient_at(const GradArgs& a, int grid, hipStream_t s)
{
    const int ks = (a.D + 3) / 4;   // k-steps of the first layer: the instantiations of gx_pgrad.hip
    if (ks <= 4) return launch_grad<4>(a, grid, s);
    if (ks <= 8) return launch_grad<8>(a, grid, s);
    if (ks <= 11) return launch_grad<11>(a, grid, s);
    if (ks <= 12) return launch_grad<12>(a, grid, s);
    if (ks <= 16) return launch_grad<16>(a, grid, s);
    if (ks <= 18) return launch_grad<18>(a, grid, s);
    if (ks <= 24) return launch_grad<24>(a, grid, s);
    return launch_grad<32>(a, grid, s);
}

GradArgs grad_args(int B, int D, int A, const float* theta, const float* obs, const float* act, const float* adv,
                   const float* logp, int loss, double clip, void* work, int grid)
{
    GradArgs a{};
    a.B = B;
    a.D = D;
    a.A = A;
    a.tiles = tiles_of(B);
    a.theta = theta;
    a.obs = obs;
    a.act = act;
    a.adv = adv;
    a.logp_old = logp;
    a.logp_loss = loss == 1;
    a.clip = !std::isnan(clip);
    a.lo = a.clip ? (float)(1.0 - clip) : 0.0f;
    a.hi = a.clip ? (float)(1.0 + clip) : 0.0f;
    a.first = 1;
    a.partial = static_cast<float*>(work);
    a.sums = reinterpret_cast<double*>(static_cast<char*>(work) + partial_bytes(param_count(D, A, kH), grid));
    a.inv_b = 1.0 / (double)B;
    return a;
}

void launch_step(const StepArgs& st, hipStream_t s)
{
    hipLaunchKernelGGL(step_kernel, dim3((st.P + kThreads - 1) / kThreads), dim3(kThreads), 0, s, st);
}

gxa_status launched(const char* who)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GXA_OK : fail(GXA_ERR_HIP, std::string(who) + " launch failed: " + hipGetErrorString(e));
}

} // namespace

extern "C" const char* gxa_last_error(void) { return g_err.c_str(); }

extern "C" const char* gxa_build_id(void) { return GXA_BUILD_ID; } // guardx_amd/build.py:ACTOR_LIBRARIES["pifit"].source_hash()

extern "C" int64_t gxa_param_count(int32_t D, int32_t A, int32_t hidden)
{
    return (D < 1 || A < 1 || hidden < 1) ? -1 : param_count(D, A, hidden);
}

extern "C" int32_t gxa_default_workgroups(int32_t B) { return B < 1 ? 0 : default_workgroups(B); }

extern "C" int64_t gxa_work_bytes(int32_t B, int32_t D, int32_t A, int32_t workgroups)
{
    if (check_shape("gxa_work_bytes", B, D, A, kH, workgroups) != GXA_OK) return -1;
    return work_bytes(param_count(D, A, kH), workgroups ? workgroups : default_workgroups(B));
}

extern "C" gxa_status gxa_tanh_act(int32_t n, const float* d_x, float* d_out, void* stream)
{
    if (!d_x || !d_out) return fail(GXA_ERR_ARG, "gxa_tanh_act: null pointer");
    if (n < 0) return fail(GXA_ERR_ARG, "gxa_tanh_act: negative n");
    if (n == 0) return GXA_OK;
    const unsigned blocks = (unsigned)(((int64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(tanh_act_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, n, d_x, d_out);
    return launched("gxa_tanh_act");
}

extern "C" gxa_status gxa_gradient(int32_t B, int32_t D, int32_t A, int32_t hidden, const float* d_theta, const float* d_obs,
                                   const float* d_act, const float* d_adv, const float* d_logp, int32_t loss, void* h_hyper,
                                   int32_t workgroups, void* d_work, float* d_g, void* d_info, void* stream)
{
    if (!d_theta || !d_obs || !d_act || !d_adv || !d_logp || !h_hyper || !d_work || !d_g || !d_info)
        return fail(GXA_ERR_ARG, "gxa_gradient: null pointer");
    const gxa_status sc = check_shape("gxa_gradient", B, D, A, hidden, workgroups);
    if (sc != GXA_OK) return sc;
    const double clip = static_cast<const double*>(h_hyper)[0];
    const gxa_status sl = check_loss("gxa_gradient", loss, clip);
    if (sl != GXA_OK) return sl;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    GradArgs a = grad_args(B, D, A, d_theta, d_obs, d_act, d_adv, d_logp, loss, clip, d_work, grid);
    a.ent = static_cast<double*>(d_info) + 3;
    const gxa_status sg = gradient_at(a, grid, s);
    if (sg != GXA_OK) return sg;
    StepArgs st{};
    st.P = (int)param_count(D, A, kH);
    st.A = A;
    st.grid = grid;
    st.B = B;
    st.partial = a.partial;
    st.sums = a.sums;
    st.g_out = d_g;
    st.info = static_cast<double*>(d_info);
    launch_step(st, s);
    return launched("gxa_gradient");
}

extern "C" gxa_status gxa_fit(int32_t B, int32_t D, int32_t A, int32_t hidden, float* d_theta, float* d_m, float* d_v, void* d_count,
                              const float* d_obs, const float* d_act, const float* d_adv, const float* d_logp, int32_t iters,
                              int32_t loss, void* h_hyper, void* d_table, int32_t t_sat, int32_t workgroups, void* d_work,
                              void* d_trace, int32_t* d_ctl, void* d_last, void* stream)
{
    if (!d_theta || !d_m || !d_v || !d_count || !d_obs || !d_act || !d_adv || !d_logp || !h_hyper || !d_table || !d_work ||
        !d_trace || !d_ctl || !d_last)
        return fail(GXA_ERR_ARG, "gxa_fit: null pointer");
    if (iters < 0) return fail(GXA_ERR_ARG, "gxa_fit: negative iters");
    if (t_sat < 1) return fail(GXA_ERR_ARG, "gxa_fit: t_sat must be at least 1");
    const gxa_status sc = check_shape("gxa_fit", B, D, A, hidden, workgroups);
    if (sc != GXA_OK) return sc;
    const double* h = static_cast<const double*>(h_hyper);
    const gxa_status sl = check_loss("gxa_fit", loss, h[5]);
    if (sl != GXA_OK) return sl;
    if (iters == 0) return GXA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = workgroups ? workgroups : default_workgroups(B);
    GradArgs a = grad_args(B, D, A, d_theta, d_obs, d_act, d_adv, d_logp, loss, h[5], d_work, grid);
    a.flag = d_ctl;
    StepArgs st{};
    st.P = (int)param_count(D, A, kH);
    st.A = A;
    st.grid = grid;
    st.B = B;
    st.fit = 1;
    st.iters = iters;
    st.t_sat = t_sat;
    st.partial = a.partial;
    st.sums = a.sums;
    st.theta = d_theta;
    st.m = d_m;
    st.v = d_v;
    st.count = static_cast<long long*>(d_count);
    st.table = static_cast<const double*>(d_table);
    st.lr = h[0];
    st.b1 = h[1];
    st.b2 = h[2];
    st.omb1 = 1.0 - h[1];
    st.omb2 = 1.0 - h[2];
    st.eps = h[3];
    st.target_kl = h[4];
    st.trace = static_cast<double*>(d_trace);
    st.ctl = d_ctl;
    st.last = static_cast<double*>(d_last);
    for (int i = 0; i < iters; ++i) {
        a.first = i == 0;
        a.count = i == 0 ? st.count : nullptr;
        a.ent = i == 0 ? st.last + 3 : nullptr;
        const gxa_status sg = gradient_at(a, grid, s);
        if (sg != GXA_OK) return sg;
        st.iter = i;
        launch_step(st, s);
    }
    return launched("gxa_fit");
}
