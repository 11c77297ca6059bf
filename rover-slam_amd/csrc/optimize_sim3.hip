// optimize_sim3.hip -- Optimizer::OptimizeSim3 (reference src/Optimizer.cc:4195-4494 over g2o's Levenberg-Marquardt), DESIGN.md 6k.
// One workgroup of 256 lanes per problem; both rounds, their LM iterations and trials and the two chi2 classifications run inside it, so the
// only synchronisation is __syncthreads.  Lane l owns the rows i = l (mod 256).  A pass publishes through LDS the estimate, the 14
// estimates exp(+-1e-9 e_d) * S of g2o's numeric linearizeOplus (lanes 1..14 build one each) and the inverse of all 15; every active pair
// then evaluates its two errors at the 15 and leaves 36 sums (the 28 entries of H's upper triangle, the 7 of b, the robust chi2), each
// lane adding its pairs in ascending i -- e12's terms, then e21's -- and the 256 partials combined by stride halving: the order of
// departure (a).  Lane 0 then runs the serial section (lambda policy, pivoted LDLT, Sim3(update), round logic) and publishes the next
// estimate.  Everything is double, one rounding per operation (-ffp-contract=off); tests/optimize_sim3_ref.py restates it operation by
// operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"

namespace rfe {
namespace {

constexpr int OS_MAX_N = 4096;
constexpr int OS_TERMS = 36;
constexpr int OS_EST = 15;                           // the estimate and its 14 perturbations
enum : uint8_t { OS_PAIR = 1, OS_OVER = 2 };         // per-row state: carries an active edge pair; the last pass found e12 or e21 over th2
enum { OS_START = 0, OS_TRIAL = 1 };
enum { OS_FLAG_ENDED_REJECTED = 1, OS_FLAG_SOLVE_FAILED = 2, OS_FLAG_NONFINITE = 4, OS_FLAG_IDX2 = 8, OS_FLAG_EARLY = 16 };

struct OsChunk { rfe_optimize_sim3_params p[OS_CHUNK]; double delta[OS_CHUNK]; };

// ---------------------------------------------------------------- the serial section's state, in LDS: lane 0 alone touches it between barriers
struct OsSerial {
    double sums[OS_TERMS];          // what the last pass left
    double est[8];                  // the estimate the next pass evaluates (q, t, s)
    double cur[8];                  // the vertex's estimate
    double H[7][7], b[7], x[7];
    double lambda, ni, current, ini, rho;
    int phase, it, its, qmax, max_trials, nbad_lm, solve_ok, accepted, done, fix_scale;
    int iters, trials, rejected, flags, ended_rejected;
};

// oplusImpl on the solver's x: update[6] = 0 in place under fix_scale, then Sim3(x) * cur -> est
__device__ void os_update(OsSerial& S) {
    if (S.fix_scale) S.x[6] = 0.0;
    lm_sim3_oplus(S.x, S.cur, S.est);
    bool fin = true;
    for (int i = 0; i < 8; ++i) fin = fin && isfinite(S.est[i]);
    if (!fin) S.flags |= OS_FLAG_NONFINITE;
}

// one trial of levenberg.cpp:102-124 up to the error pass: solve, update, publish the trial estimate
__device__ void os_make_trial(OsSerial& S) {
    ++S.trials;
    S.solve_ok = lm_ldlt_solve<7>(S.H, S.lambda, S.b, S.x) ? 1 : 0;
    if (!S.solve_ok) S.flags |= OS_FLAG_SOLVE_FAILED;
    os_update(S);
    S.phase = OS_TRIAL;
}

// levenberg.cpp:75-97: S.sums were taken at S.cur
__device__ void os_begin_iteration(OsSerial& S) {
    ++S.iters;
    S.current = S.sums[35];
    S.ini = S.current;
    int col = 0;
    for (int j = 0; j < 7; ++j)
        for (int k = j; k < 7; ++k) { S.H[j][k] = S.sums[col]; S.H[k][j] = S.sums[col]; ++col; }
    for (int j = 0; j < 7; ++j) S.b[j] = S.sums[28 + j];
    if (S.it == 0) {
        double maxd = 0.0;
        for (int j = 0; j < 7; ++j) { const double a = fabs(S.H[j][j]); maxd = (a < maxd) ? maxd : a; }
        S.lambda = 1e-5 * maxd; S.ni = 2.0; S.nbad_lm = 0;
    }
    S.rho = 0.0; S.qmax = 0;
    os_make_trial(S);
}

// what lane 0 does after a pass; leaves S.done or the next estimate to evaluate in S.est
__device__ void os_serial_step(OsSerial& S) {
    if (S.phase == OS_START) { os_begin_iteration(S); return; }
    double temp = S.sums[35];
    if (!S.solve_ok) temp = DBL_MAX;
    double scale = 0.0;
    for (int j = 0; j < 7; ++j) scale = scale + S.x[j] * (S.lambda * S.x[j] + S.b[j]);
    scale = scale + 1e-3;
    const double rho = (S.current - temp) / scale;
    S.rho = rho;
    if (rho > 0 && isfinite(temp)) {
        const double v = 2 * rho - 1;
        double alpha = 1.0 - (v * v) * v;
        alpha = ((2.0 / 3.0) < alpha) ? (2.0 / 3.0) : alpha;
        S.lambda = S.lambda * (((1.0 / 3.0) < alpha) ? alpha : (1.0 / 3.0));
        S.ni = 2.0;
        S.current = temp;
        for (int i = 0; i < 8; ++i) S.cur[i] = S.est[i];
        S.accepted = 1;
    } else {
        S.lambda = S.lambda * S.ni;
        S.ni = S.ni * 2;
        ++S.rejected;
        S.accepted = 0;
    }
    S.ended_rejected = !S.accepted;
    ++S.qmax;
    if (rho < 0 && S.qmax < S.max_trials) { os_make_trial(S); return; }
    bool term = S.qmax == S.max_trials || rho == 0;
    if (!term) {
        if ((S.ini - S.current) * 1e3 < S.ini) ++S.nbad_lm; else S.nbad_lm = 0;
        term = S.nbad_lm >= 3;
    }
    ++S.it;
    if (term || S.it >= S.its) {
        for (int i = 0; i < 8; ++i) S.est[i] = S.cur[i];
        S.done = 1;
    } else if (S.accepted) {
        os_begin_iteration(S);                       // the sums of the accepted trial are the sums at the new estimate
    } else {
        for (int i = 0; i < 8; ++i) S.est[i] = S.cur[i];
        S.phase = OS_START;
    }
}

// ---------------------------------------------------------------- pairs
struct OsProblem {
    const double* s12_0;
    const float *xw1, *xw2, *kpts1, *kpts2;
    const uint8_t* valid;
    const int32_t *octave1, *idx2, *octave2;
    double *s12, *chi2, *trace;
    float* s12_f32;
    uint8_t* keep;
    int32_t* stats;
    int N, N2;
};
struct OsCam { double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2; };
struct OsPair { double P1[3], P2[3], o1[2], o2[2], isg1, isg2; };

// R X + t in float, ((r0 x + r1 y) + r2 z) + t
__device__ void os_to_camera(const float* R, const float* t, const float* X, float* out) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = ((R[3 * r] * X[0] + R[3 * r + 1] * X[1]) + R[3 * r + 2] * X[2]) + t[r];
}
// idx2 as the optimisation reads it: at or above n2 counts as "not in KF2"
__device__ int os_idx2(const OsProblem& p, int i, int n2) {
    const int i2 = p.idx2[i];
    return i2 >= n2 ? -1 : i2;
}

__device__ OsPair os_load(const OsProblem& p, const rfe_optimize_sim3_params& P, int i, int n2) {
    OsPair Q;
    float c1[3], c2[3];
    os_to_camera(P.rcw1, P.tcw1, p.xw1 + 3 * (size_t)i, c1);
    os_to_camera(P.rcw2, P.tcw2, p.xw2 + 3 * (size_t)i, c2);
#pragma unroll
    for (int r = 0; r < 3; ++r) { Q.P1[r] = (double)c1[r]; Q.P2[r] = (double)c2[r]; }
    Q.o1[0] = (double)p.kpts1[2 * (size_t)i]; Q.o1[1] = (double)p.kpts1[2 * (size_t)i + 1];
    int o = p.octave1 ? p.octave1[i] : 0;
    if (o < 0 || o >= P.nlevels1) o = 0;
    Q.isg1 = (double)P.inv_level_sigma2_1[o];
    const int i2 = os_idx2(p, i, n2);
    if (i2 >= 0) {
        Q.o2[0] = (double)p.kpts2[2 * (size_t)i2]; Q.o2[1] = (double)p.kpts2[2 * (size_t)i2 + 1];
        o = p.octave2 ? p.octave2[i2] : 0;
        if (o < 0 || o >= P.nlevels2) o = 0;
    } else {                                         // Optimizer.cc:4373-4382: the normalised coordinates, and a KeyPoint whose octave stays 0
        const float invz = 1 / c2[2];
        Q.o2[0] = (double)(c2[0] * invz); Q.o2[1] = (double)(c2[1] * invz);
        o = 0;
    }
    Q.isg2 = (double)P.inv_level_sigma2_2[o];
    return Q;
}

// both computeError()s at one estimate e = (r t s | r^-1 t^-1 s^-1) in LDS
__device__ void os_errors(const OsCam& C, const OsPair& Q, const double* e, double& a0, double& a1, double& b0, double& b1) {
    double q[8], r0, r1, r2;
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = e[i];
    po_rotate(q, Q.P2[0], Q.P2[1], Q.P2[2], r0, r1, r2);
    double y0 = q[7] * r0 + q[4], y1 = q[7] * r1 + q[5], y2 = q[7] * r2 + q[6];
    a0 = Q.o1[0] - (C.fx1 * y0 / y2 + C.cx1);
    a1 = Q.o1[1] - (C.fy1 * y1 / y2 + C.cy1);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = e[8 + i];
    po_rotate(q, Q.P1[0], Q.P1[1], Q.P1[2], r0, r1, r2);
    y0 = q[7] * r0 + q[4]; y1 = q[7] * r1 + q[5]; y2 = q[7] * r2 + q[6];
    b0 = Q.o2[0] - (C.fx2 * y0 / y2 + C.cx2);
    b1 = Q.o2[1] - (C.fy2 * y1 / y2 + C.cy2);
}

// one edge's 36 terms added to acc (base_binary_edge.hpp:55-120 with vertex 0 fixed): J the numeric Jacobian, e the error, isg the
// information's diagonal; robust: Huber with delta (dsqr kept in a float)
__device__ void os_edge_terms(const double (&J)[2][7], double e0, double e1, double isg, double chi2, bool robust, double delta,
                              double (&acc)[OS_TERMS]) {
    double rho0 = chi2, rho1 = 1.0;
    if (robust) {
        const double dsqr = (double)(float)(delta * delta);
        if (!(chi2 <= dsqr)) {
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
        }
    }
    const double w = rho1 * isg;
    const double r0 = (-(isg * e0)) * rho1, r1 = (-(isg * e1)) * rho1;      // omega_r = -omega e, then *= rho'
    int col = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int k = j; k < 7; ++k) {
            acc[col] = acc[col] + ((J[0][j] * w) * J[0][k] + (J[1][j] * w) * J[1][k]);
            ++col;
        }
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[28 + j] = acc[28 + j] + (J[0][j] * r0 + J[1][j] * r1);
    acc[35] = acc[35] + rho0;
}

__global__ __launch_bounds__(LM_LANES) void optimize_sim3_kernel(OsChunk PC, OsProblem pr0, int first) {
    __shared__ double buf[28 * LM_LANES];            // a pass's Jacobians, 28 entries per lane; then the reduction's 128 x 36
    __shared__ double E[OS_EST][16];
    __shared__ uint8_t state[OS_MAX_N];
    __shared__ OsSerial S;
    __shared__ int cnt, oor;
    const int lane = threadIdx.x, prob = first + blockIdx.x;
    __shared__ rfe_optimize_sim3_params P;          // per-lane reads of the level tables go to LDS, not to the kernel arguments
    {
        const int32_t* src = reinterpret_cast<const int32_t*>(&PC.p[blockIdx.x]);
        int32_t* dst = reinterpret_cast<int32_t*>(&P);
        for (int w = lane; w < (int)(sizeof(P) / sizeof(int32_t)); w += LM_LANES) dst[w] = src[w];
    }
    __syncthreads();
    const double delta = PC.delta[blockIdx.x], th2 = (double)P.th2;
    const int N = pr0.N, N2 = pr0.N2;
    OsProblem p = pr0;
    p.s12_0 += (size_t)prob * 8; p.xw1 += (size_t)prob * N * 3; p.xw2 += (size_t)prob * N * 3; p.valid += (size_t)prob * N;
    p.kpts1 += (size_t)prob * N * 2; p.idx2 += (size_t)prob * N;
    if (p.octave1) p.octave1 += (size_t)prob * N;
    if (p.kpts2) p.kpts2 += (size_t)prob * N2 * 2;
    if (p.octave2) p.octave2 += (size_t)prob * N2;
    p.s12 += (size_t)prob * 8; p.keep += (size_t)prob * N; p.stats += (size_t)prob * 8;
    if (p.s12_f32) p.s12_f32 += (size_t)prob * 8;
    if (p.chi2) p.chi2 += (size_t)prob * N * 2;
    if (p.trace) p.trace += (size_t)prob * 16;
    const int n = P.n < 0 ? 0 : (P.n > N ? N : P.n);
    const int n2 = P.n2 < 0 ? 0 : (P.n2 > N2 ? N2 : P.n2);
    const OsCam C = {(double)P.fx1, (double)P.fy1, (double)P.cx1, (double)P.cy1, (double)P.fx2, (double)P.fy2, (double)P.cx2, (double)P.cy2};

    if (lane == 0) { cnt = 0; oor = 0; }
    if (p.trace && lane < 16) p.trace[lane] = 0.0;
    __syncthreads();
    // which rows carry an edge pair (Optimizer.cc:4254-4333)
    int mine = 0, over = 0;
    for (int i = lane; i < n; i += LM_LANES) {
        bool pair = p.valid[i] != 0;
        if (pair) {
            if (p.idx2[i] >= n2) over = 1;
            float c2[3];
            os_to_camera(P.rcw2, P.tcw2, p.xw2 + 3 * (size_t)i, c2);
            pair = (P.all_points != 0 || os_idx2(p, i, n2) >= 0) && !(c2[2] < 0);
        }
        state[i] = pair ? OS_PAIR : 0;
        mine += pair ? 1 : 0;
    }
    if (mine) atomicAdd(&cnt, mine);
    if (over) atomicOr(&oor, 1);
    __syncthreads();
    const int n_corr = cnt;
    if (lane == 0) {
        for (int i = 0; i < 8; ++i) { S.cur[i] = p.s12_0[i]; S.est[i] = S.cur[i]; }
        for (int i = 0; i < 7; ++i) S.x[i] = 0.0;
        S.max_trials = P.max_trials > 0 ? P.max_trials : 10;
        S.fix_scale = P.fix_scale != 0;
        S.flags = oor ? OS_FLAG_IDX2 : 0;
    }
    int rounds = 0, tot_iters = 0, tot_trials = 0, tot_rejected = 0, n_bad = 0, n_in = 0;   // lane 0's; n_bad every lane's
    bool early = n_corr == 0;
    for (int rnd = 0; rnd < 2 && !early; ++rnd) {
        const bool robust = rnd == 0;
        __syncthreads();
        if (lane == 0) {
            const int want = rnd == 0 ? P.iterations[0] : (n_bad > 0 ? P.iterations[2] : P.iterations[1]);
            S.its = want > 0 ? want : (rnd == 1 && n_bad > 0 ? 10 : 5);
            for (int i = 0; i < 8; ++i) S.est[i] = S.cur[i];
            S.phase = OS_START; S.it = 0;
            S.lambda = 0.0; S.ni = 2.0; S.nbad_lm = 0; S.current = 0.0;
            S.iters = S.trials = S.rejected = 0; S.ended_rejected = 0; S.done = 0;
            cnt = 0;
        }
        __syncthreads();
        for (;;) {                                   // at most its * (max_trials + 1) passes
            if (lane < OS_EST) {                     // the estimate, exp(+-delta e_d) * estimate (base_binary_edge.hpp:181-197), their inverses
                double est[8], out[16];
#pragma unroll
                for (int i = 0; i < 8; ++i) est[i] = S.est[i];
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) out[i] = est[i];
                } else {
                    const int d = (lane - 1) >> 1;
                    const double step = (lane & 1) ? 1e-9 : -1e-9;
                    double u[7];
#pragma unroll
                    for (int j = 0; j < 7; ++j) u[j] = (j == d) ? step : 0.0;
                    if (S.fix_scale) u[6] = 0.0;
                    lm_sim3_oplus(u, est, out);
                }
                lm_sim3_inverse(out, out + 8);
#pragma unroll
                for (int i = 0; i < 16; ++i) E[lane][i] = out[i];
            }
            __syncthreads();
            double acc[OS_TERMS];
#pragma unroll
            for (int c = 0; c < OS_TERMS; ++c) acc[c] = 0.0;
            for (int i = lane; i < n; i += LM_LANES) {
                if (!(state[i] & OS_PAIR)) continue;
                const OsPair Q = os_load(p, P, i, n2);
                double a0, a1, b0, b1;
                os_errors(C, Q, E[0], a0, a1, b0, b1);
                const double c12 = a0 * (Q.isg1 * a0) + a1 * (Q.isg1 * a1), c21 = b0 * (Q.isg2 * b0) + b1 * (Q.isg2 * b1);
                state[i] = (c12 > th2 || c21 > th2) ? (OS_PAIR | OS_OVER) : OS_PAIR;
                if (p.chi2) { p.chi2[2 * (size_t)i] = c12; p.chi2[2 * (size_t)i + 1] = c21; }
                const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll 1
                for (int d = 0; d < 7; ++d) {        // one column at a time through the lane's LDS slots: 28 more doubles in registers would spill
                    double pa0, pa1, pb0, pb1, ma0, ma1, mb0, mb1;
                    os_errors(C, Q, E[1 + 2 * d], pa0, pa1, pb0, pb1);
                    os_errors(C, Q, E[2 + 2 * d], ma0, ma1, mb0, mb1);
                    buf[d * LM_LANES + lane] = scalar * (pa0 - ma0); buf[(7 + d) * LM_LANES + lane] = scalar * (pa1 - ma1);
                    buf[(14 + d) * LM_LANES + lane] = scalar * (pb0 - mb0); buf[(21 + d) * LM_LANES + lane] = scalar * (pb1 - mb1);
                }
                double J[2][7];
#pragma unroll
                for (int d = 0; d < 7; ++d) { J[0][d] = buf[d * LM_LANES + lane]; J[1][d] = buf[(7 + d) * LM_LANES + lane]; }
                os_edge_terms(J, a0, a1, Q.isg1, c12, robust, delta, acc);
#pragma unroll
                for (int d = 0; d < 7; ++d) { J[0][d] = buf[(14 + d) * LM_LANES + lane]; J[1][d] = buf[(21 + d) * LM_LANES + lane]; }
                os_edge_terms(J, b0, b1, Q.isg2, c21, robust, delta, acc);
            }
            __syncthreads();                         // the reduction reuses buf
            lm_reduce<OS_TERMS>(acc, buf, S.sums, lane);   // its barriers also order the reads of E and S.est before lane 0's writes below
            if (lane == 0) os_serial_step(S);
            __syncthreads();
            if (S.done) break;
        }
        if (rnd == 0) {
            // Optimizer.cc:4418-4447: the chi2 the last computeActiveErrors left, stale after a rejected trial, against (double) th2
            int bad = 0;
            for (int i = lane; i < n; i += LM_LANES)
                if (state[i] == (OS_PAIR | OS_OVER)) { state[i] = 0; p.keep[i] = 0; ++bad; }
            if (bad) atomicAdd(&cnt, bad);
            __syncthreads();
            n_bad = cnt;
            early = n_corr - n_bad < 10;             // :4456
        } else {
            // :4467-4486: every surviving pair's error again at the final estimate
            if (lane == 0) {
                double out[16];
                for (int i = 0; i < 8; ++i) out[i] = S.cur[i];
                lm_sim3_inverse(out, out + 8);
                for (int i = 0; i < 16; ++i) E[0][i] = out[i];
            }
            __syncthreads();
            int in = 0;
            for (int i = lane; i < n; i += LM_LANES) {
                if (!(state[i] & OS_PAIR)) continue;
                const OsPair Q = os_load(p, P, i, n2);
                double a0, a1, b0, b1;
                os_errors(C, Q, E[0], a0, a1, b0, b1);
                const double c12 = a0 * (Q.isg1 * a0) + a1 * (Q.isg1 * a1), c21 = b0 * (Q.isg2 * b0) + b1 * (Q.isg2 * b1);
                if (p.chi2) { p.chi2[2 * (size_t)i] = c12; p.chi2[2 * (size_t)i + 1] = c21; }
                if (c12 > th2 || c21 > th2) p.keep[i] = 0; else ++in;
            }
            if (in) atomicAdd(&cnt, in);
            __syncthreads();
            n_in = cnt;
        }
        if (lane == 0) {
            if (S.ended_rejected) S.flags |= OS_FLAG_ENDED_REJECTED;
            ++rounds; tot_iters += S.iters; tot_trials += S.trials; tot_rejected += S.rejected;
            if (p.trace) {
                double* t = p.trace + rnd * 8;
                t[0] = (double)S.iters; t[1] = (double)S.trials; t[2] = S.lambda; t[3] = S.current;
                t[4] = (double)(rnd == 0 ? n_corr - n_bad : n_in);
            }
        }
    }
    if (lane == 0) {
        if (early) S.flags |= OS_FLAG_EARLY;
        bool fin = true;
        for (int i = 0; i < 8; ++i) {
            const double v = early ? p.s12_0[i] : S.cur[i];       // :4457 returns before g2oS12 is written
            p.s12[i] = v;
            if (p.s12_f32) p.s12_f32[i] = (float)v;
            fin = fin && isfinite(v);
        }
        if (!fin) S.flags |= OS_FLAG_NONFINITE;
        p.stats[0] = early ? 0 : n_in; p.stats[1] = n_corr; p.stats[2] = n_bad; p.stats[3] = rounds; p.stats[4] = tot_iters;
        p.stats[5] = tot_trials; p.stats[6] = tot_rejected; p.stats[7] = S.flags;
    }
}

}  // namespace

void launch_optimize_sim3(hipStream_t s, const rfe_optimize_sim3_params* params, const double* s12_0, const float* xw1, const float* xw2,
                          const uint8_t* valid, const float* kpts1, const int32_t* octave1, const int32_t* idx2, const float* kpts2,
                          const int32_t* octave2, int B, int N, int N2, double* s12, float* s12_f32, uint8_t* keep, double* chi2, double* trace,
                          int32_t* stats) {
    OsProblem p;
    p.s12_0 = s12_0; p.xw1 = xw1; p.xw2 = xw2; p.kpts1 = kpts1; p.kpts2 = kpts2; p.valid = valid; p.octave1 = octave1; p.idx2 = idx2;
    p.octave2 = octave2; p.s12 = s12; p.chi2 = chi2; p.trace = trace; p.s12_f32 = s12_f32; p.keep = keep; p.stats = stats; p.N = N; p.N2 = N2;
    for (int first = 0; first < B; first += OS_CHUNK) {
        const int m = B - first < OS_CHUNK ? B - first : OS_CHUNK;
        OsChunk PC;
        for (int b = 0; b < OS_CHUNK; ++b) {
            PC.p[b] = params[first + (b < m ? b : 0)];
            PC.delta[b] = (double)(float)sqrt((double)PC.p[b].th2);      // `const float deltaHuber = sqrt(th2)`
        }
        hipLaunchKernelGGL(optimize_sim3_kernel, dim3(m), dim3(LM_LANES), 0, s, PC, p, first);
    }
}

}  // namespace rfe
