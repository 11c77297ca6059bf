// pose_opt.hip -- Optimizer::PoseOptimization (reference src/Optimizer.cc:55-401 over g2o's Levenberg-Marquardt), DESIGN.md 6i.
// One workgroup of 256 lanes per problem; the four rounds, their LM iterations and the chi2 re-classification all run inside it, so the
// only synchronisation is __syncthreads.  Lane l owns the features i = l (mod 256): a pass evaluates every active edge at the estimate in
// LDS and leaves 28 sums (the 21 entries of H's upper triangle, the 6 sums whose negative is b, the robust chi2), each lane adding its
// edges in ascending i, the 256 partials combined by stride halving -- the order of departure (a), whatever the launch.  Lane 0 then
// runs the serial section (lambda policy, pivoted LDLT, exp, round logic) and publishes the next estimate.  Everything is double, one
// rounding per operation (-ffp-contract=off); tests/pose_opt_ref.py restates it operation by operation.
#include <float.h>
#include "rfe_internal.h"
#include "lm_device.h"

namespace rfe {
namespace {

constexpr int PO_LANES = 256;
constexpr int PO_MAX_N = 4096;
constexpr int PO_TERMS = 28;
enum : uint8_t { PO_EDGE = 1, PO_OUTLIER = 2 };      // per-feature state: has an edge; the edge is at level 1
enum { PO_START = 0, PO_TRIAL = 1 };
enum { PO_FLAG_ENDED_REJECTED = 1, PO_FLAG_SOLVE_FAILED = 2, PO_FLAG_NONFINITE = 4 };

struct PoseProblem {
    const float *pose0, *kpts, *uright, *xw;
    const int32_t *octave, *n;
    const uint8_t* has_mp;
    double *pose, *trace;
    float *pose_f32, *chi2;
    uint8_t* outlier;
    int32_t* stats;
    int N;
};

// ---------------------------------------------------------------- the serial section's state, in LDS: lane 0 alone touches it between barriers
struct PoseSerial {
    double sums[PO_TERMS];          // what the last pass left
    double est[7];                  // the estimate the next pass evaluates (q, t)
    double cur[7], q0[7];           // the vertex's estimate; the input pose normalised
    double H[6][6], b[6], x[6];
    double lambda, ni, current, ini, rho;
    int phase, it, its, qmax, max_trials, nbad_lm, solve_ok, accepted, done;
    int iters, trials, rejected, flags, ended_rejected;
    int n_init, n_bad;
};

// departure (c): lm_device.h's pivoted LDLT on A = H + lambda I; false: a negative pivot.  The solution replaces S.x only on success
__device__ bool po_solve(PoseSerial& S) {
    return lm_ldlt_solve<6>(S.H, S.lambda, S.b, S.x);
}

// SE3Quat::exp(x) * cur -> est (lm_device.h)
__device__ void po_update(PoseSerial& S) {
    if (!lm_se3_exp_mul(S.x, S.cur, S.est)) S.flags |= PO_FLAG_NONFINITE;
}

// one trial of levenberg.cpp:102-124 up to the error pass: solve, update, publish the trial estimate
__device__ void po_make_trial(PoseSerial& S) {
    ++S.trials;
    S.solve_ok = po_solve(S) ? 1 : 0;
    if (!S.solve_ok) S.flags |= PO_FLAG_SOLVE_FAILED;
    po_update(S);
    S.phase = PO_TRIAL;
}

// levenberg.cpp:75-97: S.sums were taken at S.cur
__device__ void po_begin_iteration(PoseSerial& S) {
    ++S.iters;
    S.current = S.sums[27];
    S.ini = S.current;
    int col = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k) { S.H[j][k] = S.sums[col]; S.H[k][j] = S.sums[col]; ++col; }
    for (int j = 0; j < 6; ++j) S.b[j] = -S.sums[21 + j];
    if (S.it == 0) {
        double maxd = 0.0;
        for (int j = 0; j < 6; ++j) { const double a = fabs(S.H[j][j]); maxd = (a < maxd) ? maxd : a; }
        S.lambda = 1e-5 * maxd; S.ni = 2.0; S.nbad_lm = 0;
    }
    S.rho = 0.0; S.qmax = 0;
    po_make_trial(S);
}

// what lane 0 does after a pass; leaves S.done or the next estimate to evaluate in S.est
__device__ void po_serial_step(PoseSerial& S) {
    if (S.phase == PO_START) { po_begin_iteration(S); return; }
    double temp = S.sums[27];
    if (!S.solve_ok) temp = DBL_MAX;
    double scale = 0.0;
    for (int j = 0; j < 6; ++j) scale = scale + S.x[j] * (S.lambda * S.x[j] + S.b[j]);
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
        for (int i = 0; i < 7; ++i) S.cur[i] = S.est[i];
        S.accepted = 1;
    } else {
        S.lambda = S.lambda * S.ni;
        S.ni = S.ni * 2;
        ++S.rejected;
        S.accepted = 0;
    }
    S.ended_rejected = !S.accepted;
    ++S.qmax;
    if (rho < 0 && S.qmax < S.max_trials) { po_make_trial(S); return; }
    bool term = S.qmax == S.max_trials || rho == 0;
    if (!term) {
        if ((S.ini - S.current) * 1e3 < S.ini) ++S.nbad_lm; else S.nbad_lm = 0;
        term = S.nbad_lm >= 3;
    }
    ++S.it;
    if (term || S.it >= S.its) {
        for (int i = 0; i < 7; ++i) S.est[i] = S.cur[i];
        S.done = 1;
    } else if (S.accepted) {
        po_begin_iteration(S);                       // the sums of the accepted trial are the sums at the new estimate
    } else {
        for (int i = 0; i < 7; ++i) S.est[i] = S.cur[i];
        S.phase = PO_START;
    }
}

// ---------------------------------------------------------------- edges
struct PoseCam { double fx, fy, cx, cy, bf; };
struct PoseEdge { double X0, X1, X2, u, v, ur, isg; bool stereo; };

__device__ PoseEdge po_load(const PoseProblem& p, const rfe_pose_params& P, int i) {
    PoseEdge e;
    e.X0 = (double)p.xw[3 * i]; e.X1 = (double)p.xw[3 * i + 1]; e.X2 = (double)p.xw[3 * i + 2];
    e.u = (double)p.kpts[2 * i]; e.v = (double)p.kpts[2 * i + 1];
    const float ur = p.uright ? p.uright[i] : -1.f;
    e.stereo = !(ur < 0);
    e.ur = (double)ur;
    int o = p.octave ? p.octave[i] : 0;
    if (o < 0 || o >= P.nlevels) o = 0;
    e.isg = (double)P.inv_level_sigma2[o];
    return e;
}

// computeError and chi2() at (q, t): the point in the camera frame in x y z, the error in e0..e2
__device__ double po_error(const PoseCam& C, const PoseEdge& E, const double* q, double& x, double& y, double& z, double& e0, double& e1,
                           double& e2) {
    po_rotate(q, E.X0, E.X1, E.X2, x, y, z);
    x = x + q[4]; y = y + q[5]; z = z + q[6];
    double chi2;
    if (E.stereo) {
        const double invz = (double)(float)(1.0 / z);
        const double pu = x * invz * C.fx + C.cx;
        const double pv = y * invz * C.fy + C.cy;
        const double pr = pu - C.bf * invz;
        e0 = E.u - pu; e1 = E.v - pv; e2 = E.ur - pr;
        chi2 = e0 * (E.isg * e0) + e1 * (E.isg * e1);
        chi2 = chi2 + e2 * (E.isg * e2);
    } else {
        e0 = E.u - (C.fx * x / z + C.cx);
        e1 = E.v - (C.fy * y / z + C.cy);
        e2 = 0.0;
        chi2 = e0 * (E.isg * e0) + e1 * (E.isg * e1);
    }
    return chi2;
}

// one edge's 28 terms added to acc
__device__ void po_edge_terms(const PoseCam& C, const PoseEdge& E, const double* q, bool robust, double (&acc)[PO_TERMS], float& chi2f) {
    double x, y, z, e[3];
    const double chi2 = po_error(C, E, q, x, y, z, e[0], e[1], e[2]);
    chi2f = (float)chi2;
    double rho0 = chi2, rho1 = 1.0;
    if (robust) {
        const double delta = E.stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991);   // `const float deltaMono = sqrt(5.991)`
        const double dsqr = (double)(float)(delta * delta);
        if (!(chi2 <= dsqr)) {
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
        }
    }
    double A[3][6];
    if (E.stereo) {
        const double invz = 1.0 / z, invz2 = invz * invz;
        A[0][0] = x * y * invz2 * C.fx;
        A[0][1] = -(1 + (x * x * invz2)) * C.fx;
        A[0][2] = y * invz * C.fx;
        A[0][3] = -invz * C.fx;
        A[0][4] = 0.0;
        A[0][5] = x * invz2 * C.fx;
        A[1][0] = (1 + y * y * invz2) * C.fy;
        A[1][1] = -x * y * invz2 * C.fy;
        A[1][2] = -x * invz * C.fy;
        A[1][3] = 0.0;
        A[1][4] = -invz * C.fy;
        A[1][5] = y * invz2 * C.fy;
        A[2][0] = A[0][0] - C.bf * y * invz2;
        A[2][1] = A[0][1] + C.bf * x * invz2;
        A[2][2] = A[0][2];
        A[2][3] = A[0][3];
        A[2][4] = 0.0;
        A[2][5] = A[0][5] - C.bf * invz2;
    } else {
        // -projectJac * SE3deriv: every product and sum of the 2x3 by 3x6 product, zeros included
        const double nJ[2][3] = {{-(C.fx / z), -0.0, -(-C.fx * x / (z * z))}, {-0.0, -(C.fy / z), -(-C.fy * y / (z * z))}};
        const double Sd[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) A[r][c] = (nJ[r][0] * Sd[0][c] + nJ[r][1] * Sd[1][c]) + nJ[r][2] * Sd[2][c];
#pragma unroll
        for (int c = 0; c < 6; ++c) A[2][c] = 0.0;
    }
    const double w = rho1 * E.isg;
    int col = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k) {
            double h = (A[0][j] * w) * A[0][k] + (A[1][j] * w) * A[1][k];
            if (E.stereo) h = h + (A[2][j] * w) * A[2][k];
            acc[col] = acc[col] + h;
            ++col;
        }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double g = ((rho1 * A[0][j]) * E.isg) * e[0] + ((rho1 * A[1][j]) * E.isg) * e[1];
        if (E.stereo) g = g + ((rho1 * A[2][j]) * E.isg) * e[2];
        acc[21 + j] = acc[21 + j] + g;
    }
    acc[27] = acc[27] + rho0;
}

__global__ __launch_bounds__(PO_LANES) void pose_opt_kernel(rfe_pose_params P, PoseProblem pr0) {
    __shared__ double red[128 * PO_TERMS];
    __shared__ float chi2f[PO_MAX_N];               // (float) chi2 of the error the last computeActiveErrors left on the edge
    __shared__ uint8_t state[PO_MAX_N];
    __shared__ PoseSerial S;
    __shared__ int cnt;
    const int lane = threadIdx.x, prob = blockIdx.x;
    const int N = pr0.N;
    PoseProblem p = pr0;
    p.pose0 += (size_t)prob * 7; p.kpts += (size_t)prob * N * 2; p.xw += (size_t)prob * N * 3; p.has_mp += (size_t)prob * N;
    if (p.uright) p.uright += (size_t)prob * N;
    if (p.octave) p.octave += (size_t)prob * N;
    p.pose += (size_t)prob * 7; p.outlier += (size_t)prob * N; p.stats += (size_t)prob * 8;
    if (p.pose_f32) p.pose_f32 += (size_t)prob * 7;
    if (p.chi2) p.chi2 += (size_t)prob * N;
    if (p.trace) p.trace += (size_t)prob * 32;
    int n = p.n ? p.n[prob] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    const PoseCam C = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.bf};

    if (lane == 0) cnt = 0;
    if (p.trace && lane < 32) p.trace[lane] = 0.0;
    __syncthreads();
    int mine = 0;
    for (int i = lane; i < n; i += PO_LANES) {
        const bool has = p.has_mp[i] != 0;
        state[i] = has ? PO_EDGE : 0;
        if (has) { p.outlier[i] = 0; ++mine; }
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    const int n_init = cnt;
    if (n_init < 3) {                                // Optimizer.cc:270: the flags are cleared, the pose is untouched
        if (lane < 7) {
            p.pose[lane] = (double)p.pose0[lane];
            if (p.pose_f32) p.pose_f32[lane] = p.pose0[lane];
        }
        if (lane < 8) p.stats[lane] = lane == 1 ? n_init : 0;
        return;
    }
    if (lane == 0) {
        for (int i = 0; i < 7; ++i) S.q0[i] = (double)p.pose0[i];
        po_normalize(S.q0);
        for (int i = 0; i < 6; ++i) S.x[i] = 0.0;
        S.max_trials = P.max_trials > 0 ? P.max_trials : 10;
        S.flags = 0; S.n_bad = 0; S.n_init = n_init;
    }
    // the lane's first two edges stay in registers for the whole call: up to 512 features no pass reads global memory
    PoseEdge E0 = PoseEdge(), E1 = PoseEdge();
    if (lane < n) E0 = po_load(p, P, lane);
    if (lane + PO_LANES < n) E1 = po_load(p, P, lane + PO_LANES);
    int rounds = 0, tot_iters = 0, tot_trials = 0, tot_rejected = 0;   // lane 0's
    for (int rnd = 0; rnd < 4; ++rnd) {
        const bool robust = rnd < 3;
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < 7; ++i) { S.cur[i] = S.q0[i]; S.est[i] = S.q0[i]; }
            S.phase = PO_START; S.it = 0; S.its = P.iterations[rnd] > 0 ? P.iterations[rnd] : 10;
            S.lambda = 0.0; S.ni = 2.0; S.nbad_lm = 0; S.current = 0.0;
            S.iters = S.trials = S.rejected = 0; S.ended_rejected = 0; S.done = 0;
            cnt = 0;
        }
        __syncthreads();
        for (;;) {                                   // at most its * (max_trials + 1) passes
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) q[i] = S.est[i];
            double acc[PO_TERMS];
#pragma unroll
            for (int c = 0; c < PO_TERMS; ++c) acc[c] = 0.0;
            for (int i = lane, slot = 0; i < n; i += PO_LANES, ++slot) {
                if (state[i] != PO_EDGE) continue;
                const PoseEdge E = slot == 0 ? E0 : (slot == 1 ? E1 : po_load(p, P, i));
                float cf;
                po_edge_terms(C, E, q, robust, acc, cf);
                chi2f[i] = cf;
            }
            lm_reduce<PO_TERMS>(acc, red, S.sums, lane);       // its barriers also order the reads of S.est above before lane 0's writes below
            if (lane == 0) po_serial_step(S);
            __syncthreads();
            if (S.done) break;
        }
        // classification at the round's estimate (Optimizer.cc:294-384): an outlier edge recomputes its error, an inlier keeps its last
        {
            double q[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) q[i] = S.est[i];
            int bad = 0;
            for (int i = lane, slot = 0; i < n; i += PO_LANES, ++slot) {
                const uint8_t st = state[i];
                if (!st) continue;
                const PoseEdge E = slot == 0 ? E0 : (slot == 1 ? E1 : po_load(p, P, i));
                float cf;
                if (st & PO_OUTLIER) {
                    double x, y, z, e0, e1, e2;
                    cf = (float)po_error(C, E, q, x, y, z, e0, e1, e2);
                    chi2f[i] = cf;
                } else {
                    cf = chi2f[i];
                }
                const bool out = cf > (E.stereo ? 7.815f : 5.991f);
                state[i] = out ? (PO_EDGE | PO_OUTLIER) : PO_EDGE;
                p.outlier[i] = out ? 1 : 0;
                if (p.chi2) p.chi2[i] = cf;
                bad += out ? 1 : 0;
            }
            if (bad) atomicAdd(&cnt, bad);
        }
        __syncthreads();
        if (lane == 0) {
            S.n_bad = cnt;
            if (S.ended_rejected) S.flags |= PO_FLAG_ENDED_REJECTED;
            ++rounds; tot_iters += S.iters; tot_trials += S.trials; tot_rejected += S.rejected;
            if (p.trace) {
                double* t = p.trace + rnd * 8;
                t[0] = (double)S.iters; t[1] = (double)S.trials; t[2] = S.lambda; t[3] = S.current; t[4] = (double)(n_init - S.n_bad);
            }
        }
        if (n_init < 10) break;                      // Optimizer.cc:386 counts every edge, not the inliers
    }
    if (lane == 0) {
        bool fin = true;
        for (int i = 0; i < 7; ++i) {
            p.pose[i] = S.cur[i];
            if (p.pose_f32) p.pose_f32[i] = (float)S.cur[i];
            fin = fin && isfinite(S.cur[i]);
        }
        if (!fin) S.flags |= PO_FLAG_NONFINITE;
        p.stats[0] = n_init - S.n_bad; p.stats[1] = n_init; p.stats[2] = S.n_bad; p.stats[3] = rounds; p.stats[4] = tot_iters;
        p.stats[5] = tot_trials; p.stats[6] = tot_rejected; p.stats[7] = S.flags;
    }
}

}  // namespace

void launch_pose_opt(hipStream_t s, const rfe_pose_params& P, const float* pose0, const float* kpts, const int32_t* octave, const float* uright,
                     const float* xw, const uint8_t* has_mp, const int32_t* n, int B, int N, double* pose, float* pose_f32, uint8_t* outlier,
                     float* chi2, double* trace, int32_t* stats) {
    if (B <= 0) return;
    PoseProblem p;
    p.pose0 = pose0; p.kpts = kpts; p.uright = uright; p.xw = xw; p.octave = octave; p.n = n; p.has_mp = has_mp;
    p.pose = pose; p.trace = trace; p.pose_f32 = pose_f32; p.chi2 = chi2; p.outlier = outlier; p.stats = stats; p.N = N;
    hipLaunchKernelGGL(pose_opt_kernel, dim3(B), dim3(PO_LANES), 0, s, P, p);
}

}  // namespace rfe
