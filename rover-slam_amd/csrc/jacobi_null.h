// jacobi_null.h -- the null vector of a 4 x 4 matrix by a fixed-schedule one-sided Jacobi, shared by triangulate.hip (DESIGN.md 6g,
// normalised coordinates) and two_view.hip (pixel units): the sweep count is the caller's, measured per use.
#pragma once

namespace rfe {

// Null vector of the 4 x 4 matrix A: one-sided Jacobi on its columns, V accumulated; every index below is a compile-time constant once the
// loops are unrolled, so A and V are 32 registers.  TOL false (6g): a pair is rotated unless its columns' inner product gamma is exactly zero.
// TOL true (6o): unless gamma^2 <= 2^-40 alpha beta, so that the iteration reaches a fixed point.  A NaN rotates (and spreads) in both.
constexpr float JACOBI_TOL2 = 0x1p-40f;
template <int SWEEPS, bool TOL = false>
__device__ __forceinline__ void jacobi_null4(float (&A)[4][4], float (&h)[4]) {
    float V[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.f : 0.f;
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep)
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const float alpha = ((A[0][p] * A[0][p] + A[1][p] * A[1][p]) + A[2][p] * A[2][p]) + A[3][p] * A[3][p];
                const float beta = ((A[0][q] * A[0][q] + A[1][q] * A[1][q]) + A[2][q] * A[2][q]) + A[3][q] * A[3][q];
                const float gamma = ((A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]) + A[3][p] * A[3][q];
                const bool rot = TOL ? !(gamma * gamma <= JACOBI_TOL2 * (alpha * beta)) : gamma != 0.f;
                const float zeta = (beta - alpha) / (2.f * gamma);
                const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
                const float c = 1.f / sqrtf(1.f + t * t);
                const float s = c * t;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float ap = A[r][p], aq = A[r][q], vp = V[r][p], vq = V[r][q];
                    A[r][p] = rot ? c * ap - s * aq : ap; A[r][q] = rot ? s * ap + c * aq : aq;
                    V[r][p] = rot ? c * vp - s * vq : vp; V[r][q] = rot ? s * vp + c * vq : vq;
                }
            }
    float nb = ((A[0][0] * A[0][0] + A[1][0] * A[1][0]) + A[2][0] * A[2][0]) + A[3][0] * A[3][0];
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = V[r][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const float nc = ((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]) + A[3][c] * A[3][c];
        const bool less = nc < nb;                                       // the first minimum stays; a NaN norm is never smaller
        nb = less ? nc : nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = less ? V[r][c] : h[r];
    }
}

}  // namespace rfe
