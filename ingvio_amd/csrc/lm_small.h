// lm_small.h — the two scalar helpers of delayed initialisation, shared by the single-filter kernels (kernels_lm.hip) and the batched
// front (kernels_delayed.hip): both paths must rotate and invert bit for bit alike.
#pragma once
#include "dev_common.h"

// Eigen::JacobiRotation<double>::makeGivens (real case)
__device__ __forceinline__ void make_givens(double p, double q, double& c, double& s)
{
    if (q == 0.0) { c = p < 0.0 ? -1.0 : 1.0; s = 0.0; }
    else if (p == 0.0) { c = 0.0; s = q < 0.0 ? 1.0 : -1.0; }
    else if (fabs(p) > fabs(q)) {
        const double t = q / p;
        double u = sqrt(1.0 + t * t);
        if (p < 0.0) u = -u;
        c = 1.0 / u; s = -t * c;
    } else {
        const double t = p / q;
        double u = sqrt(1.0 + t * t);
        if (q < 0.0) u = -u;
        s = -1.0 / u; c = -t * s;
    }
}

// s x s inverse by Gauss-Jordan with partial pivoting, in LDS, one lane
__device__ inline void inv_small(double* A, double* Ai, int s)
{
    for (int i = 0; i < s * s; ++i) Ai[i] = (i % (s + 1) == 0) ? 1.0 : 0.0;
    for (int j = 0; j < s; ++j) {
        int p = j; double mx = fabs(A[j + j * s]);
        for (int i = j + 1; i < s; ++i) if (fabs(A[i + j * s]) > mx) { mx = fabs(A[i + j * s]); p = i; }
        if (p != j)
            for (int c = 0; c < s; ++c) {
                double t = A[j + c * s]; A[j + c * s] = A[p + c * s]; A[p + c * s] = t;
                t = Ai[j + c * s]; Ai[j + c * s] = Ai[p + c * s]; Ai[p + c * s] = t;
            }
        const double d = 1.0 / A[j + j * s];
        for (int c = 0; c < s; ++c) { A[j + c * s] *= d; Ai[j + c * s] *= d; }
        for (int i = 0; i < s; ++i) {
            if (i == j) continue;
            const double f = A[i + j * s];
            for (int c = 0; c < s; ++c) { A[i + c * s] -= f * A[j + c * s]; Ai[i + c * s] -= f * Ai[j + c * s]; }
        }
    }
}
