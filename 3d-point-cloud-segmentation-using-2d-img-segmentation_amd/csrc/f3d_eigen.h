// Symmetric 3 x 3 eigen-decomposition shared by the device kernels (the box fit of f3d_hull.hip, the normals of f3d_normals.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

// cyclic Jacobi, symmetric 3 x 3: A = V diag(w) V^T.  a: a00 a01 a02 a11 a12 a22.
__device__ __forceinline__ void jacobi3(double a00, double a01, double a02, double a11, double a12, double a22, double w[3], double V[9]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (!(off > 1e-300) || off <= 1e-18 * diag) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (fabs(apq) <= 1e-300) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            const double app = A[p][p], aqq = A[q][q];
            A[p][p] = app - t * apq; A[q][q] = aqq + t * apq; A[p][q] = A[q][p] = 0.0;
            const int r = 3 - p - q;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
            for (int i = 0; i < 3; ++i) { const double vip = Q[i][p], viq = Q[i][q]; Q[i][p] = c * vip - s * viq; Q[i][q] = s * vip + c * viq; }
        }
    }
    for (int i = 0; i < 3; ++i) { w[i] = A[i][i]; for (int j = 0; j < 3; ++j) V[3 * i + j] = Q[i][j]; }
}
