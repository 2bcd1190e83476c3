// The arithmetic of the cloud-to-cloud refiner that its kernels (refine.hip) share and a host program can call as well: the
// row filter, the moved point, the cell of a coordinate with the box that bounds its rows, and the rigid step from the 17
// figures of an evaluation.  Float64 throughout, operation by operation (the unit is built without contraction).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ICP_REF_HD __host__ __device__
#else
#define ICP_REF_HD
#endif

namespace icp {

// the reference's `norm > 0` filter (slam/loop_closure.py:238-241) on a float32 row: left out unless x*x + y*y + z*z > 0 in
// float32 (a NaN row is left out, a row of subnormals whose squares underflow too, an infinite one is not)
ICP_REF_HD inline bool refine_zero_row(float x, float y, float z) {
    const float s = (x * x + y * y) + z * z;
    return !(s > 0.0f);
}

ICP_REF_HD inline bool refine_finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// p'_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3
ICP_REF_HD inline double refine_move(const double* T, int a, double x, double y, double z) {
    return ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
}

// the cell of a coordinate: floor of a ROUNDED product — the exact floor(v / cell) or its neighbour
ICP_REF_HD inline double refine_cell(double v, double inv_cell) { return floor(v * inv_cell); }

// A lower bound of |v - q| over every coordinate q whose computed cell is k: such a q lies in [k, k + 1) * cell up to the
// rounding of 1 / cell, of the product and of k * cell — a few units of 2^-53 relative to (|k| + 1) * cell; the box is
// widened by 2^-40 of that, far more.  0 inside the box
ICP_REF_HD inline double refine_axis_gap(double v, int k, double cell) {
    const double slack = ((double)(k < 0 ? -k : k) + 1.0) * cell * 9.094947017729282e-13;  // 2^-40
    const double below = ((double)k * cell - slack) - v, above = v - (((double)k + 1.0) * cell + slack);
    const double g = below > above ? below : above;
    return g > 0.0 ? g : 0.0;
}
// ... and what a sum of its squares may be compared with: the sum shrunk by more than its own rounding
ICP_REF_HD inline double refine_gap_floor(double g2) { return g2 * (1.0 - 9.094947017729282e-13); }

// ---- the step: Umeyama without scaling, by Horn's quaternion -----------------------------------------------------------------
// H [9] row-major = sum (q - mu_q)(p' - mu_p)^T / n.  The rotation R with R p' ~ q that maximises trace(R^T H) — for a
// non-degenerate H the U diag(1, 1, sign(det U det V)) V^T of its SVD — is the unit quaternion of the greatest eigenvalue of
// Horn's symmetric 4 x 4 matrix; its eigenvectors come from cyclic Jacobi rotations, so that R is a proper rotation to
// rounding whatever the rank of H (a line, one point, H = 0: the identity).  At most 24 sweeps; a 4 x 4 matrix takes 6 to 8.
ICP_REF_HD inline void refine_rotation(const double* H, double* R) {
    // S_ab = sum p'_a q_b = H_ba
    const double Sxx = H[0], Sxy = H[3], Sxz = H[6], Syx = H[1], Syy = H[4], Syz = H[7], Szx = H[2], Szy = H[5], Szz = H[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    double norm2 = 0.0;
    for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q) norm2 += A[p][q] * A[p][q];
    const double negligible = sqrt(norm2) * 8.673617379884035e-19;  // 2^-60 of the Frobenius norm: 2^-7 of its rounding
    bool rotated = true;
    // (the sweeps stay a loop: unrolled, 24 of them are half a megabyte of straight-line code for ONE lane)
#pragma unroll 1
    for (int sweep = 0; sweep < 24 && rotated; ++sweep) {
        rotated = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) <= negligible) {
                    A[p][q] = A[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = A[p][k] = c * akp - s * akq;
                        A[k][q] = A[q][k] = s * akp + c * akq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > A[best][best]) best = k;
    double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
    const double nn = ((w * w + x * x) + y * y) + z * z;
    if (!(nn > 0.0) || !isfinite(nn)) {
        w = 1.0;
        x = y = z = 0.0;
    } else {
        const double inv = 1.0 / sqrt(nn);
        w *= inv;
        x *= inv;
        y *= inv;
        z *= inv;
    }
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// update [16] = (R, t = mu_q - R mu_p) from the figures of an evaluation (count, sum d2, mu_p [3], mu_q [3], H [9]); the
// identity without a correspondence
ICP_REF_HD inline void refine_step(const double* fig, double* update) {
    for (int i = 0; i < 16; ++i) update[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (!(fig[0] > 0.0)) return;
    double R[9];
    refine_rotation(fig + 8, R);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) update[4 * a + b] = R[3 * a + b];
        update[4 * a + 3] = fig[5 + a] - ((R[3 * a] * fig[2] + R[3 * a + 1] * fig[3]) + R[3 * a + 2] * fig[4]);
    }
}

// out = a b, plain 4 x 4 float64 product, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
ICP_REF_HD inline void refine_mul44(const double* a, const double* b, double* out) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

}  // namespace icp
