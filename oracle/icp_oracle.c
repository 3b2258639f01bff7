/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY.  Nothing under fast-point-cloud-registration-with-gpus_amd/
 * may include, link, import or execute this file; only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg use it, and only as the checker / the timed CPU baseline.
 *
 * What it is: a plain-C, single-threaded restatement of the reference's CPU algorithm for the
 * ICP hot path.  Citations are file:line relative to /root/reference/.
 *
 *   fp64 point-to-point ........ src/ICP_CPU.c:217-271 (+ :342-366)          [icp_oracle_impl.h]
 *   fp32 point-to-point ........ src/CUDA/CPU_ICP_point_to_point.cpp:182-245 [icp_oracle_impl.h]
 *   fp32 point-to-plane ........ src/CUDA/CPU_ICP_point_to-plane.cpp:163-428 [this file]
 *   synthetic clouds ........... src/ICP_CPU.c:51-149, src/ICP_point_to_point.cu:103-190,
 *                                src/ICP_standard.cu:150-262
 *   hall (OS1-16) ingest ....... src/CUDA/GPU_point_to_point_real.cu:20-36,432-623
 *   bunny ingest ............... src/CUDA/GPU_point_to_point_bunny.cu:463-497
 *
 * PARITY STATUS: "parity unpinned" in the strict sense of the build rules.  The reference ships
 * no golden vectors / known-answer tests, and its CPU programs cannot be
 * built in this image without writing stand-in headers (mkl.h, cblas/lapacke prototypes,
 * cuda_runtime.h, ...) which the rules forbid, so the reference itself was not run by this
 * build.  What pins the restatement instead:
 *   (1) the run records of the unmodified reference kept in BASELINE.md section 2
 *       (ICP_CPU.c @ WIDTH 100: 61 iterations, E = 0.82815; @ WIDTH 32: 56 iterations),
 *       reproduced exactly by orc_icp_p2p_f64 (tests/test_oracle.py);
 *   (2) an independent numpy/scipy (LAPACK gesvd) restatement in tests/ref_numpy.py;
 *   (3) the ground-truth transforms the reference bakes into its datasets.
 * Third-party arithmetic: Intel MKL 2021.4.0 (cblas_i?amin, ?gemm, LAPACKE_?gesvd/ssyev/ssysv,
 * VML v?Sub/v?Sqr/v?Add) is not vendored in /root/reference; its published semantics are
 * restated here (i?amin = first index of the minimum absolute value; VML ops round once each).
 *
 * Build: make -C oracle   (gcc -O2 -ffp-contract=off, no -ffast-math, no -march flags).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ------------------------------------------------------------------------------------------
 * 3x3 SVD, one-sided (Hestenes) Jacobi in double.  A row-major; A = U * diag(S) * Vt,
 * S descending, U and V orthogonal.  Stands in for LAPACKE_dgesvd('A','A') (ICP_CPU.c:240).
 * ---------------------------------------------------------------------------------------- */
static void cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

void orc_svd3(const double* A, double* U, double* S, double* Vt)
{
    double a[3][3], v[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            a[i][j] = A[i * 3 + j];
            v[i][j] = (i == j) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 60; sweep++) {
        int rotated = 0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; i++) {
                    alpha += a[i][p] * a[i][p];
                    beta += a[i][q] * a[i][q];
                    gamma += a[i][p] * a[i][q];
                }
                if (gamma == 0.0 || fabs(gamma) <= 1e-300 + 2.3e-16 * sqrt(alpha * beta)) continue;
                rotated = 1;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; i++) {
                    const double x = a[i][p], y = a[i][q];
                    a[i][p] = c * x - s * y;
                    a[i][q] = s * x + c * y;
                    const double vx = v[i][p], vy = v[i][q];
                    v[i][p] = c * vx - s * vy;
                    v[i][q] = s * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
    double sv[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; j++) sv[j] = sqrt(a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j]);
    for (int i = 0; i < 2; i++)
        for (int j = i + 1; j < 3; j++)
            if (sv[ord[j]] > sv[ord[i]]) { int tmp = ord[i]; ord[i] = ord[j]; ord[j] = tmp; }
    double u[3][3]; /* u[k] = k-th left singular vector */
    const double tiny = 1e-14 * (sv[ord[0]] > 0 ? sv[ord[0]] : 1.0);
    int have[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {
        const int j = ord[k];
        S[k] = sv[j];
        if (sv[j] > tiny) {
            for (int i = 0; i < 3; i++) u[k][i] = a[i][j] / sv[j];
            have[k] = 1;
        }
    }
    /* complete U for rank-deficient input (any orthonormal completion) */
    if (!have[0]) { u[0][0] = 1; u[0][1] = 0; u[0][2] = 0; have[0] = 1; }
    if (!have[1]) {
        double e[3] = {0, 0, 0};
        int mi = 0;
        for (int i = 1; i < 3; i++) if (fabs(u[0][i]) < fabs(u[0][mi])) mi = i;
        e[mi] = 1;
        cross3(u[0], e, u[1]);
        const double nn = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
        for (int i = 0; i < 3; i++) u[1][i] /= nn;
        have[1] = 1;
    }
    if (!have[2]) cross3(u[0], u[1], u[2]);
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 3; i++) {
            U[i * 3 + k] = u[k][i];
            Vt[k * 3 + i] = v[i][ord[k]];
        }
}

/* ------------------------------------------------------------------------------------------
 * symmetric 3x3 eigen-decomposition (cyclic Jacobi, double).  Stands in for
 * LAPACKE_ssyev('V','U') (CPU_ICP_point_to-plane.cpp:258): only the upper triangle of A
 * (row-major) is read; w ascending; Z[i*3+k] = i-th component of the k-th eigenvector.
 * ---------------------------------------------------------------------------------------- */
void orc_eigh3(const double* A, double* w, double* Z)
{
    double a[3][3], v[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            a[i][j] = (j >= i) ? A[i * 3 + j] : A[j * 3 + i];
            v[i][j] = (i == j) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 60; sweep++) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (off <= 1e-300 + 1e-17 * dia) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; k++) { /* A <- A * J */
                    const double x = a[k][p], y = a[k][q];
                    a[k][p] = c * x - s * y;
                    a[k][q] = s * x + c * y;
                }
                for (int k = 0; k < 3; k++) { /* A <- J^T * A */
                    const double x = a[p][k], y = a[q][k];
                    a[p][k] = c * x - s * y;
                    a[q][k] = s * x + c * y;
                }
                for (int k = 0; k < 3; k++) {
                    const double x = v[k][p], y = v[k][q];
                    v[k][p] = c * x - s * y;
                    v[k][q] = s * x + c * y;
                }
            }
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; i++)
        for (int j = i + 1; j < 3; j++)
            if (a[ord[j]][ord[j]] < a[ord[i]][ord[i]]) { int tmp = ord[i]; ord[i] = ord[j]; ord[j] = tmp; }
    for (int k = 0; k < 3; k++) {
        w[k] = a[ord[k]][ord[k]];
        for (int i = 0; i < 3; i++) Z[i * 3 + k] = v[i][ord[k]];
    }
}

/* 6x6 dense solve, Gaussian elimination with partial pivoting in double.  Stands in for
 * LAPACKE_ssysv('U') (CPU_ICP_point_to-plane.cpp:371); C row-major FULL matrix (the reference
 * fills all 36 entries through its rank-1 sgemm updates, :354-355).  Returns 0, or k+1 when
 * pivot k is exactly zero (ssysv's info > 0). */
int orc_solve6(const double* C, const double* b, double* x)
{
    double a[6][7];
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < 6; j++) a[i][j] = C[i * 6 + j];
        a[i][6] = b[i];
    }
    for (int k = 0; k < 6; k++) {
        int piv = k;
        for (int i = k + 1; i < 6; i++) if (fabs(a[i][k]) > fabs(a[piv][k])) piv = i;
        if (a[piv][k] == 0.0) return k + 1;
        if (piv != k) for (int j = 0; j < 7; j++) { double tmp = a[k][j]; a[k][j] = a[piv][j]; a[piv][j] = tmp; }
        for (int i = k + 1; i < 6; i++) {
            const double f = a[i][k] / a[k][k];
            for (int j = k; j < 7; j++) a[i][j] -= f * a[k][j];
        }
    }
    for (int i = 5; i >= 0; i--) {
        double s = a[i][6];
        for (int j = i + 1; j < 6; j++) s -= a[i][j] * x[j];
        x[i] = s / a[i][i];
    }
    return 0;
}

/* threads of the matching loops (orc_nn_*): 1 = the reference's scalar loop (default); bench.py's all-cores baseline
 * raises it.  Every moving point is independent, the results do not depend on it. */
static int orc_threads_ = 1;
void orc_set_threads(int k) { orc_threads_ = k > 0 ? k : 1; }
int orc_get_threads(void) { return orc_threads_; }

/* ---- precision-generic point-to-point path ------------------------------------------------ */
#define REAL double
#define SUF f64
#include "icp_oracle_impl.h"
#undef REAL
#undef SUF
#define REAL float
#define SUF f32
#include "icp_oracle_impl.h"
#undef REAL
#undef SUF

/* ------------------------------------------------------------------------------------------
 * fp32 clouds, fp64 minimisation ("f32x").  The fp32 twin above follows the reference file to the
 * letter, including its naive sequential float sums for the centroids
 * (src/CUDA/CPU_ICP_point_to_point.cpp:335-352), which carry ~1e-5 of summation noise at 16 384
 * points.  The product keeps the reference's fp32 matching arithmetic (that is what decides the
 * indices) but reduces in fp64, i.e. it applies src/ICP_CPU.c's fp64 minimisation (:237-248) to the
 * fp32 cloud.  This variant restates exactly that combination: orc_nn_f32 for the matching,
 * orc_p2p_minimize_f64 on the widened cloud, R and t rounded to float, orc_transform_f32, and the
 * error norm of src/ICP_CPU.c:257-266 in double.
 * ---------------------------------------------------------------------------------------- */
int orc_icp_p2p_f32x(const float* D, const float* M, int n, int m, int max_iter, double tol, int fixed,
                     double* E, double* T_total, int* idx_last, float* pt_out, int* passes)
{
    const size_t ns = (size_t)n, ms = (size_t)m;
    float* pt = (float*)malloc(3 * ns * sizeof(float));
    double* ptd = (double*)malloc(3 * ns * sizeof(double));
    double* qd = (double*)malloc(3 * ms * sizeof(double));
    int* q_idx = (int*)malloc(ns * sizeof(int));
    if (!pt || !ptd || !qd || !q_idx) { free(pt); free(ptd); free(qd); free(q_idx); return -1; }
    memcpy(pt, D, 3 * ns * sizeof(float));
    for (size_t i = 0; i < 3 * ms; i++) qd[i] = (double)M[i];
    for (int k = 0; k <= max_iter; k++) E[k] = 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int i = 0, npass = 0;
    while (1) {
        orc_nn_f32(pt, n, M, m, q_idx);
        npass++;
        for (size_t k = 0; k < 3 * ns; k++) ptd[k] = (double)pt[k];
        double Rd[9], td[3];
        if (orc_p2p_minimize_f64(ptd, n, qd, m, q_idx, Rd, td, NULL)) { i = -1; break; }
        float R[9], t[3];
        for (int k = 0; k < 9; k++) R[k] = (float)Rd[k];
        for (int k = 0; k < 3; k++) t[k] = (float)td[k];
        orc_transform_f32(pt, n, R, t);
        {
            double Tk[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
            double Tn[16];
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    double s = 0;
                    for (int k = 0; k < 4; k++) s += Tk[a * 4 + k] * T[k * 4 + b];
                    Tn[a * 4 + b] = s;
                }
            memcpy(T, Tn, sizeof T);
        }
        for (size_t k = 0; k < 3 * ns; k++) ptd[k] = (double)pt[k];
        E[i + 1] = orc_rms_error_f64(ptd, n, qd, m, q_idx);
        if (!fixed && ((E[i + 1] < tol) || (fabs(E[i + 1] - E[i]) < tol))) break;
        i++;
        if (i > max_iter - 1) break;
    }
    if (T_total) memcpy(T_total, T, sizeof T);
    if (idx_last) memcpy(idx_last, q_idx, ns * sizeof(int));
    if (pt_out) memcpy(pt_out, pt, 3 * ns * sizeof(float));
    if (passes) *passes = npass;
    free(pt); free(ptd); free(qd); free(q_idx);
    return i;
}

/* ------------------------------------------------------------------------------------------
 * Synthetic clouds.
 * ---------------------------------------------------------------------------------------- */

/* ICP_CPU.c:51-149 (fp64, SoA).  lin[i] = min + i*len/(W-1); point k*W+j = (lin[k], lin[j]);
 * z = x^2 - y^2; M = r*D + t with r = (rx*ry)*rz, the matrices of :110-126 (+sin above the
 * diagonal), t = (1,-0.3,0.2), angles (1,-0.5,0.05) rad.  The reference's second dgemm aliases
 * r as input and output (:133); the mathematically intended product is restated here (it
 * reproduces the reference's recorded iteration counts, see header). */
void orc_synth_icp_cpu_f64(int W, double xy_min, double xy_max, double* D, double* M)
{
    const int n = W * W;
    const double length = xy_max - xy_min;
    double* lin = (double*)malloc((size_t)W * sizeof(double));
    for (int i = 0; i < W; i++) lin[i] = xy_min + (double)i * length / ((double)W - 1.0);
    for (int k = 0; k < W; k++)
        for (int j = 0; j < W; j++) {
            const int i = k * W + j;
            const double x = lin[k], y = lin[j];
            D[i] = x;
            D[i + n] = y;
            D[i + 2 * (size_t)n] = pow(x, 2) - pow(y, 2);
        }
    free(lin);
    const double ti[3] = {1.0, -0.3, 0.2};
    const double ri[3] = {1, -0.5, 0.05};
    const double rx[3][3] = {{1, 0, 0}, {0, cos(ri[0]), sin(ri[0])}, {0, -sin(ri[0]), cos(ri[0])}};
    const double ry[3][3] = {{cos(ri[1]), 0, -sin(ri[1])}, {0, 1, 0}, {sin(ri[1]), 0, cos(ri[1])}};
    const double rz[3][3] = {{cos(ri[2]), sin(ri[2]), 0}, {-sin(ri[2]), cos(ri[2]), 0}, {0, 0, 1}};
    double r1[3][3], r[3][3];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += rx[a][k] * ry[k][b];
            r1[a][b] = s;
        }
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += r1[a][k] * rz[k][b];
            r[a][b] = s;
        }
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            double s = r[a][0] * D[i];
            s += r[a][1] * D[i + n];
            s += r[a][2] * D[i + 2 * (size_t)n];
            M[i + (size_t)n * a] = s + ti[a];
        }
}

/* closed-form column-major rotation used by every fp32 GPU program
 * (ICP_point_to_point.cu:167-172, GPU_point_to_point_real.cu:595-599, ..._bunny.cu:146-150) */
void orc_rotation_gpu_f32(float rx, float ry, float rz, float* h_r /*9, column-major*/)
{
    const float cx = (float)cos(rx), cy = (float)cos(ry), cz = (float)cos(rz);
    const float sx = (float)sin(rx), sy = (float)sin(ry), sz = (float)sin(rz);
    h_r[0] = cy * cz; h_r[1] = (cz * sx * sy) + (cx * sz); h_r[2] = -(cx * cz * sy) + (sx * sz);
    h_r[3] = -cy * sz; h_r[4] = (cx * cz) - (sx * sy * sz); h_r[5] = (cx * sy * sz) + (cz * sx);
    h_r[6] = sy; h_r[7] = -cy * sx; h_r[8] = cx * cy;
}

/* M = h_r * D + t for AoS clouds, the arithmetic of SmatrixMul + the "+= ti" loop
 * (ICP_point_to_point.cu:182-190, :463-476): temp = 0; temp += A*B three times; then + t. */
void orc_apply_gpu_model_f32(const float* h_r, const float* t, const float* D_aos, int n, float* M_aos)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) {
            float temp = 0.0f;
            for (int q = 0; q < 3; q++) temp += h_r[j + q * 3] * D_aos[q + i * 3];
            M_aos[j + i * 3] = temp;
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) M_aos[j + i * 3] += t[j];
}

/* ICP_point_to_point.cu:103-190 / ICP_point_to_plane.cu (same generator), fp32 AoS.
 * lin[i] = (float)min + ((float)i*(float)len)/((float)W - 1.0f); z = pow(x,2) - pow(y,2)
 * evaluated in double (C++ pow(float,int) promotes) and rounded to float on assignment. */
void orc_synth_grid_f32(int W, float xy_min, float xy_max, float* D_aos)
{
    const float length = xy_max - xy_min;
    float* lin = (float*)malloc((size_t)W * sizeof(float));
    for (int i = 0; i < W; i++) lin[i] = xy_min + ((float)i * length) / ((float)W - 1.0f);
    for (int k = 0; k < W; k++)
        for (int j = 0; j < W; j++) {
            const int i = k * W + j;
            const float x = lin[k], y = lin[j];
            D_aos[3 * i + 0] = x;
            D_aos[3 * i + 1] = y;
            D_aos[3 * i + 2] = (float)(pow((double)x, 2) - pow((double)y, 2));
        }
    free(lin);
}

/* ICP_standard.cu:150-262: 32x32 grid as above, t = (1,-0.3,0.2), and the HARD-CODED h_r of
 * :247-249 (not the product of its own rx, ry, rz). */
void orc_synth_icp_standard_f32(int W, float* D_aos, float* M_aos)
{
    static const float h_r[9] = {0.876485812f, -0.37591464f, 0.300767018f,
                                 -0.04386084f, 0.559789799f, 0.827473024f,
                                 -0.47942553f, -0.73846026f, 0.474159881f};
    static const float ti[3] = {1.0f, -0.3f, 0.2f};
    orc_synth_grid_f32(W, -2.0f, 2.0f, D_aos);
    orc_apply_gpu_model_f32(h_r, ti, D_aos, W * W, M_aos);
}

/* ------------------------------------------------------------------------------------------
 * Point-to-plane, fp32: CPU_ICP_point_to-plane.cpp.  SoA clouds.
 * ---------------------------------------------------------------------------------------- */

/* :184-202  k=4 neighbours: k+1 passes of first-argmin with overwrite-by-10000, rank 0 (self
 * or an equal-distance lower index) dropped. */
void orc_knn4_f32(const float* q, int m, int* neighborIds /* m*4 */)
{
    const size_t ms = (size_t)m;
    float* dist = (float*)malloc(ms * sizeof(float));
    for (int i = 0; i < m; i++) {
        const float px = q[i], py = q[i + ms], pz = q[i + 2 * ms];
        for (int c = 0; c < m; c++) {
            float dx = q[c] - px, dy = q[c + ms] - py, dz = q[c + 2 * ms] - pz;
            dx = dx * dx; dy = dy * dy; dz = dz * dz;
            float d = dx + dy;
            dist[c] = d + dz;
        }
        for (int j = 0; j < 5; j++) {
            int idx_min = 0;
            float best = fabsf(dist[0]);
            for (int c = 1; c < m; c++)
                if (fabsf(dist[c]) < best) { best = fabsf(dist[c]); idx_min = c; }
            if (j > 0) neighborIds[(j - 1) + i * 4] = idx_min;
            dist[idx_min] = 10000.0f;
        }
    }
    free(dist);
}

/* :213-275  PCA normals.  bar = (sum of 4 neighbours) * (1/4) in float, upper-triangular
 * covariance (not divided by k) in float, eigenvector of the eigenvalue with the smallest
 * ABSOLUTE value among the ascending eigenvalues (cblas_isamin(3, w), first on ties).
 * A_out (optional, m*9) receives the float covariance that was handed to the eigen-solver. */
void orc_normals_f32(const float* q, int m, const int* neighborIds, float* normals /*SoA*/, float* A_out)
{
    const size_t ms = (size_t)m;
    const int k = 4;
    for (int i = 0; i < m; i++) {
        float bar[3] = {0.0f, 0.0f, 0.0f};
        for (int j = 0; j < k; j++) {
            const int s = neighborIds[j + i * k];
            bar[0] += q[s];
            bar[1] += q[s + ms];
            bar[2] += q[s + 2 * ms];
        }
        const float a = 1 / (float)k;
        bar[0] *= a; bar[1] *= a; bar[2] *= a;
        float A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < k; j++) {
            const int s = neighborIds[j + i * k];
            const float xi = q[s], yi = q[s + ms], zi = q[s + 2 * ms];
            A[0] += (xi - bar[0]) * (xi - bar[0]);
            A[1] += (xi - bar[0]) * (yi - bar[1]);
            A[2] += (xi - bar[0]) * (zi - bar[2]);
            A[4] += (yi - bar[1]) * (yi - bar[1]);
            A[5] += (yi - bar[1]) * (zi - bar[2]);
            A[8] += (zi - bar[2]) * (zi - bar[2]);
        }
        if (A_out) memcpy(A_out + 9 * (size_t)i, A, sizeof A);
        double Ad[9], w[3], Z[9];
        for (int e = 0; e < 9; e++) Ad[e] = (double)A[e];
        orc_eigh3(Ad, w, Z);
        int idx_min = 0;
        for (int e = 1; e < 3; e++) if (fabs((float)w[e]) < fabs((float)w[idx_min])) idx_min = e;
        for (int j = 0; j < 3; j++) normals[i + ms * j] = (float)Z[j * 3 + idx_min];
    }
}

/* :338-387  one minimisation: C = sum cn cn^T, b = -sum cn * ((p - q_idx) . n), solve C x = b,
 * R = Rz(x2) Ry(x1) Rx(x0) (row-major, :381-383), t = x[3..5].  accumulate_f64 = 0 follows the
 * reference (float accumulators); 1 accumulates C and b in double (tight check of the product). */
int orc_p2plane_minimize_f32(const float* p, int n, const float* q, int m, const int* q_idx,
                             const float* normals, int accumulate_f64, float* R, float* t,
                             double* C_out /*36 or NULL*/, double* b_out /*6 or NULL*/)
{
    const size_t ns = (size_t)n, ms = (size_t)m;
    float Cf[36], bf[6];
    double Cd[36], bd[6];
    for (int e = 0; e < 36; e++) { Cf[e] = 0; Cd[e] = 0; }
    for (int e = 0; e < 6; e++) { bf[e] = 0; bd[e] = 0; }
    for (int i = 0; i < n; i++) {
        const int s = q_idx[i];
        float cn[6];
        cn[0] = p[i + ns] * normals[s + 2 * ms] - p[i + 2 * ns] * normals[s + ms];
        cn[1] = p[i + 2 * ns] * normals[s] - p[i] * normals[s + 2 * ms];
        cn[2] = p[i] * normals[s + ms] - p[i + ns] * normals[s];
        cn[3] = normals[s];
        cn[4] = normals[s + ms];
        cn[5] = normals[s + 2 * ms];
        const float bi = (p[i] - q[s]) * cn[3] + (p[i + ns] - q[s + ms]) * cn[4] + (p[i + 2 * ns] - q[s + 2 * ms]) * cn[5];
        if (accumulate_f64) {
            for (int a = 0; a < 6; a++) {
                for (int c = 0; c < 6; c++) Cd[a * 6 + c] += (double)cn[a] * (double)cn[c];
                bd[a] += -1.0 * (double)cn[a] * (double)bi;
            }
        } else {
            for (int a = 0; a < 6; a++) {
                for (int c = 0; c < 6; c++) Cf[a * 6 + c] += cn[a] * cn[c];
                bf[a] += (-1) * cn[a] * bi;
            }
        }
    }
    if (!accumulate_f64) {
        for (int e = 0; e < 36; e++) Cd[e] = (double)Cf[e];
        for (int e = 0; e < 6; e++) bd[e] = (double)bf[e];
    }
    if (C_out) memcpy(C_out, Cd, sizeof Cd);
    if (b_out) memcpy(b_out, bd, sizeof bd);
    double x[6];
    const int info = orc_solve6(Cd, bd, x);
    if (info) return info;
    float bx[6];
    for (int e = 0; e < 6; e++) bx[e] = (float)x[e];
    const float cx = (float)cos(bx[0]), cy = (float)cos(bx[1]), cz = (float)cos(bx[2]);
    const float sx = (float)sin(bx[0]), sy = (float)sin(bx[1]), sz = (float)sin(bx[2]);
    R[0] = cy * cz; R[1] = cz * sx * sy - cx * sz; R[2] = cx * cz * sy + sx * sz;
    R[3] = cy * sz; R[4] = cx * cz + sx * sy * sz; R[5] = cx * sy * sz - cz * sx;
    R[6] = -sy; R[7] = cy * sx; R[8] = cx * cy;
    t[0] = bx[3]; t[1] = bx[4]; t[2] = bx[5];
    return 0;
}

/* :309-428 driver.  tol 1e-6 in the reference; fixed != 0 disables the tolerance test. */
int orc_icp_p2plane_f32(const float* D, const float* M, int n, int m, const float* normals, int max_iter,
                        double tol, int fixed, int accumulate_f64, float* E, double* T_total,
                        int* idx_last, float* pt_out, int* passes)
{
    const size_t ns = (size_t)n;
    float* p = (float*)malloc(3 * ns * sizeof(float));
    int* q_idx = (int*)malloc(ns * sizeof(int));
    memcpy(p, D, 3 * ns * sizeof(float));
    for (int k = 0; k <= max_iter; k++) E[k] = 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int it = 0, npass = 0, rc = 0;
    while (it < max_iter) {
        orc_nn_f32(p, n, M, m, q_idx);
        npass++;
        float R[9], t[3];
        rc = orc_p2plane_minimize_f32(p, n, M, m, q_idx, normals, accumulate_f64, R, t, NULL, NULL);
        if (rc) break;
        orc_transform_f32(p, n, R, t);
        {
            double Tk[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
            double Tn[16];
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    double s = 0;
                    for (int k = 0; k < 4; k++) s += Tk[a * 4 + k] * T[k * 4 + b];
                    Tn[a * 4 + b] = s;
                }
            memcpy(T, Tn, sizeof T);
        }
        E[it + 1] = orc_rms_error_f32(p, n, M, m, q_idx);
        if (!fixed && ((E[it + 1] < tol) || (fabs((double)E[it + 1] - (double)E[it]) < tol))) break;
        it++;
    }
    if (T_total) memcpy(T_total, T, sizeof T);
    if (idx_last) memcpy(idx_last, q_idx, ns * sizeof(int));
    if (pt_out) memcpy(pt_out, p, 3 * ns * sizeof(float));
    if (passes) *passes = npass;
    free(p);
    free(q_idx);
    return rc ? -rc : it;
}

/* ------------------------------------------------------------------------------------------
 * Point-to-plane with fp32 matching and fp64 minimisation -- the point-to-plane sibling of
 * orc_icp_p2p_f32x, and for the same reason: the letter-faithful fp32 twin above accumulates the
 * 6x6 system, evaluates the Euler rotation and sums the error norm in float (1e-4 .. 1e-3 of noise
 * in the motion of one pass), which no tight gate can be hung on.  Here the float cloud and the
 * float normals are widened, c = p x n, C = sum [c;n][c;n]^T and b = -sum [c;n]((p - q).n) are formed
 * and summed in double (statements of CPU_ICP_point_to-plane.cpp:338-376), the 6x6 system is solved
 * in double, R = Rz Ry Rx (:379-387) is evaluated in double and rounded to float together with t,
 * the cloud is moved in float (orc_transform_f32: the arithmetic of RyT) and the error norm
 * (src/ICP_CPU.c:257-266) is taken in double.  Matching stays orc_nn_f32: the indices -- the part
 * that has to be bit-exact -- are decided by float arithmetic alone.
 * ---------------------------------------------------------------------------------------- */
int orc_p2plane_minimize_f32x(const float* p, int n, const float* q, int m, const int* q_idx,
                              const float* normals, double* R /*9, row-major*/, double* t /*3*/,
                              double* C_out /*36 or NULL*/, double* b_out /*6 or NULL*/)
{
    const size_t ns = (size_t)n, ms = (size_t)m;
    double Cd[36], bd[6];
    for (int e = 0; e < 36; e++) Cd[e] = 0;
    for (int e = 0; e < 6; e++) bd[e] = 0;
    for (int i = 0; i < n; i++) {
        const int s = q_idx[i];
        const double px = (double)p[i], py = (double)p[i + ns], pz = (double)p[i + 2 * ns];
        const double nx = (double)normals[s], ny = (double)normals[s + ms], nz = (double)normals[s + 2 * ms];
        double cn[6];
        cn[0] = py * nz - pz * ny;
        cn[1] = pz * nx - px * nz;
        cn[2] = px * ny - py * nx;
        cn[3] = nx; cn[4] = ny; cn[5] = nz;
        const double bi = (px - (double)q[s]) * nx + (py - (double)q[s + ms]) * ny + (pz - (double)q[s + 2 * ms]) * nz;
        for (int a = 0; a < 6; a++) {
            for (int c = 0; c < 6; c++) Cd[a * 6 + c] += cn[a] * cn[c];
            bd[a] -= cn[a] * bi;
        }
    }
    if (C_out) memcpy(C_out, Cd, sizeof Cd);
    if (b_out) memcpy(b_out, bd, sizeof bd);
    double x[6];
    const int info = orc_solve6(Cd, bd, x);
    if (info) return info;
    const double cx = cos(x[0]), cy = cos(x[1]), cz = cos(x[2]);
    const double sx = sin(x[0]), sy = sin(x[1]), sz = sin(x[2]);
    R[0] = cy * cz; R[1] = cz * sx * sy - cx * sz; R[2] = cx * cz * sy + sx * sz;
    R[3] = cy * sz; R[4] = cx * cz + sx * sy * sz; R[5] = cx * sy * sz - cz * sx;
    R[6] = -sy; R[7] = cy * sx; R[8] = cx * cy;
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
    return 0;
}

int orc_icp_p2plane_f32x(const float* D, const float* M, int n, int m, const float* normals, int max_iter,
                         double tol, int fixed, double* E, double* T_total, int* idx_last, float* pt_out, int* passes)
{
    const size_t ns = (size_t)n, ms = (size_t)m;
    float* p = (float*)malloc(3 * ns * sizeof(float));
    double* pd = (double*)malloc(3 * ns * sizeof(double));
    double* qd = (double*)malloc(3 * ms * sizeof(double));
    int* q_idx = (int*)malloc(ns * sizeof(int));
    if (!p || !pd || !qd || !q_idx) { free(p); free(pd); free(qd); free(q_idx); return -1; }
    memcpy(p, D, 3 * ns * sizeof(float));
    for (size_t i = 0; i < 3 * ms; i++) qd[i] = (double)M[i];
    for (int k = 0; k <= max_iter; k++) E[k] = 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int it = 0, npass = 0, rc = 0;
    while (it < max_iter) {   /* CPU_ICP_point_to-plane.cpp:309 */
        orc_nn_f32(p, n, M, m, q_idx);
        npass++;
        double Rd[9], td[3];
        rc = orc_p2plane_minimize_f32x(p, n, M, m, q_idx, normals, Rd, td, NULL, NULL);
        if (rc) break;
        float R[9], t[3];
        for (int k = 0; k < 9; k++) R[k] = (float)Rd[k];
        for (int k = 0; k < 3; k++) t[k] = (float)td[k];
        orc_transform_f32(p, n, R, t);
        {
            double Tk[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
            double Tn[16];
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    double s = 0;
                    for (int k = 0; k < 4; k++) s += Tk[a * 4 + k] * T[k * 4 + b];
                    Tn[a * 4 + b] = s;
                }
            memcpy(T, Tn, sizeof T);
        }
        for (size_t k = 0; k < 3 * ns; k++) pd[k] = (double)p[k];
        E[it + 1] = orc_rms_error_f64(pd, n, qd, m, q_idx);
        if (!fixed && ((E[it + 1] < tol) || (fabs(E[it + 1] - E[it]) < tol))) break;   /* :420-421 */
        it++;
    }
    if (T_total) memcpy(T_total, T, sizeof T);
    if (idx_last) memcpy(idx_last, q_idx, ns * sizeof(int));
    if (pt_out) memcpy(pt_out, p, 3 * ns * sizeof(float));
    if (passes) *passes = npass;
    free(p); free(pd); free(qd); free(q_idx);
    return rc ? -rc : it;
}

/* ------------------------------------------------------------------------------------------
 * Point-to-plane, fp64.  The reference has no such program (its fp64 program, src/ICP_CPU.c, is
 * point-to-point only); the product offers ICP_F64 + ICP_POINT_TO_PLANE, and this is its checker:
 * the statements of the fp32 plane path above with `double` throughout, the matching of
 * src/ICP_CPU.c (orc_nn_f64).
 * ---------------------------------------------------------------------------------------- */

/* k=4 neighbours: distance (dx*dx + dy*dy) + dz*dz with every operation rounded in double; the
 * first five of the (d, j)-ascending order of the model, rank 0 (self or an equal-distance lower
 * index) dropped.  The order is stated directly -- a sorted top-5 kept over one ascending scan,
 * a candidate going behind every entry with d_e <= d -- instead of the fp32 twin's k+1 passes of
 * first-argmin with overwrite-by-10000, which stop being that order once distances exceed 10000.
 * The candidates are the points with d < +inf (include/icp_mi355x.h, icp_estimate_normals): an
 * overflowed distance enters nothing, and a rank that does not exist holds index 0. */
void orc_knn4_f64(const double* q, int m, int* neighborIds /* m*4 */)
{
    const size_t ms = (size_t)m;
    for (int i = 0; i < m; i++) {
        const double px = q[i], py = q[i + ms], pz = q[i + 2 * ms];
        double bd[5];
        int bj[5], have = 0;
        for (int c = 0; c < m; c++) {
            double dx = q[c] - px, dy = q[c + ms] - py, dz = q[c + 2 * ms] - pz;
            dx = dx * dx; dy = dy * dy; dz = dz * dz;
            double d = dx + dy;
            d = d + dz;
            if (!(d < INFINITY)) continue;
            if (have == 5 && !(d < bd[4])) continue;
            int r = have < 5 ? have : 4;              /* the slot that opens at the end */
            while (r > 0 && d < bd[r - 1]) { bd[r] = bd[r - 1]; bj[r] = bj[r - 1]; r--; }
            bd[r] = d; bj[r] = c;
            if (have < 5) have++;
        }
        for (int r = 1; r < 5; r++) neighborIds[(r - 1) + i * 4] = r < have ? bj[r] : 0;
    }
}

/* orc_normals_f32's statements in double: bar = (sum of 4 neighbours) * 0.25, upper-triangular
 * covariance (not divided by k), orc_eigh3, the eigenvector of the eigenvalue of smallest magnitude
 * among the ascending ones (first on ties).  A_out (optional, m*9): the covariance handed to the
 * eigen-solver. */
void orc_normals_f64(const double* q, int m, const int* neighborIds, double* normals /*SoA*/, double* A_out)
{
    const size_t ms = (size_t)m;
    const int k = 4;
    for (int i = 0; i < m; i++) {
        double bar[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < k; j++) {
            const int s = neighborIds[j + i * k];
            bar[0] += q[s];
            bar[1] += q[s + ms];
            bar[2] += q[s + 2 * ms];
        }
        const double a = 1 / (double)k;
        bar[0] *= a; bar[1] *= a; bar[2] *= a;
        double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < k; j++) {
            const int s = neighborIds[j + i * k];
            const double xi = q[s], yi = q[s + ms], zi = q[s + 2 * ms];
            A[0] += (xi - bar[0]) * (xi - bar[0]);
            A[1] += (xi - bar[0]) * (yi - bar[1]);
            A[2] += (xi - bar[0]) * (zi - bar[2]);
            A[4] += (yi - bar[1]) * (yi - bar[1]);
            A[5] += (yi - bar[1]) * (zi - bar[2]);
            A[8] += (zi - bar[2]) * (zi - bar[2]);
        }
        if (A_out) memcpy(A_out + 9 * (size_t)i, A, sizeof A);
        /* orc_eigh3's stop test has an absolute floor (1e-300) and adds magnitudes: a covariance
         * beyond 2^+-400 is handed over times an exact power of two, which changes no rotation,
         * and its eigenvalues are scaled back; every other one goes through as it is. */
        double As[9], w[3], Z[9], amax = 0.0, sc = 1.0;
        for (int e = 0; e < 9; e++) if (fabs(A[e]) > amax) amax = fabs(A[e]);
        if (amax > 0x1p+400) sc = 0x1p-600;
        else if (amax < 0x1p-400 && amax > 0.0) sc = 0x1p+600;
        for (int e = 0; e < 9; e++) As[e] = A[e] * sc;
        orc_eigh3(As, w, Z);
        for (int e = 0; e < 3; e++) w[e] *= 1.0 / sc;
        int idx_min = 0;
        for (int e = 1; e < 3; e++) if (fabs(w[e]) < fabs(w[idx_min])) idx_min = e;
        for (int j = 0; j < 3; j++) normals[i + ms * j] = Z[j * 3 + idx_min];
    }
}

/* the statements of orc_p2plane_minimize_f32x on double inputs */
int orc_p2plane_minimize_f64(const double* p, int n, const double* q, int m, const int* q_idx,
                             const double* normals, double* R /*9, row-major*/, double* t /*3*/,
                             double* C_out /*36 or NULL*/, double* b_out /*6 or NULL*/)
{
    const size_t ns = (size_t)n, ms = (size_t)m;
    double Cd[36], bd[6];
    for (int e = 0; e < 36; e++) Cd[e] = 0;
    for (int e = 0; e < 6; e++) bd[e] = 0;
    for (int i = 0; i < n; i++) {
        const int s = q_idx[i];
        const double px = p[i], py = p[i + ns], pz = p[i + 2 * ns];
        const double nx = normals[s], ny = normals[s + ms], nz = normals[s + 2 * ms];
        double cn[6];
        cn[0] = py * nz - pz * ny;
        cn[1] = pz * nx - px * nz;
        cn[2] = px * ny - py * nx;
        cn[3] = nx; cn[4] = ny; cn[5] = nz;
        const double bi = (px - q[s]) * nx + (py - q[s + ms]) * ny + (pz - q[s + 2 * ms]) * nz;
        for (int a = 0; a < 6; a++) {
            for (int c = 0; c < 6; c++) Cd[a * 6 + c] += cn[a] * cn[c];
            bd[a] -= cn[a] * bi;
        }
    }
    if (C_out) memcpy(C_out, Cd, sizeof Cd);
    if (b_out) memcpy(b_out, bd, sizeof bd);
    double x[6];
    const int info = orc_solve6(Cd, bd, x);
    if (info) return info;
    const double cx = cos(x[0]), cy = cos(x[1]), cz = cos(x[2]);
    const double sx = sin(x[0]), sy = sin(x[1]), sz = sin(x[2]);
    R[0] = cy * cz; R[1] = cz * sx * sy - cx * sz; R[2] = cx * cz * sy + sx * sz;
    R[3] = cy * sz; R[4] = cx * cz + sx * sy * sz; R[5] = cx * sy * sz - cz * sx;
    R[6] = -sy; R[7] = cy * sx; R[8] = cx * cy;
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
    return 0;
}

/* orc_icp_p2plane_f32x's loop with the cloud, R = Rz Ry Rx and t kept in double: orc_nn_f64,
 * orc_transform_f64, orc_rms_error_f64; the same stop rule and the same `fixed` flag. */
int orc_icp_p2plane_f64(const double* D, const double* M, int n, int m, const double* normals, int max_iter,
                        double tol, int fixed, double* E, double* T_total, int* idx_last, double* pt_out, int* passes)
{
    const size_t ns = (size_t)n;
    double* p = (double*)malloc(3 * ns * sizeof(double));
    int* q_idx = (int*)malloc(ns * sizeof(int));
    if (!p || !q_idx) { free(p); free(q_idx); return -1; }
    memcpy(p, D, 3 * ns * sizeof(double));
    for (int k = 0; k <= max_iter; k++) E[k] = 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int it = 0, npass = 0, rc = 0;
    while (it < max_iter) {
        orc_nn_f64(p, n, M, m, q_idx);
        npass++;
        double R[9], t[3];
        rc = orc_p2plane_minimize_f64(p, n, M, m, q_idx, normals, R, t, NULL, NULL);
        if (rc) break;
        orc_transform_f64(p, n, R, t);
        {
            double Tk[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
            double Tn[16];
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    double s = 0;
                    for (int k = 0; k < 4; k++) s += Tk[a * 4 + k] * T[k * 4 + b];
                    Tn[a * 4 + b] = s;
                }
            memcpy(T, Tn, sizeof T);
        }
        E[it + 1] = orc_rms_error_f64(p, n, M, m, q_idx);
        if (!fixed && ((E[it + 1] < tol) || (fabs(E[it + 1] - E[it]) < tol))) break;
        it++;
    }
    if (T_total) memcpy(T_total, T, sizeof T);
    if (idx_last) memcpy(idx_last, q_idx, ns * sizeof(int));
    if (pt_out) memcpy(pt_out, p, 3 * ns * sizeof(double));
    if (passes) *passes = npass;
    free(p); free(q_idx);
    return rc ? -rc : it;
}

/* ------------------------------------------------------------------------------------------
 * Hall ingest: GPU_point_to_point_real.cu:432-623.
 * ---------------------------------------------------------------------------------------- */

/* :457-488  the line-number state machine over the one-byte-per-line dump.  `lines` holds the
 * atoi() of every text line (n_lines of them).  Writes up to cap ranges (mm, as float) and the
 * encoder count of the first azimuth block; returns the number of ranges produced. */
int orc_os1_ranges_from_lines(const int* lines, int n_lines, float* h_r, int cap, unsigned long* encoder_count)
{
    unsigned long h_encoder_count = 0;
    int offset = 0;
    unsigned long word = 0;
    int channel = 2, azimuth_block = 0, lidar_packet = 0, idx_line;
    int j = 1;
    for (int li = 0; li < n_lines; li++) {
        const int v = lines[li];
        if (j == 13) h_encoder_count = (unsigned long)v;
        if (j == 14) h_encoder_count = (unsigned long)(v << 8) | h_encoder_count;
        idx_line = 17 + 12 * channel + 788 * azimuth_block + 12608 * lidar_packet;
        if (j == idx_line) word = (unsigned long)v;
        if (j == idx_line + 1) word = (unsigned long)(v << 8) | word;
        if (j == idx_line + 2) word = (unsigned long)((v & 0x0000000F) << 16) | word;
        if (j > (idx_line + 2)) {
            if (offset < cap) h_r[offset] = (float)word;
            offset++;
            channel += 4;
        }
        if (channel >= 64) { channel = 2; azimuth_block++; }
        if (azimuth_block >= 16) { azimuth_block = 0; lidar_packet++; }
        if (lidar_packet >= 64) break;
        j++;
    }
    if (encoder_count) *encoder_count = h_encoder_count;
    return offset;
}

/* :503-527  beam_intrinsics.csv: line 1 header, lines 2..65 altitude, 66 blank, 67 header,
 * 68..131 azimuth; every 4th value starting at the 3rd (j%4==0 resp. (j-66)%4==0). */
void orc_os1_select_beams(const double* alt64, const double* az64, float* alt16, float* az16)
{
    int o = 0;
    for (int j = 2; j <= 65; j++) if (j % 4 == 0) alt16[o++] = (float)alt64[j - 2];
    o = 0;
    for (int j = 68; j <= 131; j++) if ((j - 66) % 4 == 0) az16[o++] = (float)az64[j - 68];
}

/* :20-36  Conversion kernel, one point per thread, output AoS in mm. */
void orc_os1_conversion_f32(const float* r, int n, unsigned long encoder0, const float* altitude,
                            const float* azimuth, float* point_cloud)
{
    for (int i = 0; i < n; i++) {
        const int azimuth_block = i / 16;
        const unsigned long counter = (encoder0 + (unsigned long)azimuth_block * 88) % 90112;
        const int channel = i % 16;
        const float theta = (float)(2 * M_PI * (counter / 90112.0 + azimuth[channel] / 360.0));
        const float phi = (float)(2 * M_PI * altitude[channel] / 360.0);
        point_cloud[0 + 3 * i] = (float)(r[i] * cosf(theta) * cosf(phi));
        point_cloud[1 + 3 * i] = (float)(-r[i] * sinf(theta) * cosf(phi));
        point_cloud[2 + 3 * i] = (float)(r[i] * sinf(phi));
    }
}

/* RyT, :81-88 of ICP_point_to_point.cu (column-major R, AoS clouds), as used to build the hall
 * model cloud in mm (GPU_point_to_point_real.cu:606) */
void orc_ryt_f32(const float* R, const float* T, const float* P, int n, float* Q)
{
    for (int i = 0; i < n; i++) {
        const float x = P[0 + i * 3], y = P[1 + i * 3], z = P[2 + i * 3];
        Q[0 + i * 3] = R[0 + 0 * 3] * x + R[0 + 1 * 3] * y + R[0 + 2 * 3] * z + T[0];
        Q[1 + i * 3] = R[1 + 0 * 3] * x + R[1 + 1 * 3] * y + R[1 + 2 * 3] * z + T[1];
        Q[2 + i * 3] = R[2 + 0 * 3] * x + R[2 + 1 * 3] * y + R[2 + 2 * 3] * z + T[2];
    }
}

/* bunny: GPU_point_to_point_bunny.cu:463-497 -- tokens split on " \n" (';' accepted as well so
 * that both Bunny_res.csv and Bunny.csv parse), strtof each token into AoS order. */
int orc_read_xyz_text(const char* path, float* out_aos, int cap_floats)
{
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    char line[2048];
    int i = 0;
    while (fgets(line, sizeof line, f)) {
        char* save = NULL;
        for (char* tok = strtok_r(line, " ;\n", &save); tok; tok = strtok_r(NULL, " ;\n", &save)) {
            char* end = NULL;
            const float v = strtof(tok, &end);
            if (end == tok) continue; /* e.g. a lone "\r" */
            if (i < cap_floats) out_aos[i] = v;
            i++;
        }
    }
    fclose(f);
    return i;
}

/* layout helpers for the tests */
void orc_aos_to_soa_f32(const float* aos, int n, float* soa)
{
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) soa[i + (size_t)n * k] = aos[3 * i + k];
}
void orc_aos_to_soa_f64(const double* aos, int n, double* soa)
{
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) soa[i + (size_t)n * k] = aos[3 * i + k];
}
