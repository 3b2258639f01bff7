// icp_host_math.cpp -- the tiny dense solves that north_star keeps on the host:
//   3x3 SVD -> R = U*Vt        replaces cusolverDnSgesvd + cublasSgemm (src/ICP_point_to_point.cu:369-381)
//                              and LAPACKE_dgesvd + dgemm (src/ICP_CPU.c:240-246)
//   6x6 Cholesky (upper)       replaces cusolverDnSpotrf/Spotrs (src/ICP_point_to_plane.cu:576-581)
//   symmetric 3x3 eigen-solve  replaces LAPACKE_ssyev (src/ICP_point_to_plane.cu:429-438)
// Everything is fp64.  No device code here; the CPU test-suite calls these through the C ABI.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/icp_mi355x.h"
#include "icp_host_math.h"

namespace icp {

// One-sided Jacobi run on the ROWS of a working copy W = A: row rotations (accumulated in Ut) drive
// the rows mutually orthogonal, W = Ut^T... i.e. J * A = diag(s) * Vt with J orthogonal.  Then
// A = J^T * diag(s) * Vt and the orthogonal polar factor is R = J^T * Vt_normalised = U * Vt.
// Row orientation keeps the rotation accumulation on the U side.
void svd3_rows(const double A[9], double U[9], double S[3], double Vt[9])
{
    double W[3][3], J[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            W[i][j] = A[i * 3 + j];
            J[i][j] = i == j ? 1.0 : 0.0;
        }
    const double eps = 2.220446049250313e-16;
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool changed = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double app = 0, aqq = 0, apq = 0;
                for (int k = 0; k < 3; ++k) {
                    app += W[p][k] * W[p][k];
                    aqq += W[q][k] * W[q][k];
                    apq += W[p][k] * W[q][k];
                }
                if (apq == 0.0 || std::fabs(apq) <= eps * std::sqrt(app * aqq)) continue;
                changed = true;
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = std::copysign(1.0, tau) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double wp = W[p][k], wq = W[q][k];
                    W[p][k] = c * wp - s * wq;
                    W[q][k] = s * wp + c * wq;
                    const double jp = J[p][k], jq = J[q][k];
                    J[p][k] = c * jp - s * jq;
                    J[q][k] = s * jp + c * jq;
                }
            }
        if (!changed) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i) nrm[i] = std::sqrt(W[i][0] * W[i][0] + W[i][1] * W[i][1] + W[i][2] * W[i][2]);
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (nrm[ord[j]] > nrm[ord[i]]) std::swap(ord[i], ord[j]);
    double v[3][3];
    bool have[3] = {false, false, false};
    const double tiny = 1e-14 * (nrm[ord[0]] > 0 ? nrm[ord[0]] : 1.0);
    for (int k = 0; k < 3; ++k) {
        const int r = ord[k];
        S[k] = nrm[r];
        if (nrm[r] > tiny) {
            for (int c = 0; c < 3; ++c) v[k][c] = W[r][c] / nrm[r];
            have[k] = true;
        }
    }
    auto cross = [](const double* a, const double* b, double* c) {
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
    };
    if (!have[0]) { v[0][0] = 1; v[0][1] = 0; v[0][2] = 0; }
    if (!have[1]) {
        int mi = 0;
        for (int c = 1; c < 3; ++c) if (std::fabs(v[0][c]) < std::fabs(v[0][mi])) mi = c;
        double e[3] = {0, 0, 0};
        e[mi] = 1;
        cross(v[0], e, v[1]);
        const double nn = std::sqrt(v[1][0] * v[1][0] + v[1][1] * v[1][1] + v[1][2] * v[1][2]);
        for (int c = 0; c < 3; ++c) v[1][c] /= nn;
    }
    if (!have[2]) cross(v[0], v[1], v[2]);
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) {
            Vt[k * 3 + c] = v[k][c];
            U[c * 3 + k] = J[ord[k]][c];  // U = J^T with columns permuted like the singular values
        }
}

int solve_point_to_point(const double* mom, double* R, double* t)
{
    const double n = mom[ICP_MOM_CNT];
    if (!(n > 0)) return ICP_ERR_INVALID;
    double pb[3], qb[3];
    for (int a = 0; a < 3; ++a) {
        pb[a] = mom[ICP_MOM_SP + a] / n;
        qb[a] = mom[ICP_MOM_SQ + a] / n;
    }
    double N[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) N[a * 3 + b] = mom[ICP_MOM_SQP + a * 3 + b] - n * qb[a] * pb[b];
    double U[9], S[3], Vt[9];
    svd3_rows(N, U, S, Vt);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += U[a * 3 + k] * Vt[k * 3 + b];
            R[a * 3 + b] = s;  // no det(R) check: src/ICP_CPU.c:246 has none
        }
    for (int a = 0; a < 3; ++a) t[a] = qb[a] - (R[a * 3 + 0] * pb[0] + R[a * 3 + 1] * pb[1] + R[a * 3 + 2] * pb[2]);
    return ICP_OK;
}

// solve_point_to_point with the determinant fix (Kabsch / Umeyama): the singular values come out in descending order, so the last
// column of U belongs to the smallest; flipping it when det(U Vt) < 0 gives the rotation nearest to the cross-covariance.
int solve_rigid(const double* mom, double* R, double* t)
{
    const double n = mom[ICP_MOM_CNT];
    if (!(n > 0)) return ICP_ERR_INVALID;
    double pb[3], qb[3];
    for (int a = 0; a < 3; ++a) {
        pb[a] = mom[ICP_MOM_SP + a] / n;
        qb[a] = mom[ICP_MOM_SQ + a] / n;
    }
    double N[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) N[a * 3 + b] = mom[ICP_MOM_SQP + a * 3 + b] - n * qb[a] * pb[b];
    double U[9], S[3], Vt[9];
    svd3_rows(N, U, S, Vt);
    for (int pass = 0; pass < 2; ++pass) {
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += U[a * 3 + k] * Vt[k * 3 + b];
                R[a * 3 + b] = s;
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(det < 0)) break;
        for (int a = 0; a < 3; ++a) U[a * 3 + 2] = -U[a * 3 + 2];
    }
    for (int a = 0; a < 3; ++a) t[a] = qb[a] - (R[a * 3 + 0] * pb[0] + R[a * 3 + 1] * pb[1] + R[a * 3 + 2] * pb[2]);
    return ICP_OK;
}

// Upper Cholesky C = Ut*U of the 6x6 SPD matrix given by its upper triangle (row-major packed, 21), then Ut y = b and U x = y.
static int cholesky6_solve(const double* mom, double x[6])
{
    double Uc[6][6];
    {
        int o = ICP_MOM_C;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) Uc[a][c] = mom[o++];
    }
    for (int k = 0; k < 6; ++k) {
        double d = Uc[k][k];
        for (int r = 0; r < k; ++r) d -= Uc[r][k] * Uc[r][k];
        if (!(d > 0.0)) return ICP_ERR_SINGULAR;  // potrf's info > 0
        d = std::sqrt(d);
        Uc[k][k] = d;
        for (int c = k + 1; c < 6; ++c) {
            double s = Uc[k][c];
            for (int r = 0; r < k; ++r) s -= Uc[r][k] * Uc[r][c];
            Uc[k][c] = s / d;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {  // Ut y = b
        double s = mom[ICP_MOM_B + i];
        for (int r = 0; r < i; ++r) s -= Uc[r][i] * y[r];
        y[i] = s / Uc[i][i];
    }
    for (int i = 5; i >= 0; --i) {  // U x = y
        double s = y[i];
        for (int c = i + 1; c < 6; ++c) s -= Uc[i][c] * x[c];
        x[i] = s / Uc[i][i];
    }
    return ICP_OK;
}

int solve_point_to_plane(const double* mom, double* R, double* t, double* x6)
{
    double x[6];
    if (int rc = cholesky6_solve(mom, x)) return rc;
    if (x6) std::memcpy(x6, x, sizeof x);
    const double cx = std::cos(x[0]), cy = std::cos(x[1]), cz = std::cos(x[2]);
    const double sx = std::sin(x[0]), sy = std::sin(x[1]), sz = std::sin(x[2]);
    // R = Rz(gamma) Ry(beta) Rx(alpha), row-major (src/CUDA/CPU_ICP_point_to-plane.cpp:381-383)
    R[0] = cy * cz; R[1] = cz * sx * sy - cx * sz; R[2] = cx * cz * sy + sx * sz;
    R[3] = cy * sz; R[4] = cx * cz + sx * sy * sz; R[5] = cx * sy * sz - cz * sx;
    R[6] = -sy;     R[7] = cy * sx;                R[8] = cx * cy;
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
    return ICP_OK;
}

// The symmetric metric's step (include/icp_mi355x.h, "the symmetric metric"): x = (a, tt) from the plane solve's Cholesky, a the axis
// times tan(theta), tt the translation over cos(theta); Ra the rotation by theta = atan(|a|) about a, without trigonometry and
// without a division by |a|; the motion p -> Ra (Ra p + t'), t' = c tt, as R = Ra Ra and t = Ra t'.
int solve_symmetric(const double* mom, double* R, double* t, double* x6)
{
    double x[6];
    if (int rc = cholesky6_solve(mom, x)) return rc;
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(x[i])) return ICP_ERR_SINGULAR;
    const double a[3] = {x[0], x[1], x[2]};
    const double l2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    if (!std::isfinite(l2)) return ICP_ERR_SINGULAR;
    if (x6) std::memcpy(x6, x, sizeof x);
    const double c = 1.0 / std::sqrt(1.0 + l2), k = (c * c) / (1.0 + c);
    const double E[3][3] = {{1.0, -a[2], a[1]}, {a[2], 1.0, -a[0]}, {-a[1], a[0], 1.0}};   // I + [a]x
    double Ra[3][3], tp[3];
    for (int r = 0; r < 3; ++r) {
        for (int s = 0; s < 3; ++s) Ra[r][s] = c * E[r][s] + k * (a[r] * a[s]);
        tp[r] = c * x[3 + r];
    }
    for (int r = 0; r < 3; ++r) {
        for (int s = 0; s < 3; ++s) R[r * 3 + s] = (Ra[r][0] * Ra[0][s] + Ra[r][1] * Ra[1][s]) + Ra[r][2] * Ra[2][s];
        t[r] = (Ra[r][0] * tp[0] + Ra[r][1] * tp[1]) + Ra[r][2] * tp[2];
    }
    return ICP_OK;
}

// cyclic Jacobi on the full symmetric matrix built from the upper triangle.  The stop test squares the entries, and the squares of
// a matrix beyond 2^+-400 leave the range (off = inf or 0 ends the sweeps at once: the identity would come out whatever the matrix):
// with amax the largest magnitude of the six entries, amax > 2^400 multiplies them by 2^-600 and 0 < amax < 2^-400 by 2^+600 -- an
// exact power of two, which changes no rotation -- and the eigenvalues are multiplied back once their order is fixed.  Every other
// matrix, and every matrix with an entry that is not finite, goes through as it is, bit for bit.
void eigh3(const double A[9], double w[3], double Z[9])
{
    double a[3][3], v[3][3];
    double amax = 0.0;
    bool finite = true;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            a[i][j] = j >= i ? A[i * 3 + j] : A[j * 3 + i];
            v[i][j] = i == j ? 1.0 : 0.0;
            amax = std::fmax(amax, std::fabs(a[i][j]));   // (fmax drops a NaN)
            finite = finite && std::isfinite(a[i][j]);
        }
    double unscale = 1.0;
    if (finite && (amax > 0x1p+400 || (amax < 0x1p-400 && amax > 0.0))) {
        const double sc = amax > 1.0 ? 0x1p-600 : 0x1p+600;
        unscale = amax > 1.0 ? 0x1p+600 : 0x1p-600;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) a[i][j] *= sc;
    }
    for (int sweep = 0; sweep < 64; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
        const double dia = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
        if (off <= 1e-34 * dia || off == 0.0) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                const double app = a[p][p], aqq = a[q][q];
                a[p][p] = app - t * apq;
                a[q][q] = aqq + t * apq;
                a[p][q] = a[q][p] = 0.0;
                const int r = 3 - p - q;  // the remaining index
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = a[p][r] = c * arp - s * arq;
                a[r][q] = a[q][r] = s * arp + c * arq;
                for (int k = 0; k < 3; ++k) {
                    const double vp = v[k][p], vq = v[k][q];
                    v[k][p] = c * vp - s * vq;
                    v[k][q] = s * vp + c * vq;
                }
            }
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (a[ord[j]][ord[j]] < a[ord[i]][ord[i]]) std::swap(ord[i], ord[j]);
    for (int k = 0; k < 3; ++k) {
        w[k] = a[ord[k]][ord[k]] * unscale;
        for (int i = 0; i < 3; ++i) Z[i * 3 + k] = v[i][ord[k]];
    }
}

// ---- plane segmentation (icp_batch_segment_plane): every statement is the header's, one IEEE double operation each (this unit is
// compiled with contraction off)
namespace {
// all three components negated iff the component of largest magnitude is negative; the lowest index decides among equal magnitudes
void plane_sign(double n[3])
{
    int k = 0;
    for (int a = 1; a < 3; ++a)
        if (std::fabs(n[a]) > std::fabs(n[k])) k = a;
    if (n[k] < 0.0)
        for (int a = 0; a < 3; ++a) n[a] = -n[a];
}
}  // namespace

bool plane_from_points(const double* a, const double* b, const double* c, double plane4[4])
{
    plane4[0] = plane4[1] = plane4[2] = plane4[3] = 0.0;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double l = std::sqrt((wx * wx + wy * wy) + wz * wz);
    if (!(l > 0.0 && std::isfinite(l))) return false;   // (NaN fails both)
    double n[3] = {wx / l, wy / l, wz / l};
    plane_sign(n);
    plane4[0] = n[0];
    plane4[1] = n[1];
    plane4[2] = n[2];
    plane4[3] = -((n[0] * a[0] + n[1] * a[1]) + n[2] * a[2]);
    return true;
}

bool plane_from_moments(const double centroid[3], const double cov6[6], double plane4[4])
{
    plane4[0] = plane4[1] = plane4[2] = plane4[3] = 0.0;
    const double A[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4], cov6[2], cov6[4], cov6[5]};
    double w[3], Z[9];
    eigh3(A, w, Z);
    double n[3] = {Z[0], Z[3], Z[6]};   // column 0: the smallest eigenvalue's, not renormalised
    if (!(std::isfinite(n[0]) && std::isfinite(n[1]) && std::isfinite(n[2]))) return false;
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return false;
    plane_sign(n);
    plane4[0] = n[0];
    plane4[1] = n[1];
    plane4[2] = n[2];
    plane4[3] = -((n[0] * centroid[0] + n[1] * centroid[1]) + n[2] * centroid[2]);
    return true;
}

bool plane_axis_ok(const double plane4[4], const double axis[3], double min_cos)
{
    if (axis[0] == 0.0 && axis[1] == 0.0 && axis[2] == 0.0) return true;
    const double la = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    const double hx = axis[0] / la, hy = axis[1] / la, hz = axis[2] / la;
    return std::fabs((plane4[0] * hx + plane4[1] * hy) + plane4[2] * hz) >= min_cos;
}

int shard_range(int64_t n, int rank, int world, int64_t* begin, int64_t* count)
{
    if (n < 0 || world <= 0 || rank < 0 || rank >= world) return ICP_ERR_INVALID;
    const int64_t base = n / world, rem = n % world;
    *begin = rank * base + (rank < rem ? rank : rem);
    *count = base + (rank < rem ? 1 : 0);
    return ICP_OK;
}

}  // namespace icp

extern "C" {
int icp_solve_point_to_point(const double* mom, double* R9, double* t3)
{
    if (!mom || !R9 || !t3) return ICP_ERR_INVALID;
    return icp::solve_point_to_point(mom, R9, t3);
}
int icp_solve_rigid(const double* mom, double* R9, double* t3)
{
    if (!mom || !R9 || !t3) return ICP_ERR_INVALID;
    return icp::solve_rigid(mom, R9, t3);
}
int icp_solve_point_to_plane(const double* mom, double* R9, double* t3, double* x6)
{
    if (!mom || !R9 || !t3) return ICP_ERR_INVALID;
    return icp::solve_point_to_plane(mom, R9, t3, x6);
}
int icp_solve_symmetric(const double* mom, double* R9, double* t3, double* x6)
{
    if (!mom || !R9 || !t3) return ICP_ERR_INVALID;
    return icp::solve_symmetric(mom, R9, t3, x6);
}
int icp_shard_range(int64_t n, int rank, int world, int64_t* begin, int64_t* count)
{
    if (!begin || !count) return ICP_ERR_INVALID;
    return icp::shard_range(n, rank, world, begin, count);
}
int icp_plane_from_points(const double* abc9, double* plane4)
{
    if (!abc9 || !plane4) return ICP_ERR_INVALID;
    return icp::plane_from_points(abc9, abc9 + 3, abc9 + 6, plane4) ? ICP_OK : ICP_ERR_EMPTY;
}
int icp_plane_from_moments(const double* centroid3, const double* cov6, double* plane4)
{
    if (!centroid3 || !cov6 || !plane4) return ICP_ERR_INVALID;
    return icp::plane_from_moments(centroid3, cov6, plane4) ? ICP_OK : ICP_ERR_EMPTY;
}
int icp_eigh3(const double* A9, double* w3, double* Z9)
{
    if (!A9 || !w3 || !Z9) return ICP_ERR_INVALID;
    icp::eigh3(A9, w3, Z9);
    return ICP_OK;
}
}
