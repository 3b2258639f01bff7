// eigh3_check.cpp -- icp::eigh3 (csrc/icp_host_math.cpp) across the double range, on the CPU.  Built together with that file and run
// by tests/test_batch_range_ref.py (with the address and undefined-behaviour sanitizers); prints one line per failed check, a
// summary, and exits 0 when all hold.  Three things:
//   * IN RANGE.  Matrices whose largest magnitude lies within [2^-400, 2^400], the zero matrix, and matrices with an entry that is
//     not finite: the bytes of a restatement of the statements without the range rule.
//   * BEYOND.  The same matrices times 2^m for |m| in {401, 600, 1000}: the eigenvectors' bytes are those of m = 0, the eigenvalues
//     are the m = 0 eigenvalues times 2^m as IEEE rounds the product (ldexp), the eigenvectors are orthonormal and A z = w z to
//     1e-13 of the largest magnitude.
//   * DEFICIENT.  v v^T and v v^T + u u^T from integer vectors at 2^+-1000: the first eigenvector is orthogonal to v (and u).
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../fast-point-cloud-registration-with-gpus_amd/csrc/icp_host_math.h"

static int g_failed = 0, g_checks = 0;

static bool check(bool ok, const char* what, ...)
{
    ++g_checks;
    if (ok) return true;
    char line[512];
    va_list ap;
    va_start(ap, what);
    vsnprintf(line, sizeof line, what, ap);
    va_end(ap);
    if (++g_failed <= 40) printf("FAIL %s\n", line);
    return false;
}

// icp::eigh3's statements as they were before the range rule
static void plain_eigh3(const double A[9], double w[3], double Z[9])
{
    double a[3][3], v[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            a[i][j] = j >= i ? A[i * 3 + j] : A[j * 3 + i];
            v[i][j] = i == j ? 1.0 : 0.0;
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
                const int r = 3 - p - q;
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
            if (a[ord[j]][ord[j]] < a[ord[i]][ord[i]]) {
                const int t = ord[i];
                ord[i] = ord[j];
                ord[j] = t;
            }
    for (int k = 0; k < 3; ++k) {
        w[k] = a[ord[k]][ord[k]];
        for (int i = 0; i < 3; ++i) Z[i * 3 + k] = v[i][ord[k]];
    }
}

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform()   // in (-1, 1), 21 bits: sums of a few products of these are exact
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((int64_t)(g_state >> 43) - (1 << 20)) / (double)(1 << 20);
}

// R R^T of a random 3 x 3 R: symmetric positive semi-definite, every entry exact (42 bits)
static void random_psd(double A[9])
{
    double R[9];
    for (double& r : R) r = uniform();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i * 3 + j] = (R[i * 3] * R[j * 3] + R[i * 3 + 1] * R[j * 3 + 1]) + R[i * 3 + 2] * R[j * 3 + 2];
}

static void times(const double A[9], int m, double S[9])
{
    for (int k = 0; k < 9; ++k) S[k] = std::ldexp(A[k], m);
}

static bool same(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

static void check_solution(const double S[9], const double w[3], const double Z[9], const char* tag, int i, int m)
{
    double amax = 0.0;
    for (int k = 0; k < 9; ++k) amax = std::fmax(amax, std::fabs(S[k]));
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            const double d = (Z[a] * Z[b] + Z[3 + a] * Z[3 + b]) + Z[6 + a] * Z[6 + b];
            check(std::fabs(d - (a == b ? 1.0 : 0.0)) < 1e-14, "%s %d 2^%d: columns %d, %d: dot %.17g", tag, i, m, a, b, d);
        }
    for (int k = 0; k < 3; ++k)
        for (int r = 0; r < 3; ++r) {
            const double az = (S[r * 3] * Z[k] + S[r * 3 + 1] * Z[3 + k]) + S[r * 3 + 2] * Z[6 + k];
            const double res = std::fabs(az - w[k] * Z[r * 3 + k]);
            check(res <= 1e-13 * amax, "%s %d 2^%d: A z - w z, column %d row %d: %.3g of the largest magnitude", tag, i, m, k, r, res / amax);
        }
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // IN RANGE and BEYOND
    const int inside[] = {-399, -200, 0, 200, 399}, beyond[] = {-1000, -600, -401, 401, 600, 1000};
    for (int i = 0; i < 200; ++i) {
        double A[9], S[9], w0[3], Z0[9], w[3], Z[9], pw[3], pZ[9];
        random_psd(A);
        double amax = 0.0;
        for (double a : A) amax = std::fmax(amax, std::fabs(a));
        int ex;
        std::frexp(amax, &ex);
        times(A, -ex, A);   // the largest magnitude in [0.5, 1)
        icp::eigh3(A, w0, Z0);
        check_solution(A, w0, Z0, "psd", i, 0);
        for (int m : inside) {
            times(A, m, S);
            icp::eigh3(S, w, Z);
            plain_eigh3(S, pw, pZ);
            check(same(w, pw, 3) && same(Z, pZ, 9), "psd %d 2^%d: not the bytes of the statements without the range rule", i, m);
        }
        for (int m : beyond) {
            times(A, m, S);
            icp::eigh3(S, w, Z);
            double want[3];
            for (int k = 0; k < 3; ++k) want[k] = std::ldexp(w0[k], m);
            check(same(Z, Z0, 9), "psd %d 2^%d: the eigenvectors are not those of 2^0", i, m);
            check(same(w, want, 3), "psd %d 2^%d: w %.17g %.17g %.17g, want %.17g %.17g %.17g", i, m, w[0], w[1], w[2], want[0], want[1], want[2]);
            check_solution(S, w, Z, "psd", i, m);
        }
    }
    {   // the zero matrix, and entries that are not finite: as before the rule, whatever the other entries
        double Zr[9] = {0}, w[3], Z[9], pw[3], pZ[9];
        icp::eigh3(Zr, w, Z);
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
        check(same(w, z3, 3) && same(Z, I, 9), "the zero matrix: not (0, 0, 0) and the identity");
        const double bad[] = {inf, -inf, nan};
        for (double b : bad)
            for (int at : {0, 1, 2, 4, 5, 8})
                for (int m : {-1000, 0, 1000}) {
                    double A[9], S[9];
                    random_psd(A);
                    times(A, m, S);
                    S[at] = b;
                    icp::eigh3(S, w, Z);
                    plain_eigh3(S, pw, pZ);
                    check(same(w, pw, 3) && same(Z, pZ, 9), "entry %d = %g at 2^%d: not the bytes of the statements without the range rule", at, b, m);
                }
    }
    // DEFICIENT
    const double v[4][3] = {{1, 2, 3}, {2, -1, 0}, {0, 0, 5}, {3, 1, -2}}, u[4][3] = {{2, 0, -1}, {1, 1, 4}, {1, -3, 0}, {-1, 2, 2}};
    for (int i = 0; i < 4; ++i)
        for (int rank = 1; rank <= 2; ++rank)
            for (int m : {-1000, 0, 1000}) {
                double A[9], S[9], w[3], Z[9];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) A[a * 3 + b] = v[i][a] * v[i][b] + (rank == 2 ? u[i][a] * u[i][b] : 0.0);
                times(A, m, S);
                icp::eigh3(S, w, Z);
                const double nv = std::sqrt(v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2]);
                const double nu = std::sqrt(u[i][0] * u[i][0] + u[i][1] * u[i][1] + u[i][2] * u[i][2]);
                const double dv = (Z[0] * v[i][0] + Z[3] * v[i][1] + Z[6] * v[i][2]) / nv, du = (Z[0] * u[i][0] + Z[3] * u[i][1] + Z[6] * u[i][2]) / nu;
                check(std::fabs(dv) < 1e-12, "rank %d matrix %d 2^%d: z0 . v = %.3g", rank, i, m, dv);
                if (rank == 2) check(std::fabs(du) < 1e-12, "rank 2 matrix %d 2^%d: z0 . u = %.3g", i, m, du);
                check_solution(S, w, Z, rank == 1 ? "rank 1" : "rank 2", i, m);
            }
    printf("eigh3_check: %d checks, %d failed\n", g_checks, g_failed);
    if (g_failed == 0) printf("eigh3_check passed\n");
    return g_failed == 0 ? 0 : 1;
}
