// icp_host_math.h -- host-side dense solves of the ICP loop (see icp_host_math.cpp)
#pragma once
#include <stdint.h>

namespace icp {
void svd3_rows(const double A[9], double U[9], double S[3], double Vt[9]);
int solve_point_to_point(const double* mom, double* R9, double* t3);
int solve_rigid(const double* mom, double* R, double* t);   // ... with the determinant fix: R is always a rotation
int solve_point_to_plane(const double* mom, double* R9, double* t3, double* x6);
int solve_symmetric(const double* mom, double* R9, double* t3, double* x6);   // the same Cholesky, the step split into two half rotations
void eigh3(const double A[9], double w[3], double Z[9]);
int shard_range(int64_t n, int rank, int world, int64_t* begin, int64_t* count);
// plane segmentation's host statements (the rule: include/icp_mi355x.h, icp_batch_segment_plane).  false: the hypothesis is invalid
// (plane4: four zeros)
bool plane_from_points(const double* a, const double* b, const double* c, double plane4[4]);
bool plane_from_moments(const double centroid[3], const double cov6[6], double plane4[4]);
// the axis constraint: true where axis == (0, 0, 0) or fabs(n . ahat) >= min_cos
bool plane_axis_ok(const double plane4[4], const double axis[3], double min_cos);
}  // namespace icp
