// The arithmetic of align.hip that needs no GPU: the 3 x 3 SVD by one-sided Jacobi rotations, the Umeyama / Kabsch solve from weighted
// moments, and the digit step of the radix select.  Plain functions in double, compiled for the device by align.hip and for the host by
// tools/align_host_check.cpp (the sanitizer run of the solve).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FIND_HD __host__ __device__ inline
#else
#define FIND_HD inline
#endif

namespace find {
namespace align {

// the sums a pair contributes to, about the pivots px, py (the cloud's first points): x' = x - px, y' = y - py
enum { M_W = 0, M_X = 1, M_Y = 4, M_XY = 7, M_XX = 16, M_D2 = 17, M_CNT = 18, N_MOMENTS = 19 };
enum { STATUS_MAX_ITERATIONS = 1, STATUS_DEGENERATE = 2 };
// a covariance whose second singular value is at most this fraction of its first has rank < 2: what double rounding leaves of an exactly
// singular one is ~1e-16.  Points that are collinear only up to the rounding of their fp32 coordinates give ~1e-8: rank 2, badly
// conditioned, and solved as given.
constexpr double RANK_TOL = 1e-12;

// H (row-major 3 x 3) = U diag(d) V^T with d[0] >= d[1] >= d[2] >= 0, U and V orthogonal (their determinants may be -1).
// One-sided Jacobi (Hestenes): plane rotations from the right until the columns of H V are orthogonal; their norms are the singular
// values, the normalised columns U.  U's third column is the cross product of the first two with the sign of the rotated column (a
// column of norm ~0 has no direction of its own), so U is orthogonal whenever d[1] > 0.
FIND_HD void svd3(const double H[9], double U[9], double d[3], double V[9]) {
	double A[9], W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	for (int i = 0; i < 9; ++i) A[i] = H[i];
	for (int sweep = 0; sweep < 60; ++sweep) {
		bool rotated = false;
		for (int p = 0; p < 2; ++p)
			for (int q = p + 1; q < 3; ++q) {
				double a = 0, b = 0, c = 0;
				for (int i = 0; i < 3; ++i) { a += A[3 * i + p] * A[3 * i + p]; b += A[3 * i + q] * A[3 * i + q]; c += A[3 * i + p] * A[3 * i + q]; }
				if (c == 0 || fabs(c) <= 1e-15 * sqrt(a * b)) continue;
				rotated = true;
				const double zeta = (b - a) / (2 * c);
				const double t = (zeta >= 0 ? 1. : -1.) / (fabs(zeta) + sqrt(1 + zeta * zeta));
				const double cs = 1 / sqrt(1 + t * t), sn = cs * t;
				for (int i = 0; i < 3; ++i) {
					const double ap = A[3 * i + p], aq = A[3 * i + q];
					A[3 * i + p] = cs * ap - sn * aq; A[3 * i + q] = sn * ap + cs * aq;
					const double wp = W[3 * i + p], wq = W[3 * i + q];
					W[3 * i + p] = cs * wp - sn * wq; W[3 * i + q] = sn * wp + cs * wq;
				}
			}
		if (!rotated) break;
	}
	double nrm[3];
	int o[3] = {0, 1, 2};
	for (int j = 0; j < 3; ++j) nrm[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
	// descending, stable (three elements: three compare-exchanges)
	if (nrm[o[0]] < nrm[o[1]]) { const int s = o[0]; o[0] = o[1]; o[1] = s; }
	if (nrm[o[1]] < nrm[o[2]]) { const int s = o[1]; o[1] = o[2]; o[2] = s; }
	if (nrm[o[0]] < nrm[o[1]]) { const int s = o[0]; o[0] = o[1]; o[1] = s; }
	for (int j = 0; j < 3; ++j) {
		d[j] = nrm[o[j]];
		for (int i = 0; i < 3; ++i) {
			V[3 * i + j] = W[3 * i + o[j]];
			U[3 * i + j] = d[j] > 0 ? A[3 * i + o[j]] / d[j] : (i == j ? 1. : 0.);
		}
	}
	const double cx = U[3] * U[7] - U[6] * U[4], cy = U[6] * U[1] - U[0] * U[7], cz = U[0] * U[4] - U[3] * U[1];
	const double sg = (cx * A[o[2]] + cy * A[3 + o[2]] + cz * A[6 + o[2]]) < 0 ? -1. : 1.;
	U[2] = sg * cx; U[5] = sg * cy; U[8] = sg * cz;
}

FIND_HD double det3(const double M[9]) {
	return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama / Kabsch from the moments m[N_MOMENTS] about the pivots px, py: the R, t, s that minimise sum w |s (x @ R) + t - y|^2 (row
// vectors).  false -- and nothing written -- for fewer than 3 pairs of positive weight, a covariance of rank < 2, or with estimate_scale a
// cloud x without spread.
FIND_HD bool solve(const double* m, const double px[3], const double py[3], bool estimate_scale, bool allow_reflection, double R[9], double t[3],
				   double* s) {
	const double sw = m[M_W];
	if (!(m[M_CNT] >= 3) || !(sw > 0)) return false;
	double mx[3], my[3], H[9];
	for (int i = 0; i < 3; ++i) { mx[i] = m[M_X + i] / sw; my[i] = m[M_Y + i] / sw; }
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) H[3 * i + j] = m[M_XY + 3 * i + j] - m[M_X + i] * my[j];   // sum w (x - mu_x)(y - mu_y)^T
	double U[9], d[3], V[9];
	svd3(H, U, d, V);
	if (!(d[0] > 0) || !(d[1] > RANK_TOL * d[0]) || !isfinite(d[0])) return false;
	const double e = allow_reflection ? 1. : (det3(U) * det3(V) < 0 ? -1. : 1.);
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + e * U[3 * i + 2] * V[3 * j + 2];
	double sc = 1;
	if (estimate_scale) {
		const double var = m[M_XX] - (m[M_X] * mx[0] + m[M_X + 1] * mx[1] + m[M_X + 2] * mx[2]);   // sum w |x - mu_x|^2
		if (!(var > 0)) return false;
		sc = (d[0] + d[1] + e * d[2]) / var;
		if (!(sc > 0) || !isfinite(sc)) return false;
	}
	*s = sc;
	for (int j = 0; j < 3; ++j) {
		const double ax = px[0] + mx[0], ay = px[1] + mx[1], az = px[2] + mx[2];
		t[j] = (py[j] + my[j]) - sc * (ax * R[j] + ay * R[3 + j] + az * R[6 + j]);
	}
	return true;
}

// One digit of the radix select: among the values that share the digits found so far, hist[256] counts the next digit; the k-th smallest
// (1-based, k <= sum of hist) lies in the returned bin, and k becomes its rank inside that bin.
FIND_HD int select_bin(const int* hist, int* k) {
	int b = 0;
	while (b < 255 && *k > hist[b]) { *k -= hist[b]; ++b; }
	return b;
}

// k of the trim rule: m - floor(trim * m) pairs of the m valid ones are kept (0 <= trim < 1, so k >= 1 for m >= 1)
FIND_HD int keep_count(int m, double trim) {
	const int k = m - (int)floor(trim * (double)m);
	return k < 1 ? (m >= 1 ? 1 : 0) : (k > m ? m : k);
}

}  // namespace align
}  // namespace find
