// The arithmetic of arap.hip that needs no GPU: what one cell (a vertex and its neighbours) of the as-rigid-as-possible energy computes.
// Plain functions in double, compiled for the device by arap.hip and for the host by tools/arap_host_check.cpp (the sanitizer run).
//   S = sum_j w_j e_q,j e_p,j^T  (e_q = q_i - q_j of the rest mesh, e_p = p_i - p_j of the deformed one)
//   S = U D V^T,  R = V diag(1, 1, det(V U^T)) U^T: the rotation with e_p ~ R e_q
//   E = sum_j w_j |e_p,j - R e_q,j|^2
#pragma once
#include "align_math.h"

namespace find {
namespace arap {

FIND_HD void zero9(double S[9]) {
	for (int i = 0; i < 9; ++i) S[i] = 0.;
}

// S += w e_q e_p^T (row-major: S[3 a + b] = sum w e_q[a] e_p[b])
FIND_HD void accumulate(double S[9], double w, const double eq[3], const double ep[3]) {
	for (int a = 0; a < 3; ++a) {
		const double we = w * eq[a];
		for (int b = 0; b < 3; ++b) S[3 * a + b] += we * ep[b];
	}
}

// R (row-major) from S, and the singular values d.  Returns false -- R = I -- for a cell without a unique rotation: d[0] = 0 (no
// neighbours, or all of them collapsed), d[1] <= RANK_TOL d[0] (collinear ones), or an S that is not finite.  Never NaN in R.
FIND_HD bool fit_rotation(const double S[9], double R[9], double d[3]) {
	double U[9], V[9];
	bool finite = true;
	for (int i = 0; i < 9; ++i) finite = finite && isfinite(S[i]);
	if (finite) find::align::svd3(S, U, d, V);
	if (!finite || !(d[0] > 0) || !(d[1] > find::align::RANK_TOL * d[0]) || !isfinite(d[0])) {
		for (int i = 0; i < 9; ++i) R[i] = i % 4 == 0 ? 1. : 0.;
		if (!finite) d[0] = d[1] = d[2] = 0.;
		return false;
	}
	const double e = find::align::det3(U) * find::align::det3(V) < 0 ? -1. : 1.;
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) R[3 * i + j] = V[3 * i] * U[3 * j] + V[3 * i + 1] * U[3 * j + 1] + e * V[3 * i + 2] * U[3 * j + 2];
	return true;
}

// R e
FIND_HD void rotate(const double R[9], const double e[3], double out[3]) {
	for (int a = 0; a < 3; ++a) out[a] = R[3 * a] * e[0] + R[3 * a + 1] * e[1] + R[3 * a + 2] * e[2];
}

// w |e_p - R e_q|^2: one neighbour's share of the cell energy
FIND_HD double cell_term(double w, const double R[9], const double eq[3], const double ep[3]) {
	double r[3];
	rotate(R, eq, r);
	const double dx = ep[0] - r[0], dy = ep[1] - r[1], dz = ep[2] - r[2];
	return w * (dx * dx + dy * dy + dz * dz);
}

// one neighbour's share of dE/dp_i (before the 2 / W): w [2 e_p - (R_i + R_j) e_q]
FIND_HD void grad_term(double w, const double Ri[9], const double Rj[9], const double eq[3], const double ep[3], double g[3]) {
	double a[3], b[3];
	rotate(Ri, eq, a);
	rotate(Rj, eq, b);
	for (int k = 0; k < 3; ++k) g[k] += w * (2. * ep[k] - (a[k] + b[k]));
}

}  // namespace arap
}  // namespace find
