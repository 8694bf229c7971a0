// Host check of csrc/arap_math.h, the per-cell arithmetic of arap.hip that needs no GPU: the sums S, the fitted rotation with its
// reflection and degeneracy rules, and the cell energy.  A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/arap_host_check.cpp -o arap_host_check
// Over random, mirrored, planar, identity, collapsed, collinear and empty cells: R^T R = I, det R = +1, the energy of R against the closed
// form sum w (|e_p|^2 + |e_q|^2) - 2 (d1 + d2 +- d3) (minus when det S < 0) and against a search over rotations (none may do better).
// Exit status 0 and "ok" when every check holds.
#include <stdio.h>
#include <algorithm>
#include <random>
#include <vector>

#include "arap_math.h"

using namespace find::arap;

static int failures = 0;
#define CHECK(cond, ...)                                  \
	do {                                                  \
		if (!(cond)) {                                    \
			++failures;                                   \
			printf("FAILED %s:%d: ", __FILE__, __LINE__); \
			printf(__VA_ARGS__);                          \
			printf("\n");                                 \
		}                                                 \
	} while (0)

struct CellData {
	std::vector<double> w, eq, ep;   // (k), (k, 3), (k, 3)
	size_t size() const { return w.size(); }
};

static void axis_angle(const double ax[3], double angle, double* R) {
	const double n = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
	const double x = ax[0] / n, y = ax[1] / n, z = ax[2] / n, c = cos(angle), s = sin(angle), t = 1 - c;
	const double M[9] = {t * x * x + c, t * x * y - s * z, t * x * z + s * y, t * x * y + s * z, t * y * y + c, t * y * z - s * x,
						 t * x * z - s * y, t * y * z + s * x, t * z * z + c};
	for (int i = 0; i < 9; ++i) R[i] = M[i];
}

static void random_rotation(std::mt19937_64& g, double max_angle, double* R) {
	std::normal_distribution<double> nd;
	std::uniform_real_distribution<double> ud(0., max_angle);
	double ax[3] = {nd(g), nd(g), nd(g)};
	if (ax[0] == 0 && ax[1] == 0 && ax[2] == 0) ax[0] = 1;
	axis_angle(ax, ud(g), R);
}

static void matmul(const double* A, const double* B, double* C) {
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

static double ortho_error(const double* M) {
	double e = 0;
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double s = 0;
			for (int k = 0; k < 3; ++k) s += M[3 * k + i] * M[3 * k + j];
			e = std::max(e, fabs(s - (i == j ? 1. : 0.)));
		}
	return e;
}

static double energy(const CellData& c, const double* R) {
	double e = 0;
	for (size_t k = 0; k < c.size(); ++k) e += cell_term(c.w[k], R, &c.eq[3 * k], &c.ep[3 * k]);
	return e;
}

static CellData make(std::mt19937_64& g, int valence, const double* R0, bool mirror, double noise, bool planar) {
	std::normal_distribution<double> nd;
	std::uniform_real_distribution<double> ud(0., 1.);
	CellData c;
	for (int k = 0; k < valence; ++k) {
		double eq[3] = {0.01 * nd(g), 0.01 * nd(g), planar ? 0. : 0.01 * nd(g)}, ep[3];
		rotate(R0, eq, ep);
		if (mirror) ep[2] = -ep[2];
		for (int t = 0; t < 3; ++t) ep[t] += noise * nd(g);
		c.w.push_back(k % 5 == 4 ? 0. : ud(g) * 2);   // (clamped cotangent weights: some are exactly 0)
		c.eq.insert(c.eq.end(), eq, eq + 3);
		c.ep.insert(c.ep.end(), ep, ep + 3);
	}
	return c;
}

// everything a well-posed cell must satisfy; returns the fitted rotation in R
static void check_cell(const CellData& c, std::mt19937_64& g, const char* what, double* R) {
	double S[9], d[3];
	zero9(S);
	double norm = 0;
	for (size_t k = 0; k < c.size(); ++k) {
		accumulate(S, c.w[k], &c.eq[3 * k], &c.ep[3 * k]);
		for (int t = 0; t < 3; ++t) norm += c.w[k] * (c.eq[3 * k + t] * c.eq[3 * k + t] + c.ep[3 * k + t] * c.ep[3 * k + t]);
	}
	const bool ok = fit_rotation(S, R, d);
	CHECK(ok, "%s: reported degenerate (d = %g %g %g)", what, d[0], d[1], d[2]);
	CHECK(ortho_error(R) <= 1e-12, "%s: R^T R - I = %g", what, ortho_error(R));
	CHECK(fabs(find::align::det3(R) - 1.) <= 1e-12, "%s: det R = %.17g", what, find::align::det3(R));
	const double e = energy(c, R), sign = find::align::det3(S) < 0 ? -1. : 1.;
	const double closed = norm - 2. * (d[0] + d[1] + sign * d[2]);
	CHECK(fabs(e - closed) <= 1e-12 * norm, "%s: energy %.17g, closed form %.17g (scale %g)", what, e, closed, norm);
	// no rotation does better: anywhere, and near R
	for (int trial = 0; trial < 400; ++trial) {
		double Q[9], T[9];
		if (trial < 200) {
			random_rotation(g, M_PI, Q);
		} else {
			random_rotation(g, trial < 300 ? 1e-2 : 1e-5, T);
			matmul(T, R, Q);
		}
		const double other = energy(c, Q);
		CHECK(other >= e - 1e-12 * norm, "%s: a rotation with energy %.17g < %.17g", what, other, e);
	}
}

static void check_degenerate(const CellData& c, const char* what) {
	double S[9], R[9], d[3];
	zero9(S);
	for (size_t k = 0; k < c.size(); ++k) accumulate(S, c.w[k], &c.eq[3 * k], &c.ep[3 * k]);
	CHECK(!fit_rotation(S, R, d), "%s: not reported degenerate (d = %g %g %g)", what, d[0], d[1], d[2]);
	for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1. : 0.), "%s: R[%d] = %g, identity expected", what, i, R[i]);
	const double e = energy(c, R);
	CHECK(std::isfinite(e) && e >= 0, "%s: energy %g", what, e);
}

int main() {
	std::mt19937_64 g(7);
	double R0[9], R[9];
	char what[64];
	for (int trial = 0; trial < 200; ++trial) {
		const int valence = 3 + trial % 10;
		random_rotation(g, M_PI, R0);
		snprintf(what, sizeof what, "random %d", trial);
		const CellData c = make(g, valence, R0, false, trial % 2 ? 5e-3 : 5e-4, false);
		check_cell(c, g, what, R);
		snprintf(what, sizeof what, "mirrored %d", trial);
		check_cell(make(g, valence, R0, true, 5e-4, false), g, what, R);
		snprintf(what, sizeof what, "planar %d", trial);   // (rest edges in a plane: S of rank 2, the rotation still unique)
		check_cell(make(g, valence, R0, false, 5e-4, true), g, what, R);
		// without noise the rotation is recovered and the energy vanishes
		snprintf(what, sizeof what, "rigid %d", trial);
		const CellData r = make(g, valence + 1, R0, false, 0., false);
		check_cell(r, g, what, R);
		for (int i = 0; i < 9; ++i) CHECK(fabs(R[i] - R0[i]) <= 1e-10, "%s: R[%d] = %.17g, %.17g expected", what, i, R[i], R0[i]);
		CHECK(energy(r, R) <= 1e-24, "%s: energy %g", what, energy(r, R));
	}
	{   // identity: e_p bitwise e_q
		const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		CellData c = make(g, 6, I, false, 0., false);
		c.ep = c.eq;
		check_cell(c, g, "identity", R);
		for (int i = 0; i < 9; ++i) CHECK(fabs(R[i] - I[i]) <= 1e-14, "identity: R[%d] = %.17g", i, R[i]);
		CHECK(energy(c, R) <= 1e-30, "identity: energy %g", energy(c, R));
	}
	{   // collapsed: every deformed edge is zero
		CellData c = make(g, 6, R0, false, 0., false);
		std::fill(c.ep.begin(), c.ep.end(), 0.);
		check_degenerate(c, "collapsed");
		// collinear: every deformed edge on the x axis (exactly rank 1)
		c = make(g, 7, R0, false, 1e-3, false);
		for (size_t k = 0; k < c.size(); ++k) c.ep[3 * k + 1] = c.ep[3 * k + 2] = 0.;
		check_degenerate(c, "collinear deformed");
		// ... or every rest edge
		c = make(g, 7, R0, false, 1e-3, false);
		for (size_t k = 0; k < c.size(); ++k) c.eq[3 * k + 1] = c.eq[3 * k + 2] = 0.;
		check_degenerate(c, "collinear rest");
		// all weights zero, and no neighbours at all
		c = make(g, 5, R0, false, 1e-3, false);
		std::fill(c.w.begin(), c.w.end(), 0.);
		check_degenerate(c, "weightless");
		check_degenerate(CellData(), "empty");
		// not finite: reported, never NaN in R
		c = make(g, 5, R0, false, 1e-3, false);
		c.ep[4] = NAN;
		double S[9], d[3];
		zero9(S);
		for (size_t k = 0; k < c.size(); ++k) accumulate(S, c.w[k], &c.eq[3 * k], &c.ep[3 * k]);
		CHECK(!fit_rotation(S, R, d), "nan: not reported degenerate");
		for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1. : 0.), "nan: R[%d] = %g", i, R[i]);
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
