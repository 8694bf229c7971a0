// Host check of csrc/align_math.h, the arithmetic of align.hip that needs no GPU: the Jacobi SVD, the Umeyama solve and the radix select.
// A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/align_host_check.cpp -o align_host_check
// Exit status 0 and "ok" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

#include "align_math.h"

using namespace find::align;

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

static void matmul(const double* A, const double* B, double* C, bool tb) {
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double s = 0;
			for (int k = 0; k < 3; ++k) s += A[3 * i + k] * (tb ? B[3 * j + k] : B[3 * k + j]);
			C[3 * i + j] = s;
		}
}

static double ortho_error(const double* M) {
	double G[9], e = 0;
	double Mt[9];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) Mt[3 * i + j] = M[3 * j + i];
	matmul(Mt, M, G, false);
	for (int i = 0; i < 9; ++i) e = std::max(e, fabs(G[i] - (i % 4 == 0 ? 1. : 0.)));
	return e;
}

static void check_svd(const double* H, double scale, const char* what) {
	double U[9], d[3], V[9], UD[9], R[9];
	svd3(H, U, d, V);
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) UD[3 * i + j] = U[3 * i + j] * d[j];
	matmul(UD, V, R, true);
	double e = 0;
	for (int i = 0; i < 9; ++i) e = std::max(e, fabs(R[i] - H[i]));
	CHECK(e <= 1e-13 * scale, "%s: |U D V^T - H| = %g", what, e);
	CHECK(d[0] >= d[1] && d[1] >= d[2] && d[2] >= 0, "%s: singular values %g %g %g", what, d[0], d[1], d[2]);
	CHECK(ortho_error(V) <= 1e-13, "%s: V^T V - I = %g", what, ortho_error(V));
	if (d[1] > 1e-12 * d[0]) CHECK(ortho_error(U) <= 1e-12, "%s: U^T U - I = %g", what, ortho_error(U));
}

static void rotation(std::mt19937_64& g, double angle, double* R) {
	std::normal_distribution<double> nd;
	double a[3] = {nd(g), nd(g), nd(g)};
	const double n = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	for (double& v : a) v /= n;
	const double c = cos(angle), s = sin(angle), K[9] = {0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0};
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) R[3 * i + j] = (i == j ? c : 0.) + s * K[3 * i + j] + (1 - c) * a[i] * a[j];
}

// the moments of align.hip's moments_kernel, in plain order
static void moments(const std::vector<double>& x, const std::vector<double>& y, const std::vector<double>& w, double* m, double* px, double* py) {
	memset(m, 0, sizeof(double) * N_MOMENTS);
	for (int k = 0; k < 3; ++k) { px[k] = x[k]; py[k] = y[k]; }
	for (size_t i = 0; i < w.size(); ++i) {
		if (!(w[i] > 0)) continue;
		double dx[3], dy[3];
		for (int k = 0; k < 3; ++k) { dx[k] = x[3 * i + k] - px[k]; dy[k] = y[3 * i + k] - py[k]; }
		m[M_W] += w[i]; m[M_CNT] += 1;
		m[M_XX] += w[i] * (dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
		for (int k = 0; k < 3; ++k) {
			m[M_X + k] += w[i] * dx[k]; m[M_Y + k] += w[i] * dy[k];
			for (int l = 0; l < 3; ++l) m[M_XY + 3 * k + l] += w[i] * dx[k] * dy[l];
		}
	}
}

int main() {
	std::mt19937_64 g(7);
	std::uniform_real_distribution<double> ud(-1, 1);
	// ---- SVD: random, rank 2, rank 1, zero, diagonal, huge and tiny
	for (int trial = 0; trial < 2000; ++trial) {
		double H[9];
		for (double& v : H) v = ud(g);
		check_svd(H, 3, "random");
		for (int i = 0; i < 3; ++i) H[3 * i + 2] = 0.5 * H[3 * i] - 2 * H[3 * i + 1];
		check_svd(H, 8, "rank 2");
		for (int i = 0; i < 3; ++i) H[3 * i + 1] = 3 * H[3 * i];
		check_svd(H, 30, "rank 1");
		for (double& v : H) v = ud(g) * 1e-30;
		check_svd(H, 3e-30, "tiny");
		for (double& v : H) v = ud(g) * 1e30;
		check_svd(H, 3e30, "huge");
	}
	const double zero[9] = {0}, diag[9] = {1, 0, 0, 0, 3, 0, 0, 0, 2};
	check_svd(zero, 1, "zero");
	check_svd(diag, 3, "diagonal");
	// ---- solve: known transforms, with weights, far from the origin, reflections, degenerate clouds
	for (int trial = 0; trial < 500; ++trial) {
		const int P = 3 + trial % 40;
		const bool scale = trial & 1, mirror = (trial & 6) == 6;
		double R0[9], t0[3] = {10 * ud(g), 10 * ud(g), 10 * ud(g)}, s0 = scale ? 0.5 + (ud(g) + 1) : 1.;
		rotation(g, 3 * ud(g), R0);
		if (mirror)
			for (int i = 0; i < 3; ++i) R0[3 * i] = -R0[3 * i];
		const double far = trial % 5 == 0 ? 1e4 : 0.;
		std::vector<double> x(3 * P), y(3 * P), w(P);
		for (int i = 0; i < P; ++i) {
			x[3 * i] = far + 0.25 * ud(g); x[3 * i + 1] = far + 0.10 * ud(g); x[3 * i + 2] = 0.08 * ud(g);
			for (int j = 0; j < 3; ++j) y[3 * i + j] = s0 * (x[3 * i] * R0[j] + x[3 * i + 1] * R0[3 + j] + x[3 * i + 2] * R0[6 + j]) + t0[j];
			w[i] = trial % 3 == 0 && i >= 4 && i % 4 == 0 ? 0. : 0.5 + (ud(g) + 1);
		}
		double m[N_MOMENTS], px[3], py[3], R[9], t[3], s;
		moments(x, y, w, m, px, py);
		const bool ok = solve(m, px, py, scale, mirror, R, t, &s);
		CHECK(ok, "trial %d: solve refused", trial);
		if (!ok) continue;
		double e = fabs(s - s0);
		for (int i = 0; i < 9; ++i) e = std::max(e, fabs(R[i] - R0[i]));
		CHECK(e <= 1e-8, "trial %d: R, s off by %g", trial, e);
		for (int j = 0; j < 3; ++j) CHECK(fabs(t[j] - t0[j]) <= 1e-7 * (1 + far), "trial %d: t[%d] off by %g", trial, j, fabs(t[j] - t0[j]));
		if (!mirror) CHECK(fabs(det3(R) - 1) <= 1e-12 && ortho_error(R) <= 1e-12, "trial %d: det %g", trial, det3(R));
		// a mirrored target without allow_reflection: still a proper rotation
		if (mirror) {
			CHECK(solve(m, px, py, scale, false, R, t, &s), "trial %d: refused", trial);
			CHECK(fabs(det3(R) - 1) <= 1e-12 && ortho_error(R) <= 1e-12, "trial %d: det %g (reflection not allowed)", trial, det3(R));
		}
	}
	{
		double m[N_MOMENTS], px[3], py[3], R[9], t[3], s;
		std::vector<double> x = {0, 0, 0, 1, 2, 3}, y = {1, 1, 1, 2, 2, 2}, w = {1, 1};
		moments(x, y, w, m, px, py);
		CHECK(!solve(m, px, py, true, false, R, t, &s), "two pairs accepted");
		x = {0, 0, 0, 1, 2, 3, 2, 4, 6, 3, 6, 9}; y = {0, 0, 0, 0, 1, 0, 0, 2, 0, 0, 3, 0}; w = {1, 1, 1, 1};
		moments(x, y, w, m, px, py);
		CHECK(!solve(m, px, py, false, false, R, t, &s), "collinear pairs accepted");
		x = {1, 1, 1, 1, 1, 1, 1, 1, 1}; y = {0, 0, 0, 0, 1, 0, 5, 2, 0}; w = {1, 1, 1};
		moments(x, y, w, m, px, py);
		CHECK(!solve(m, px, py, true, false, R, t, &s), "coincident points accepted");
		w = {1, 0, 1};
		moments(x, y, w, m, px, py);
		CHECK(!solve(m, px, py, false, false, R, t, &s), "two pairs of positive weight accepted");
	}
	// ---- radix select against std::nth_element, ties included
	for (int trial = 0; trial < 300; ++trial) {
		const int mcount = 1 + (int)(g() % 700);
		std::vector<float> d(mcount);
		for (float& v : d) v = trial % 3 == 0 ? (float)(g() % 5) * 0.25f : (float)((ud(g) + 1) * (trial % 2 ? 1e-6 : 1e3));
		const double trims[] = {0., 0.2, 0.25, 0.5, (mcount - 1 + 0.5) / mcount};
		for (double trim : trims) {
			int k = keep_count(mcount, trim);
			CHECK(k >= 1 && k <= mcount && k == mcount - (int)floor(trim * mcount), "keep_count(%d, %g) = %d", mcount, trim, k);
			const int k0 = k;
			uint32_t prefix = 0;
			for (int shift = 24; shift >= 0; shift -= 8) {
				int hist[256] = {0};
				const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
				for (float v : d) {
					uint32_t b;
					memcpy(&b, &v, 4);
					if ((b & mask) == prefix) ++hist[(b >> shift) & 255u];
				}
				prefix |= (uint32_t)select_bin(hist, &k) << shift;
			}
			float tau;
			memcpy(&tau, &prefix, 4);
			std::vector<float> sorted(d);
			std::sort(sorted.begin(), sorted.end());
			CHECK(tau == sorted[k0 - 1], "select: m %d trim %g: %g, sorted[k - 1] = %g", mcount, trim, tau, sorted[k0 - 1]);
		}
	}
	CHECK(keep_count(0, 0.5) == 0, "keep_count(0)");
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
