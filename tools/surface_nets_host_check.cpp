// Host check of csrc/surface_nets_math.h, the arithmetic of surface_nets.hip that needs no GPU: the sides, the vertex of a cell and the backward
// term of a sample.  A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/surface_nets_host_check.cpp -o surface_nets_host_check
// The edge table is the twelve corner pairs that differ in one bit, in lexicographic order.  For every one of the 254 mixed corner masks, with
// random values: n is the number of crossing edges, every t lies in [0, 1], the vertex equals the mean of corner_a + t (corner_b - corner_a)
// written out independently, and float32 agrees with double.  value == iso, NaN and both infinities are outside, and a cell with such a corner
// has a finite vertex.  On a random 5 x 6 x 7 grid the backward terms (d L / d value of every sample, d L / d iso) of L = sum g . r equal
// central differences of the double forward.  Exit status 0 and "ok" when every check holds.
#include <stdio.h>
#include <random>
#include <vector>

#include "surface_nets_math.h"

using namespace find::surface_nets;

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

struct Field {
	int nx, ny, nz;
	std::vector<float> v;
	int64_t cells() const { return (int64_t)(nx - 1) * (ny - 1) * (nz - 1); }
	int64_t at(int i, int j, int k) const { return ((int64_t)i * ny + j) * nz + k; }
};

// The cell -> vertex map in flat cell order (sides from the float32 values), and the number of vertices.
static int64_t build_map(const Field& f, float iso, std::vector<int32_t>& map) {
	map.assign((size_t)f.cells(), -1);
	int64_t n = 0, c = 0;
	for (int i = 0; i + 1 < f.nx; ++i)
		for (int j = 0; j + 1 < f.ny; ++j)
			for (int k = 0; k + 1 < f.nz; ++k, ++c) {
				float v[8];
				for (int q = 0; q < 8; ++q) v[q] = f.v[(size_t)f.at(i + ((q >> 2) & 1), j + ((q >> 1) & 1), k + (q & 1))];
				const int m = corner_mask(v, iso);
				if (m != 0 && m != 255) map[(size_t)c] = (int32_t)n++;
			}
	return n;
}

// L = sum over the vertices of g . r in double, the samples shifted by dv at one index and iso by diso; the map stays.
static double forward(const Field& f, double iso, const std::vector<int32_t>& map, const std::vector<float>& r, int64_t shifted, double dv) {
	double L = 0.;
	int64_t c = 0;
	for (int i = 0; i + 1 < f.nx; ++i)
		for (int j = 0; j + 1 < f.ny; ++j)
			for (int k = 0; k + 1 < f.nz; ++k, ++c) {
				const int32_t m = map[(size_t)c];
				if (m < 0) continue;
				double v[8], p[3];
				for (int q = 0; q < 8; ++q) {
					const int64_t s = f.at(i + ((q >> 2) & 1), j + ((q >> 1) & 1), k + (q & 1));
					v[q] = (double)f.v[(size_t)s] + (s == shifted ? dv : 0.);
				}
				const int n = cell_vertex(v, iso, p);
				CHECK(n > 0, "cell %lld lost its vertex under a shift", (long long)c);
				L += (i + p[0]) * r[(size_t)(3 * m)] + (j + p[1]) * r[(size_t)(3 * m + 1)] + (k + p[2]) * r[(size_t)(3 * m + 2)];
			}
	return L;
}

int main() {
	{   // the edge table
		int e = 0;
		for (int a = 0; a < 8; ++a)
			for (int b = a + 1; b < 8; ++b) {
				const int x = a ^ b;
				if (x != 1 && x != 2 && x != 4) continue;
				CHECK(e < 12 && edge_a(e) == a && edge_b(e) == b, "edge %d is (%d, %d), want (%d, %d)", e, edge_a(e), edge_b(e), a, b);
				++e;
			}
		CHECK(e == 12, "%d edges", e);
	}
	{   // the sides
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		CHECK(is_inside(-1.f, 0.f) && !is_inside(0.f, 0.f) && !is_inside(1.f, 0.f), "value < iso, exactly");
		CHECK(is_inside(0.25f, 0.25f + 2.9802322e-8f) && !is_inside(0.25f, 0.25f), "one ulp below iso is inside");
		CHECK(!is_inside(nan, 0.f) && !is_inside(inf, 0.f) && !is_inside(-inf, 0.f), "non-finite samples are outside");
		CHECK(is_finite(3.4e38f) && !is_finite(inf) && !is_finite(-inf) && !is_finite(nan), "is_finite");
		CHECK(edge_t(-1.f, nan, 0.f) == 0.5f && edge_t(-inf, -1.f, 0.f) == 0.5f && edge_t(-1.f, inf, 0.f) == 0.f && edge_t(-1.f, 3.f, 0.f) == 0.25f, "edge_t");
	}
	std::mt19937_64 gen(11);
	std::uniform_real_distribution<float> u01(0.01f, 1.f);
	for (int mask = 1; mask < 255; ++mask) {   // every mixed mask
		for (int rep = 0; rep < 20; ++rep) {
			const float iso = 0.5f * (u01(gen) - 0.5f);
			float v[8], p[3];
			double vd[8], pd[3];
			for (int c = 0; c < 8; ++c) {
				v[c] = (mask >> c) & 1 ? iso - u01(gen) : iso + (rep == 7 && c == 0 ? 0.f : u01(gen));   // (rep 7: a corner exactly at iso is outside)
				if ((mask >> c) & 1 && !(v[c] < iso)) v[c] = iso - 0.5f;
				vd[c] = v[c];
			}
			CHECK(corner_mask(v, iso) == mask, "mask %d read back as %d", mask, corner_mask(v, iso));
			const int n = cell_vertex(v, iso, p), nd = cell_vertex(vd, (double)iso, pd);
			int want_n = 0;
			double sum[3] = {0, 0, 0};
			for (int a = 0; a < 8; ++a)
				for (int bit = 1; bit < 8; bit <<= 1) {
					const int b = a | bit;
					if (b == a || ((mask >> a) & 1) == ((mask >> b) & 1)) continue;
					const double t = ((double)iso - vd[a]) / (vd[b] - vd[a]);
					CHECK(t >= 0. && t <= 1., "mask %d edge (%d, %d): t = %g", mask, a, b, t);
					const int ca[3] = {(a >> 2) & 1, (a >> 1) & 1, a & 1}, cb[3] = {(b >> 2) & 1, (b >> 1) & 1, b & 1};
					for (int k = 0; k < 3; ++k) sum[k] += ca[k] + t * (cb[k] - ca[k]);
					++want_n;
				}
			CHECK(n == want_n && nd == want_n && n >= 3, "mask %d: n = %d / %d, want %d", mask, n, nd, want_n);
			for (int k = 0; k < 3; ++k) {
				CHECK(fabs(pd[k] - sum[k] / want_n) <= 1e-14, "mask %d: p[%d] = %.17g, want %.17g", mask, k, pd[k], sum[k] / want_n);
				CHECK(fabs((double)p[k] - pd[k]) <= 4e-6 && p[k] >= 0.f && p[k] <= 1.f, "mask %d: float p[%d] = %.9g, double %.17g", mask, k, p[k], pd[k]);
			}
		}
		{   // an inside corner next to a NaN, an infinity: the vertex stays finite
			float v[8], p[3];
			for (int c = 0; c < 8; ++c) v[c] = (mask >> c) & 1 ? -u01(gen) : (c % 3 == 0 ? std::numeric_limits<float>::quiet_NaN() : c % 3 == 1 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity());
			CHECK(corner_mask(v, 0.f) == mask, "mask %d with non-finite outside corners read back as %d", mask, corner_mask(v, 0.f));
			CHECK(cell_vertex(v, 0.f, p) >= 3 && is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]), "mask %d: a non-finite vertex", mask);
		}
	}
	{   // all inside, all outside: no vertex
		float v[8], p[3] = {7.f, 7.f, 7.f};
		for (int c = 0; c < 8; ++c) v[c] = 1.f;
		CHECK(cell_vertex(v, 0.f, p) == 0 && cell_vertex(v, 2.f, p) == 0 && p[0] == 7.f, "a cell on one side has no vertex");
	}
	{   // the backward terms against central differences of the double forward
		Field f{5, 6, 7, {}};
		std::uniform_real_distribution<float> u(-1.f, 1.f);
		const float iso = 0.1f;
		f.v.resize((size_t)(f.nx * f.ny * f.nz));
		for (auto& x : f.v) {
			do x = u(gen); while (fabsf(x - iso) < 0.02f);   // (no side changes under the shift)
		}
		std::vector<int32_t> map;
		const int64_t nv = build_map(f, iso, map);
		CHECK(nv > 50, "%lld vertices", (long long)nv);
		std::vector<float> r((size_t)(3 * nv));
		for (auto& x : r) x = u(gen);
		const double h = 1e-5;
		double d_iso = 0., worst = 0., scale = 0.;
		std::vector<double> got(f.v.size()), want(f.v.size());
		for (int i = 0; i < f.nx; ++i)
			for (int j = 0; j < f.ny; ++j)
				for (int k = 0; k < f.nz; ++k) {
					const int64_t s = f.at(i, j, k);
					got[(size_t)s] = sample_backward(f.v.data(), f.nx, f.ny, f.nz, i, j, k, iso, map.data(), r.data(), nv, &d_iso);
					want[(size_t)s] = (forward(f, iso, map, r, s, h) - forward(f, iso, map, r, s, -h)) / (2 * h);
					scale = fmax(scale, fabs(want[(size_t)s]));
					worst = fmax(worst, fabs(got[(size_t)s] - want[(size_t)s]));
				}
		printf("d L / d value: worst difference %.3e at scale %.3e\n", worst, scale);
		CHECK(scale > 0.1 && worst <= 1e-4 * scale, "d L / d value: worst %.3e, scale %.3e", worst, scale);
		const double want_iso = (forward(f, (double)iso + h, map, r, -1, 0.) - forward(f, (double)iso - h, map, r, -1, 0.)) / (2 * h);
		printf("d L / d iso: %.9g, central difference %.9g\n", d_iso, want_iso);
		CHECK(fabs(d_iso - want_iso) <= 1e-4 * fmax(1., fabs(want_iso)), "d L / d iso: %.9g, want %.9g", d_iso, want_iso);
		// vertices at or past the capacity have no gradient
		double none = 0.;
		for (int i = 0; i < f.nx; ++i)
			for (int j = 0; j < f.ny; ++j)
				for (int k = 0; k < f.nz; ++k) CHECK(sample_backward(f.v.data(), f.nx, f.ny, f.nz, i, j, k, iso, map.data(), r.data(), 0, &none) == 0.f, "capacity 0");
		CHECK(none == 0., "capacity 0: d iso %g", none);
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
