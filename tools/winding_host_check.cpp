// Host check of csrc/winding_math.h, the arithmetic of winding.hip that needs no GPU: the solid angle of a triangle with its zero rules, and
// the fixed order of the sum.  A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/winding_host_check.cpp -o winding_host_check
// The octant triangle seen from the origin subtends 4 pi / 8; a cube gives 1 inside, 0 outside and -1 with its faces flipped; a corner at
// the query, a query in the face's plane (on the face and off it) and a face collapsed to a point give exactly 0, never NaN; the ordered sum
// equals the plain one to rounding at face counts on each side of a sub-chunk and of a chunk.  Exit status 0 and "ok" when every check holds.
#include <stdio.h>
#include <random>
#include <vector>

#include "winding_math.h"

using namespace find::winding;

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

struct Mesh {
	std::vector<float> v;   // (V, 3)
	std::vector<int> f;     // (F, 3)
	int64_t n_faces() const { return (int64_t)f.size() / 3; }
};

static float winding(const Mesh& m, const float p[3]) {
	return to_winding(ordered_sum(m.n_faces(), [&](int64_t j) { return face_angle(p, &m.v[3 * m.f[3 * j]], &m.v[3 * m.f[3 * j + 1]], &m.v[3 * m.f[3 * j + 2]]); }));
}

static Mesh cube(bool flipped) {
	Mesh m;
	for (int x = 0; x < 2; ++x)
		for (int y = 0; y < 2; ++y)
			for (int z = 0; z < 2; ++z) { m.v.push_back((float)x); m.v.push_back((float)y); m.v.push_back((float)z); }
	const int F[12][3] = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1}, {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};
	for (auto& t : F) { m.f.push_back(t[0]); m.f.push_back(flipped ? t[2] : t[1]); m.f.push_back(flipped ? t[1] : t[2]); }
	return m;
}

int main() {
	{   // the octant
		const float o[3] = {0, 0, 0}, a[3] = {1, 0, 0}, b[3] = {0, 1, 0}, c[3] = {0, 0, 1};
		const float om = face_angle(o, a, b, c);
		CHECK(fabs(fabs(om) - M_PI / 2) <= 1e-6, "octant: %.9g", om);
		CHECK(fabs(fabs(to_winding(om)) - 0.125) <= 1e-7, "octant: w = %.9g", to_winding(om));
		CHECK(face_angle(o, a, c, b) == -om, "octant flipped: %.9g", face_angle(o, a, c, b));
	}
	{   // a cube: random points inside and outside, both orientations
		const Mesh out = cube(false), in = cube(true);
		std::mt19937_64 g(3);
		std::uniform_real_distribution<float> u(-1.f, 2.f);
		int n_in = 0;
		for (int t = 0; t < 4000; ++t) {
			const float p[3] = {u(g), u(g), u(g)};
			float edge = 1.f;   // distance to the nearest side's plane
			for (int k = 0; k < 3; ++k) edge = fminf(edge, fminf(fabsf(p[k]), fabsf(p[k] - 1.f)));
			if (edge < 1e-3f) continue;
			const bool inside = p[0] > 0 && p[0] < 1 && p[1] > 0 && p[1] < 1 && p[2] > 0 && p[2] < 1;
			n_in += inside;
			const float w = winding(out, p), wf = winding(in, p);
			CHECK(fabsf(w - (inside ? 1.f : 0.f)) <= 2e-5f, "cube: w(%g, %g, %g) = %.9g", p[0], p[1], p[2], w);
			CHECK(fabsf(wf + (inside ? 1.f : 0.f)) <= 2e-5f, "flipped cube: w(%g, %g, %g) = %.9g", p[0], p[1], p[2], wf);
		}
		CHECK(n_in > 50, "cube: %d points inside", n_in);
		// at a corner of the cube the six faces that meet there do not count, and the other six are seen edge-on or from inside: 1 / 8
		const float corner[3] = {0, 0, 0};
		CHECK(fabsf(winding(out, corner) - 0.125f) <= 1e-6f, "cube corner: %.9g", winding(out, corner));
	}
	{   // the zero rules: exactly 0, never NaN
		const float a[3] = {0.25f, 0.5f, 0.125f}, b[3] = {1.25f, 0.5f, 0.125f}, c[3] = {0.25f, 2.5f, 0.125f};
		CHECK(face_angle(a, a, b, c) == 0.f && face_angle(b, a, b, c) == 0.f && face_angle(c, a, b, c) == 0.f, "a corner at the query");
		const float on[3] = {0.5f, 0.75f, 0.125f}, off[3] = {-3.f, 7.f, 0.125f}, edge[3] = {0.75f, 0.5f, 0.125f};
		CHECK(face_angle(on, a, b, c) == 0.f, "in the plane, on the face: %.9g", face_angle(on, a, b, c));
		CHECK(face_angle(off, a, b, c) == 0.f, "in the plane, off the face: %.9g", face_angle(off, a, b, c));
		CHECK(face_angle(edge, a, b, c) == 0.f, "on an edge: %.9g", face_angle(edge, a, b, c));
		const float p[3] = {0.3f, 0.1f, 0.9f}, mid[3] = {0.75f, 0.5f, 0.125f};
		CHECK(fabsf(face_angle(p, a, b, mid)) <= 1e-6f, "a face collapsed to a line: %.9g", face_angle(p, a, b, mid));   // (det is rounding, den > 0)
		CHECK(face_angle(p, a, a, a) == 0.f, "a face collapsed to a point: %.9g", face_angle(p, a, a, a));
		// just off the face the angle is half the sphere, with the side's sign
		const float above[3] = {0.5f, 0.75f, 0.125f + 1e-6f}, below[3] = {0.5f, 0.75f, 0.125f - 1e-6f};
		CHECK(fabs(face_angle(above, a, b, c) + 2 * M_PI) <= 1e-4 && fabs(face_angle(below, a, b, c) - 2 * M_PI) <= 1e-4, "beside the face: %.9g, %.9g",
			  face_angle(above, a, b, c), face_angle(below, a, b, c));
		std::mt19937_64 g(5);
		std::uniform_real_distribution<float> u(-1.f, 1.f);
		for (int t = 0; t < 100000; ++t) {
			float q[3], x[3], y[3], z[3];
			for (int k = 0; k < 3; ++k) { q[k] = u(g); x[k] = t % 3 ? u(g) : q[k] + 1e-7f * u(g); y[k] = u(g); z[k] = t % 5 ? u(g) : y[k]; }
			const float om = face_angle(q, x, y, z);
			CHECK(std::isfinite(om) && fabsf(om) <= 6.2831855f, "random %d: %.9g", t, om);
		}
	}
	{   // the sum's order: the same value as a plain sum to rounding, at counts on each side of a sub-chunk and of a chunk
		std::mt19937_64 g(9);
		std::uniform_real_distribution<float> u(-6.f, 6.f);
		for (int64_t n : {0, 1, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 5000}) {
			std::vector<float> om((size_t)n);
			for (auto& x : om) x = u(g);
			long double plain = 0, mag = 0;
			for (float x : om) { plain += x; mag += fabsl(x); }
			const double s = ordered_sum(n, [&](int64_t j) { return om[(size_t)j]; });
			CHECK(fabsl(s - plain) <= 1e-15L * mag, "ordered_sum(%lld) = %.17g, plain %.17Lg", (long long)n, s, plain);
			CHECK(s == ordered_sum(n, [&](int64_t j) { return om[(size_t)j]; }), "ordered_sum(%lld) does not repeat", (long long)n);
			if (n == 0) CHECK(s == 0. && to_winding(s) == 0.f, "no faces: %g", s);
		}
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
