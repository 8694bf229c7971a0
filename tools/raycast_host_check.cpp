// Host check of csrc/raycast_math.h, the arithmetic of raycast.hip that needs no GPU: the watertight ray / triangle pair test with its rules.
// A stand-alone program for a sanitizer run on the CPU:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I find_amd/csrc tools/raycast_host_check.cpp -o raycast_host_check
// Without arguments: axis rays against the unit cube give exact t, the right face and the right barycentrics; a ray in a face's plane misses;
// a ray from a corner skips the faces at that corner; the interval is open below and closed above; dead rays hit nothing; rays from inside a
// cube aimed at its vertices, edge midpoints and random points all hit (watertightness); the key orders hits by t, then by face.  Exit
// status 0 and "ok" when every check holds.
// With `pairs IN OUT`: IN holds records of 17 float32 -- o, d, a, b, c (3 each), t_min, t_max --; for each, OUT gets 5 float32 -- 1 or 0
// (hit), t, u, v, w (0 for a miss): tests/test_rays_host.py compares them bit for bit with the float32 flavour of tests/rays_ref.py.
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>

#include "raycast_math.h"

using namespace find::raycast;

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

static const float CUBE_V[8][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}, {1, 1, 1}};   // vertex 4 x + 2 y + z
static const int CUBE_F[12][3] = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1}, {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};

// The closest hit on the cube, by the key: the face, or -1.
static int closest(const float o[3], const float d[3], float t_min, float t_max, Hit& best) {
	const Frame f = ray_frame(o[0], o[1], o[2], d[0], d[1], d[2]);
	unsigned long long key = ~0ull;
	for (int j = 0; j < 12; ++j) {
		Hit h;
		if (ray_face(f, CUBE_V[CUBE_F[j][0]], CUBE_V[CUBE_F[j][1]], CUBE_V[CUBE_F[j][2]], t_min, t_max, h) && hit_key(h.t, j) < key) {
			key = hit_key(h.t, j);
			best = h;
		}
	}
	if (key == ~0ull) return -1;
	CHECK(key_time(key) == best.t, "key_time does not return the hit's t");
	return (int)(unsigned)key;
}

static int run_pairs(const char* in, const char* out) {
	FILE* fi = fopen(in, "rb");
	if (!fi) { printf("cannot open %s\n", in); return 2; }
	std::vector<float> rec;
	float buf[17];
	while (fread(buf, sizeof(float), 17, fi) == 17) rec.insert(rec.end(), buf, buf + 17);
	fclose(fi);
	std::vector<float> res;
	for (size_t i = 0; i + 17 <= rec.size(); i += 17) {
		const float* r = &rec[i];
		Hit h = {0.f, 0.f, 0.f, 0.f};
		const bool hit = ray_face(ray_frame(r[0], r[1], r[2], r[3], r[4], r[5]), r + 6, r + 9, r + 12, r[15], r[16], h);
		const float o[5] = {hit ? 1.f : 0.f, hit ? h.t : 0.f, hit ? h.u : 0.f, hit ? h.v : 0.f, hit ? h.w : 0.f};
		res.insert(res.end(), o, o + 5);
	}
	FILE* fo = fopen(out, "wb");
	if (!fo) { printf("cannot open %s\n", out); return 2; }
	const bool ok = fwrite(res.data(), sizeof(float), res.size(), fo) == res.size();
	fclose(fo);
	printf("%zu pairs\n", res.size() / 5);
	return ok ? 0 : 2;
}

int main(int argc, char** argv) {
	if (argc == 4 && !strcmp(argv[1], "pairs")) return run_pairs(argv[2], argv[3]);
	const float inf = INFINITY;
	{   // axis rays: exact t, the right face, the right barycentrics
		const float o[3] = {0.25f, 0.5f, -1.f}, d[3] = {0, 0, 2};
		Hit h;
		const int j = closest(o, d, 0.f, inf, h);   // the side z = 0: faces 8 (0, 2, 6) and 9 (0, 6, 4); (0.25, 0.5) = 0.5 v0 + 0.25 v2 + 0.25 v6
		CHECK(j == 8 && h.t == 0.5f && h.u == 0.5f && h.v == 0.25f && h.w == 0.25f, "axis ray: face %d t %.9g bary %.9g %.9g %.9g", j, h.t, h.u, h.v, h.w);
		const float back[3] = {0, 0, -2};
		CHECK(closest(o, back, 0.f, inf, h) == -1, "a ray pointing away hits");
		// the interval: open below, closed above
		CHECK(closest(o, d, 0.5f, inf, h) == 11 && h.t == 1.f, "t_min = t of the first hit: the second hit expected, t %.9g", h.t);
		CHECK(closest(o, d, 0.f, 0.5f, h) == 8 && closest(o, d, 0.f, 0.49999997f, h) == -1, "t_max");
		// on the diagonal both faces of the side hold the point: the smallest face wins
		const float od[3] = {0.5f, 0.5f, -1.f};
		CHECK(closest(od, d, 0.f, inf, h) == 8 && h.t == 0.5f && h.v == 0.f, "diagonal: bary %.9g %.9g %.9g", h.u, h.v, h.w);
		// negative directions, each axis
		for (int k = 0; k < 3; ++k) {
			float p[3] = {0.3f, 0.6f, 0.7f}, q[3] = {0, 0, 0};
			p[k] = 3.f; q[k] = -1.f;
			const int jj = closest(p, q, 0.f, inf, h);
			CHECK(jj >= 0 && h.t == 2.f && fabsf(h.u + h.v + h.w - 1.f) <= 1e-6f, "axis %d: face %d t %.9g", k, jj, h.t);
		}
	}
	{   // in a face's plane: det == 0, a miss; from a corner: the faces at the corner never hit
		const float o[3] = {-1.f, 0.5f, 0.f}, d[3] = {1, 0, 0};
		Hit h;
		const Frame f = ray_frame(o[0], o[1], o[2], d[0], d[1], d[2]);
		CHECK(!ray_face(f, CUBE_V[0], CUBE_V[2], CUBE_V[6], 0.f, inf, h) && !ray_face(f, CUBE_V[0], CUBE_V[6], CUBE_V[4], 0.f, inf, h), "a ray in the plane hits");
		const float c[3] = {0, 0, 0}, dc[3] = {1, 1, 1};
		const int j = closest(c, dc, 0.f, inf, h);
		CHECK(j >= 0 && h.t == 1.f, "from a corner along the diagonal: face %d t %.9g", j, h.t);
		for (int jj : {CUBE_F[j][0], CUBE_F[j][1], CUBE_F[j][2]}) CHECK(jj != 0, "a face at the origin's corner was hit");
		const float graze[3] = {1, 0.5f, 0.25f};   // from the corner into the cube: only the far faces
		CHECK(closest(c, graze, 0.f, inf, h) == 2 && h.t == 1.f, "from a corner: t %.9g", h.t);
	}
	{   // dead rays
		const float o[3] = {0.5f, 0.5f, 0.5f};
		Hit h;
		const float zero[3] = {0, 0, 0}, nan[3] = {NAN, 1, 0}, big[3] = {inf, 0, 0};
		CHECK(closest(o, zero, 0.f, inf, h) == -1 && closest(o, nan, 0.f, inf, h) == -1 && closest(o, big, 0.f, inf, h) == -1, "a dead direction hits");
		const float on[3] = {NAN, 0.5f, 0.5f}, d[3] = {1, 0, 0};
		CHECK(closest(on, d, 0.f, inf, h) == -1 && closest(o, d, 0.f, inf, h) == 2, "a dead origin hits");
	}
	{   // watertightness: from inside the cube at its vertices, its edge midpoints and random points -- exactly one side is hit, at t > 0
		std::mt19937_64 g(7);
		std::uniform_real_distribution<float> u(0.05f, 0.95f), w(-1.f, 1.f);
		int aimed = 0;
		for (int t = 0; t < 20000; ++t) {
			const float o[3] = {u(g), u(g), u(g)};
			float target[3];
			if (t % 3 == 0) { for (int k = 0; k < 3; ++k) target[k] = CUBE_V[t % 8][k]; }
			else if (t % 3 == 1) { for (int k = 0; k < 3; ++k) target[k] = 0.5f * (CUBE_V[CUBE_F[t % 12][0]][k] + CUBE_V[CUBE_F[t % 12][1]][k]); }
			else { for (int k = 0; k < 3; ++k) target[k] = o[k] + w(g); }
			const float d[3] = {target[0] - o[0], target[1] - o[1], target[2] - o[2]};
			Hit h;
			const int j = closest(o, d, 0.f, inf, h);
			CHECK(j >= 0, "a ray from inside the cube escapes: o %.9g %.9g %.9g d %.9g %.9g %.9g", o[0], o[1], o[2], d[0], d[1], d[2]);
			if (j >= 0 && t % 3 != 2) { CHECK(fabsf(h.t - 1.f) <= 4e-6f, "aimed ray: t %.9g", h.t); ++aimed; }
			CHECK(j < 0 || (h.u >= 0.f && h.v >= 0.f && h.w >= 0.f && fabsf(h.u + h.v + h.w - 1.f) <= 1e-6f), "barycentrics %.9g %.9g %.9g", h.u, h.v, h.w);
		}
		CHECK(aimed > 13000, "%d aimed rays", aimed);
	}
	{   // keys
		CHECK(hit_key(0.5f, 7) < hit_key(0.50000006f, 0) && hit_key(0.5f, 3) < hit_key(0.5f, 4) && hit_key(1e-30f, 1 << 29) < ~0ull, "key order");
		CHECK(key_time(hit_key(0.3f, 11)) == 0.3f && (int)(unsigned)hit_key(0.3f, 11) == 11, "key round trip");
	}
	if (failures) {
		printf("%d checks failed\n", failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
