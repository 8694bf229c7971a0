// The arithmetic of raycast.hip that needs no GPU: the watertight ray / triangle pair test (Woop, Benthin & Wald 2013, written without the
// axis permutation).  Plain functions, compiled for the device by raycast.hip and for the host by tools/raycast_host_check.cpp.
//   per ray, once (ray_frame):
//     kz = argmax |d| (the first of equals), kx, ky the other two axes in cyclic order, swapped if d[kz] < 0
//     e1 = axis(kx) - (d[kx] / d[kz]) axis(kz),   e2 = axis(ky) - (d[ky] / d[kz]) axis(kz),   dd = d . d
//   per corner p, by ONE function of (p - o, e1, e2) (project):
//     P = p - o,   x = (P0 e1_0 + P1 e1_1) + P2 e1_2,   y likewise with e2        -- a vertex has the same (x, y) bits in every face
//   per pair (pair_test), with (ax, ay), (bx, by), (cx, cy) the projected corners:
//     U = cx by - cy bx,   V = ax cy - ay cx,   W = bx ay - by ax,   det = (U + V) + W
//     inside: U, V, W all >= 0 or all <= 0 (a zero is inside: closed triangles) and det != 0
//     z = (P0 d0 + P1 d1) + P2 d2 per corner,   t = ((U za + V zb) + W zc) / (det dd)   in units of |d|;   barycentrics (U, V, W) / det
//     a hit: t_min < t <= t_max and t finite (an overflowed t is a miss: +inf means a miss and nothing else)
//   never a hit: a corner at the origin (P == 0, the rule of winding_math.h for a corner at the query); a ray with a non-finite component
//   or d == 0 (ray_frame says so).
// Every product and sum is rounded on its own, in the order written (contraction off): U = cx by - cy bx fused is the rounding error of one
// product where the two are equal, with a sign the compiler chooses.  Rounding is monotone, so the computed sign of cx by - cy bx is the
// sign of the exact difference or zero, never the opposite one; the two faces at an edge see the same two products, so a ray cannot pass
// between them.  That is why NO double-precision fallback is needed (Woop et al. fall back to double where an edge function is 0): a zero
// counts as inside here, and the only pairs refused are those with det == 0, edge-on triangles, which have no t.
// tests/rays_ref.py states the same operations in the same order in numpy; its float32 flavour is this file's twin, bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FIND_RC_HD __host__ __device__ inline
#else
#define FIND_RC_HD inline
#endif

namespace find {
namespace raycast {

constexpr int RC_SUB = 128;    // faces of a tile that one wave scans
constexpr int RC_TILE = 512;   // faces per tile: 4 waves x RC_SUB

struct Frame {
	float ox, oy, oz, dx, dy, dz;
	float e1x, e1y, e1z, e2x, e2y, e2z;
	float dd;
	bool live;   // false: a non-finite component or d == 0 -- the ray hits nothing
};

FIND_RC_HD bool finite3(float x, float y, float z) { return fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f; }

FIND_RC_HD Frame ray_frame(float ox, float oy, float oz, float dx, float dy, float dz) {
#pragma clang fp contract(off)
	Frame f;
	f.ox = ox; f.oy = oy; f.oz = oz; f.dx = dx; f.dy = dy; f.dz = dz;
	f.live = finite3(ox, oy, oz) && finite3(dx, dy, dz) && !(dx == 0.f && dy == 0.f && dz == 0.f);
	const float d[3] = {dx, dy, dz};
	int kz = 0;
	if (fabsf(d[1]) > fabsf(d[kz])) kz = 1;
	if (fabsf(d[2]) > fabsf(d[kz])) kz = 2;
	int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
	if (d[kz] < 0.f) { const int s = kx; kx = ky; ky = s; }
	float e1[3] = {0.f, 0.f, 0.f}, e2[3] = {0.f, 0.f, 0.f};
	e1[kx] = 1.f; e1[kz] = -(d[kx] / d[kz]);
	e2[ky] = 1.f; e2[kz] = -(d[ky] / d[kz]);
	f.e1x = e1[0]; f.e1y = e1[1]; f.e1z = e1[2];
	f.e2x = e2[0]; f.e2y = e2[1]; f.e2z = e2[2];
	f.dd = (dx * dx + dy * dy) + dz * dz;
	return f;
}

// (x, y) of the corner P = p - o in the ray's plane.
FIND_RC_HD void project(float Px, float Py, float Pz, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float& x, float& y) {
#pragma clang fp contract(off)
	x = (Px * e1x + Py * e1y) + Pz * e1z;
	y = (Px * e2x + Py * e2y) + Pz * e2z;
}

struct Hit {
	float t, u, v, w;   // u, v, w: the barycentrics of corners a, b, c
};

// The pair test on corners given relative to the origin.  True: a hit, h filled.
FIND_RC_HD bool pair_test(float Ax, float Ay, float Az, float Bx, float By, float Bz, float Cx, float Cy, float Cz, float e1x, float e1y, float e1z, float e2x,
						  float e2y, float e2z, float dx, float dy, float dz, float dd, float t_min, float t_max, Hit& h) {
#pragma clang fp contract(off)
	float ax, ay, bx, by, cx, cy;
	project(Ax, Ay, Az, e1x, e1y, e1z, e2x, e2y, e2z, ax, ay);
	project(Bx, By, Bz, e1x, e1y, e1z, e2x, e2y, e2z, bx, by);
	project(Cx, Cy, Cz, e1x, e1y, e1z, e2x, e2y, e2z, cx, cy);
	const float U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
	// (& and |, not && and ||: one branch for the device, which nearly every pair takes; a NaN is outside)
	const bool in = ((U >= 0.f) & (V >= 0.f) & (W >= 0.f)) | ((U <= 0.f) & (V <= 0.f) & (W <= 0.f));
	const float det = (U + V) + W;
	if (!(in & (det != 0.f))) return false;
	if (((Ax == 0.f) & (Ay == 0.f) & (Az == 0.f)) | ((Bx == 0.f) & (By == 0.f) & (Bz == 0.f)) | ((Cx == 0.f) & (Cy == 0.f) & (Cz == 0.f))) return false;
	const float za = (Ax * dx + Ay * dy) + Az * dz, zb = (Bx * dx + By * dy) + Bz * dz, zc = (Cx * dx + Cy * dy) + Cz * dz;
	const float t = ((U * za + V * zb) + W * zc) / (det * dd);
	if (!(t > t_min && t <= t_max && t <= 3.4028234663852886e38f)) return false;
	h.t = t; h.u = U / det; h.v = V / det; h.w = W / det;
	return true;
}

FIND_RC_HD bool ray_face(const Frame& f, const float a[3], const float b[3], const float c[3], float t_min, float t_max, Hit& h) {
	if (!f.live) return false;
	return pair_test(a[0] - f.ox, a[1] - f.oy, a[2] - f.oz, b[0] - f.ox, b[1] - f.oy, b[2] - f.oz, c[0] - f.ox, c[1] - f.oy, c[2] - f.oz, f.e1x, f.e1y, f.e1z,
					 f.e2x, f.e2y, f.e2z, f.dx, f.dy, f.dz, f.dd, t_min, t_max, h);
}

// The merge key: t > t_min >= 0, and positive floats order like their bits; among equal t the smallest face wins.
FIND_RC_HD unsigned long long hit_key(float t, int face) {
	union { float f; uint32_t u; } b;
	b.f = t;
	return ((unsigned long long)b.u << 32) | (unsigned long long)(uint32_t)face;
}
FIND_RC_HD float key_time(unsigned long long k) {
	union { float f; uint32_t u; } b;
	b.u = (uint32_t)(k >> 32);
	return b.f;
}

}  // namespace raycast
}  // namespace find
