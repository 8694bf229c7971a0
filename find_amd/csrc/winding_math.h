// The arithmetic of winding.hip that needs no GPU: the solid angle one triangle subtends at a query point, and the order in which the solid
// angles of a mesh are added.  Plain functions, compiled for the device by winding.hip and for the host by tools/winding_host_check.cpp
// (the sanitizer run).
//   A = a - p, B = b - p, C = c - p                                   (float32, relative to the query)
//   det = A . (B x C),   den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|
//   Omega = 2 atan2(det, den)                                         (Van Oosterom & Strackee 1983),   w = sum Omega / 4 pi
// Exactly 0, never NaN: a corner at the query (a zero length), and det == 0 (the query in the face's plane, on the face or off it).
// det is formed with every product and sum rounded on its own, in the order written below: fused, B.y C.z - B.z C.y of a query in the plane
// is the rounding error of one product, not zero, and its sign -- half a turn of w for a query ON the face -- would depend on what the
// compiler contracts.  tests/inside_ref.py forms det in the same order, so the float32 restatement decides det == 0 and its sign as here.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FIND_WN_HD __host__ __device__ inline
#else
#define FIND_WN_HD inline
#endif

namespace find {
namespace winding {

constexpr int WN_SUB = 128;      // faces a wave sums in face order, from 0.0, into one double: a sub-chunk
constexpr int WN_CHUNK = 1024;   // faces per chunk: 8 sub-chunks, added in their order into the chunk's double (from 0.0)
constexpr double WN_INV_4PI = 0.079577471545947667884441881686257181;

FIND_WN_HD float det3(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
#pragma clang fp contract(off)
	const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
	return (ax * nx + ay * ny) + az * nz;
}

// The solid angle of the triangle (A, B, C), given relative to the query, in (-2 pi, 2 pi].
FIND_WN_HD float solid_angle(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
	const float la = sqrtf(fmaf(az, az, fmaf(ay, ay, ax * ax)));
	const float lb = sqrtf(fmaf(bz, bz, fmaf(by, by, bx * bx)));
	const float lc = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
	const float det = det3(ax, ay, az, bx, by, bz, cx, cy, cz);
	if (la == 0.f || lb == 0.f || lc == 0.f || det == 0.f) return 0.f;
	const float ab = fmaf(az, bz, fmaf(ay, by, ax * bx));
	const float bc = fmaf(bz, cz, fmaf(by, cy, bx * cx));
	const float ca = fmaf(cz, az, fmaf(cy, ay, cx * ax));
	const float den = fmaf(ca, lb, fmaf(bc, la, fmaf(ab, lc, la * lb * lc)));
	return 2.f * atan2f(det, den);
}

// One face of a mesh seen from p: the corners are subtracted in float32.
FIND_WN_HD float face_angle(const float p[3], const float a[3], const float b[3], const float c[3]) {
	return solid_angle(a[0] - p[0], a[1] - p[1], a[2] - p[2], b[0] - p[0], b[1] - p[1], b[2] - p[2], c[0] - p[0], c[1] - p[1], c[2] - p[2]);
}

FIND_WN_HD float to_winding(double sum_of_angles) { return (float)(sum_of_angles * WN_INV_4PI); }

// The sum's order, which is a function of the face count alone: faces in sub-chunks of WN_SUB, each summed in face order from 0.0; the
// sub-chunks of a chunk of WN_CHUNK faces added in their order from 0.0; the chunks added in their order from 0.0.  angle(j) is face j's
// solid angle (0 for a face that does not count).  The kernels follow this order whichever wave or workgroup forms a part; this is the
// plain loop the host check and a reader can hold them to.
template <typename Angle>
FIND_WN_HD double ordered_sum(int64_t n_faces, Angle angle) {
	double total = 0.;
	for (int64_t c0 = 0; c0 < n_faces; c0 += WN_CHUNK) {
		double chunk = 0.;
		for (int64_t s0 = c0; s0 < n_faces && s0 < c0 + WN_CHUNK; s0 += WN_SUB) {
			double sub = 0.;
			for (int64_t j = s0; j < n_faces && j < s0 + WN_SUB; ++j) sub += (double)angle(j);
			chunk += sub;
		}
		total += chunk;
	}
	return total;
}

}  // namespace winding
}  // namespace find
