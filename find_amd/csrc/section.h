// The section rule of include/find_hip.h (find_plane_sections_*, find_section_hull_*), shared by measure.hip and girth.hip so that both cut a
// face in the same bits: s = fmaf(nz, z, fmaf(ny, y, nx * x)) - d per vertex, "above" iff s >= 0; on a crossing edge lo -> hi the point
// p = fmaf(t, hi - lo, lo), t = s_lo / (s_lo - s_hi).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace find {
namespace measure {

struct Mesh {
	const float* verts;     // (N, V, 3)
	const int32_t* faces;   // (fb, F, 3)
	const float* planes;    // (pb, P, 4)
	int64_t fb, pb;
	int V, F, P;
};

struct V3 {
	float x, y, z;
};

__device__ __forceinline__ V3 load3(const float* __restrict__ p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ float signed_distance(const float* __restrict__ pl, const V3& v) {
	return fmaf(pl[2], v.z, fmaf(pl[1], v.y, pl[0] * v.x)) - pl[3];
}
// the point where the edge lo -> hi (s_lo < 0 <= s_hi) meets the plane, and t
__device__ __forceinline__ V3 crossing(const V3& lo, const V3& hi, float s_lo, float s_hi, float& t) {
	t = s_lo / (s_lo - s_hi);
	return V3{fmaf(t, hi.x - lo.x, lo.x), fmaf(t, hi.y - lo.y, lo.y), fmaf(t, hi.z - lo.z, lo.z)};
}

// the face of this thread: its three vertices; false for a face past the end, with an index outside [0, V) or with a repeated vertex
__device__ __forceinline__ bool load_face(const Mesh& m, int mesh, int f, V3 v[3]) {
	if (f >= m.F) return false;
	const int32_t* fm = m.faces + ((int64_t)(m.fb == 1 ? 0 : mesh) * m.F + f) * 3;
	const int i0 = fm[0], i1 = fm[1], i2 = fm[2];
	if (!((unsigned)i0 < (unsigned)m.V && (unsigned)i1 < (unsigned)m.V && (unsigned)i2 < (unsigned)m.V) || i0 == i1 || i1 == i2 || i0 == i2) return false;
	const float* vp = m.verts + (int64_t)mesh * m.V * 3;
	v[0] = load3(vp + 3 * (int64_t)i0); v[1] = load3(vp + 3 * (int64_t)i1); v[2] = load3(vp + 3 * (int64_t)i2);
	return true;
}

// A crossing face seen from the vertex that is alone on its side: L that vertex (corner k), A and B the corners k + 1 and k + 2.
struct Cut {
	V3 L, A, B;
	float sL, sA, sB;
	int k;
	bool up;   // L is the one above
};

__device__ __forceinline__ bool cut_of(const float* __restrict__ pl, const V3 v[3], Cut& c) {
	const float s0 = signed_distance(pl, v[0]), s1 = signed_distance(pl, v[1]), s2 = signed_distance(pl, v[2]);
	const bool a0 = s0 >= 0.f, a1 = s1 >= 0.f, a2 = s2 >= 0.f;
	if (a0 == a1 && a1 == a2) return false;
	if (a0 == a1) {
		c.k = 2; c.L = v[2]; c.A = v[0]; c.B = v[1]; c.sL = s2; c.sA = s0; c.sB = s1; c.up = a2;
	} else if (a0 == a2) {
		c.k = 1; c.L = v[1]; c.A = v[2]; c.B = v[0]; c.sL = s1; c.sA = s2; c.sB = s0; c.up = a1;
	} else {
		c.k = 0; c.L = v[0]; c.A = v[1]; c.B = v[2]; c.sL = s0; c.sA = s1; c.sB = s2; c.up = a0;
	}
	return true;
}

}  // namespace measure
}  // namespace find
