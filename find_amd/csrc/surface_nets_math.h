// The arithmetic of surface_nets.hip that needs no GPU: which side a sample lies on, the vertex of one grid cell and the backward term of one
// sample.  Plain functions, compiled for the device by surface_nets.hip and for the host by tools/surface_nets_host_check.cpp (the sanitizer
// run), which also instantiates the vertex in double for its central differences.
//   a sample is INSIDE iff value < iso and the value is finite (an exact comparison: value == iso, NaN and both infinities are outside)
//   corner c = 4 di + 2 dj + dk of cell (i, j, k); the 12 edges (a, b), a < b, join corners that differ in one bit, in lexicographic order
//   on a crossing edge  t = (iso - v_a) / (v_b - v_a)  (0.5 if that is not finite),  p = corner_a + t (corner_b - corner_a)
//   the cell's vertex, relative to the cell's first corner:  (sum of p in edge order) / n,  n the number of crossing edges
#pragma once
#include <math.h>
#include <stdint.h>
#include <limits>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FIND_SN_HD __host__ __device__ inline
#else
#define FIND_SN_HD inline
#endif

namespace find {
namespace surface_nets {

constexpr int SN_BLOCK = 256;   // cells (emit of vertices) and samples (counting, emit of faces) per workgroup: FIND_SURFACE_NETS_BLOCK
// corner a and corner b of edge e in nibble e: (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6) (5,7) (6,7)
constexpr uint64_t SN_EDGE_A = 0x654432211000ull;
constexpr uint64_t SN_EDGE_B = 0x776576353421ull;

FIND_SN_HD int edge_a(int e) { return (int)((SN_EDGE_A >> (4 * e)) & 15); }
FIND_SN_HD int edge_b(int e) { return (int)((SN_EDGE_B >> (4 * e)) & 15); }

template <typename T>
FIND_SN_HD bool is_finite(T v) { return (v < 0 ? -v : v) <= std::numeric_limits<T>::max(); }   // (false for NaN)
template <typename T>
FIND_SN_HD bool is_inside(T v, T iso) { return v < iso && is_finite(v); }

// bit c set: corner c is inside
template <typename T>
FIND_SN_HD int corner_mask(const T v[8], T iso) {
	int m = 0;
	for (int c = 0; c < 8; ++c) m |= (int)is_inside(v[c], iso) << c;
	return m;
}

// bit e set: edge e crosses
FIND_SN_HD int crossing_edges(int mask) {
	int x = 0;
	for (int e = 0; e < 12; ++e) x |= (((mask >> edge_a(e)) ^ (mask >> edge_b(e))) & 1) << e;
	return x;
}

FIND_SN_HD int popcount12(int x) {
	int n = 0;
	for (int e = 0; e < 12; ++e) n += (x >> e) & 1;
	return n;
}

template <typename T>
FIND_SN_HD T edge_t(T va, T vb, T iso) {
	const T t = (iso - va) / (vb - va);
	return is_finite(t) ? t : (T)0.5;
}

// The vertex of a cell with the corner values v: p = (sum over the crossing edges, in edge order) / n.  Returns n: 0 for a cell that is not
// active (p is then left alone).
template <typename T>
FIND_SN_HD int cell_vertex(const T v[8], T iso, T p[3]) {
	const int mask = corner_mask(v, iso);
	if (mask == 0 || mask == 255) return 0;
	const int cross = crossing_edges(mask);
	T s[3] = {0, 0, 0};
	int n = 0;
	for (int e = 0; e < 12; ++e) {
		if (!((cross >> e) & 1)) continue;
		const int a = edge_a(e), b = edge_b(e);
		const int axis = b - a == 4 ? 0 : b - a == 2 ? 1 : 2;
		const T t = edge_t(v[a], v[b], iso);
		// corner a has a 0 along the edge's axis, so the point is corner a with t in that place
		s[0] += axis == 0 ? t : (T)((a >> 2) & 1);
		s[1] += axis == 1 ? t : (T)((a >> 1) & 1);
		s[2] += axis == 2 ? t : (T)(a & 1);
		++n;
	}
	p[0] = s[0] / (T)n; p[1] = s[1] / (T)n; p[2] = s[2] / (T)n;
	return n;
}

// The backward term of sample (i, j, k) of one mesh: d L / d value, a gather over the <= 8 cells that have the sample as a corner and the
// <= 3 edges of each that end there.  values: the mesh's (nx, ny, nz) samples; cellmap: its (nx-1, ny-1, nz-1) cell -> vertex map (-1: no
// vertex); grad_g (vcap, 3): d L / d g.  With d = v_b - v_a:  dt/dv_a = (iso - v_b) / d^2,  dt/dv_b = -(iso - v_a) / d^2,  dt/diso = 1 / d;
// n is a constant, and an edge whose t fell back to 0.5 has no gradient.  An edge's d L / d iso is counted at its corner a and ADDED to
// *d_iso.  Every term is formed in float32 and added in double, cells in the order di, dj, dk = 0, 1 and edges in the order x, y, z.
FIND_SN_HD float sample_backward(const float* values, int nx, int ny, int nz, int i, int j, int k, float iso, const int32_t* cellmap,
								 const float* grad_g, int64_t vcap, double* d_iso) {
	double grad = 0., giso = 0.;
	for (int corner = 0; corner < 8; ++corner) {
		const int ci = i - ((corner >> 2) & 1), cj = j - ((corner >> 1) & 1), ck = k - (corner & 1);
		if (ci < 0 || cj < 0 || ck < 0 || ci > nx - 2 || cj > ny - 2 || ck > nz - 2) continue;
		const int64_t m = cellmap[((int64_t)ci * (ny - 1) + cj) * (nz - 1) + ck];
		if (m < 0 || m >= vcap) continue;
		float v[8];
		for (int c = 0; c < 8; ++c) v[c] = values[((int64_t)(ci + ((c >> 2) & 1)) * ny + (cj + ((c >> 1) & 1))) * nz + (ck + (c & 1))];
		const int mask = corner_mask(v, iso);
		const int n = popcount12(crossing_edges(mask));
		if (n == 0) continue;
		for (int axis = 0; axis < 3; ++axis) {
			const int other = corner ^ (4 >> axis);
			if (!(((mask >> corner) ^ (mask >> other)) & 1)) continue;
			const int a = corner < other ? corner : other, b = corner < other ? other : corner;
			const float d = v[b] - v[a];
			if (!is_finite((iso - v[a]) / d)) continue;
			const float gg = grad_g[3 * m + axis] / (float)n;
			if (corner == a) {
				grad += (double)(gg * ((iso - v[b]) / (d * d)));
				giso += (double)(gg / d);
			} else {
				grad += (double)(gg * (-(iso - v[a]) / (d * d)));
			}
		}
	}
	*d_iso += giso;
	return (float)grad;
}

}  // namespace surface_nets
}  // namespace find
