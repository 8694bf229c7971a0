// Tape girths: the perimeter of the convex hull of the section of a mesh by a plane.  Not in the reference.
//   hull_fwd_kernel     a workgroup per (mesh, plane).  (1) The faces in chunks of 256, by the section rule of section.h (the bits of
//                       find_plane_sections_*): the crossing faces are compacted in face order by a ballot / wave-count scan -- no cursor, no
//                       atomics -- and each writes its two points (edge 0: L-A, edge 1: L-B of its Cut; id = 2 face + edge) in the plane's
//                       2-D coordinates (p . e1, p . e2), fp32 fma chains, to the workspace and, the first LDS_POINTS of them, to LDS.
//                       (2) Gift wrapping, counter-clockwise from the lexicographically smallest point: per step every thread folds its
//                       points by the orientation predicate -- double, on the fp32 coordinates, uncontracted: the products of two
//                       differences and their comparison --, lanes by butterfly, waves in wave order.  Among collinear points the farthest
//                       wins, among identical ones the smallest id, so corners are strict.  A section of more than LDS_POINTS points walks
//                       the workspace copy: the same code, the same result.  At most one step per point: a walk that has not come back to
//                       its start by then sets status bit 2.  (3) Corner i recomputes its 3-D point and its successor's from their ids;
//                       |p_i - p_i+1| in fp32, summed in double (lanes by butterfly, waves in wave order, chunks of 256 corners in order).
//   hull_bwd_kernel     a workgroup per mesh over its corners, plane after plane in one list, 256 at a time: a thread per corner forms
//                       g ((p - a) / |p - a| + (p - b) / |p - b|) from its neighbours a, b (a zero distance is masked), chains it through
//                       p, t and s to the two vertices of its mesh edge -- two records (vertex, gradient) in LDS -- and to the plane's four
//                       components (thread 4 p + k adds component k of plane p in corner order).  All of it in DOUBLE from the fp32 inputs, the sides as the fp32 rule decided them:
//                       a hull has few corners, each with its own 1 / (s_lo - s_hi), and a sum over a dozen such terms in fp32 is as good
//                       as its worst one (there are only hundreds of corners: the cost is nothing).  The first record of a vertex among
//                       a round's 512 adds them all, in record order, and adds that sum into d_verts (rounded to fp32 once per round):
//                       one writer per vertex and barrier, so the order is fixed.  No float atomics.
//   hull_dplane_kernel  a thread per plane component adds the meshes' partials in mesh order (shared planes) and rounds to fp32.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"
#include "section.h"

namespace find {
namespace girth {

using measure::Cut;
using measure::Mesh;
using measure::V3;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_PLANES = 64;
constexpr int LDS_POINTS = 2048;   // points (two per crossing face) a workgroup keeps on chip: 16 KB
static_assert(THREADS >= 4 * MAX_PLANES, "hull_bwd_kernel: a thread per plane component");

struct Basis {
	V3 e1, e2;
};

// a: the coordinate axis of the smallest |n_k| (lowest index on ties); e1 = normalize(n x a), e2 = n x e1
__device__ __forceinline__ Basis basis_of(const float* __restrict__ pl) {
	const float nx = pl[0], ny = pl[1], nz = pl[2];
	const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
	const bool k1 = ay < ax, k2 = az < (k1 ? ay : ax);
	// n x (1, 0, 0) = (0, nz, -ny); n x (0, 1, 0) = (-nz, 0, nx); n x (0, 0, 1) = (ny, -nx, 0)
	const float x = k2 ? ny : (k1 ? -nz : 0.f), y = k2 ? -nx : (k1 ? 0.f : nz), z = k2 ? 0.f : (k1 ? nx : -ny);
	const float inv = 1.f / sqrtf(x * x + y * y + z * z);
	Basis b;
	b.e1 = V3{x * inv, y * inv, z * inv};
	b.e2 = V3{ny * b.e1.z - nz * b.e1.y, nz * b.e1.x - nx * b.e1.z, nx * b.e1.y - ny * b.e1.x};
	return b;
}

__device__ __forceinline__ float2 project(const Basis& b, const V3& p) {
	return make_float2(fmaf(b.e1.z, p.z, fmaf(b.e1.y, p.y, b.e1.x * p.x)), fmaf(b.e2.z, p.z, fmaf(b.e2.y, p.y, b.e2.x * p.x)));
}

// The point of a crossing face on edge e (0: L-A, 1: L-B), oriented from the vertex below to the one above.
struct EdgeCut {
	V3 lo, hi, p;
	float s_lo, s_hi, t;
	int c_lo, c_hi;   // corners of the face (0 .. 2)
};

__device__ __forceinline__ void edge_of(const Cut& c, int e, EdgeCut& o) {
	const V3 other = e ? c.B : c.A;
	const float s_other = e ? c.sB : c.sA;
	const int k_other = (c.k + 1 + e) % 3;
	if (c.up) {
		o.lo = other; o.hi = c.L; o.s_lo = s_other; o.s_hi = c.sL; o.c_lo = k_other; o.c_hi = c.k;
	} else {
		o.lo = c.L; o.hi = other; o.s_lo = c.sL; o.s_hi = s_other; o.c_lo = c.k; o.c_hi = k_other;
	}
	o.p = measure::crossing(o.lo, o.hi, o.s_lo, o.s_hi, o.t);
}

// the point of id = 2 face + edge; false (and zeros) for an id that names no crossing face
__device__ __forceinline__ bool point_of(const Mesh& m, int mesh, const float* __restrict__ pl, int id, EdgeCut& o) {
	V3 v[3];
	Cut c;
	o.p = V3{0.f, 0.f, 0.f};
	if (id < 0 || !measure::load_face(m, mesh, id >> 1, v) || !measure::cut_of(pl, v, c)) return false;
	edge_of(c, id & 1, o);
	return true;
}

struct Cand {
	float x, y;
	int slot;   // -1: none
};

// From the corner c, does r come before q?  r lies clockwise of c -> q; collinear: the farther one; identical: the smaller slot.
// Differences of fp32 numbers are exact in double and so, short of 2^-53, are their products: kept apart from the subtraction.
__device__ __forceinline__ bool turns_before(float cx, float cy, const Cand& q, const Cand& r) {
#pragma clang fp contract(off)
	const double qx = (double)q.x - (double)cx, qy = (double)q.y - (double)cy, rx = (double)r.x - (double)cx, ry = (double)r.y - (double)cy;
	const double a = qx * ry, b = qy * rx;
	if (a < b) return true;
	if (a > b) return false;
	if (fabs(rx) != fabs(qx)) return fabs(rx) > fabs(qx);
	if (fabs(ry) != fabs(qy)) return fabs(ry) > fabs(qy);
	return r.slot < q.slot;
}

struct NextFrom {
	float cx, cy;
	__device__ __forceinline__ Cand operator()(const Cand& q, const Cand& r) const {
		const bool take = r.slot >= 0 && (q.slot < 0 || turns_before(cx, cy, q, r));
		return Cand{take ? r.x : q.x, take ? r.y : q.y, take ? r.slot : q.slot};
	}
};

struct LexMin {
	__device__ __forceinline__ Cand operator()(const Cand& q, const Cand& r) const {
		const bool before = r.x < q.x || (r.x == q.x && (r.y < q.y || (r.y == q.y && r.slot < q.slot)));
		const bool take = r.slot >= 0 && (q.slot < 0 || before);
		return Cand{take ? r.x : q.x, take ? r.y : q.y, take ? r.slot : q.slot};
	}
};

// every thread gets the same winner: lanes by butterfly (lane 0's result), waves in wave order
template <typename Op>
__device__ __forceinline__ Cand block_fold(Cand v, const Op& op, Cand* s_wave) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		Cand other;
		other.x = __shfl_xor(v.x, o, 64); other.y = __shfl_xor(v.y, o, 64); other.slot = __shfl_xor(v.slot, o, 64);
		v = op(v, other);
	}
	if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
	__syncthreads();
	Cand best = s_wave[0];
#pragma unroll
	for (int w = 1; w < WAVES; ++w) best = op(best, s_wave[w]);
	__syncthreads();
	return best;
}

__device__ __forceinline__ void wave_sums(double* v, int n, double (*s_wave)[4]) {
	for (int k = 0; k < n; ++k) v[k] = wave_sum(v[k]);
	if ((threadIdx.x & 63) == 0)
		for (int k = 0; k < n; ++k) s_wave[threadIdx.x >> 6][k] = v[k];
	__syncthreads();
	for (int k = 0; k < n; ++k) {
		double s = 0.0;
		for (int w = 0; w < WAVES; ++w) s += s_wave[w][k];
		v[k] = s;
	}
	__syncthreads();
}

__global__ __launch_bounds__(THREADS) void hull_fwd_kernel(const Mesh m, int max_points, int max_hull, int32_t* __restrict__ ws_faces, float2* __restrict__ ws_xy,
															float* __restrict__ girth, int32_t* __restrict__ count, int32_t* __restrict__ n_hull,
															int32_t* __restrict__ status, int32_t* __restrict__ hull_ids, float* __restrict__ hull_points) {
	__shared__ float2 s_xy[LDS_POINTS];
	__shared__ int s_cnt[WAVES];
	__shared__ Cand s_cand[WAVES];
	__shared__ double s_sum[WAVES][4];
	const int p = blockIdx.x, mesh = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int64_t row = (int64_t)mesh * m.P + p;
	const float* pl = m.planes + ((int64_t)(m.pb == 1 ? 0 : mesh) * m.P + p) * 4;
	const Basis basis = basis_of(pl);
	int32_t* faces_of = ws_faces + row * max_points;
	float2* xy_of = ws_xy + row * 2 * max_points;
	int32_t* hull = hull_ids + row * 2 * max_points;

	// (1) the crossing faces, compacted in face order
	int total = 0;
	for (int f0 = 0; f0 < m.F; f0 += THREADS) {
		V3 v[3];
		Cut c;
		const int f = f0 + tid;
		const bool cuts = measure::load_face(m, mesh, f, v) && measure::cut_of(pl, v, c);
		const unsigned long long mask = __ballot(cuts);
		if (lane == 0) s_cnt[wave] = __popcll(mask);
		__syncthreads();
		int off = total + __popcll(mask & ((1ull << lane) - 1ull));
		for (int w = 0; w < WAVES; ++w) {
			if (w < wave) off += s_cnt[w];
			total += s_cnt[w];
		}
		if (cuts && off < max_points) {
			faces_of[off] = f;
#pragma unroll
			for (int e = 0; e < 2; ++e) {
				EdgeCut ec;
				edge_of(c, e, ec);
				const float2 q = project(basis, ec.p);
				xy_of[2 * off + e] = q;
				if (2 * off + e < LDS_POINTS) s_xy[2 * off + e] = q;
			}
		}
		__syncthreads();
	}
	int st = total > max_points ? 1 : 0;
	const int n_pts = st ? 0 : 2 * total;
	const float2* pts = n_pts <= LDS_POINTS ? (const float2*)s_xy : (const float2*)xy_of;

	// (2) the walk
	int nh = 0;
	if (n_pts > 0) {
		Cand mine{0.f, 0.f, -1};
		const LexMin lex;
		for (int j = tid; j < n_pts; j += THREADS) mine = lex(mine, Cand{pts[j].x, pts[j].y, j});
		const Cand start = block_fold(mine, lex, s_cand);
		if (tid == 0) hull[0] = 2 * faces_of[start.slot >> 1] + (start.slot & 1);
		nh = 1;
		bool closed = false;
		NextFrom from{start.x, start.y};
		for (int step = 0; step < n_pts; ++step) {
			mine = Cand{0.f, 0.f, -1};
			for (int j = tid; j < n_pts; j += THREADS) {
				const float2 q = pts[j];
				if (q.x == from.cx && q.y == from.cy) continue;
				mine = from(mine, Cand{q.x, q.y, j});
			}
			const Cand next = block_fold(mine, from, s_cand);
			if (next.slot < 0 || (next.x == start.x && next.y == start.y)) {   // one distinct point, or back at the start
				closed = true;
				break;
			}
			if (nh >= n_pts) break;
			if (tid == 0) hull[nh] = 2 * faces_of[next.slot >> 1] + (next.slot & 1);
			++nh;
			from.cx = next.x; from.cy = next.y;
		}
		if (!closed) {
			st |= 2;
			nh = 0;
		}
	}
	__syncthreads();   // hull[] is thread 0's

	// (3) the girth and the corners' points
	double sum = 0.0;
	const int top = max(nh, hull_points ? max_hull : 0);
	for (int base = 0; base < top; base += THREADS) {
		const int i = base + tid;
		EdgeCut a, b;
		a.p = V3{0.f, 0.f, 0.f};
		double d = 0.0;
		if (i < nh) {
			point_of(m, mesh, pl, hull[i], a);
			point_of(m, mesh, pl, hull[i + 1 < nh ? i + 1 : 0], b);
			const float dx = a.p.x - b.p.x, dy = a.p.y - b.p.y, dz = a.p.z - b.p.z;
			d = (double)sqrtf(dx * dx + dy * dy + dz * dz);
		}
		if (hull_points && i < max_hull) {
			float* o = hull_points + (row * max_hull + i) * 3;
			o[0] = a.p.x; o[1] = a.p.y; o[2] = a.p.z;
		}
		if (base < nh) {
			double part[4] = {d, 0.0, 0.0, 0.0};
			wave_sums(part, 1, s_sum);
			sum += part[0];
		}
	}
	if (tid == 0) {
		girth[row] = (float)sum;
		count[row] = total;
		n_hull[row] = nh;
		status[row] = st;
	}
}

// The corner of `c` once more, in double from the same fp32 inputs (the sides are the fp32 rule's: c says which vertex is below).
struct EdgeCutD {
	double lo[3], hi[3], p[3], s_lo, s_hi, t;
};

__device__ __forceinline__ void in_double(const EdgeCut& c, const float* __restrict__ pl, EdgeCutD& o) {
	o.lo[0] = c.lo.x; o.lo[1] = c.lo.y; o.lo[2] = c.lo.z;
	o.hi[0] = c.hi.x; o.hi[1] = c.hi.y; o.hi[2] = c.hi.z;
	const double nx = pl[0], ny = pl[1], nz = pl[2], d = pl[3];
	o.s_lo = fma(nz, o.lo[2], fma(ny, o.lo[1], nx * o.lo[0])) - d;
	o.s_hi = fma(nz, o.hi[2], fma(ny, o.hi[1], nx * o.hi[0])) - d;
	const double den = o.s_lo - o.s_hi;
	o.t = den < 0.0 ? o.s_lo / den : (double)c.t;   // (fp32 has s_lo < 0 <= s_hi; within its rounding double may not)
	for (int k = 0; k < 3; ++k) o.p[k] = fma(o.t, o.hi[k] - o.lo[k], o.lo[k]);
}

// adds (p - q) / |p - q| to u; a distance of 0 has no direction: masked
__device__ __forceinline__ void add_direction(const double* p, const double* q, double* u) {
	const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2], len = sqrt(dx * dx + dy * dy + dz * dz);
	if (len > 0.0) { u[0] += dx / len; u[1] += dy / len; u[2] += dz / len; }
}

__global__ __launch_bounds__(THREADS) void hull_bwd_kernel(const Mesh m, int cap, const float* __restrict__ g, const int32_t* __restrict__ n_hull,
															const int32_t* __restrict__ hull_ids, float* __restrict__ d_verts, double* __restrict__ part) {
	__shared__ int s_off[MAX_PLANES + 1];   // the mesh's corners, plane after plane: where each plane's begin
	__shared__ __attribute__((aligned(16))) int s_vid[2 * THREADS];
	__shared__ double s_g[2 * THREADS][3];
	__shared__ double s_dpl[THREADS][4];
	const int mesh = blockIdx.x, tid = threadIdx.x;
	float* dv = d_verts + (int64_t)mesh * m.V * 3;
	for (int64_t i = tid; i < (int64_t)m.V * 3; i += THREADS) dv[i] = 0.f;
	if (tid == 0) {
		int off = 0;
		for (int p = 0; p < m.P; ++p) {
			const int nh = min(max(n_hull[(int64_t)mesh * m.P + p], 0), cap);
			s_off[p] = off;
			off += nh >= 2 ? nh : 0;   // (one corner or none: a girth of 0, nothing to differentiate)
		}
		s_off[m.P] = off;
	}
	__syncthreads();
	const int total = s_off[m.P];
	const int32_t* fm = m.faces + (int64_t)(m.fb == 1 ? 0 : mesh) * m.F * 3;
	const int my_plane = tid >> 2, my_k = tid & 3;   // thread 4 p + k sums component k of plane p
	double acc = 0.0;
	for (int base = 0; base < total; base += THREADS) {
		const int i = base + tid;
		int v_lo = -1, v_hi = -1;
		double d_lo[3] = {0.0, 0.0, 0.0}, d_hi[3] = {0.0, 0.0, 0.0}, dpl[4] = {0.0, 0.0, 0.0, 0.0};
		if (i < total) {
			int p = 0;
			for (int step = 32; step > 0; step >>= 1)   // the last plane that begins at or before i (P <= 64)
				if (p + step < m.P && s_off[p + step] <= i) p += step;
			while (p + 1 < m.P && s_off[p + 1] <= i) ++p;
			const int64_t row = (int64_t)mesh * m.P + p;
			const float* pl = m.planes + ((int64_t)(m.pb == 1 ? 0 : mesh) * m.P + p) * 4;
			const int32_t* hull = hull_ids + row * cap;
			const int nh = s_off[p + 1] - s_off[p], k = i - s_off[p];
			const double gr = (double)g[row];
			EdgeCut c, a, b;
			if (point_of(m, mesh, pl, hull[k], c)) {
				const bool has_a = point_of(m, mesh, pl, hull[k > 0 ? k - 1 : nh - 1], a), has_b = point_of(m, mesh, pl, hull[k + 1 < nh ? k + 1 : 0], b);
				EdgeCutD cd, nb;
				in_double(c, pl, cd);
				double gp[3] = {0.0, 0.0, 0.0};
				if (has_a) {
					in_double(a, pl, nb);
					add_direction(cd.p, nb.p, gp);
				}
				if (has_b) {
					in_double(b, pl, nb);
					add_direction(cd.p, nb.p, gp);
				}
				// p = lo + t (hi - lo), t = s_lo / (s_lo - s_hi), s = n . v - d
				const double den = cd.s_lo - cd.s_hi, t = cd.t;
				if (den < 0.0) {
					double g_t = 0.0;
					for (int q = 0; q < 3; ++q) {
						gp[q] *= gr;
						g_t += gp[q] * (cd.hi[q] - cd.lo[q]);
					}
					const double g_slo = g_t * (-cd.s_hi / den / den), g_shi = g_t * (t / den);
					for (int q = 0; q < 3; ++q) {
						d_lo[q] = (1.0 - t) * gp[q] + g_slo * (double)pl[q];
						d_hi[q] = t * gp[q] + g_shi * (double)pl[q];
						dpl[q] = g_slo * cd.lo[q] + g_shi * cd.hi[q];
					}
					dpl[3] = -(g_slo + g_shi);
					const int32_t* fr = fm + 3 * (int64_t)(hull[k] >> 1);   // (point_of has checked the face)
					v_lo = fr[c.c_lo]; v_hi = fr[c.c_hi];
				}
			}
		}
		s_vid[2 * tid] = v_lo; s_vid[2 * tid + 1] = v_hi;
		for (int q = 0; q < 3; ++q) {
			s_g[2 * tid][q] = d_lo[q];
			s_g[2 * tid + 1][q] = d_hi[q];
		}
		for (int q = 0; q < 4; ++q) s_dpl[tid][q] = dpl[q];
		__syncthreads();
		const int n_here = min(THREADS, total - base);
		const int4* vid4 = reinterpret_cast<const int4*>(s_vid);   // (every lane reads the same address: a broadcast)
		for (int r = 2 * tid; r < 2 * tid + 2; ++r) {
			const int v = s_vid[r];
			if (v < 0) continue;
			bool first = true;
			double sx = 0.0, sy = 0.0, sz = 0.0;
			auto hit = [&](int vid, int j) {   // records of this vertex: one before r makes that one the writer; r and those after it are added in order
				if (vid != v) return;
				if (j < r) {
					first = false;
				} else {
					sx += s_g[j][0]; sy += s_g[j][1]; sz += s_g[j][2];
				}
			};
#pragma unroll 4
			for (int q = 0; q < (2 * n_here + 3) / 4; ++q) {   // (the records past 2 n_here are -1)
				const int4 w = vid4[q];
				hit(w.x, 4 * q); hit(w.y, 4 * q + 1); hit(w.z, 4 * q + 2); hit(w.w, 4 * q + 3);
			}
			if (!first) continue;
			float* o = dv + 3 * (int64_t)v;
			o[0] = (float)((double)o[0] + sx); o[1] = (float)((double)o[1] + sy); o[2] = (float)((double)o[2] + sz);
		}
		if (my_plane < m.P) {
			const int from = max(s_off[my_plane], base) - base, to = min(s_off[my_plane + 1], base + n_here) - base;
			for (int j = from; j < to; ++j) acc += s_dpl[j][my_k];
		}
		__syncthreads();
	}
	if (my_plane < m.P) part[((int64_t)mesh * m.P + my_plane) * 4 + my_k] = acc;
}

// d_planes[r, p, k]: the partial of the row's mesh; shared planes (one row): mesh after mesh
__global__ __launch_bounds__(THREADS) void hull_dplane_kernel(const double* __restrict__ part, int64_t rows, int P, int meshes_per_row, float* __restrict__ d_planes) {
	const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (i >= rows * P * 4) return;
	const int64_t r = i / (P * 4), pk = i - r * (P * 4);
	double s = 0.0;
	for (int64_t mesh = r * meshes_per_row; mesh < (r + 1) * meshes_per_row; ++mesh) s += part[mesh * P * 4 + pk];
	d_planes[i] = (float)s;
}

// forward: [faces (N P max_points) int32 | xy (N P 2 max_points) float2]; backward: [part (N P 4) double]
inline int64_t fwd_bytes(int64_t N, int64_t P, int64_t mp) { return align_up(N * P * mp * 4, 256) + align_up(N * P * 2 * mp * 8, 256); }
inline int64_t bwd_bytes(int64_t N, int64_t P) { return align_up(N * P * 4 * 8, 256); }

}  // namespace girth
}  // namespace find

using namespace find;

static bool hull_sizes(int64_t N, int64_t V, int64_t F, int64_t P, int64_t max_points) {
	return N >= 1 && N < 65536 && V >= 1 && V < ((int64_t)1 << 28) && F >= 1 && F < ((int64_t)1 << 24) && P >= 1 && P <= girth::MAX_PLANES
		   && N * F < ((int64_t)1 << 32) && max_points >= 1 && max_points <= F;
}

static int hull_args(const char* who, const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
					 int64_t V, int64_t F, int64_t P, int64_t max_points, measure::Mesh* m) {
	if (!verts || !faces || !planes) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!hull_sizes(N, V, F, P, max_points) || !(faces_batch == 1 || faces_batch == N) || !(planes_batch == 1 || planes_batch == N)) {
		set_error("%s: bad sizes N=%lld V=%lld F=%lld P=%lld (1 .. %d) max_points=%lld (1 .. F) faces_batch=%lld planes_batch=%lld (1 or N)", who, (long long)N,
				  (long long)V, (long long)F, (long long)P, girth::MAX_PLANES, (long long)max_points, (long long)faces_batch, (long long)planes_batch);
		return FIND_EINVAL;
	}
	m->verts = verts; m->faces = faces; m->planes = planes; m->fb = faces_batch; m->pb = planes_batch; m->V = (int)V; m->F = (int)F; m->P = (int)P;
	return FIND_OK;
}

static int hull_ws(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
	if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7)) {
		set_error("%s: workspace of %lld bytes, %lld needed (8-byte aligned)", who, (long long)ws_bytes, (long long)need);
		return FIND_EWORKSPACE;
	}
	return FIND_OK;
}

extern "C" int64_t find_section_hull_ws_bytes(int64_t N, int64_t F, int64_t P, int64_t max_points, int backward) {
	if (!hull_sizes(N, 1, F, P, max_points)) {
		set_error("find_section_hull_ws_bytes: bad sizes N=%lld F=%lld P=%lld (1 .. %d) max_points=%lld (1 .. F)", (long long)N, (long long)F, (long long)P,
				  girth::MAX_PLANES, (long long)max_points);
		return -1;
	}
	return backward ? girth::bwd_bytes(N, P) : girth::fwd_bytes(N, P, max_points);
}

extern "C" int find_section_hull_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
									 int64_t V, int64_t F, int64_t P, int64_t max_points, int64_t max_hull, float* girth_out, int32_t* count, int32_t* n_hull,
									 int32_t* status, int32_t* hull_ids, float* hull_points, void* ws, int64_t ws_bytes, void* stream) {
	measure::Mesh m;
	if (hull_args("find_section_hull_fwd", verts, faces, faces_batch, planes, planes_batch, N, V, F, P, max_points, &m) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(girth_out && count && n_hull && status && hull_ids, "find_section_hull_fwd: NULL argument");
	FIND_REQUIRE(max_hull >= 0 && max_hull <= 2 * max_points && (hull_points || max_hull == 0), "find_section_hull_fwd: bad max_hull=%lld (0 .. 2 max_points; 0 without hull_points)",
				 (long long)max_hull);
	int rc = hull_ws("find_section_hull_fwd", ws, ws_bytes, girth::fwd_bytes(N, P, max_points));
	if (rc != FIND_OK) return rc;
	Carver cv(ws);
	int32_t* ws_faces = cv.take<int32_t>(N * P * max_points);
	float2* ws_xy = cv.take<float2>(N * P * 2 * max_points);
	hipLaunchKernelGGL(girth::hull_fwd_kernel, dim3((unsigned)P, (unsigned)N), dim3(girth::THREADS), 0, reinterpret_cast<hipStream_t>(stream), m, (int)max_points,
					   (int)max_hull, ws_faces, ws_xy, girth_out, count, n_hull, status, hull_ids, max_hull > 0 ? hull_points : (float*)nullptr);
	FIND_LAUNCH_CHECK("girth hull_fwd_kernel");
	return FIND_OK;
}

extern "C" int find_section_hull_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
									 int64_t V, int64_t F, int64_t P, int64_t max_points, const float* g, const int32_t* n_hull, const int32_t* hull_ids,
									 float* d_verts, float* d_planes, void* ws, int64_t ws_bytes, void* stream) {
	measure::Mesh m;
	if (hull_args("find_section_hull_bwd", verts, faces, faces_batch, planes, planes_batch, N, V, F, P, max_points, &m) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(g && n_hull && hull_ids && d_verts, "find_section_hull_bwd: NULL argument");
	int rc = hull_ws("find_section_hull_bwd", ws, ws_bytes, girth::bwd_bytes(N, P));
	if (rc != FIND_OK) return rc;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	double* part = reinterpret_cast<double*>(ws);
	hipLaunchKernelGGL(girth::hull_bwd_kernel, dim3((unsigned)N), dim3(girth::THREADS), 0, s, m, (int)(2 * max_points), g, n_hull, hull_ids, d_verts, part);
	FIND_LAUNCH_CHECK("girth hull_bwd_kernel");
	if (d_planes) {
		const int64_t rows = planes_batch == 1 ? 1 : N;
		hipLaunchKernelGGL(girth::hull_dplane_kernel, dim3((unsigned)cdiv(rows * P * 4, girth::THREADS)), dim3(girth::THREADS), 0, s, (const double*)part, rows, (int)P,
						   (int)(planes_batch == 1 ? N : 1), d_planes);
		FIND_LAUNCH_CHECK("girth hull_dplane_kernel");
	}
	return FIND_OK;
}
