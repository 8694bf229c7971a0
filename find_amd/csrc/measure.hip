// Foot measurements: the section of a mesh by planes (perimeter of the cut polyline, the number of faces cut) and the extents of a mesh
// along given directions.  Not in the reference.
//   section_fwd_kernel    a thread per face: the face is loaded once and tried against every plane.  s = fmaf(nz, z, fmaf(ny, y, nx * x)) - d
//                         per vertex (the same bits for a vertex in every face that shares it), "above" iff s >= 0.  A face whose vertices
//                         are not all on one side has one vertex alone on its side; the two edges from it cross, each at
//                         p = fmaf(t, hi - lo, lo), t = s_lo / (s_lo - s_hi) (lo below, hi above: the denominator is < 0), and the face
//                         adds |p1 - p2|.  fp32 per face; per plane a double (and a count) per workgroup, the waves' sums added in wave order.
//   section_sum_kernel    a thread per (mesh, plane) adds the workgroups' partials in workgroup order.  No float atomics anywhere.
//   section_bwd_kernel    the same pass with the chain rule through p, t and s: the nine corner gradients of every face, summed over the
//                         planes in plane order (zeros for a face that crosses none), and per plane a double partial of d perimeter / d d.
//   section_gather_kernel a thread per vertex adds its corners' gradients in the order of the vertex -> corner table (as vnormals_bwd_kernel).
//   section_doff_kernel   a thread per plane row adds the partials in workgroup order, and over the meshes in mesh order for shared planes.
//   extents_fwd_kernel    a workgroup per mesh, every direction in one pass: min / max of fmaf(dz, z, fmaf(dy, y, dx * x)) over the first
//                         v_len vertices and where they are taken; among equal values the smallest index.
//   extents_bwd_kernel    a thread per mesh walks lo_0, hi_0, lo_1, hi_1, ... and adds g * dir at the arg vertex.
// A face with an index outside [0, V) (the -1 rows that pad ragged meshes) or a repeated vertex contributes nothing and is never read through.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"
#include "section.h"

namespace find {
namespace measure {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_PLANES = 64;
constexpr int MAX_DIRS = 8;
constexpr int EXT_THREADS = 1024;

__device__ __forceinline__ float cut_length(const Cut& c) {
	float t;
	const V3 p1 = c.up ? crossing(c.A, c.L, c.sA, c.sL, t) : crossing(c.L, c.A, c.sL, c.sA, t);
	const V3 p2 = c.up ? crossing(c.B, c.L, c.sB, c.sL, t) : crossing(c.L, c.B, c.sL, c.sB, t);
	const float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
	return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(THREADS) void section_fwd_kernel(const Mesh m, double* __restrict__ part_len, int32_t* __restrict__ part_cnt) {
	__shared__ double w_len[WAVES][MAX_PLANES];
	__shared__ int32_t w_cnt[WAVES][MAX_PLANES];
	const int mesh = blockIdx.y, f = blockIdx.x * THREADS + threadIdx.x, wave = threadIdx.x >> 6;
	V3 v[3];
	const bool ok = load_face(m, mesh, f, v);
	const float* planes = m.planes + (int64_t)(m.pb == 1 ? 0 : mesh) * m.P * 4;
	for (int p = 0; p < m.P; ++p) {
		Cut c;
		const bool cuts = ok && cut_of(planes + 4 * p, v, c);
		const unsigned long long any = __ballot(cuts);
		double len = 0.0;
		if (any) {   // (the same for the whole wave)
			if (cuts) len = (double)cut_length(c);
			len = wave_sum(len);
		}
		if ((threadIdx.x & 63) == 0) {
			w_len[wave][p] = len;
			w_cnt[wave][p] = __popcll(any);
		}
	}
	__syncthreads();
	if ((int)threadIdx.x < m.P) {
		double len = 0.0;
		int cnt = 0;
		for (int w = 0; w < WAVES; ++w) {
			len += w_len[w][threadIdx.x];
			cnt += w_cnt[w][threadIdx.x];
		}
		const int64_t o = ((int64_t)mesh * gridDim.x + blockIdx.x) * m.P + threadIdx.x;
		part_len[o] = len;
		part_cnt[o] = cnt;
	}
}

__global__ __launch_bounds__(THREADS) void section_sum_kernel(const double* __restrict__ part_len, const int32_t* __restrict__ part_cnt, int64_t NP, int P,
															   int blocks, float* __restrict__ perimeter, int32_t* __restrict__ count) {
	const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (i >= NP) return;
	const int64_t mesh = i / P, p = i - mesh * P;
	double len = 0.0;
	int cnt = 0;
	for (int b = 0; b < blocks; ++b) {
		const int64_t o = (mesh * blocks + b) * P + p;
		len += part_len[o];
		cnt += part_cnt[o];
	}
	perimeter[i] = (float)len;
	count[i] = cnt;
}

// d |p1 - p2| of one crossing edge lo -> hi: gp = d / d p.  Adds to d lo, d hi; returns d / d d of the plane.
__device__ __forceinline__ float edge_bwd(const V3& lo, const V3& hi, float s_lo, float s_hi, const float* __restrict__ pl, const V3& gp, V3& d_lo, V3& d_hi) {
	const float den = s_lo - s_hi, t = s_lo / den;
	const float g_t = gp.x * (hi.x - lo.x) + gp.y * (hi.y - lo.y) + gp.z * (hi.z - lo.z);
	const float g_slo = g_t * (-s_hi / den / den), g_shi = g_t * (t / den);   // t = s_lo / (s_lo - s_hi)
	d_lo.x += (1.f - t) * gp.x + g_slo * pl[0]; d_lo.y += (1.f - t) * gp.y + g_slo * pl[1]; d_lo.z += (1.f - t) * gp.z + g_slo * pl[2];
	d_hi.x += t * gp.x + g_shi * pl[0]; d_hi.y += t * gp.y + g_shi * pl[1]; d_hi.z += t * gp.z + g_shi * pl[2];
	return -(g_slo + g_shi);   // s = n . v - d
}

__global__ __launch_bounds__(THREADS) void section_bwd_kernel(const Mesh m, const float* __restrict__ g, float* __restrict__ corner, double* __restrict__ part_doff) {
	__shared__ double w_doff[WAVES][MAX_PLANES];
	const int mesh = blockIdx.y, f = blockIdx.x * THREADS + threadIdx.x, wave = threadIdx.x >> 6;
	V3 v[3];
	const bool ok = load_face(m, mesh, f, v);
	const float* planes = m.planes + (int64_t)(m.pb == 1 ? 0 : mesh) * m.P * 4;
	const float* gm = g + (int64_t)mesh * m.P;
	const V3 zero{0.f, 0.f, 0.f};
	V3 d0 = zero, d1 = zero, d2 = zero;
	for (int p = 0; p < m.P; ++p) {
		const float* pl = planes + 4 * p;
		Cut c;
		const bool cuts = ok && cut_of(pl, v, c);
		double doff = 0.0;
		if (__ballot(cuts)) {
			if (cuts) {
				float t;
				const V3 p1 = c.up ? crossing(c.A, c.L, c.sA, c.sL, t) : crossing(c.L, c.A, c.sL, c.sA, t);
				const V3 p2 = c.up ? crossing(c.B, c.L, c.sB, c.sL, t) : crossing(c.L, c.B, c.sL, c.sB, t);
				const float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
				const float len = sqrtf(dx * dx + dy * dy + dz * dz);
				if (len > 0.f) {   // a segment of length 0 (a plane through one vertex) has no direction: gradient 0
					const float sc = gm[p] / len;
					const V3 g1{sc * dx, sc * dy, sc * dz}, g2{-g1.x, -g1.y, -g1.z};
					V3 dL = zero, dA = zero, dB = zero;
					float dd;
					if (c.up) {
						dd = edge_bwd(c.A, c.L, c.sA, c.sL, pl, g1, dA, dL);
						dd += edge_bwd(c.B, c.L, c.sB, c.sL, pl, g2, dB, dL);
					} else {
						dd = edge_bwd(c.L, c.A, c.sL, c.sA, pl, g1, dL, dA);
						dd += edge_bwd(c.L, c.B, c.sL, c.sB, pl, g2, dL, dB);
					}
					doff = (double)dd;
					// L is corner k, A corner k + 1, B corner k + 2
					const V3 e0 = c.k == 0 ? dL : (c.k == 1 ? dB : dA);
					const V3 e1 = c.k == 0 ? dA : (c.k == 1 ? dL : dB);
					const V3 e2 = c.k == 0 ? dB : (c.k == 1 ? dA : dL);
					d0.x += e0.x; d0.y += e0.y; d0.z += e0.z;
					d1.x += e1.x; d1.y += e1.y; d1.z += e1.z;
					d2.x += e2.x; d2.y += e2.y; d2.z += e2.z;
				}
			}
			doff = wave_sum(doff);
		}
		if ((threadIdx.x & 63) == 0) w_doff[wave][p] = doff;
	}
	if (f < m.F) {
		float* o = corner + ((int64_t)mesh * m.F + f) * 9;
		o[0] = d0.x; o[1] = d0.y; o[2] = d0.z; o[3] = d1.x; o[4] = d1.y; o[5] = d1.z; o[6] = d2.x; o[7] = d2.y; o[8] = d2.z;
	}
	__syncthreads();
	if ((int)threadIdx.x < m.P) {
		double s = 0.0;
		for (int w = 0; w < WAVES; ++w) s += w_doff[w][threadIdx.x];
		part_doff[((int64_t)mesh * gridDim.x + blockIdx.x) * m.P + threadIdx.x] = s;
	}
}

__global__ __launch_bounds__(THREADS) void section_gather_kernel(const int32_t* __restrict__ vf_off, const int32_t* __restrict__ vf_items, int64_t fb, int V,
																  int F, const float* __restrict__ corner, float* __restrict__ d_verts) {
	const int mesh = blockIdx.y, v = blockIdx.x * THREADS + threadIdx.x;
	if (v >= V) return;
	const int tb = fb == 1 ? 0 : mesh;
	const int32_t* off = vf_off + (int64_t)tb * (V + 1);
	const int32_t* items = vf_items + (int64_t)tb * F * 3;
	const float* cm = corner + (int64_t)mesh * F * 9;
	const int b = max(off[v], 0), e = min(off[v + 1], 3 * F);
	float dx = 0.f, dy = 0.f, dz = 0.f;
	for (int j = b; j < e; ++j) {
		const int item = items[j];
		if ((unsigned)item >= (unsigned)(3 * F)) continue;
		const float* q = cm + 3 * (int64_t)item;   // (face * 9 + corner * 3)
		dx += q[0]; dy += q[1]; dz += q[2];
	}
	float* o = d_verts + ((int64_t)mesh * V + v) * 3;
	o[0] = dx; o[1] = dy; o[2] = dz;
}

// d_offset[row, p]: the partials of the row's mesh in workgroup order; shared planes (pb == 1): mesh after mesh
__global__ __launch_bounds__(THREADS) void section_doff_kernel(const double* __restrict__ part_doff, int64_t rows, int P, int blocks, int meshes_per_row,
																float* __restrict__ d_offset) {
	const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (i >= rows * P) return;
	const int64_t row = i / P, p = i - row * P;
	double s = 0.0;
	for (int64_t mesh = row * meshes_per_row; mesh < (row + 1) * meshes_per_row; ++mesh)
		for (int b = 0; b < blocks; ++b) s += part_doff[(mesh * blocks + b) * P + p];
	d_offset[i] = (float)s;
}

// ------------------------------------------------------------------------------------------------ extents
struct Dirs {
	float d[MAX_DIRS][3];
};

__device__ __forceinline__ void load_dirs(const float* __restrict__ dirs, int D, Dirs& out) {
#pragma unroll
	for (int d = 0; d < MAX_DIRS; ++d)
#pragma unroll
		for (int k = 0; k < 3; ++k) out.d[d][k] = d < D ? dirs[3 * d + k] : 0.f;
}

// (value, index) a before b: the smaller value (want_max: the larger), then the smaller index; an index of -1 is "nothing yet"
__device__ __forceinline__ bool before(float va, int ia, float vb, int ib, bool want_max) {
	if (ib < 0) return ia >= 0;
	if (ia < 0) return false;
	return (want_max ? va > vb : va < vb) || (va == vb && ia < ib);
}

__global__ __launch_bounds__(EXT_THREADS) void extents_fwd_kernel(const float* __restrict__ verts, const int32_t* __restrict__ v_len, const float* __restrict__ dirs_in, int V, int D,
																   float* __restrict__ lo, float* __restrict__ hi, int32_t* __restrict__ arg_lo,
																   int32_t* __restrict__ arg_hi) {
	__shared__ float w_val[2][MAX_DIRS][EXT_THREADS / 64];
	__shared__ int32_t w_idx[2][MAX_DIRS][EXT_THREADS / 64];
	const int mesh = blockIdx.x;
	Dirs dirs;
	load_dirs(dirs_in, D, dirs);
	const int n = v_len ? min(max(v_len[mesh], 0), V) : V;
	const float* vp = verts + (int64_t)mesh * V * 3;
	float vmin[MAX_DIRS], vmax[MAX_DIRS];
	int imin[MAX_DIRS], imax[MAX_DIRS];
#pragma unroll
	for (int d = 0; d < MAX_DIRS; ++d) {
		vmin[d] = vmax[d] = 0.f;
		imin[d] = imax[d] = -1;
	}
	for (int v = threadIdx.x; v < n; v += EXT_THREADS) {   // (ascending per thread: the first of equal values stays)
		const float x = vp[3 * (int64_t)v], y = vp[3 * (int64_t)v + 1], z = vp[3 * (int64_t)v + 2];
#pragma unroll
		for (int d = 0; d < MAX_DIRS; ++d) {
			if (d < D) {
				const float s = fmaf(dirs.d[d][2], z, fmaf(dirs.d[d][1], y, dirs.d[d][0] * x));
				if (imin[d] < 0 || s < vmin[d]) { vmin[d] = s; imin[d] = v; }
				if (imax[d] < 0 || s > vmax[d]) { vmax[d] = s; imax[d] = v; }
			}
		}
	}
	const int wave = threadIdx.x >> 6;
#pragma unroll
	for (int d = 0; d < MAX_DIRS; ++d) {
		if (d < D) {
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				const float a = __shfl_xor(vmin[d], o, 64), b = __shfl_xor(vmax[d], o, 64);
				const int ia = __shfl_xor(imin[d], o, 64), ib = __shfl_xor(imax[d], o, 64);
				if (before(a, ia, vmin[d], imin[d], false)) { vmin[d] = a; imin[d] = ia; }
				if (before(b, ib, vmax[d], imax[d], true)) { vmax[d] = b; imax[d] = ib; }
			}
			if ((threadIdx.x & 63) == 0) {
				w_val[0][d][wave] = vmin[d]; w_idx[0][d][wave] = imin[d];
				w_val[1][d][wave] = vmax[d]; w_idx[1][d][wave] = imax[d];
			}
		}
	}
	__syncthreads();
	if ((int)threadIdx.x < 2 * D) {
		const int which = threadIdx.x & 1, d = threadIdx.x >> 1;
		float best = 0.f;
		int at = -1;
		for (int w = 0; w < EXT_THREADS / 64; ++w)
			if (before(w_val[which][d][w], w_idx[which][d][w], best, at, which == 1)) { best = w_val[which][d][w]; at = w_idx[which][d][w]; }
		const int64_t o = (int64_t)mesh * D + d;
		if (at < 0) best = 0.f;
		if (which) { hi[o] = best; arg_hi[o] = at; } else { lo[o] = best; arg_lo[o] = at; }
	}
}

__global__ __launch_bounds__(64) void extents_bwd_kernel(const float* __restrict__ g_lo, const float* __restrict__ g_hi, const int32_t* __restrict__ arg_lo,
														  const int32_t* __restrict__ arg_hi, const float* __restrict__ dirs_in, int64_t N, int V, int D, float* __restrict__ d_verts) {
	const int64_t mesh = (int64_t)blockIdx.x * 64 + threadIdx.x;
	if (mesh >= N) return;
	float* dv = d_verts + mesh * V * 3;
	for (int d = 0; d < D; ++d) {
		for (int which = 0; which < 2; ++which) {
			const int at = (which ? arg_hi : arg_lo)[mesh * D + d];
			const float* gp = which ? g_hi : g_lo;
			if ((unsigned)at >= (unsigned)V || !gp) continue;
			const float gv = gp[mesh * D + d];
			float* o = dv + 3 * (int64_t)at;
			o[0] += gv * dirs_in[3 * d]; o[1] += gv * dirs_in[3 * d + 1]; o[2] += gv * dirs_in[3 * d + 2];
		}
	}
}

inline int64_t blocks_of(int64_t F) { return cdiv(F, THREADS); }
// forward: [part_len (N B P) double | part_cnt (N B P) int32]; backward: [corner (N F 9) float | part_doff (N B P) double]
inline int64_t fwd_bytes(int64_t N, int64_t F, int64_t P) { return align_up(N * blocks_of(F) * P * 8, 256) + align_up(N * blocks_of(F) * P * 4, 256); }
inline int64_t bwd_bytes(int64_t N, int64_t F, int64_t P) { return align_up(N * F * 9 * 4, 256) + align_up(N * blocks_of(F) * P * 8, 256); }

}  // namespace measure
}  // namespace find

using namespace find;

static bool section_sizes(int64_t N, int64_t V, int64_t F, int64_t P) {
	return N >= 1 && N < 65536 && V >= 1 && V < ((int64_t)1 << 28) && F >= 1 && F < ((int64_t)1 << 24) && P >= 1 && P <= measure::MAX_PLANES
		   && N * F < ((int64_t)1 << 32);
}

static int section_args(const char* who, const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
						int64_t V, int64_t F, int64_t P, measure::Mesh* m) {
	if (!verts || !faces || !planes) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!section_sizes(N, V, F, P) || !(faces_batch == 1 || faces_batch == N) || !(planes_batch == 1 || planes_batch == N)) {
		set_error("%s: bad sizes N=%lld V=%lld F=%lld P=%lld (1 .. %d) faces_batch=%lld planes_batch=%lld (1 or N)", who, (long long)N, (long long)V, (long long)F,
				  (long long)P, measure::MAX_PLANES, (long long)faces_batch, (long long)planes_batch);
		return FIND_EINVAL;
	}
	m->verts = verts; m->faces = faces; m->planes = planes; m->fb = faces_batch; m->pb = planes_batch; m->V = (int)V; m->F = (int)F; m->P = (int)P;
	return FIND_OK;
}

static int section_ws(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
	if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7)) {
		set_error("%s: workspace of %lld bytes, %lld needed (8-byte aligned)", who, (long long)ws_bytes, (long long)need);
		return FIND_EWORKSPACE;
	}
	return FIND_OK;
}

extern "C" int64_t find_plane_sections_ws_bytes(int64_t N, int64_t F, int64_t P, int backward) {
	if (!section_sizes(N, 1, F, P)) {
		set_error("find_plane_sections_ws_bytes: bad sizes N=%lld F=%lld P=%lld (1 .. %d)", (long long)N, (long long)F, (long long)P, measure::MAX_PLANES);
		return -1;
	}
	return backward ? measure::bwd_bytes(N, F, P) : measure::fwd_bytes(N, F, P);
}

extern "C" int find_plane_sections_fwd(const float* verts, const int32_t* faces, int64_t faces_batch, const float* planes, int64_t planes_batch, int64_t N,
									   int64_t V, int64_t F, int64_t P, float* perimeter, int32_t* count, void* ws, int64_t ws_bytes, void* stream) {
	measure::Mesh m;
	if (section_args("find_plane_sections_fwd", verts, faces, faces_batch, planes, planes_batch, N, V, F, P, &m) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(perimeter && count, "find_plane_sections_fwd: NULL argument");
	int rc = section_ws("find_plane_sections_fwd", ws, ws_bytes, measure::fwd_bytes(N, F, P));
	if (rc != FIND_OK) return rc;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = measure::blocks_of(F);
	Carver cv(ws);
	double* part_len = cv.take<double>(N * blocks * P);
	int32_t* part_cnt = cv.take<int32_t>(N * blocks * P);
	hipLaunchKernelGGL(measure::section_fwd_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(measure::THREADS), 0, s, m, part_len, part_cnt);
	FIND_LAUNCH_CHECK("measure section_fwd_kernel");
	hipLaunchKernelGGL(measure::section_sum_kernel, dim3((unsigned)cdiv(N * P, measure::THREADS)), dim3(measure::THREADS), 0, s, (const double*)part_len,
					   (const int32_t*)part_cnt, N * P, (int)P, (int)blocks, perimeter, count);
	FIND_LAUNCH_CHECK("measure section_sum_kernel");
	return FIND_OK;
}

extern "C" int find_plane_sections_bwd(const float* verts, const int32_t* faces, int64_t faces_batch, const int32_t* vf_off, const int32_t* vf_items,
									   const float* planes, int64_t planes_batch, int64_t N, int64_t V, int64_t F, int64_t P, const float* g, float* d_verts,
									   float* d_offset, void* ws, int64_t ws_bytes, void* stream) {
	measure::Mesh m;
	if (section_args("find_plane_sections_bwd", verts, faces, faces_batch, planes, planes_batch, N, V, F, P, &m) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(vf_off && vf_items && g && d_verts, "find_plane_sections_bwd: NULL argument");
	int rc = section_ws("find_plane_sections_bwd", ws, ws_bytes, measure::bwd_bytes(N, F, P));
	if (rc != FIND_OK) return rc;
	hipStream_t s = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = measure::blocks_of(F);
	Carver cv(ws);
	float* corner = cv.take<float>(N * F * 9);
	double* part_doff = cv.take<double>(N * blocks * P);
	hipLaunchKernelGGL(measure::section_bwd_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(measure::THREADS), 0, s, m, g, corner, part_doff);
	FIND_LAUNCH_CHECK("measure section_bwd_kernel");
	hipLaunchKernelGGL(measure::section_gather_kernel, dim3((unsigned)cdiv(V, measure::THREADS), (unsigned)N), dim3(measure::THREADS), 0, s, vf_off, vf_items,
					   faces_batch, (int)V, (int)F, (const float*)corner, d_verts);
	FIND_LAUNCH_CHECK("measure section_gather_kernel");
	if (d_offset) {
		const int64_t rows = planes_batch == 1 ? 1 : N;
		hipLaunchKernelGGL(measure::section_doff_kernel, dim3((unsigned)cdiv(rows * P, measure::THREADS)), dim3(measure::THREADS), 0, s, (const double*)part_doff,
						   rows, (int)P, (int)blocks, (int)(planes_batch == 1 ? N : 1), d_offset);
		FIND_LAUNCH_CHECK("measure section_doff_kernel");
	}
	return FIND_OK;
}

static int extents_args(const char* who, const void* a, const void* b, const float* dirs, int64_t N, int64_t V, int64_t D) {
	if (!a || !b || !dirs) {
		set_error("%s: NULL argument", who);
		return FIND_EINVAL;
	}
	if (!(N >= 1 && N < ((int64_t)1 << 24) && V >= 1 && V < ((int64_t)1 << 28) && D >= 1 && D <= measure::MAX_DIRS)) {
		set_error("%s: bad sizes N=%lld V=%lld D=%lld (1 .. %d)", who, (long long)N, (long long)V, (long long)D, measure::MAX_DIRS);
		return FIND_EINVAL;
	}
	return FIND_OK;
}

extern "C" int find_extents_fwd(const float* verts, const int32_t* v_len, const float* dirs, int64_t N, int64_t V, int64_t D, float* lo, float* hi,
								int32_t* arg_lo, int32_t* arg_hi, void* stream) {
	if (extents_args("find_extents_fwd", verts, lo, dirs, N, V, D) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(hi && arg_lo && arg_hi, "find_extents_fwd: NULL argument");
	hipLaunchKernelGGL(measure::extents_fwd_kernel, dim3((unsigned)N), dim3(measure::EXT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), verts, v_len, dirs,
					   (int)V, (int)D, lo, hi, arg_lo, arg_hi);
	FIND_LAUNCH_CHECK("measure extents_fwd_kernel");
	return FIND_OK;
}

extern "C" int find_extents_bwd(const float* g_lo, const float* g_hi, const int32_t* arg_lo, const int32_t* arg_hi, const float* dirs, int64_t N,
								int64_t V, int64_t D, float* d_verts, void* stream) {
	if (extents_args("find_extents_bwd", arg_lo, arg_hi, dirs, N, V, D) != FIND_OK) return FIND_EINVAL;
	FIND_REQUIRE(d_verts && (g_lo || g_hi), "find_extents_bwd: NULL argument");
	hipLaunchKernelGGL(measure::extents_bwd_kernel, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), g_lo, g_hi, arg_lo, arg_hi,
					   dirs, N, (int)V, (int)D, d_verts);
	FIND_LAUNCH_CHECK("measure extents_bwd_kernel");
	return FIND_OK;
}
