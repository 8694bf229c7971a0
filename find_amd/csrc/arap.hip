// The as-rigid-as-possible energy (Sorkine & Alexa 2007) of N deformed meshes p (N, V, 3) against one rest mesh q (V, 3) that they share,
// over the vertex -> neighbour CSR of MeshTopology with one weight per entry.  Not in the reference.
//   E_n = (1 / W) sum_i sum_{j in N(i)} w_ij |(p_i - p_j) - R_i (q_i - q_j)|^2,   R_i: the rotation fitted to the cell (arap_math.h)
//   dE_n/dp_i = (2 / W) sum_{j in N(i)} w_ij [2 (p_i - p_j) - (R_i + R_j)(q_i - q_j)]      (the rotations held fixed: they minimise E)
//   cells_kernel     FWD_LANES = 4 lanes per vertex, TILE = 4 meshes per workgroup: a lane walks every fourth neighbour of its vertex, reads the
//                    entry's index, weight and rest edge ONCE and uses them for the tile's meshes, whose sums it keeps in registers; the four
//                    lanes add by xor-butterfly (every lane ends with the same bits); lane m of a vertex fits the rotation of mesh m -- no
//                    fit is done twice --; a second walk forms the cell energies.  Writes R (double), the cell energies / W and a partial
//                    sum per workgroup and mesh.
//   finish_kernel    a workgroup per mesh: the partials in a fixed order (a thread every 256th, lanes by butterfly, waves in wave order).
//   grad_kernel      the same layout with BWD_LANES = 8 lanes per vertex (no fit to share out; it gathers 72 bytes of R_j per neighbour and
//                    mesh): sum w e_p, sum w e_q and sum w R_j e_q per vertex, then 2 A - R_i B - C, scaled by 2 g_n / W.
//                    (Measured on the MI355X at (16, 6890) / (16, 50002): cells_kernel 49.5 / 237 us with 8 lanes -- every fit done twice --
//                    and 37.8 / 169 with 4; grad_kernel 20.4 / 98 us with 8 lanes and 23.2 / 126 with 4.)
// Everything in double, no atomics, every sum in a fixed order: two runs agree bit for bit, and a mesh's values do not depend on the batch
// (a tile's slots past the last mesh repeat that mesh and are not written).  Valence is unbounded: the walks are loops.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"
#include "arap_math.h"

namespace find {
namespace arap {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int FWD_LANES = 4, BWD_LANES = 8;  // per vertex: a workgroup holds THREADS / LANES vertices
constexpr int TILE = 4;                      // meshes per workgroup; TILE <= FWD_LANES: lane m of a vertex fits mesh m
static_assert(TILE <= FWD_LANES, "a lane per mesh of the tile");

struct Mesh {
	const float* p;          // (n, v, 3)
	const float* q;          // (v, 3)
	const int32_t* off;      // (v + 1)
	const int32_t* idx;      // (n_nbr)
	const float* w;          // (n_nbr)
	int n, v, n_nbr;
	double inv_w;            // 1 / W, or 0 for a mesh without edges
};

// the sum over the LANES lanes of a vertex, the same bits in each of them
template <int LANES>
__device__ __forceinline__ double vertex_sum(double x) {
#pragma unroll
	for (int o = 1; o < LANES; o <<= 1) x += __shfl_xor(x, o, 64);
	return x;
}

struct Cell {   // what a thread knows of its vertex
	int i, begin, end, sub;
	bool have;
	double q[3];
};

template <int LANES>
__device__ __forceinline__ Cell cell_of(const Mesh& a) {
	Cell c;
	c.sub = threadIdx.x & (LANES - 1);
	c.i = blockIdx.x * (THREADS / LANES) + (threadIdx.x / LANES);
	c.have = c.i < a.v;
	if (!c.have) c.i = a.v - 1;   // (such a thread walks nothing and writes nothing; it stays for the shuffles)
	const int b = min(max(a.off[c.i], 0), a.n_nbr), e = min(max(a.off[c.i + 1], b), a.n_nbr);
	c.begin = b + c.sub;
	c.end = c.have ? e : b;
	for (int k = 0; k < 3; ++k) c.q[k] = (double)a.q[3 * (int64_t)c.i + k];
	return c;
}

__global__ __launch_bounds__(THREADS) void cells_kernel(const Mesh a, double* __restrict__ R, float* __restrict__ cell, double* __restrict__ part_e,
														 int32_t* __restrict__ part_deg) {
	__shared__ double sm_e[WAVES][TILE];
	__shared__ int sm_d[WAVES][TILE];
	constexpr int LANES = FWD_LANES;
	const Cell c = cell_of<LANES>(a);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m0 = blockIdx.y * TILE;
	int64_t row[TILE];   // of the tile's meshes, in vertices
	double pi[TILE][3], S[TILE][9];
#pragma unroll
	for (int m = 0; m < TILE; ++m) {
		row[m] = (int64_t)min(m0 + m, a.n - 1) * a.v;
		for (int k = 0; k < 3; ++k) pi[m][k] = (double)a.p[3 * (row[m] + c.i) + k];
		zero9(S[m]);
	}
	for (int k = c.begin; k < c.end; k += LANES) {
		const int j = a.idx[k];
		if ((unsigned)j >= (unsigned)a.v) continue;
		const double w = (double)a.w[k];
		double eq[3];
		for (int t = 0; t < 3; ++t) eq[t] = c.q[t] - (double)a.q[3 * (int64_t)j + t];
#pragma unroll
		for (int m = 0; m < TILE; ++m) {
			double ep[3];
			for (int t = 0; t < 3; ++t) ep[t] = pi[m][t] - (double)a.p[3 * (row[m] + j) + t];
			accumulate(S[m], w, eq, ep);
		}
	}
	double mine[9];   // the sums of the mesh this lane fits
#pragma unroll
	for (int t = 0; t < 9; ++t) {
#pragma unroll
		for (int m = 0; m < TILE; ++m) S[m][t] = vertex_sum<LANES>(S[m][t]);
		mine[t] = S[0][t];
#pragma unroll
		for (int m = 1; m < TILE; ++m)
			if ((c.sub & (TILE - 1)) == m) mine[t] = S[m][t];
	}
	double Rm[9], d[3];
	const int ok = fit_rotation(mine, Rm, d) ? 1 : 0;
	// every lane of the vertex gets the tile's rotations from the lanes that fitted them
	const int first = lane & ~(LANES - 1);
	double Rt[TILE][9], E[TILE];
	int okt[TILE];
#pragma unroll
	for (int m = 0; m < TILE; ++m) {
#pragma unroll
		for (int t = 0; t < 9; ++t) Rt[m][t] = __shfl(Rm[t], first + m, 64);
		okt[m] = __shfl(ok, first + m, 64);
		E[m] = 0.;
	}
	for (int k = c.begin; k < c.end; k += LANES) {
		const int j = a.idx[k];
		if ((unsigned)j >= (unsigned)a.v) continue;
		const double w = (double)a.w[k];
		double eq[3];
		for (int t = 0; t < 3; ++t) eq[t] = c.q[t] - (double)a.q[3 * (int64_t)j + t];
#pragma unroll
		for (int m = 0; m < TILE; ++m) {
			double ep[3];
			for (int t = 0; t < 3; ++t) ep[t] = pi[m][t] - (double)a.p[3 * (row[m] + j) + t];
			E[m] += cell_term(w, Rt[m], eq, ep);
		}
	}
#pragma unroll
	for (int m = 0; m < TILE; ++m) {
		E[m] = vertex_sum<LANES>(E[m]);
		if (c.have && c.sub == m && m0 + m < a.n) {   // (lane m fitted mesh m: Rm is its rotation)
			const int64_t o = row[m] + c.i;
			for (int t = 0; t < 9; ++t) R[9 * o + t] = Rm[t];
			cell[o] = (float)(E[m] * a.inv_w);
		}
		const double e = wave_sum(c.have && c.sub == 0 ? E[m] : 0.);
		int deg = c.have && c.sub == 0 && !okt[m] ? 1 : 0;
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o, 64);
		if (lane == 0) { sm_e[wave][m] = e; sm_d[wave][m] = deg; }
	}
	__syncthreads();
	if (threadIdx.x < TILE && m0 + (int)threadIdx.x < a.n) {
		double e = sm_e[0][threadIdx.x];
		int deg = sm_d[0][threadIdx.x];
#pragma unroll
		for (int wv = 1; wv < WAVES; ++wv) { e += sm_e[wv][threadIdx.x]; deg += sm_d[wv][threadIdx.x]; }
		const int64_t o = (int64_t)(m0 + threadIdx.x) * gridDim.x + blockIdx.x;
		part_e[o] = e;
		part_deg[o] = deg;
	}
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const double* __restrict__ part_e, const int32_t* __restrict__ part_deg, int blocks, double inv_w,
														  float* __restrict__ energy, int32_t* __restrict__ degenerate) {
	__shared__ double sm_e[WAVES];
	__shared__ int sm_d[WAVES];
	const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	double e = 0.;
	int deg = 0;
	for (int b = threadIdx.x; b < blocks; b += THREADS) { e += part_e[(int64_t)n * blocks + b]; deg += part_deg[(int64_t)n * blocks + b]; }
	e = wave_sum(e);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o, 64);
	if (lane == 0) { sm_e[wave] = e; sm_d[wave] = deg; }
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int wv = 1; wv < WAVES; ++wv) { e += sm_e[wv]; deg += sm_d[wv]; }
		energy[n] = (float)(e * inv_w);
		degenerate[n] = deg;
	}
}

__global__ __launch_bounds__(THREADS) void grad_kernel(const Mesh a, const double* __restrict__ R, const float* __restrict__ g, float* __restrict__ d_p) {
	constexpr int LANES = BWD_LANES;
	const Cell c = cell_of<LANES>(a);
	const int m0 = blockIdx.y * TILE;
	int64_t row[TILE];
	double pi[TILE][3], A[TILE][3], C[TILE][3], B[3] = {0., 0., 0.};   // sum w e_p, sum w R_j e_q, sum w e_q
#pragma unroll
	for (int m = 0; m < TILE; ++m) {
		row[m] = (int64_t)min(m0 + m, a.n - 1) * a.v;
		for (int k = 0; k < 3; ++k) { pi[m][k] = (double)a.p[3 * (row[m] + c.i) + k]; A[m][k] = 0.; C[m][k] = 0.; }
	}
	for (int k = c.begin; k < c.end; k += LANES) {
		const int j = a.idx[k];
		if ((unsigned)j >= (unsigned)a.v) continue;
		const double w = (double)a.w[k];
		double eq[3];
		for (int t = 0; t < 3; ++t) { eq[t] = c.q[t] - (double)a.q[3 * (int64_t)j + t]; B[t] += w * eq[t]; }
#pragma unroll
		for (int m = 0; m < TILE; ++m) {
			double Rj[9], r[3];
			for (int t = 0; t < 9; ++t) Rj[t] = R[9 * (row[m] + j) + t];
			rotate(Rj, eq, r);
			for (int t = 0; t < 3; ++t) {
				A[m][t] += w * (pi[m][t] - (double)a.p[3 * (row[m] + j) + t]);
				C[m][t] += w * r[t];
			}
		}
	}
#pragma unroll
	for (int t = 0; t < 3; ++t) B[t] = vertex_sum<LANES>(B[t]);
#pragma unroll
	for (int m = 0; m < TILE; ++m) {
#pragma unroll
		for (int t = 0; t < 3; ++t) { A[m][t] = vertex_sum<LANES>(A[m][t]); C[m][t] = vertex_sum<LANES>(C[m][t]); }
		if (c.have && c.sub == m && m0 + m < a.n) {
			const int64_t o = row[m] + c.i;
			double Ri[9], r[3];
			for (int t = 0; t < 9; ++t) Ri[t] = R[9 * o + t];
			rotate(Ri, B, r);
			const double s = 2. * a.inv_w * (double)g[m0 + m];
			for (int t = 0; t < 3; ++t) d_p[3 * o + t] = (float)(s * (2. * A[m][t] - r[t] - C[m][t]));
		}
	}
}

static bool sizes_ok(int64_t n, int64_t v, int64_t n_nbr) {
	return n >= 1 && n < 65536 && v >= 1 && v < (1ll << 24) && n * v < (1ll << 31) && n_nbr >= 0 && n_nbr < (1ll << 31);
}
static int64_t blocks_of(int64_t v, int lanes) { return cdiv(v, THREADS / lanes); }

struct Ws {
	double* part_e;
	int32_t* part_deg;
	int64_t bytes;
};
static void carve(int64_t n, int64_t v, void* ws, Ws* o) {
	Carver c(ws);
	o->part_e = c.take<double>(n * blocks_of(v, FWD_LANES));
	o->part_deg = c.take<int32_t>(n * blocks_of(v, FWD_LANES));
	o->bytes = c.off;
}

static Mesh mesh_of(const float* verts, const float* rest, const int32_t* nbr_off, const int32_t* nbr_idx, const float* nbr_w, int64_t n, int64_t v,
					int64_t n_nbr, double w_sum) {
	Mesh a;
	a.p = verts; a.q = rest; a.off = nbr_off; a.idx = nbr_idx; a.w = nbr_w; a.n = (int)n; a.v = (int)v; a.n_nbr = (int)n_nbr;
	a.inv_w = w_sum > 0. ? 1. / w_sum : 0.;
	return a;
}

}  // namespace arap
}  // namespace find

using namespace find;

extern "C" int64_t find_arap_ws_bytes(int64_t n, int64_t v) {
	if (!arap::sizes_ok(n, v, 0)) {
		set_error("find_arap_ws_bytes: bad sizes n=%lld v=%lld", (long long)n, (long long)v);
		return -1;
	}
	arap::Ws w;
	arap::carve(n, v, nullptr, &w);
	return w.bytes;
}

extern "C" int find_arap_fwd(const float* verts, const float* rest, const int32_t* nbr_off, const int32_t* nbr_idx, const float* nbr_w, int64_t n, int64_t v,
							 int64_t n_nbr, double w_sum, double* R, float* cell, float* energy, int32_t* degenerate, void* ws, int64_t ws_bytes,
							 void* stream) {
	FIND_REQUIRE(verts && rest && nbr_off && R && cell && energy && degenerate && (n_nbr == 0 || (nbr_idx && nbr_w)), "find_arap_fwd: NULL argument");
	FIND_REQUIRE(arap::sizes_ok(n, v, n_nbr), "find_arap_fwd: bad sizes n=%lld v=%lld n_nbr=%lld", (long long)n, (long long)v, (long long)n_nbr);
	FIND_REQUIRE(w_sum >= 0. && w_sum < INFINITY, "find_arap_fwd: the weight sum must be finite and >= 0, got %g", w_sum);
	arap::Ws k;
	arap::carve(n, v, ws, &k);
	if (!ws || ws_bytes < k.bytes || (reinterpret_cast<uintptr_t>(ws) & 7)) {
		set_error("find_arap_fwd: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)ws_bytes, (long long)k.bytes);
		return FIND_EWORKSPACE;
	}
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const arap::Mesh a = arap::mesh_of(verts, rest, nbr_off, nbr_idx, nbr_w, n, v, n_nbr, w_sum);
	const int64_t blocks = arap::blocks_of(v, arap::FWD_LANES);
	hipLaunchKernelGGL(arap::cells_kernel, dim3((unsigned)blocks, (unsigned)cdiv(n, arap::TILE)), dim3(arap::THREADS), 0, st, a, R, cell, k.part_e, k.part_deg);
	FIND_LAUNCH_CHECK("arap cells_kernel");
	hipLaunchKernelGGL(arap::finish_kernel, dim3((unsigned)n), dim3(arap::THREADS), 0, st, (const double*)k.part_e, (const int32_t*)k.part_deg, (int)blocks,
					   a.inv_w, energy, degenerate);
	FIND_LAUNCH_CHECK("arap finish_kernel");
	return FIND_OK;
}

extern "C" int find_arap_bwd(const float* verts, const float* rest, const int32_t* nbr_off, const int32_t* nbr_idx, const float* nbr_w, int64_t n, int64_t v,
							 int64_t n_nbr, double w_sum, const double* R, const float* g, float* d_verts, void* stream) {
	FIND_REQUIRE(verts && rest && nbr_off && R && g && d_verts && (n_nbr == 0 || (nbr_idx && nbr_w)), "find_arap_bwd: NULL argument");
	FIND_REQUIRE(arap::sizes_ok(n, v, n_nbr), "find_arap_bwd: bad sizes n=%lld v=%lld n_nbr=%lld", (long long)n, (long long)v, (long long)n_nbr);
	FIND_REQUIRE(w_sum >= 0. && w_sum < INFINITY, "find_arap_bwd: the weight sum must be finite and >= 0, got %g", w_sum);
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const arap::Mesh a = arap::mesh_of(verts, rest, nbr_off, nbr_idx, nbr_w, n, v, n_nbr, w_sum);
	hipLaunchKernelGGL(arap::grad_kernel, dim3((unsigned)arap::blocks_of(v, arap::BWD_LANES), (unsigned)cdiv(n, arap::TILE)), dim3(arap::THREADS), 0, st, a, R, g, d_verts);
	FIND_LAUNCH_CHECK("arap grad_kernel");
	return FIND_OK;
}
