// Rigid and similarity alignment of point clouds: Umeyama / Kabsch on given pairs (find_align_fit) and trimmed ICP as one call
// (find_icp_run).  Not in the reference; stands in for pytorch3d.ops.corresponding_points_alignment / iterative_closest_point.
// Row vectors: x' = s (x @ R) + t.
//   icp_init_kernel     a thread per cloud: the transform (the caller's or identity), the counters and the loop's state.
//   apply_kernel        a thread per point: xt = fmaf(s, fmaf(x2, R2j, fmaf(x1, R1j, x0 * R0j)), tj) in fp32; rows past x_len get zeros.
//   (match)             find_nn_fwd, the library's own search, on xt and y.
//   select_kernel       a workgroup per cloud: tau = the k-th smallest d2 of the cloud's valid queries, k = m - floor(trim m), by a radix
//                       select over the bit patterns of the non-negative floats: four digits of eight bits, integer histograms in LDS.
//   moments_kernel      a workgroup per 256 pairs and cloud: the N_MOMENTS sums of align_math.h in double about the pivots (the cloud's
//                       first x and first y), lanes by xor-butterfly, waves in wave order.
//   solve_kernel        a thread per cloud: the partials in workgroup order, the solve of align_math.h, and for ICP the loop's rule.
// No float atomics; every sum in double in a fixed order: two runs agree bit for bit, and a cloud's row does not depend on the batch
// (a workgroup past a cloud's end adds zeros).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"
#include "align_math.h"

namespace find {
namespace align {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

struct Pairs {
	const float* x;         // (n, p_max, 3)
	const int32_t* x_len;   // (n) or NULL
	const float* y;         // fit: (n, p_max, 3) paired by row; ICP: (n, p2_max, 3) through idx
	const int32_t* y_len;   // ICP: (n) or NULL
	const float* w;         // fit: (n, p_max) or NULL
	const float* dist;      // ICP: (n, p_max) d2 of the match
	const int32_t* idx;     // ICP: (n, p_max) or NULL (= fit)
	const float* tau;       // ICP: (n)
	float max_d2;
	int p_max, p2_max;
};

struct State {   // of the ICP loop, per cloud, in the workspace
	double* prev_rmse;
	int32_t* frozen;
};

// a pivot only shifts the sums: a row 0 that is not finite (it can carry weight 0) gives 0
__device__ __forceinline__ double pivot(const float* p, int k) { return isfinite(p[k]) ? (double)p[k] : 0.; }
__device__ __forceinline__ int valid_len(const int32_t* len, int n, int p_max) { return len ? min(max(len[n], 0), p_max) : p_max; }

__global__ __launch_bounds__(64) void icp_init_kernel(int n, const float* init_R, const float* init_t, const float* init_s, float* R, float* t, float* s,
													  float* rmse, int32_t* iterations, int32_t* status, float* tau, int32_t* used, State st) {
	const int c = blockIdx.x * 64 + threadIdx.x;
	if (c >= n) return;
	for (int i = 0; i < 9; ++i) R[9 * c + i] = init_R ? init_R[9 * c + i] : (i % 4 == 0 ? 1.f : 0.f);
	for (int i = 0; i < 3; ++i) t[3 * c + i] = init_t ? init_t[3 * c + i] : 0.f;
	s[c] = init_s ? init_s[c] : 1.f;
	rmse[c] = 0.f; iterations[c] = 0; status[c] = 0; tau[c] = INFINITY; used[c] = 0;   // (tau: +inf unless select_kernel runs)
	st.prev_rmse[c] = 0.; st.frozen[c] = 0;
}

__global__ __launch_bounds__(THREADS) void apply_kernel(const float* __restrict__ x, const int32_t* x_len, int p_max, const float* __restrict__ R,
														const float* __restrict__ t, const float* __restrict__ s, float* __restrict__ xt) {
	const int c = blockIdx.y, i = blockIdx.x * THREADS + threadIdx.x;
	if (i >= p_max) return;
	const int64_t o = ((int64_t)c * p_max + i) * 3;
	if (i >= valid_len(x_len, c, p_max)) { xt[o] = 0.f; xt[o + 1] = 0.f; xt[o + 2] = 0.f; return; }
	const float* Rc = R + 9 * c;
	const float x0 = x[o], x1 = x[o + 1], x2 = x[o + 2], sc = s[c];
#pragma unroll
	for (int j = 0; j < 3; ++j) xt[o + j] = fmaf(sc, fmaf(x2, Rc[6 + j], fmaf(x1, Rc[3 + j], x0 * Rc[j])), t[3 * c + j]);
}

__global__ __launch_bounds__(THREADS) void select_kernel(const float* __restrict__ dist, const int32_t* x_len, int p_max, double trim, float* tau) {
	__shared__ int hist[256];
	__shared__ unsigned s_prefix;
	__shared__ int s_k;
	const int c = blockIdx.x, tid = threadIdx.x;
	const int m = valid_len(x_len, c, p_max);
	if (m == 0) { if (tid == 0) tau[c] = INFINITY; return; }
	const float* d = dist + (int64_t)c * p_max;
	if (tid == 0) { s_prefix = 0u; s_k = keep_count(m, trim); }
	for (int shift = 24; shift >= 0; shift -= 8) {
		hist[tid] = 0;
		__syncthreads();
		const unsigned prefix = s_prefix, mask = shift == 24 ? 0u : ~0u << (shift + 8);
		for (int i = tid; i < m; i += THREADS) {
			const unsigned b = __float_as_uint(d[i]);
			if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1);
		}
		__syncthreads();
		if (tid == 0) {
			int k = s_k;
			const int bin = select_bin(hist, &k);
			s_k = k; s_prefix = prefix | ((unsigned)bin << shift);
		}
		__syncthreads();
	}
	if (tid == 0) tau[c] = __uint_as_float(s_prefix);
}

__global__ __launch_bounds__(THREADS) void moments_kernel(const Pairs a, double* __restrict__ part) {
	__shared__ double sm[WAVES][N_MOMENTS];
	const int c = blockIdx.y, i = blockIdx.x * THREADS + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int m = valid_len(a.x_len, c, a.p_max);
	double v[N_MOMENTS];
#pragma unroll
	for (int k = 0; k < N_MOMENTS; ++k) v[k] = 0.;
	if (i < m) {
		const int64_t o = (int64_t)c * a.p_max + i;
		double w = 0., d2 = 0.;
		int64_t yo = -1, y0 = 0;
		if (a.idx) {
			const int j = a.idx[o];
			const float d = a.dist[o];
			if (j >= 0 && j < valid_len(a.y_len, c, a.p2_max) && d <= a.tau[c] && d <= a.max_d2) { w = 1.; d2 = (double)d; }
			yo = ((int64_t)c * a.p2_max + j) * 3; y0 = (int64_t)c * a.p2_max * 3;
		} else {
			const float wf = a.w ? a.w[o] : 1.f;
			if (wf > 0.f && wf < INFINITY) w = (double)wf;
			yo = o * 3; y0 = (int64_t)c * a.p_max * 3;
		}
		if (w > 0.) {   // (a pair of weight 0 is never read: its row may hold anything)
			const float* xp = a.x + o * 3;
			const float* x0 = a.x + (int64_t)c * a.p_max * 3;
			double dx[3], dy[3];
#pragma unroll
			for (int k = 0; k < 3; ++k) { dx[k] = (double)xp[k] - pivot(x0, k); dy[k] = (double)a.y[yo + k] - pivot(a.y + y0, k); }
			v[M_W] = w; v[M_CNT] = 1.; v[M_D2] = w * d2;
			v[M_XX] = w * (dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				v[M_X + k] = w * dx[k]; v[M_Y + k] = w * dy[k];
#pragma unroll
				for (int l = 0; l < 3; ++l) v[M_XY + 3 * k + l] = w * dx[k] * dy[l];
			}
		}
	}
#pragma unroll
	for (int k = 0; k < N_MOMENTS; ++k) {
		const double r = wave_sum(v[k]);
		if (lane == 0) sm[wave][k] = r;
	}
	__syncthreads();
	if (threadIdx.x < N_MOMENTS) {
		double r = sm[0][threadIdx.x];
#pragma unroll
		for (int wv = 1; wv < WAVES; ++wv) r += sm[wv][threadIdx.x];
		part[((int64_t)c * gridDim.x + blockIdx.x) * N_MOMENTS + threadIdx.x] = r;
	}
}

struct Solve {
	const double* part;
	int blocks, n;
	const float* x;   // the pivots: row 0 of each cloud
	const float* y;
	int64_t x_stride, y_stride;
	int estimate_scale, allow_reflection;
	float *R, *t, *s;
	int32_t* status;
	// ICP only (rmse != NULL)
	float* rmse;
	int32_t *iterations, *used;
	State st;
	int round, last;
	double rel_tol;
};

__global__ __launch_bounds__(64) void solve_kernel(const Solve a) {
	const int c = blockIdx.x * 64 + threadIdx.x;
	if (c >= a.n) return;
	double m[N_MOMENTS];
	for (int k = 0; k < N_MOMENTS; ++k) m[k] = 0.;
	for (int b = 0; b < a.blocks; ++b)
		for (int k = 0; k < N_MOMENTS; ++k) m[k] += a.part[((int64_t)c * a.blocks + b) * N_MOMENTS + k];
	const bool icp = a.rmse != nullptr;
	if (icp) {
		const double r = m[M_W] > 0. ? sqrt(m[M_D2] / m[M_W]) : 0.;
		a.rmse[c] = (float)r;
		a.used[c] = (int32_t)m[M_CNT];
		if (a.st.frozen[c]) return;
		if (a.round > 0 && fabs(a.st.prev_rmse[c] - r) <= a.rel_tol * a.st.prev_rmse[c]) { a.st.frozen[c] = 1; return; }
		if (a.last) { a.status[c] |= STATUS_MAX_ITERATIONS; return; }
		a.st.prev_rmse[c] = r;
	}
	double R[9], t[3], s = 1.;
	bool ok = m[M_CNT] >= 3.;
	if (ok) {   // (the pivots of a cloud without three pairs may be padding)
		const float* xp = a.x + c * a.x_stride;
		const float* yp = a.y + c * a.y_stride;
		const double px[3] = {pivot(xp, 0), pivot(xp, 1), pivot(xp, 2)}, py[3] = {pivot(yp, 0), pivot(yp, 1), pivot(yp, 2)};
		ok = solve(m, px, py, a.estimate_scale != 0, a.allow_reflection != 0, R, t, &s);
	}
	if (!ok) {
		if (icp) {
			a.st.frozen[c] = 1; a.status[c] |= STATUS_DEGENERATE;
		} else {
			for (int i = 0; i < 9; ++i) a.R[9 * c + i] = i % 4 == 0 ? 1.f : 0.f;
			for (int i = 0; i < 3; ++i) a.t[3 * c + i] = 0.f;
			a.s[c] = 1.f; a.status[c] = STATUS_DEGENERATE;
		}
		return;
	}
	for (int i = 0; i < 9; ++i) a.R[9 * c + i] = (float)R[i];
	for (int i = 0; i < 3; ++i) a.t[3 * c + i] = (float)t[i];
	a.s[c] = (float)s;
	if (icp) a.iterations[c] = a.round + 1;
	else a.status[c] = 0;
}

static bool sizes_ok(int64_t n, int64_t p_max) { return n >= 1 && n < 65536 && p_max >= 1 && p_max < (1ll << 24) && n * p_max < (1ll << 31); }
static int64_t blocks_of(int64_t p_max) { return cdiv(p_max, THREADS); }

struct IcpWs {
	double* part;
	State st;
	int64_t bytes;
};
static void carve(int64_t n, int64_t p_max, bool icp, void* ws, IcpWs* o) {
	Carver c(ws);
	o->part = c.take<double>(n * blocks_of(p_max) * N_MOMENTS);
	if (icp) {
		o->st.prev_rmse = c.take<double>(n);
		o->st.frozen = c.take<int32_t>(n);
	}
	o->bytes = c.off;
}

static int ws_ok(const char* who, const void* ws, int64_t ws_bytes, int64_t need) {
	if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7)) {
		set_error("%s: workspace of %lld bytes, %lld needed (8-byte aligned)", who, (long long)ws_bytes, (long long)need);
		return FIND_EWORKSPACE;
	}
	return FIND_OK;
}

}  // namespace align
}  // namespace find

using namespace find;

extern "C" int64_t find_align_ws_bytes(int64_t n, int64_t p_max) {
	if (!align::sizes_ok(n, p_max)) {
		set_error("find_align_ws_bytes: bad sizes n=%lld p_max=%lld", (long long)n, (long long)p_max);
		return -1;
	}
	align::IcpWs w;
	align::carve(n, p_max, false, nullptr, &w);
	return w.bytes;
}

extern "C" int64_t find_icp_ws_bytes(int64_t n, int64_t p1_max, int64_t p2_max) {
	if (!align::sizes_ok(n, p1_max) || !align::sizes_ok(n, p2_max)) {
		set_error("find_icp_ws_bytes: bad sizes n=%lld p1_max=%lld p2_max=%lld", (long long)n, (long long)p1_max, (long long)p2_max);
		return -1;
	}
	align::IcpWs w;
	align::carve(n, p1_max, true, nullptr, &w);
	return w.bytes;
}

extern "C" int find_align_fit(const float* x, const float* y, const int32_t* len, const float* w, int64_t n, int64_t p_max, int estimate_scale,
							  int allow_reflection, float* R, float* t, float* s, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(x && y && R && t && s && status, "find_align_fit: NULL argument");
	FIND_REQUIRE(align::sizes_ok(n, p_max), "find_align_fit: bad sizes n=%lld p_max=%lld", (long long)n, (long long)p_max);
	align::IcpWs k;
	align::carve(n, p_max, false, ws, &k);
	int rc = align::ws_ok("find_align_fit", ws, ws_bytes, k.bytes);
	if (rc != FIND_OK) return rc;
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = align::blocks_of(p_max);
	align::Pairs p = {};
	p.x = x; p.x_len = len; p.y = y; p.w = w; p.p_max = (int)p_max; p.p2_max = (int)p_max; p.max_d2 = INFINITY;
	hipLaunchKernelGGL(align::moments_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(align::THREADS), 0, st, p, k.part);
	FIND_LAUNCH_CHECK("align moments_kernel");
	align::Solve a = {};
	a.part = k.part; a.blocks = (int)blocks; a.n = (int)n; a.x = x; a.y = y; a.x_stride = p_max * 3; a.y_stride = p_max * 3;
	a.estimate_scale = estimate_scale; a.allow_reflection = allow_reflection; a.R = R; a.t = t; a.s = s; a.status = status;
	hipLaunchKernelGGL(align::solve_kernel, dim3((unsigned)cdiv(n, 64)), dim3(64), 0, st, a);
	FIND_LAUNCH_CHECK("align solve_kernel");
	return FIND_OK;
}

extern "C" int find_icp_run(const float* x, const int32_t* x_len, const float* y, const int32_t* y_len, int64_t n, int64_t p1_max, int64_t p2_max,
							const float* init_R, const float* init_t, const float* init_s, int64_t max_iterations, double rel_tol, int estimate_scale,
							double trim, float max_dist, float* R, float* t, float* s, float* rmse, int32_t* iterations, int32_t* status, float* xt,
							float* dist, int32_t* idx, float* tau, int32_t* used, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(x && y && R && t && s && rmse && iterations && status && xt && dist && idx && tau && used, "find_icp_run: NULL argument");
	FIND_REQUIRE((init_R && init_t && init_s) || (!init_R && !init_t && !init_s), "find_icp_run: init_R, init_t, init_s: all three or none");
	FIND_REQUIRE(align::sizes_ok(n, p1_max) && align::sizes_ok(n, p2_max), "find_icp_run: bad sizes n=%lld p1_max=%lld p2_max=%lld", (long long)n,
				 (long long)p1_max, (long long)p2_max);
	FIND_REQUIRE(max_iterations >= 0 && max_iterations <= 10000 && rel_tol >= 0. && trim >= 0. && trim < 1. && max_dist > 0.f,
				 "find_icp_run: max_iterations in [0, 10000], rel_tol >= 0, trim in [0, 1), max_dist > 0 (INFINITY: none) expected, got %lld, %g, %g, %g",
				 (long long)max_iterations, rel_tol, trim, (double)max_dist);
	align::IcpWs k;
	align::carve(n, p1_max, true, ws, &k);
	int rc = align::ws_ok("find_icp_run", ws, ws_bytes, k.bytes);
	if (rc != FIND_OK) return rc;
	hipStream_t st = reinterpret_cast<hipStream_t>(stream);
	const int64_t blocks = align::blocks_of(p1_max);
	const dim3 cloud_grid((unsigned)cdiv(n, 64));
	hipLaunchKernelGGL(align::icp_init_kernel, cloud_grid, dim3(64), 0, st, (int)n, init_R, init_t, init_s, R, t, s, rmse, iterations, status, tau, used, k.st);
	FIND_LAUNCH_CHECK("align icp_init_kernel");
	align::Pairs p = {};
	p.x = x; p.x_len = x_len; p.y = y; p.y_len = y_len; p.dist = dist; p.idx = idx; p.tau = tau; p.p_max = (int)p1_max; p.p2_max = (int)p2_max;
	p.max_d2 = max_dist * max_dist;
	align::Solve a = {};
	a.part = k.part; a.blocks = (int)blocks; a.n = (int)n; a.x = x; a.y = y; a.x_stride = p1_max * 3; a.y_stride = p2_max * 3;
	a.estimate_scale = estimate_scale; a.R = R; a.t = t; a.s = s; a.status = status; a.rmse = rmse; a.iterations = iterations; a.used = used; a.st = k.st;
	a.rel_tol = rel_tol;
	// max_iterations updates, then one more apply + match + sums: what is returned belongs to the returned transform
	for (int64_t round = 0; round <= max_iterations; ++round) {
		hipLaunchKernelGGL(align::apply_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(align::THREADS), 0, st, x, x_len, (int)p1_max, (const float*)R,
						   (const float*)t, (const float*)s, xt);
		FIND_LAUNCH_CHECK("align apply_kernel");
		rc = find_nn_fwd(xt, x_len, y, y_len, n, p1_max, p2_max, dist, idx, stream);
		if (rc != FIND_OK) return rc;
		if (trim > 0.) {
			hipLaunchKernelGGL(align::select_kernel, dim3((unsigned)n), dim3(align::THREADS), 0, st, (const float*)dist, x_len, (int)p1_max, trim, tau);
			FIND_LAUNCH_CHECK("align select_kernel");
		}
		hipLaunchKernelGGL(align::moments_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(align::THREADS), 0, st, p, k.part);
		FIND_LAUNCH_CHECK("align moments_kernel");
		a.round = (int)round; a.last = round == max_iterations;
		hipLaunchKernelGGL(align::solve_kernel, cloud_grid, dim3(64), 0, st, a);
		FIND_LAUNCH_CHECK("align solve_kernel");
	}
	return FIND_OK;
}
