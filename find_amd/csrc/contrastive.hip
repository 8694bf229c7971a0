// Contrastive pose loss and its gradient (reference src/model/losses.py:305-333, ContrastiveLoss; applied in ModelWithLoss.forward,
// src/model/model.py:1042-1049).  The reference loops over the drawn pairs in Python, eight small torch ops per pair, and its hinge
// -- Python's max() on a device tensor -- reads every pair's distance on the host.  Here the pairs arrive as a device int32 (P, 2)
// table (drawn on the host by find_amd.losses.draw_pairs, numpy's generator as upstream) and the whole loss is one launch each way.
//   per pair p = (a, b):  y = <code_a, code_b>,  d2 = ||v_a - v_b||^2,  L_p = y d2 + (1 - y) max(margin - d2, 0)^2
//   loss = sum_p L_p / P  (pair order);  coef_p = dL_p/d(d2) / P  is kept for the backward
//   d v_r = g * sum_{p : a_p = r} 2 coef_p (v_a - v_b)  -  g * sum_{p : b_p = r} 2 coef_p (v_a - v_b)     (pair order, no atomics)
// At d = 0 the gradient is 2 coef (v_a - v_b) = 0, as torch's norm backward gives.  Sums of squares, codes products and the per-pair
// combination run in double, the loss is rounded to fp32 once.  A pair index outside [0, N) gives NaN (loss and every gradient
// entry), following find_latent_gather_fwd: loud downstream, no fault and no host synchronisation here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "find_hip.h"
#include "common.h"

namespace find {
namespace contrastive {

constexpr int FWD_THREADS = 256;              // 4 waves; wave w takes pairs w, w + 4, ... of a chunk
constexpr int FWD_WAVES = FWD_THREADS / 64;
constexpr int CHUNK = 256;                    // pairs whose terms sit in LDS at a time (summed in pair order by one thread)
constexpr int PAIR_TILE = 256;                // pairs staged in LDS per step of the backward

__device__ inline double wave_sum(double v) {
	// fixed butterfly: every lane ends with the same value, the same on every run
	for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

__global__ __launch_bounds__(FWD_THREADS) void fwd_kernel(const float* __restrict__ vecs, int N, int K, const float* __restrict__ codes, int C,
														  const int32_t* __restrict__ pairs, int P, double margin, float* __restrict__ loss_out,
														  float* __restrict__ coef) {
	__shared__ double term[CHUNK];
	const int lane = threadIdx.x & 63;
	const int wave = threadIdx.x >> 6;
	const double inv_p = 1.0 / (double)P;
	double total = 0.0;   // (thread 0 only)
	for (int p0 = 0; p0 < P; p0 += CHUNK) {
		const int np = min(CHUNK, P - p0);
		for (int q = wave; q < np; q += FWD_WAVES) {
			const int p = p0 + q;
			const int a = pairs[2 * p], b = pairs[2 * p + 1];
			if (a < 0 || a >= N || b < 0 || b >= N) {   // (wave-uniform)
				if (lane == 0) {
					term[q] = __builtin_nan("");
					coef[p] = __builtin_nanf("");
				}
				continue;
			}
			const float* va = vecs + (int64_t)a * K;
			const float* vb = vecs + (int64_t)b * K;
			double s = 0.0;
			for (int k = lane; k < K; k += 64) {
				const double d = (double)va[k] - (double)vb[k];
				s += d * d;
			}
			const float* ca = codes + (int64_t)a * C;
			const float* cb = codes + (int64_t)b * C;
			double y = 0.0;
			for (int c = lane; c < C; c += 64) y += (double)ca[c] * (double)cb[c];
			const double d2 = wave_sum(s);
			y = wave_sum(y);
			if (lane == 0) {
				const double h = fmax(margin - d2, 0.0);
				term[q] = y * d2 + (1.0 - y) * h * h;
				coef[p] = (float)((y - 2.0 * (1.0 - y) * h) * inv_p);
			}
		}
		__syncthreads();
		if (threadIdx.x == 0)
			for (int q = 0; q < np; ++q) total += term[q];
		__syncthreads();
	}
	if (threadIdx.x == 0) *loss_out = (float)(total * inv_p);
}

__global__ __launch_bounds__(256) void bwd_kernel(const float* __restrict__ vecs, int N, int K, const int32_t* __restrict__ pairs, int P,
												  const float* __restrict__ coef, const float* __restrict__ d_loss, float* __restrict__ d_vecs) {
	__shared__ int32_t sa[PAIR_TILE], sb[PAIR_TILE];
	__shared__ float sc[PAIR_TILE];
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = e < (int64_t)N * K;
	const int r = live ? (int)(e / K) : -1;
	const int j = live ? (int)(e - (int64_t)r * K) : 0;
	float acc = 0.f;
	for (int p0 = 0; p0 < P; p0 += PAIR_TILE) {
		const int np = min(PAIR_TILE, P - p0);
		__syncthreads();
		if ((int)threadIdx.x < np) {
			sa[threadIdx.x] = pairs[2 * (p0 + threadIdx.x)];
			sb[threadIdx.x] = pairs[2 * (p0 + threadIdx.x) + 1];
			sc[threadIdx.x] = coef[p0 + threadIdx.x];
		}
		__syncthreads();
		if (!live) continue;
		for (int q = 0; q < np; ++q) {
			const int a = sa[q], b = sb[q];
			if (a < 0 || a >= N || b < 0 || b >= N) {   // never read the row of an invalid index; the gradient goes NaN
				acc += __builtin_nanf("");
				continue;
			}
			if (r != a && r != b) continue;
			const float g = 2.f * sc[q] * (vecs[(int64_t)a * K + j] - vecs[(int64_t)b * K + j]);
			acc += (r == a) ? g : -g;   // (a == b: d = 0, g = 0 either way)
		}
	}
	if (live) d_vecs[e] = acc * *d_loss;
}

}  // namespace contrastive
}  // namespace find

using namespace find;

extern "C" int find_contrastive_fwd(const float* vecs, int64_t N, int64_t K, const float* codes, int64_t C, const int32_t* pairs, int64_t P,
									float margin, float* loss_out, float* coef_ws, void* stream) {
	FIND_REQUIRE(vecs && codes && pairs && loss_out && coef_ws, "find_contrastive_fwd: NULL argument");
	FIND_REQUIRE(N >= 2 && N < (1 << 24) && K >= 1 && K < (1 << 24) && C >= 1 && C < (1 << 24), "find_contrastive_fwd: bad sizes N=%lld K=%lld C=%lld",
				 (long long)N, (long long)K, (long long)C);
	FIND_REQUIRE(P >= 1 && P <= N * (N - 1) && P < (1 << 30), "find_contrastive_fwd: %lld pairs for %lld rows (1 .. N(N-1))", (long long)P, (long long)N);
	hipLaunchKernelGGL(contrastive::fwd_kernel, dim3(1), dim3(contrastive::FWD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), vecs, (int)N,
					   (int)K, codes, (int)C, pairs, (int)P, (double)margin, loss_out, coef_ws);
	FIND_LAUNCH_CHECK("contrastive fwd_kernel");
	return FIND_OK;
}

extern "C" int find_contrastive_bwd(const float* vecs, int64_t N, int64_t K, const int32_t* pairs, int64_t P, const float* coef_ws,
									const float* d_loss, float* d_vecs, void* stream) {
	FIND_REQUIRE(vecs && pairs && coef_ws && d_loss && d_vecs, "find_contrastive_bwd: NULL argument");
	FIND_REQUIRE(N >= 2 && N < (1 << 24) && K >= 1 && K < (1 << 24) && N * K < ((int64_t)1 << 31), "find_contrastive_bwd: bad sizes N=%lld K=%lld",
				 (long long)N, (long long)K);
	FIND_REQUIRE(P >= 1 && P <= N * (N - 1) && P < (1 << 30), "find_contrastive_bwd: %lld pairs for %lld rows (1 .. N(N-1))", (long long)P, (long long)N);
	const int64_t total = N * K;
	hipLaunchKernelGGL(contrastive::bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), vecs,
					   (int)N, (int)K, pairs, (int)P, coef_ws, d_loss, d_vecs);
	FIND_LAUNCH_CHECK("contrastive bwd_kernel");
	return FIND_OK;
}
