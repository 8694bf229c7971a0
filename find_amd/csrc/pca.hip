// Linear PCA foot model (reference src/model/model.py:581, PCAModel.get_meshes):
//   offsets[n,v,c] = sum_b coefs[v,b,c] * shapevec[n,b]                      (find_pca_fwd)
//   d_shapevec[n,b] = sum_{v,c} d_offsets[n,v,c] * coefs[v,b,c]              (find_pca_bwd)
// coefs is read in its state_dict layout (V, B, 3): the 3B floats of a vertex row are contiguous.  A block owns a tile of TV vertex rows
// -- one contiguous run of TV * 3B floats in global memory -- stages it through LDS once with coalesced loads and serves every foot from
// there, so the coefficients cross HBM once per call whatever n_feet is.  In LDS a row is padded to a stride P = 3 (mod 32) floats: output
// element e = 3v + c of a tile then reads bank (3v + c + 3b) % 32 = (e + 3b) % 32, consecutive lanes on consecutive banks.
#include "common.h"

namespace find {
namespace pca {

constexpr int THREADS = 256;
constexpr int TILE_FLOATS = 12288;  // coefficient tile: 48 KiB of LDS
constexpr int FEET_FLOATS = 4096;   // shapevec rows (fwd) / d_offsets rows (bwd) of a chunk of feet: 16 KiB
constexpr int MAX_B = 4000;         // one padded row (3B rounded up to 3 mod 32) must fit the tile
constexpr int MAX_TV = 64;

inline __host__ __device__ int row_stride(int B) { return 3 * B + ((3 - 3 * B) % 32 + 32) % 32; }

// vertices per block: as many rows as the tile holds (at most 64), but no more than it takes to give ~256 blocks; a function of (V, B) only
inline int tile_verts(int64_t V, int B) {
	const int cap = std::min(MAX_TV, TILE_FLOATS / row_stride(B));
	return (int)std::max<int64_t>(1, std::min<int64_t>(cap, cdiv(V, 256)));
}

// rows [v0, v0 + tv) of coefs -> tile[r * P + k]
__device__ __forceinline__ void stage_tile(const float* __restrict__ coefs, int64_t v0, int tv, int B, int P, float* tile) {
	const int row = 3 * B;
	const int n = tv * row;
	const float* src = coefs + v0 * row;
	for (int i = threadIdx.x; i < n; i += THREADS) {
		const int r = i / row;
		tile[r * P + (i - r * row)] = src[i];
	}
}

__global__ __launch_bounds__(THREADS) void pca_fwd_kernel(const float* __restrict__ coefs, int64_t V, int B, int TV,
														   const float* __restrict__ shapevec, int64_t n_feet, float* __restrict__ offsets) {
	__shared__ float tile[TILE_FLOATS];
	__shared__ float sv[FEET_FLOATS];
	const int P = row_stride(B);
	const int64_t v0 = (int64_t)blockIdx.x * TV;
	const int tv = (int)std::min<int64_t>(TV, V - v0);
	const int E = 3 * tv;   // output elements (v, c) of this tile per foot
	stage_tile(coefs, v0, tv, B, P, tile);
	const int NC = (int)std::min<int64_t>(n_feet, FEET_FLOATS / B);
	for (int64_t n0 = 0; n0 < n_feet; n0 += NC) {
		const int nc = (int)std::min<int64_t>(NC, n_feet - n0);
		__syncthreads();   // (the tile is complete / the previous chunk's rows are no longer read)
		for (int i = threadIdx.x; i < nc * B; i += THREADS) sv[i] = shapevec[n0 * B + i];
		__syncthreads();
		for (int i = threadIdx.x; i < nc * E; i += THREADS) {
			const int nl = i / E, e = i - nl * E;
			const int v = e / 3, c = e - 3 * v;
			const float* t = tile + v * P + c;
			const float* s = sv + nl * B;
			float acc = 0.f;
#pragma unroll 4
			for (int b = 0; b < B; ++b) acc = fmaf(t[3 * b], s[b], acc);
			offsets[((n0 + nl) * V + v0) * 3 + e] = acc;
		}
	}
}

// partial[blk][n][b] = sum over the tile's (v, c) of d_offsets[n, v0 + v, c] * coefs[v0 + v, b, c]
__global__ __launch_bounds__(THREADS) void pca_bwd_kernel(const float* __restrict__ coefs, int64_t V, int B, int TV,
														   const float* __restrict__ d_offsets, int64_t n_feet, float* __restrict__ partial) {
	__shared__ float tile[TILE_FLOATS];
	__shared__ float gt[FEET_FLOATS];
	const int P = row_stride(B);
	const int64_t v0 = (int64_t)blockIdx.x * TV;
	const int tv = (int)std::min<int64_t>(TV, V - v0);
	const int E = 3 * tv;
	stage_tile(coefs, v0, tv, B, P, tile);
	const int NC = (int)std::min<int64_t>(n_feet, FEET_FLOATS / (3 * MAX_TV));
	float* out = partial + (int64_t)blockIdx.x * n_feet * B;
	for (int64_t n0 = 0; n0 < n_feet; n0 += NC) {
		const int nc = (int)std::min<int64_t>(NC, n_feet - n0);
		__syncthreads();
		for (int i = threadIdx.x; i < nc * E; i += THREADS) {
			const int nl = i / E;
			gt[nl * E + (i - nl * E)] = d_offsets[((n0 + nl) * V + v0) * 3 + (i - nl * E)];
		}
		__syncthreads();
		for (int i = threadIdx.x; i < nc * B; i += THREADS) {
			const int nl = i / B, b = i - nl * B;
			const float* g = gt + nl * E;
			const float* t = tile + 3 * b;
			float acc = 0.f;
			for (int v = 0; v < tv; ++v) {
				acc = fmaf(g[3 * v + 0], t[v * P + 0], acc);
				acc = fmaf(g[3 * v + 1], t[v * P + 1], acc);
				acc = fmaf(g[3 * v + 2], t[v * P + 2], acc);
			}
			out[n0 * B + i] = acc;
		}
	}
}

// one thread per (n, b): the blocks' partials added in block order (no atomics: bit-identical from run to run)
__global__ __launch_bounds__(THREADS) void pca_bwd_finalize_kernel(const float* __restrict__ partial, int nblk, int64_t nb,
																	float* __restrict__ d_shapevec) {
	const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
	if (i >= nb) return;
	float s = 0.f;
	// (unrolled so that the loads of 16 partials are in flight together; the additions stay in block order)
#pragma unroll 16
	for (int k = 0; k < nblk; ++k) s += partial[(int64_t)k * nb + i];
	d_shapevec[i] = s;
}

inline bool bad_sizes(int64_t V, int64_t B, int64_t n_feet) {
	// (the last bound keeps the workspace size, nblk * n_feet * B floats with nblk <= V, far from overflow)
	return V < 1 || V >= (1ll << 29) || B < 1 || B > MAX_B || n_feet < 1 || n_feet > (1ll << 20) || V * n_feet * B > (1ll << 40);
}

}  // namespace pca
}  // namespace find

using namespace find;

extern "C" int find_pca_fwd(const float* coefs, int64_t V, int64_t B, const float* shapevec, int64_t n_feet, float* offsets, void* stream) {
	FIND_REQUIRE(coefs && shapevec && offsets, "find_pca_fwd: NULL argument");
	FIND_REQUIRE(!pca::bad_sizes(V, B, n_feet), "find_pca_fwd: bad sizes (V %lld, B %lld, n_feet %lld; 1 <= B <= %d)", (long long)V, (long long)B,
				 (long long)n_feet, pca::MAX_B);
	const int TV = pca::tile_verts(V, (int)B);
	hipLaunchKernelGGL(pca::pca_fwd_kernel, dim3((unsigned)cdiv(V, TV)), dim3(pca::THREADS), 0, (hipStream_t)stream, coefs, V, (int)B, TV, shapevec,
					   n_feet, offsets);
	FIND_LAUNCH_CHECK("pca_fwd_kernel");
	return FIND_OK;
}

extern "C" int64_t find_pca_bwd_ws_bytes(int64_t n_feet, int64_t V, int64_t B) {
	if (pca::bad_sizes(V, B, n_feet)) return -1;
	return align_up(cdiv(V, pca::tile_verts(V, (int)B)) * n_feet * B * (int64_t)sizeof(float), 256);
}

extern "C" int find_pca_bwd(const float* coefs, int64_t V, int64_t B, const float* d_offsets, int64_t n_feet, float* d_shapevec, void* ws,
							int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(coefs && d_offsets && d_shapevec && ws, "find_pca_bwd: NULL argument");
	FIND_REQUIRE(!pca::bad_sizes(V, B, n_feet), "find_pca_bwd: bad sizes (V %lld, B %lld, n_feet %lld; 1 <= B <= %d)", (long long)V, (long long)B,
				 (long long)n_feet, pca::MAX_B);
	if (ws_bytes < find_pca_bwd_ws_bytes(n_feet, V, B)) {
		set_error("find_pca_bwd: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)find_pca_bwd_ws_bytes(n_feet, V, B));
		return FIND_EWORKSPACE;
	}
	const int TV = pca::tile_verts(V, (int)B);
	const int nblk = (int)cdiv(V, TV);
	hipStream_t s = (hipStream_t)stream;
	float* partial = reinterpret_cast<float*>(ws);
	hipLaunchKernelGGL(pca::pca_bwd_kernel, dim3((unsigned)nblk), dim3(pca::THREADS), 0, s, coefs, V, (int)B, TV, d_offsets, n_feet, partial);
	FIND_LAUNCH_CHECK("pca_bwd_kernel");
	const int64_t nb = n_feet * B;
	hipLaunchKernelGGL(pca::pca_bwd_finalize_kernel, dim3((unsigned)cdiv(nb, pca::THREADS)), dim3(pca::THREADS), 0, s, (const float*)partial, nblk, nb,
					   d_shapevec);
	FIND_LAUNCH_CHECK("pca_bwd_finalize_kernel");
	return FIND_OK;
}
