// Skinned foot model (the reference's SUPRModel.get_meshes, model.py:726-727: self.supr_model(poses, betas, trans)): SMPL-family linear blend
// skinning with quaternion pose correctives as STAR / SUPR publish it.  Per foot n and joint j, with th = pose[n, 3j:3j+3], a = |th|:
//   R_j = I + (sin a / a) K + ((1 - cos a) / a^2) K^2,  K = [th]x            q_j = ((sin(a/2) / a) th, cos(a/2) - 1)
//   c = [betas | q of every joint (P = 4J) or of joints 1.. (P = 4(J-1))]       v_posed = v_template + sum_k dirs[:, k] c_k
//   Jn = J0 + JS . betas                                                          G_0 = [R_0 | Jn_0],  G_j = G_parent(j) o [R_j | Jn_j - Jn_parent(j)]
//   A_j = [G_j.R | G_j.t - G_j.R Jn_j]                                            out[n, v] = sum_j weights[v, j] (A_j.R v_posed + A_j.t) + trans[n]
// The angle is |th| exactly (STAR / SUPR evaluate |th + 1e-8|); below a^2 = 1 every coefficient is a power series in a^2, so values and
// derivatives are finite and exact at th = 0.
//
// Forward: skin_pose_kernel (one wave per foot: the exponential maps, c, Jn, the chain, A) and skin_fwd_kernel (a block owns a tile of vertex
// rows -- dirs and weights staged in LDS once, every foot served from there; v_posed is never stored).  Backward: the same pose kernel, then
// skin_bwd_kernel (recomputes v_posed per tile and writes the tile's partial d_c, dA = sum_v w d_out (x) [v_posed; 1] and d_trans),
// skin_reduce_kernel (adds the partials in a fixed order) and skin_chain_bwd_kernel (one wave per foot: the chain in reverse, the derivatives
// of the two exponential maps, JS).  No atomics anywhere; a foot's rows do not depend on n_feet; nothing is read back.
#include "common.h"

namespace find {
namespace skin {

constexpr int THREADS = 256;
constexpr int TILE_FLOATS = 9216;   // dirs rows + weight rows of a vertex tile: 36 KiB of LDS
constexpr int FEET_FLOATS = 3072;   // c and A of a chunk of feet: 12 KiB
constexpr int VALS_FLOATS = 4096;   // backward only: (d_out, v_posed, d_v_posed) of a chunk's (foot, vertex) pairs: 16 KiB
constexpr int MAX_TV = 64;
constexpr int MAX_J = 128;
constexpr int WAVE = 64;

// the dirs row of a vertex, 3K floats, padded to a stride = 3 (mod 32): lanes on consecutive vertices read consecutive-by-3 banks
inline __host__ __device__ int row_stride(int K) { return 3 * K + ((3 - 3 * K) % 32 + 32) % 32; }
inline __host__ __device__ int weight_stride(int J) { return J | 1; }   // odd: lanes on consecutive vertices never share a bank

struct Sizes {
	int64_t V, n_feet;
	int J, B, P, K, W;   // K = B + P coefficients per foot; W = K + 12 J + 3 gradient sums per foot and tile
};

inline bool bad_sizes(int64_t V, int64_t J, int64_t B, int64_t P, int64_t n_feet) {
	if (V < 1 || V >= (1ll << 29) || J < 1 || J > MAX_J || B < 1 || B > FEET_FLOATS || n_feet < 1 || n_feet > (1ll << 20)) return true;
	if (P != 4 * J && P != 4 * (J - 1)) return true;
	const int64_t K = B + P;
	if (row_stride((int)K) + weight_stride((int)J) > TILE_FLOATS || K + 12 * J > FEET_FLOATS) return true;
	return V * n_feet * (K + 12 * J + 3) > (1ll << 40);   // (the partials: at most one row per vertex)
}
#define FIND_SKIN_SIZES_FMT "bad sizes (V %lld, J %lld, B %lld, P %lld, n_feet %lld; 1 <= J <= %d, P = 4J or 4(J-1), 3(B+P) + J within an LDS row tile of %d floats, B + P + 12J <= %d)"
#define FIND_SKIN_SIZES_ARGS (long long)V, (long long)J, (long long)B, (long long)P, (long long)n_feet, skin::MAX_J, skin::TILE_FLOATS, skin::FEET_FLOATS

inline Sizes sizes(int64_t V, int64_t J, int64_t B, int64_t P, int64_t n_feet) {
	Sizes s;
	s.V = V, s.n_feet = n_feet, s.J = (int)J, s.B = (int)B, s.P = (int)P, s.K = (int)(B + P), s.W = (int)(B + P + 12 * J + 3);
	return s;
}

// vertices per block: as many rows as the tile holds (at most 64), but no more than it takes to give ~256 blocks; a function of (V, K, J) only
inline int tile_verts(const Sizes& s) {
	const int cap = std::min(MAX_TV, TILE_FLOATS / (row_stride(s.K) + weight_stride(s.J)));
	return (int)std::max<int64_t>(1, std::min<int64_t>(cap, cdiv(s.V, 256)));
}

// what the per-foot kernel leaves for the tile kernels (and for the backward chain)
struct Pose {
	float *c, *A, *G, *Jn;   // (N, K), (N, J, 12), (N, J, 12), (N, J, 3)
};
inline Pose carve_pose(Carver& cv, const Sizes& s) {
	Pose p;
	p.c = cv.take<float>(s.n_feet * s.K);
	p.A = cv.take<float>(s.n_feet * s.J * 12);
	p.G = cv.take<float>(s.n_feet * s.J * 12);
	p.Jn = cv.take<float>(s.n_feet * s.J * 3);
	return p;
}
inline int64_t pose_bytes(const Sizes& s) {
	Carver cv(nullptr);
	carve_pose(cv, s);
	return cv.off;
}

// ---------------------------------------------------------------------------------------------------------------- the exponential map
// For x = a^2:  A = sin a / a,  Bc = (1 - cos a) / a^2,  A1 = (dA/da) / a = (cos a - A) / a^2,  B1 = (dBc/da) / a = (A - 2 Bc) / a^2.
// Below x = 1 the power series (the first neglected term is under 2e-11 of the leading one); from there on the closed forms, whose
// differences have lost at most four bits (Bc as 2 sin^2(a/2) / a^2 loses none).
struct Coefs {
	float A, Bc, A1, B1;
};
__device__ __forceinline__ Coefs coefs(float x) {
	Coefs k;
	if (x < 1.f) {
		k.A = 1.f + x * (-1.f / 6 + x * (1.f / 120 + x * (-1.f / 5040 + x * (1.f / 362880 + x * (-1.f / 39916800 + x * (1.f / 6227020800.f))))));
		k.Bc = 0.5f + x * (-1.f / 24 + x * (1.f / 720 + x * (-1.f / 40320 + x * (1.f / 3628800 + x * (-1.f / 479001600 + x * (1.f / 87178291200.f))))));
		k.A1 = -1.f / 3 + x * (1.f / 30 + x * (-1.f / 840 + x * (1.f / 45360 + x * (-1.f / 3991680 + x * (1.f / 518918400.f)))));
		k.B1 = -1.f / 12 + x * (1.f / 180 + x * (-1.f / 6720 + x * (1.f / 453600 + x * (-1.f / 47900160 + x * (1.f / 7264857600.f)))));
	} else {
		const float a = sqrtf(x);
		float s, c;
		sincosf(a, &s, &c);
		const float sh = sinf(0.5f * a);
		k.A = s / a;
		k.Bc = 2.f * sh * sh / x;
		k.A1 = (c - k.A) / x;
		k.B1 = (k.A - 2.f * k.Bc) / x;
	}
	return k;
}

// R (row-major 3 x 3) = I + A K + Bc (th th^T - a^2 I)
__device__ __forceinline__ void rodrigues(const float th[3], float* R) {
	const float x = th[0], y = th[1], z = th[2];
	const Coefs k = coefs(x * x + y * y + z * z);
	R[0] = 1.f - k.Bc * (y * y + z * z);
	R[1] = k.Bc * x * y - k.A * z;
	R[2] = k.Bc * x * z + k.A * y;
	R[3] = k.Bc * x * y + k.A * z;
	R[4] = 1.f - k.Bc * (x * x + z * z);
	R[5] = k.Bc * y * z - k.A * x;
	R[6] = k.Bc * x * z - k.A * y;
	R[7] = k.Bc * y * z + k.A * x;
	R[8] = 1.f - k.Bc * (x * x + y * y);
}

// where joint j's quaternion sits in the pose features (-1: the root of a model whose features leave it out)
__device__ __forceinline__ int feature_slot(int j, int J, int P) { return P == 4 * J ? j : j - 1; }

// parent[j], with anything that is no earlier joint read as "root": the chain below then stays inside its arrays whatever the table holds
__device__ __forceinline__ int parent_of(const int32_t* __restrict__ parent, int j) {
	const int p = parent[j];
	return (p < 0 || p >= j) ? -1 : p;
}

// One wave per foot: steps 1-3 and 5-7 of the definition.
__global__ __launch_bounds__(WAVE) void skin_pose_kernel(const float* __restrict__ J0, const float* __restrict__ JS, const int32_t* __restrict__ parent,
															 int J, int B, int P, const float* __restrict__ pose, const float* __restrict__ betas, Pose o,
															 float* __restrict__ joints) {
	__shared__ float Rl[MAX_J * 9], Jn[MAX_J * 3], G[MAX_J * 12];
	const int64_t n = blockIdx.x;
	const int lane = threadIdx.x;
	const int K = B + P;
	const float* bt = betas + n * B;
	float* c = o.c + n * K;
	for (int b = lane; b < B; b += WAVE) c[b] = bt[b];
	for (int j = lane; j < J; j += WAVE) {
		const float* p = pose + (n * J + j) * 3;
		const float th[3] = {p[0], p[1], p[2]};
		rodrigues(th, Rl + j * 9);
		const int slot = feature_slot(j, J, P);
		if (slot >= 0) {
			const float h2 = 0.25f * (th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
			const Coefs k = coefs(h2);   // of the half angle: sin(a/2) / a = A(h) / 2, cos(a/2) - 1 = -h^2 Bc(h)
			float* q = c + B + 4 * slot;
			q[0] = 0.5f * k.A * th[0];
			q[1] = 0.5f * k.A * th[1];
			q[2] = 0.5f * k.A * th[2];
			q[3] = -h2 * k.Bc;
		}
		// (the small shape offset is summed on its own and meets the rest joint once: one rounding at the joint's magnitude, not B)
		float a0 = 0.f, a1 = 0.f, a2 = 0.f;
		const float* js = JS + (int64_t)j * B * 3;
		for (int b = 0; b < B; ++b) {
			const float s = bt[b];
			a0 = fmaf(js[3 * b + 0], s, a0);
			a1 = fmaf(js[3 * b + 1], s, a1);
			a2 = fmaf(js[3 * b + 2], s, a2);
		}
		Jn[j * 3 + 0] = J0[j * 3 + 0] + a0, Jn[j * 3 + 1] = J0[j * 3 + 1] + a1, Jn[j * 3 + 2] = J0[j * 3 + 2] + a2;
	}
	__syncthreads();
	// the chain, parents first: twelve lanes form the twelve entries of G_j (rows r of [R | t], column cc)
	const int r = (lane & 15) >> 2, cc = lane & 3;
	for (int j = 0; j < J; ++j) {
		const int p = parent_of(parent, j);
		if (lane < 12) {
			float v;
			if (p < 0) {
				v = cc < 3 ? Rl[j * 9 + r * 3 + cc] : Jn[j * 3 + r];
			} else {
				const float* Gp = G + p * 12 + r * 4;
				if (cc < 3) {
					v = Gp[0] * Rl[j * 9 + cc];
					v = fmaf(Gp[1], Rl[j * 9 + 3 + cc], v);
					v = fmaf(Gp[2], Rl[j * 9 + 6 + cc], v);
				} else {
					// (the short bone first, the parent's position last: one rounding at the position's magnitude per level, not three)
					v = Gp[0] * (Jn[j * 3 + 0] - Jn[p * 3 + 0]);
					v = fmaf(Gp[1], Jn[j * 3 + 1] - Jn[p * 3 + 1], v);
					v = fmaf(Gp[2], Jn[j * 3 + 2] - Jn[p * 3 + 2], v);
					v += Gp[3];
				}
			}
			G[j * 12 + lane] = v;
		}
		__syncthreads();
	}
	for (int i = lane; i < J * 12; i += WAVE) {
		const int j = i / 12, e = i - j * 12, rr = e >> 2, ce = e & 3;
		const float* g = G + j * 12 + rr * 4;
		float a = g[ce];
		if (ce == 3) {
			a -= fmaf(g[0], Jn[j * 3 + 0], fmaf(g[1], Jn[j * 3 + 1], g[2] * Jn[j * 3 + 2]));
			if (joints) joints[(n * J + j) * 3 + rr] = g[3];
		}
		o.A[n * J * 12 + i] = a;
		o.G[n * J * 12 + i] = G[i];
	}
	for (int i = lane; i < J * 3; i += WAVE) o.Jn[n * J * 3 + i] = Jn[i];
}

// ---------------------------------------------------------------------------------------------------------------- the vertex tiles
// rows [v0, v0 + tv) of dirs -> tile[r * P3 + k], of weights -> wt[r * JP + j]
__device__ __forceinline__ void stage_tile(const float* __restrict__ dirs, const float* __restrict__ weights, int64_t v0, int tv, int K, int J,
										   float* tile, float* wt) {
	const int row = 3 * K, P3 = row_stride(K), JP = weight_stride(J);
	const float* src = dirs + v0 * row;
	for (int i = threadIdx.x; i < tv * row; i += THREADS) {
		const int r = i / row;
		tile[r * P3 + (i - r * row)] = src[i];
	}
	const float* wsrc = weights + v0 * J;
	for (int i = threadIdx.x; i < tv * J; i += THREADS) {
		const int r = i / J;
		wt[r * JP + (i - r * J)] = wsrc[i];
	}
}

// c and A of feet [n0, n0 + nc) -> feet[nl * (K + 12 J)]: c first, then A
__device__ __forceinline__ void stage_feet(const Pose& o, int64_t n0, int nc, int K, int J, float* feet) {
	const int FW = K + 12 * J;
	for (int i = threadIdx.x; i < nc * FW; i += THREADS) {
		const int nl = i / FW, e = i - nl * FW;
		feet[i] = e < K ? o.c[(n0 + nl) * K + e] : o.A[(n0 + nl) * J * 12 + (e - K)];
	}
}

// feet per pass: what the LDS rows hold, the feet spread evenly over the passes
__device__ __forceinline__ int feet_per_pass(int64_t n_feet, int cap) {
	const int64_t passes = (n_feet + cap - 1) / cap;
	return (int)((n_feet + passes - 1) / passes);
}

// v_posed of one (foot, vertex) and the vertex's blended transform M = sum_j w_j A_j (3 x 4, row-major)
__device__ __forceinline__ void pose_vertex(const float* __restrict__ vt, const float* t, const float* w, const float* fc, int K, int J, float vp[3],
											 float M[12]) {
	// (the offsets are summed on their own and meet the template once, as the joints do in skin_pose_kernel)
	vp[0] = vp[1] = vp[2] = 0.f;
#pragma unroll 4
	for (int k = 0; k < K; ++k) {
		const float ck = fc[k];
		vp[0] = fmaf(t[3 * k + 0], ck, vp[0]);
		vp[1] = fmaf(t[3 * k + 1], ck, vp[1]);
		vp[2] = fmaf(t[3 * k + 2], ck, vp[2]);
	}
	vp[0] += vt[0], vp[1] += vt[1], vp[2] += vt[2];
#pragma unroll
	for (int e = 0; e < 12; ++e) M[e] = 0.f;
	const float* A = fc + K;
	for (int j = 0; j < J; ++j) {
		const float wj = w[j];
		if (wj == 0.f) continue;   // (skinning weights are sparse in the published models; a zero term adds nothing)
#pragma unroll
		for (int e = 0; e < 12; ++e) M[e] = fmaf(wj, A[j * 12 + e], M[e]);
	}
}

__global__ __launch_bounds__(THREADS) void skin_fwd_kernel(const float* __restrict__ v_template, const float* __restrict__ dirs,
															const float* __restrict__ weights, int64_t V, int J, int K, int TV, Pose o,
															const float* __restrict__ trans, int64_t n_feet, float* __restrict__ out) {
	__shared__ float tile[TILE_FLOATS];
	__shared__ float feet[FEET_FLOATS];
	const int P3 = row_stride(K), JP = weight_stride(J), FW = K + 12 * J;
	const int64_t v0 = (int64_t)blockIdx.x * TV;
	const int tv = (int)std::min<int64_t>(TV, V - v0);
	float* wt = tile + TV * P3;
	stage_tile(dirs, weights, v0, tv, K, J, tile, wt);
	const int NC = feet_per_pass(n_feet, FEET_FLOATS / FW);
	for (int64_t n0 = 0; n0 < n_feet; n0 += NC) {
		const int nc = (int)std::min<int64_t>(NC, n_feet - n0);
		__syncthreads();   // (the tile is complete / the previous feet are no longer read)
		stage_feet(o, n0, nc, K, J, feet);
		__syncthreads();
		for (int i = threadIdx.x; i < nc * tv; i += THREADS) {
			const int nl = i / tv, v = i - nl * tv;
			float vp[3], M[12];
			pose_vertex(v_template + (v0 + v) * 3, tile + v * P3, wt + v * JP, feet + nl * FW, K, J, vp, M);
			const float* tr = trans + (n0 + nl) * 3;
			float* dst = out + ((n0 + nl) * V + v0 + v) * 3;
#pragma unroll
			for (int r = 0; r < 3; ++r) dst[r] = fmaf(M[r * 4 + 0], vp[0], fmaf(M[r * 4 + 1], vp[1], fmaf(M[r * 4 + 2], vp[2], M[r * 4 + 3]))) + tr[r];
		}
	}
}

// partial[blk][n][o]: o < K: d_c[k] = sum_v dirs[v, k, :] . (M.R^T d_out);  then dA[j][r][cc] = sum_v w[v, j] d_out[r] [v_posed; 1][cc];  then
// d_trans[r] = sum_v d_out[r] -- each over the tile's vertices in vertex order
__global__ __launch_bounds__(THREADS) void skin_bwd_kernel(const float* __restrict__ v_template, const float* __restrict__ dirs,
															const float* __restrict__ weights, int64_t V, int J, int K, int TV, Pose o,
															const float* __restrict__ d_out, int64_t n_feet, float* __restrict__ partial) {
	__shared__ float tile[TILE_FLOATS];
	__shared__ float feet[FEET_FLOATS];
	__shared__ float vals[VALS_FLOATS];
	const int P3 = row_stride(K), JP = weight_stride(J), FW = K + 12 * J, W = FW + 3;
	const int64_t v0 = (int64_t)blockIdx.x * TV;
	const int tv = (int)std::min<int64_t>(TV, V - v0);
	float* wt = tile + TV * P3;
	stage_tile(dirs, weights, v0, tv, K, J, tile, wt);
	const int NC = feet_per_pass(n_feet, std::min(FEET_FLOATS / FW, VALS_FLOATS / (9 * TV)));
	for (int64_t n0 = 0; n0 < n_feet; n0 += NC) {
		const int nc = (int)std::min<int64_t>(NC, n_feet - n0);
		__syncthreads();
		stage_feet(o, n0, nc, K, J, feet);
		__syncthreads();
		for (int i = threadIdx.x; i < nc * tv; i += THREADS) {
			const int nl = i / tv, v = i - nl * tv;
			float vp[3], M[12];
			pose_vertex(v_template + (v0 + v) * 3, tile + v * P3, wt + v * JP, feet + nl * FW, K, J, vp, M);
			const float* g = d_out + ((n0 + nl) * V + v0 + v) * 3;
			const float g0 = g[0], g1 = g[1], g2 = g[2];
			float* q = vals + i * 9;
			q[0] = g0, q[1] = g1, q[2] = g2;
			q[3] = vp[0], q[4] = vp[1], q[5] = vp[2];
#pragma unroll
			for (int cc = 0; cc < 3; ++cc) q[6 + cc] = fmaf(M[cc], g0, fmaf(M[4 + cc], g1, M[8 + cc] * g2));
		}
		__syncthreads();
		for (int i = threadIdx.x; i < nc * W; i += THREADS) {
			const int nl = i / W, e = i - nl * W;
			const float* q = vals + nl * tv * 9;
			float acc = 0.f;
			if (e < K) {
				const float* t = tile + 3 * e;
				for (int v = 0; v < tv; ++v) {
					acc = fmaf(t[v * P3 + 0], q[v * 9 + 6], acc);
					acc = fmaf(t[v * P3 + 1], q[v * 9 + 7], acc);
					acc = fmaf(t[v * P3 + 2], q[v * 9 + 8], acc);
				}
			} else if (e < FW) {
				const int j = (e - K) / 12, a = (e - K) - j * 12, r = a >> 2, cc = a & 3;
				if (cc < 3) {
					for (int v = 0; v < tv; ++v) acc = fmaf(wt[v * JP + j] * q[v * 9 + r], q[v * 9 + 3 + cc], acc);
				} else {
					for (int v = 0; v < tv; ++v) acc = fmaf(wt[v * JP + j], q[v * 9 + r], acc);
				}
			} else {
				for (int v = 0; v < tv; ++v) acc += q[v * 9 + (e - FW)];
			}
			partial[((int64_t)blockIdx.x * n_feet + n0 + nl) * W + e] = acc;
		}
	}
}

// red[i] = sum over the tiles of partial[blk][i], i = (n, o): sixteen lanes per sum, lane l adding tiles l, l + 16, ... in order, then the
// sixteen added pairwise (8, 4, 2, 1 apart).  The order depends on the number of tiles only.
__global__ __launch_bounds__(THREADS) void skin_reduce_kernel(const float* __restrict__ partial, int nblk, int64_t nw, float* __restrict__ red) {
	const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) >> 4;
	const int l = threadIdx.x & 15;
	float s = 0.f;
	if (i < nw) {
#pragma unroll 4
		for (int k = l; k < nblk; k += 16) s += partial[(int64_t)k * nw + i];
	}
#pragma unroll
	for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
	if (i < nw && l == 0) red[i] = s;
}

// One wave per foot: from red = (d_c, dA, d_trans) of the foot, the chain in reverse (dA -> dG -> dR_j, dJn), then the derivatives of the two
// exponential maps and JS.
__global__ __launch_bounds__(WAVE) void skin_chain_bwd_kernel(const float* __restrict__ JS, const int32_t* __restrict__ parent, int J, int B, int P,
																  const float* __restrict__ pose, Pose o, const float* __restrict__ red,
																  float* __restrict__ d_pose, float* __restrict__ d_betas, float* __restrict__ d_trans) {
	__shared__ float Rl[MAX_J * 9], Jn[MAX_J * 3], G[MAX_J * 12], dG[MAX_J * 12], dR[MAX_J * 9], dJn[MAX_J * 3];
	const int64_t n = blockIdx.x;
	const int lane = threadIdx.x;
	const int K = B + P;
	const float* dc = red + n * (K + 12 * J + 3);
	const float* dA = dc + K;
	if (lane < 3) d_trans[n * 3 + lane] = dA[12 * J + lane];
	for (int i = lane; i < J * 12; i += WAVE) G[i] = o.G[n * J * 12 + i];
	for (int i = lane; i < J * 3; i += WAVE) Jn[i] = o.Jn[n * J * 3 + i];
	for (int j = lane; j < J; j += WAVE) {
		const float* p = pose + (n * J + j) * 3;
		const float th[3] = {p[0], p[1], p[2]};
		rodrigues(th, Rl + j * 9);
	}
	__syncthreads();
	// A_j = [G_j.R | G_j.t - G_j.R Jn_j]:  dG_j.R = dA_j.R - dA_j.t Jn_j^T,  dG_j.t = dA_j.t,  dJn_j = -G_j.R^T dA_j.t
	for (int i = lane; i < J * 12; i += WAVE) {
		const int j = i / 12, e = i - j * 12, r = e >> 2, cc = e & 3;
		const float at = dA[j * 12 + r * 4 + 3];
		dG[i] = cc < 3 ? fmaf(-at, Jn[j * 3 + cc], dA[i]) : at;
	}
	for (int i = lane; i < J * 3; i += WAVE) {
		const int j = i / 3, k = i - j * 3;
		const float* g = G + j * 12;
		const float* a = dA + j * 12;
		dJn[i] = -fmaf(g[k], a[3], fmaf(g[4 + k], a[7], g[8 + k] * a[11]));
	}
	__syncthreads();
	// children first.  G_j = G_p o [R_j | d_j], d_j = Jn_j - Jn_p:  lanes 0-11 add dG_j [R_j | d_j]^T into dG_p, lanes 16-24 form
	// dR_j = G_p.R^T dG_j.R, lanes 32-34 dd = G_p.R^T dG_j.t, which goes to dJn_j and, negated, to dJn_p
	const int r = (lane & 15) >> 2, cc = lane & 3;
	for (int j = J - 1; j >= 0; --j) {
		const int p = parent_of(parent, j);
		const float* g = dG + j * 12;
		if (lane < 12) {
			if (p >= 0) {
				float v;
				if (cc < 3) {
					const float* rl = Rl + j * 9 + cc * 3;
					v = fmaf(g[r * 4 + 0], rl[0], fmaf(g[r * 4 + 1], rl[1], g[r * 4 + 2] * rl[2]));
					v = fmaf(g[r * 4 + 3], Jn[j * 3 + cc] - Jn[p * 3 + cc], v);
				} else {
					v = g[r * 4 + 3];
				}
				dG[p * 12 + lane] += v;
			}
		} else if (lane >= 16 && lane < 25) {
			const int a = (lane - 16) / 3, b = (lane - 16) - a * 3;
			dR[j * 9 + lane - 16] = p < 0 ? g[a * 4 + b] : fmaf(G[p * 12 + a], g[b], fmaf(G[p * 12 + 4 + a], g[4 + b], G[p * 12 + 8 + a] * g[8 + b]));
		} else if (lane >= 32 && lane < 35) {
			const int a = lane - 32;
			const float dd = p < 0 ? g[a * 4 + 3] : fmaf(G[p * 12 + a], g[3], fmaf(G[p * 12 + 4 + a], g[7], G[p * 12 + 8 + a] * g[11]));
			dJn[j * 3 + a] += dd;
			if (p >= 0) dJn[p * 3 + a] -= dd;
		}
		__syncthreads();
	}
	// d theta_k = th_k (A1 (th . w) + B1 (th^T D th - a^2 tr D)) + A w_k + Bc ((D th)_k + (D^T th)_k - 2 th_k tr D),  D = dR_j,
	// w = (D21 - D12, D02 - D20, D10 - D01);  plus the quaternion's: S dq_k + S1 th_k (th . dq_xyz) - S th_k dq_w / 2,  S = A(h) / 2, S1 = A1(h) / 8
	for (int j = lane; j < J; j += WAVE) {
		const float* p = pose + (n * J + j) * 3;
		const float th[3] = {p[0], p[1], p[2]};
		const float* D = dR + j * 9;
		const float a2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
		const Coefs k = coefs(a2);
		const float w[3] = {D[7] - D[5], D[2] - D[6], D[3] - D[1]};
		const float tr = D[0] + D[4] + D[8];
		float Dt[3], Dtt[3];
#pragma unroll
		for (int a = 0; a < 3; ++a) {
			Dt[a] = D[a * 3] * th[0] + D[a * 3 + 1] * th[1] + D[a * 3 + 2] * th[2];
			Dtt[a] = D[a] * th[0] + D[3 + a] * th[1] + D[6 + a] * th[2];
		}
		const float tw = th[0] * w[0] + th[1] * w[1] + th[2] * w[2];
		const float tDt = th[0] * Dt[0] + th[1] * Dt[1] + th[2] * Dt[2];
		const float radial = k.A1 * tw + k.B1 * (tDt - a2 * tr);
		float d[3];
#pragma unroll
		for (int a = 0; a < 3; ++a) d[a] = th[a] * radial + k.A * w[a] + k.Bc * (Dt[a] + Dtt[a] - 2.f * th[a] * tr);
		const int slot = feature_slot(j, J, P);
		if (slot >= 0) {
			const float* dq = dc + B + 4 * slot;
			const Coefs kh = coefs(0.25f * a2);
			const float S = 0.5f * kh.A, S1 = 0.125f * kh.A1;
			const float tq = th[0] * dq[0] + th[1] * dq[1] + th[2] * dq[2];
			const float rq = S1 * tq - 0.5f * S * dq[3];
#pragma unroll
			for (int a = 0; a < 3; ++a) d[a] += S * dq[a] + th[a] * rq;
		}
		float* dst = d_pose + (n * J + j) * 3;
		dst[0] = d[0], dst[1] = d[1], dst[2] = d[2];
	}
	// d_betas[b] = d_c[b] + sum_j JS[j, b, :] . dJn_j, joints in order
	for (int b = lane; b < B; b += WAVE) {
		float acc = dc[b];
		for (int j = 0; j < J; ++j) {
			const float* js = JS + ((int64_t)j * B + b) * 3;
			acc = fmaf(js[0], dJn[j * 3 + 0], fmaf(js[1], dJn[j * 3 + 1], fmaf(js[2], dJn[j * 3 + 2], acc)));
		}
		d_betas[n * B + b] = acc;
	}
}

}  // namespace skin
}  // namespace find

using namespace find;

extern "C" int64_t find_skin_fwd_ws_bytes(int64_t n_feet, int64_t V, int64_t J, int64_t B, int64_t P) {
	if (skin::bad_sizes(V, J, B, P, n_feet)) return -1;
	return skin::pose_bytes(skin::sizes(V, J, B, P, n_feet));
}

extern "C" int64_t find_skin_bwd_ws_bytes(int64_t n_feet, int64_t V, int64_t J, int64_t B, int64_t P) {
	if (skin::bad_sizes(V, J, B, P, n_feet)) return -1;
	const skin::Sizes s = skin::sizes(V, J, B, P, n_feet);
	const int64_t nblk = cdiv(V, skin::tile_verts(s));
	return skin::pose_bytes(s) + align_up(nblk * n_feet * s.W * (int64_t)sizeof(float), 256) + align_up(n_feet * s.W * (int64_t)sizeof(float), 256);
}

extern "C" int find_skin_fwd(const float* v_template, const float* dirs, const float* J0, const float* JS, const float* weights, const int32_t* parent,
							 int64_t V, int64_t J, int64_t B, int64_t P, const float* pose, const float* betas, const float* trans, int64_t n_feet,
							 float* out, float* joints, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(v_template && dirs && J0 && JS && weights && parent && pose && betas && trans && out && ws, "find_skin_fwd: NULL argument");
	FIND_REQUIRE(!skin::bad_sizes(V, J, B, P, n_feet), "find_skin_fwd: " FIND_SKIN_SIZES_FMT, FIND_SKIN_SIZES_ARGS);
	if (ws_bytes < find_skin_fwd_ws_bytes(n_feet, V, J, B, P)) {
		set_error("find_skin_fwd: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)find_skin_fwd_ws_bytes(n_feet, V, J, B, P));
		return FIND_EWORKSPACE;
	}
	const skin::Sizes s = skin::sizes(V, J, B, P, n_feet);
	hipStream_t st = (hipStream_t)stream;
	Carver cv(ws);
	const skin::Pose o = skin::carve_pose(cv, s);
	hipLaunchKernelGGL(skin::skin_pose_kernel, dim3((unsigned)n_feet), dim3(skin::WAVE), 0, st, J0, JS, parent, s.J, s.B, s.P, pose, betas, o, joints);
	FIND_LAUNCH_CHECK("skin_pose_kernel");
	const int TV = skin::tile_verts(s);
	hipLaunchKernelGGL(skin::skin_fwd_kernel, dim3((unsigned)cdiv(V, TV)), dim3(skin::THREADS), 0, st, v_template, dirs, weights, V, s.J, s.K, TV, o,
					   trans, n_feet, out);
	FIND_LAUNCH_CHECK("skin_fwd_kernel");
	return FIND_OK;
}

extern "C" int find_skin_bwd(const float* v_template, const float* dirs, const float* J0, const float* JS, const float* weights, const int32_t* parent,
							 int64_t V, int64_t J, int64_t B, int64_t P, const float* pose, const float* betas, const float* d_out, int64_t n_feet,
							 float* d_pose, float* d_betas, float* d_trans, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(v_template && dirs && J0 && JS && weights && parent && pose && betas && d_out && d_pose && d_betas && d_trans && ws,
				 "find_skin_bwd: NULL argument");
	FIND_REQUIRE(!skin::bad_sizes(V, J, B, P, n_feet), "find_skin_bwd: " FIND_SKIN_SIZES_FMT, FIND_SKIN_SIZES_ARGS);
	if (ws_bytes < find_skin_bwd_ws_bytes(n_feet, V, J, B, P)) {
		set_error("find_skin_bwd: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)find_skin_bwd_ws_bytes(n_feet, V, J, B, P));
		return FIND_EWORKSPACE;
	}
	const skin::Sizes s = skin::sizes(V, J, B, P, n_feet);
	hipStream_t st = (hipStream_t)stream;
	Carver cv(ws);
	const skin::Pose o = skin::carve_pose(cv, s);
	const int TV = skin::tile_verts(s);
	const int nblk = (int)cdiv(V, TV);
	const int64_t nw = n_feet * s.W;
	float* partial = cv.take<float>(nblk * nw);
	float* red = cv.take<float>(nw);
	hipLaunchKernelGGL(skin::skin_pose_kernel, dim3((unsigned)n_feet), dim3(skin::WAVE), 0, st, J0, JS, parent, s.J, s.B, s.P, pose, betas, o,
					   (float*)nullptr);
	FIND_LAUNCH_CHECK("skin_pose_kernel");
	hipLaunchKernelGGL(skin::skin_bwd_kernel, dim3((unsigned)nblk), dim3(skin::THREADS), 0, st, v_template, dirs, weights, V, s.J, s.K, TV, o, d_out,
					   n_feet, partial);
	FIND_LAUNCH_CHECK("skin_bwd_kernel");
	hipLaunchKernelGGL(skin::skin_reduce_kernel, dim3((unsigned)cdiv(nw * 16, skin::THREADS)), dim3(skin::THREADS), 0, st, (const float*)partial, nblk, nw,
					   red);
	FIND_LAUNCH_CHECK("skin_reduce_kernel");
	hipLaunchKernelGGL(skin::skin_chain_bwd_kernel, dim3((unsigned)n_feet), dim3(skin::WAVE), 0, st, JS, parent, s.J, s.B, s.P, pose, o, (const float*)red,
					   d_pose, d_betas, d_trans);
	FIND_LAUNCH_CHECK("skin_chain_bwd_kernel");
	return FIND_OK;
}
