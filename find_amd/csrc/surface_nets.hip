// Iso-surface extraction by surface nets (gfx950; Gibson 1998, "naive dual contouring"): a scalar field on a grid goes in, an indexed triangle
// mesh comes out -- one vertex per grid cell the level set passes through, one quad (two triangles) per lattice edge whose ends lie on different
// sides.  Not in the reference; find_amd.isosurface builds the watertight remesh and offset surfaces on it.  The definition (sides, edge order,
// the vertex, the faces' order and orientation, the status bits) is written out in include/find_hip.h; the per-cell and per-sample arithmetic is
// surface_nets_math.h, which tools/surface_nets_host_check.cpp compiles for the host.
//
// Three counted passes, no atomics.  A workgroup of SN_BLOCK = 256 threads owns 256 consecutive SAMPLES (flat sample order: the lattice edges
// that start there) and 256 consecutive CELLS (flat cell order); both are numbered by blockIdx.x, a mesh is blockIdx.y.
//   count   count_kernel: per block the number of active cells and of quads, and the block's status bits.  A flag's rank within a wave is the
//           popcount of its ballot below the lane; the four waves' totals meet in LDS.  scan_kernel (one block per mesh): exclusive scans of
//           both counts in block order -> block offsets, the mesh's totals and status.
//   emit    vertex_kernel ranks the active cells again (the same ballots), writes the cell -> vertex map and g; face_kernel ranks the quads in
//           (sample, axis) order and gathers the four cells' vertices from the map; pad_kernel writes the rows past the counts and the two
//           capacity bits.  Every store is guarded by the capacity.
//   bwd     grad_kernel: one gather per sample (sample_backward), the block's d L / d iso reduced in double in a fixed tree; iso_kernel adds
//           the blocks' sums per mesh, a thread its stride in block order, then the same tree.
// Every index and sum is a function of the mesh's own grid: the result does not depend on N, on the mesh's place in the batch or on anything
// the launch chooses, and two runs agree bit for bit.  The passes are bandwidth-light gathers out of L2 (a field of 128^3 floats is 8 MiB);
// nothing here is tuned beyond coalesced sample order.
#include "common.h"
#include "surface_nets_math.h"

namespace find {
namespace surface_nets {

static_assert(SN_BLOCK == 256 && SN_BLOCK == FIND_SURFACE_NETS_BLOCK, "four waves of 64 per workgroup");

struct Grid {
	int nx, ny, nz;
	int64_t samples, cells;
	int nb;   // blocks per mesh: ceil(samples / SN_BLOCK) (>= the cells' blocks)
};

static Grid make_grid(int64_t nx, int64_t ny, int64_t nz) {
	Grid g;
	g.nx = (int)nx; g.ny = (int)ny; g.nz = (int)nz;
	g.samples = nx * ny * nz;
	g.cells = (nx - 1) * (ny - 1) * (nz - 1);
	g.nb = (int)cdiv(g.samples, SN_BLOCK);
	return g;
}

// The workspace: the cell -> vertex map FIRST (the backward call is handed that part), then the per-block counts, status and offsets.
struct Workspace {
	int32_t* cellmap;   // (N, cells)
	int32_t *vcount, *qcount, *bstatus;   // (N, nb)
	int64_t *voff, *qoff;   // (N, nb)
	int64_t bytes;
	Workspace(void* ws, int64_t n, const Grid& g) {
		Carver c(ws);
		cellmap = c.take<int32_t>(n * g.cells);
		vcount = c.take<int32_t>(n * g.nb); qcount = c.take<int32_t>(n * g.nb); bstatus = c.take<int32_t>(n * g.nb);
		voff = c.take<int64_t>(n * g.nb); qoff = c.take<int64_t>(n * g.nb);
		bytes = c.off;
	}
};

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Cell c of the mesh (flat cell order): its corner values; returns whether the cell exists.
__device__ __forceinline__ bool load_cell(const float* __restrict__ vals, const Grid& g, int64_t c, int& ci, int& cj, int& ck, float v[8]) {
	if (c >= g.cells) return false;
	ck = (int)(c % (g.nz - 1));
	cj = (int)((c / (g.nz - 1)) % (g.ny - 1));
	ci = (int)(c / ((int64_t)(g.nz - 1) * (g.ny - 1)));
#pragma unroll
	for (int k = 0; k < 8; ++k) v[k] = vals[((int64_t)(ci + ((k >> 2) & 1)) * g.ny + (cj + ((k >> 1) & 1))) * g.nz + (ck + (k & 1))];
	return true;
}

// Sample s of the mesh (flat sample order): which of its +x, +y, +z lattice edges emit a quad (bits 0, 1, 2), whether the sample is inside
// and whether it is finite.
__device__ __forceinline__ int sample_quads(const float* __restrict__ vals, const Grid& g, float iso, int64_t s, int& i, int& j, int& k, bool& in, bool& finite) {
	in = false; finite = true;
	if (s >= g.samples) return 0;
	k = (int)(s % g.nz);
	j = (int)((s / g.nz) % g.ny);
	i = (int)(s / ((int64_t)g.nz * g.ny));
	const float v = vals[s];
	finite = is_finite(v);
	in = is_inside(v, iso);
	const bool mi = i >= 1 && i <= g.nx - 2, mj = j >= 1 && j <= g.ny - 2, mk = k >= 1 && k <= g.nz - 2;
	int q = 0;
	if (i + 1 < g.nx && mj && mk && is_inside(vals[s + (int64_t)g.ny * g.nz], iso) != in) q |= 1;
	if (j + 1 < g.ny && mk && mi && is_inside(vals[s + g.nz], iso) != in) q |= 2;
	if (k + 1 < g.nz && mi && mj && is_inside(vals[s + 1], iso) != in) q |= 4;
	return q;
}

// The rank of this thread's flag among the block's flags in thread order, and the block's count.  tot: 4 ints of LDS; two barriers.
__device__ __forceinline__ int rank_flags(bool flag, int* tot, int& block_total) {
	const uint64_t b = __ballot(flag);
	const int wave = threadIdx.x >> 6;
	__syncthreads();   // (tot may still be read from the use before)
	if ((threadIdx.x & 63) == 0) tot[wave] = __popcll(b);
	__syncthreads();
	int base = 0;
	block_total = 0;
#pragma unroll
	for (int w = 0; w < 4; ++w) {
		if (w < wave) base += tot[w];
		block_total += tot[w];
	}
	return base + __popcll(b & lanes_below());
}

// The rank of this thread's first quad among the block's quads in (thread, axis) order, and the block's count.
__device__ __forceinline__ int rank_quads(int q, int* tot, int& block_total) {
	const uint64_t bx = __ballot(q & 1), by = __ballot(q & 2), bz = __ballot(q & 4);
	const int wave = threadIdx.x >> 6;
	__syncthreads();
	if ((threadIdx.x & 63) == 0) tot[wave] = __popcll(bx) + __popcll(by) + __popcll(bz);
	__syncthreads();
	int base = 0;
	block_total = 0;
#pragma unroll
	for (int w = 0; w < 4; ++w) {
		if (w < wave) base += tot[w];
		block_total += tot[w];
	}
	const uint64_t lt = lanes_below();
	return base + __popcll(bx & lt) + __popcll(by & lt) + __popcll(bz & lt);
}

// grid (nb, N)
__global__ __launch_bounds__(SN_BLOCK) void count_kernel(const float* __restrict__ values, float iso, Grid g, int32_t* __restrict__ vcount,
														 int32_t* __restrict__ qcount, int32_t* __restrict__ bstatus) {
	__shared__ int tot[4];
	__shared__ int st[4];
	const int n = blockIdx.y;
	const float* vals = values + (int64_t)n * g.samples;
	const int64_t t = (int64_t)blockIdx.x * SN_BLOCK + threadIdx.x;
	int i, j, k, ci, cj, ck;
	bool in, finite;
	float v[8];
	const int q = sample_quads(vals, g, iso, t, i, j, k, in, finite);
	bool active = false, edge = false;
	if (load_cell(vals, g, t, ci, cj, ck, v)) {
		const int mask = corner_mask(v, iso);
		active = mask != 0 && mask != 255;
		edge = active && (ci == 0 || cj == 0 || ck == 0 || ci == g.nx - 2 || cj == g.ny - 2 || ck == g.nz - 2);
	}
	int nv, nq;
	rank_flags(active, tot, nv);
	rank_quads(q, tot, nq);
	const int mine = (__ballot(edge) ? 1 : 0) | (__ballot(!finite) ? 8 : 0);
	if ((threadIdx.x & 63) == 0) st[threadIdx.x >> 6] = mine;
	__syncthreads();
	if (threadIdx.x == 0) {
		const int64_t o = (int64_t)n * g.nb + blockIdx.x;
		vcount[o] = nv;
		qcount[o] = nq;
		bstatus[o] = st[0] | st[1] | st[2] | st[3];
	}
}

// grid (N): exclusive scans in block order, the totals and the status word
__global__ __launch_bounds__(SN_BLOCK) void scan_kernel(int nb, const int32_t* __restrict__ vcount, const int32_t* __restrict__ qcount,
														const int32_t* __restrict__ bstatus, int64_t* __restrict__ voff, int64_t* __restrict__ qoff,
														int64_t* __restrict__ n_verts, int64_t* __restrict__ n_faces, int32_t* __restrict__ status) {
	__shared__ int wv[4], wq[4], wst[4];
	const int n = blockIdx.x;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int64_t carry_v = 0, carry_q = 0;
	int st = 0;
	for (int base = 0; base < nb; base += SN_BLOCK) {
		const int idx = base + threadIdx.x;
		const int64_t o = (int64_t)n * nb + idx;
		const int v = idx < nb ? vcount[o] : 0, q = idx < nb ? qcount[o] : 0;
		st |= idx < nb ? bstatus[o] : 0;
		int iv = v, iq = q;   // (inclusive within the wave: at most 64 * 256 and 64 * 768)
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const int tv = __shfl_up(iv, d, 64), tq = __shfl_up(iq, d, 64);
			if (lane >= d) { iv += tv; iq += tq; }
		}
		if (lane == 63) { wv[wave] = iv; wq[wave] = iq; }
		__syncthreads();
		int64_t bv = carry_v, bq = carry_q;
#pragma unroll
		for (int w = 0; w < 4; ++w) {
			if (w < wave) { bv += wv[w]; bq += wq[w]; }
			carry_v += wv[w]; carry_q += wq[w];
		}
		if (idx < nb) { voff[o] = bv + iv - v; qoff[o] = bq + iq - q; }
		__syncthreads();
	}
	const int mine = (__ballot(st & 1) ? 1 : 0) | (__ballot(st & 8) ? 8 : 0);
	if (lane == 0) wst[wave] = mine;
	__syncthreads();
	if (threadIdx.x == 0) {
		n_verts[n] = carry_v;
		n_faces[n] = 2 * carry_q;
		status[n] = wst[0] | wst[1] | wst[2] | wst[3];
	}
}

// grid (ceil(cells / 256), N): the cell -> vertex map (every cell) and g (rows below vcap)
__global__ __launch_bounds__(SN_BLOCK) void vertex_kernel(const float* __restrict__ values, float iso, Grid g, const int64_t* __restrict__ voff, int64_t vcap,
														  int32_t* __restrict__ cellmap, float* __restrict__ out_g) {
	__shared__ int tot[4];
	const int n = blockIdx.y;
	const float* vals = values + (int64_t)n * g.samples;
	const int64_t c = (int64_t)blockIdx.x * SN_BLOCK + threadIdx.x;
	int ci = 0, cj = 0, ck = 0;
	float v[8], p[3];
	const bool exists = load_cell(vals, g, c, ci, cj, ck, v);
	const bool active = exists && cell_vertex(v, iso, p) > 0;
	int nv;
	const int64_t idx = voff[(int64_t)n * g.nb + blockIdx.x] + rank_flags(active, tot, nv);
	if (exists) cellmap[(int64_t)n * g.cells + c] = active ? (int32_t)idx : -1;
	if (active && idx < vcap) {
		float* o = out_g + ((int64_t)n * vcap + idx) * 3;
		o[0] = (float)ci + p[0]; o[1] = (float)cj + p[1]; o[2] = (float)ck + p[2];
	}
}

// grid (nb, N): two triangles per quad, rows below fcap
__global__ __launch_bounds__(SN_BLOCK) void face_kernel(const float* __restrict__ values, float iso, Grid g, const int64_t* __restrict__ qoff,
														const int32_t* __restrict__ cellmap, int64_t fcap, int32_t* __restrict__ faces) {
	__shared__ int tot[4];
	const int n = blockIdx.y;
	const float* vals = values + (int64_t)n * g.samples;
	const int32_t* map = cellmap + (int64_t)n * g.cells;
	const int64_t s = (int64_t)blockIdx.x * SN_BLOCK + threadIdx.x;
	int ijk[3] = {0, 0, 0};
	bool in, finite;
	const int q = sample_quads(vals, g, iso, s, ijk[0], ijk[1], ijk[2], in, finite);
	int nq;
	int64_t quad = qoff[(int64_t)n * g.nb + blockIdx.x] + rank_quads(q, tot, nq);
	const int64_t cstride[3] = {(int64_t)(g.ny - 1) * (g.nz - 1), g.nz - 1, 1};
	const int64_t here = ijk[0] * cstride[0] + ijk[1] * cstride[1] + ijk[2] * cstride[2];   // (the cell with the sample as its first corner)
#pragma unroll
	for (int ax = 0; ax < 3; ++ax) {
		if (!((q >> ax) & 1)) continue;
		const int64_t su = cstride[(ax + 1) % 3], sw = cstride[(ax + 2) % 3];
		int32_t c[4] = {map[here - su - sw], map[here - sw], map[here], map[here - su]};
		if (!in) { const int32_t a = c[0], b = c[1]; c[0] = c[3]; c[1] = c[2]; c[2] = b; c[3] = a; }
		const int64_t row = 2 * quad;
		int32_t* o = faces + ((int64_t)n * fcap + row) * 3;
		if (row < fcap) { o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
		if (row + 1 < fcap) { o[3] = c[0]; o[4] = c[2]; o[5] = c[3]; }
		++quad;
	}
}

// grid (max(1, ceil(max(vcap, fcap) / 256)), N): rows at or past the counts, and the capacity bits
__global__ __launch_bounds__(SN_BLOCK) void pad_kernel(const int64_t* __restrict__ n_verts, const int64_t* __restrict__ n_faces, int64_t vcap, int64_t fcap,
													   float* __restrict__ out_g, int32_t* __restrict__ faces, int32_t* __restrict__ status) {
	const int n = blockIdx.y;
	const int64_t r = (int64_t)blockIdx.x * SN_BLOCK + threadIdx.x;
	const int64_t nv = n_verts[n], nf = n_faces[n];
	if (r >= nv && r < vcap) {
		float* o = out_g + ((int64_t)n * vcap + r) * 3;
		o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
	}
	if (r >= nf && r < fcap) {
		int32_t* o = faces + ((int64_t)n * fcap + r) * 3;
		o[0] = -1; o[1] = -1; o[2] = -1;
	}
	if (r == 0) status[n] = (status[n] & ~6) | (nv > vcap ? 2 : 0) | (nf > fcap ? 4 : 0);
}

// A block's double in a fixed tree: the butterfly within each wave, then the four waves in their order.  part: 4 doubles of LDS.
__device__ __forceinline__ double block_sum(double x, double* part) {
	x = wave_sum(x);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
	__syncthreads();
	return ((part[0] + part[1]) + part[2]) + part[3];
}

// grid (nb, N): d L / d value of every sample, and the block's share of d L / d iso
__global__ __launch_bounds__(SN_BLOCK) void grad_kernel(const float* __restrict__ values, float iso, Grid g, const int32_t* __restrict__ cellmap,
														const float* __restrict__ grad_g, int64_t vcap, float* __restrict__ grad_values, double* __restrict__ iso_part) {
	__shared__ double part[4];
	const int n = blockIdx.y;
	const int64_t s = (int64_t)blockIdx.x * SN_BLOCK + threadIdx.x;
	double d_iso = 0.;
	if (s < g.samples) {
		const int k = (int)(s % g.nz), j = (int)((s / g.nz) % g.ny), i = (int)(s / ((int64_t)g.nz * g.ny));
		grad_values[(int64_t)n * g.samples + s] = sample_backward(values + (int64_t)n * g.samples, g.nx, g.ny, g.nz, i, j, k, iso, cellmap + (int64_t)n * g.cells,
																  grad_g + (int64_t)n * vcap * 3, vcap, &d_iso);
	}
	const double sum = block_sum(d_iso, part);
	if (threadIdx.x == 0) iso_part[(int64_t)n * g.nb + blockIdx.x] = sum;
}

// grid (N)
__global__ __launch_bounds__(SN_BLOCK) void iso_kernel(int nb, const double* __restrict__ iso_part, float* __restrict__ grad_iso) {
	__shared__ double part[4];
	const int n = blockIdx.x;
	double x = 0.;
	for (int b = threadIdx.x; b < nb; b += SN_BLOCK) x += iso_part[(int64_t)n * nb + b];
	const double sum = block_sum(x, part);
	if (threadIdx.x == 0) grad_iso[n] = (float)sum;
}

static inline bool bad_dims(int64_t n, int64_t nx, int64_t ny, int64_t nz) {
	return n < 0 || n >= (1 << 16) || nx < 2 || nx > 1024 || ny < 2 || ny > 1024 || nz < 2 || nz > 1024;
}

}  // namespace surface_nets
}  // namespace find

using namespace find;
using namespace find::surface_nets;

extern "C" int64_t find_surface_nets_ws_bytes(int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz) {
	if (surface_nets::bad_dims(n_meshes, nx, ny, nz)) return -1;
	return std::max<int64_t>(256, Workspace(nullptr, n_meshes, make_grid(nx, ny, nz)).bytes);
}

extern "C" int64_t find_surface_nets_bwd_ws_bytes(int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz) {
	if (surface_nets::bad_dims(n_meshes, nx, ny, nz)) return -1;
	return std::max<int64_t>(256, align_up(n_meshes * make_grid(nx, ny, nz).nb * (int64_t)sizeof(double), 256));
}

extern "C" int find_surface_nets_count(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, int64_t* n_verts, int64_t* n_faces,
									   int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!surface_nets::bad_dims(n_meshes, nx, ny, nz), "find_surface_nets_count: bad sizes");
	if (n_meshes == 0) return FIND_OK;
	FIND_REQUIRE(values && n_verts && n_faces && status && ws, "find_surface_nets_count: NULL argument");
	if (ws_bytes < find_surface_nets_ws_bytes(n_meshes, nx, ny, nz)) { set_error("find_surface_nets_count: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	const Grid g = make_grid(nx, ny, nz);
	const Workspace w(ws, n_meshes, g);
	hipLaunchKernelGGL(count_kernel, dim3((unsigned)g.nb, (unsigned)n_meshes), dim3(SN_BLOCK), 0, s, values, iso, g, w.vcount, w.qcount, w.bstatus);
	FIND_LAUNCH_CHECK("surface_nets count_kernel");
	hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n_meshes), dim3(SN_BLOCK), 0, s, g.nb, w.vcount, w.qcount, w.bstatus, w.voff, w.qoff, n_verts, n_faces, status);
	FIND_LAUNCH_CHECK("surface_nets scan_kernel");
	return FIND_OK;
}

extern "C" int find_surface_nets_emit(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, const int64_t* n_verts,
									  const int64_t* n_faces, int64_t vcap, int64_t fcap, float* g_out, int32_t* faces, int32_t* status, void* ws, int64_t ws_bytes,
									  void* stream) {
	FIND_REQUIRE(!surface_nets::bad_dims(n_meshes, nx, ny, nz), "find_surface_nets_emit: bad sizes");
	FIND_REQUIRE(vcap >= 0 && vcap < (1ll << 30) && fcap >= 0 && fcap < (1ll << 33), "find_surface_nets_emit: bad capacities");
	if (n_meshes == 0) return FIND_OK;
	FIND_REQUIRE(values && n_verts && n_faces && status && ws, "find_surface_nets_emit: NULL argument");
	FIND_REQUIRE((g_out || vcap == 0) && (faces || fcap == 0), "find_surface_nets_emit: NULL argument");
	if (ws_bytes < find_surface_nets_ws_bytes(n_meshes, nx, ny, nz)) { set_error("find_surface_nets_emit: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	const Grid g = make_grid(nx, ny, nz);
	const Workspace w(ws, n_meshes, g);
	hipLaunchKernelGGL(vertex_kernel, dim3((unsigned)cdiv(g.cells, SN_BLOCK), (unsigned)n_meshes), dim3(SN_BLOCK), 0, s, values, iso, g, w.voff, vcap, w.cellmap, g_out);
	FIND_LAUNCH_CHECK("surface_nets vertex_kernel");
	hipLaunchKernelGGL(face_kernel, dim3((unsigned)g.nb, (unsigned)n_meshes), dim3(SN_BLOCK), 0, s, values, iso, g, w.qoff, w.cellmap, fcap, faces);
	FIND_LAUNCH_CHECK("surface_nets face_kernel");
	hipLaunchKernelGGL(pad_kernel, dim3((unsigned)std::max<int64_t>(1, cdiv(std::max(vcap, fcap), SN_BLOCK)), (unsigned)n_meshes), dim3(SN_BLOCK), 0, s, n_verts,
					   n_faces, vcap, fcap, g_out, faces, status);
	FIND_LAUNCH_CHECK("surface_nets pad_kernel");
	return FIND_OK;
}

extern "C" int find_surface_nets_bwd(const float* values, float iso, int64_t n_meshes, int64_t nx, int64_t ny, int64_t nz, const int32_t* cellmap,
									 const float* grad_g, int64_t vcap, float* grad_values, float* grad_iso, void* ws, int64_t ws_bytes, void* stream) {
	FIND_REQUIRE(!surface_nets::bad_dims(n_meshes, nx, ny, nz), "find_surface_nets_bwd: bad sizes");
	FIND_REQUIRE(vcap >= 0 && vcap < (1ll << 30), "find_surface_nets_bwd: bad capacities");
	if (n_meshes == 0) return FIND_OK;
	FIND_REQUIRE(values && cellmap && grad_values && grad_iso && ws && (grad_g || vcap == 0), "find_surface_nets_bwd: NULL argument");
	if (ws_bytes < find_surface_nets_bwd_ws_bytes(n_meshes, nx, ny, nz)) { set_error("find_surface_nets_bwd: workspace too small"); return FIND_EWORKSPACE; }
	hipStream_t s = (hipStream_t)stream;
	const Grid g = make_grid(nx, ny, nz);
	double* part = reinterpret_cast<double*>(ws);
	hipLaunchKernelGGL(grad_kernel, dim3((unsigned)g.nb, (unsigned)n_meshes), dim3(SN_BLOCK), 0, s, values, iso, g, cellmap, grad_g, vcap, grad_values, part);
	FIND_LAUNCH_CHECK("surface_nets grad_kernel");
	hipLaunchKernelGGL(iso_kernel, dim3((unsigned)n_meshes), dim3(SN_BLOCK), 0, s, g.nb, part, grad_iso);
	FIND_LAUNCH_CHECK("surface_nets iso_kernel");
	return FIND_OK;
}
