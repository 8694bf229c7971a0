"""The smoothness kernels (cot_weights_kernel, smooth_fwd / bwd_kernel, smooth_finalize_kernel; FN.mesh_edge_and_laplacian and
FN.mesh_smoothness_loss) against float64, on a closed template and on an open, irregular, scan-like mesh (tests/scan_meshes.py: boundary
loop, vertices in no face, a repeated-vertex face, a sliver, a zero-length edge), at V = 3, 63 / 64 / 65 (partial SMOOTH_VPB = 64 blocks),
1 002, 6 890 and 3 x 50 002.  The float64 reference is the sparse restatement oracle.geom_ref.mesh_laplacian_smoothing_cot_sparse (equal
to the dense one: test_oracle_smooth_sparse), which runs at any V.

The bar follows test_gpu_mlp_f64: per tensor, e_hip <= C * e_fp32 + A, e_fp32 the same restatement in float32 measured against float64
(relative to the float64 tensor's largest entry for gradients and to the value for losses).

Exclusions.  Two kinds of vertex have a result float32 cannot determine:
  - a vertex of a face whose Heron product is within float32 rounding (16 u s^4, s the semi-perimeter) of the 1e-12 clamp: which side
    of the clamp the face lands on is a coin toss, and its cotangent weights jump;
  - a vertex whose |lap| is within K u of |(L V) * norm_w| + |V| (K = 512): the direction lap / |lap|, which the gradient carries, is
    rounding noise.
Such a vertex is left out of the gradient check together with its one-ring (their gradients read its lap direction); the loss values
keep every vertex.  At most 1 % of a mesh's vertices (or the 8 vertices of the built-in degenerate faces of a small mesh) may be
undetermined, and at most 5 % may be left out with the one-rings."""
import pytest
import torch

from oracle import geom_ref as G
from scan_meshes import closed_mesh, open_irregular_mesh

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
C_REL, A_REL = 4.0, 2e-7
K_LAP = 512.0
UPSTREAM = [(3.0, -0.7), (3.0, 0.0), (0.0, -0.7)]
SMALL_EXCLUDED = 8    # undetermined vertices a small mesh may have: the vertices of its three degenerate faces
RING_FRACTION = 0.05  # their one-rings (a pole of the latitude-longitude template has 82 neighbours)


def make_case(kind, V, N, seed):
	v, f = (open_irregular_mesh(V, seed=seed) if kind == 'open' else closed_mesh(V))
	g = torch.Generator().manual_seed(seed)
	e = (v[f[:, 0]] - v[f[:, 1]]).norm(dim=1).mean().item() if V > 3 else 0.01
	verts = (v[None].double() + 0.2 * e * torch.randn(N, V, 3, generator=g, dtype=torch.float64)).float()
	if kind == 'open':
		# keep the zero-length edge and the repeated vertex exact after the per-mesh jitter: the twin copies its vertex again
		ff = f[-1]
		verts[:, ff[1]] = verts[:, ff[2]]
	return verts, f


def undetermined(v64, faces):
	"""(vertex mask of results float32 cannot determine, its one-ring closure) for one mesh, float64 arithmetic."""
	V = v64.shape[0]
	f = faces.long()
	hp, s = G.heron_product(v64, f)
	tie = (hp - 1e-12).abs() <= 16 * U32 * s ** 4
	bad = torch.zeros(V, dtype=torch.bool)
	bad[f[tie].reshape(-1)] = True
	lap, lvn = G.laplacian_terms_sparse(v64, f)
	lap, lvn = lap.detach(), lvn.detach()
	bad |= lap.norm(dim=1) <= K_LAP * U32 * (lvn.norm(dim=1) + v64.norm(dim=1))
	ring = bad.clone()
	touch = bad[f].any(1)
	ring[f[touch].reshape(-1)] = True
	return bad, ring


def reference(verts, faces, edges, ge, gl, dtype, w=None):
	"""(edge, lap, d_verts) of the sparse restatement in `dtype`, upstream gradients ge, gl (or one scalar loss w_edge, w_lap)."""
	x = verts.to(dtype).clone().requires_grad_(True)
	lap = G.mesh_laplacian_smoothing_cot_sparse(x, faces)
	edge = G.mesh_edge_loss(x, edges)
	(ge * edge + gl * lap).backward()
	return edge.detach().double(), lap.detach().double(), x.grad.double()


def compare(name, hip, ref64, ref32, mask=None):
	"""e_hip <= C e_fp32 + A, relative to the float64 tensor's largest entry; mask (N, V): the vertices to compare."""
	if mask is not None:
		hip, ref64, ref32 = hip[mask], ref64[mask], ref32[mask]
	s = max(ref64.abs().max().item(), 1e-300)
	e_hip = (hip - ref64).abs().max().item() / s
	e32 = (ref32 - ref64).abs().max().item() / s
	bar = C_REL * e32 + A_REL
	print(f'  {name}: e_hip {e_hip:.3e}  e_fp32 {e32:.3e}  bar {bar:.3e}  ({e_hip / bar:.2f} of it)')
	assert e_hip <= bar, (name, e_hip, e32, bar)


def check_case(verts, faces, hip_fn, label):
	"""hip_fn(verts, ge, gl) -> (edge, lap, d_verts) for the edge / Laplacian pair, hip_fn(verts, None, None, w_edge, w_lap) for the
	scalar loss.  Everything measured is printed."""
	N, V, _ = verts.shape
	edges = G.unique_edges(faces)
	v64 = verts.double()
	keep = torch.ones(N, V, dtype=torch.bool)
	nbad = n_ring = 0
	for n in range(N):
		b, r = undetermined(v64[n], faces)
		keep[n] = ~r
		nbad, n_ring = max(nbad, int(b.sum())), max(n_ring, int(r.sum()))
	print(f'[smooth {label}] V={V} N={N}: {nbad} undetermined vertices, {n_ring} left out of the gradient check (worst mesh)')
	assert nbad <= max(0.01 * V, SMALL_EXCLUDED), (nbad, V)
	assert n_ring <= max(RING_FRACTION * V, 3 * SMALL_EXCLUDED), (n_ring, V)
	# distinct upstream gradients of the two terms, then each term alone (the Laplacian's float32 error, which cancellation in
	# (L V) * norm_w - V makes large, would hide an error in the edge term's gradient)
	for ge, gl in UPSTREAM:
		e64, l64, d64 = reference(verts, faces, edges, ge, gl, torch.float64)
		e32, l32, d32 = reference(verts, faces, edges, ge, gl, torch.float32)
		he, hl, hd = hip_fn(verts, ge, gl)
		if ge and gl:
			compare('edge loss', he.reshape(1, 1), e64.reshape(1, 1), e32.reshape(1, 1))
			compare('laplacian loss', hl.reshape(1, 1), l64.reshape(1, 1), l32.reshape(1, 1))
		compare(f'd_verts (g_edge {ge}, g_lap {gl})', hd, d64, d32, keep)
	we, wl = 10.0, 0.1   # MeshSmoothnessLoss's weights, through the one-scalar entry point
	s64 = we * e64 + wl * l64
	s32 = we * e32 + wl * l32
	hs, hds = hip_fn(verts, None, None, we, wl)
	_, _, ds64 = reference(verts, faces, edges, we, wl, torch.float64)
	_, _, ds32 = reference(verts, faces, edges, we, wl, torch.float32)
	compare('smoothness loss', hs.reshape(1, 1), s64.reshape(1, 1), s32.reshape(1, 1))
	compare('d_verts (smoothness loss)', hds, ds64, ds32, keep)


def hip_smooth(faces):
	from find_amd import functional as FN
	fc = faces.cuda()

	def run(verts, ge, gl, w_edge=None, w_lap=None):
		topo = FN.MeshTopology.get(fc, verts.shape[1])
		x = verts.clone().cuda().requires_grad_(True)
		if w_edge is None:
			e, l = FN.mesh_edge_and_laplacian(x, topo)
			(ge * e + gl * l).backward()
			return e.detach().double().cpu(), l.detach().double().cpu(), x.grad.double().cpu()
		loss = FN.mesh_smoothness_loss(x, topo, w_edge=w_edge, w_lap=w_lap)
		loss.backward()
		return loss.detach().double().cpu(), x.grad.double().cpu()
	return run


CASES = [(kind, V, N) for kind in ('open', 'closed') for V in (3, 63, 64, 65, 1002, 6890) for N in (1, 3, 16)
		 if not (kind == 'open' and V == 3)] + [('open', 50002, 3), ('closed', 50002, 3)]


@pytest.mark.parametrize('kind,V,N', CASES)
def test_smoothness_vs_float64(kind, V, N):
	verts, faces = make_case(kind, V, N, seed=V + N)
	check_case(verts, faces, hip_smooth(faces), f'{kind}')
