"""CPU: the scan-like test mesh has every feature the smoothness tests rely on, and the sparse smoothness restatement
(oracle.geom_ref.mesh_laplacian_smoothing_cot_sparse) equals the dense one in float64, values and autograd gradients."""
import pytest
import torch

from oracle import geom_ref as G
from scan_meshes import closed_mesh, mesh_features, open_irregular_mesh

SIZES = [63, 64, 65, 1002, 6890]


@pytest.mark.parametrize('V', SIZES + [50002])
def test_open_irregular_mesh_has_every_feature(V):
	v, f = open_irregular_mesh(V, seed=V)
	assert v.shape == (V, 3) and v.dtype == torch.float32
	assert int(f.min()) >= 0 and int(f.max()) < V
	feat = mesh_features(v, f)
	print(V, feat)
	assert feat['boundary_edges'] >= 3, feat              # the cut: a boundary loop
	assert feat['unused_vertices'] >= 2, feat             # the cut-off end and the isolated vertex
	assert feat['repeated_vertex_faces'] >= 1, feat
	assert feat['sliver_faces'] >= 1, feat
	assert feat['zero_length_edge_faces'] >= 1, feat
	assert feat['used_vertices_with_zero_rowsum'] >= 1, feat
	assert feat['obtuse_entries'] >= 1, feat              # irregular: negative cotangent weights


@pytest.mark.parametrize('V', [3, 63, 1002])
def test_closed_mesh_sizes(V):
	v, f = closed_mesh(V)
	assert v.shape == (V, 3) and int(f.max()) < V


def _tetrahedron():
	v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.3, 0.2, 1.1]])
	f = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
	return v, f


@pytest.mark.parametrize('case', ['tetrahedron', 'open1002', 'open63', 'closed65'])
def test_sparse_restatement_equals_dense_float64(case):
	if case == 'tetrahedron':
		v, f = _tetrahedron()
		verts = torch.stack([v, v * 1.3 + 0.05])
	else:
		V = int(case[-4:] if case.endswith('1002') else case[-2:])
		v, f = open_irregular_mesh(V, seed=3) if case.startswith('open') else closed_mesh(V)
		g = torch.Generator().manual_seed(V)
		verts = v[None] + 0.002 * torch.randn(2, V, 3, generator=g)
	edges = G.unique_edges(f)
	ga, gb = 0.7, -1.9   # distinct upstream gradients for the two terms
	out = {}
	for kind in ('dense', 'sparse'):
		x = verts.double().clone().requires_grad_(True)
		lap = G.mesh_laplacian_smoothing_cot(x, f) if kind == 'dense' else G.mesh_laplacian_smoothing_cot_sparse(x, f)
		edge = G.mesh_edge_loss(x, edges)
		(ga * lap + gb * edge).backward()
		out[kind] = (lap.item(), edge.item(), x.grad)
	(ld, ed, gd), (ls, es, gs) = out['dense'], out['sparse']
	assert abs(ld - ls) <= 1e-12 * max(1.0, abs(ld)), (ld, ls)
	assert ed == es
	assert (gd - gs).abs().max().item() <= 1e-12 * max(1.0, gd.abs().max().item())


def test_sparse_restatement_runs_in_float32():
	v, f = open_irregular_mesh(1002, seed=5)
	x = v[None].clone().requires_grad_(True)
	lap = G.mesh_laplacian_smoothing_cot_sparse(x, f)
	lap.backward()
	assert lap.dtype == torch.float32 and x.grad.dtype == torch.float32 and torch.isfinite(x.grad).all()
	x64 = v[None].double().requires_grad_(True)
	l64 = G.mesh_laplacian_smoothing_cot_sparse(x64, f)
	assert abs(lap.item() - l64.item()) < 1e-4 * abs(l64.item())


def _grad64(verts, faces, edges, ge, gl, drop_entry=None, drop_edge=None):
	"""float64 gradient of ge * edge + gl * lap; drop_entry = (vertex): its row of L loses one directed entry (in L V and in the row sum),
	drop_edge = (vertex): one edge leaves that vertex's neighbour sum (mesh 0 only) -- what a kernel that skipped one item would compute."""
	x = verts.double().clone().requires_grad_(True)
	N, V, _ = x.shape
	tot = 0
	for n in range(N):
		ent = G.cot_entries(x[n], faces)
		if n == 0 and drop_entry is not None:
			k = int((ent[0] == drop_entry).nonzero()[0, 0])
			keep = torch.arange(ent[0].shape[0]) != k
			ent = tuple(t[keep] for t in ent)
		lap, _ = G.laplacian_terms_sparse(x[n], faces, ent)
		tot = tot + lap.norm(dim=1).sum() / V
	a, b = x[:, edges[:, 0]], x[:, edges[:, 1]]
	if drop_edge is not None:
		k = int(((edges[:, 0] == drop_edge) | (edges[:, 1] == drop_edge)).nonzero()[0, 0])
		other = 1 if int(edges[k, 0]) == drop_edge else 0
		a, b = a.clone(), b.clone()
		# the dropped vertex's side of the edge is detached in mesh 0: its gradient misses that term, its neighbour's does not
		if other == 1:
			a[0, k] = a[0, k].detach()
		else:
			b[0, k] = b[0, k].detach()
	edge = ((a - b).norm(dim=-1) ** 2).sum(1).div(edges.shape[0]).sum() / N
	(ge * edge + gl * tot / N).backward()
	return x.grad


@pytest.mark.parametrize('kind,V,N', [('closed', 6890, 16), ('open', 65, 3)])
def test_one_missing_item_is_resolved_by_the_smoothness_bar(kind, V, N):
	"""Dropping ONE corner entry from one vertex's row of L, or one edge from one vertex's neighbour sum, moves the float64 gradient by
	at least 5 x the bar of test_gpu_smooth_f64 (C * e_fp32 + A on the vertices that test compares)."""
	import test_gpu_smooth_f64 as S
	verts, faces = S.make_case(kind, V, N, seed=V + N)
	edges = G.unique_edges(faces)
	keep = torch.ones(N, V, dtype=torch.bool)
	for n in range(N):
		keep[n] = ~S.undetermined(verts[n].double(), faces)[1]
	used = torch.zeros(V, dtype=torch.bool)
	used[faces.reshape(-1)] = True
	# each against the bar of the gradient it lands in: the pair with both upstream gradients, and the term alone
	for what, kw, (ge, gl) in [('corner entry', 'drop_entry', up) for up in S.UPSTREAM if up[1]] + \
							  [('edge', 'drop_edge', up) for up in S.UPSTREAM if up[0] and not up[1]]:
		_, _, d64 = S.reference(verts, faces, edges, ge, gl, torch.float64)
		_, _, d32 = S.reference(verts, faces, edges, ge, gl, torch.float32)
		g_own = _grad64(verts, faces, edges, ge, gl)
		assert (g_own - d64).abs().max().item() <= 1e-12 * d64.abs().max().item()
		scale = d64[keep].abs().max().item()
		bar = S.C_REL * (d32 - d64)[keep].abs().max().item() / scale + S.A_REL
		# a vertex of typical gradient that the GPU test compares
		mag = d64[0].norm(dim=1)
		cand = (keep[0] & used).nonzero()[:, 0]
		i = int(cand[(mag[cand] - mag[cand].median()).abs().argmin()])
		g = _grad64(verts, faces, edges, ge, gl, **{kw: i})
		move = (g - d64)[keep].abs().max().item() / scale
		print(f'[resolution {kind} V={V} N={N}] g_edge {ge} g_lap {gl}: dropping one {what} of vertex {i}: gradient moves {move:.3e} = {move / bar:.1f} x the bar {bar:.3e}')
		assert move >= 5 * bar, (what, move, bar)
