"""Test meshes shaped like a foot scan, for the smoothness tests (not product code).

open_irregular_mesh(V) has exactly V vertices: a jittered ellipsoid with one end cut off (a boundary loop, and the cut-off vertices left
in no face), plus
  - a degenerate face with a repeated vertex                    (Heron product 0: the 1e-12 clamp)
  - a sliver face whose Heron product is far below 1e-12        (the clamp, on a face of positive area)
  - a face with a zero-length edge (a vertex duplicated in place), opposite a vertex that is in no other face: its row of L sums to 0
  - vertices that are in no face                                 (row sum 0: the rowsum > 0 ? 1/rowsum : rowsum branch)
mesh_features() finds every one of these in a mesh, so a test can assert that they are there."""
import math

import numpy as np
import torch

HERON_EPS = 1e-12


def _grid(n):
	"""(rings, segs) of an ellipsoid with rings * segs + 2 <= n vertices, rings >= 3."""
	segs = max(3, int(math.sqrt(2.0 * n)))
	rings = max(3, (n - 2) // segs)
	while rings * segs + 2 > n and segs > 3:
		segs -= 1
		rings = max(3, (n - 2) // segs)
	return rings, segs


def closed_mesh(V):
	"""A closed, near-uniform ellipsoid of exactly V vertices (synthetic.template for the sizes it has; vertices beyond the grid are left
	in no face otherwise); V = 3 is a single triangle."""
	from find_amd import synthetic
	if V == 3:
		return torch.tensor([[0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.005, 0.017, 0.003]]), torch.tensor([[0, 1, 2]])
	if V in synthetic.TEMPLATE_GRIDS:
		return synthetic.template(V)
	rings, segs = _grid(V)
	v, f = synthetic.ellipsoid_mesh(rings, segs)
	extra = V - v.shape[0]
	return torch.cat([v, v[:extra] * 0.5]), f


def open_irregular_mesh(V, seed=0):
	"""verts (V,3) float32, faces (F,3) int64 as in the module docstring.  V >= 16."""
	from find_amd import synthetic
	assert V >= 16
	g = np.random.default_rng(seed)
	rings, segs = _grid(V - 5)
	v, f = synthetic.ellipsoid_mesh(rings, segs)
	v, f = v.numpy().astype(np.float64), f.numpy()
	# cut off the top: every face touching the pole or the first ring goes; those vertices stay, in no face
	cut = 1 + segs
	f = f[(f >= cut).all(1)]
	# jitter: a quarter of the mean edge length, so the triangles are irregular (some obtuse: negative cotangents)
	e = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
	v = v + g.uniform(-0.25, 0.25, v.shape) * e
	nv = v.shape[0]
	a, b, c = f[len(f) // 2]          # a face of the mesh, for the three special faces to sit on
	p, q = f[len(f) // 3][:2]
	# the sliver: apex on the segment a-b, lifted by 1e-4 of it; Heron product ~ (0.5 |ab| h)^2 = 2.5e-9 |ab|^4 << 1e-12
	ab = v[b] - v[a]
	nrm = np.cross(ab, v[c] - v[a])
	nrm /= np.linalg.norm(nrm)
	apex = v[a] + 0.37 * ab + 1e-4 * np.linalg.norm(ab) * nrm
	# the zero-length edge: a copy of p in place, and a vertex that is in this face only
	twin = v[p].copy()
	lone = v[p] + (v[q] - v[p]) * 0.5 + nrm * e
	isolated = v[cut + 3] * 1.1     # in no face at all
	v = np.concatenate([v, [apex, twin, lone, isolated]])
	i_apex, i_twin, i_lone = nv, nv + 1, nv + 2
	extra = [[a, a, c], [a, b, i_apex], [i_lone, i_twin, p]]
	f = np.concatenate([f, np.asarray(extra)])
	# exactly V vertices: any left over sit in no face
	pad = V - v.shape[0]
	assert pad >= 0
	v = np.concatenate([v, v[cut + 4:cut + 4 + pad] * 0.9])
	return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int64))


def mesh_features(verts, faces):
	"""Counts of the features of open_irregular_mesh in any mesh (float64 arithmetic on the given vertices)."""
	from oracle import geom_ref as G
	v = verts.double()
	f = faces.long()
	V = v.shape[0]
	hp, _ = G.heron_product(v, f)
	e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
	e, _ = e.sort(dim=1)
	ue, cnt = torch.unique(e, dim=0, return_counts=True)
	proper = ue[:, 0] != ue[:, 1]
	used = torch.zeros(V, dtype=torch.bool)
	used[f.reshape(-1)] = True
	rows, cols, w = G.cot_entries(v, f)
	rowsum = torch.zeros(V, dtype=torch.float64).index_add(0, rows, w)
	elen = (v[f[:, [1, 2, 0]]] - v[f]).norm(dim=-1)        # (F,3) edge lengths
	repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
	return {
		'boundary_edges': int(((cnt == 1) & proper).sum()),
		'unused_vertices': int((~used).sum()),
		'repeated_vertex_faces': int(repeated.sum()),
		'sliver_faces': int(((hp < HERON_EPS) & ~repeated & (elen.min(1).values > 0)).sum()),
		'zero_length_edge_faces': int(((elen == 0).any(1) & ~repeated).sum()),
		'used_vertices_with_zero_rowsum': int((used & (rowsum.abs() <= 1e-9 * w.abs().max())).sum()),
		'obtuse_entries': int((w < 0).sum()),
	}
