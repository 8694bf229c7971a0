"""A numpy restatement of the generalised winding number as include/find_hip.h defines it (find_winding_fwd), the zero rules included.  A helper
of test_inside_host.py and test_gpu_inside.py, not a test.

With A = a - p, B = b - p, C = c - p formed in `dtype`:  det = A . (B x C),  den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|,
Omega = 2 atan2(det, den),  w = sum Omega / 4 pi, the sum in float64 whatever the dtype.  A face contributes exactly 0 when it is a -1 row or
has an index outside [0, V), when a corner is at the query (a zero length) and when det == 0 exactly.  det is formed product by product in
the order written in det() below: nothing else is prescribed bit for bit, and the float32 evaluation then decides det == 0, and its sign
on a face the query lies ON, as any other float32 evaluation in that order does."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

OCTANT = (np.array([[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]), np.array([[0, 1, 2]]))
CUBE_VERTS = np.array([[x, y, z] for x in (0., 1.) for y in (0., 1.) for z in (0., 1.)])   # vertex 4 x + 2 y + z
# two triangles per side, outward orientation
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def det(A, B, C):
	nx = B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1]
	ny = B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2]
	nz = B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]
	return (A[..., 0] * nx + A[..., 1] * ny) + A[..., 2] * nz


def solid_angles(points, a, b, c, dtype):
	"""(P, F) in `dtype`: the solid angle of every face (a, b, c: (F, 3)) at every point (P, 3), 0 by the zero rules."""
	p = points.astype(dtype)[:, None, :]
	A, B, C = a.astype(dtype)[None] - p, b.astype(dtype)[None] - p, c.astype(dtype)[None] - p
	la, lb, lc = (np.sqrt((X * X).sum(-1)) for X in (A, B, C))
	d = det(A, B, C)
	den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
	om = dtype(2) * np.arctan2(d, den)
	assert om.dtype == dtype
	return np.where((la == 0) | (lb == 0) | (lc == 0) | (d == 0), dtype(0), om)


def valid_faces(faces, n_verts):
	faces = np.asarray(faces)
	return ((faces >= 0) & (faces < n_verts)).all(-1)


def winding(points, verts, faces, dtype=np.float64, pairs_per_chunk=1 << 20, threads=8):
	"""w (P,) float64 of points (P, 3) about the mesh verts (V, 3), faces (F, 3) (integer; -1 rows and out-of-range rows do not count): the
	per-face arithmetic in `dtype`, the sum over the faces in float64."""
	points, verts, faces = np.asarray(points), np.asarray(verts), np.asarray(faces).reshape(-1, 3)
	dtype = np.dtype(dtype).type
	f = faces[valid_faces(faces, verts.shape[0])].astype(np.int64)
	P = points.shape[0]
	out = np.zeros(P, np.float64)
	if P == 0 or f.shape[0] == 0:
		return out
	a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
	step = max(1, pairs_per_chunk // f.shape[0])

	def part(s):
		out[s:s + step] = solid_angles(points[s:s + step], a, b, c, dtype).astype(np.float64).sum(1) / (4 * np.pi)
	starts = range(0, P, step)
	if len(starts) > 1 and threads > 1:
		with ThreadPoolExecutor(max_workers=threads) as ex:
			list(ex.map(part, starts))
	else:
		for s in starts:
			part(s)
	return out


def box_points(verts, n, pad, seed):
	"""n points uniform in the box of verts grown by pad on every side, float32."""
	rng = np.random.RandomState(seed)
	lo, hi = verts.min(0) - pad, verts.max(0) + pad
	return (lo + rng.rand(n, 3) * (hi - lo)).astype(np.float32)


def without_top(verts, faces, share=0.15):
	"""The faces whose centroid is not in the top `share` of the mesh's z range: a mesh open at the top, as a scan is at the ankle."""
	z = verts[faces].mean(1)[:, 2]
	return faces[z <= verts[:, 2].max() - share * (verts[:, 2].max() - verts[:, 2].min())]


def exact_volume(verts, faces):
	v = np.asarray(verts, np.float64)
	return (v[faces[:, 0]] * np.cross(v[faces[:, 1]], v[faces[:, 2]])).sum() / 6.
