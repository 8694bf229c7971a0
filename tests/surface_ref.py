"""Reference of the point-to-surface distance (find_amd/csrc/surface.hip) in torch, on the CPU, in the dtype of its inputs (float64: the
truth; float32: what the same formulas give in the kernels' precision).  A helper of test_surface_host.py and test_gpu_surface.py, not a test.

The closest point on a triangle is found by its seven Voronoi regions (Ericson, Real-Time Collision Detection, 5.1.5), here with the six dot
products formed from the points themselves (ab.bp from bp = p - b, ...), not from the face's precomputed ones as the kernel forms them: another
route to the same point.  The search is a brute force over all faces, a chunk of queries at a time."""
import torch

SEVEN_TRIANGLE = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
# a point per region: inside, edges ab, ac, bc, corners a, b, c -- with its squared distance and the barycentrics of its closest point, all exact
SEVEN_POINTS = torch.tensor([[0.25, 0.25, 0.5], [0.5, -0.5, 0.], [-0.5, 0.5, 0.], [1., 1., 0.], [-1., -1., 0.], [2., -0.5, 0.], [-0.5, 2., 0.]])
SEVEN_DIST2 = torch.tensor([0.25, 0.25, 0.25, 0.5, 2., 1.25, 1.25])
SEVEN_BARY = torch.tensor([[0.5, 0.25, 0.25], [0.5, 0.5, 0.], [0.5, 0., 0.5], [0., 0.5, 0.5], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])


def _dot(x, y):
	return (x * y).sum(-1)


def _nz(x):
	return torch.where(x != 0, x, torch.ones_like(x))


def closest_vw(p, a, b, c):
	"""(v, w): the point of the closed triangle (a, b, c) nearest to p is a + v (b - a) + w (c - a).  All arguments (..., 3), broadcast."""
	ab, ac = b - a, c - a
	ap, bp, cp = p - a, p - b, p - c
	d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
	vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
	den = _nz(va + vb + vc)
	v, w = vb / den, vc / den                                  # inside
	zero, one = torch.zeros_like(v), torch.ones_like(v)
	# the regions in the reverse of Ericson's order: the test he makes first is applied last and wins
	m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)            # edge bc
	t = (d4 - d3) / _nz((d4 - d3) + (d5 - d6))
	v, w = torch.where(m, 1 - t, v), torch.where(m, t, w)
	m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)                      # edge ac
	v, w = torch.where(m, zero, v), torch.where(m, d2 / _nz(d2 - d6), w)
	m = (d6 >= 0) & (d5 <= d6)                                 # corner c
	v, w = torch.where(m, zero, v), torch.where(m, one, w)
	m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)                      # edge ab
	v, w = torch.where(m, d1 / _nz(d1 - d3), v), torch.where(m, zero, w)
	m = (d3 >= 0) & (d4 <= d3)                                 # corner b
	v, w = torch.where(m, one, v), torch.where(m, zero, w)
	m = (d1 <= 0) & (d2 <= 0)                                  # corner a
	v, w = torch.where(m, zero, v), torch.where(m, zero, w)
	return v, w


def closest_point(p, a, b, c):
	"""(closest point (..., 3), barycentrics (..., 3)) of p on the closed triangle (a, b, c)."""
	v, w = closest_vw(p, a, b, c)
	return a + v[..., None] * (b - a) + w[..., None] * (c - a), torch.stack([1 - v - w, v, w], -1)


def usable_faces(verts, faces):
	"""(F) bool: no -1 row, and (b - a) x (c - a) not exactly zero IN FLOAT32, whatever the dtype of verts: the set of faces is the kernel's."""
	ok = (faces >= 0).all(-1)
	f = faces.clamp(min=0).long()
	v = verts.float()
	a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
	return ok & (torch.linalg.cross(b - a, c - a) != 0).any(-1)


def point_face(points, verts, faces, chunk=None, far=None):
	"""Brute force over all usable faces.  points (P, 3), verts (V, 3), faces (F, 3) integer -> dict of dist2 (P), idx (P) int64 (the smallest
	index among equal distances; -1 and dist2 0 when no face is usable), closest (P, 3), bary (P, 3).
	far: a length; then also runner_up (P), the smallest squared distance among the faces whose closest point lies more than `far` from the
	winner's (inf if there is none) -- what the medial-axis test of test_gpu_surface.py reads."""
	P, F = points.shape[0], faces.shape[0]
	dt = points.dtype
	out = dict(dist2=torch.zeros(P, dtype=dt), idx=torch.full((P,), -1, dtype=torch.int64), closest=points.clone(), bary=torch.zeros(P, 3, dtype=dt))
	if far is not None:
		out['runner_up'] = torch.full((P,), float('inf'), dtype=dt)
	use = usable_faces(verts, faces) if F else torch.zeros(0, dtype=torch.bool)
	if P == 0 or not use.any():
		return out
	f = faces.clamp(min=0).long()
	a, b, c = verts[f[:, 0]][None], verts[f[:, 1]][None], verts[f[:, 2]][None]
	chunk = chunk or max(1, (1 << 21) // F)
	for s in range(0, P, chunk):
		p = points[s:s + chunk, None]
		cp, bary = closest_point(p, a, b, c)
		d = ((p - cp) ** 2).sum(-1).masked_fill(~use[None], float('inf'))
		best, k = d.min(1)
		k = d.argmin(1)   # (documented: the first of equal minima)
		rows = torch.arange(k.shape[0])
		out['dist2'][s:s + chunk], out['idx'][s:s + chunk] = best, k
		out['closest'][s:s + chunk], out['bary'][s:s + chunk] = cp[rows, k], bary[rows, k]
		if far is not None:
			apart = ((cp - cp[rows, k][:, None]) ** 2).sum(-1) > far * far
			out['runner_up'][s:s + chunk] = d.masked_fill(~apart, float('inf')).min(1).values
	return out


def dist2_to_face(points, verts, faces, idx):
	"""Squared distance of points (P, 3) to the faces idx (P) of the mesh."""
	f = faces[idx].long()
	cp, _ = closest_point(points, verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])
	return ((points - cp) ** 2).sum(-1)


def gradients(points, verts, faces, idx, bary, g):
	"""The gradient of sum_i g_i dist2_i with the barycentrics held constant (the envelope theorem: the closest point minimises the distance
	over the triangle): d_points (P, 3) = 2 g (p - c), d_verts (V, 3) with -2 g bary_k (p - c) added at the corners of face idx.  Rows with
	idx -1 give nothing."""
	ok = idx >= 0
	f = faces[idx.clamp(min=0)].long()
	c = (bary[..., None] * verts[f]).sum(1)
	gd = torch.where(ok[:, None], 2 * g[:, None] * (points - c), torch.zeros_like(points))
	d_verts = torch.zeros_like(verts)
	for k in range(3):
		d_verts.index_add_(0, f[:, k], -bary[:, k, None] * gd)
	return gd, d_verts
