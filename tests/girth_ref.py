"""The tape-girth rule of include/find_hip.h (find_section_hull_*) restated in torch and numpy, in the dtype of the vertices (float64 for the
tests' reference, float32 to measure what that format can reach), and the meshes the girth tests share.  The crossing points follow the
formula order of measure_ref.plane_sections_ref and are differentiable in the vertices and in all four plane components; the corners are
found on the detached 2-D points by a strict monotone chain after np.unique; the girth is the sum of |h_i - h_i+1| over the differentiable
3-D points.  Nothing here reads the code under test."""
import math

import numpy as np
import torch


def basis(n):
	"""a: the coordinate axis of the smallest |n_k| (lowest index on ties); e1 = normalize(n x a), e2 = n x e1."""
	k = int(torch.argmin(n.abs()))   # (the first of equal minima)
	a = torch.zeros(3, dtype=n.dtype)
	a[k] = 1
	e1 = torch.linalg.cross(n, a)
	e1 = e1 / e1.norm()
	return e1, torch.linalg.cross(n, e1)


def crossing_points(verts, faces, plane):
	"""verts (V, 3), faces (F, 3) integers, plane (4): the crossing points (M, 3), two per crossing face, and the number of crossing faces."""
	V = verts.shape[0]
	faces = faces.long()
	i0, i1, i2 = faces.unbind(-1)
	valid = ((faces >= 0) & (faces < V)).all(-1) & (i0 != i1) & (i1 != i2) & (i0 != i2)
	tri = verts[faces[valid]]                                            # (F', corner, xyz)
	n, d = plane[:3], plane[3]
	s = (n[0] * tri[..., 0] + n[1] * tri[..., 1]) + n[2] * tri[..., 2] - d   # the order of the kernel's fma chain
	above = s >= 0
	crosses = ~((above[:, 0] == above[:, 1]) & (above[:, 1] == above[:, 2]))
	pts = []
	for a, b in ((0, 1), (1, 2), (2, 0)):
		idx = torch.nonzero(above[:, a] != above[:, b])[:, 0]
		a_up = above[idx, a]
		v_a, v_b, s_a, s_b = tri[idx, a], tri[idx, b], s[idx, a], s[idx, b]
		lo, hi = torch.where(a_up[:, None], v_b, v_a), torch.where(a_up[:, None], v_a, v_b)
		s_lo, s_hi = torch.where(a_up, s_b, s_a), torch.where(a_up, s_a, s_b)
		t = s_lo / (s_lo - s_hi)
		pts.append(lo + t[:, None] * (hi - lo))
	return torch.cat(pts), int(crosses.sum())


def strict_chain(xy):
	"""Andrew's monotone chain on distinct points xy (M, 2) float64, sorted or not: the indices of the strict corners, counter-clockwise from
	the lexicographically smallest point (collinear points are dropped: cross <= 0 pops)."""
	order = np.lexsort((xy[:, 1], xy[:, 0]))

	def cross(o, a, b):
		return (xy[a, 0] - xy[o, 0]) * (xy[b, 1] - xy[o, 1]) - (xy[a, 1] - xy[o, 1]) * (xy[b, 0] - xy[o, 0])
	lower, upper = [], []
	for i in order:
		while len(lower) >= 2 and cross(lower[-2], lower[-1], i) <= 0:
			lower.pop()
		lower.append(i)
	for i in order[::-1]:
		while len(upper) >= 2 and cross(upper[-2], upper[-1], i) <= 0:
			upper.pop()
		upper.append(i)
	return lower[:-1] + upper[:-1] if len(order) > 1 else list(order)


def hull_of_points(p, normal):
	"""p (M, 3) differentiable, normal (3): (girth, corner indices into p in order)."""
	if p.shape[0] == 0:
		return p.sum() * 0, []
	e1, e2 = basis(normal.detach())
	q = p.detach()
	xy = torch.stack([q @ e1, q @ e2], 1).double().numpy()
	xy, first = np.unique(xy, axis=0, return_index=True)
	h = [int(first[i]) for i in strict_chain(xy)]
	if len(h) < 2:
		return p.sum() * 0, h
	hp = p[h]
	return (hp - hp.roll(-1, 0)).norm(dim=1).sum(), h   # (two corners: there and back)


def section_hulls_ref(verts, faces, planes, return_points=False):
	"""verts (N, V, 3); faces (F, 3) or (N, F, 3); planes (P, 4) or (N, P, 4), in verts' dtype.  Returns girth (N, P) in that dtype,
	n_hull (N, P) and count (N, P) int64 (and the corners' points, a list of lists of (n_hull, 3) tensors)."""
	N = verts.shape[0]
	P = planes.shape[-2]
	planes = planes.to(verts.dtype)
	rows, n_hull, count, points = [], torch.zeros(N, P, dtype=torch.long), torch.zeros(N, P, dtype=torch.long), []
	for n in range(N):
		f = faces if faces.dim() == 2 else faces[n if faces.shape[0] > 1 else 0]
		row, prow = [], []
		for k in range(P):
			pl = planes[k] if planes.dim() == 2 else planes[n if planes.shape[0] > 1 else 0, k]
			p, cnt = crossing_points(verts[n], f, pl)
			g, h = hull_of_points(p, pl[:3])
			row.append(g)
			prow.append(p[h].detach())
			n_hull[n, k], count[n, k] = len(h), cnt
		rows.append(torch.stack(row))
		points.append(prow)
	out = (torch.stack(rows), n_hull, count)
	return out + (points,) if return_points else out


# ------------------------------------------------------------------ meshes
def arched(v, b=0.045, c=0.04, k=0.6):
	"""The template with an arch: for vertices with z < 0, z += k c max(0, 1 - (y / b)^2) (-z / c).  x is unchanged."""
	v = v.clone()
	lift = k * c * (1 - (v[:, 1] / b) ** 2).clamp(min=0)
	v[:, 2] = torch.where(v[:, 2] < 0, v[:, 2] + lift * (-v[:, 2] / c), v[:, 2])
	return v


def two_feet(v, f, b=0.045):
	"""Two copies of a mesh in one, the second shifted by 3 b in y: a plane normal to x cuts two loops."""
	return torch.cat([v, v + torch.tensor([0., 3 * b, 0.], dtype=v.dtype)]), torch.cat([f, f + v.shape[0]])


def ring_strip(two_k, h=0.25, pulled=False, dtype=torch.float32):
	"""2K vertices at angle pi i / K on the unit circle, z = +h for even i and -h for odd i, faces (i, i + 1, i + 2) mod 2K: the plane z = 0
	crosses all 2K faces in the 2K corners of a regular polygon, girth 2K sin(pi / K).  pulled: every third vertex at radius 0.7."""
	i = torch.arange(two_k)
	ang = (math.pi / (two_k // 2)) * i.double()
	r = torch.where((i % 3 == 0) & pulled, 0.7, 1.0).double()
	z = torch.where(i % 2 == 0, h, -h).double()
	v = torch.stack([r * torch.cos(ang), r * torch.sin(ang), z], 1).to(dtype)
	f = torch.stack([i, (i + 1) % two_k, (i + 2) % two_k], 1)
	return v, f


def ring_girth(two_k):
	"""The crossing points of the unit ring strip are the midpoints of its 2K edges (i, i + 1): a regular 2K-gon of circumradius cos(pi / 2K)."""
	return two_k * math.sin(2 * math.pi / two_k)   # = 2K sin(pi / K)
