"""The section rule of include/find_hip.h (find_plane_sections_*) and the extents (find_extents_*) restated in torch, in the dtype of the
vertices (float64 for the tests' reference, float32 to measure what that format can reach): a vectorised `where` formulation over
(N, P, F) that autograd differentiates.  Nothing here reads the code under test."""
import torch


def _expand(t, N, tail):
	"""(tail) or (1 | N, tail) -> (N, tail)"""
	if t.dim() == len(tail):
		t = t[None]
	return t.expand((N,) + tuple(t.shape[1:]))


def plane_sections_ref(verts, faces, planes):
	"""verts (N, V, 3); faces (F, 3) or (N, F, 3) integers (-1 rows, indices outside [0, V) and repeated vertices contribute nothing); planes
	(P, 4) or (N, P, 4) rows (nx, ny, nz, d).  Returns perimeter (N, P) in verts' dtype and count (N, P) int64."""
	N, V, _ = verts.shape
	faces = _expand(faces.long(), N, (0, 3))                       # (N, F, 3)
	planes = _expand(planes.to(verts.dtype), N, (0, 4))            # (N, P, 4)
	i0, i1, i2 = faces.unbind(-1)
	valid = ((faces >= 0) & (faces < V)).all(-1) & (i0 != i1) & (i1 != i2) & (i0 != i2)
	safe = torch.where(valid[..., None], faces, torch.zeros_like(faces))
	tri = torch.gather(verts, 1, safe.reshape(N, -1, 1).expand(-1, -1, 3)).reshape(N, -1, 3, 3)   # (N, F, corner, xyz)
	n, d = planes[..., :3], planes[..., 3]
	# s (N, P, F, corner) = (nx x + ny y) + nz z - d, the order of the kernel's fma chain
	t_ = tri[:, None]
	s = (n[:, :, None, None, 0] * t_[..., 0] + n[:, :, None, None, 1] * t_[..., 1]) + n[:, :, None, None, 2] * t_[..., 2] - d[:, :, None, None]
	above = s >= 0
	crosses = valid[:, None] & ~((above[..., 0] == above[..., 1]) & (above[..., 1] == above[..., 2]))
	points, edge_cross = [], []
	for a, b in ((0, 1), (1, 2), (2, 0)):
		ec = above[..., a] != above[..., b]
		a_up = above[..., a]
		v_a, v_b = t_[:, :, :, a].expand(-1, s.shape[1], -1, -1), t_[:, :, :, b].expand(-1, s.shape[1], -1, -1)
		lo = torch.where(a_up[..., None], v_b, v_a)
		hi = torch.where(a_up[..., None], v_a, v_b)
		s_lo = torch.where(a_up, s[..., b], s[..., a])
		s_hi = torch.where(a_up, s[..., a], s[..., b])
		den = torch.where(ec, s_lo - s_hi, -torch.ones_like(s_lo))   # (< 0 on a crossing edge)
		t = torch.where(ec, s_lo, torch.zeros_like(s_lo)) / den
		points.append(lo + t[..., None] * (hi - lo))
		edge_cross.append(ec)
	p01, p12, p20 = points
	# exactly two edges of a crossing face cross: the segment joins their points
	diff = torch.where(~edge_cross[0][..., None], p12 - p20, torch.where(~edge_cross[1][..., None], p01 - p20, p01 - p12))
	sq = (diff * diff).sum(-1)
	pos = crosses & (sq > 0)   # a segment of length 0 (a plane through one vertex): masked out, not norm's subgradient
	length = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
	return length.sum(-1), crosses.sum(-1)


def extents_ref(verts, dirs, v_len=None):
	"""lo, hi (N, D) and arg_lo, arg_hi (N, D) int64 of dir . v over the first v_len[n] rows; ties to the smallest index; v_len 0: 0, 0, -1, -1."""
	N, V, _ = verts.shape
	dirs = torch.as_tensor(dirs, dtype=verts.dtype)
	lo, hi, alo, ahi = [], [], [], []
	for n in range(N):
		k = V if v_len is None else int(v_len[n])
		if k == 0:
			z = torch.zeros(dirs.shape[0], dtype=verts.dtype)
			m1 = torch.full((dirs.shape[0],), -1, dtype=torch.long)
			lo.append(z); hi.append(z); alo.append(m1); ahi.append(m1)
			continue
		v = verts[n, :k]
		s = (dirs[:, None, 0] * v[None, :, 0] + dirs[:, None, 1] * v[None, :, 1]) + dirs[:, None, 2] * v[None, :, 2]   # (D, k)
		first = torch.arange(k)[None].expand_as(s)
		mn, mx = s.min(1).values, s.max(1).values
		i_lo = torch.where(s == mn[:, None], first, torch.full_like(first, k)).min(1).values
		i_hi = torch.where(s == mx[:, None], first, torch.full_like(first, k)).min(1).values
		lo.append(torch.gather(s, 1, i_lo[:, None])[:, 0]); hi.append(torch.gather(s, 1, i_hi[:, None])[:, 0])
		alo.append(i_lo); ahi.append(i_hi)
	return torch.stack(lo), torch.stack(hi), torch.stack(alo), torch.stack(ahi)


def foot_measurements_ref(verts, faces, length_axis=(1., 0., 0.), width_axis=(0., 1., 0.), fractions=(0.68, 0.50), v_len=None):
	"""(N, 2 + G): length, width and the girths at the fractions of the foot's own length from the heel, by the two functions above."""
	la = torch.tensor(length_axis, dtype=verts.dtype)
	lo, hi, _, _ = extents_ref(verts, [length_axis, width_axis], v_len)
	size = hi - lo
	d = lo[:, :1] + torch.tensor(fractions, dtype=verts.dtype)[None] * size[:, :1]
	planes = torch.cat([la.expand(verts.shape[0], len(fractions), 3), d[..., None]], -1)
	girth, _ = plane_sections_ref(verts, faces, planes)
	return torch.cat([size, girth], 1)


def ellipse_perimeter(a, b, n=200001):
	"""Perimeter of the ellipse of semi-axes a, b by the trapezoid rule over a full period (spectrally accurate), float64."""
	th = torch.arange(n, dtype=torch.float64) * (2 * torch.pi / n)
	return float(torch.sqrt((a * torch.sin(th)) ** 2 + (b * torch.cos(th)) ** 2).sum() * (2 * torch.pi / n))


def octahedron(dtype=torch.float64):
	"""Vertices +-e_i (0: +x, 1: -x, 2: +y, 3: -y, 4: +z, 5: -z), eight outward faces."""
	v = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=dtype)
	f = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
	return v, f


def cube(dtype=torch.float64):
	"""The unit cube [0, 1]^3, twelve outward triangles; faces 0, 1 are the bottom z = 0, faces 2, 3 the top z = 1."""
	v = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=dtype)
	f = torch.tensor([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]])
	return v, f
