"""The z-clip reference of the split mode (find_render_params.clip_faces = 1), local to the tests, and its analytic checks (CPU).

PyTorch3D's rasterize_meshes clips a face that straddles the plane z = z_clip (clip.py, cull_to_frustum=False): with one vertex behind
the plane the face becomes a quad, split into two triangles, with two behind it becomes one triangle, with three it is culled.  The
rasteriser then works on the clipped triangles; pix_to_face and the barycentrics are converted back to the original face.  clip_split
below states that on an already projected mesh (x_ndc, y_ndc, z_view per vertex): it is written in torch so that the gradient tests
differentiate through it, and evaluated in float64 for values.  Its vertex order and quad diagonal are the library's:
p1 the vertex alone on its side of the plane, p2 and p3 following it cyclically, q4 on edge p1 p2, q5 on edge p1 p3;
one behind: (q4, p2, p3) in slot f and (q4, p3, q5) in slot F + f; two behind: (p1, q4, q5) in slot f.
The output feeds the unmodified oracle (oracle.render_ref.rasterize / silhouette / torch_fragments): every slot is a face of its own
with three vertices of its own."""
import numpy as np
import torch


def clip_structure(z, faces, zc):
	"""Discrete part (numpy): z (n_img, V) view depths, faces (F, 3) or (n_img, F, 3).  Returns, per image and slot of 2F, the original
	vertex ids (A, B) of the two ends of the edge each sub-vertex lies on (A == B: an original vertex), its local indices (la, lb) in the
	face, and whether the slot holds a triangle."""
	z = np.asarray(z, np.float64)
	n_img = z.shape[0]
	faces = np.asarray(faces, np.int64)
	fc = np.broadcast_to(faces, (n_img,) + faces.shape[-2:])
	F = fc.shape[1]
	zf = np.take_along_axis(z[:, None, :].repeat(F, 1), fc, axis=2)   # (n_img, F, 3)
	bh = zf < zc
	nb = bh.sum(-1)
	p1 = np.where(nb == 1, np.argmax(bh, -1), np.argmax(~bh, -1))
	p2, p3 = (p1 + 1) % 3, (p1 + 2) % 3
	la = np.zeros((n_img, 2 * F, 3), np.int64)
	lb = np.zeros((n_img, 2 * F, 3), np.int64)
	live = np.zeros((n_img, 2 * F), bool)
	ident = np.arange(3)
	for sl, cond, a, b in (
			(0, nb == 0, [ident[0], ident[1], ident[2]], [ident[0], ident[1], ident[2]]),
			(0, nb == 1, [p1, p2, p3], [p2, p2, p3]),
			(1, nb == 1, [p1, p3, p1], [p2, p3, p3]),
			(0, nb == 2, [p1, p2, p3], [p1, p1, p1])):
		s = slice(sl * F, (sl + 1) * F)
		for k in range(3):
			la[:, s, k] = np.where(cond, a[k], la[:, s, k])
			lb[:, s, k] = np.where(cond, b[k], lb[:, s, k])
		live[:, s] |= cond
	fc2 = np.concatenate([fc, fc], 1)
	A = np.take_along_axis(fc2, la, axis=2)
	B = np.take_along_axis(fc2, lb, axis=2)
	return A, B, la, lb, live


def clip_split(vproj, faces, zc):
	"""vproj (n_img, V, 3) torch -> (vs (n_img, 6F, 3): three vertices of its own per slot, fs (n_img, 2F, 3) int64 with -1 for an empty
	slot, conv (n_img, 2F, 3, 3): original barycentrics = sub-triangle barycentrics @ conv, live (n_img, 2F))."""
	n_img, V, _ = vproj.shape
	A, B, la, lb, live = clip_structure(vproj[..., 2].detach().cpu().numpy(), faces, zc)
	F2 = A.shape[1]
	At, Bt = torch.from_numpy(A).reshape(n_img, -1), torch.from_numpy(B).reshape(n_img, -1)
	va = torch.gather(vproj, 1, At[..., None].expand(-1, -1, 3))
	vb = torch.gather(vproj, 1, Bt[..., None].expand(-1, -1, 3))
	same = (At == Bt)[..., None]
	za, zb = va[..., 2:3], vb[..., 2:3]
	dz = torch.where(same, torch.ones_like(za), zb - za)
	w = torch.where(same, torch.zeros_like(za), (zc - za) / dz)
	xy = ((1 - w) * va[..., :2] * za + w * vb[..., :2] * zb) / zc
	xy = torch.where(same, va[..., :2], xy)
	z = torch.where(same, za, torch.full_like(za, zc))
	vs = torch.cat([xy, z], -1)
	fs = torch.arange(3 * F2).view(1, F2, 3).repeat(n_img, 1, 1)
	fs[~torch.from_numpy(live)] = -1
	eye = torch.eye(3, dtype=vproj.dtype)
	ea, eb = eye[torch.from_numpy(la)], eye[torch.from_numpy(lb)]   # (n_img, 2F, 3, 3)
	conv = (1 - w.view(n_img, F2, 3, 1)) * ea + w.view(n_img, F2, 3, 1) * eb
	return vs, fs, conv, live


def bary_perspective(vs3, px, py):
	"""Perspective-correct barycentrics of triangles vs3 (..., 3 verts, 3) at NDC points (px, py) (float64 numpy)."""
	x, y, z = vs3[..., 0], vs3[..., 1], vs3[..., 2]

	def edge(qx, qy, ax, ay, bx, by):
		return (qx - ax) * (by - ay) - (qy - ay) * (bx - ax)
	area = edge(x[..., 2], y[..., 2], x[..., 0], y[..., 0], x[..., 1], y[..., 1])
	w0 = edge(px, py, x[..., 1], y[..., 1], x[..., 2], y[..., 2]) / area
	w1 = edge(px, py, x[..., 2], y[..., 2], x[..., 0], y[..., 0]) / area
	w2 = edge(px, py, x[..., 0], y[..., 0], x[..., 1], y[..., 1]) / area
	t = np.stack([w0 * z[..., 1] * z[..., 2], z[..., 0] * w1 * z[..., 2], z[..., 0] * z[..., 1] * w2], -1)
	return t / t.sum(-1, keepdims=True)


def _one(v3, zc=0.01):
	vproj = torch.tensor(np.asarray(v3, np.float64)[None])
	return clip_split(vproj, torch.tensor([[0, 1, 2]]), zc)


def _project(P, s=1.7320508075688772):
	P = np.asarray(P, np.float64)
	return np.stack([s * P[:, 0] / P[:, 2], s * P[:, 1] / P[:, 2], P[:, 2]], -1)


def _view(vs):
	"""Back from (x_ndc, y_ndc, z) to view space (x z / s, y z / s, z)."""
	s = 1.7320508075688772
	return np.stack([vs[..., 0] * vs[..., 2] / s, vs[..., 1] * vs[..., 2] / s, vs[..., 2]], -1)


def test_zero_vertices_behind_keeps_the_face():
	P = [[0.01, 0.0, 0.3], [0.0, 0.02, 0.31], [-0.01, -0.01, 0.29]]
	vs, fs, conv, live = _one(_project(P))
	assert live.tolist() == [[True, False]]
	assert np.array_equal(vs[0, :3].numpy(), _project(P))
	assert np.array_equal(conv[0, 0].numpy(), np.eye(3))


def test_three_vertices_behind_culls_the_face():
	P = [[0.01, 0.0, 0.005], [0.0, 0.02, 0.006], [-0.01, -0.01, -0.2]]
	vs, fs, conv, live = _one(_project(P))
	assert live.tolist() == [[False, False]] and (fs == -1).all()


def test_one_vertex_behind_makes_a_quad_of_two_triangles():
	zc = 0.01
	P = np.array([[0.01, 0.0, 0.3], [0.0, 0.02, -0.1], [-0.01, -0.01, 0.29]])   # vertex 1 behind: p1 = 1, p2 = 2, p3 = 0
	vs, fs, conv, live = _one(_project(P), zc)
	assert live.tolist() == [[True, True]]
	t1, t2 = _view(vs[0, :3].numpy()), _view(vs[0, 3:].numpy())
	q4 = P[1] + (zc - P[1, 2]) / (P[2, 2] - P[1, 2]) * (P[2] - P[1])   # on edge p1 p2 = (1, 2)
	q5 = P[1] + (zc - P[1, 2]) / (P[0, 2] - P[1, 2]) * (P[0] - P[1])   # on edge p1 p3 = (1, 0)
	np.testing.assert_allclose(t1, [q4, P[2], P[0]], rtol=0, atol=1e-15)
	np.testing.assert_allclose(t2, [q4, P[0], q5], rtol=0, atol=1e-15)
	assert (vs[0, :, 2].numpy() >= zc - 1e-15).all()
	# the two triangles tile the visible part: their view-space areas add up to the face's minus the clipped-off corner
	def area3(T):
		return 0.5 * np.linalg.norm(np.cross(T[1] - T[0], T[2] - T[0]))
	corner = area3(np.array([P[1], q4, q5]))
	assert abs(area3(t1) + area3(t2) + corner - area3(P)) < 1e-15
	# the orientation (screen-space winding) of both triangles is the face's
	def wind(T):
		return np.sign(np.cross(T[1] - T[0], T[2] - T[0])[2])
	assert wind(t1) == wind(P) == wind(t2)


def test_two_vertices_behind_makes_one_triangle():
	zc = 0.01
	P = np.array([[0.01, 0.0, 0.005], [0.0, 0.02, 0.3], [-0.01, -0.01, -0.01]])   # vertex 1 alone in front: p1 = 1, p2 = 2, p3 = 0
	vs, fs, conv, live = _one(_project(P), zc)
	assert live.tolist() == [[True, False]] and (fs[0, 1] == -1).all()
	q4 = P[2] + (zc - P[2, 2]) / (P[1, 2] - P[2, 2]) * (P[1] - P[2])
	q5 = P[0] + (zc - P[0, 2]) / (P[1, 2] - P[0, 2]) * (P[1] - P[0])
	np.testing.assert_allclose(_view(vs[0, :3].numpy()), [P[1], q4, q5], rtol=0, atol=1e-15)
	# conversion rows: sub-vertex k -> its original barycentrics (view space is linear in them)
	np.testing.assert_allclose(conv[0, 0].sum(-1).numpy(), 1.0, atol=1e-15)
	np.testing.assert_allclose(conv[0, 0].numpy() @ P, [P[1], q4, q5], atol=1e-15)


def _random_faces(rng, n, zc):
	"""n faces each straddling the plane (one or two vertices behind it; some vertices behind the camera too)."""
	P = rng.uniform(-0.05, 0.05, (n, 3, 3))
	P[..., 2] = rng.uniform(zc + 1e-3, 0.08, (n, 3))
	nb = rng.randint(1, 3, n)
	for i in range(n):
		idx = rng.permutation(3)[:nb[i]]
		P[i, idx, 2] = rng.uniform(-0.03, zc - 1e-3, nb[i])
	return P


def test_sub_triangles_are_coplanar_with_the_parent():
	rng = np.random.RandomState(0)
	zc = 0.01
	P = _random_faces(rng, 200, zc)
	vproj = torch.tensor(np.stack([_project(p) for p in P]).reshape(1, -1, 3))
	faces = torch.arange(3 * len(P)).view(-1, 3)
	vs, fs, conv, live = clip_split(vproj, faces, zc)
	F = len(P)
	assert live[0, :F].all()
	V = _view(vs[0].numpy()).reshape(2 * F, 3, 3)
	for s in np.nonzero(live[0])[0]:
		p = P[s % F]
		n = np.cross(p[1] - p[0], p[2] - p[0])
		n /= np.linalg.norm(n)
		d = np.abs((V[s] - p[0]) @ n).max()
		assert d < 1e-14, (s, d)
		assert (V[s][:, 2] >= zc - 1e-15).all()


def test_converted_barycentrics_equal_the_parents_at_pixel_centres():
	rng = np.random.RandomState(1)
	zc = 0.01
	P = _random_faces(rng, 200, zc)
	vproj = torch.tensor(np.stack([_project(p) for p in P]).reshape(1, -1, 3))
	vp = vproj[0].numpy().reshape(-1, 3, 3)
	faces = torch.arange(3 * len(P)).view(-1, 3)
	vs, fs, conv, live = clip_split(vproj, faces, zc)
	F = len(P)
	S = vs[0].numpy().reshape(2 * F, 3, 3)
	checked = 0
	for s in np.nonzero(live[0])[0]:
		tri = S[s]
		# pixel centres of a 512^2 image inside the sub-triangle (barycentric sampling, snapped to the pixel grid)
		u = rng.dirichlet([1, 1, 1], 64)
		q = u @ tri[:, :2]
		pix = np.floor((1.0 - q) * 512 / 2)
		c = 1.0 - (2.0 * pix + 1.0) / 512
		b_sub = bary_perspective(np.broadcast_to(tri, (64, 3, 3)), c[:, 0], c[:, 1])
		inside = (b_sub > 0).all(-1)
		if not inside.any():
			continue
		b_orig = b_sub[inside] @ conv[0, s].numpy()
		b_par = bary_perspective(np.broadcast_to(vp[s % F], (int(inside.sum()), 3, 3)), c[inside, 0], c[inside, 1])
		np.testing.assert_allclose(b_orig, b_par, rtol=0, atol=1e-12)
		checked += int(inside.sum())
	assert checked > 1000, checked


def test_public_switch_reaches_the_c_struct_and_defaults_off():
	"""make_params / FootRenderer carry the flag; it shares the four bytes of the former int32 K, so the struct keeps its size and an
	int32 K written there reads as (K, clip_faces = 0)."""
	import ctypes
	from find_amd import _lib
	from find_amd import functional_render as FR
	from find_amd.renderer import FootRenderer
	assert FR.make_params(64).clip_faces == 0 and FootRenderer(64).params.clip_faces == 0
	p = FR.make_params(64, clip_faces=True)
	assert p.clip_faces == 1 and p.sil_faces_per_pixel == 100
	assert FootRenderer(64, clip_faces=True).params.clip_faces == 1
	RP = _lib.RenderParams
	assert RP.clip_faces.offset == RP.sil_faces_per_pixel.offset + 2 and ctypes.sizeof(RP) == 21 * 4
	q = RP()
	ctypes.c_int32.from_buffer(q, RP.sil_faces_per_pixel.offset).value = 100
	assert q.sil_faces_per_pixel == 100 and q.clip_faces == 0
	import pytest
	with pytest.raises(ValueError):
		FR.make_params(64, faces_per_pixel=40000)
