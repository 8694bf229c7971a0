"""The point-to-surface distance on the MI355X: find_point_face_fwd / _bwd against the float64 torch reference (surface_ref.py), and their
place in the losses, ModelWithLoss, the Trainer, the evaluation metrics and the heat maps.

Margins: none is a constant of the code under test.  Every comparison also evaluates the reference in float32 on the CPU; with e32 its
worst error against float64 on the same inputs, the HIP result must satisfy e_hip <= 4 e32 + 1e-7 scale (scale: the largest reference
magnitude; the factor 4 allows for another evaluation order).  Each comparison prints e_hip, e32 and scale (DESIGN 7.5 records them).

Face indices are not compared for equality: two faces that share an edge are equally near to a point whose closest point lies on it.
Instead the float64 distance to the face the kernel names must be the float64 minimum, to the same margin.

Figures measured on one MI355X, worst over the cases of each kind (e_hip / e32 / scale): see DESIGN 7.5."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import surface_ref as SR   # noqa: E402


def _held(name, hip, ref64, ref32):
	e_hip = (hip.detach().double().cpu() - ref64).abs().max().item()
	e32 = (ref32.detach().double() - ref64).abs().max().item()
	scale = ref64.abs().max().item()
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  scale {scale:.3e}')
	assert np.isfinite(e_hip) and e_hip <= 4 * e32 + 1e-7 * scale, (name, e_hip, e32, scale)


def _hip(points, verts, faces, p_len=None, g=None):
	"""(dist2, idx, bary[, d_points, d_verts]) of the HIP path, on the CPU."""
	from find_amd import functional as FN
	p, v = points.cuda().requires_grad_(g is not None), verts.cuda().requires_grad_(g is not None)
	dist2, idx, bary = FN.point_face_distance(p, v, faces.cuda(), None if p_len is None else torch.as_tensor(p_len))
	out = [dist2.detach(), idx, bary]
	if g is not None:
		out += list(torch.autograd.grad(dist2, (p, v), g.cuda()))
	torch.cuda.synchronize()
	for t in out:
		assert torch.isfinite(t).all() if t.is_floating_point() else True
	return [t.cpu() for t in out]


def _refs(points, verts, faces, far=None):
	return (SR.point_face(points.double(), verts.double(), faces, far=far), SR.point_face(points, verts, faces))


class _Batch:
	"""The comparisons of one case.  The margin belongs to the case's inputs as a whole: what each mesh contributes (HIP, float64, float32) is
	gathered here and held once, over all meshes -- a mesh with a single valid row, on the surface, has no scale of its own."""

	def __init__(self, name):
		self.name, self.parts = name, {}

	def add(self, what, hip, ref64, ref32):
		self.parts.setdefault(what, []).append((hip.detach().double().cpu().reshape(-1), ref64.double().reshape(-1), ref32.double().reshape(-1)))

	def hold(self):
		assert self.parts
		for what, rows in self.parts.items():
			_held(f'{self.name}: {what}', *(torch.cat(c) for c in zip(*rows)))


def _compare(batch, points, verts, faces, hip, r64, r32, g=None):
	"""One mesh of a case: dist2, the closest point and the named face (and with g both gradients) go to `batch`; what has a bound of its
	own is asserted here."""
	dist2, idx, bary = hip[:3]
	idx = idx.long()
	v64 = verts.double()
	assert (idx >= 0).all() and (idx < faces.shape[0]).all() and SR.usable_faces(verts, faces)[idx].all()
	assert (bary >= 0).all() and (bary.sum(-1) - 1).abs().max().item() <= 2e-7
	batch.add('dist2', dist2, r64['dist2'], r32['dist2'])
	cp = lambda b, i: (b.double()[..., None] * v64[faces[i].long()]).sum(1)
	batch.add('closest point', cp(bary, idx), r64['closest'], cp(r32['bary'], r32['idx']))
	batch.add('distance to the named face', SR.dist2_to_face(points.double(), v64, faces, idx), r64['dist2'], SR.dist2_to_face(points.double(), v64, faces, r32['idx']))
	# dist2 is the distance to the closest point of the barycentrics stored.  Three float32 weights, each rounded by up to 2^-24 of itself,
	# place sum w_i v_i within 4 * 2^-24 * max |v| =: s of the point they stand for, and its squared distance within 2 d s + s^2.
	s = 4 * 2.0 ** -24 * v64.abs().max().item()
	stored = (dist2.double() - ((points.double() - cp(bary, idx)) ** 2).sum(-1)).abs().max().item()
	print(f'{batch.name}: dist2 against the stored barycentrics {stored:.3e}')
	assert stored <= 2 * r64['dist2'].max().sqrt().item() * s + s * s
	if g is not None:
		gp64, gv64 = SR.gradients(points.double(), v64, faces, r64['idx'], r64['bary'], g.double())
		gp32, gv32 = SR.gradients(points, verts, faces, r32['idx'], r32['bary'], g)
		batch.add('d points', hip[3], gp64, gp32)
		batch.add('d verts', hip[4], gv64, gv32)


def _off_the_medial_axis(r64):
	"""False for a query whose float64 runner-up (the nearest face with a closest point more than 1e-4 m from the winner's: _refs(far=1e-4))
	is within 1e-4 d^2 + 1e-12 of the winner: there the last bit decides the face, and with it the gradient."""
	return ~(r64['runner_up'] <= r64['dist2'] * (1 + 1e-4) + 1e-12)


def _queries(verts, faces, n_faces, P, g, push=0.005):
	"""P query points of a mesh: 64 on the surface, 64 at vertices, the rest surface points pushed up to `push` in random directions."""
	fi = torch.randint(0, n_faces, (P,), generator=g)
	w = torch.rand(P, 3, generator=g)
	w = w / w.sum(1, keepdim=True)
	pts = (w[..., None] * verts[faces[fi].long()]).sum(1)
	pts[64:128] = verts[torch.randint(0, verts.shape[0], (64,), generator=g)]
	d = torch.randn(P - 128, 3, generator=g)
	pts[128:] += d / d.norm(dim=1, keepdim=True) * (torch.rand(P - 128, 1, generator=g) * push)
	return pts


def _deformed(v, n, g):
	return torch.stack([v * (1 + 0.15 * torch.randn(3, generator=g)) + 0.002 * torch.randn(v.shape, generator=g) for _ in range(n)])


# ------------------------------------------------------------------ 1. seven regions
def test_seven_regions():
	tri = SR.SEVEN_TRIANGLE
	dist2, idx, bary = _hip(SR.SEVEN_POINTS[None], tri[None], torch.tensor([[0, 1, 2]]))
	assert torch.equal(idx[0], torch.zeros(7, dtype=torch.int32))
	assert torch.equal(dist2[0], SR.SEVEN_DIST2) and torch.equal(bary[0], SR.SEVEN_BARY)
	# among equal distances the smallest face; a face without area and a -1 row are no candidates
	dist2, idx, bary = _hip(SR.SEVEN_POINTS[None], tri[None], torch.tensor([[1, 2, 2], [-1, -1, -1], [0, 1, 2], [0, 1, 2]]))
	assert (idx == 2).all() and torch.equal(dist2[0], SR.SEVEN_DIST2) and torch.equal(bary[0], SR.SEVEN_BARY)


# ------------------------------------------------------------------ 2. against float64
P2, LEN2 = 1500, (1500, 1437, 1)


@pytest.fixture(scope='module')
def small():
	"""synthetic.template(1002) plus a vertex no face touches and the face (3, 7, 7): F = 2001; N = 3 differently deformed copies; the
	float64 and float32 references of the valid rows, computed once."""
	from find_amd import synthetic
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(4)
	v = torch.cat([v, torch.tensor([[0.01, 0.02, 0.03]])])
	f = torch.cat([f, torch.tensor([[3, 7, 7]])])
	assert f.shape[0] == 2001
	verts = _deformed(v, 3, g)
	pts = torch.stack([_queries(verts[i], f, 2000, P2, g) for i in range(3)])
	gout = torch.randn(3, P2, generator=g)
	refs = [_refs(pts[i, :n], verts[i], f, far=1e-4) for i, n in enumerate(LEN2)]
	return verts, f, pts, gout, refs


def test_against_float64(small):
	verts, f, pts, gout, refs = small
	# queries on the medial axis: a second closest point more than 1e-4 m from the winner's, as near as the winner to 1e-4 d^2 + 1e-12.
	# There the nearest face, and with it the gradient, is decided by the last bit; the GRADIENT comparison leaves them out, dist2 does not.
	keep = torch.zeros(3, P2, dtype=torch.bool)
	for i, n in enumerate(LEN2):
		keep[i, :n] = _off_the_medial_axis(refs[i][0])
	left_out = sum(LEN2) - int(keep.sum())
	print(f'medial-axis queries left out of the gradient comparison: {left_out} of {sum(LEN2)}')
	assert left_out <= 0.01 * sum(LEN2)
	g = gout * keep
	dist2, idx, bary, d_points, d_verts = _hip(pts, verts, f, LEN2, g)
	batch = _Batch('template(1002) + 1 vertex + face (3, 7, 7)')
	for i, n in enumerate(LEN2):
		r64, r32 = refs[i]
		print(f'mesh {i}: indices other than float64\'s: HIP {(idx[i, :n].long() != r64["idx"]).sum().item()}, float32 reference {(r32["idx"] != r64["idx"]).sum().item()} of {n}')
		_compare(batch, pts[i, :n], verts[i], f, (dist2[i, :n], idx[i, :n], bary[i, :n], d_points[i, :n], d_verts[i]), r64, r32, g[i, :n])
		# rows at or past p_len
		assert (dist2[i, n:] == 0).all() and (idx[i, n:] == -1).all() and (bary[i, n:] == 0).all() and (d_points[i, n:] == 0).all()
	batch.hold()
	assert (idx != 2000).all()               # the face (3, 7, 7) never wins
	assert (d_verts[:, 1002] == 0).all()     # the vertex of no face
	assert (dist2[0, :64] <= 1e-12).all()    # on the surface


def test_run_to_run(small):
	verts, f, pts, gout, refs = small
	a, b = _hip(pts, verts, f, LEN2, gout), _hip(pts, verts, f, LEN2, gout)
	for x, y in zip(a[:4], b[:4]):   # dist2, idx, bary, d_points: no atomics
		assert torch.equal(x, y)
	# d_verts: float atomics, the same addends in another order -- held to the margin of the comparison with float64
	gv = {torch.float64: [], torch.float32: []}
	for i, n in enumerate(LEN2):
		for r, dt in zip(refs[i], gv):
			gv[dt].append(SR.gradients(pts[i, :n].to(dt), verts[i].to(dt), f, r['idx'], r['bary'], gout[i, :n].to(dt))[1].double())
	gv64, gv32 = torch.stack(gv[torch.float64]), torch.stack(gv[torch.float32])
	e32, scale = (gv32 - gv64).abs().max().item(), gv64.abs().max().item()
	rr = (a[4] - b[4]).abs().max().item()
	print(f'd verts run to run {rr:.3e}  e32 {e32:.3e}  scale {scale:.3e}')
	assert rr <= 4 * e32 + 1e-7 * scale


# ------------------------------------------------------------------ 3. ragged faces
def test_ragged_faces_and_a_mesh_without_faces():
	from find_amd import synthetic
	from find_amd.losses import point_mesh_distance
	from find_amd.structures import Meshes
	(v1, f1), (v2, f2) = synthetic.ellipsoid_mesh(4, 9), synthetic.ellipsoid_mesh(10, 10)
	v3 = v1 * 1.2
	g = torch.Generator().manual_seed(6)
	m = Meshes([v1.cuda(), v2.cuda(), v3.cuda()], [f1.cuda(), f2.cuda(), torch.zeros(0, 3, dtype=torch.int64).cuda()])
	assert m.faces_padded().shape == (3, 200, 3) and (m.faces_padded()[0, 72:] == -1).all() and (m.faces_padded()[2] == -1).all()
	P = 257
	pts = torch.stack([_queries(v, f, f.shape[0], P, g, push=0.01) for v, f in ((v1, f1), (v2, f2), (v1, f1))])
	refs = [_refs(pts[i], v, f, far=1e-4) for i, (v, f) in enumerate(((v1, f1), (v2, f2)))]
	keep = torch.stack([_off_the_medial_axis(refs[0][0]), _off_the_medial_axis(refs[1][0]), torch.ones(P, dtype=torch.bool)])
	print(f'medial-axis queries left out of the gradient comparison: {int((~keep).sum())} of {2 * P}')
	assert int((~keep).sum()) <= 0.01 * 2 * P
	gout = torch.randn(3, P, generator=g) * keep
	p = pts.cuda().requires_grad_(True)
	x = m.verts_padded().clone().requires_grad_(True)
	dist2, idx, bary = point_mesh_distance(p, m.update_padded(x))
	d_points, d_verts = torch.autograd.grad(dist2, (p, x), gout.cuda())
	torch.cuda.synchronize()
	dist2, idx, bary, d_points, d_verts = (t.detach().cpu() for t in (dist2, idx, bary, d_points, d_verts))
	batch = _Batch('ragged faces')
	for i, (v, f) in enumerate(((v1, f1), (v2, f2))):
		r64, r32 = refs[i]
		V = v.shape[0]
		_compare(batch, pts[i], v, f, (dist2[i], idx[i], bary[i], d_points[i], d_verts[i, :V]), r64, r32, gout[i])
		assert (d_verts[i, V:] == 0).all()
	batch.hold()
	assert (idx[2] == -1).all() and (dist2[2] == 0).all() and (bary[2] == 0).all() and (d_points[2] == 0).all() and (d_verts[2] == 0).all()
	# no points at all, and no faces at all
	from find_amd import functional as FN
	e = FN.point_face_distance(torch.zeros(3, 0, 3).cuda(), m.verts_padded(), m.faces_padded())
	assert e[0].shape == (3, 0) and e[1].shape == (3, 0) and e[2].shape == (3, 0, 3)
	e = FN.point_face_distance(pts.cuda(), m.verts_padded(), torch.zeros(0, 3, dtype=torch.int32).cuda())
	assert (e[0] == 0).all() and (e[1] == -1).all() and (e[2] == 0).all()


# ------------------------------------------------------------------ 4. past one tile, and onto the split path
@pytest.fixture(scope='module')
def large():
	"""synthetic.template(6890): F = 13 776, 27 face tiles; N = 3 deformed copies, P = 700 (no multiple of 64)."""
	from find_amd import synthetic
	v, f = synthetic.template(6890)
	g = torch.Generator().manual_seed(8)
	verts = _deformed(v, 3, g)
	pts = torch.stack([_queries(verts[i], f, f.shape[0], 700, g) for i in range(3)])
	return verts, f, pts, [_refs(pts[i], verts[i], f) for i in range(3)]


@pytest.mark.parametrize('n_meshes', [1, 3])
def test_many_tiles_split_and_unsplit(large, n_meshes):
	"""The launch splits a mesh's faces over up to 16 workgroups while it has fewer than 512 of them: both batches here take that path, and
	with the switch that forbids it the unsplit one, whose waves walk all 27 tiles.  The two must agree bit for bit.  A winner culled by
	mistake shows as a dist2 error far above the margin."""
	from find_amd import _lib
	verts, f, pts, refs = large
	assert f.shape[0] == 13776
	got = {}
	for unsplit in (False, True):
		_lib.set_tuning('raster_ablate', 8192 if unsplit else 0)
		try:
			got[unsplit] = _hip(pts[:n_meshes], verts[:n_meshes], f)
		finally:
			_lib.set_tuning('raster_ablate', 0)
	for a, b in zip(got[False], got[True]):
		assert torch.equal(a, b)
	dist2, idx, bary = got[False]
	batch = _Batch(f'template(6890), N = {n_meshes}')
	for i in range(n_meshes):
		_compare(batch, pts[i], verts[i], f, (dist2[i], idx[i], bary[i]), *refs[i])
	batch.hold()


# ------------------------------------------------------------------ 6. SurfaceDistanceLoss, ModelWithLoss, Trainer
def _sample64(verts, faces, face_idx, uv):
	su = uv[:, 0].sqrt()
	w = torch.stack([1 - su, su * (1 - uv[:, 1]), su * uv[:, 1]], -1)
	return (w[..., None] * verts[faces[face_idx.long()].long()]).sum(1), w


def test_surface_distance_loss_against_float64():
	from find_amd import synthetic
	from find_amd.losses import SurfaceDistanceLoss, chamfer_distance, sample_points_from_meshes
	from find_amd.structures import Meshes
	N, S = 2, 300
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(11)
	pv = _deformed(v, N, g)
	gv, gf, _ = synthetic.gt_feet(N, 1002, seed=2, device='cpu')
	draws_p = synthetic.surface_draws(N, S, f.shape[0], seed=1, device='cpu')
	draws_g = synthetic.surface_draws(N, S, gf.shape[0], seed=2, device='cpu')
	x = pv.cuda().requires_grad_(True)
	pred, gt = Meshes(x, f.cuda()), Meshes(gv.cuda(), gf.cuda())
	to_dev = lambda d: (d[0].cuda(), d[1].cuda())
	gs = sample_points_from_meshes(gt, draws=to_dev(draws_g))
	ps = sample_points_from_meshes(pred, draws=to_dev(draws_p))
	loss = SurfaceDistanceLoss()(pred, gt, gt_samples=gs, pred_samples=ps)
	assert loss.dim() == 0
	(d,) = torch.autograd.grad(loss, x)
	torch.cuda.synchronize()
	ref = {}
	for dt in (torch.float64, torch.float32):
		total, grad = 0, torch.zeros(N, v.shape[0], 3, dtype=dt)
		for n in range(N):
			pvn, gvn = pv[n].to(dt), gv[n].to(dt)
			g_pts, _ = _sample64(gvn, gf, draws_g[0][n], draws_g[1][n].to(dt))
			p_pts, w = _sample64(pvn, f, draws_p[0][n], draws_p[1][n].to(dt))
			a, b = SR.point_face(g_pts, pvn, f), SR.point_face(p_pts, gvn, gf)
			total = total + a['dist2'].mean() + b['dist2'].mean()
			# first term: through the closest points; second: through the samples' own barycentrics
			_, dv = SR.gradients(g_pts, pvn, f, a['idx'], a['bary'], torch.full((S,), 1 / (S * N), dtype=dt))
			dp, _ = SR.gradients(p_pts, gvn, gf, b['idx'], b['bary'], torch.full((S,), 1 / (S * N), dtype=dt))
			for k in range(3):
				dv.index_add_(0, f[draws_p[0][n].long(), k], w[:, k, None] * dp)
			grad[n] = dv
		ref[dt] = (total / N, grad)
	_held('SurfaceDistanceLoss', loss, ref[torch.float64][0], ref[torch.float32][0])
	_held('SurfaceDistanceLoss, d verts', d, ref[torch.float64][1], ref[torch.float32][1])
	# drawing its own samples: the same quantity up to the draw
	own = SurfaceDistanceLoss()(pred, gt, num_samples=S)
	assert 0.3 * loss.item() < own.item() < 3 * loss.item()
	# a mesh against itself: nothing of the floor the Chamfer distance of the same samples has
	same = Meshes(gv.cuda(), gf.cuda())
	s1 = sample_points_from_meshes(same, draws=to_dev(draws_g))
	s2 = sample_points_from_meshes(same, draws=to_dev(synthetic.surface_draws(N, S, gf.shape[0], seed=3, device='cpu')))
	zero = SurfaceDistanceLoss()(same, gt, gt_samples=s1, pred_samples=s2).item()
	floor = chamfer_distance(s1, s2)[0].item()
	print(f'mesh against itself: surface {zero:.3e}  Chamfer of the same samples {floor:.3e}')
	assert floor > 0 and 0 <= zero < 1e-3 * floor


@pytest.fixture(scope='module')
def step():
	from find_amd import optim, synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.structures import Meshes, TexturesVertex
	n = 2
	v, f = synthetic.template(1002)
	opts = Opts(chamf_loss=True)
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=n, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None)
	mwl = mwl.to('cuda')
	mwl.model.set_template(v.cuda(), f.cuda())
	lat = synthetic.latents(n, seed=3, device='cuda')
	with torch.no_grad():
		for k in ('shapevec', 'texvec', 'posevec', 'reg'):
			getattr(mwl.model, k).data.copy_(lat[k])
		gen = torch.Generator().manual_seed(1234)   # (a displacement head that carries gradient: synthetic.make_model)
		mwl.model.mlp_disp[-1].weight.copy_((torch.randn(mwl.model.mlp_disp[-1].weight.shape, generator=gen) * 0.01).cuda())
	gv, gf, gc = synthetic.gt_feet(n, 1002, seed=3, device='cuda')
	batch = dict(mesh=Meshes(gv, gf, TexturesVertex(gc.clamp(0.05, 0.95))), idx=torch.arange(n, device='cuda'), name=[f'{i:04d}' for i in range(n)])
	opt = optim.Adam(mwl.model.main_params, lr=1e-4, capturable=True)
	return mwl, opts, batch, opt


def _sampled(mwl, batch):
	from find_amd.train_utils import sample_latent_vectors
	b = dict(batch)
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	return b


def test_model_with_loss_reports_the_p2s_term(step):
	from find_amd.opts import Opts
	mwl, opts, batch, opt = step
	b = _sampled(mwl, batch)
	torch.manual_seed(3)
	loss, losses = mwl(b, 0, opts, p2s=True)
	assert list(losses) == ['loss_p2s'] and torch.equal(loss, losses['loss_p2s'])
	# the raw term on the same draws
	torch.manual_seed(3)
	raw = mwl.surface_loss(mwl.model.get_meshes_from_batch(b, is_train=True)['meshes'], b['mesh']).item()
	got = losses['loss_p2s'].item()
	print('loss_p2s', got, 'raw', raw)
	assert raw > 0 and abs(got - opts.weight_p2s * raw) <= 1e-6 * got
	torch.manual_seed(3)
	_, twice = mwl(b, 0, Opts(chamf_loss=True, weight_p2s=2e4), p2s=True)
	assert abs(twice['loss_p2s'].item() - 2 * got) <= 1e-6 * got
	mwl.zero_grad()
	losses['loss_p2s'].backward()
	torch.cuda.synchronize()
	named = dict(mwl.model.named_parameters())
	for k in ('shapevec.data', 'reg.data'):
		gk = named[k].grad
		assert gk is not None and torch.isfinite(gk).all() and gk.abs().max().item() > 0, k
	mwl.zero_grad()
	# beside the Chamfer term: registry order, and the scans' samples drawn once for both
	torch.manual_seed(3)
	_, both = mwl(b, 0, opts, chamf=True, p2s=True)
	assert list(both) == ['loss_chamf', 'loss_p2s'] and torch.isfinite(both['loss_p2s']).item()
	# flag off: what a call that never mentions it returns, bit for bit
	torch.manual_seed(3)
	la, a = mwl(b, 0, opts, chamf=True)
	torch.manual_seed(3)
	lb, c = mwl(b, 0, opts, chamf=True, p2s=False)
	assert list(a) == list(c) == ['loss_chamf'] and torch.equal(la, lb)


def test_p2s_term_on_the_pca_model(tmp_path):
	from test_gpu_pca import _fixture_mwl
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	z = np.load(os.path.join(HERE, 'golden', 'pca.npz'))
	mwl, opts = _fixture_mwl(z, tmp_path)
	gv, gf = (torch.from_numpy(z[f'gt/{k}']).cuda() for k in ('verts', 'faces'))
	idx = [0, 2]
	b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(torch.full_like(gv[idx], 0.5))), idx=torch.tensor(idx, device='cuda'))
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	loss, losses = mwl(b, 0, opts, p2s=True)
	assert list(losses) == ['loss_p2s'] and torch.isfinite(losses['loss_p2s']).item() and losses['loss_p2s'].item() > 0
	losses['loss_p2s'].backward()
	gs = dict(mwl.model.named_parameters())['shapevec.data'].grad
	assert gs is not None and torch.isfinite(gs).all() and gs.abs().max().item() > 0


def test_trainer_runs_the_term_eagerly(step):
	from find_amd.trainer import Trainer
	mwl, opts, batch, opt = step
	kw = dict(chamf=True, p2s=True)
	tr = Trainer([opt], mwl, [batch, batch], [], opts, latent_vectors_train=mwl.model.latent_vectors_train, device='cuda', graph='auto')
	assert 'p2s' in tr._why_not_graph(tr.optims, kw)
	msg = tr.train_epoch(0, model_kwargs=dict(kw))
	assert tr.last_mode == 'eager', msg
	vals = tr.log[0]['train_loss']['P2S']
	assert len(vals) == 2 and all(np.isfinite(vals)) and all(np.isfinite(tr.log[0]['train_loss']['Chamf']))
	tr.graph = True
	with pytest.raises(RuntimeError, match='p2s'):
		tr.train_epoch(1, model_kwargs=dict(kw))


# ------------------------------------------------------------------ 7. evaluation metrics, heat maps
def test_eval_3d_metrics_surface_and_surface_errors():
	from find_amd import synthetic, vis
	from find_amd.eval_metrics import eval_3d_metrics
	from find_amd.structures import Meshes
	N, S = 2, 400
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(21)
	pv = _deformed(v, N, g)
	scans = [synthetic.ellipsoid_mesh(10, 14), synthetic.ellipsoid_mesh(12, 16)]   # two sizes: a ragged batch
	scans = [(sv * torch.tensor([1.03, 0.97, 1.05]), sf) for sv, sf in scans]
	pred = Meshes(pv.cuda(), f.cuda())
	gt = Meshes([sv.cuda() for sv, _ in scans], [sf.cuda() for _, sf in scans])
	Fg = gt.faces_padded().shape[1]
	draws_p = synthetic.surface_draws(N, S, f.shape[0], seed=1, device='cpu')
	draws_g = (torch.stack([torch.randint(0, sf.shape[0], (S,), generator=g) for _, sf in scans]).to(torch.int32), torch.rand(N, S, 2, generator=g))
	to_dev = lambda d: (d[0].cuda(), d[1].cuda())
	kw = dict(samples=S, draws_gt=to_dev(draws_g), draws_pred=to_dev(draws_p))
	plain = eval_3d_metrics(pred, gt, **kw)
	out, per_foot = eval_3d_metrics(pred, gt, surface=True, return_per_foot=True, **kw)
	assert list(plain) == ['Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)']
	assert list(out) == list(plain) + ['Scan→pred (mm)', 'Pred→scan (mm)', 'Surf (μm)'] and all(torch.equal(out[k], plain[k]) for k in plain)
	pred_err, gt_err = vis.surface_errors(pred, gt)
	Vg = max(sv.shape[0] for sv, _ in scans)
	assert pred_err.shape == (N, 1002) and gt_err.shape == (N, Vg) and (gt_err[0, scans[0][0].shape[0]:] == 0).all()
	ref = {}
	for dt in (torch.float64, torch.float32):
		r = dict(s2p=[], p2s=[], surf=[], pe=[], ge=[])
		for n in range(N):
			pvn, (sv, sf) = pv[n].to(dt), scans[n]
			sv = sv.to(dt)
			a, b = SR.point_face(sv, pvn, f)['dist2'], SR.point_face(pvn, sv, sf)['dist2']
			r['ge'].append(a), r['pe'].append(b)
			r['s2p'].append(a.sqrt().mean() * 1e3), r['p2s'].append(b.sqrt().mean() * 1e3)
			g_pts, _ = _sample64(sv, sf, draws_g[0][n], draws_g[1][n].to(dt))
			p_pts, _ = _sample64(pvn, f, draws_p[0][n], draws_p[1][n].to(dt))
			r['surf'].append(SR.point_face(g_pts, pvn, f)['dist2'].mean() + SR.point_face(p_pts, sv, sf)['dist2'].mean())
		ref[dt] = r
	r64, r32 = ref[torch.float64], ref[torch.float32]
	mean = lambda x: torch.stack(x).mean()
	_held('Scan→pred (mm)', out['Scan→pred (mm)'], mean(r64['s2p']), mean(r32['s2p']))
	_held('Pred→scan (mm)', out['Pred→scan (mm)'], mean(r64['p2s']), mean(r32['p2s']))
	_held('Surf (μm)', out['Surf (μm)'], mean(r64['surf']) * 1e6, mean(r32['surf']) * 1e6)
	_held('per foot, Scan→pred (mm)', per_foot['Scan→pred (mm)'], torch.stack(r64['s2p']), torch.stack(r32['s2p']))
	for n in range(N):
		_held(f'surface_errors, prediction {n}', pred_err[n], r64['pe'][n], r32['pe'][n])
		_held(f'surface_errors, scan {n}', gt_err[n, :scans[n][0].shape[0]], r64['ge'][n], r32['ge'][n])
	assert out['Surf (μm)'].item() < out['Chamf (μm)'].item()   # no floor from the sample count
	assert Fg == scans[1][1].shape[0]


def test_eval_3d_passes_surface_through(tmp_path):
	"""evaluate.eval_3d(surface=True): the three keys beside today's numbers, the per-foot values, and heat maps from vis.surface_errors."""
	from tests.test_gpu_eval2d import _model
	from tests.test_gpu_vis import _foot3d_val2
	from find_amd import evaluate
	ds = _foot3d_val2(str(tmp_path / 'data'))
	model = _model(2)
	kp_idx = [3, 17, 40, 101]
	torch.manual_seed(21)
	plain, plain_extra = evaluate.eval_3d(model, ds, kp_idx, samples=500, produce_spins=True, out_dir=str(tmp_path / 'a'), spin_frames=2, spin_image_size=32)
	torch.manual_seed(21)
	res, extra = evaluate.eval_3d(model, ds, kp_idx, samples=500, surface=True, return_per_foot=True, produce_spins=True, out_dir=str(tmp_path / 'b'),
								  spin_frames=2, spin_image_size=32)
	new = ['Scan→pred (mm)', 'Pred→scan (mm)', 'Surf (μm)']
	assert list(res) == list(plain) + new and all(res[k] == plain[k] for k in plain)   # no draw was added
	assert all(np.isfinite(res[k]) and res[k] > 0 for k in new) and res['Surf (μm)'] <= res['Chamf (μm)']
	assert extra['scan_to_pred_mm'].shape == (2,) and extra['pred_to_scan_mm'].shape == (2,) and extra['keypoint_mm'].shape == (2, 4)
	assert abs(extra['scan_to_pred_mm'].mean().item() - res['Scan→pred (mm)']) <= 1e-6 * res['Scan→pred (mm)']
	assert len(extra['files']) == 12 and all(os.path.exists(f) for f in extra['files'])
	# the heat maps' errors: to the other SURFACE, so never farther than to its nearest vertex (what they showed before)
	assert extra['pred_vertex_error'].shape == (2, 1002) and [tuple(t.shape) for t in extra['gt_vertex_error']] == [(49,), (81,)]
	before, after = plain_extra['pred_vertex_error'], extra['pred_vertex_error']
	assert (after <= before * (1 + 1e-5) + 1e-12).all() and (after < 0.9 * before).any()
