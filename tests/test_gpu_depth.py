"""Depth on the MI355X: find_depth_bwd through FootRenderer's out['depth'] against autograd through the oracle's fragments
(oracle.render_ref.torch_project + torch_fragments(clip_bary=False), evaluated on the pix_to_face the renderer returned), find_depth_loss_*
against the float64 torch evaluation of its formula (test_depth_host.py), and their place in ModelWithLoss and eval_metrics.

Margins: none is a constant of the code under test.  Every comparison also evaluates the same reference in float32 on the CPU; with e32 its
worst error against float64, the HIP result must satisfy e_hip <= 4 e32 + 1e-7 scale (scale: the largest reference magnitude; DESIGN 7.4's
rule).  The gradient tests also print the summation-order term of fp32 (the fp32 oracle with the covered pixels in three orders).  Each test
prints its figures (DESIGN 7.6 records them)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)

from oracle import camera_ref   # noqa: E402
from test_depth_host import depth_loss_ref, oracle_depth_grad   # noqa: E402


def _held(name, hip, ref64, ref32):
	e_hip = (hip.detach().double().cpu() - ref64).abs().max().item()
	e32 = (ref32.detach().double() - ref64).abs().max().item()
	scale = ref64.abs().max().item()
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  scale {scale:.3e}')
	assert np.isfinite(e_hip) and e_hip <= 4 * e32 + 1e-7 * scale, (name, e_hip, e32, scale)


def _views(dist, elev, azim):
	R, T = camera_ref.look_at_view_transform(dist=np.asarray(dist, np.float64), elev=np.asarray(elev, np.float64), azim=np.asarray(azim, np.float64),
											 up=((1, 0, 0),))
	return torch.from_numpy(R).float(), torch.from_numpy(T).float()


def _upstream(p2f, seed):
	"""A random d L / d depth, zero on a third of the covered pixels (and anything on the background: it must not matter)."""
	g = torch.Generator().manual_seed(seed)
	up = torch.randn(p2f.shape, generator=g)
	up[(torch.rand(p2f.shape, generator=g) < 0.33) & (p2f.cpu() >= 0)] = 0
	return up


def _through_renderer(rdr, verts, faces, R, T, up_seed):
	"""out['depth'] of FootRenderer and its gradient, with the pix_to_face of the same raster pass."""
	from find_amd import functional_render as FR
	from find_amd.structures import Meshes
	x = verts.cuda().requires_grad_(True)
	m = Meshes(x, faces.cuda())
	out = rdr(m, R.cuda(), T.cuda(), return_images=False, return_depth=True)
	depth = out['depth']
	assert set(out) == {'depth'} and depth.requires_grad
	fc = m.faces_shared() if m.faces_shared() is not None else m.faces_padded()
	_, _, p2f, zbuf = FR.render(x.detach(), None, fc, R.cuda(), T.cuda(), rdr.params, want_mask=False, want_image=False, want_frags=True)
	assert torch.equal(zbuf, depth.detach()) and ((p2f >= 0) == (zbuf > 0)).all() and (zbuf[p2f < 0] == -1).all()
	up = _upstream(p2f, up_seed)
	(d,) = torch.autograd.grad(depth, x, up.cuda())
	torch.cuda.synchronize()
	return depth.detach(), p2f, up, d, fc


def _against_oracle(name, verts, fc, R, T, p2f, up, depth, d, fov=60.0):
	"""The gradient (and, loosely, the depth itself) against the oracle on the same selection; returns the figures."""
	N, M, H, W = p2f.shape
	sel, g = p2f.cpu().reshape(N * M, H, W), up.reshape(N * M, H, W)
	pz64, g64 = oracle_depth_grad(verts, fc, R, T, sel, g, torch.float64, fov)
	pz32, g32 = oracle_depth_grad(verts, fc, R, T, sel, g, torch.float32, fov)
	others = [oracle_depth_grad(verts, fc, R, T, sel, g, torch.float32, fov, order=o)[1] for o in ('reverse', 1)]
	scale = g64.abs().max().item()
	e_order = max((a.double() - b.double()).abs().max().item() for a in [g32] + others for b in others)
	covered = sel >= 0
	ez = (depth.cpu().reshape(N * M, H, W)[covered].double() - pz64).abs().max().item()
	print(f'{name}: {int(covered.sum())} covered pixels, depth vs float64 oracle {ez:.2e}; summation-order term of fp32 {e_order:.3e} (scale {scale:.3e})')
	assert ez < 1e-5   # (the forward is render.hip's: test_gpu_render.py's bound on zbuf)
	assert torch.isfinite(d).all()
	_held(name + ', d verts', d, g64, g32)
	return g64


# ------------------------------------------------------------------ find_depth_bwd through the renderer
def test_depth_gradient_shared_faces():
	"""synthetic.template(1002) (foot-sized), two deformed copies, three views of which one oblique, 32^2: 4 workgroups per image."""
	from find_amd import synthetic
	from find_amd.renderer import FootRenderer
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(21)
	verts = torch.stack([v * (1 + 0.1 * torch.rand(3, generator=g)) + 0.001 * torch.randn(v.shape, generator=g) for _ in range(2)])
	R, T = _views([0.3, 0.3, 0.27], [0., 90., 35.], [0., 0., 50.])
	rdr = FootRenderer(image_size=32, device='cuda')
	depth, p2f, up, d, fc = _through_renderer(rdr, verts, f, R, T, 1)
	assert depth.shape == (2, 3, 32, 32) and 0.05 < (p2f >= 0).float().mean().item() < 0.6
	g64 = _against_oracle('shared faces', verts, f, R, T, p2f, up, depth, d)
	# a vertex no covered pixel sees gets exactly zero
	seen = torch.zeros(2, v.shape[0], dtype=torch.bool)
	img = torch.arange(6).view(2, 3, 1, 1)
	local = torch.where(p2f.cpu() >= 0, p2f.cpu() - img * f.shape[0], p2f.cpu())
	for n in range(2):
		faces_seen = local[n][(local[n] >= 0) & (up[n] != 0)].unique()
		seen[n, f[faces_seen].reshape(-1)] = True
	assert (~seen).any() and (d.cpu()[~seen] == 0).all() and (g64[~seen] == 0).all()


def test_depth_gradient_ragged_faces():
	"""Two per-mesh, -1-padded face lists, V = 38 / 102."""
	from find_amd import synthetic
	from find_amd.renderer import FootRenderer
	(v1, f1), (v2, f2) = synthetic.ellipsoid_mesh(4, 9), synthetic.ellipsoid_mesh(10, 10)
	assert v1.shape[0] == 38 and v2.shape[0] == 102
	verts = torch.zeros(2, 102, 3)
	verts[0, :38], verts[1] = v1, v2
	R, T = _views([0.3, 0.28], [10., -60.], [0., 40.])
	rdr = FootRenderer(image_size=32, device='cuda')
	from find_amd import functional_render as FR
	from find_amd.structures import Meshes
	x = verts.cuda().requires_grad_(True)
	m = Meshes([x[0, :38], x[1]], [f1.cuda(), f2.cuda()])
	fc = m.faces_padded()
	assert fc.shape == (2, 200, 3) and (fc[0, 72:] == -1).all()
	depth = rdr(m, R.cuda(), T.cuda(), return_images=False, return_depth=True)['depth']
	assert depth.requires_grad
	_, _, p2f, zbuf = FR.render(m.verts_padded().detach(), None, fc, R.cuda(), T.cuda(), rdr.params, want_mask=False, want_image=False, want_frags=True)
	assert torch.equal(zbuf, depth.detach())
	up = _upstream(p2f, 2)
	(d,) = torch.autograd.grad(depth, x, up.cuda())
	torch.cuda.synchronize()
	assert all((p2f[n] >= 0).any() for n in range(2))
	_against_oracle('ragged faces', verts, fc.cpu().clamp(min=0), R, T, p2f, up, depth, d)
	assert (d[0, 38:] == 0).all()


def test_depth_gradient_rectangular_image():
	"""24 x 40: the pixel centres are 1 - (2 i + 1) / W and 1 - (2 j + 1) / H, each with its own size."""
	from find_amd import functional as FN
	from find_amd import functional_render as FR
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(10, 10)
	verts = torch.stack([v, v * 1.1])
	R, T = _views([0.3, 0.3], [0., 40.], [0., 30.])
	params = FR.make_params((24, 40))
	assert (params.image_h, params.image_w) == (24, 40)
	x = verts.cuda().requires_grad_(True)
	_, _, p2f, zbuf = FR.render(x.detach(), None, f.cuda(), R.cuda(), T.cuda(), params, want_mask=False, want_image=False, want_frags=True)
	assert p2f.shape == (2, 2, 24, 40)
	depth = FN.depth_map(x, f.cuda(), R.cuda(), T.cuda(), params, p2f, zbuf)
	assert torch.equal(depth.detach(), zbuf)
	up = _upstream(p2f, 3)
	(d,) = torch.autograd.grad(depth, x, up.cuda())
	torch.cuda.synchronize()
	_against_oracle('24 x 40', verts, f, R, T, p2f, up, depth, d)


def test_depth_gradient_in_split_mode():
	"""clip_faces=True with the clip plane through the middle of the mesh (z_clip 0.3 m, the camera 0.3 m away): the faces along the cut
	straddle it, the pixels there see their clipped triangles, and pix_to_face names the whole face -- whose plane the clipped triangle
	lies in.  Every vertex is in front of the camera, so the oracle's unclipped fragment arithmetic is well defined on these faces."""
	from find_amd import synthetic
	from find_amd.renderer import FootRenderer
	v, f = synthetic.ellipsoid_mesh(14, 18)
	verts = torch.stack([v, v * torch.tensor([1.05, 0.9, 1.1])])
	R, T = _views([0.3, 0.31], [0., 25.], [0., 15.])
	rdr = FootRenderer(image_size=32, device='cuda', z_clip_value=0.3, clip_faces=True)
	assert rdr.params.clip_faces == 1 and abs(rdr.params.z_clip - 0.3) < 1e-7
	depth, p2f, up, d, fc = _through_renderer(rdr, verts, f, R, T, 4)
	assert (depth[p2f >= 0] >= 0.3 * (1 - 1e-6)).all()   # (requires_grad: checked in _through_renderer)
	# some covered pixel with a gradient names a face that straddles the plane
	vz = (torch.einsum('nvi,mij->nmvj', verts, R) + T[None, :, None, :])[..., 2]       # (N, M, V)
	assert vz.min().item() > 0.1
	img = torch.arange(4).view(2, 2, 1, 1)
	local = torch.where(p2f.cpu() >= 0, p2f.cpu() - img * f.shape[0], p2f.cpu())
	straddling = 0
	for n in range(2):
		for m in range(2):
			ids = local[n, m][(local[n, m] >= 0) & (up[n, m] != 0)].unique()
			z3 = vz[n, m][f[ids]]
			straddling += int(((z3.min(1).values < 0.3) & (z3.max(1).values > 0.3)).sum())
	print('split mode: faces with a gradient that straddle the clip plane:', straddling)
	assert straddling >= 10
	_against_oracle('split mode', verts, f, R, T, p2f, up, depth, d)


def test_depth_gradient_ignores_bad_indices():
	from find_amd import functional as FN
	from find_amd import functional_render as FR
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(10, 10)
	V, F = v.shape[0], f.shape[0]
	verts = torch.stack([v, v * 1.1]).cuda()
	R, T = (t.cuda() for t in _views([0.3, 0.3], [0., 40.], [0., 30.]))
	params = FR.make_params(32)
	_, _, p2f, zbuf = FR.render(verts, None, f.cuda(), R, T, params, want_mask=False, want_image=False, want_frags=True)
	up = torch.randn(p2f.shape, generator=torch.Generator().manual_seed(5)).cuda()

	def grad(faces, sel):
		x = verts.clone().requires_grad_(True)
		(d,) = torch.autograd.grad(FN.depth_map(x, faces, R, T, params, sel, zbuf), x, up)
		torch.cuda.synchronize()
		return d
	# no face anywhere: zeros, every element written
	assert (grad(f.cuda(), torch.full_like(p2f, -1)) == 0).all()
	good = grad(f.cuda(), p2f)
	assert good.abs().max().item() > 0
	# packed ids whose face index lies outside [0, F): nothing
	img = torch.arange(4, device='cuda', dtype=torch.int32).view(2, 2, 1, 1)
	beyond = torch.where(p2f >= 0, img * F + F + 3, p2f)
	before = torch.where(p2f >= 0, img * F - 1, p2f)   # (the last face of the image before: face -1 of this one)
	assert (grad(f.cuda(), beyond) == 0).all() and (grad(f.cuda(), before) == 0).all()
	# faces with a vertex index outside [0, V): those faces add nothing, the others what they added before
	seen = (p2f[p2f >= 0].long() % F).unique()
	bad = f.clone()
	bad[seen[0], 1] = V + 5
	bad[seen[1], 2] = -7
	bad[seen[2], 0] = 2 ** 31 - 1
	local = torch.where(p2f >= 0, p2f - img * F, p2f)
	hit = torch.isin(local, seen[:3].to(local.dtype))
	assert hit.any()
	d_bad = grad(bad.cuda(), p2f)
	d_ref = grad(f.cuda(), torch.where(hit, torch.full_like(p2f, -1), p2f))
	d_ref2 = grad(f.cuda(), torch.where(hit, torch.full_like(p2f, -1), p2f))
	rr = (d_ref - d_ref2).abs().max().item()   # (float atomics: the run-to-run spread)
	err = (d_bad - d_ref).abs().max().item()
	print(f'bad vertex indices: err {err:.3e}  run-to-run {rr:.3e}  max |d| {d_ref.abs().max().item():.3e}')
	assert torch.isfinite(d_bad).all() and err <= 4 * rr + 1e-6 * d_ref.abs().max().item()


def test_forward_is_unchanged():
	from find_amd import synthetic
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesVertex
	gv, gf, gc = synthetic.gt_feet(2, 1002, seed=5, device='cuda')
	rdr = FootRenderer(image_size=32, device='cuda')
	R, T = rdr.view_from(['topdown', 'side1'])
	R, T = R.cuda().float(), T.cuda().float()
	plain = rdr(Meshes(gv, gf, TexturesVertex(gc)), R, T, return_depth=True, return_mask=True)
	x = gv.clone().requires_grad_(True)
	grad = rdr(Meshes(x, gf, TexturesVertex(gc)), R, T, return_depth=True, return_mask=True)
	assert set(plain) == set(grad) == {'depth', 'image', 'mask'}
	assert not plain['depth'].requires_grad and grad['depth'].requires_grad
	for k in ('depth', 'mask'):
		assert torch.equal(plain[k], grad[k].detach()), k
	# (the shader's vertex normals are summed with float atomics: two image renders differ in the last bits)
	assert (plain['image'] - grad['image'].detach()).abs().max().item() <= 1e-5
	assert (plain['depth'] > 0).any() and (plain['depth'][plain['depth'] <= 0] == -1).all()
	with torch.no_grad():
		off = rdr(Meshes(x, gf, TexturesVertex(gc)), R, T, return_depth=True)
	assert not off['depth'].requires_grad and torch.equal(off['depth'], plain['depth'])
	# the depth's gradient adds to the mask's and the image's
	(d_all,) = torch.autograd.grad(grad['depth'].sum() + grad['mask'].sum(), x, retain_graph=True)
	(d_depth,) = torch.autograd.grad(grad['depth'].sum(), x, retain_graph=True)
	(d_mask,) = torch.autograd.grad(grad['mask'].sum(), x)
	s = d_all.abs().max().item()
	assert d_depth.abs().max().item() > 0 and (d_all - d_depth - d_mask).abs().max().item() <= 1e-4 * s


# ------------------------------------------------------------------ depth loss
def _loss_inputs(n_img, n_pix, seed):
	g = torch.Generator().manual_seed(seed)
	t = 0.3 + 0.03 * torch.randn(n_img, n_pix, generator=g)
	p = t + 0.012 * torch.randn(n_img, n_pix, generator=g)
	p[torch.rand(n_img, n_pix, generator=g) < 0.1] = -1
	t[torch.rand(n_img, n_pix, generator=g) < 0.1] = -1
	same = torch.rand(n_img, n_pix, generator=g) < 0.05
	p[same] = t[same]                                   # r = 0 exactly: sign(0) = 0
	w = torch.rand(n_img, n_pix, generator=g)
	w[torch.rand(n_img, n_pix, generator=g) < 0.3] = 0
	return p, t, w


def _hip_loss(p, t, w, gl=1.7, **kw):
	from find_amd import functional as FN
	x = p.cuda().requires_grad_(True)
	loss, per = FN.depth_loss(x, t.cuda(), None if w is None else w.cuda(), return_per_image=True, **kw)
	assert loss.dim() == 0 and loss.dtype == torch.float32 and per.dtype == torch.float64 and per.shape == (p.shape[0], 2) and not per.requires_grad
	(d,) = torch.autograd.grad(loss * gl, x)
	torch.cuda.synchronize()
	return loss.detach(), per, d


@pytest.mark.parametrize('shape', [(3, 37 * 29), (5, 64 * 64), (1, 1025)])
def test_depth_loss_against_float64(shape):
	"""(3, 1073): no multiple of 4, images 1 and 2 start off a 16-byte boundary (scalar form), image 0 on one; two workgroups per image, the
	second partly filled.  (5, 4096): 16-byte loads throughout, four workgroups per image, 20 pairs for the second stage.  (1, 1025): one
	pixel in the second workgroup."""
	p, t, w = _loss_inputs(*shape, seed=sum(shape))
	gl, delta, trunc = 1.7, 0.01, 0.02
	assert ((p - t).abs() > trunc).sum() > 5 and ((p - t).abs() < delta).sum() > 50
	for kind in ('l1', 'l2', 'huber'):
		for weight in (w, None):
			for tr in (0., trunc):
				kw = dict(kind=kind, delta=delta, trunc=tr)
				loss, per, d = _hip_loss(p, t, weight, gl, **kw)
				ref = {}
				for dt in (torch.float64, torch.float32):
					x = p.detach().clone().to(dt).requires_grad_(True)
					l, pi = depth_loss_ref(x, t.to(dt), None if weight is None else weight.to(dt), per_image=True, **kw)
					(l * gl).backward()
					ref[dt] = (l.detach(), pi.detach(), x.grad)
				tag = f'depth loss {shape} {kind} weight={weight is not None} trunc={tr}'
				_held(tag, loss, ref[torch.float64][0], ref[torch.float32][0])
				_held(tag + ', d pred', d, ref[torch.float64][2], ref[torch.float32][2])
				for c, what in enumerate(('sum w rho', 'sum w')):
					_held(tag + ', per image ' + what, per[:, c], ref[torch.float64][1][:, c], ref[torch.float32][1][:, c])
				dead = (p <= 0) | (t <= 0) | (p == t)
				if weight is not None:
					dead = dead | (weight == 0)
				if tr > 0:
					dead = dead | ((p.double() - t.double()).abs() > tr * (1 + 1e-6))
				assert dead.sum() > 100 and (d[dead.cuda()] == 0).all()
				loss2, per2, d2 = _hip_loss(p, t, weight, gl, **kw)
				assert torch.equal(loss, loss2) and torch.equal(per, per2) and torch.equal(d, d2)
	# an unaligned view takes the scalar form: the same per-pixel arithmetic, the same sums
	from find_amd import functional as FN
	buf = torch.zeros(p.numel() + 1, device='cuda')
	buf[1:] = p.cuda().reshape(-1)
	off = buf[1:].view(*shape).requires_grad_(True)
	assert off.data_ptr() % 16
	kw = dict(kind='huber', delta=delta, trunc=trunc)
	loss, per, d = _hip_loss(p, t, w, gl, **kw)
	l_off, per_off = FN.depth_loss(off, t.cuda(), w.cuda(), return_per_image=True, **kw)
	(d_off,) = torch.autograd.grad(l_off * gl, off)
	assert torch.equal(l_off, loss) and torch.equal(per_off, per) and torch.equal(d_off, d)


def test_depth_loss_without_a_valid_pixel():
	p, t, w = _loss_inputs(3, 37 * 29, 1)
	for args in ((-p.abs(), t, w), (p, torch.full_like(t, -1), None), (p, t, torch.zeros_like(w))):
		for kind in ('l1', 'l2', 'huber'):
			loss, per, d = _hip_loss(*args, kind=kind)
			assert loss.item() == 0.0 and (d == 0).all() and (per == 0).all()
	# truncation that cuts everything
	loss, per, d = _hip_loss(p + 1, t, None, trunc=0.02)
	assert loss.item() == 0.0 and (d == 0).all()


def test_depth_loss_class_and_shapes():
	from find_amd import functional as FN
	from find_amd.losses import DepthLoss
	p, t, w = _loss_inputs(6, 16 * 16, 3)
	a = DepthLoss('huber', 0.01, 0.02)(p.cuda().view(2, 3, 16, 16), t.cuda().view(2, 3, 16, 16), w.cuda().view(2, 3, 16, 16))
	b = FN.depth_loss(p.cuda(), t.cuda(), w.cuda(), kind='huber', delta=0.01, trunc=0.02)
	# (2, 3, 16, 16) folds to two images of 768 pixels, (6, 256) to six: other partial sums, the same loss to double rounding
	assert abs(a.item() - b.item()) <= 1e-6 * b.item()
	with pytest.raises(RuntimeError, match='shape'):
		FN.depth_loss(p.cuda(), t.cuda()[:, :-1])


# ------------------------------------------------------------------ ModelWithLoss, eval_metrics
@pytest.fixture(scope='module')
def step():
	from find_amd import optim, synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesVertex
	n = 2
	v, f = synthetic.template(1002)
	opts = Opts(sil_loss=True, num_views=2)
	mwl = ModelWithLoss(opts=opts, device='cpu', use_shapevec=True, use_texvec=True, use_posevec=True, train_size=n, val_size=1,
						shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None)
	mwl = mwl.to('cuda')
	mwl.model.set_template(v.cuda(), f.cuda())
	mwl.rdr = FootRenderer(image_size=32, device='cuda')
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


def _named_grads(mwl):
	return {k: q.grad.clone() for k, q in mwl.model.named_parameters() if q.grad is not None}


def test_model_with_loss_reports_the_depth_term(step):
	from find_amd import functional as FN
	from find_amd.opts import Opts
	mwl, opts, batch, opt = step
	b = _sampled(mwl, batch)
	flags = dict(sil=True, render_foot=True, return_renders=True)
	np.random.seed(5)
	loss, losses, rdr = mwl(b, 0, opts, depth=True, **flags)
	assert list(losses) == ['loss_sil', 'loss_depth']
	pd, gd = rdr['pred']['depth'], rdr['gt']['depth']
	assert pd.shape == (2, 2, 32, 32) and gd.shape == pd.shape and pd.requires_grad and not gd.requires_grad
	want = FN.depth_loss(pd.reshape(4, -1), gd.reshape(4, -1), kind='l1', trunc=0.02).item() * opts.weight_depth
	got = losses['loss_depth'].item()
	print('loss_depth', got, want)
	assert 0 < got < 0.02 * opts.weight_depth and abs(got - want) <= 1e-6 * want
	# gradients of the term alone reach the shape code, the network and the registration
	mwl.zero_grad()
	losses['loss_depth'].backward()
	torch.cuda.synchronize()
	grads = _named_grads(mwl)
	for k in ('shapevec.data', 'reg.data'):
		assert k in grads and torch.isfinite(grads[k]).all() and grads[k].abs().max().item() > 0, k
	assert all(torch.isfinite(q).all() for q in grads.values())
	mwl.zero_grad()
	# another kind, weight and truncation through the options; a reference Opts without them means the defaults
	np.random.seed(5)
	o2 = Opts(sil_loss=True, num_views=2, weight_depth=7., depth_loss_kind='huber', depth_loss_delta=0.002, depth_trunc=0.)
	_, losses2, rdr2 = mwl(b, 0, o2, depth=True, **flags)
	want2 = FN.depth_loss(rdr2['pred']['depth'].reshape(4, -1), rdr2['gt']['depth'].reshape(4, -1), kind='huber', delta=0.002, trunc=0.).item() * 7.
	assert abs(losses2['loss_depth'].item() - want2) <= 1e-6 * want2 and torch.equal(losses2['loss_sil'], losses['loss_sil'])

	class Bare:
		pass
	bare = Bare()
	bare.__dict__.update({k: v for k, v in vars(opts).items() if 'depth' not in k})
	assert not hasattr(bare, 'weight_depth') and not hasattr(bare, 'depth_trunc')
	np.random.seed(5)
	_, losses3, _ = mwl(b, 0, bare, depth=True, **flags)
	assert torch.equal(losses3['loss_depth'], losses['loss_depth'])
	# what the GT's mask-out map hides does not count: the weight is 0 there
	hide = torch.arange(0, batch['mesh'].faces_shared().shape[0] // 2, device='cuda')
	bm = dict(b, masked_faces=hide)
	np.random.seed(5)
	_, losses4, rdr4 = mwl(bm, 0, opts, depth=True, **flags)
	mo = rdr4['gt']['mask_out_masks']
	assert mo.any() and not mo.all() and not rdr4['gt']['nothing_hidden']
	w = (~mo).float().reshape(4, -1)
	want4 = FN.depth_loss(rdr4['pred']['depth'].reshape(4, -1), rdr4['gt']['depth'].reshape(4, -1), w, kind='l1', trunc=0.02).item() * opts.weight_depth
	assert abs(losses4['loss_depth'].item() - want4) <= 1e-6 * want4 and abs(want4 - want) > 1e-6 * want
	# without renders the term is skipped silently, as pix is; alone, it renders no image
	_, losses_c = mwl(b, 0, opts, depth=True, pix=True, smooth=True, render_foot=False)
	assert list(losses_c) == ['loss_smooth']
	np.random.seed(5)
	loss_d, losses_d = mwl(b, 0, opts, depth=True, render_foot=True)
	assert list(losses_d) == ['loss_depth'] and torch.equal(loss_d, losses_d['loss_depth'])
	assert abs(losses_d['loss_depth'].item() - got) <= 1e-6 * got


def test_flag_off_is_the_step_it_was(step):
	"""depth=False (and a call that never mentions it): the same dictionary, no depth in the renders, gradients within the run-to-run spread of
	the silhouette backward's float atomics."""
	mwl, opts, batch, opt = step
	flags = dict(sil=True, smooth=True, render_foot=True, return_renders=True)
	runs = []
	for kw in ({}, dict(depth=False), {}):
		b = _sampled(mwl, batch)   # (the latent gather's graph is freed by each backward)
		np.random.seed(5)
		mwl.zero_grad()
		loss, losses, rdr = mwl(b, 0, opts, **flags, **kw)
		loss.backward()
		torch.cuda.synchronize()
		runs.append((loss.detach(), {k: v.detach() for k, v in losses.items()}, rdr, _named_grads(mwl)))
	mwl.zero_grad()
	(la, da, ra, ga), (lb, db, rb, gb), (lc, dc, rc, gc) = runs
	assert list(da) == list(db) == ['loss_smooth', 'loss_sil'] and torch.equal(la, lb) and all(torch.equal(da[k], db[k]) for k in da)
	assert set(ra['pred']) == set(rb['pred']) and set(ra['gt']) == set(rb['gt']) and 'depth' not in rb['pred'] and 'depth' not in rb['gt']
	assert set(ga) == set(gb)
	for k in ga:
		rr = (ga[k] - gc[k]).abs().max().item()
		assert (ga[k] - gb[k]).abs().max().item() <= 4 * rr + 1e-6 * ga[k].abs().max().item(), k


def test_depth_term_on_the_pca_model(tmp_path):
	from test_gpu_pca import _fixture_mwl
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	z = np.load(os.path.join(GOLD, 'pca.npz'))
	mwl, opts = _fixture_mwl(z, tmp_path)
	mwl.rdr = FootRenderer(image_size=32, device='cuda')
	gv, gf = (torch.from_numpy(z[f'gt/{k}']).cuda() for k in ('verts', 'faces'))
	idx = [0, 2]
	b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(torch.full_like(gv[idx], 0.5))), idx=torch.tensor(idx, device='cuda'))
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	opts.num_views = 2
	np.random.seed(5)
	loss, losses = mwl(b, 0, opts, depth=True, sil=True, render_foot=True)
	assert list(losses) == ['loss_sil', 'loss_depth'] and torch.isfinite(losses['loss_depth']).item()
	losses['loss_depth'].backward()
	g = dict(mwl.model.named_parameters())['shapevec.data'].grad
	assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0


def test_adam_on_the_depth_loss_lowers_depth_error_mm():
	"""A scan displaced by 3 mm along the first camera's axis, fitted back to its own depth maps: ten Adam steps lower the metric."""
	from find_amd import eval_metrics, synthetic
	from find_amd.losses import DepthLoss
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes
	gv, gf, _ = synthetic.gt_feet(1, 1002, seed=7, device='cuda')
	rdr = FootRenderer(image_size=32, device='cuda')
	R, T = rdr.view_from(['topdown', 'side1', '45'])
	R, T = R.cuda().float(), T.cuda().float()
	kw = dict(return_images=False, return_depth=True, return_mask_out_masks=True)
	with torch.no_grad():
		gt = rdr(Meshes(gv, gf), R, T, **kw)
	x = (gv + torch.tensor([0., 0., 0.003], device='cuda')).requires_grad_(True)
	opt = torch.optim.Adam([x], lr=3e-4)
	crit = DepthLoss('l1', trunc=0.02)

	def metric():
		with torch.no_grad():
			err, cover = eval_metrics.depth_error_mm(rdr(Meshes(x.detach(), gf), R, T, **kw), gt, return_coverage=True)
		assert err.shape == (3,) and err.dtype == torch.float64 and cover.shape == (3,)
		return err, cover
	before, cover = metric()
	assert torch.isfinite(before).all() and (cover > 0.8).all() and (cover <= 1).all() and before.max().item() < 4 and before.max().item() > 1
	for _ in range(10):
		opt.zero_grad()
		crit(rdr(Meshes(x, gf), R, T, **kw)['depth'].reshape(3, -1), gt['depth'].reshape(3, -1)).backward()
		opt.step()
	after, _ = metric()
	print('depth_error_mm before', before.tolist(), 'after', after.tolist())
	assert (after.mean() < 0.8 * before.mean()).item()
	# identical maps: 0; no shared pixel: NaN
	same, cover = eval_metrics.depth_error_mm(gt, gt, return_coverage=True)
	assert (same == 0).all() and (cover == 1).all()
	empty = dict(depth=torch.full_like(gt['depth'], -1))
	err, cover = eval_metrics.depth_error_mm(empty, gt, return_coverage=True)
	assert torch.isnan(err).all() and (cover == 0).all()
	assert torch.isnan(eval_metrics.depth_error_mm(gt, empty, return_coverage=True)[1]).all()


def test_eval_2d_reports_the_depth_columns(tmp_path):
	"""evaluate.eval_2d(depth=True) on the four synthetic scans of test_gpu_eval2d.py (one of them hides faces): the five columns it had,
	and per image the depth error and coverage, against a float64 evaluation of the same renders."""
	from test_gpu_eval2d import _foot3d_val, _model
	from find_amd import evaluate
	from find_amd.dataset import BatchCollator
	from find_amd.renderer import FootRenderer
	ds = _foot3d_val(tmp_path)
	model = _model(len(ds))
	size, nviews, bs = 48, 4, 2
	plain = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3)
	res, per = evaluate.eval_2d(model, ds, image_size=size, nviews=nviews, batch_size=bs, feet_per_call=3, return_per_image=True, depth=True)
	assert list(res) == list(plain) + ['Depth (mm)', 'Depth coverage'] and model.training
	for k in plain:   # (the image render's vertex normals are float atomics: last bits)
		assert abs(res[k] - plain[k]) <= 1e-5 * max(1.0, abs(plain[k])), k
	err, cover = per['Depth (mm)'], per['Depth coverage']
	assert err.shape == (len(ds) * nviews,) and cover.shape == err.shape and err.dtype == torch.float64
	rdr = FootRenderer(image_size=size, device='cuda')
	R, T = rdr.linspace_views(nviews=nviews, dist=0.3, elev_min=-90, elev_max=90)
	collate = BatchCollator(device='cuda').collate_batches
	model.eval()
	want_err, want_cover, hidden = [], [], 0
	with torch.no_grad():
		for i in range(len(ds)):
			batch = collate([ds[i]])
			batch.update({vec.name: vec.data[batch['idx']] for vec in model.latent_vectors_val})
			out = model.get_meshes_from_batch(batch, is_train=False)
			gt = rdr(batch['mesh'], R, T, return_depth=True, mask_out_faces=True, return_mask_out_masks=True)
			pred = rdr(out['meshes'], R, T, return_depth=True)
			w = (~gt['mask_out_masks'])[0].reshape(nviews, -1).double().cpu()
			hidden += int(gt['mask_out_masks'].sum())
			_, pi = depth_loss_ref(pred['depth'][0].reshape(nviews, -1).double().cpu(), gt['depth'][0].reshape(nviews, -1).double().cpu(), w, per_image=True)
			n_gt = ((gt['depth'][0].reshape(nviews, -1).cpu() > 0) & (w > 0)).sum(1).double()
			want_err.append(1000 * pi[:, 0] / pi[:, 1])       # (0 / 0 = nan where nothing is shared)
			want_cover.append(pi[:, 1] / n_gt)
	model.train()
	want_err, want_cover = torch.cat(want_err), torch.cat(want_cover)
	assert hidden > 0 and torch.isfinite(want_err).sum() >= len(ds)
	print('Depth (mm)', res['Depth (mm)'], 'coverage', res['Depth coverage'], 'per image', err.tolist())
	assert torch.allclose(err.cpu(), want_err, rtol=1e-6, atol=1e-9, equal_nan=True)
	assert torch.allclose(cover.cpu(), want_cover, rtol=1e-9, atol=0, equal_nan=True)
	assert abs(res['Depth (mm)'] - float(want_err.nanmean())) <= 1e-6 * float(want_err.nanmean()) and 0 < res['Depth coverage'] <= 1
