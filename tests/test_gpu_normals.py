"""Surface normals on the MI355X: find_vertex_normals_*, find_normal_map_*, find_normal_loss_* against the float64 torch evaluation of
their formulas (test_normals_host.py), and their place in FootRenderer, ModelWithLoss and the Trainer.

Margins: none is a constant of the code under test.  Every comparison also evaluates the same formula in float32 torch on the CPU; with
e32 its worst error against float64, the HIP result must satisfy e_hip <= 4 e32 + 1e-7 scale (scale: the largest reference magnitude; the
factor 4 allows for another summation order).  Each test prints e_hip and e32 (DESIGN 7.4 records them)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
sys.path.insert(0, HERE)

from test_normals_host import normal_loss_ref, normal_map_ref, octahedron, vertex_normals_ref   # noqa: E402


def _held(name, hip, ref64, ref32):
	e_hip = (hip.detach().double().cpu() - ref64).abs().max().item()
	e32 = (ref32.detach().double() - ref64).abs().max().item()
	scale = ref64.abs().max().item()
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  scale {scale:.3e}')
	assert np.isfinite(e_hip) and e_hip <= 4 * e32 + 1e-7 * scale, (name, e_hip, e32, scale)


def _with_grad(fn, x, g, dtype):
	"""fn(x) and d (sum g * fn(x)) / d x in `dtype` on the CPU."""
	x = x.detach().cpu().to(dtype).requires_grad_(True)
	out = fn(x)
	(out * g.detach().cpu().to(dtype)).sum().backward()
	return out.detach(), x.grad


# ------------------------------------------------------------------ vertex normals
def test_vertex_normals_of_an_octahedron():
	from find_amd import functional as FN
	v, f = octahedron()
	n = FN.vertex_normals(v[None].cuda(), f.cuda())
	assert n.shape == (1, 6, 3) and (n[0].cpu() - v).abs().max().item() <= 1e-6
	n2 = FN.vertex_normals((v * 0.03)[None].cuda(), f[None].cuda())   # per-mesh faces, another size: the same unit vectors
	assert (n2[0].cpu() - v).abs().max().item() <= 1e-6


@pytest.fixture(scope='module')
def shared():
	"""synthetic.template(1002) (poles of valence 40) plus a vertex no face touches (V = 1003, no multiple of 64) and a zero-area face,
	N = 3 differently deformed copies; the float64 and float32 references, computed once."""
	from find_amd import synthetic
	v, f = synthetic.template(1002)
	g = torch.Generator().manual_seed(4)
	v = torch.cat([v, torch.tensor([[0.01, 0.02, 0.03]])])
	f = torch.cat([f, torch.tensor([[3, 7, 7]])])
	verts = torch.stack([v * (1 + 0.15 * torch.randn(3, generator=g)) + 0.002 * torch.randn(v.shape, generator=g) for _ in range(3)])
	proj = torch.randn(verts.shape, generator=g)
	ref = {}
	for dt in (torch.float64, torch.float32):
		ref[dt] = [_with_grad(lambda x: vertex_normals_ref(x, f), verts[i], proj[i], dt) for i in range(3)]
	return verts, f, proj, ref


def _hip_vertex_normals(verts, faces, proj):
	from find_amd import functional as FN
	x = verts.cuda().requires_grad_(True)
	n = FN.vertex_normals(x, faces)
	(d,) = torch.autograd.grad(n, x, proj.cuda())
	torch.cuda.synchronize()
	return n.detach(), d


def test_vertex_normals_shared_topology_against_float64(shared):
	verts, f, proj, ref = shared
	fc = f.cuda()
	n, d = _hip_vertex_normals(verts, fc, proj)
	assert torch.isfinite(n).all() and torch.isfinite(d).all()
	assert (n[:, 1002] == 0).all() and (d[:, 1002] == 0).all()   # the vertex of no face
	for i in range(3):
		_held(f'vertex normals, mesh {i}', n[i], ref[torch.float64][i][0], ref[torch.float32][i][0])
		_held(f'vertex normals, d verts, mesh {i}', d[i], ref[torch.float64][i][1], ref[torch.float32][i][1])
	n2, d2 = _hip_vertex_normals(verts, fc, proj)
	assert torch.equal(n, n2) and torch.equal(d, d2)


def test_vertex_normals_per_mesh_faces():
	from find_amd import functional as FN
	from find_amd import synthetic
	from find_amd.structures import Meshes
	(v1, f1), (v2, f2) = synthetic.ellipsoid_mesh(4, 9), synthetic.ellipsoid_mesh(10, 10)
	assert v1.shape[0] == 38 and v2.shape[0] == 102
	m = Meshes([v1.cuda(), v2.cuda()], [f1.cuda(), f2.cuda()])
	assert m.verts_padded().shape == (2, 102, 3) and m.faces_padded().shape == (2, 200, 3) and (m.faces_padded()[0, 72:] == -1).all()
	n = m.verts_normals_padded()
	torch.cuda.synchronize()
	for i, (v, f) in enumerate(((v1, f1), (v2, f2))):
		V = v.shape[0]
		_held(f'per-mesh faces, mesh {i}', n[i, :V], vertex_normals_ref(v.double(), f), vertex_normals_ref(v, f))
	assert (n[0, 38:] == 0).all()   # padding vertices: no face touches them
	assert torch.equal(n, m.verts_normals_padded())
	# the same faces given per mesh and shared: the same table order, the same bits
	g = torch.Generator().manual_seed(2)
	two = torch.stack([v2, v2 * 1.1 + 0.001 * torch.randn(v2.shape, generator=g)]).cuda()
	per_mesh = FN.vertex_normals(two, torch.stack([f2, f2]).cuda())
	assert torch.equal(per_mesh, FN.vertex_normals(two, f2.cuda()))
	assert torch.equal(per_mesh, FN.vertex_normals(two, f2[None].cuda()))   # (1, F, 3): one list for both


# ------------------------------------------------------------------ normal map
def _rotations(M, seed):
	q, r = torch.linalg.qr(torch.randn(M, 3, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
	q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
	return q * torch.linalg.det(q)[:, None, None]


def test_normal_map_against_float64():
	from find_amd import functional as FN
	N, M, H, W = 2, 3, 16, 16
	g = torch.Generator().manual_seed(7)
	raw = torch.randn(N, M, H, W, 3, generator=g) * torch.rand(N, M, H, W, 1, generator=g) * 3
	raw[torch.rand(N, M, H, W, generator=g) < 0.2] = 0
	raw[0, 1, 0, 0] = torch.tensor([5e-7, 0, 0])   # under the threshold: zero as well
	R = _rotations(M, 1)
	assert (R[0] - R[1]).abs().max() > 0.1 and (R[1] - R[2]).abs().max() > 0.1
	proj = torch.randn(N, M, H, W, 3, generator=g)
	for space in ('view', 'world'):
		world = space == 'world'
		x = raw.cuda().requires_grad_(True)
		out = FN.normal_map(x, None if world else R.float().cuda(), space=space)
		(d,) = torch.autograd.grad(out, x, proj.cuda())
		o64, d64 = _with_grad(lambda t: normal_map_ref(t, R, world), raw, proj, torch.float64)
		o32, d32 = _with_grad(lambda t: normal_map_ref(t, R.float(), world), raw, proj, torch.float32)
		_held(f'normal map ({space})', out, o64, o32)
		_held(f'normal map ({space}), d raw', d, d64, d32)
		zero = (raw.norm(dim=-1) <= 1e-6)
		assert zero.sum() > 100 and (out[zero.cuda()] == 0).all() and (d[zero.cuda()] == 0).all()
		flat = FN.normal_map(raw.cuda().reshape(N * M, H, W, 3), None if world else R.float().cuda(), space=space)
		assert torch.equal(flat.reshape(out.shape), out)
	# the rotation is the view's: image = mesh * M + view
	w = FN.normal_map(raw.cuda(), None, space='world')
	v = FN.normal_map(raw.cuda(), R.float().cuda())
	for m in range(M):
		assert (torch.einsum('nhwj,jk->nhwk', w[:, m].double().cpu(), R[m]) - v[:, m].double().cpu()).abs().max() < 1e-6


# ------------------------------------------------------------------ normal loss
def _loss_inputs(shape, seed):
	g = torch.Generator().manual_seed(seed)
	p = torch.randn(*shape, 3, generator=g) * (0.2 + torch.rand(*shape, 1, generator=g))
	t = torch.randn(*shape, 3, generator=g) * (0.5 + 4 * torch.rand(*shape, 1, generator=g))   # not unit
	p[torch.rand(shape, generator=g) < 0.1] = 0
	t[torch.rand(shape, generator=g) < 0.1] = 0
	w = torch.rand(shape, generator=g)
	w[torch.rand(shape, generator=g) < 0.3] = 0
	return p, t, w


def _hip_loss(p, t, w, gl=1.7):
	from find_amd import functional as FN
	x = p.cuda().requires_grad_(True)
	loss = FN.normal_loss(x, t.cuda(), w.cuda())
	assert loss.dim() == 0 and loss.dtype == torch.float32
	(d,) = torch.autograd.grad(loss * gl, x)
	torch.cuda.synchronize()
	return loss.detach(), d


@pytest.mark.parametrize('shape', [(3, 37, 29), (5, 64, 64)])
def test_normal_loss_against_float64(shape):
	"""(3, 37, 29): 3219 pixels, no multiple of 4, the last workgroup partly filled; (5, 64, 64): 20 workgroups for the second stage."""
	p, t, w = _loss_inputs(shape, sum(shape))
	gl = 1.7
	loss, d = _hip_loss(p, t, w, gl)
	ref = {}
	for dt in (torch.float64, torch.float32):
		x = p.to(dt).requires_grad_(True)
		l = normal_loss_ref(x, t.to(dt), w.to(dt))
		(l * gl).backward()
		ref[dt] = (l.detach(), x.grad)
	_held(f'normal loss {shape}', loss, ref[torch.float64][0], ref[torch.float32][0])
	_held(f'normal loss {shape}, d pred', d, ref[torch.float64][1], ref[torch.float32][1])
	dead = ((p.norm(dim=-1) <= 1e-6) | (t.norm(dim=-1) <= 1e-6) | (w == 0)).cuda()
	assert dead.sum() > 100 and (d[dead] == 0).all()
	loss2, d2 = _hip_loss(p, t, w, gl)
	assert torch.equal(loss, loss2) and torch.equal(d, d2)
	# an unaligned view takes the scalar path: the same per-pixel arithmetic, the same sums
	from find_amd import functional as FN
	buf = torch.zeros(p.numel() + 1, device='cuda')
	buf[1:] = p.cuda().reshape(-1)
	off = buf[1:].view(*shape, 3)
	assert off.data_ptr() % 16 and torch.equal(FN.normal_loss(off, t.cuda(), w.cuda()), loss)


def test_normal_loss_with_all_weights_zero():
	p, t, w = _loss_inputs((3, 37, 29), 1)
	loss, d = _hip_loss(p, t, torch.zeros_like(w))
	assert loss.item() == 0.0 and (d == 0).all()


# ------------------------------------------------------------------ FootRenderer
@pytest.fixture(scope='module')
def scene():
	from find_amd import synthetic
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes
	gv, gf, _ = synthetic.gt_feet(2, 1002, seed=5, device='cuda')
	rdr = FootRenderer(image_size=32, device='cuda')
	R, T = rdr.view_from(['topdown', 'side1'])
	return rdr, gv, gf, R.cuda().float(), T.cuda().float(), Meshes


def test_renderer_normals_are_the_feature_render_of_the_vertex_normals(scene):
	from find_amd import functional as FN
	rdr, gv, gf, R, T, Meshes = scene
	m = Meshes(gv, gf)
	out = rdr(m, R, T, return_images=False, return_normals=True)
	assert set(out) == {'normals'} and out['normals'].shape == (2, 2, 32, 32, 3)
	feats = rdr(m, R, T, return_images=False, return_features=True, features=FN.vertex_normals(gv, gf))['features']
	assert torch.equal(out['normals'], FN.normal_map(feats, R))
	ln = out['normals'].norm(dim=-1)
	inside = ln > 0
	assert inside.any() and not inside.all() and (ln[inside] - 1).abs().max().item() < 1e-5
	assert torch.equal(rdr(m, R, T, return_images=False, return_normals=True, normals_space='world')['normals'], FN.normal_map(feats, None, space='world'))
	# with other features in the same call: both are what the separate calls give
	other = torch.randn(2, gv.shape[1], 5, generator=torch.Generator().manual_seed(0)).cuda()
	both = rdr(m, R, T, return_images=False, return_mask=True, return_normals=True, return_features=True, features=other)
	assert torch.equal(both['normals'], out['normals'])
	assert torch.equal(both['features'], rdr(m, R, T, return_images=False, return_features=True, features=other)['features'])
	# hidden pixels
	hide = torch.arange(0, gf.shape[0] // 2, device='cuda')
	hid = rdr(m, R, T, return_images=False, return_normals=True, mask_out_faces=True, masked_faces=hide, return_mask_out_masks=True)
	mo = hid['mask_out_masks']
	assert mo.any() and not mo.all() and (hid['normals'][mo] == 0).all() and torch.equal(hid['normals'][~mo], out['normals'][~mo])


def test_renderer_normals_gradient_reaches_the_vertices(scene):
	from find_amd import functional as FN
	rdr, gv, gf, R, T, Meshes = scene
	g = torch.randn(2, 2, 32, 32, 3, generator=torch.Generator().manual_seed(3)).cuda()

	def composition():
		x = gv.clone().requires_grad_(True)
		feats = rdr(Meshes(x, gf), R, T, return_images=False, return_features=True, features=FN.vertex_normals(x, gf))['features']
		(d,) = torch.autograd.grad(FN.normal_map(feats, R), x, g)
		return d
	x = gv.clone().requires_grad_(True)
	(d,) = torch.autograd.grad(rdr(Meshes(x, gf), R, T, return_images=False, return_normals=True)['normals'], x, g)
	c1, c2 = composition(), composition()
	torch.cuda.synchronize()
	rr = (c1 - c2).abs().max().item()   # the feature render's backward accumulates with float atomics
	err = (d - c1).abs().max().item()
	print(f'd verts through out[normals]: err {err:.3e}  run-to-run {rr:.3e}  max |d| {c1.abs().max().item():.3e}')
	assert torch.isfinite(d).all() and c1.abs().max().item() > 0
	assert err <= 4 * rr + 1e-6 * g.abs().max().item(), (err, rr)


# ------------------------------------------------------------------ ModelWithLoss, Trainer
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
	# the scans carry their faces per mesh, as ragged GT scans do: the step builds their corner tables on the device
	batch = dict(mesh=Meshes(gv, gf[None].expand(n, -1, -1).contiguous(), TexturesVertex(gc.clamp(0.05, 0.95))), idx=torch.arange(n, device='cuda'),
				 name=[f'{i:04d}' for i in range(n)])
	opt = optim.Adam(mwl.model.main_params, lr=1e-4, capturable=True)
	return mwl, opts, batch, opt


def _sampled(mwl, batch):
	from find_amd.train_utils import sample_latent_vectors
	b = dict(batch)
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	return b


def test_model_with_loss_reports_the_normal_term(step):
	from find_amd import functional as FN
	from find_amd.opts import Opts
	mwl, opts, batch, opt = step
	b = _sampled(mwl, batch)
	flags = dict(sil=True, render_foot=True, return_renders=True)
	np.random.seed(5)
	loss, losses, rdr = mwl(b, 0, opts, normal=True, **flags)
	assert list(losses) == ['loss_sil', 'loss_normal']
	pn, gn = rdr['pred']['normals_raw'], rdr['gt']['normals_raw']
	assert pn.shape == (2, 2, 32, 32, 3) and gn.shape == pn.shape and pn.requires_grad and not gn.requires_grad
	weight = rdr['gt']['mask'] * rdr['pred']['mask'].detach()
	assert (weight > 0).any() and (weight == 0).any()
	want = FN.normal_loss(pn, gn, weight).item() * opts.weight_normal
	got = losses['loss_normal'].item()
	print('loss_normal', got, want)
	assert 0 < got < 2 and abs(got - want) <= 1e-6 * want
	# gradients of the term alone reach the network and the registration
	mwl.zero_grad()
	losses['loss_normal'].backward()
	torch.cuda.synchronize()
	grads = [p.grad for p in mwl.model.main_params if p.grad is not None]
	assert grads and all(torch.isfinite(q).all() for q in grads) and any(q.abs().max().item() > 0 for q in grads)
	rg = dict(mwl.model.named_parameters())['reg.data'].grad
	assert rg is not None and torch.isfinite(rg).all() and rg.abs().max().item() > 0
	mwl.zero_grad()
	# twice the weight, twice the term
	np.random.seed(5)
	_, losses2, _ = mwl(b, 0, Opts(sil_loss=True, num_views=2, weight_normal=2.), normal=True, **flags)
	assert abs(losses2['loss_normal'].item() - 2 * got) <= 1e-6 * got and torch.equal(losses2['loss_sil'], losses['loss_sil'])
	# a reference Opts has no weight_normal: 1
	class Bare:
		pass
	bare = Bare()
	bare.__dict__.update({k: v for k, v in vars(opts).items() if k not in ('normal_loss', 'weight_normal')})
	np.random.seed(5)
	_, losses3, _ = mwl(b, 0, bare, normal=True, **flags)
	assert torch.equal(losses3['loss_normal'], losses['loss_normal'])
	# flag off: what a call that never mentions it returns, bit for bit, and no normal render
	np.random.seed(5)
	loss_a, losses_a, rdr_a = mwl(b, 0, opts, **flags)
	np.random.seed(5)
	loss_b, losses_b, rdr_b = mwl(b, 0, opts, normal=False, **flags)
	assert list(losses_a) == list(losses_b) == ['loss_sil'] and torch.equal(loss_a, loss_b) and torch.equal(losses_a['loss_sil'], losses_b['loss_sil'])
	assert torch.equal(losses_a['loss_sil'], losses['loss_sil'])
	assert set(rdr_a['pred']) == set(rdr_b['pred']) and 'normals_raw' not in rdr_b['pred'] and 'normals_raw' not in rdr_b['gt']
	# without renders the term is skipped silently, as pix is
	_, losses_c = mwl(b, 0, opts, normal=True, pix=True, smooth=True, render_foot=False)
	assert list(losses_c) == ['loss_smooth']


def test_normal_term_alone_renders_no_image(step):
	"""The term reads no colours: a step with it alone renders masks and normals only."""
	mwl, opts, batch, opt = step
	np.random.seed(5)
	loss, losses = mwl(_sampled(mwl, batch), 0, opts, normal=True, render_foot=True)
	assert list(losses) == ['loss_normal'] and torch.isfinite(loss).item() and torch.equal(loss, losses['loss_normal'])


def test_normal_term_beside_the_part_loss(step, tmp_path):
	"""Both feature consumers in one step: the normals ride as channels 0-2 in front of the 21 class logits of one raster pass.  The normal
	term is then what it is alone -- the same per-channel arithmetic in the same first chunk of channels; 1e-5 relative leaves room for a
	kernel that rounds a 24-channel blend differently from a 3-channel one, far below what a wrong slice would give."""
	from test_gpu_part_loss import StubEncoder
	from find_amd import synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	from find_amd.renderer import FootRenderer
	mwl0, _, batch, _ = step
	v, f = synthetic.template(1002)
	path = str(tmp_path / 'classes.pth')
	torch.save({'state_dict': {'features': torch.randn(v.shape[0], 21, generator=torch.Generator().manual_seed(1))}}, path)
	opts = Opts(sil_loss=True, restyle_perc_cluster_loss=True, restyle_cluster_per_vertex=True, template_features_pth=path, num_views=2,
				restyle_feature_maps=[8])
	mwl = ModelWithLoss(opts=opts, device='cpu', restyle_encoder=StubEncoder(21), use_shapevec=True, use_texvec=True, use_posevec=True, train_size=2,
						val_size=1, shapevec_size=100, texvec_size=100, posevec_size=100, template_mesh_loc=None, restyle_cluster_per_vertex=True)
	mwl = mwl.to('cuda')
	mwl.model.set_template(v.cuda(), f.cuda())
	mwl.rdr = FootRenderer(image_size=32, device='cuda')
	own = dict(mwl.model.named_parameters())
	with torch.no_grad():   # the weights and codes of the fixture's model
		for k, q in mwl0.model.named_parameters():
			own[k].copy_(q)
	b = _sampled(mwl, batch)
	flags = dict(sil=True, render_foot=True, return_renders=True, restyle_feature_maps=[8])
	np.random.seed(5)
	_, alone, _ = mwl(b, 0, opts, normal=True, **flags)
	np.random.seed(5)
	loss, losses, rdr = mwl(b, 0, opts, normal=True, restyle_perc_cluster=True, **flags)
	assert list(losses) == ['loss_sil', 'loss_restyle_perc_cluster', 'loss_normal']
	assert rdr['pred']['features'].shape == (2, 2, 32, 32, 21) and rdr['pred']['normals_raw'].shape == (2, 2, 32, 32, 3)
	a, c = alone['loss_normal'].item(), losses['loss_normal'].item()
	print('loss_normal alone', a, 'beside the part loss', c)
	assert a > 0 and abs(a - c) <= 1e-5 * a and torch.isfinite(losses['loss_restyle_perc_cluster']).item()
	np.random.seed(5)
	_, part, rdr_p = mwl(b, 0, opts, restyle_perc_cluster=True, **flags)
	assert abs(part['loss_restyle_perc_cluster'].item() - losses['loss_restyle_perc_cluster'].item()) <= 1e-5 * abs(part['loss_restyle_perc_cluster'].item())
	loss.backward()
	torch.cuda.synchronize()
	assert mwl.model.per_vertex_features.grad is not None and torch.isfinite(mwl.model.per_vertex_features.grad).all()
	assert all(torch.isfinite(q.grad).all() for q in mwl.model.main_params if q.grad is not None)


def test_normal_term_on_the_pca_model(tmp_path):
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
	loss, losses = mwl(b, 0, opts, normal=True, sil=True, render_foot=True)
	assert list(losses) == ['loss_sil', 'loss_normal'] and torch.isfinite(losses['loss_normal']).item()
	losses['loss_normal'].backward()
	g = dict(mwl.model.named_parameters())['shapevec.data'].grad
	assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0


def test_trainer_runs_the_term_eagerly(step):
	from find_amd.trainer import Trainer
	mwl, opts, batch, opt = step
	kw = dict(sil=True, normal=True, render_foot=True)
	tr = Trainer([opt], mwl, [batch, batch], [], opts, latent_vectors_train=mwl.model.latent_vectors_train, device='cuda', graph='auto')
	assert 'normal' in tr._why_not_graph(tr.optims, kw)
	np.random.seed(3)
	msg = tr.train_epoch(0, model_kwargs=dict(kw))
	assert tr.last_mode == 'eager', msg
	vals = tr.log[0]['train_loss']['Normal']
	assert len(vals) == 2 and all(np.isfinite(vals)) and all(np.isfinite(tr.log[0]['train_loss']['Sil']))
	tr.graph = True
	with pytest.raises(RuntimeError, match='normal'):
		tr.train_epoch(1, model_kwargs=dict(kw))
