"""Split mode of the HIP renderer (make_params(clip_faces=True) / FootRenderer(..., clip_faces=True)): faces that straddle the z-clip
plane are clipped as PyTorch3D's rasterize_meshes does, instead of being rasterised whole and reported.

The reference is the local clip of tests/test_zclip_host.py (float64) feeding the unmodified oracle: the projected mesh is pre-split
into one face per slot, rasterised by oracle.render_ref.rasterize, and pix_to_face / the barycentrics are converted back to the
original faces; gradients come from torch autograd through the same clip and the oracle's torch fragment functions.  Tolerances are
those of tests/test_gpu_render.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import camera_ref, render_ref
from test_zclip_host import clip_split

pytestmark = pytest.mark.gpu

TOL = 1e-4
GRAD_TOL = 1e-4
ZC = 0.01


@pytest.fixture(autouse=True, params=['list', 'band'])
def rasteriser(request):
	"""Both forward rasterisers (switch bits 4096 / 2048 of find_render_switches force one at every size, as in test_gpu_render.py)."""
	from find_amd import _lib
	_lib.set_tuning('raster_ablate', 2048 if request.param == 'band' else 4096)
	yield request.param
	_lib.set_tuning('raster_ablate', 0)


def _ellipsoid(n_meshes=2, rings=14, segs=18, seed=0):
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(rings, segs)
	g = torch.Generator().manual_seed(seed)
	verts = v[None] * (1 + 0.1 * torch.rand(n_meshes, 1, 3, generator=g)) + 0.002 * torch.randn(n_meshes, v.shape[0], 3, generator=g)
	cols = torch.rand(n_meshes, v.shape[0], 3, generator=g)
	return verts, f, cols


def _views(dist, elev, azim):
	R, T = camera_ref.look_at_view_transform(dist=np.asarray(dist, np.float64), elev=np.asarray(elev, np.float64),
											 azim=np.asarray(azim, np.float64), up=((1, 0, 0),))
	return torch.from_numpy(R), torch.from_numpy(T)


def _gpu(verts, faces, cols, R, T, size, clip, **kw):
	from find_amd import functional_render as FR
	params = FR.make_params(size, clip_faces=clip)
	return FR.render(verts.cuda(), cols.cuda() if cols is not None else None, faces.cuda(), R.cuda(), T.cuda(), params, **kw)


# ---------------------------------------------------------------------------------------------- reference
def _split_np(verts, faces, R, T, size):
	rp = render_ref.default_params(size)
	vproj = torch.from_numpy(render_ref.project(rp, verts.numpy(), R.numpy(), T.numpy()).astype(np.float64))
	vs, fs, conv, live = clip_split(vproj, faces, ZC)
	return rp, vs.numpy().astype(np.float32), fs.numpy().astype(np.int32), conv.numpy(), fs.shape[1]


def _to_orig(p2f_s, bary_s, conv, F2):
	"""Slot ids (packed img * 2F + slot) and sub-triangle barycentrics -> original packed ids and barycentrics."""
	F = F2 // 2
	img = np.arange(p2f_s.shape[0]).reshape(-1, *([1] * (p2f_s.ndim - 1)))
	slot = np.where(p2f_s >= 0, p2f_s - img * F2, 0)
	p2f = np.where(p2f_s >= 0, img * F + slot % F, -1)
	c = conv[np.broadcast_to(img, slot.shape), slot]      # (..., 3, 3)
	bary = np.einsum('...k,...ki->...i', bary_s, c)
	return p2f, bary


def reference(verts, faces, cols, R, T, size):
	"""dict(mask, image, pix_to_face, zbuf) of the split mode, from the local clip + the oracle."""
	rp, vs, fs, conv, F2 = _split_np(verts, faces, R, T, size)
	N, M = verts.shape[0], R.shape[0]
	p2f, zb, ba, di = render_ref.rasterize(vs, fs, 1, size, size, rp.sil_faces_per_pixel, rp.sil_blur_radius, z_clip=rp.z_clip)
	out = {'mask': render_ref.silhouette(p2f, di, rp.sil_sigma).reshape(N, M, size, size)}
	p1, z1, b1, d1 = render_ref.rasterize(vs, fs, 1, size, size, 1, 0.0, z_clip=rp.z_clip)
	po, bo = _to_orig(p1, b1, conv, F2)
	po, bo = np.ascontiguousarray(po, np.int32), np.ascontiguousarray(bo, np.float32)
	if cols is not None:
		vv = np.ascontiguousarray(verts.numpy(), np.float32)
		nrm = render_ref.vertex_normals(vv, faces.numpy())
		fc = np.ascontiguousarray(faces.numpy(), np.int32)
		cc = np.ascontiguousarray(camera_ref.camera_center(R.numpy(), T.numpy()), np.float32)
		img = np.empty((N * M, size, size, 3), np.float32)
		P = render_ref._p
		render_ref.lib().ref_phong_blend(ctypes.byref(rp), P(po), P(z1), P(bo), P(d1), P(vv), P(nrm), P(np.ascontiguousarray(cols.numpy(), np.float32)),
										 P(fc), 1, P(cc), N * M, M, verts.shape[1], fc.shape[-2], P(img))
		out['image'] = img.reshape(N, M, size, size, 3)
	out['pix_to_face'] = po[..., 0].reshape(N, M, size, size)
	out['zbuf'] = z1[..., 0].reshape(N, M, size, size)
	out['bary'] = bo[..., 0, :].reshape(N, M, size, size, 3)
	out['_split'] = (vs, fs, conv, F2, p2f, p1)
	return out


def torch_reference(verts, cols, faces, R, T, size, p2f_s, p1_s, want):
	"""Differentiable mask / image of the split mode given the oracle's selections on the pre-split mesh (p2f_s: K = 100, p1_s: K = 1)."""
	rp = render_ref.default_params(size)
	N, M = verts.shape[0], R.shape[0]
	vproj = render_ref.torch_project(verts, R.to(verts.dtype), T.to(verts.dtype), rp.fov_deg)
	vs, fs, conv, live = clip_split(vproj, faces, ZC)
	fs = fs.clamp(min=0)   # (an empty slot is never selected; a valid index keeps the padding's arithmetic finite)
	F2 = fs.shape[1]
	if want == 'mask':
		pz, bary, dist, valid, fv = render_ref.torch_fragments(vs, fs, torch.from_numpy(p2f_s).long(), 1, size, size, clip_bary=True)
		return render_ref.torch_silhouette(dist, valid, rp.sil_sigma).reshape(N, M, size, size)
	p1 = torch.from_numpy(p1_s).long()
	pz, bs, dist, valid, fv = render_ref.torch_fragments(vs, fs, p1, 1, size, size, clip_bary=False)
	n_img = vproj.shape[0]
	img = torch.arange(n_img).view(n_img, 1, 1, 1)
	slot = torch.where(p1 >= 0, p1 - img * F2, torch.zeros_like(p1))
	c = conv[img.expand_as(slot), slot]                              # (n_img, H, W, 1, 3, 3)
	bary = torch.einsum('...k,...ki->...i', bs, c)
	face = faces.long()[slot % (F2 // 2)]                            # (n_img, H, W, 1, 3)
	mesh = (img // M).unsqueeze(-1).expand_as(face)
	nrm = render_ref.torch_vertex_normals(verts, faces)

	def interp(attr):
		return (bary.unsqueeze(-1) * attr[mesh, face]).sum(dim=-2)
	pos, nn, tex = interp(verts), interp(nrm), interp(cols)
	n = nn / nn.norm(dim=-1, keepdim=True).clamp(min=1e-6)
	light = torch.tensor(list(rp.light_pos), dtype=verts.dtype)
	l = light - pos
	l = l / l.norm(dim=-1, keepdim=True).clamp(min=1e-6)
	cosang = (n * l).sum(-1)
	diff = rp.diffuse * torch.relu(cosang)
	cc = -torch.einsum('mj,mij->mi', T.to(verts.dtype), R.to(verts.dtype))
	vd = cc[(img % M).view(n_img, 1, 1).expand(p1.shape[:-1]).unsqueeze(-1)] - pos
	vd = vd / vd.norm(dim=-1, keepdim=True).clamp(min=1e-6)
	r = -l + 2 * cosang.unsqueeze(-1) * n
	al = torch.relu((vd * r).sum(-1)) * (cosang > 0)
	spec = rp.specular * al ** rp.shininess
	col = (rp.ambient + diff).unsqueeze(-1) * tex + spec.unsqueeze(-1)
	bg = torch.tensor(list(rp.background), dtype=verts.dtype)
	out = render_ref.torch_softmax_blend(col, dist, pz, valid, rp.rgb_sigma, rp.rgb_gamma, rp.znear, rp.zfar, bg)
	return out.reshape(N, M, size, size, 3)


def _check_forward(got, ref, min_same=0.998):
	mask, image, p2f, zbuf = [t.cpu().numpy() if t is not None else None for t in got]
	em = np.abs(mask - ref['mask']).max()
	assert em < TOL, em
	same = p2f == ref['pix_to_face']
	assert same.mean() >= min_same, same.mean()
	ez = np.abs(zbuf - ref['zbuf'])[same].max()
	assert ez < 1e-5, ez
	if image is not None:
		ei = np.abs(image - ref['image'])[same].max()
		assert ei < TOL, ei
	return same


# ---------------------------------------------------------------------------------------------- 1. no crossing faces: bit-identical
@pytest.mark.parametrize('size', [64, 512])
@pytest.mark.parametrize('per_mesh', [False, True])
def test_without_crossing_faces_the_split_mode_equals_the_default(size, per_mesh):
	"""Mask, pix_to_face and zbuf bit for bit; image and gradients to the default mode's own run-to-run spread (vertex normals and the
	backward's vertex sums are float atomics, whose order varies between any two runs)."""
	verts, faces, cols = _ellipsoid()
	R, T = _views([0.3, 0.3], [20.0, -50.0], [10.0, 70.0])
	if per_mesh:
		faces = torch.stack([faces, faces.flip(0)])
	outs = []
	for clip in (False, True, False):
		vg = verts.clone().cuda().requires_grad_(True)
		cg = cols.clone().cuda().requires_grad_(True)
		mask, image, p2f, zbuf = _gpu(vg, faces, cg, R, T, size, clip, want_frags=True)
		g = torch.Generator().manual_seed(3)
		wm, wi = torch.rand(mask.shape, generator=g).cuda(), torch.rand(image.shape, generator=g).cuda()
		((mask * wm).sum() + (image * wi).sum()).backward()
		outs.append([t.detach() for t in (mask, image, p2f, zbuf, vg.grad, cg.grad)])
	d0, s, d1 = outs
	for i in (0, 2, 3):
		assert torch.equal(d0[i], s[i]), i
	for i in (1, 4, 5):
		spread = (d0[i] - d1[i]).abs().max().item()
		scale = d0[i].abs().max().item()
		err = (d0[i] - s[i]).abs().max().item()
		assert err <= max(4 * spread, 1e-5 * scale), (i, err, spread, scale)   # (1e-5: ten times below the gradient tests' bound)


# ---------------------------------------------------------------------------------------------- 2. shallow crossing
def test_shallow_crossing_matches_the_default_oracle_behind_the_plane_and_the_clip_in_front():
	"""Crossing vertices at 0 < z < z_clip: the unclipped render is well defined.  Where its nearest fragment lies behind the plane the
	split render equals it; in front of the plane the clipped reference decides."""
	verts, faces, cols = _ellipsoid(n_meshes=1)
	R, T = _views([0.06], [0.0], [0.0])
	z0 = render_ref.project(render_ref.default_params(64), verts.numpy(), R.numpy(), T.numpy())[0, :, 2].min()
	R, T = _views([0.06 - z0 + 0.005, 0.3], [0.0, 30.0], [0.0, 40.0])   # the nearest vertex 5 mm in front of the camera
	vz = render_ref.project(render_ref.default_params(64), verts.numpy(), R.numpy(), T.numpy())[0, :, 2]
	assert vz.min() > 0 and (vz < ZC).sum() > 0
	for size in (64, 512):
		got = _gpu(verts, faces, cols, R, T, size, True, want_frags=True)
		unclipped = render_ref.render(verts.numpy(), faces.numpy(), cols.numpy(), R.numpy(), T.numpy(), image_size=size)
		ref = reference(verts, faces, cols, R, T, size)
		same = _check_forward(got, ref)
		p2f, zbuf, image = got[2].cpu().numpy(), got[3].cpu().numpy(), got[1].cpu().numpy()
		behind = (unclipped['zbuf'] >= ZC * 1.01) & (unclipped['pix_to_face'] == p2f)
		assert behind.sum() > 100
		assert np.abs(zbuf - unclipped['zbuf'])[behind].max() < 1e-5
		assert np.abs(image - unclipped['image'])[behind].max() < TOL
		front = (unclipped['pix_to_face'] >= 0) & (unclipped['zbuf'] < ZC)
		assert front.sum() > 0 and same[front].mean() > 0.99
		assert (zbuf[p2f >= 0] >= ZC * (1 - 1e-6)).all()


# ---------------------------------------------------------------------------------------------- 3. camera inside the mesh
@pytest.mark.parametrize('size', [64, 512])
def test_camera_inside_the_mesh_in_a_mixed_batch(size):
	"""The scene of test_gpu_render.py's straddle test (1002-vertex template, camera 0.02 m from the origin) beside clean views; under
	FLAG_POLICY = 'sync' nothing is raised."""
	from find_amd import functional_render as FR
	from find_amd import synthetic
	v, f = synthetic.template(1002)
	verts = v[None].clone()
	cols = torch.rand(1, v.shape[0], 3, generator=torch.Generator().manual_seed(9))
	R, T = _views([0.3, 0.02, 0.3, 0.02], [0.0, 0.0, 45.0, 30.0], [0.0, 0.0, 20.0, 60.0])
	prev, FR.FLAG_POLICY = FR.FLAG_POLICY, 'sync'
	try:
		got = _gpu(verts, f, cols, R, T, size, True, want_frags=True)
		FR.check_render_flags(wait=True)
	finally:
		FR.FLAG_POLICY = prev
	ref = reference(verts, f, cols, R, T, size)
	_check_forward(got, ref)
	# the inside views are not empty and show the far wall in front of the plane's cut
	p2f = got[2].cpu().numpy()
	assert (p2f[0, 1] >= 0).mean() > 0.5 and (p2f[0, 3] >= 0).mean() > 0.5


# ---------------------------------------------------------------------------------------------- 4. gradients
@pytest.mark.parametrize('size', [48, 512])
def test_gradients_through_the_clip_vs_autograd(size):
	"""d_verts from a mask loss and d_verts / d_colors from an image loss against torch autograd through the local clip."""
	from find_amd import synthetic
	v, f = synthetic.ellipsoid_mesh(8, 10)
	verts = v[None].clone() + 0.001 * torch.randn(1, v.shape[0], 3, generator=torch.Generator().manual_seed(1))
	cols = torch.rand(1, v.shape[0], 3, generator=torch.Generator().manual_seed(2))
	R, T = _views([0.02, 0.3, 0.046], [0.0, 20.0, 0.0], [0.0, 30.0, 0.0])
	ref = reference(verts, f, cols, R, T, size)
	vs, fs, conv, F2, p2f_s, p1_s = ref['_split']
	# mask
	vg = verts.clone().cuda().requires_grad_(True)
	mask = _gpu(vg, f, None, R, T, size, True, want_image=False)[0]
	gt = torch.rand(mask.shape, generator=torch.Generator().manual_seed(4))
	((mask - gt.cuda()) ** 2).sum().backward()
	vr = verts.clone().double().requires_grad_(True)
	rm = torch_reference(vr, None, f, R, T, size, p2f_s, p1_s, 'mask')
	assert (mask.detach().cpu() - rm.detach().float()).abs().max().item() < TOL
	((rm - gt.double()) ** 2).sum().backward()
	sc = vr.grad.abs().max().item()
	err = (vg.grad.cpu().double() - vr.grad).abs().max().item()
	print(f'mask gradient @{size}: {err:.2e} of {sc:.2e}')
	assert sc > 0 and err < GRAD_TOL * sc, (err, sc)
	# image
	vg = verts.clone().cuda().requires_grad_(True)
	cg = cols.clone().cuda().requires_grad_(True)
	image = _gpu(vg, f, cg, R, T, size, True, want_mask=False)[1]
	w = torch.rand(image.shape, generator=torch.Generator().manual_seed(5))
	(image * w.cuda()).sum().backward()
	vr = verts.clone().double().requires_grad_(True)
	cr = cols.clone().double().requires_grad_(True)
	ri = torch_reference(vr, cr, f, R, T, size, p2f_s, p1_s, 'image')
	assert (image.detach().cpu() - ri.detach().float()).abs().max().item() < TOL
	(ri * w.double()).sum().backward()
	for name, a, b in (('verts', vg.grad, vr.grad), ('colors', cg.grad, cr.grad)):
		sc = b.abs().max().item()
		err = (a.cpu().double() - b).abs().max().item()
		print(f'image gradient ({name}) @{size}: {err:.2e} of {sc:.2e}')
		assert sc > 0 and err < GRAD_TOL * sc, (name, err, sc)


# ---------------------------------------------------------------------------------------------- 5. GT path
def test_render_uv_clips_a_crossing_view():
	"""render_uv (GT scans) with clip_faces=True on a camera inside the mesh: a map linear in (u, v) reproduces the per-vertex-colour
	reference, through the converted face ids and barycentrics of find_render_frags."""
	from find_amd import functional_render as FR
	from find_amd import synthetic
	from find_amd.structures import TexturesUV
	v, f = synthetic.template(1002)
	verts = v[None].clone()
	R, T = _views([0.02], [0.0], [0.0])
	size = 64
	uv = torch.rand(1, v.shape[0], 2, generator=torch.Generator().manual_seed(6))
	Ht = Wt = 64
	gx, gy = torch.meshgrid(torch.linspace(0, 1, Wt), torch.linspace(1, 0, Ht), indexing='xy')
	maps = torch.stack([gx, gy, 0.5 * torch.ones_like(gx)], -1)[None]   # colour (u, v, 0.5): bilinear reads are exact
	tex = TexturesUV(maps=maps.cuda(), faces_uvs=f[None].cuda(), verts_uvs=uv.cuda())
	params = FR.make_params(size, clip_faces=True)
	mask, image, p2f, zbuf = FR.render_uv(verts.cuda(), tex, f.cuda(), R.cuda(), T.cuda(), params, want_frags=True)
	cols = torch.cat([uv, 0.5 * torch.ones(1, v.shape[0], 1)], -1)
	ref = reference(verts, f, cols, R, T, size)
	same = _check_forward((mask, image, p2f, zbuf), ref)
	assert (p2f.cpu().numpy() >= 0).mean() > 0.5


# ---------------------------------------------------------------------------------------------- 6. graph replay
def test_graphed_step_with_a_clipping_renderer_captures_and_replays():
	"""A GraphedStep whose renderer clips, with a camera inside the mesh (sil + render_foot): the split mode needs no host synchronisation,
	so the step captures; with the learning rate at 0 every replay of a batch reproduces the first one bit for bit, and the watchdog,
	read at the boundary, stays silent (the default renderer reports this very step: test_gpu_trainloop.py)."""
	import warnings
	from find_amd import functional_render as FR
	from find_amd import optim
	from find_amd.cameras import look_at_view_transform
	from find_amd.graph import GraphedStep
	from find_amd.renderer import FootRenderer
	from test_gpu_train3d import _setup
	prev = FR.FLAG_POLICY
	FR.FLAG_POLICY = 'warn'
	try:
		FR.check_render_flags(wait=True)
		R, T = look_at_view_transform(dist=np.array([0.02, 0.3]), elev=np.array([0.0, 30.0]), azim=np.array([0.0, 40.0]), up=((1, 0, 0),))
		mwl, opts, batch_of, _, _ = _setup(1002, 1002, capturable=True)
		mwl.rdr = FootRenderer(image_size=64, device='cuda', clip_faces=True)
		assert mwl.rdr.params.clip_faces == 1
		opt = optim.Adam(mwl.model.main_params, lr=0.0, capturable=True)
		gs = GraphedStep(mwl, opts, [opt], warmup=1, sil=True, render_foot=True, views=(R.cuda(), T.cuda()))
		with warnings.catch_warnings(record=True) as wlist:
			warnings.simplefilter('always')
			out = []
			for i in (0, 1, 0, 1):
				loss, _ = gs(batch_of(i))
				out.append(loss.detach().clone())
			FR.check_render_flags(wait=True)
		assert not [w for w in wlist if 'straddle' in str(w.message)], [str(w.message)[:120] for w in wlist]
		assert gs.n_captures >= 1
		vals = [o.item() for o in out]
		assert np.isfinite(vals).all(), vals
		assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3]), vals
	finally:
		FR.FLAG_POLICY = prev


# ---------------------------------------------------------------------------------------------- 7. determinism
def test_split_mode_forward_is_bit_reproducible_and_backward_within_atomics_order():
	"""Two identical split-mode runs on a crossing batch: mask, pix_to_face, zbuf bit for bit (the forward has no float atomics in the
	silhouette path); the image and the gradients -- float atomics into vertex sums, as in the default mode -- within 1e-5 of their scale."""
	from find_amd import synthetic
	v, f = synthetic.template(1002)
	verts = v[None].clone()
	cols = torch.rand(1, v.shape[0], 3, generator=torch.Generator().manual_seed(9))
	R, T = _views([0.02, 0.3, 0.046], [0.0, 45.0, 0.0], [0.0, 20.0, 0.0])
	runs = []
	for _ in range(2):
		vg = verts.clone().cuda().requires_grad_(True)
		cg = cols.clone().cuda().requires_grad_(True)
		mask, image, p2f, zbuf = _gpu(vg, f, cg, R, T, 128, True, want_frags=True)
		g = torch.Generator().manual_seed(3)
		((mask * torch.rand(mask.shape, generator=g).cuda()).sum() + (image * torch.rand(image.shape, generator=g).cuda()).sum()).backward()
		runs.append([t.detach() for t in (mask, p2f, zbuf, image, vg.grad, cg.grad)])
	a, b = runs
	for i in (0, 1, 2):
		assert torch.equal(a[i], b[i]), i
	for i in (3, 4, 5):
		assert (a[i] - b[i]).abs().max().item() <= 1e-5 * a[i].abs().max().item(), i
