"""find_amd.vis on the GPU: find_frames_u8 bit for bit against numpy, a turntable spin against the CPU render oracle on ROTATED VERTICES
(what reference src/vis/mesh_turntable.py:46-62 renders; the library rotates the cameras instead), independence of the chunking, UV scans,
the per-vertex Chamfer errors against float64 brute force, and the two callers: evaluate.eval_3d(produce_spins, export_meshes) and
Trainer.export_meshes."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import camera_ref, mlp_ref, render_ref

pytestmark = pytest.mark.gpu

AZIM, DIST = 70, 0.35   # what eval_3d.py:201 passes (upstream's default azim = -90 looks along the up vector: nothing is drawn)


# ---------------------------------------------------------------------------------------------- find_frames_u8
def _planted():
	k = torch.arange(256, dtype=torch.float32) / 255
	return torch.cat([torch.tensor([0.0, 1.0, -0.5, 1.5, 1 + 1e-7, float('nan'), -0.0]), k, k + 2.0 ** -24, k - 2.0 ** -24])


@pytest.mark.parametrize('shape', [(1, 1, 1, 3), (2, 3, 5, 3), (3, 17, 33, 3), (2, 64, 64, 3), (1, 5, 7, 1)])
def test_frames_u8_is_exact(shape):
	"""(uint8) min(max(255 x, 0), 255) -- numpy's astype truncation -- with and without the 180 degree turn, on the vector path (64 x 64: the
	pixels of an image a multiple of 4) and the pixel-per-thread path (w * c = 15, 99, 7, 3), values on and next to every level planted."""
	from find_amd import functional as FN
	g = torch.Generator().manual_seed(sum(shape))
	x = torch.rand(shape, generator=g)
	every = _planted()
	p = every[torch.randperm(every.numel(), generator=g)][:x.numel()]
	x.view(-1)[torch.randperm(x.numel(), generator=g)[:p.numel()]] = p
	xn = x.numpy()
	with np.errstate(invalid='ignore'):
		ref = np.where(np.isnan(xn), np.float32(0), np.clip(255 * xn, 0, 255)).astype(np.uint8)
	assert (255 * xn).dtype == np.float32
	xd = x.cuda()
	plain, turned = FN.frames_u8(xd, rot180=False), FN.frames_u8(xd, rot180=True)
	assert plain.dtype == torch.uint8 and plain.shape == shape and turned.shape == shape
	assert np.array_equal(plain.cpu().numpy(), ref)
	assert np.array_equal(turned.cpu().numpy(), ref[:, ::-1, ::-1])
	if x.numel() >= every.numel():   # (every level is there, and the values outside [0, 1])
		assert set(np.unique(ref)) == set(range(256))
	# leading dimensions are batch dimensions, and `out` takes a slice of a larger buffer
	buf = torch.zeros((2,) + shape, dtype=torch.uint8, device='cuda')
	FN.frames_u8(xd, rot180=True, out=buf[1])
	assert torch.equal(buf[1], turned) and not buf[0].any()
	assert torch.equal(FN.frames_u8(torch.stack([xd, xd]), rot180=True), torch.stack([turned, turned]))


def test_frames_u8_refusals():
	from find_amd import functional as FN
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.frames_u8(torch.zeros(1, 2, 2, 3))
	with pytest.raises(RuntimeError, match='fp32'):
		FN.frames_u8(torch.zeros(1, 2, 2, 3, dtype=torch.float64, device='cuda'))
	with pytest.raises(ValueError, match='out must be'):
		FN.frames_u8(torch.zeros(1, 2, 2, 3, device='cuda'), out=torch.zeros(1, 2, 2, 3, device='cuda'))


# ---------------------------------------------------------------------------------------------- spins
def _mesh():
	from tests.test_gpu_render import _scene
	from find_amd.structures import Meshes, TexturesVertex
	verts, faces, cols, _, _ = _scene(n_meshes=1)
	return Meshes(verts.cuda(), faces.cuda(), TexturesVertex(cols.cuda())), verts, faces, cols


@pytest.fixture(scope='module')
def spin():
	"""One 9-frame spin at 64^2 with the default chunking, shared by the tests below."""
	from find_amd import vis
	mesh, verts, faces, cols = _mesh()
	frames = vis.turntable(mesh, None, image_size=64, nframes=9, azim=AZIM, dist=DIST, silent=True)
	return mesh, verts, faces, cols, frames


def test_spin_equals_the_oracle_on_rotated_vertices(spin):
	"""Expected: for each theta the oracle's render of verts @ Rz(theta) under the one camera (R0, T0), then (255 x).astype(uint8) and the 180
	degree turn -- upstream's loop.  Bars: 99.9 % of the pixels within one level (tests/test_gpu_render.py's agreement bar for nearest-face
	maps; a truncation may fall either side of a level), none beyond 13 levels (its 5e-2), and the expected frames are not blank."""
	mesh, verts, faces, cols, frames = spin
	n, size = 9, 64
	assert frames.shape == (n, size, size, 3) and frames.dtype == torch.uint8 and frames.is_cuda
	R0, T0 = camera_ref.look_at_view_transform(dist=DIST, elev=0.0, azim=float(AZIM), up=((1, 0, 0),))
	theta = torch.linspace(0, 2 * math.pi, n)
	e = torch.zeros(n, 3)
	e[:, 2] = theta
	Rz = mlp_ref.euler_angles_to_matrix_xyz(e)   # float32, as upstream's Transform3d
	want = []
	for i in range(n):
		img = render_ref.render((verts @ Rz[i]).numpy(), faces.numpy(), cols.numpy(), R0, T0, image_size=size, want_mask=False)['image'][0, 0]
		want.append((255 * img).astype(np.uint8)[::-1, ::-1])
	want = np.stack(want).astype(np.int16)
	got = frames.cpu().numpy().astype(np.int16)
	d = np.abs(got - want).max(-1)
	covered = (want < 255).any(-1).mean()
	print(f'spin vs oracle: {(d <= 1).mean():.5f} of the pixels within one level, worst {d.max()}, covered {covered:.3f}')
	assert covered >= 0.05, covered
	assert (d <= 1).mean() >= 0.999, (d <= 1).mean()
	assert d.max() <= 13, d.max()


def test_spin_does_not_depend_on_the_chunking(spin):
	from find_amd import vis
	mesh, _, _, _, frames = spin
	for per_call in (2, 4, 9):
		again = vis.turntable(mesh, None, image_size=64, nframes=9, azim=AZIM, dist=DIST, silent=True, views_per_call=per_call)
		assert torch.equal(again, frames), per_call


def test_first_and_last_frame_show_the_same_pose(spin):
	frames = spin[-1].cpu().numpy().astype(np.int16)
	assert np.abs(frames[0] - frames[-1]).max() <= 1
	assert np.abs(frames[0] - frames[4]).max() > 13   # (half a turn away it is another picture)


def test_more_than_one_mesh_renders_the_first_with_a_warning(spin):
	from find_amd import vis
	from find_amd.structures import Meshes, TexturesVertex
	mesh, verts, faces, cols, frames = spin
	two = Meshes(torch.cat([verts, verts * 0.5]).cuda(), faces.cuda(), TexturesVertex(torch.cat([cols, cols]).cuda()))
	with pytest.warns(UserWarning, match='only rendering first mesh'):
		got = vis.turntable(two, None, image_size=64, nframes=9, azim=AZIM, dist=DIST, silent=True)
	assert torch.equal(got, frames)


def test_uv_scan_spins_and_files_are_written(tmp_path):
	"""A TexturesUV scan (open, irregular: tests/scan_meshes.py) at 32^2, 3 frames: the frames are frames_u8 of one FootRenderer call with the
	spin's views; .npy holds them, .gif / .png hold as many frames of that size."""
	from PIL import Image
	from tests.scan_meshes import open_irregular_mesh
	from find_amd import functional as FN, vis
	from find_amd.renderer import FootRenderer
	from find_amd.structures import Meshes, TexturesUV
	v, f = open_irregular_mesh(200, seed=2)
	lo, hi = v.amin(0, keepdim=True), v.amax(0, keepdim=True)
	uv = ((v - lo) / (hi - lo))[:, :2].contiguous()
	maps = torch.rand(1, 16, 12, 3, generator=torch.Generator().manual_seed(6)) * 0.8
	mesh = Meshes(v[None].cuda(), f[None].cuda(), TexturesUV(maps.cuda(), f[None].cuda(), uv[None].cuda()))
	npy = str(tmp_path / 'spin.npy')
	frames = vis.turntable(mesh, npy, image_size=32, nframes=3, azim=AZIM, dist=DIST, silent=True)
	rdr = FootRenderer(image_size=32, device='cuda')
	R, T = vis.turntable_views(rdr, nframes=3, azim=AZIM, dist=DIST)
	with torch.no_grad():
		image = rdr(mesh, R, T)['image']
	assert torch.equal(frames, FN.frames_u8(image[0], rot180=True))
	assert ((frames < 255).any(-1).float().mean(dim=(1, 2)) > 0.01).all()   # covered pixels in every frame
	assert np.array_equal(np.load(npy), frames.cpu().numpy())
	for ext in ('gif', 'png'):
		loc = str(tmp_path / f'spin.{ext}')
		again = vis.turntable(mesh, loc, image_size=32, nframes=3, fps=10, azim=AZIM, dist=DIST, silent=True)
		assert torch.equal(again, frames)
		with Image.open(loc) as im:
			assert im.size == (32, 32) and getattr(im, 'n_frames', 1) == 3, ext
			assert im.info.get('duration') == pytest.approx(100), ext
			if ext == 'png':   # (lossless: the first frame comes back as written)
				assert np.array_equal(np.asarray(im.convert('RGB')), frames[0].cpu().numpy())


# ---------------------------------------------------------------------------------------------- heat maps
def test_vertex_errors_vs_float64_brute_force():
	from find_amd import vis
	g = torch.Generator().manual_seed(12)
	scale = torch.tensor([0.12, 0.045, 0.04])
	pred = (torch.rand(2, 254, 3, generator=g) - 0.5) * scale
	gt = (torch.rand(2, 301, 3, generator=g) - 0.5) * scale * 1.05
	samples = (torch.rand(2, 500, 3, generator=g) - 0.5) * scale
	lens = [37, 301]
	gt[0, 37:] = 1e6   # padding: never a target, never a query
	pe, ge = vis.vertex_errors(pred.cuda(), gt.cuda(), samples.cuda(), torch.tensor(lens))
	assert pe.shape == (2, 254) and ge.shape == (2, 301)
	for n, L in enumerate(lens):
		want_p = torch.cdist(pred[n].double(), gt[n, :L].double()).min(1).values ** 2
		want_g = torch.cdist(gt[n, :L].double(), samples[n].double()).min(1).values ** 2
		for got, want in ((pe[n], want_p), (ge[n, :L], want_g)):
			err = (got.cpu().double() - want).abs()
			assert (err <= 1e-6 * want + 1e-12).all(), (n, float((err / want).max()))
		assert not ge[n, L:].any()
	# the heat map: red saturates at 30e-6 (eval_3d.py:180), green and blue stay 0
	err = torch.tensor([0.0, 10e-6, 30e-6, 30.1e-6, 5e-3], device='cuda')
	col = vis.error_colours(err)
	assert col.shape == (5, 3) and not col[:, 1:].any()
	assert col[0, 0] == 0 and 0.33 < col[1, 0] < 0.34 and torch.equal(col[2:, 0], torch.ones(3, device='cuda'))
	assert torch.allclose(vis.error_colours(pe)[..., 0], torch.clamp(pe / 30e-6, 0, 1), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------- eval_3d
def _foot3d_val2(root):
	"""Two validation scans with four keypoints each, in the folder layout of tests/test_host_dataset.py."""
	from tests.test_host_dataset import CFG_POSE, _write_scan
	from find_amd.dataset import Foot3DDataset
	mesh_dir = os.path.join(root, 'Meshes_sliced')
	data, val = [], []
	for k, fid in enumerate(['0031', '0032']):
		rel = f'{fid}/A/{fid}-A'
		n = 7 + 2 * k
		_write_scan(mesh_dir, rel + '.obj', rel + '.png', n, (0.0, 0.0, 0.0))
		data.append({'Foot ID': fid, 'Scan ID': 'A', 'footedness': 'Left', 'pose': ['T-Pose'], 'keypoints': [0, n + 1, 2 * n + 3, n * n - 1],
					 'OBJ file': rel + '.obj', 'PNG file': rel + '.png'})
		val.append(fid)
	jpath = os.path.join(root, 'index.json')
	with open(jpath, 'w') as fh:
		json.dump({'keypoint_labels': ['a', 'b', 'c', 'd'], 'data': data}, fh)
	cfg = {'DATASET_FOLDER': root, 'DATASET_JSON': jpath, 'DATASET_NAME': 'Meshes_sliced', 'LOWPOLY_DATASET_NAME': 'x', 'VAL_FEET': val,
		   'TEMPLATE_FEET': [], 'POSE_VECTOR': CFG_POSE}
	return Foot3DDataset(cfg, device='cpu', is_train=False)


def test_eval_3d_writes_spins_and_meshes_and_keeps_its_numbers(tmp_path):
	from PIL import Image
	from tests.test_gpu_eval2d import _model
	from find_amd import evaluate, vis
	from find_amd.dataset import BatchCollator
	ds = _foot3d_val2(str(tmp_path / 'data'))
	assert len(ds) == 2
	model = _model(2)
	kp_idx = [3, 17, 40, 101]
	out_dir = str(tmp_path / 'out')
	torch.manual_seed(21)
	plain = evaluate.eval_3d(model, ds, kp_idx, samples=2000)
	torch.manual_seed(21)
	res, extra = evaluate.eval_3d(model, ds, kp_idx, samples=2000, produce_spins=True, export_meshes=True, out_dir=out_dir,
								  spin_frames=3, spin_image_size=32)
	assert res == plain and set(res) == {'Keypoint (mm)', 'Chamf z-cutoff 0.07 (μm)', 'Chamf (μm)'}   # exactly: no draw was added
	assert model.training
	spins = sorted(os.listdir(os.path.join(out_dir, 'spins')))
	assert spins == sorted(f'{n:02d}_{k}.gif' for n in range(2) for k in ('pred_rgb', 'pred_chamf', 'pred_grey', 'gt_rgb', 'gt_chamf', 'gt_grey'))
	assert sorted(os.listdir(os.path.join(out_dir, 'meshes'))) == ['00_gt_mesh.obj', '00_pred_mesh.obj', '01_gt_mesh.obj', '01_pred_mesh.obj']
	assert sorted(extra['files']) == sorted([os.path.join(out_dir, 'spins', s) for s in spins]
											+ [os.path.join(out_dir, 'meshes', f'{n:02d}_{k}_mesh.obj') for n in range(2) for k in ('gt', 'pred')])
	for s in spins:
		with Image.open(os.path.join(out_dir, 'spins', s)) as im:
			# (PIL folds a frame that repeats its predecessor into it: a square scan in one colour looks the same after half a turn)
			assert im.size == (32, 32) and (im.n_frames == 3 if '_rgb' in s else 1 <= im.n_frames <= 3), s
	# the meshes: the prediction bit for bit with its colours, the scan's geometry
	collate = BatchCollator(device='cuda').collate_batches
	model.eval()
	with torch.no_grad():
		batch = collate([ds[0], ds[1]])
		batch.update({vec.name: vec.data[batch['idx']] for vec in model.latent_vectors_val})
		want = model.get_meshes_from_batch(batch, is_train=False)
	model.train()
	for n in range(2):
		v, c, f = vis.read_obj_colours(os.path.join(out_dir, 'meshes', f'{n:02d}_pred_mesh.obj'))
		assert torch.equal(v, want['verts'][n].cpu()) and torch.equal(c, want['col'][n, :, :3].cpu())
		assert torch.equal(f, want['meshes'].faces_list()[n].cpu().long())
		v, c, f = vis.read_obj_colours(os.path.join(out_dir, 'meshes', f'{n:02d}_gt_mesh.obj'))
		assert c is None and torch.equal(v, batch['mesh'].verts_list()[n].cpu()) and torch.equal(f, batch['mesh'].faces_list()[n].cpu().long())
	# the per-vertex errors behind the heat maps
	assert extra['pred_vertex_error'].shape == (2, 1002) and (extra['pred_vertex_error'] > 0).any()
	assert [tuple(t.shape) for t in extra['gt_vertex_error']] == [(49,), (81,)]
	want_p = torch.stack([torch.cdist(want['verts'][n].double(), batch['mesh'].verts_list()[n].double()).min(1).values ** 2 for n in range(2)])
	assert torch.allclose(extra['pred_vertex_error'].double(), want_p, rtol=1e-5, atol=1e-12)
	with pytest.raises(ValueError, match='out_dir'):
		evaluate.eval_3d(model, ds, kp_idx, samples=500, export_meshes=True)


# ---------------------------------------------------------------------------------------------- Trainer.export_meshes
def test_trainer_export_meshes(tmp_path):
	from tests.test_gpu_train3d import _setup
	from tests.test_gpu_trainloop import _fill_val_tables, _val_batch
	from find_amd import vis
	from find_amd.trainer import Trainer
	mwl, opts, batch_of, (gv, gf, gc), opt = _setup(1002, 1002)
	m = mwl.model
	_fill_val_tables(m)
	val_loader = [_val_batch(gv, gf, gc, 0, '9000-A'), _val_batch(gv, gf, gc, 1, '9000-B')]
	tr = Trainer([opt], mwl, [batch_of(0), batch_of(3)], val_loader, opts, latent_vectors_train=m.latent_vectors_train,
				 latent_vectors_val=m.latent_vectors_val, val_optim=opt, device='cuda')
	before = {k: p.detach().clone() for k, p in mwl.named_parameters()}
	mode = mwl.training
	for is_train, loader, names in ((False, val_loader, ['9000-A', '9000-B']), (True, tr.train_loader, None)):
		loc = str(tmp_path / ('train' if is_train else 'val') / 'meshes')
		files = tr.export_meshes(loc, is_train=is_train, export_gt=not is_train)
		names = names or [b['name'][0] for b in loader]
		assert sorted(os.listdir(loc)) == sorted(f'{n}.obj' for n in names)
		assert len(files) == len(names) * (1 if is_train else 2)
		for b in loader:
			b = dict(b)
			b.update(**tr.sample_latent_vectors(b, latent_vectors=m.latent_vectors_train if is_train else m.latent_vectors_val))
			with torch.no_grad():
				want = m.get_meshes_from_batch(b, is_train=is_train)
			v, c, f = vis.read_obj_colours(os.path.join(loc, b['name'][0] + '.obj'))
			assert torch.equal(v, want['verts'][0].cpu()) and torch.equal(c, want['col'][0, :, :3].cpu())
			assert torch.equal(f, want['meshes'].faces_list()[0].cpu().long())
			if not is_train:   # export_gt: the scan's geometry beside it, under meshes_gt
				gt_loc = os.path.join(loc.replace('meshes', 'meshes_gt'), b['name'][0] + '.obj')   # (str.replace, as upstream: every 'meshes' of the path)
				v, c, f = vis.read_obj_colours(gt_loc)
				assert c is None and torch.equal(v, b['mesh'].verts_list()[0].cpu()) and torch.equal(f, b['mesh'].faces_list()[0].cpu().long())
	assert mwl.training == mode
	for k, p in mwl.named_parameters():
		assert torch.equal(p, before[k]) and p.grad is None, k
	with pytest.raises(NotImplementedError):
		tr.plot(str(tmp_path / 'plot.png'))
