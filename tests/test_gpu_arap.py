"""The as-rigid-as-possible energy on the MI355X: find_arap_fwd / find_arap_bwd through FN.arap_energy against the float64 restatement of the
definition (tests/arap_ref.py) on the same fp32 inputs, and the term's place in ModelWithLoss and Trainer.

Margins: none is a constant of the code under test.  Every float comparison follows tests/test_gpu_measure.py's _held: the same restatement is
also evaluated in float32 on the CPU; with e32 its worst error against float64 over the case's tensor, the HIP result must lie within
max(4 e32, 2 ulp of the largest value) of the float64 one.  Each case prints its figures (DESIGN 7.13 records the worst).

Shapes, the smallest that cross each boundary: a tetrahedron (V = 4, valence 3); lat-long ellipsoids (rings, segs) -> V = rings segs + 2:
(4, 16) V = 66, just past a wave, poles of valence 16; (8, 32) V = 258, past 256; (2, 130) V = 262, poles of valence 130 (more than a wave of
neighbours); (25, 40) V = 1002; one case at (16, 6890), the (84, 82) grid.  The kernels give a workgroup 4 meshes and 64 vertices (forward: 4 lanes
each) or 32 (backward: 8 lanes each): (1, 29), (2, 15), (1, 31) -> V = 31, 32, 33 and (1, 61), (2, 31), (3, 21) -> V = 63, 64, 65 sit on each
side of the two vertex tiles (their pole valences 15 ... 61 on each side of multiples of both lane strides as well), N = 3, 4, 5 on each side of the
mesh tile, beside N = 1 and 17.  Every case runs twice and must repeat bit for bit.

A condition on the inputs, asserted before anything is compared: the restatement reports min_i (D_2 - D_3) / D_1 >= 1e-3 for the mirrored
deformation and min_i (D_2 + D_3) / D_1 >= 1e-3 for the others -- every cell has a well-defined rotation (the degenerate cases apart, which
are exactly degenerate)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import arap_ref as ref   # noqa: E402
import poison   # noqa: E402

WORST = {}   # name of a quantity -> the worst e_hip / max(e32, ulp) seen (printed by the last test of the file)
_MESHES, _RESTS, _REFS = {}, {}, {}


def _ulp(x):
	return float(np.spacing(np.float32(abs(float(x)))))


def _held(name, hip, ref64, ref32, kind=None):
	hip, ref64, ref32 = hip.detach().double().cpu(), ref64.detach().double(), ref32.detach().double()
	assert hip.shape == ref64.shape, (name, hip.shape, ref64.shape)
	e_hip = (hip - ref64).abs().max().item()
	e32 = (ref32 - ref64).abs().max().item()
	ulp = _ulp(ref64.abs().max().item())
	ratio = e_hip / max(e32, ulp)
	print(f'{name}: e_hip {e_hip:.3e}  e32 {e32:.3e}  ulp {ulp:.3e}  scale {ref64.abs().max().item():.3e}  e_hip / max(e32, ulp) {ratio:.2f}')
	if kind:
		WORST[kind] = max(WORST.get(kind, 0.), ratio)
	assert np.isfinite(e_hip) and e_hip <= max(4 * e32, 2 * ulp), (name, e_hip, e32, ulp)


# ------------------------------------------------------------------ inputs, the reference (computed once per case), the HIP run
def _mesh(key):
	"""key: 'tet', (rings, segs), or ('open', rings, segs): the ellipsoid without the faces at its first pole -- vertex 0 is unreferenced."""
	if key not in _MESHES:
		from find_amd import synthetic
		if key == 'tet':
			q = torch.tensor([[0.03, 0.03, 0.03], [0.03, -0.03, -0.03], [-0.03, 0.03, -0.03], [-0.03, -0.03, 0.03]])
			f = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
		elif key[0] == 'open':
			q, f = synthetic.ellipsoid_mesh(*key[1:])
			f = f[~(f == 0).any(1)].contiguous()
		else:
			q, f = synthetic.ellipsoid_mesh(*key)
		_MESHES[key] = (q, f)
	return _MESHES[key]


def _rests(key, weights):
	"""(the restatement's rest mesh, the package's) for a mesh and a weight mode, built once."""
	if (key, weights) not in _RESTS:
		from find_amd import functional as FN
		q, f = _mesh(key)
		_RESTS[key, weights] = (ref.Rest(q, f, weights), FN.ArapRest(q.cuda(), f.cuda(), weights))
	return _RESTS[key, weights]


def _reference(key, weights, kind, N, seed=0):
	"""The case's inputs and the restatement in float64 and float32, computed once and shared."""
	k = (key, weights, kind, N, seed)
	if k not in _REFS:
		rest = _rests(key, weights)[0]
		p = ref.deform(_mesh(key)[0], kind, N, seed=seed)
		g = torch.randn(N, generator=torch.Generator().manual_seed(100 + seed))
		out = {}
		for tag, dt in (('64', torch.float64), ('32', torch.float32)):
			r = ref.energy(p, rest, dt)
			r['grad'] = ref.gradient(p, rest, g, dt, R=r['R'])
			out[tag] = r
		_REFS[k] = (p, g, out['64'], out['32'])
	return _REFS[k]


def _hip(rest, p, g):
	from find_amd import functional as FN
	pc = p.cuda().requires_grad_(True)
	E, cell, (R, deg) = FN.arap_energy(pc, rest, return_per_vertex=True, return_rotations=True)
	assert E.requires_grad and not cell.requires_grad and not R.requires_grad and R.dtype == torch.float32 and deg.dtype == torch.int32
	(d,) = torch.autograd.grad(E, pc, g.cuda())
	torch.cuda.synchronize()
	return dict(E=E.detach(), cell=cell, R=R, degenerate=deg, grad=d)


def _check(key, weights, kind, N, seed=0, well_posed=True):
	tag = f'{key} {weights} {kind} N={N}'
	p, g, r64, r32 = _reference(key, weights, kind, N, seed)
	if well_posed:   # a condition on the inputs, not a measurement
		margin = ref.margins(r64['D'], kind == 'mirror')
		print(f'{tag}: worst cell margin {margin:.4f}')
		assert margin >= 1e-3, (tag, margin)
		assert int(r64['degenerate'].sum()) == 0
	rest = _rests(key, weights)[1]
	a, b = _hip(rest, p, g), _hip(rest, p, g)
	for k in a:
		assert torch.equal(a[k], b[k]), (tag, k, 'two runs differ')
		assert torch.isfinite(a[k].float()).all(), (tag, k)
	assert a['degenerate'].cpu().tolist() == r64['degenerate'].tolist(), (tag, a['degenerate'].tolist(), r64['degenerate'].tolist())
	_held(f'{tag} E', a['E'], r64['E'], r32['E'], 'E')
	_held(f'{tag} cell', a['cell'], r64['cell'], r32['cell'], 'cell')
	_held(f'{tag} R', a['R'], r64['R'], r32['R'], 'R')
	_held(f'{tag} grad', a['grad'], r64['grad'], r32['grad'], 'grad')
	# the cell energies are the energy's addends
	assert abs(a['cell'].double().sum(1) - a['E'].double()).max().item() <= 1e-5 * max(a['E'].abs().max().item(), 1e-30) + 1e-30
	return a


# ------------------------------------------------------------------ the cases
KINDS = ('identity', 'bend', 'noise', 'mirror', 'scale')


@pytest.mark.parametrize('key', ['tet', (1, 29), (2, 15), (1, 31), (1, 61), (2, 31), (3, 21), (4, 16), (8, 32), (2, 130), (25, 40)], ids=str)
def test_shapes(key):
	_check(key, 'cotangent', 'bend', 3)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('key', [(4, 16), (25, 40)], ids=str)
def test_deformations(key, kind):
	a = _check(key, 'cotangent', kind, 3, seed=2)
	if kind == 'identity':   # p bitwise q: nothing to pay, no gradient (what is left is rounding in double)
		assert a['E'].abs().max().item() <= 1e-20 and a['grad'].abs().max().item() <= 1e-12


@pytest.mark.parametrize('kind', ['mirror', 'noise'])
@pytest.mark.parametrize('key', [(8, 32), (2, 130)], ids=str)
def test_mirror_and_noise_past_a_block_and_at_high_valence(key, kind):
	_check(key, 'cotangent', kind, 3, seed=3)


@pytest.mark.parametrize('N', [1, 4, 5, 17])
def test_batch_sizes(N):
	_check((8, 32), 'cotangent', 'bend', N, seed=4)


@pytest.mark.parametrize('key', ['tet', (4, 16), (2, 130)], ids=str)
def test_uniform_weights(key):
	_check(key, 'uniform', 'bend', 3, seed=5)
	_check(key, 'uniform', 'mirror', 3, seed=5)


def test_training_size():
	_check((84, 82), 'cotangent', 'bend', 16, seed=6)


@pytest.mark.parametrize('kind', ['collapsed', 'line', 'bend'])
def test_degenerate_cells(kind):
	"""Valid inputs with defined results: a mesh collapsed to a point and one projected onto the x axis (every cell exactly rank 0 / rank 1:
	R = I everywhere, all V cells counted), and an open mesh whose vertex 0 no face references (one cell counted, energy and gradient 0 there)."""
	key = ('open', 4, 16)
	a = _check(key, 'cotangent', kind, 3, seed=7, well_posed=False)
	V = _mesh(key)[0].shape[0]
	assert a['degenerate'].cpu().tolist() == [1 if kind == 'bend' else V] * 3
	assert a['grad'][:, 0].abs().max().item() == 0 and a['cell'][:, 0].abs().max().item() == 0
	assert torch.equal(a['R'][:, 0], torch.eye(3, device='cuda').expand(3, 3, 3))
	if kind != 'bend':
		assert torch.equal(a['R'], torch.eye(3, device='cuda').expand(3, V, 3, 3))
	# the closed mesh, collapsed: the same, without the isolated vertex
	if kind == 'collapsed':
		c = _check((4, 16), 'uniform', 'collapsed', 2, seed=7, well_posed=False)
		assert c['degenerate'].cpu().tolist() == [66, 66] and c['E'].min().item() > 0


def test_a_mesh_does_not_depend_on_its_batch():
	key = (8, 32)
	p, g, _, _ = _reference(key, 'cotangent', 'bend', 17, seed=4)
	rest = _rests(key, 'cotangent')[1]
	batch = _hip(rest, p, g)
	for n in (0, 16):   # the first slot of a tile, and a tile's only mesh
		alone = _hip(rest, p[n:n + 1], g[n:n + 1])
		for k in batch:
			assert torch.equal(batch[k][n:n + 1], alone[k]), (n, k)


@pytest.mark.parametrize('key,N', [((2, 130), 5), ((25, 40), 3)], ids=str)
def test_poisoned_allocations(key, N):
	"""Workspace, rotations, outputs and the gradient are torch.empty: whatever they hold before the call, the results are the same bits.
	The workspace comes from functional._ws, which tests/poison.py covers; the op's own module, find_amd.arap, is given the harness's proxy for
	its module-level `torch` here, the way the harness does it for its four modules."""
	from find_amd import arap as arap_module
	p, g, _, _ = _reference(key, 'cotangent', 'bend', N, seed=8)
	rest = _rests(key, 'cotangent')[1]
	clean = _hip(rest, p, g)
	runs = []
	for byte in poison.PATTERNS:
		with poison.poisoned(byte) as proxy:
			assert arap_module.torch is torch
			arap_module.torch = proxy
			try:
				runs.append(_hip(rest, p, g))
			finally:
				arap_module.torch = torch
		assert proxy.calls == 6, proxy.calls   # workspace, R, cell, energy, degenerate, gradient
	bad = poison.compare(f'arap {key}', clean, runs[0], runs[1])
	assert not bad, '\n'.join(bad)


def test_wrapper_checks():
	from find_amd import functional as FN
	from find_amd.losses import ARAPLoss
	q, f = _mesh((4, 16))
	rest = _rests((4, 16), 'cotangent')[1]
	with pytest.raises(RuntimeError, match='66 vertices'):
		FN.arap_energy(torch.zeros(2, 65, 3, device='cuda'), rest)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.arap_energy(torch.zeros(2, 66, 3), rest)
	# the rest mesh is built once per tensor objects
	qc, fc = q.cuda(), f.cuda()
	assert FN.ArapRest.get(qc, fc) is FN.ArapRest.get(qc, fc) and FN.ArapRest.get(qc, fc, 'uniform') is not FN.ArapRest.get(qc, fc)
	assert FN.ArapRest.get(qc, fc).nbr_w.dtype == torch.float32 and FN.ArapRest.get(qc, fc).nbr_w.shape == FN.ArapRest.get(qc, fc).topo.nbr_idx.shape
	# plain call: E alone; the loss: its mean
	p = ref.deform(q, 'bend', 3).cuda()
	E = FN.arap_energy(p, rest)
	assert torch.is_tensor(E) and E.shape == (3,)
	assert torch.equal(ARAPLoss(qc, fc)(p), E.mean())
	E2, cell = FN.arap_energy(p, rest, return_per_vertex=True)
	assert torch.equal(E, E2) and cell.shape == (3, 66)


# ------------------------------------------------------------------ the term in a training step
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


def test_model_with_loss_reports_the_arap_term_last(step):
	from find_amd.losses import ARAPLoss
	from find_amd.opts import Opts
	mwl, opts, batch, opt = step
	m = mwl.model
	b = _sampled(mwl, batch)
	torch.manual_seed(3)
	loss, losses = mwl(b, 0, opts, arap=True, chamf=True, smooth=True)
	assert list(losses) == ['loss_chamf', 'loss_smooth', 'loss_arap']
	# the raw term: template + offsets (before the registration) against the template
	with torch.no_grad():
		verts = m.template_verts.data + m.get_meshes_from_batch(b, is_train=True)['offsets']
		raw = ARAPLoss(m.template_verts, m.template_faces)(verts).item()
	got = losses['loss_arap'].item()
	print('loss_arap', got, 'raw', raw)
	assert raw > 0 and abs(got - opts.weight_arap * raw) <= 1e-6 * got
	# ... which is the restatement's value on those vertices
	rest = ref.Rest(m.template_verts.data[0].cpu(), m.template_faces.data[0].cpu())
	r64, r32 = (ref.energy(verts.cpu(), rest, dt)['E'].mean() for dt in (torch.float64, torch.float32))
	_held('loss_arap raw', torch.tensor(raw), r64, r32, 'E')
	_, twice = mwl(b, 0, Opts(chamf_loss=True, weight_arap=2e4), arap=True)
	assert list(twice) == ['loss_arap'] and abs(twice['loss_arap'].item() - 2 * got) <= 1e-6 * got
	_, uniform = mwl(b, 0, Opts(chamf_loss=True, arap_weights='uniform'), arap=True)
	assert uniform['loss_arap'].item() > 0 and uniform['loss_arap'].item() != got
	# the gradient reaches the network and the shape codes, not the registration
	mwl.zero_grad()
	losses['loss_arap'].backward()
	torch.cuda.synchronize()
	named = dict(m.named_parameters())
	gs = named['shapevec.data'].grad
	assert gs is not None and torch.isfinite(gs).all() and gs.abs().max().item() > 0
	head = [p.grad for k, p in named.items() if k.startswith('mlp_disp') and p.grad is not None]
	assert head and all(torch.isfinite(t).all() for t in head) and any(t.abs().max().item() > 0 for t in head)
	assert named['reg.data'].grad is None or named['reg.data'].grad.abs().max().item() == 0
	mwl.zero_grad()
	# flag off: the other terms' values, bit for bit -- beside the term and in a call that never mentions it
	torch.manual_seed(3)
	la, a = mwl(b, 0, opts, chamf=True, smooth=True)
	torch.manual_seed(3)
	lb, c = mwl(b, 0, opts, chamf=True, smooth=True, arap=False)
	assert list(a) == list(c) == ['loss_chamf', 'loss_smooth'] and torch.equal(la, lb)
	for k in a:
		assert torch.equal(a[k], c[k]) and torch.equal(a[k], losses[k]), k


def test_arap_term_on_the_pca_model(tmp_path):
	from test_gpu_pca import _fixture_mwl
	from find_amd.structures import Meshes, TexturesVertex
	from find_amd.train_utils import sample_latent_vectors
	z = np.load(os.path.join(HERE, 'golden', 'pca.npz'))
	mwl, opts = _fixture_mwl(z, tmp_path)
	gv, gf = (torch.from_numpy(z[f'gt/{k}']).cuda() for k in ('verts', 'faces'))
	idx = [0, 2]
	b = dict(mesh=Meshes(gv[idx].contiguous(), gf, TexturesVertex(torch.full_like(gv[idx], 0.5))), idx=torch.tensor(idx, device='cuda'))
	b.update(sample_latent_vectors(b, mwl.model.latent_vectors_train))
	loss, losses = mwl(b, 0, opts, arap=True)
	assert list(losses) == ['loss_arap'] and torch.isfinite(losses['loss_arap']).item() and losses['loss_arap'].item() > 0
	losses['loss_arap'].backward()
	named = dict(mwl.model.named_parameters())
	gs = named['shapevec.data'].grad
	assert gs is not None and torch.isfinite(gs).all() and gs.abs().max().item() > 0
	assert named['reg.data'].grad is None or named['reg.data'].grad.abs().max().item() == 0


def test_skinned_model_has_no_offsets(tmp_path):
	from find_amd import synthetic
	from find_amd.model_with_loss import ModelWithLoss
	from find_amd.opts import Opts
	np.savez(str(tmp_path / 'm.npz'), **synthetic.skinned_model(V=1002, J=5, B=10, chain='tree', seed=1))
	opts = Opts(model_type='skinned', load_model=str(tmp_path / 'm.npz'))
	mwl = ModelWithLoss(opts=opts, device='cuda', train_size=3, val_size=2)
	with pytest.raises(NotImplementedError, match='offsets'):
		mwl({}, 0, opts, arap=True)


def test_trainer_runs_the_term_eagerly(step):
	from find_amd.trainer import Trainer
	mwl, opts, batch, opt = step
	kw = dict(chamf=True, arap=True)
	tr = Trainer([opt], mwl, [batch, batch], [], opts, latent_vectors_train=mwl.model.latent_vectors_train, device='cuda', graph='auto')
	assert 'arap' in tr._why_not_graph(tr.optims, kw)
	msg = tr.train_epoch(0, model_kwargs=dict(kw))
	assert tr.last_mode == 'eager', msg
	vals = tr.log[0]['train_loss']['Arap']
	assert len(vals) == 2 and all(np.isfinite(vals)) and all(np.isfinite(tr.log[0]['train_loss']['Chamf']))
	tr.graph = True
	with pytest.raises(RuntimeError, match='arap'):
		tr.train_epoch(1, model_kwargs=dict(kw))


def test_zz_worst_ratios():
	"""Prints the worst e_hip / max(e32, ulp) per quantity over the file's cases."""
	for k, v in sorted(WORST.items()):
		print(f'worst {k}: {v:.3f}')
	assert all(v <= 4. for v in WORST.values())
