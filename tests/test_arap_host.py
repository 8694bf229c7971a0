"""The as-rigid-as-possible energy on the host: the float64 restatement (tests/arap_ref.py) against autograd through the SVD and against
closed forms, the cotangent weights of functional.arap_cotangent_weights against a face-by-face evaluation, the host build of the per-cell
arithmetic, the C interface, the term's place in the registry and what the wrappers say before any kernel runs."""
import inspect
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import arap_ref as ref   # noqa: E402

SYMBOLS = ('find_arap_fwd', 'find_arap_bwd')
GRIDS = ((4, 16), (8, 32), (25, 40))   # V = 66, 258, 1002


def _mesh(rings, segs):
	from find_amd import synthetic
	return synthetic.ellipsoid_mesh(rings, segs)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('kind', ['bend', 'noise', 'mirror'])
def test_fixed_rotation_gradient_is_the_full_gradient(grid, kind):
	"""R_i minimises its cell's energy, so the term through dR vanishes: the gather formula equals float64 autograd through torch.linalg.svd."""
	q, f = _mesh(*grid)
	rest = ref.Rest(q, f)
	p = ref.deform(q, kind, 2, seed=1).double().requires_grad_(True)
	g = torch.tensor([0.7, -1.3], dtype=torch.float64)
	out = ref.energy(p, rest)
	assert ref.margins(out['D'], kind == 'mirror') >= 1e-3
	(auto,) = torch.autograd.grad((out['E'] * g).sum(), p)
	fixed = ref.gradient(p.detach(), rest, g)
	err = (auto - fixed).abs().max().item()
	print(f'V {rest.V} {kind}: |autograd - fixed| {err:.3e}, scale {fixed.abs().max().item():.3e}')
	assert err <= 1e-12 * fixed.abs().max().item()


@pytest.mark.parametrize('grid', GRIDS)
@pytest.mark.parametrize('weights', ['cotangent', 'uniform'])
def test_closed_forms(grid, weights):
	q, f = _mesh(*grid)
	rest = ref.Rest(q, f, weights)
	qd = rest.q.double()
	eq = qd[rest.ei] - qd[rest.ej]
	spread = float((rest.w.double() * (eq * eq).sum(-1)).sum() / rest.W)   # sum w |q_i - q_j|^2 / W
	# a global rotation and translation: nothing to pay, no gradient
	R = torch.from_numpy(ref.rotation_matrix([0.3, -1., 0.5], 2.2))
	p = (qd @ R.T + torch.tensor([0.1, -0.2, 0.05], dtype=torch.float64))[None]
	out = ref.energy(p, rest)
	assert out['E'].item() <= 1e-25 * spread / 1e-6 and int(out['degenerate']) == 0
	assert (out['R'][0] - R).abs().max().item() <= 1e-9
	assert ref.gradient(p, rest, torch.ones(1)).abs().max().item() <= 1e-12 * spread ** 0.5
	# a uniform scale: every fitted rotation is the identity, what is left is (s - 1)^2 sum w |e_q|^2 / W
	for s in (0.9, 1.25):
		out = ref.energy(qd[None] * s, rest)
		assert abs(out['E'].item() - (s - 1) ** 2 * spread) <= 1e-12 * spread
	# the mirror image pays: no rotation maps the mesh onto it
	assert ref.energy(qd[None] * torch.tensor([1., 1., -1.], dtype=torch.float64), rest)['E'].item() > 1e-3 * spread


def test_degenerate_cells_of_the_restatement():
	q, f = _mesh(4, 16)
	keep = ~(f == 0).any(1)                     # without the faces at the first pole: vertex 0 has no neighbours, its ring is a boundary
	rest = ref.Rest(q, f[keep])
	assert not (rest.ei == 0).any()
	for kind, count in (('collapsed', rest.V), ('line', rest.V), ('bend', 1)):
		out = ref.energy(ref.deform(q, kind, 2), rest)
		assert out['degenerate'].tolist() == [count, count], kind
		assert torch.isfinite(out['E']).all() and torch.isfinite(out['R']).all()
		assert out['cell'][:, 0].abs().max() == 0 and ref.gradient(ref.deform(q, kind, 2), rest, torch.ones(2))[:, 0].abs().max() == 0
	assert ref.energy(ref.deform(q, 'collapsed', 1), rest)['R'][0].equal(torch.eye(3, dtype=torch.float64).expand(rest.V, 3, 3))


# ------------------------------------------------------------------ the weights of the package
@pytest.mark.parametrize('grid', GRIDS)
def test_cotangent_weights(grid):
	from find_amd import functional as FN
	q, f = _mesh(*grid)
	keep = ~(f == 0).any(1)                     # an open mesh: the first ring's edges have ONE face each
	f = f[keep]
	topo = FN.MeshTopology(f, q.shape[0])
	off, idx = topo.nbr_off.numpy(), topo.nbr_idx.numpy()
	w = FN.arap_cotangent_weights(q.numpy(), f.numpy(), off, idx)
	raw = ref.cotangent_by_face(q.numpy(), f.numpy())
	rows = np.repeat(np.arange(q.shape[0]), np.diff(off))
	direct = np.array([raw[(int(i), int(j))] for i, j in zip(rows, idx)])
	assert w.dtype == np.float64 and w.shape == idx.shape
	assert np.abs(w - np.maximum(direct, 0.)).max() <= 1e-13 * np.abs(direct).max()
	# the clamp acts, and leaves every vertex that has neighbours a weight sum well above zero
	negative = direct < 0
	assert 0.1 < negative.mean() < 0.3 and (w[negative] == 0).all() and (w >= 0).all()
	sums = np.bincount(rows, weights=w, minlength=q.shape[0])
	assert sums[0] == 0 and sums[1:].min() >= 1.
	# symmetric
	lookup = {(int(i), int(j)): x for i, j, x in zip(rows, idx, w)}
	assert all(lookup[(j, i)] == x for (i, j), x in lookup.items())
	# a boundary edge (ring 0: vertices 1, 2) has one face: one cotangent, the angle at the ring-1 vertex opposite
	segs = grid[1]
	tri = [t for t in f.tolist() if 1 in t and 2 in t]
	assert len(tri) == 1
	o = [v for v in tri[0] if v not in (1, 2)][0]
	qd = q.double().numpy()
	u, v = qd[1] - qd[o], qd[2] - qd[o]
	assert abs(raw[(1, 2)] - 0.5 * (u @ v) / np.linalg.norm(np.cross(u, v))) <= 1e-12 * abs(raw[(1, 2)]) and segs >= 3
	# a face without area contributes nothing
	flat = FN.arap_cotangent_weights(np.array([[0., 0, 0], [1, 0, 0], [2, 0, 0]]), np.array([[0, 1, 2]]), np.array([0, 2, 4, 6]), np.array([1, 2, 0, 2, 0, 1]))
	assert (flat == 0).all()


# ------------------------------------------------------------------ the host build of the per-cell arithmetic
def test_host_build_of_the_cell_arithmetic():
	"""csrc/arap_math.h -- the sums S, the fitted rotation with its reflection and degeneracy rules, the cell energy: the functions arap.hip
	compiles for the device -- built for the host and run by tools/arap_host_check.cpp."""
	cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
	assert cxx is not None, 'no host C++ compiler'
	with tempfile.TemporaryDirectory() as tmp:
		exe = os.path.join(tmp, 'arap_host_check')
		subprocess.run([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'find_amd', 'csrc'), os.path.join(ROOT, 'tools', 'arap_host_check.cpp'), '-o', exe],
					   check=True, capture_output=True)
		r = subprocess.run([exe], capture_output=True, text=True)
	assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]


# ------------------------------------------------------------------ interface
def test_header_bindings_and_library_agree():
	from find_amd import _lib
	hdr = open(os.path.join(ROOT, 'include', 'find_hip.h')).read()
	assert '#define FIND_ABI_VERSION 3' in hdr and _lib.ABI_VERSION == 3 and _lib.lib().find_abi_version() == 3
	for name, n_args in zip(SYMBOLS, (16, 13)):
		decl = re.search(r'\bint ' + name + r'\(([^;]*)\);', hdr).group(1)
		assert len(decl.split(',')) == n_args == len(_lib.PROTOTYPES[name][1]), name
		assert hasattr(_lib.lib(), name)
	assert re.search(r'\bint64_t find_arap_ws_bytes\(int64_t n, int64_t v\);', hdr) and len(_lib.PROTOTYPES['find_arap_ws_bytes'][1]) == 2
	assert os.path.exists(os.path.join(ROOT, 'find_amd', 'csrc', 'arap.hip')) and os.path.exists(os.path.join(ROOT, 'find_amd', 'csrc', 'arap_math.h'))


def test_ws_bytes_and_refusals():
	from find_amd import _lib
	L = _lib.lib()
	# a double and an int32 per forward workgroup (64 vertices) and mesh, each array rounded up to 256 bytes
	assert L.find_arap_ws_bytes(1, 4) == 512 and L.find_arap_ws_bytes(16, 6890) == 16 * 108 * 8 + 16 * 108 * 4
	for bad in ((0, 10), (1, 0), (65536, 10), (1, 1 << 24), (60000, 60000)):
		L.find_image_mse_ws_bytes()
		assert L.find_arap_ws_bytes(*bad) == -1 and b'bad sizes' in L.find_last_error() and b'find_arap_ws_bytes' in L.find_last_error(), bad
	one = torch.zeros(64)
	p = one.data_ptr()   # (host memory: nothing may touch it)
	assert L.find_arap_fwd(None, p, p, p, p, 1, 4, 6, 1., p, p, p, p, p, 1 << 20, None) != 0 and b'NULL' in L.find_last_error()
	assert L.find_arap_fwd(p, p, p, p, p, 0, 4, 6, 1., p, p, p, p, p, 1 << 20, None) != 0 and b'bad sizes' in L.find_last_error()
	assert L.find_arap_fwd(p, p, p, p, p, 1, 4, -1, 1., p, p, p, p, p, 1 << 20, None) != 0 and b'bad sizes' in L.find_last_error()
	assert L.find_arap_fwd(p, p, p, p, p, 1, 4, 6, -1., p, p, p, p, p, 1 << 20, None) != 0 and b'weight sum' in L.find_last_error()
	assert L.find_arap_fwd(p, p, p, p, p, 1, 4, 6, float('nan'), p, p, p, p, p, 1 << 20, None) != 0 and b'weight sum' in L.find_last_error()
	assert L.find_arap_fwd(p, p, p, p, p, 1, 4, 6, 1., p, p, p, p, p, 8, None) != 0 and b'workspace' in L.find_last_error()
	assert L.find_arap_bwd(p, p, p, p, p, 1, 4, 6, 1., None, p, p, None) != 0 and b'find_arap_bwd' in L.find_last_error()
	assert L.find_arap_bwd(p, p, p, p, p, 1, 1 << 24, 6, 1., p, p, p, None) != 0 and b'bad sizes' in L.find_last_error()


# ------------------------------------------------------------------ the term's place
def test_registry_and_options():
	from find_amd import model_with_loss as M
	from find_amd.opts import Opts
	term = M.Term('arap', 'loss_arap', 'weight_arap', True, False, '_raw_arap')
	assert M.EXTENSION_TERMS_ARAP == (term,)
	# the tuples before it are what they were; one new name for everything after ALL_TERMS, the new term last
	assert M.EVERY_EXTENSION_TERM == M.ALL_EXTENSION_TERMS + M.EXTENSION_TERMS_DEPTH
	assert [t.flag for t in M.EVERY_EXTENSION_TERM] == ['normal', 'p2s', 'depth'] and not any(t.flag == 'arap' for t in M.ALL_TERMS + M.EVERY_EXTENSION_TERM)
	after = [getattr(M, n) for n in dir(M) if isinstance(getattr(M, n), tuple) and getattr(M, n) == M.EVERY_EXTENSION_TERM + M.EXTENSION_TERMS_ARAP]
	assert len(after) == 1 and after[0][-1] == term
	src = inspect.getsource(M.ModelWithLoss.forward)
	assert 'EVERY_EXTENSION_TERM' not in src
	sig = inspect.signature(M.ModelWithLoss.forward).parameters
	assert sig['arap'].default is False and callable(M.ModelWithLoss._raw_arap)
	assert M.EXTENSION_WEIGHTS['weight_arap'] == 10000.
	o = Opts()
	assert (o.arap_loss, o.weight_arap, o.arap_weights) == (False, 10000., 'cotangent') and o.weight_arap == o.weight_chamf == o.weight_p2s
	assert len(o.net_train_kwargs()) == 10 and 'arap' not in o.net_train_kwargs()
	Opts(arap_loss=True, weight_arap=1., arap_weights='uniform')


def test_trainer_runs_an_arap_step_eagerly():
	from find_amd.opts import Opts
	from find_amd.trainer import Trainer
	t = Trainer.__new__(Trainer)
	t.graph, t.opts, t.device = 'auto', Opts(), 'cuda'
	why = t._why_not_graph([], dict(chamf=True, arap=True))
	assert why is not None and 'arap' in why and 'capture' in why
	assert 'arap' not in (t._why_not_graph([], dict(chamf=True)) or '')


# ------------------------------------------------------------------ the wrappers before any launch
def test_cpu_tensors_raise():
	from find_amd import functional as FN
	from find_amd.losses import ARAPLoss
	q, f = _mesh(4, 16)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.ArapRest(q, f)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		ARAPLoss(q, f)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		FN.arap_energy(q[None], rest=None)
	with pytest.raises(ValueError, match='cotangent'):
		FN.ArapRest(q, f, weights='mean-value')
	assert FN.ARAP_WEIGHTS == ('cotangent', 'uniform')
	assert list(inspect.signature(FN.arap_energy).parameters) == ['verts', 'rest', 'return_per_vertex', 'return_rotations']
