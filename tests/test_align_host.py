"""Alignment on the host: the numpy restatement (tests/align_ref.py) against known transforms, the registration rows against the oracle's
Euler matrices, the C interface, the host build of the solve's arithmetic, and what the wrappers say before any kernel runs."""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import align_ref as ref   # noqa: E402

SYMBOLS = ('find_align_fit', 'find_icp_run')
BOX = np.array([0.25, 0.10, 0.08])   # a foot's proportions


def _cloud(P, seed):
	return (np.random.default_rng(seed).random((P, 3)) * BOX).astype(np.float32)


# ------------------------------------------------------------------ the reference against known transforms
@pytest.mark.parametrize('scale,mirror', [(False, False), (True, False), (True, True)])
def test_reference_fit_recovers_a_known_transform(scale, mirror):
	rng = np.random.default_rng(3)
	x = _cloud(50, 1).astype(np.float64)
	R0 = ref.rotation(rng.normal(size=3), 2.5)
	if mirror:
		R0 = R0 * np.array([-1., 1., 1.])[:, None]
	s0, t0 = (1.3 if scale else 1.), np.array([0.02, -0.01, 0.015])
	y = ref.apply(x, R0, t0, s0)
	w = rng.random(50) + 0.5
	w[::7] = 0
	R, t, s, status = ref.umeyama(x, y, w, estimate_scale=scale, allow_reflection=mirror)
	assert status == 0 and np.abs(R - R0).max() < 1e-12 and np.abs(t - t0).max() < 1e-13 and abs(s - s0) < 1e-12
	if mirror:   # the mirror image without allow_reflection: still a proper rotation
		R, _, _, status = ref.umeyama(x, y, w, estimate_scale=scale)
		assert status == 0 and abs(np.linalg.det(R) - 1) < 1e-12


def test_reference_fit_refuses_degenerate_pairs():
	x = _cloud(10, 2).astype(np.float64)
	for xs, ys, w in ((x[:2], x[:2], None), (x, x, np.array([1., 1.] + [0.] * 8)), (np.outer(np.arange(10.), [1, 2, 3]), x, None), (x * 0 + 1, x, None)):
		R, t, s, status = ref.umeyama(xs, ys, w, estimate_scale=True)
		assert status == ref.DEGENERATE and np.array_equal(R, np.eye(3)) and not t.any() and s == 1


def test_reference_icp_recovers_a_shuffled_copy():
	rng = np.random.default_rng(5)
	x = _cloud(257, 4)
	R0, t0 = ref.rotation(rng.normal(size=3), math.radians(12)), np.array([0.020, -0.010, 0.015])
	y = ref.apply(x.astype(np.float64), R0, t0, 1.)[rng.permutation(257)].astype(np.float32)
	out = ref.icp(x, y, max_iterations=30)
	assert out['status'] == 0 and out['iterations'] < 30 and out['rmse'] < 1e-7
	assert ref.rotation_error(out['R'], R0) < 1e-6 and np.abs(out['t'] - t0).max() < 1e-7
	# the returned match belongs to the returned transform
	d2, idx = ref.nearest(ref.apply(x.astype(np.float64), out['R'], out['t'], out['s']), y.astype(np.float64))
	assert np.array_equal(idx, out['idx']) and np.array_equal(d2, out['d2'])


def test_reference_trim_rule():
	d2 = np.array([4., 1., 1., 9., 0., 1.], dtype=np.float32)
	assert ref.trim_rule(d2)[0] == np.inf and ref.trim_rule(d2)[1].all()
	tau, used = ref.trim_rule(d2, trim=0.5)            # k = 3: the ties at 1 all count
	assert tau == 1 and used.tolist() == [False, True, True, False, True, True]
	tau, used = ref.trim_rule(d2, trim=0.9)            # k = 6 - 5 = 1
	assert tau == 0 and used.sum() == 1
	tau, used = ref.trim_rule(d2, trim=0.1)            # floor(0.6) = 0: k = m
	assert tau == 9 and used.all()
	assert ref.trim_rule(d2, trim=0.1, max_dist=1.5)[1].tolist() == [False, True, True, False, True, True]


# ------------------------------------------------------------------ registration rows
def test_reg_round_trip_through_the_oracle():
	sys.path.insert(0, ROOT)
	from oracle.mlp_ref import euler_angles_to_matrix_xyz, registration
	from find_amd.align import SimilarityTransform, reg_from_transform, transform_from_reg
	g = torch.Generator().manual_seed(11)
	e = (torch.rand(64, 3, generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor([3.1, 1.5, 3.1], dtype=torch.float64)
	T = torch.randn(64, 3, generator=g, dtype=torch.float64)
	s = torch.rand(64, generator=g, dtype=torch.float64) + 0.5
	R = euler_angles_to_matrix_xyz(e)
	reg = reg_from_transform(SimilarityTransform(R, T, s))
	assert reg.shape == (64, 9) and torch.allclose(reg[:, 3:6], e, rtol=0, atol=1e-12) and torch.equal(reg[:, :3], T)
	assert torch.equal(reg[:, 6:], s[:, None].expand(-1, 3))
	back = transform_from_reg(reg)
	assert torch.allclose(back.R, R, rtol=0, atol=1e-14) and torch.equal(back.T, T) and torch.equal(back.s, s)
	# the row means what the model's registration makes of it
	pts = torch.randn(64, 9, 3, generator=g, dtype=torch.float64)
	assert torch.allclose(registration(pts, torch.zeros_like(pts), reg), back.apply(pts), rtol=0, atol=1e-13)
	# gimbal lock: |e1| = pi/2 has no row
	for e1 in (math.pi / 2, -math.pi / 2):
		for dtype in (torch.float32, torch.float64):
			lock = euler_angles_to_matrix_xyz(torch.tensor([[0.3, e1, -0.2]], dtype=dtype))
			with pytest.raises(ValueError, match='pi/2'):
				reg_from_transform(SimilarityTransform(lock, torch.zeros(1, 3, dtype=dtype), torch.ones(1, dtype=dtype)))
	with pytest.raises(ValueError, match='anisotropic'):
		transform_from_reg(torch.tensor([[0., 0, 0, 0, 0, 0, 1, 1, 1.01]]))
	with pytest.raises(ValueError, match=r'\(N, 9\)'):
		transform_from_reg(torch.zeros(3, 8))


# ------------------------------------------------------------------ interface
def test_header_and_bindings_declare_the_symbols():
	from find_amd import _lib, align
	hdr = open(os.path.join(ROOT, 'include', 'find_hip.h')).read()
	for name in SYMBOLS:
		assert re.search(r'\bint ' + name + r'\(', hdr), name
		assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name), name
	for name in ('find_align_ws_bytes', 'find_icp_ws_bytes'):
		assert re.search(r'\bint64_t ' + name + r'\(', hdr) and name in _lib.PROTOTYPES
	# the declared parameters, counted from the header
	for name, n_args in zip(SYMBOLS, (15, 29)):
		decl = re.search(r'\bint ' + name + r'\(([^;]*)\);', hdr).group(1)
		assert len(decl.split(',')) == n_args == len(_lib.PROTOTYPES[name][1]), name
	assert f'#define FIND_ALIGN_MAX_ITERATIONS {align.STATUS_MAX_ITERATIONS}' in hdr and f'#define FIND_ALIGN_DEGENERATE {align.STATUS_DEGENERATE}' in hdr
	assert (align.STATUS_MAX_ITERATIONS, align.STATUS_DEGENERATE) == (ref.MAX_ITERATIONS, ref.DEGENERATE)
	assert os.path.exists(os.path.join(ROOT, 'find_amd', 'csrc', 'align.hip'))
	# the wave and launch rules the header promises
	assert 'no float atomics' in hdr and 'wasted but harmless' in hdr and '|mu - pivot|^2 / sigma^2 * 2^-53' in hdr


def test_ws_bytes_and_refusals():
	from find_amd import _lib
	L = _lib.lib()
	# 19 doubles per workgroup of 256 pairs and cloud; ICP: also a double and an int32 per cloud, each array rounded up to 256 bytes
	assert L.find_align_ws_bytes(1, 4) == 256 and L.find_align_ws_bytes(3, 1000) == 2048
	assert L.find_icp_ws_bytes(1, 256, 7) == 256 + 512 and L.find_icp_ws_bytes(16, 5000, 5000) == 16 * 20 * 19 * 8 + 2 * 256
	for bad in ((0, 10), (1, 0), (65536, 10), (1, 1 << 24), (60000, 60000)):
		L.find_image_mse_ws_bytes()
		assert L.find_align_ws_bytes(*bad) == -1 and b'bad sizes' in L.find_last_error() and b'find_align_ws_bytes' in L.find_last_error(), bad
		assert L.find_icp_ws_bytes(*bad, 5) == -1 and L.find_icp_ws_bytes(1, 5, bad[1] if bad[0] == 1 else 0) == -1
	# NULL arguments and bad numbers are refused before any launch
	assert L.find_align_fit(None, None, None, None, 1, 4, 0, 0, None, None, None, None, None, 0, None) != 0 and b'NULL' in L.find_last_error()
	one = torch.zeros(64)
	p = one.data_ptr()   # (host memory: nothing may touch it)
	for kw in (dict(trim=1.0), dict(trim=-0.1), dict(max_dist=0.), dict(rel_tol=-1.), dict(iters=-1), dict(iters=10001)):
		rc = L.find_icp_run(p, None, p, None, 1, 4, 4, None, None, None, kw.get('iters', 5), kw.get('rel_tol', 1e-6), 0, kw.get('trim', 0.), kw.get('max_dist', math.inf),
							p, p, p, p, p, p, p, p, p, p, p, p, 1 << 20, None)
		assert rc != 0 and b'find_icp_run' in L.find_last_error(), kw
	assert L.find_icp_run(p, None, p, None, 1, 4, 4, p, None, None, 5, 1e-6, 0, 0., math.inf, p, p, p, p, p, p, p, p, p, p, p, p, 1 << 20, None) != 0
	assert b'all three or none' in L.find_last_error()
	assert L.find_icp_run(p, None, p, None, 1, 4, 4, None, None, None, 5, 1e-6, 0, 0., math.inf, p, p, p, p, p, p, p, p, p, p, p, p, 8, None) != 0
	assert b'workspace' in L.find_last_error()


def test_host_build_of_the_solve():
	"""csrc/align_math.h -- the Jacobi SVD, the Umeyama solve and the radix select's digit step, the functions align.hip compiles for the
	device -- built for the host and run by tools/align_host_check.cpp: random, rank-deficient, tiny and huge matrices against U D V^T,
	known transforms (weights, reflections, clouds 1e4 from the origin), degenerate pairs, the select against a sort with ties."""
	cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'), '/opt/rocm/llvm/bin/clang++') if c and os.path.exists(c)), None)
	assert cxx is not None, 'no host C++ compiler'
	import tempfile
	with tempfile.TemporaryDirectory() as tmp:
		exe = os.path.join(tmp, 'align_host_check')
		subprocess.run([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'find_amd', 'csrc'), os.path.join(ROOT, 'tools', 'align_host_check.cpp'), '-o', exe],
					   check=True, capture_output=True)
		r = subprocess.run([exe], capture_output=True, text=True)
	assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:]


# ------------------------------------------------------------------ the wrappers before any launch
def test_wrappers_refuse_bad_arguments():
	from find_amd import align
	x, y = torch.zeros(2, 10, 3), torch.zeros(2, 12, 3)
	for bad in (dict(X=torch.zeros(10, 3)), dict(X=torch.zeros(2, 10, 2)), dict(X=torch.zeros(3, 10, 3)), dict(X=torch.zeros(2, 10, 3, dtype=torch.int32)),
				dict(trim=1.0), dict(trim=-0.5), dict(x_len=torch.zeros(3, dtype=torch.int32)), dict(y_len=torch.zeros(2)), dict(max_iterations=-1),
				dict(relative_rmse_thr=-1.), dict(max_distance=0.), dict(init_transform=(torch.eye(3), torch.zeros(3), torch.ones(1))),
				dict(init_transform=align.SimilarityTransform(torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.ones(3)))):
		kw = dict(X=x, Y=y)
		kw.update(bad)
		with pytest.raises(ValueError, match='iterative_closest_point'):
			align.iterative_closest_point(**kw)
	for bad in (dict(Y=y), dict(weights=torch.ones(2, 9)), dict(weights=torch.ones(2, 10, dtype=torch.int32)), dict(lengths=torch.zeros(2)), dict(X=torch.zeros(10, 3))):
		kw = dict(X=x, Y=torch.zeros(2, 10, 3))
		kw.update(bad)
		with pytest.raises(ValueError, match='corresponding_points_alignment'):
			align.corresponding_points_alignment(**kw)
	# CPU tensors: the module's usual GPU error, before the library is asked for anything
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		align.iterative_closest_point(x, y)
	with pytest.raises(RuntimeError, match='no CPU fallback'):
		align.corresponding_points_alignment(x, x)
	for fn in (align.corresponding_points_alignment, align.iterative_closest_point):
		assert 'Not differentiable' in fn.__doc__
	assert align.ICPSolution._fields[:8] == ('converged', 'rmse', 'Xt', 'RTs', 'iterations', 'status', 'idx', 'dist')
	assert align.SimilarityTransform._fields == ('R', 'T', 's')


def test_eval_keywords_are_checked():
	from find_amd import eval_metrics, evaluate
	with pytest.raises(ValueError, match="'rigid' or 'similarity'"):
		eval_metrics.eval_3d_metrics(None, None, align='affine')
	with pytest.raises(ValueError, match="'rigid' or 'similarity'"):
		evaluate.eval_3d(None, None, None, align=True)
